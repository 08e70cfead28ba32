"""The settle rule of RANSAC.run against the model it relies on, on CPU, on synthetic hypothesis tables: the rule
(ransac_with_homography_amd/csrc/rwh_settle.h) through the library's host-only export rwh_settle_decide, driven through ctypes, and
through ransac._settle_on_host -- the Python plumbing around the same export (`pre`, slots, masks, the H rows returned) -- with the host
solver, the scorer and the interval kernel replaced by table lookups.

Every table lists, per hypothesis, K1's flags, K2's raw count, a count interval [lo, hi] (what rwh_score_interval would return) and the
reference's TRUE count.  In-model tables obey the model stated in rwh_settle.h (and include/rwh.h):
  * no always-bit (RWH_HYP_REPEATED / SINGULAR / DEGENERATE): lo <= true <= hi and lo <= raw <= hi;
  * unflagged: |true - raw| <= IV_NEAR / 2;
  * RWH_HYP_ILLCOND: true is bounded by the interval only;
  * always-bit rows: anything.
The oracle is the reference's accept rules (ransac.py:186-202) on the true counts of all k hypotheses.  For the margin rule
('backward' / 'reproj', margin cap 0 or 8) the model is |true - raw| <= min(3, cap) for unflagged rows.  Out-of-model tables
(containment broken on purpose) have no right answer; there the two paths must still agree."""
import ctypes

import numpy as np
import pytest
import torch

from ransac_with_homography_amd import _lib, kernels
from ransac_with_homography_amd import ransac as impl

REP, SING, ILL, DEG = 1, 2, 4, 8
NEAR = 32                                     # IV_NEAR of rwh_settle.h


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


class Table(object):
    def __init__(self, flags, raw, lo, hi, true, need, use_iv=True, cap=8, family=""):
        self.flags = np.asarray(flags, np.uint8)
        self.raw, self.lo, self.hi, self.true = (np.asarray(a, np.int64) for a in (raw, lo, hi, true))
        self.need, self.use_iv, self.cap, self.family = int(need), bool(use_iv), int(cap), family
        self.k = len(self.flags)

    def __repr__(self):
        return "Table(%s, need=%d, use_iv=%s, cap=%d, flags=%s, raw=%s, lo=%s, hi=%s, true=%s)" % (
            self.family, self.need, self.use_iv, self.cap, self.flags.tolist(), self.raw.tolist(), self.lo.tolist(), self.hi.tolist(),
            self.true.tolist())


def oracle(t):
    """ransac.py:186-202 on the true counts: the first hypothesis reaching `need` wins and stops; otherwise the first index of the
    maximum (strict >, from 0); no count above 0: no winner."""
    hit = np.flatnonzero(t.true >= t.need)
    if hit.size:
        return int(hit[0]), 1, int(t.true[hit[0]])
    w, best = -1, 0
    for i, c in enumerate(t.true.tolist()):
        if c > best:
            w, best = i, c
    return w, 0, best


def run_native(lib, t):
    """rwh_settle_decide on table t; like rwh_ransac_run, the RWH_HYP_REPEATED rows are settled first (through the same solve
    callback) and handed in as slots 0 .. n_rep-1."""
    asked_iv, settled = [], []

    def iv(rows, n, cscale, lo, hi, _):
        assert cscale == 1.0                  # pts_a is all zeros: the coordinate scale is its floor
        for j in range(n):
            r = rows[j]
            asked_iv.append(r)
            lo[r], hi[r] = int(t.lo[r]), int(t.hi[r])
        return 0

    def settle(rows, n, cnt, _):
        for j in range(n):
            r = rows[j]
            settled.append(r)
            cnt[r] = int(t.true[r])
        return 0

    out = np.zeros(5, np.int32)
    cnt = np.array(t.raw, np.int32)
    slot = np.full(t.k, -1, np.int32)
    rep = np.flatnonzero(t.flags & REP).astype(np.int32)
    if rep.size:
        i32p = ctypes.POINTER(ctypes.c_int32)
        assert settle(rep.ctypes.data_as(i32p), rep.size, cnt.ctypes.data_as(i32p), None) == 0
        slot[rep] = np.arange(rep.size)
    pa = np.zeros((1, 2), np.float32)
    st = lib.rwh_settle_decide(t.k, t.flags.ctypes.data, cnt.ctypes.data, slot.ctypes.data, pa.ctypes.data, 1, t.need, int(t.use_iv),
                               t.cap, _lib.SETTLE_INTERVAL_FN(iv), _lib.SETTLE_SOLVE_FN(settle), None, out.ctypes.data)
    assert st == 0
    assert len(settled) == len(set(settled)), ("a hypothesis settled twice", t)
    assert set(np.flatnonzero(slot >= 0).tolist()) == set(settled)
    assert sorted(slot[slot >= 0].tolist()) == list(range(len(settled)))
    assert all(cnt[r] == t.true[r] for r in settled)
    return dict(res=(int(out[0]), int(out[1]), int(out[2])), settled=set(settled), asked_iv=set(asked_iv))


class Twin(object):
    """ransac._settle_on_host with the GPU / LAPACK work looked up in the current table: H rows and mask rows carry their hypothesis
    index."""

    def __init__(self, monkeypatch):
        self.t = None
        monkeypatch.setattr(impl, "svd_hypotheses", self._svd)
        monkeypatch.setattr(impl, "_score_settled", self._score)
        monkeypatch.setattr(kernels, "score_interval", self._interval)

    def _svd(self, pa, pb, idx_rows, threads=None):
        r = np.asarray(idx_rows).reshape(-1, 4)[:, 0]
        H = np.zeros((len(r), 9), np.float32)
        H[:, 0] = r
        return H

    def _score(self, H, pa_dev, pb_dev, th, method):
        r = H[:, 0].astype(np.int64)
        self.settled.extend(r.tolist())
        return torch.from_numpy(self.t.true[r].astype(np.int32)), torch.from_numpy(r[:, None].copy())

    def _interval(self, H, rows, flags, pa, pb, th, cscale, d0, d1):
        assert cscale == 1.0                  # pts_a is all zeros: the coordinate scale the library computed is its floor
        rows = np.asarray(rows, np.int64)
        self.asked_iv.extend(rows.tolist())
        return self.t.lo[rows].copy(), self.t.hi[rows].copy()

    def run(self, t):
        self.t, self.settled, self.asked_iv = t, [], []
        idx = np.repeat(np.arange(t.k, dtype=np.int32)[:, None], 4, axis=1)
        pa = np.zeros((1, 2), np.float32)
        method = "fwd" if t.use_iv else "backward"
        pre = impl.presettle(None, None, pa, pa, idx, np.flatnonzero(t.flags & REP), 1.0, method)
        w, early, cnt, words, rows, counts = impl._settle_on_host(
            None, None, pa, pa, idx, t.raw.astype(np.int32), t.flags, t.need, 1.0, method, t.cap, {}, pre=pre,
            H_dev=torch.zeros(1) if t.use_iv else None, flags_dev=torch.from_numpy(t.flags) if t.use_iv else None)
        assert len(self.settled) == len(set(self.settled)), ("a hypothesis settled twice", t)
        assert set(rows) == set(self.settled) and all(int(h[0]) == i for i, h in rows.items())
        want = t.raw.copy()
        want[sorted(self.settled)] = t.true[sorted(self.settled)]
        assert counts.dtype == np.int64 and np.array_equal(counts, want)
        assert words is None or (w is not None and int(words[0]) == w)
        return dict(res=(-1 if w is None else w, int(early), int(cnt)), settled=set(self.settled), asked_iv=set(self.asked_iv),
                    mask_settled=words is not None)


# ---- generators ---------------------------------------------------------------------------------------------------------------
def _always_flag(rng):
    return int(rng.choice([REP, SING, DEG | ILL, REP | ILL]))


def fwd_row(rng, kind, raw, true=None, width=6, point=0.2):
    """One in-model row: (flags, raw, lo, hi, true).  kind 'u' unflagged, 'i' RWH_HYP_ILLCOND, 'a' an always-bit."""
    raw = max(int(raw), 0)
    if kind == "a":
        t = int(rng.integers(0, 300)) if true is None else int(true)
        return _always_flag(rng), raw, raw, raw, t
    if true is None:
        if kind == "u":
            true = raw + int(rng.integers(-NEAR // 2, NEAR // 2 + 1))
        else:
            true = int(rng.integers(0, raw + 80))
    t = max(int(true), 0)
    if kind == "u":
        assert abs(t - raw) <= NEAR // 2
    if t == raw and rng.random() < point:
        return (0 if kind == "u" else ILL), raw, raw, raw, t
    lo = max(min(raw, t) - int(rng.integers(0, width + 1)), 0)
    hi = max(raw, t) + int(rng.integers(0, width + 1))
    return (0 if kind == "u" else ILL), raw, lo, hi, t


def table_from_rows(rows, need, family, use_iv=True, cap=8):
    f, r, lo, hi, t = zip(*rows) if rows else ((), (), (), (), ())
    return Table(f, r, lo, hi, t, need, use_iv, cap, family)


def gen_random(rng):
    k = int(rng.choice([1, 2, 3, 5, 12, 40, 120]))
    top = int(rng.integers(0, 250))
    need = int(rng.choice([top // 2 + 1, top + 1, top + 40, 10 ** 6, max(top - 5, 1)]))
    p = rng.dirichlet([4, 1.5, 1])
    rows = []
    for _ in range(k):
        kind = rng.choice(["u", "i", "a"], p=p)
        raw = top - int(rng.integers(0, 60)) if rng.random() < 0.6 else int(rng.integers(0, top + 1))
        rows.append(fwd_row(rng, kind, raw, width=int(rng.integers(0, 40)), point=0.3))
    return table_from_rows(rows, need, "random")


def gen_illcond_above(rng):
    """an RWH_HYP_ILLCOND row far above the best unflagged row that collapses when settled; the unflagged rows near the
    top disagree with their raw order by a few counts."""
    X = int(rng.integers(40, 200))
    k = int(rng.integers(4, 30))
    rows = [fwd_row(rng, "u", X - int(rng.integers(0, 4)), width=int(rng.integers(0, 3)), point=0.4) for _ in range(k)]
    # two near-tie rows, the earlier one below in raw counts and level or above in true counts
    a, b = sorted(rng.choice(k, 2, replace=False).tolist())
    rows[a] = fwd_row(rng, "u", X - 1, true=X + int(rng.integers(0, 3)), width=1)
    rows[b] = fwd_row(rng, "u", X, true=X, point=1.0)
    raw_i = X + NEAR + 1 + int(rng.integers(0, 200))
    true_i = int(rng.integers(0, X // 2))
    pos = int(rng.integers(0, k + 1))
    rows.insert(pos, (ILL, raw_i, true_i, raw_i, true_i))
    for _ in range(int(rng.integers(0, 20))):
        rows.insert(int(rng.integers(0, len(rows) + 1)), fwd_row(rng, "u", int(rng.integers(0, max(X - NEAR, 1)))))
    return table_from_rows(rows, int(rng.choice([10 ** 6, raw_i + 1, X + 17])), "illcond_above")


def gen_wide_top(rng):
    """the top row has a wide interval and settles low; runners-up sit just outside the 32-count window."""
    T = int(rng.integers(50, 300))
    k = int(rng.integers(3, 25))
    rows = []
    for _ in range(k):
        c = T - NEAR - 1 - int(rng.integers(0, NEAR // 2))
        rows.append(fwd_row(rng, "u", c, true=c + int(rng.integers(0, NEAR // 2 + 1)), width=int(rng.integers(0, 4))))
    top = ("u", T, T - NEAR // 2) if rng.random() < 0.5 else ("i", T, int(rng.integers(0, T)))
    rows.insert(int(rng.integers(0, k + 1)), fwd_row(rng, top[0], top[1], true=top[2], width=int(rng.integers(0, 60))))
    return table_from_rows(rows, int(rng.choice([10 ** 6, T + 1])), "wide_top")


def gen_ties(rng):
    """Several hypotheses share the maximum true count: the first index must win, whatever the raw counts and intervals say."""
    T = int(rng.integers(5, 200))
    k = int(rng.integers(2, 30))
    rows = []
    for _ in range(k):
        kind = rng.choice(["u", "i", "a"], p=[0.6, 0.25, 0.15])
        if rng.random() < 0.4:
            raw = T + int(rng.integers(-NEAR // 2, NEAR // 2 + 1)) if kind == "u" else int(rng.integers(0, T + 40))
            rows.append(fwd_row(rng, kind, raw, true=T, width=int(rng.integers(0, 8)), point=0.5))
        else:
            raw = T - int(rng.integers(0, 40))
            row = fwd_row(rng, kind, raw, width=int(rng.integers(0, 8)))
            if row[4] >= T:
                row = fwd_row(rng, kind, raw, true=min(T - 1, raw + 16) if kind == "u" else T - 1, width=2)
            rows.append(row)
    return table_from_rows(rows, 10 ** 6, "ties")


def gen_need_edges(rng):
    """Counts at need - 1, need and need + 1; intervals that straddle `need`."""
    need = int(rng.integers(1, 200))
    k = int(rng.integers(1, 25))
    rows = []
    for _ in range(k):
        kind = rng.choice(["u", "i", "a"], p=[0.6, 0.25, 0.15])
        t = need + int(rng.choice([-1, 0, 1, -1, -2, -20]))
        raw = t + (int(rng.integers(-3, 4)) if kind == "u" else int(rng.integers(-30, 31)))
        if kind == "u":
            raw = min(max(raw, t - 16), t + 16)
        rows.append(fwd_row(rng, kind, max(raw, 0), true=max(t, 0), width=int(rng.choice([0, 1, 2, 5])), point=0.3))
    return table_from_rows(rows, need, "need_edges")


def gen_edges(rng):
    """All rows flagged; all counts 0; k = 1."""
    which = int(rng.integers(0, 3))
    if which == 0:
        k = int(rng.integers(1, 12))
        rows = [fwd_row(rng, rng.choice(["i", "a"]), int(rng.integers(0, 100))) for _ in range(k)]
    elif which == 1:
        k = int(rng.integers(1, 12))
        rows = [fwd_row(rng, rng.choice(["u", "i", "a"]), 0, true=0) for _ in range(k)]
    else:
        rows = [fwd_row(rng, rng.choice(["u", "i", "a"]), int(rng.integers(0, 50)))]
    return table_from_rows(rows, int(rng.choice([1, 10, 10 ** 6])), "edges")


def gen_early(rng):
    """The early-exit row first, in the middle or last; the others below `need`, some with intervals reaching it."""
    need = int(rng.integers(10, 200))
    k = int(rng.integers(1, 30))
    rows = []
    for _ in range(k):
        kind = rng.choice(["u", "i", "a"], p=[0.6, 0.25, 0.15])
        t = need - 1 - int(rng.integers(0, 30))
        if kind == "a":
            rows.append(fwd_row(rng, "a", int(rng.integers(0, 2 * need)), true=t))
            continue
        raw = t + int(rng.integers(-16, 17)) if kind == "u" else int(rng.integers(0, 2 * need))
        rows.append(fwd_row(rng, kind, raw, true=max(t, 0), width=int(rng.integers(0, 10))))
    e = [0, k // 2, k][int(rng.integers(0, 3))]
    kind = rng.choice(["u", "i", "a"], p=[0.6, 0.25, 0.15])
    t = need + int(rng.integers(0, 5))
    raw = t + int(rng.integers(-16, 17)) if kind == "u" else int(rng.integers(0, 2 * need))
    rows.insert(e, fwd_row(rng, kind, raw, true=t, width=int(rng.integers(0, 10))))
    return table_from_rows(rows, need, "early")


def gen_margin(rng, cap):
    """'backward' / 'reproj': the margin rule.  Unflagged rows within min(3, cap) of their true count; flagged rows anything."""
    e = min(3, cap)
    k = int(rng.choice([1, 3, 10, 40]))
    top = int(rng.integers(0, 200))
    need = int(rng.choice([top + 1, top // 2 + 1, 10 ** 6]))
    rows = []
    for _ in range(k):
        t = top - int(rng.integers(0, 20)) if rng.random() < 0.7 else int(rng.integers(0, top + 1))
        if rng.random() < 0.7:
            raw = max(t + int(rng.integers(-e, e + 1)), 0)
            rows.append((0, raw, raw, raw, t))
        else:
            raw = int(rng.integers(0, top + 60))
            rows.append((int(rng.choice([REP, SING, ILL, DEG | ILL])), raw, raw, raw, t))
    return table_from_rows(rows, need, "margin_cap%d" % cap, use_iv=False, cap=cap)


def break_model(rng, t):
    """The same table with containment broken on some rows: true counts outside [lo, hi], unflagged rows far from their raw count,
    raw counts outside the interval."""
    true, lo, hi, raw = t.true.copy(), t.lo.copy(), t.hi.copy(), t.raw.copy()
    for i in range(t.k):
        u = rng.random()
        if u < 0.25:
            true[i] = max(lo[i] - int(rng.integers(1, 60)), 0)
        elif u < 0.4:
            true[i] = hi[i] + int(rng.integers(1, 60))
        elif u < 0.5:
            raw[i] = hi[i] + int(rng.integers(1, 60))
    return Table(t.flags, raw, lo, hi, true, t.need, t.use_iv, t.cap, t.family + "+broken")


FWD_FAMILIES = [(gen_random, 900), (gen_illcond_above, 400), (gen_wide_top, 300), (gen_ties, 300), (gen_need_edges, 300),
                (gen_edges, 120), (gen_early, 300)]


def _tables(seed):
    rng = np.random.default_rng(seed)
    for gen, n in FWD_FAMILIES:
        for _ in range(n):
            yield gen(rng)
    for cap in (0, 8):
        for _ in range(300):
            yield gen_margin(rng, cap)


def _check_in_model(t, nat, twin):
    want = oracle(t)
    assert nat["res"] == want, ("native", nat["res"], want, t)
    assert twin["res"] == want, ("twin", twin["res"], want, t)
    assert nat["settled"] == twin["settled"], (sorted(nat["settled"] ^ twin["settled"]), t)
    w = want[0]
    if w >= 0:
        if t.use_iv:
            # the winner was settled, or its interval is a point: then K2's count and mask on K1's H are the reference's
            assert w in nat["settled"] or (w in nat["asked_iv"] and t.lo[w] == t.hi[w]), ("winner neither settled nor exact", t)
        else:
            assert w in nat["settled"], ("margin rule: winner not settled", t)
        assert twin["mask_settled"] == (w in twin["settled"])


def test_settle_rule_model_native_and_twin(lib, monkeypatch):
    """Every in-model table: the export and _settle_on_host each return the oracle's (winner, early, count), settle the same rows,
    and the winner is settled unless its interval is a point."""
    twin = Twin(monkeypatch)
    seen = {}
    for t in _tables(20261016):
        nat, tw = run_native(lib, t), twin.run(t)
        _check_in_model(t, nat, tw)
        seen[t.family] = seen.get(t.family, 0) + 1
    assert sum(seen.values()) >= 3000, seen


def test_settle_rule_out_of_model_drivers_agree(lib, monkeypatch):
    """Containment broken on purpose: there is no right answer, but the export and _settle_on_host must take the same
    decision and settle the same rows (ADVICE finding 3: a row that seeded the first sure exit settling below `need`)."""
    twin = Twin(monkeypatch)
    rng = np.random.default_rng(7)
    n = 0
    for t in _tables(99):
        b = break_model(rng, t)
        nat, tw = run_native(lib, b), twin.run(b)
        assert nat["res"] == tw["res"], (nat["res"], tw["res"], b)
        assert nat["settled"] == tw["settled"], (sorted(nat["settled"] ^ tw["settled"]), b)
        n += 1
    # the targeted case: the first sure row (lo >= need) settles below need; the next sure row decides the prefix
    need = 50
    b = Table([0, 0, 0, 0], [10, 60, 40, 55], [10, 50, 30, 55], [10, 70, 49, 55], [10, 20, 45, 55], need, family="fs_lost")
    nat, tw = run_native(lib, b), twin.run(b)
    assert nat["res"] == tw["res"] == (3, 1, 55), (nat, tw)
    assert nat["settled"] == tw["settled"]


@pytest.mark.parametrize("where, exc", [("solve", np.linalg.LinAlgError("SVD did not converge")),
                                        ("interval", RuntimeError("rwh_score_interval failed"))])
def test_settle_callback_exception_propagates(lib, monkeypatch, where, exc):
    """An exception raised by the work _settle_on_host does for the rule -- numpy's LinAlgError from the host solver (why RANSAC.run
    falls back to this path), a kernel or torch error -- leaves _settle_on_host as that same exception, not as a library error; the
    library returns the status of the callback that caught it."""
    twin = Twin(monkeypatch)

    def boom(*a, **kw):
        raise exc
    monkeypatch.setattr(impl, "svd_hypotheses", boom) if where == "solve" else monkeypatch.setattr(kernels, "score_interval", boom)
    real, returned = lib.rwh_settle_decide, []

    def spy(*a):
        returned.append(real(*a))
        return returned[-1]
    monkeypatch.setattr(lib, "rwh_settle_decide", spy)
    # 'fwd': all three rows get an interval, then rows 1 and 2 (open intervals reaching the best lower bound) are settled
    t = Table([0, ILL, 0], [40, 90, 38], [40, 0, 36], [40, 95, 41], [40, 10, 39], 10 ** 6, family="raises")
    with pytest.raises(type(exc)) as e:
        twin.run(t)
    assert e.value is exc and returned == [1]


def test_settle_callback_status_is_returned(lib):
    """A nonzero status from either callback ends rwh_settle_decide with that status, the state as far as the rule got."""
    pa = np.zeros((1, 2), np.float32)
    flags = np.array([0, ILL, 0], np.uint8)
    for iv_status, solve_status, rounds in ((7, 0, 0), (0, -3, 1)):
        def iv(rows, n, cscale, lo, hi, _):
            for j in range(n):
                lo[rows[j]], hi[rows[j]] = ((40, 40), (0, 95), (36, 41))[rows[j]]
            return iv_status
        cnt, slot, out = np.array([40, 90, 38], np.int32), np.full(3, -1, np.int32), np.zeros(5, np.int32)
        st = lib.rwh_settle_decide(3, flags.ctypes.data, cnt.ctypes.data, slot.ctypes.data, pa.ctypes.data, 1, 10 ** 6, 1, 8,
                                   _lib.SETTLE_INTERVAL_FN(iv), _lib.SETTLE_SOLVE_FN(lambda rows, n, c, _: solve_status), None,
                                   out.ctypes.data)
        assert st == (iv_status or solve_status)
        assert out.tolist() == [-1, 0, 0, rounds, 3] and cnt.tolist() == [40, 90, 38] and slot.tolist() == [-1, -1, -1]
