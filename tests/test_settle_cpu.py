"""Host logic of the solver-parity step (ransac_with_homography_amd/ransac.py: svd_hypotheses, _settle_on_host) on CPU.

The GPU scorer is replaced by the oracle (the checker) and K1 / K2's device results are EMULATED from the reference's
per-iteration table in tests/golden/g9_low_inlier.npz (written by the unmodified reference, make_golden.py g9): flagged
(repeated-index) samples get count 0 like K1's NaN rows give, and a few unflagged counts are nudged inside the margin.
The accept rules must then return the reference's winner -- a repeated-index sample on every g9 case."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import rwh_oracle as orc
from ransac_with_homography_amd import kernels
from ransac_with_homography_amd import ransac as impl


@pytest.fixture(scope="module", autouse=True)
def lib():
    """_settle_on_host takes its rule from the library (rwh_settle_decide, host code: no GPU needed)."""
    import __graft_entry__ as g
    g.build()


@pytest.fixture
def oracle_scorer(monkeypatch):
    def score_count(H, pa, pb, th, loss, need, best, **kw):
        X, Y = pa.numpy().T, pb.numpy().T
        K, M = H.shape[0], X.shape[1]
        counts = np.zeros(K, np.int32)
        masks = np.zeros((K, (M + 63) // 64), np.uint64)
        with np.errstate(all="ignore"):
            for i in range(K):
                inl = orc.compute_loss(H[i].numpy().reshape(3, 3), X, Y, loss) < th
                counts[i] = inl.sum()
                bits = np.zeros(masks.shape[1] * 64, np.uint8)
                bits[:M] = inl
                masks[i] = np.packbits(bits, bitorder="little").view(np.uint64)
        return torch.from_numpy(counts), torch.from_numpy(masks.view(np.int64)), None
    monkeypatch.setattr(kernels, "score_count", score_count)
    monkeypatch.setattr(kernels, "new_best", lambda dev: None)


def test_svd_hypotheses_is_the_reference_solver(matches):
    """Stacked host SVD == the reference's per-sample calcHomography, bit for bit, degenerate samples included."""
    z = load_golden("g9_low_inlier")
    ptsA, _ = matches
    for key in [str(c) for c in z["cases"]]:
        B = z["ptsB_" + key[0]]
        got = impl.svd_hypotheses(ptsA, B, z[key + "_idx"])
        ref = z[key + "_hyp_H"]
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), key
    g = load_golden("g2_hyp_seed0")
    got = impl.svd_hypotheses(ptsA, matches[1], g["idx"][:2000])
    assert np.array_equal(got.view(np.uint32), g["H"][:2000].view(np.uint32))


def test_oracle_reproduces_low_inlier_runs(matches):
    z = load_golden("g9_low_inlier")
    ptsA, _ = matches
    for key in [str(c) for c in z["cases"]]:
        tag, s, th, d, k, m = key.split("_")
        B = z["ptsB_" + tag]
        np.random.seed(int(s[1:]))
        with np.errstate(all="ignore"):
            H, inl, cnt, it = orc.ransac_run(ptsA.T, B.T, th=int(th[2:]), d=int(d[1:]), n=4, k=int(k[1:]), method=m)
        assert int(cnt) == int(z[key + "_count"]) and it == int(z[key + "_winner"])
        assert np.array_equal(inl[0], z[key + "_inliers"])
        assert len(set(z[key + "_idx"][it].tolist())) < 4          # the reference's winner repeats an index


@pytest.mark.parametrize("margin", [0, 8])
def test_settle_returns_reference_winner(matches, oracle_scorer, margin):
    z = load_golden("g9_low_inlier")
    ptsA, _ = matches
    rng = np.random.default_rng(3)
    for key in [str(c) for c in z["cases"]]:
        tag, s, th, d, k, m = key.split("_")
        B = z["ptsB_" + tag]
        idx = z[key + "_idx"]
        ref_counts = z[key + "_hyp_counts"].astype(np.int32)
        flags = np.array([len(set(r)) < 4 for r in idx.tolist()], np.uint8)
        dev_counts = np.where(flags != 0, 0, ref_counts).astype(np.int32)    # what K1 (NaN rows) + K2 report
        if margin:   # K1 round-off on ill-conditioned samples: counts off by up to 2 on a few unflagged hypotheses
            pick = rng.choice(np.flatnonzero(flags == 0), 30, replace=False)
            dev_counts[pick] = np.maximum(dev_counts[pick] + rng.integers(-2, 3, 30), 0)
        need = kernels.need_count(185, int(d[1:]), 4)
        stats = {}
        w, early, cnt, words, rows, counts = impl._settle_on_host(
            torch.from_numpy(ptsA), torch.from_numpy(B), ptsA, B, idx, dev_counts, flags, need, float(th[2:]), m, margin, stats)
        assert (w, cnt, early) == (int(z[key + "_winner"]), int(z[key + "_count"]), bool(z[key + "_early"])), key
        bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:185]
        assert np.array_equal(np.nonzero(bits)[0], z[key + "_inliers"])
        assert np.array_equal(rows[w].view(np.uint32), z[key + "_hyp_H"][w].view(np.uint32))
        end = w + 1 if early else len(idx)
        assert stats["host_settled"] >= int(flags[:end].sum()) and stats["host_rounds"] <= 4
        assert np.array_equal(counts[:end][flags[:end] != 0], ref_counts[:end][flags[:end] != 0])


def test_settle_without_suspects_keeps_device_decision(matches, oracle_scorer):
    """Golden table G2 restricted to distinct samples: the settled winner is the table's own argmax (6354 / 121)."""
    g = load_golden("g2_hyp_seed0")
    ptsA, ptsB = matches
    lo, hi = 6000, 6600
    idx, c = g["idx"][lo:hi], g["counts_fwd"][lo:hi].astype(np.int32)
    flags = g["degenerate"][lo:hi].astype(np.uint8)
    w, early, cnt, words, rows, _ = impl._settle_on_host(torch.from_numpy(ptsA), torch.from_numpy(ptsB), ptsA, ptsB, idx,
                                                      np.where(flags != 0, 0, c), flags, 134, 5.0, "fwd", 8)
    assert (lo + w, cnt, early) == (int(g["winner"]), int(g["winner_count"]), False)
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:185]
    assert np.array_equal(np.nonzero(bits)[0], g["winner_inliers"])


def test_native_host_solver_is_numpy_svd(matches):
    """rwh_host_dlt4_svd (the settle step's native loop over numpy's own dgesdd) == the stacked numpy.linalg.svd path ==
    the reference's per-sample H (G2: 10 000 samples, 373 with a repeated index), bit for bit; 1 and many threads."""
    from ransac_with_homography_amd import _lapack
    from ransac_with_homography_amd.homography import _pair_rows
    ptsA, ptsB = matches
    g = load_golden("g2_hyp_seed0")
    if _lapack.dgesdd_address() is None:
        pytest.skip("numpy's LAPACK symbol not found: svd_hypotheses stays on numpy.linalg.svd")
    for threads in (1, 5):
        got = impl.svd_hypotheses(ptsA, ptsB, g["idx"], threads=threads)
        assert np.array_equal(got.view(np.uint32), g["H"].view(np.uint32))
    flat = g["idx"][:3000].reshape(-1)
    mats = _pair_rows(ptsA[flat], ptsB[flat], -1).reshape(-1, 8, 9)
    with np.errstate(all="ignore"):
        _, _, vt = np.linalg.svd(mats)
        ref = vt[:, -1, :] / vt[:, -1, 8:9]
    assert np.array_equal(impl.svd_hypotheses(ptsA, ptsB, g["idx"][:3000]).view(np.uint32), ref.astype(np.float32).view(np.uint32))
    # the single-call solver of the module surface takes the same host path (homography.py:71-88), degenerate samples included
    from ransac_with_homography_amd import homography as hg
    for i in list(np.flatnonzero(g["degenerate"])[:20]) + list(range(20)):
        H = hg.calcHomography(ptsA[g["idx"][i]], ptsB[g["idx"][i]])
        assert H.dtype == np.float32 and np.array_equal(H.reshape(9).view(np.uint32), g["H"][i].view(np.uint32))


def test_native_host_solver_survives_a_fork(matches):
    """The library's one piece of state is its pool of host worker threads.  A forked child has none of the parent's
    threads: it must get a pool of its own and return the same bits (not wait for workers that do not exist)."""
    import os
    from ransac_with_homography_amd import _lapack
    ptsA, ptsB = matches
    g = load_golden("g2_hyp_seed0")
    if _lapack.dgesdd_address() is None:
        pytest.skip("numpy's LAPACK symbol not found")
    want = g["H"][:4000].view(np.uint32)
    assert np.array_equal(impl.svd_hypotheses(ptsA, ptsB, g["idx"][:4000], threads=5).view(np.uint32), want)     # the pool now has workers
    pid = os.fork()
    if pid == 0:
        ok = False
        try:
            import signal
            signal.alarm(60)                                                  # a hang ends the child, and the test fails
            ok = np.array_equal(impl.svd_hypotheses(ptsA, ptsB, g["idx"][:4000], threads=5).view(np.uint32), want)
        finally:
            os._exit(0 if ok else 1)
    _, status = os.waitpid(pid, 0)
    assert os.WIFEXITED(status) and os.WEXITSTATUS(status) == 0, status


def test_illcond_flag_and_settle_on_lattice_problems(oracle_scorer):
    """Ill-conditioned samples WITHOUT a repeated index (three collinear source points, equal coordinates at different
    indices): K1's elimination returns a finite H that has nothing to do with LAPACK's (counts apart by hundreds).  With
    K1 emulated in float64 (tests/k1_emulation.py: same elimination, same flag thresholds) and the oracle as scorer, the
    settle step must return the reference's winner, count and inlier list on every case of g12 (written by the unmodified
    reference): lattice and cluster problems, with and without an early exit, ties at the top."""
    from k1_emulation import RWH_HYP_ILLCOND, RWH_HYP_REPEATED, dlt4
    z = load_golden("g12_illcond")
    for key in [str(c) for c in z["cases"]]:
        tag, s, th, d, k, m = key.split("_")
        A, B = z["ptsA_" + tag], z["ptsB_" + tag]
        idx = z[key + "_idx"]
        ref_counts = z[key + "_hyp_counts"].astype(np.int64)
        th_f = float(th[2:])
        H, flags = dlt4(A, B, idx)
        # what the GPU would report: K2 on K1's H (NaN rows count 0)
        dev_counts = np.zeros(len(idx), np.int32)
        X, Y = A.T, B.T
        with np.errstate(all="ignore"):
            for i in range(len(idx)):
                if np.isfinite(H[i]).all():
                    dev_counts[i] = int((orc.compute_loss(H[i].reshape(3, 3), X, Y, m) < th_f).sum())
        unflagged = flags == 0
        dif = np.abs(dev_counts.astype(np.int64) - ref_counts)
        assert dif[unflagged].max() <= impl.RESCORE_MARGIN, (key, dif[unflagged].max())      # the flag leaves only small differences
        assert dif[(flags & RWH_HYP_ILLCOND) != 0].max() > 20, key                            # ... and catches the big ones
        assert ((flags & RWH_HYP_REPEATED) != 0).sum() == sum(len(set(r)) < 4 for r in idx.tolist())
        need = kernels.need_count(A.shape[0], int(d[1:]), 4)
        stats = {}
        pre = impl.presettle(torch.from_numpy(A), torch.from_numpy(B), A, B, idx, np.flatnonzero(impl.repeated_rows(idx)), th_f, m)
        w, early, cnt, words, rows, counts = impl._settle_on_host(torch.from_numpy(A), torch.from_numpy(B), A, B, idx, dev_counts, flags,
                                                                  need, th_f, m, impl.RESCORE_MARGIN, stats, pre=pre)
        assert w == int(z[key + "_winner"]) and cnt == int(z[key + "_count"]) and early == bool(z[key + "_early"]), (key, w, cnt, early)
        if words is None:           # the winner was not settled: its mask is K2's own on K1's H
            inl = np.flatnonzero(orc.compute_loss(H[w].reshape(3, 3), X, Y, m) < th_f)
        else:
            inl = np.flatnonzero(np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:A.shape[0]])
        assert np.array_equal(inl, z[key + "_inliers"]), key
        assert stats["host_rounds"] <= 2, (key, stats)


def test_interval_settle_rule_on_lattice_problems(oracle_scorer, monkeypatch):
    """The 'fwd' settle rule of round 4 -- count INTERVALS (rwh_score_interval) decide which hypotheses get the reference's solver,
    not a flat margin -- on the lattice / cluster fixture g12, with K1 and the interval kernel emulated in numpy
    (tests/k1_emulation.py, tests/interval_emulation.py) and the oracle as scorer.  Per case: (1) CONTAINMENT, the property the
    rule stands on: the reference's own count of every hypothesis that is not repeated / non-finite / degenerate lies inside
    its interval; (2) the settle step returns the reference's winner, count, early-exit flag and inlier list; (3) it hands
    FEWER hypotheses to the host than the margin rule does."""
    import interval_emulation as ive
    from k1_emulation import RWH_HYP_DEGENERATE, RWH_HYP_REPEATED, RWH_HYP_SINGULAR, dlt4
    monkeypatch.setattr(kernels, "score_interval", lambda H, rows, flags, pa, pb, th, c, d0, d1: ive.score_interval(
        H.numpy(), rows, None if flags is None else flags.numpy(), pa.numpy(), pb.numpy(), th, c, d0, d1))
    z = load_golden("g12_illcond")
    for key in [str(c) for c in z["cases"]]:
        tag, s, th, d, k, m = key.split("_")
        if m != "fwd":
            continue
        A, B = z["ptsA_" + tag], z["ptsB_" + tag]
        idx = z[key + "_idx"]
        ref_counts = z[key + "_hyp_counts"].astype(np.int64)
        th_f = float(th[2:])
        H, flags = dlt4(A, B, idx)
        X, Y = A.T, B.T
        dev_counts = np.zeros(len(idx), np.int32)
        with np.errstate(all="ignore"):
            for i in range(len(idx)):
                if np.isfinite(H[i]).all():
                    dev_counts[i] = int((orc.compute_loss(H[i].reshape(3, 3), X, Y, m) < th_f).sum())
        always = (flags & (RWH_HYP_REPEATED | RWH_HYP_SINGULAR | RWH_HYP_DEGENERATE)) != 0
        rows = np.flatnonzero(~always)
        Hs = np.where(np.isfinite(H), H, 0).astype(np.float32)
        lo, hi = ive.score_interval(Hs, rows, flags, A, B, th_f, max(1.0, float(np.abs(A).max())), impl.IV_DELTA0, impl.IV_DELTA1)
        assert ((lo <= ref_counts[rows]) & (ref_counts[rows] <= hi)).all(), (key, int(((lo > ref_counts[rows]) | (ref_counts[rows] > hi)).sum()))
        need = kernels.need_count(A.shape[0], int(d[1:]), 4)
        out = {}
        for use_iv in (True, False):
            stats = {}
            pre = impl.presettle(torch.from_numpy(A), torch.from_numpy(B), A, B, idx, np.flatnonzero(impl.repeated_rows(idx)), th_f, m)
            w, early, cnt, words, _, _ = impl._settle_on_host(torch.from_numpy(A), torch.from_numpy(B), A, B, idx, dev_counts, flags, need, th_f, m,
                                                              impl.RESCORE_MARGIN, stats, pre=pre, H_dev=torch.from_numpy(Hs) if use_iv else None,
                                                              flags_dev=torch.from_numpy(flags) if use_iv else None)
            assert w == int(z[key + "_winner"]) and cnt == int(z[key + "_count"]) and early == bool(z[key + "_early"]), (key, use_iv, w, cnt, early)
            if words is None:
                inl = np.flatnonzero(orc.compute_loss(H[w].reshape(3, 3), X, Y, m) < th_f)
            else:
                inl = np.flatnonzero(np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:A.shape[0]])
            assert np.array_equal(inl, z[key + "_inliers"]), (key, use_iv)
            out[use_iv] = stats["host_settled"]
        assert out[True] <= out[False], (key, out)


def test_native_legacy_randint_is_numpys_stream():
    """rwh_host_legacy_randint (the index table of RANSAC.run, ransac.py:177) against numpy's own legacy randint: the same
    values, the same dtype for the int64 form, and the global generator left in the same place -- for ranges on and around
    powers of two (the rejection mask changes there), m = 1 (no draw), the largest range, arbitrary starting positions
    inside the MT19937 block, and table sizes that end inside / exactly on a block of 624 outputs."""
    rng = np.random.default_rng(1)
    ms = [1, 2, 3, 4, 5, 127, 128, 129, 185, 255, 256, 257, 1000, 65535, 65536, 65537, 2 ** 31 - 1]
    for case in range(120):
        m = int(ms[case % len(ms)]) if case < 60 else int(rng.integers(1, 10 ** 6))
        k, n = int(rng.integers(1024, 3000)), int(rng.choice([4, 4, 6, 1]))
        np.random.seed(int(rng.integers(0, 2 ** 31)))
        np.random.randint(0, 1000, int(rng.integers(0, 700)))
        st = np.random.get_state()
        a64, a32 = impl.legacy_randint_table(m, k, n)
        nxt_a = np.random.randint(0, 2 ** 30, 3)
        np.random.set_state(st)
        b = np.random.randint(0, m, (k, n))
        nxt_b = np.random.randint(0, 2 ** 30, 3)
        assert a64.dtype == b.dtype and np.array_equal(a64, b) and a32.dtype == np.int32 and np.array_equal(a32, b), (m, k, n)
        assert np.array_equal(nxt_a, nxt_b), (m, k, n)
    # a small table (numpy's own call is used) and the int32-only form
    np.random.seed(5); st = np.random.get_state()
    a64, a32 = impl.legacy_randint_table(185, 10, 4)
    np.random.set_state(st)
    assert np.array_equal(a64, np.random.randint(0, 185, (10, 4)))
    np.random.seed(6); st = np.random.get_state()
    none64, a32 = impl.legacy_randint_table(185, 5000, 4, want64=False)
    nxt = np.random.randint(0, 99)
    np.random.set_state(st)
    assert none64 is None and np.array_equal(a32, np.random.randint(0, 185, (5000, 4))) and nxt == np.random.randint(0, 99)


def test_interval_window_ignores_illcond_raw_counts(oracle_scorer, monkeypatch):
    """The candidate window of the 'fwd' interval rule is placed by the best raw count of an UNFLAGGED hypothesis only.  An
    RWH_HYP_ILLCOND raw count says nothing about the reference's count (the flag exists for exactly that disagreement): when it
    placed the window (best0 over every row without an always-bit), one ill-conditioned row far above the rest pushed the near-best
    unflagged rows out of it, they kept their raw K1 counts, and the row the reference ranks second won.  Real K1 / reference data
    (K1 emulated, intervals emulated, the oracle as scorer): rows 25 (K1 64, reference 65) and 82 (65 / 65), 40 low unflagged rows
    whose counts agree, and one low unflagged row re-flagged ill-conditioned with K1 count 209 and the reference H of row 25.
    The reference's winner is 25 (the first of the two 65s); the old window returned 82."""
    import bench
    import interval_emulation as ive
    from k1_emulation import RWH_HYP_ILLCOND, dlt4
    monkeypatch.setattr(kernels, "score_interval", lambda H, rows, flags, pa, pb, th, c, d0, d1: ive.score_interval(
        H.numpy(), rows, None if flags is None else flags.numpy(), pa.numpy(), pb.numpy(), th, c, d0, d1))
    rng = np.random.default_rng(7000)
    M = int(rng.integers(150, 400))
    G = rng.normal(500, 3, (M, 2))
    P = np.c_[G, np.ones(M)] @ bench.H_S.T
    B = P[:, :2] / P[:, 2:3] + rng.normal(0, 1, (M, 2))
    o = rng.random(M) < 0.35
    B[o] = rng.uniform(B.min(), B.max(), (o.sum(), 2))
    A, B = G.astype(np.float32), B.astype(np.float32)
    idx = rng.integers(0, M, (1500, 4)).astype(np.int32)
    th, X, Y = 3.0, A.T, B.T
    H, flags = dlt4(A, B, idx)
    Href = impl.svd_hypotheses(A, B, idx)

    def count(h):
        with np.errstate(all="ignore"):
            return int((orc.compute_loss(h.reshape(3, 3), X, Y, "fwd") < th).sum()) if np.isfinite(h).all() else 0
    dev = np.array([count(h) for h in H])
    ref = np.array([count(h) for h in Href])
    assert M == 339 and (dev[25], ref[25], dev[82], ref[82]) == (64, 65, 65, 65) and flags[25] == flags[82] == 0
    unflagged = np.flatnonzero(flags == 0)
    low = [int(i) for i in unflagged if dev[i] == ref[i] < 20][:40]
    fab = [int(i) for i in unflagged if ref[i] < 20 and int(i) not in low][0]
    rows = sorted([25, 82] + low + [fab])
    t_H, t_flags, t_cnt = H[rows].copy(), flags[rows].copy(), dev[rows].astype(np.int32)
    j = rows.index(fab)
    t_flags[j], t_H[j], t_cnt[j] = RWH_HYP_ILLCOND, Href[25], 209
    Ad, Bd = torch.from_numpy(A), torch.from_numpy(B)
    w, early, cnt, words, _, _ = impl._settle_on_host(Ad, Bd, A, B, idx[rows], t_cnt, t_flags, 10 ** 6, th, "fwd", impl.RESCORE_MARGIN, {},
                                                      H_dev=torch.from_numpy(t_H), flags_dev=torch.from_numpy(t_flags))
    assert (rows[w], early, cnt) == (25, False, 65), (rows[w], early, cnt)
    inl = np.flatnonzero(np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:M]) if words is not None else \
        np.flatnonzero(orc.compute_loss(H[25].reshape(3, 3), X, Y, "fwd") < th)
    assert np.array_equal(inl, np.flatnonzero(orc.compute_loss(Href[25].reshape(3, 3), X, Y, "fwd") < th))
