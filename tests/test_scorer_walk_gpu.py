"""The scorer (K2) with several hypotheses per wavefront, on the MI355X.  rwh_lab_tune RWH_TUNE_SCORE_HPW forces what the
launchers only choose from 14 000 hypotheses up, so every path of the walk -- the block of 7 matrices a wave fetches at a time, lane q
inverting hypothesis q of a block, the running count / mask pointers, a short last wave, waves that end at a problem's boundary --
is reached at K = 100: every kernel form (filter W = 1..4 with and without masks, chunked, general with registers and streamed,
single and batched, the caller's inverses), against oracle/rwh_oracle.py hypothesis by hypothesis with no tolerance.  Inputs and
the oracle helpers: tests/scorer_cases.py; what makes "no tolerance" legitimate is asserted by tests/test_scorer_walk_cpu.py.
A run of the kernel at another hpw is never the expected value."""
import contextlib

import numpy as np
import pytest

import scorer_cases as sc
from oracle import rwh_oracle as orc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

UNREACHABLE = 1 << 30


@pytest.fixture(scope="module")
def gpu():
    from ransac_with_homography_amd import _lib
    return _lib.require_gpu()  # raises (test error, not skip) when the HIP path is unavailable


def _tune(knob, value):
    from ransac_with_homography_amd import _lib
    assert _lib.load().rwh_lab_tune(getattr(_lib, knob), int(value)) == 0


@pytest.fixture(autouse=True)
def release_scorer_knobs():
    """The knobs are process globals: whatever a test did, the next one starts from the library's own choice."""
    yield
    _tune("RWH_TUNE_SCORE_HPW", 0)
    _tune("RWH_TUNE_SCORE_EXACT", 0)


@contextlib.contextmanager
def forced_hpw(hpw):
    _tune("RWH_TUNE_SCORE_HPW", hpw)
    try:
        yield
    finally:
        _tune("RWH_TUNE_SCORE_HPW", 0)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _want_winner(counts, need):
    """select_winner, with the reference's "no model" when nothing scored above zero (decode_best's None)."""
    w, early = orc.select_winner(np.asarray(counts), need)
    return (None, False) if (not early and counts[w] <= 0) else (w, early)


def _check_keys(best_words, counts_o, need, label, hyp_base=0):
    from ransac_with_homography_amd import kernels
    w, early = _want_winner(counts_o, need)
    got = kernels.decode_best(best_words, len(counts_o))
    assert (got[0], got[2]) == (None if w is None else hyp_base + w, early), (label, got, w, early)
    if w is not None and not early:
        assert got[1] == int(counts_o[w]), (label, got)


def _check_rows(counts, masks, bits_o, counts_o, m, label):
    """Counts, and (masks given) every mask bit, equal the oracle's; bits and words past m are clear."""
    bad = np.nonzero(np.asarray(counts) != counts_o)[0]
    assert bad.size == 0, (label, "first differing hypothesis %d (position %d of its block of 7): count %d, oracle %d"
                           % (bad[0], bad[0] % 7, counts[bad[0]], counts_o[bad[0]]))
    if masks is not None:
        got = sc.unpack(masks, m)
        bad = np.nonzero((got[:, :m] != bits_o).any(axis=1))[0]
        assert bad.size == 0, (label, "first hypothesis with a differing mask: %d (position %d of its block of 7)" % (bad[0], bad[0] % 7))
        assert not got[:, m:].any(), (label, "bits past M")


# ---------------------------------------------------------------------------------------------------------------------------
# 1 + 2: single search, every kernel form, and its accept keys
# ---------------------------------------------------------------------------------------------------------------------------
_single_cache = {}


def single_configs(M):
    """Per M, once: (label, case, H [100, 9], method, numpy's inverses or None, oracle errors, bits, counts)."""
    if M not in _single_cache:
        from ransac_with_homography_amd import kernels
        a, b = sc.stress(M), sc.cleared(M)
        hb = sc.cleared_hypotheses(b, sc.K_SINGLE)
        hinv = kernels.host_inverses(a["H"])
        cfgs = []
        for label, case, H, method, inv in (("stress fwd", a, a["H"], "fwd", None), ("stress backward hinv", a, a["H"], "backward", hinv),
                                            ("stress reproj hinv", a, a["H"], "reproj", hinv), ("cleared backward", b, hb, "backward", None),
                                            ("cleared reproj", b, hb, "reproj", None)):
            err = sc.oracle_errors(H, case["X"], case["Y"], method)
            bits, counts = sc.decisions(err, sc.threshold(method))
            cfgs.append(dict(label=label, case=case, H=H, method=method, hinv=inv, err=err, bits=bits, counts=counts))
        _single_cache[M] = cfgs
    return _single_cache[M]


def _reached_need(cfg):
    """A `need` some hypothesis reaches: cleared cases -- group 3's count, first met at hypothesis 3 (the CPU test asserts it);
    stress cases -- the third largest count."""
    if "G" in cfg["case"]:
        return sc.group_need(cfg["case"], cfg["counts"])
    return int(np.sort(cfg["counts"])[-3])


@pytest.mark.parametrize("M", sc.SINGLE_SIZES)
def test_single_search_every_form_and_its_keys(gpu, M):
    """kernels.score_count on uploaded H: K = 100 and K = 3, every hpw of HPW_SINGLE, masks on and off, a `need` nothing reaches
    (the tie between hypotheses i and i + G has to go to the lower index) and one that is reached: counts, masks and decode_best
    against the oracle; without masks the same counts and the same two key words."""
    from ransac_with_homography_amd import kernels
    for cfg in single_configs(M):
        case, method, th = cfg["case"], cfg["method"], sc.threshold(cfg["method"])
        pa, pb = _dev(case["A"], gpu), _dev(case["B"], gpu)
        for K in (sc.K_SINGLE, 3):
            Hd = _dev(cfg["H"][:K], gpu)
            hinv = _dev(cfg["hinv"][:K], gpu) if cfg["hinv"] is not None else None
            bits_o, counts_o = cfg["bits"][:K], cfg["counts"][:K]
            for hpw in sc.HPW_SINGLE:
                for need in (UNREACHABLE, _reached_need(cfg)):
                    label = (M, cfg["label"], "K", K, "hpw", hpw, "need", need)
                    got = {}
                    with forced_hpw(hpw):
                        for want_masks in (True, False):
                            best = kernels.new_best(gpu)
                            counts, masks, _ = kernels.score_count(Hd, pa, pb, th, method, need, best, want_masks=want_masks, hinv=hinv)
                            got[want_masks] = (counts.cpu().numpy(), masks.cpu().numpy() if want_masks else None, best.cpu().numpy())
                    assert got[False][1] is None
                    _check_rows(got[True][0], got[True][1], bits_o, counts_o, M, label + ("masks",))
                    _check_rows(got[False][0], None, bits_o, counts_o, M, label + ("no masks",))
                    _check_keys(got[True][2], counts_o, need, label)
                    assert np.array_equal(got[True][2], got[False][2]), label


@pytest.mark.parametrize("M", [185, 700])
def test_error_rows_are_the_oracles_bits(gpu, M):
    """want_err=True switches to the general kernel (M = 185: points in registers, 700: streamed): 'fwd' error rows bit-identical
    to the oracle's float32, with counts and masks, at every hpw."""
    from ransac_with_homography_amd import kernels
    cfg = single_configs(M)[0]
    assert cfg["method"] == "fwd"
    case = cfg["case"]
    pa, pb = _dev(case["A"], gpu), _dev(case["B"], gpu)
    for K in (sc.K_SINGLE, 3):
        Hd = _dev(cfg["H"][:K], gpu)
        for hpw in sc.HPW_SINGLE:
            label = (M, "K", K, "hpw", hpw)
            with forced_hpw(hpw):
                counts, masks, err = kernels.score_count(Hd, pa, pb, sc.TH, "fwd", UNREACHABLE, kernels.new_best(gpu), want_err=True)
            _check_rows(counts.cpu().numpy(), masks.cpu().numpy(), cfg["bits"][:K], cfg["counts"][:K], M, label)
            e, ref = err.cpu().numpy(), cfg["err"][:K]
            fin = np.isfinite(ref)
            bad = np.nonzero(((e.view(np.uint32) != ref.view(np.uint32)) & fin).any(axis=1) | (np.isnan(e) != np.isnan(ref)).any(axis=1))[0]
            assert bad.size == 0, (label, "first hypothesis with a differing error row: %d" % bad[0])


def test_accept_keys_carry_the_index_bits(gpu):
    """hyp_base = 4 000 000 000 (inside the 0xFFFFFFFF limit): the winner's index comes back offset, at hpw 14 as at 1."""
    from ransac_with_homography_amd import kernels
    base = 4_000_000_000
    for cfg in (single_configs(185)[0], single_configs(185)[3]):
        case, method = cfg["case"], cfg["method"]
        pa, pb, Hd = _dev(case["A"], gpu), _dev(case["B"], gpu), _dev(cfg["H"], gpu)
        for hpw in (1, 14):
            for need in (UNREACHABLE, _reached_need(cfg)):
                best = kernels.new_best(gpu)
                with forced_hpw(hpw):
                    counts, _, _ = kernels.score_count(Hd, pa, pb, sc.threshold(method), method, need, best, hyp_base=base, want_masks=False)
                assert np.array_equal(counts.cpu().numpy(), cfg["counts"])
                _check_keys(best.cpu().numpy(), cfg["counts"], need, (cfg["label"], hpw, need), hyp_base=base)


# ---------------------------------------------------------------------------------------------------------------------------
# 3 .. 6: the batched walk
# ---------------------------------------------------------------------------------------------------------------------------
_batch_cache = {}
_row_cache = {}


def batch_of(sizes, k_per, gpu, seeds=None):
    """Per (sizes, k_per, seeds), once: the cleared problems, their sample rows, the device tensors and, per loss, the oracle's
    decisions on its OWN 4-point fits of those rows (what the CPU test cleared)."""
    seeds = tuple(seeds) if seeds else (sc.SEED,) * len(sizes)
    key = (tuple(sizes), k_per, seeds)
    if key not in _batch_cache:
        cases = [sc.cleared(m, seed=s) for m, s in zip(sizes, seeds)]
        idx = np.stack([sc.cleared_samples(c, k_per) for c in cases])
        A, B, off = sc.concat(cases)
        once = {}                                       # (copies of one problem: one fit)
        for p, ms in enumerate(zip(sizes, seeds)):
            if ms not in once:
                once[ms] = sc.fitted(cases[p], idx[p])
        fitted = [once[ms] for ms in zip(sizes, seeds)]
        _batch_cache[key] = dict(cases=cases, idx=idx, off=off, fitted=fitted, fitted_dec={}, pa=_dev(A, gpu), pb=_dev(B, gpu),
                                 off_d=_dev(off, gpu), idx_d=_dev(idx, gpu))
    return _batch_cache[key]


def fitted_decisions(b, method):
    if method not in b["fitted_dec"]:
        b["fitted_dec"][method] = [oracle_rows(c, f, method) for c, f in zip(b["cases"], b["fitted"])]
    return b["fitted_dec"][method]


def oracle_rows(case, H, method):
    """(bits, counts) of the oracle on the rows of H; rows seen before (the same sample, or an earlier run) are not recomputed."""
    bits = np.empty((len(H), case["M"]), dtype=bool)
    for i, h in enumerate(H):
        key = (case["M"], case["seed"], method, h.tobytes())
        if key not in _row_cache:
            _row_cache[key] = sc.decisions(sc.oracle_errors(h[None], case["X"], case["Y"], method), sc.threshold(method))[0][0]
        bits[i] = _row_cache[key]
    return bits, bits.sum(axis=1).astype(np.int64)


def run_batched(b, sizes, k_per, method, needs, want_masks, gpu, early_stop=False):
    """One rwh_ransac_batched call into buffers filled with sentinels -> (H, counts, masks or None, best) on the host."""
    from ransac_with_homography_amd import kernels
    ws = kernels.BatchWorkspace(len(sizes), k_per, max(sizes), gpu, want_masks=want_masks)
    ws.counts.fill_(-7)
    if want_masks:
        ws.masks.fill_(-1)
    kernels.ransac_batched(b["pa"], b["pb"], b["off_d"], _dev(np.asarray(needs, dtype=np.int32), gpu), sc.threshold(method), method, ws,
                           idx=b["idx_d"], early_stop=early_stop)
    return ws.H.cpu().numpy(), ws.counts.cpu().numpy(), ws.masks.cpu().numpy() if want_masks else None, ws.best.cpu().numpy()


def need_sets(b, method):
    """Per problem: a `need` nothing reaches, and group 3's count (first met at hypothesis 3; one group: at 0)."""
    dec = fitted_decisions(b, method)
    return [[UNREACHABLE] * len(dec), [sc.group_need(c, d[1]) for c, d in zip(b["cases"], dec)]]


def check_batched(b, sizes, k_per, method, needs, out, label):
    """Per problem: counts and masks equal the oracle on the rows of ws.H read back -- whose decisions are those of the oracle's own
    fits --, words past ceil(m / 64) are zero, decode_best(ws.best[p]) is select_winner's."""
    H, counts, masks, best = out
    for p, (case, m) in enumerate(zip(b["cases"], sizes)):
        bits_o, counts_o = oracle_rows(case, H[p], method)
        assert np.array_equal(bits_o, fitted_decisions(b, method)[p][0]), (label, p, "K1's H and LAPACK's decide differently")
        _check_rows(counts[p], masks[p] if masks is not None else None, bits_o, counts_o, m, label + ("problem", p, "M", m))
        _check_keys(best[p], counts_o, needs[p], label + ("problem", p))


def _batched_walk(gpu, sizes):
    b = batch_of(sizes, sc.K_PER, gpu)
    for method in sc.METHODS:
        for needs in need_sets(b, method):
            for hpw in sc.HPW_BATCHED:
                for want_masks in (True, False):
                    with forced_hpw(hpw):
                        out = run_batched(b, sizes, sc.K_PER, method, needs, want_masks, gpu)
                    check_batched(b, sizes, sc.K_PER, method, needs, out, (method, "hpw", hpw, "masks", want_masks, "needs", needs[0]))


def test_batched_walk_register_form(gpu):
    """Sizes 5 .. 256 (m_max = 256: the filter kernel with W = 4, shorter problems ride along), 23 hypotheses per problem, every
    hpw of HPW_BATCHED (64 is clamped to 23 on the host), all three losses, K1's own H, masks pre-filled with -1, and without masks."""
    _batched_walk(gpu, sc.REGISTER_BATCH)


def test_batched_walk_streamed_form(gpu):
    """Sizes 700, 30, 257 (m_max = 700: the general kernel with offsets and a mask stride of 11 words): as the register form."""
    _batched_walk(gpu, sc.STREAMED_BATCH)


@pytest.mark.parametrize("k_per", sc.K_PER_BENCH)
def test_bench_configuration_in_miniature(gpu, k_per):
    """bench.py's scorer configuration at a size the oracle can follow: hpw 14, 'fwd', no masks, the caller's samples, one cleared
    problem of 185 pairs three times, more than one argmax block per problem; k_per = 2102 ends every problem in a short wave.
    Three identical problems cannot show a wave that walks on into the next problem (it meets the same pairs there), so the
    same launch is repeated with another cleared problem of 185 pairs in the middle: the outer two stay bit-identical."""
    sizes = (185, 185, 185)
    for seeds in (None, (sc.SEED, sc.SEED + 1, sc.SEED)):
        b = batch_of(sizes, k_per, gpu, seeds)
        dec = fitted_decisions(b, "fwd")
        for needs in ([UNREACHABLE] * 3, [sc.group_need(b["cases"][0], dec[0][1], 3), sc.group_need(b["cases"][1], dec[1][1], 5), UNREACHABLE]):
            with forced_hpw(14):
                out = run_batched(b, sizes, k_per, "fwd", needs, False, gpu)
            check_batched(b, sizes, k_per, "fwd", needs, out, ("bench", k_per, "seeds", seeds, "needs", needs[0]))
            H, counts, _, best = out
            for p in (2,) if seeds else (1, 2):
                assert np.array_equal(H[p].view(np.uint32), H[0].view(np.uint32)) and np.array_equal(counts[p], counts[0]), p
                if needs[p] == needs[0]:
                    assert np.array_equal(best[p], best[0]), p


@pytest.mark.parametrize("k_per", [sc.K_PER, sc.K_PER_BENCH[1]])
@pytest.mark.parametrize("hpw", [7, 14])
def test_early_stop_with_several_hypotheses_per_wave(gpu, hpw, k_per):
    """RWH_BATCH_EARLY_STOP at hpw 7 and 14: `needs` from the oracle's counts put every problem's exit at a known hypothesis (0, 3, 5,
    or none).  decode_best is select_winner's; every hypothesis up to the exit carries the oracle's count and mask; a count of -1
    lies after the exit and has an all-zero mask row; every other count (and mask) is the oracle's."""
    sizes = sc.REGISTER_BATCH if k_per == sc.K_PER else (185, 185, 185)
    b = batch_of(sizes, k_per, gpu)
    for method in (sc.METHODS if k_per == sc.K_PER else ("fwd",)):
        dec = fitted_decisions(b, method)
        pick = (3, 3, 5, None, 3) if k_per == sc.K_PER else (3, 5, None)
        needs = [UNREACHABLE if g is None else sc.group_need(c, d[1], g) for c, d, g in zip(b["cases"], dec, pick)]
        for want_masks in (True, False):
            with forced_hpw(hpw):
                H, counts, masks, best = run_batched(b, sizes, k_per, method, needs, want_masks, gpu, early_stop=True)
            for p, (case, m) in enumerate(zip(b["cases"], sizes)):
                label = (method, "hpw", hpw, "k_per", k_per, "masks", want_masks, "problem", p)
                bits_o, counts_o = oracle_rows(case, H[p], method)
                w, early = _want_winner(counts_o, needs[p])
                assert early == (pick[p] is not None) and (not early or w == min(pick[p], case["G"] - 1)), label   # the exit is where it was put
                _check_keys(best[p], counts_o, needs[p], label)
                skipped = counts[p] == -1
                assert not skipped[:w + 1].any() if early else not skipped.any(), label
                assert np.array_equal(counts[p][~skipped], counts_o[~skipped]), label
                if masks is not None:
                    got = sc.unpack(masks[p], m)
                    assert not got[skipped].any(), label
                    assert np.array_equal(got[~skipped][:, :m], bits_o[~skipped]) and not got[:, m:].any(), label
