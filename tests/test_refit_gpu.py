"""The device refit on the MI355X: kernels.refit_batched (rwh_refit_batched) on one batch of the problems of refit_cases.PROBLEMS,
whose offsets are no multiples of 64, under every mask family -- within 1/16 of one inlier's effect of the exact fit and no further
from it than float64 lstsq (conditions A and B of tests/refit_cases.py), statuses, determinism, bit identity with the host twin,
garbage mask bits, non-finite coordinates, rank-deficient inlier sets, 66 000 problems in one launch -- and
run_batch(refit="device") against refit=True: same inliers, H within both conditions, H left on the device, no download of the
correspondences."""
import numpy as np
import pytest

import refit_cases as rc

pytestmark = pytest.mark.gpu

SIZES = tuple(len(rc.problem(name)[0]) for name in rc.PROBLEMS)
CASES = ["%s %s" % c for c in rc.cases()]
NAN33 = np.full((3, 3), np.nan)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch


def _upload(torch, rows):
    return torch.from_numpy(np.stack(rows).view(np.int64)).cuda()


def _refit(pa, pb, off, masks):
    from ransac_with_homography_amd import kernels
    H, st = kernels.refit_batched(pa, pb, off, masks)
    return H.cpu().numpy(), st.cpu().numpy()


@pytest.fixture(scope="module")
def batch(gpu):
    """The problems of refit_cases.PROBLEMS in one launch per mask family, and the first call's results."""
    torch = gpu
    probs = [rc.problem(name) for name in rc.PROBLEMS]
    offsets = np.zeros(len(SIZES) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(SIZES)
    assert (offsets[1:] % 64 != 0).all() and 0 < rc.PROBLEMS.index("empty") < len(SIZES) - 1
    bits = {family: [rc.family_bits(name, family) for name in rc.PROBLEMS] for family in rc.FAMILIES}
    b = dict(probs=probs, bits=bits, offsets=offsets,
             pa=torch.from_numpy(np.concatenate([u for u, _ in probs])).cuda(),
             pb=torch.from_numpy(np.concatenate([v for _, v in probs])).cuda(),
             off=torch.from_numpy(offsets).cuda(),
             masks={k: _upload(torch, [rc.pack(x, rc.MASK_WORDS) for x in v]) for k, v in bits.items()})
    b["first"] = {k: _refit(b["pa"], b["pb"], b["off"], m) for k, m in b["masks"].items()}
    return b


@pytest.fixture(scope="module")
def lib(gpu):
    from ransac_with_homography_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("which", ["all ones", "random"])
def test_batch_meets_yardstick(batch, which):
    """The earlier, loose yardstick: no further from lstsq's solution than the reference's float32 refit is."""
    family = {"all ones": "all", "random": "random half"}[which]
    H, st = batch["first"][family]
    assert H.shape == (len(SIZES), 3, 3) and H.dtype == np.float64 and st.dtype == np.int32
    for p, m in enumerate(SIZES):
        if m < 4:
            assert st[p] == rc.FEW and np.isnan(H[p]).all()
            continue
        u, v = batch["probs"][p]
        bits = batch["bits"][family][p]
        assert st[p] == rc.OK and np.isfinite(H[p]).all() and H[p, 2, 2] == 1.0
        H_ls, dev_ref = rc.yardstick(u, v, bits)
        dev = rc.deviation(H[p], H_ls, u)
        assert dev <= dev_ref, (m, which, dev, dev_ref)


@pytest.mark.parametrize("case", CASES, ids=[c.replace(" ", "_") for c in CASES])
def test_batch_is_within_one_inlier_of_the_exact_fit(batch, case):
    """Every (problem, family) that leaves 4 bits: OK, h33 == 1, and conditions A and B of refit_cases against the exact fit.
    "clustered M=300 top bits" is the case that takes the kernel's second pass (the corrected step of csrc/rwh_refit.h); every
    other case stays below its threshold."""
    name, family = rc.cases()[CASES.index(case)]
    p = rc.PROBLEMS.index(name)
    H, st = batch["first"][family]
    assert st[p] == rc.OK and np.isfinite(H[p]).all() and H[p, 2, 2] == 1.0
    rc.hold("gpu", case, H[p], *batch["probs"][p], batch["bits"][family][p])


def test_fewer_than_four_bits_give_few(batch):
    """The 3-point problem, the empty problem in the middle of the batch, and every problem a family leaves fewer than 4 bits of:
    FEW and an all-NaN H; every other status of the launch is OK."""
    for family, (H, st) in batch["first"].items():
        for p, name in enumerate(rc.PROBLEMS):
            few = batch["bits"][family][p].sum() < 4
            assert not (name in ("three", "empty") and not few)
            assert st[p] == (rc.FEW if few else rc.OK), (family, name)
            assert np.isnan(H[p]).all() if few else np.isfinite(H[p]).all(), (family, name)


def test_second_call_is_bit_identical(gpu, batch):
    for k, m in batch["masks"].items():
        H, st = _refit(batch["pa"], batch["pb"], batch["off"], m)
        assert np.array_equal(H, batch["first"][k][0], equal_nan=True)
        assert np.array_equal(st, batch["first"][k][1])


def test_host_twin_agrees_with_the_kernel(batch, lib):
    """rwh_host_refit runs the kernel's operations in the kernel's order (csrc/rwh_refit.h): the same statuses and the same H, bit
    for bit, for every problem under every family (both targets round float64 sqrt and divide correctly; neither contracts)."""
    for family, (H, st) in batch["first"].items():
        for p, (u, v) in enumerate(batch["probs"]):
            Hh, sh = rc.host_refit(lib, u, v, rc.pack(batch["bits"][family][p]))
            same = np.array_equal(Hh, H[p], equal_nan=True)
            if sh == rc.OK and st[p] == rc.OK:
                print("refit host-twin vs gpu %s %s: %.3e px apart, bit-identical %s" % (rc.PROBLEMS[p], family, rc.deviation(Hh, H[p], u), same))
            assert sh == st[p], (family, rc.PROBLEMS[p])
            assert same, (family, rc.PROBLEMS[p])


def test_corrected_step_walks_every_trip(gpu, lib):
    """refit_cases.patch(), 700 ill-conditioned correspondences, once per family in one launch, between two small problems: every
    one takes the kernel's second pass, through three trips of the stride loop.  OK, conditions A and B, and the twin's bits."""
    u, v = rc.patch()
    few, m = rc.problem("three"), len(u)
    bits = [rc.FAMILIES[family](m) for family in rc.PATCH_FAMILIES]
    assert all(rc.inverse_trace(u, v, b) >= 2.0 ** 34 for b in bits)
    probs = [few] + [(u, v)] * len(bits) + [rc.problem("synthetic M=5")]
    sizes = [len(a) for a, _ in probs]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    words = (m + 63) // 64
    rows = [np.ones(3, dtype=bool)] + bits + [np.ones(5, dtype=bool)]
    H, st = _refit(gpu.from_numpy(np.concatenate([a for a, _ in probs])).cuda(), gpu.from_numpy(np.concatenate([b for _, b in probs])).cuda(),
                   gpu.from_numpy(off).cuda(), _upload(gpu, [rc.pack(r, words) for r in rows]))
    assert st.tolist() == [rc.FEW] + [rc.OK] * (len(bits) + 1)
    for p, (family, b) in enumerate(zip(rc.PATCH_FAMILIES, bits), start=1):
        assert H[p, 2, 2] == 1.0
        rc.hold("gpu", "patch M=700 %s" % family, H[p], u, v, b)
        Hh, sh = rc.host_refit(lib, u, v, rc.pack(b))
        assert sh == rc.OK and np.array_equal(Hh, H[p])


def test_degenerate_problem_leaves_its_neighbours_alone(gpu, batch, lib):
    """One problem's points replaced by a single repeated correspondence: its own status is the host twin's (SINGULAR or OK, as the
    rounding of a zero pivot falls) with H NaN exactly when not OK, and the other results keep every bit."""
    p = SIZES.index(130)
    o0, o1 = int(batch["offsets"][p]), int(batch["offsets"][p + 1])
    pa, pb = batch["pa"].clone(), batch["pb"].clone()
    pa[o0:o1], pb[o0:o1] = pa[o0], pb[o0]
    H, st = _refit(pa, pb, batch["off"], batch["masks"]["all"])
    H0, st0 = batch["first"]["all"]
    others = [q for q in range(len(SIZES)) if q != p]
    assert np.array_equal(H[others], H0[others], equal_nan=True) and np.array_equal(st[others], st0[others])
    assert st[p] in (rc.OK, rc.SINGULAR)
    assert np.isnan(H[p]).all() if st[p] != rc.OK else np.isfinite(H[p]).all()
    u, v = (np.repeat(a[:1], 130, axis=0) for a in batch["probs"][p])
    Hh, sh = rc.host_refit(lib, u, v, rc.pack(np.ones(130, dtype=bool)))
    assert st[p] == sh and np.array_equal(H[p], Hh, equal_nan=True)


def test_bits_at_or_past_m_are_ignored(gpu, batch):
    """Every mask bit at or past M_p set -- the rest of the last word and every later word of the row: H and status keep every bit
    of the clean-mask result."""
    dirty = [rc.dirty(bits) for bits in batch["bits"]["random half"]]
    clean = batch["masks"]["random half"].cpu().numpy().view(np.uint64)
    assert all((d != c).sum() == rc.MASK_WORDS - m // 64 for d, c, m in zip(dirty, clean, SIZES))
    H, st = _refit(batch["pa"], batch["pb"], batch["off"], _upload(gpu, dirty))
    H0, st0 = batch["first"]["random half"]
    assert np.array_equal(st, st0) and np.array_equal(H, H0, equal_nan=True)


def _poison(batch, names, inlier):
    """The batch's points with one non-finite coordinate (refit_cases.POISONS, one each) in a correspondence of each problem of
    `names` whose random-half bit is set (inlier) or clear."""
    pa, pb = batch["pa"].cpu().numpy().copy(), batch["pb"].cpu().numpy().copy()
    for k, (name, (which, coordinate, value)) in enumerate(zip(names, rc.POISONS)):
        p = rc.PROBLEMS.index(name)
        at = np.flatnonzero(batch["bits"]["random half"][p] == inlier)
        i = int(batch["offsets"][p]) + int(at[-1 - k])
        (pa, pb)[which][i, coordinate] = value
    return pa, pb


POISONED = ("synthetic M=65", "synthetic M=257", "synthetic M=1281", "clustered M=300")


def test_non_finite_outliers_do_not_enter(gpu, batch):
    """A NaN or an infinity in a correspondence whose bit is clear leaves the same bits as a finite value there."""
    pa, pb = _poison(batch, POISONED, inlier=False)
    assert not np.isfinite(pa).all() and not np.isfinite(pb).all()
    H, st = _refit(gpu.from_numpy(pa).cuda(), gpu.from_numpy(pb).cuda(), batch["off"], batch["masks"]["random half"])
    H0, st0 = batch["first"]["random half"]
    assert np.array_equal(st, st0) and np.array_equal(H, H0, equal_nan=True)


def test_non_finite_inliers_give_singular(gpu, batch):
    """The same NaN or infinity in an inlier makes a moment non-finite, which fails the solve's `diagonal > 0 and finite` test:
    SINGULAR and an all-NaN H for that problem, every other result untouched."""
    pa, pb = _poison(batch, POISONED, inlier=True)
    H, st = _refit(gpu.from_numpy(pa).cuda(), gpu.from_numpy(pb).cuda(), batch["off"], batch["masks"]["random half"])
    H0, st0 = batch["first"]["random half"]
    hit = [rc.PROBLEMS.index(name) for name in POISONED]
    others = [q for q in range(len(SIZES)) if q not in hit]
    assert (st[hit] == rc.SINGULAR).all() and np.isnan(H[hit]).all()
    assert np.array_equal(st[others], st0[others]) and np.array_equal(H[others], H0[others], equal_nan=True)


def test_rank_deficient_inlier_sets(gpu, lib):
    """All inliers on one line, 4 inliers of which two are equal, one correspondence repeated: the device's status is the host
    twin's, H is NaN exactly when the status is not OK and bit-equal to the twin's when it is."""
    u1, v1 = rc.synthetic(64)
    u1[:], v1[:] = u1[0], v1[0]
    probs = [(u, v) for _, u, v in rc.rank_deficient()] + [(u1, v1)]
    sizes = [len(u) for u, _ in probs]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    words = (max(sizes) + 63) // 64
    masks = _upload(gpu, [rc.pack(np.ones(m, dtype=bool), words) for m in sizes])
    H, st = _refit(gpu.from_numpy(np.concatenate([u for u, _ in probs])).cuda(), gpu.from_numpy(np.concatenate([v for _, v in probs])).cuda(),
                   gpu.from_numpy(off).cuda(), masks)
    for p, (u, v) in enumerate(probs):
        Hh, sh = rc.host_refit(lib, u, v, rc.pack(np.ones(len(u), dtype=bool)))
        assert st[p] == sh and st[p] in (rc.OK, rc.SINGULAR), (p, st[p], sh)
        assert np.isnan(H[p]).all() if st[p] != rc.OK else np.isfinite(H[p]).all()
        assert np.array_equal(H[p], Hh, equal_nan=True), p


def test_many_small_problems_in_one_launch(gpu, lib):
    """66 000 problems of 4 to 7 correspondences, all bits set; every 97th has 3 and every 1013th is empty (its offset advances by
    0): block indices past 65 535.  Every status and H is the host twin's."""
    P = 66000
    sizes = np.random.default_rng(66000).integers(4, 8, P)
    sizes[96::97] = 3
    sizes[1012::1013] = 0
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    u, v = rc.synthetic(int(off[-1]))
    masks = gpu.full((P, 1), -1, dtype=gpu.int64, device="cuda")
    H, st = _refit(gpu.from_numpy(u).cuda(), gpu.from_numpy(v).cuda(), gpu.from_numpy(off).cuda(), masks)
    Hh, sh, word = np.empty((P, 9)), np.full(P, -1, dtype=np.int32), np.full(1, 2 ** 64 - 1, dtype=np.uint64)
    ua, va, ha, sa, wa = u.ctypes.data, v.ctypes.data, Hh.ctypes.data, sh.ctypes.data, word.ctypes.data
    for p, (o, m) in enumerate(zip(off[:-1].tolist(), sizes.tolist())):
        assert lib.rwh_host_refit(ua + 8 * o, va + 8 * o, m, wa, ha + 72 * p, sa + 4 * p) == 0
    assert (sh[sizes < 4] == rc.FEW).all() and (sh[sizes >= 4] != rc.FEW).all() and (sh == rc.OK).sum() > P // 2
    assert np.array_equal(st, sh)
    assert np.array_equal(H.reshape(P, 9), Hh, equal_nan=True)


def test_short_mask_rows_are_not_read_past(gpu, batch):
    """A mask narrower than a problem (the caller's error) is not read past its end: correspondences beyond it count as outliers."""
    from ransac_with_homography_amd import kernels
    torch = gpu
    u, v = batch["probs"][SIZES.index(130)]
    pa, pb = torch.from_numpy(u.copy()).cuda(), torch.from_numpy(v.copy()).cuda()
    off = torch.tensor([0, 130], dtype=torch.int32, device="cuda")
    one_word = torch.full((1, 1), -1, dtype=torch.int64, device="cuda")
    three = torch.tensor([[-1, 0, 0]], dtype=torch.int64, device="cuda")       # what the problem needs, the same inliers
    H1, s1 = kernels.refit_batched(pa, pb, off, one_word)
    H3, s3 = kernels.refit_batched(pa, pb, off, three)
    assert int(s1[0]) == int(s3[0]) == rc.OK and torch.equal(H1, H3)


def _pairs():
    u, v = rc.matchespoints()
    return [[u.T.copy(), v.T.copy()], [u[:40].T.copy(), v[:40].T.copy()], [u.T.copy(), v.T.copy()]]


def _device_problems(torch, rmod, probs):
    pa = torch.from_numpy(np.concatenate([X.T for X, _ in probs])).cuda()
    pb = torch.from_numpy(np.concatenate([Y.T for _, Y in probs])).cuda()
    return rmod.DeviceProblems(pa, pb, [X.shape[1] for X, _ in probs])


KW = dict(seed=0, k=256, d=70, th=5, method="fwd")


def _check_against_host_refit(probs, got, want, label):
    for p, ((X, Y), g, w) in enumerate(zip(probs, got, want)):
        assert np.array_equal(g[1][0], w[1][0]) and int(g[2]) == int(w[2])
        assert g[0] is not None and g[0].dtype == np.float64 and g[0].shape == (3, 3)
        bits = np.zeros(X.shape[1], dtype=bool)
        bits[g[1][0]] = True
        H_ls, dev_ref = rc.yardstick(X.T, Y.T, bits)
        assert rc.deviation(g[0], H_ls, X.T) <= dev_ref
        assert g[0][2, 2] == 1.0
        rc.hold("gpu", "%s problem %d" % (label, p), g[0], np.ascontiguousarray(X.T), np.ascontiguousarray(Y.T), bits)    # A and B on the winner's inliers


def test_run_batch_device_refit(gpu, monkeypatch):
    from ransac_with_homography_amd import ransac as rmod
    torch = gpu
    probs = _pairs()
    dp = _device_problems(torch, rmod, probs)
    total = sum(dp.sizes)
    want = rmod.run_batch(dp, refit=True, **KW)
    asked = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (asked.append(tuple(self.shape)), real_cpu(self, *a, **k))[1])
    info = {}
    got = rmod.run_batch(dp, refit="device", info=info, **KW)
    from_list = rmod.run_batch(probs, refit="device", **KW)
    monkeypatch.undo()
    assert asked and (total, 2) not in asked, asked        # the correspondences never visit the host
    _check_against_host_refit(probs, got, want, "run_batch")
    Hd, st = info["H_device"], info["refit_status"]
    assert Hd.is_cuda and Hd.dtype == torch.float64 and tuple(Hd.shape) == (3, 3, 3) and st.is_cuda and st.dtype == torch.int32
    assert (st.cpu().numpy() == rc.OK).all()
    for p, g in enumerate(got):
        assert np.array_equal(Hd[p].cpu().numpy(), g[0])
        assert np.array_equal(from_list[p][0], g[0]) and np.array_equal(from_list[p][1][0], g[1][0])


def test_run_batch_device_refit_with_index_tables(gpu):
    """idx= mode: the host settle step may replace a winner's mask; those words are uploaded over the gathered rows."""
    from ransac_with_homography_amd import ransac as rmod
    probs = _pairs()
    dp = _device_problems(gpu, rmod, probs)
    rs = np.random.RandomState(0)
    idx = [rs.randint(0, X.shape[1], (KW["k"], 4)) for X, _ in probs]
    kw = {k: v for k, v in KW.items() if k != "seed"}
    want = rmod.run_batch(dp, refit=True, idx=idx, **kw)
    got = rmod.run_batch(dp, refit="device", idx=idx, **kw)
    _check_against_host_refit(probs, got, want, "run_batch idx=")


def test_run_batch_too_few_inliers_gives_none(gpu):
    """A problem of three correspondences: FEW on the device, None in the list, as the host refit."""
    from ransac_with_homography_amd import ransac as rmod
    u, v = rc.matchespoints()
    probs = [[u.T.copy(), v.T.copy()], [u[:3].T.copy(), v[:3].T.copy()]]
    info = {}
    got = rmod.run_batch(probs, refit="device", info=info, **KW)
    want = rmod.run_batch(probs, refit=True, **KW)
    assert got[0][0] is not None and got[1][0] is None and want[1][0] is None
    assert int(got[1][2]) == int(want[1][2]) and np.array_equal(got[1][1][0], want[1][1][0])
    assert info["refit_status"].cpu().numpy().tolist() == [rc.OK, rc.FEW] and bool(info["H_device"][1].isnan().all())


def test_run_batch_refit_values(gpu):
    from ransac_with_homography_amd import ransac as rmod
    probs = _pairs()
    with pytest.raises(ValueError):
        rmod.run_batch(probs, refit="bogus", **KW)
    a = rmod.run_batch(probs, refit=False, **KW)
    assert all(r[0] is None for r in a)


def test_sharded_wrapper_forwards_the_mode(gpu):
    from ransac_with_homography_amd import ransac as rmod
    from ransac_with_homography_amd import sharded
    probs = _pairs()
    got, span = sharded.run_batch_sharded(probs, refit="device", **KW)
    want = rmod.run_batch(probs, refit="device", **KW)
    assert span == (0, 3)
    for g, w in zip(got, want):
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1][0], w[1][0]) and int(g[2]) == int(w[2])
