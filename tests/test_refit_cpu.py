"""rwh_host_refit, the host twin of the device refit (csrc/rwh_refit.h: the same moment update and 8 x 8 solve the kernel runs),
without a GPU: accuracy against the yardstick of tests/refit_cases.py, mask handling, degenerate inputs, argument validation."""
import numpy as np
import pytest

import refit_cases as rc


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ransac_with_homography_amd import _lib
    return _lib.load()


def _cases():
    ua, va = rc.matchespoints()
    yield "matchespoints all", ua, va, np.ones(len(ua), dtype=bool)
    yield "matchespoints random half", ua, va, rc.random_bits(len(ua), 7)
    for m in rc.SYNTHETIC_SIZES:
        u, v = rc.synthetic(m)
        yield "synthetic M=%d all" % m, u, v, np.ones(m, dtype=bool)


CASES = list(_cases())


@pytest.mark.parametrize("name,u,v,bits", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_host_refit_meets_yardstick(lib, name, u, v, bits):
    """The host twin is no further from the float64 least-squares solution than the reference's float32 refit is."""
    H_ls, dev_ref = rc.yardstick(u, v, bits)
    H, st = rc.host_refit(lib, u, v, rc.pack(bits))
    assert st == rc.OK and np.isfinite(H).all() and H[2, 2] == 1.0
    dev = rc.deviation(H, H_ls, u)
    rc.report("host-twin", name, dev, dev_ref)
    assert dev <= dev_ref


def test_bits_beyond_m_are_ignored(lib):
    """Bits at or past M in the last word do not enter: the same H, bit for bit, as with the clean mask."""
    for m in (5, 63, 65, 185):
        u, v = rc.synthetic(m)
        bits = rc.random_bits(m, 3)
        clean = rc.pack(bits)
        dirty = clean.copy()
        dirty[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(m % 64) if m % 64 else np.uint64(0)
        assert m % 64 == 0 or dirty[-1] != clean[-1]
        H0, s0 = rc.host_refit(lib, u, v, clean)
        H1, s1 = rc.host_refit(lib, u, v, dirty)
        assert s0 == s1 == rc.OK and np.array_equal(H0, H1)


def test_random_masks_select_the_subset(lib):
    """The mask selects: over a random half of every synthetic size the fit is that subset's least-squares fit (the yardstick on
    the subset; one wrong, dropped or extra point moves the fit by a visible fraction of the 1 px noise)."""
    for m in rc.SYNTHETIC_SIZES[1:]:
        u, v = rc.synthetic(m)
        bits = rc.random_bits(m, 11)
        H_ls, dev_ref = rc.yardstick(u, v, bits)
        H, st = rc.host_refit(lib, u, v, rc.pack(bits))
        assert st == rc.OK
        dev = rc.deviation(H, H_ls, u)
        rc.report("host-twin", "synthetic M=%d random half" % m, dev, dev_ref)
        assert dev <= dev_ref


def test_three_bits_give_few(lib):
    u, v = rc.synthetic(65)
    for pos in ((0, 1, 2), (3, 40, 64)):
        bits = np.zeros(65, dtype=bool)
        bits[list(pos)] = True
        H, st = rc.host_refit(lib, u, v, rc.pack(bits))
        assert st == rc.FEW and np.isnan(H).all()
    H, st = rc.host_refit(lib, u[:0], v[:0], rc.pack(np.zeros(0, dtype=bool)))
    assert st == rc.FEW and np.isnan(H).all()


def test_four_points_are_fitted_exactly(lib):
    """M = 4, all bits: the system is square, the least-squares solution interpolates, so the four points reproject onto their
    targets up to the solver's rounding.  Bound, from the method and float64 alone: with B = A D (D the equilibration, unit
    columns, |row of B| <= sqrt 8) and g = D^-1 h, a Cholesky solve of the normal equations is backward stable in B^T B, so
    |g^ - g| <= C u cond2(B^T B) |g|, u = 2^-53, C = n (3 n + 1) + n (M + 3) for n = 8 (Cholesky and triangular solves: Higham,
    Accuracy and Stability, thm 10.4; M + 3 roundings in every moment).  A row's residual moves by at most sqrt 8 |g^ - g| and the
    reprojection error is the residual over the point's denominator w.  That worst-case bound is loose (6.4e-07 px), so the cap
    that bites is the yardstick's own error: the four points reproject no worse through H than through H_ls, numpy's float64
    lstsq on the same system (2.4e-09 px: its SVD works on the unscaled A, cond 1e7).  Measured: 5.9e-12 px."""
    u, v = rc.synthetic(4)
    bits = np.ones(4, dtype=bool)
    H_ls, dev_ref = rc.yardstick(u, v, bits)
    H, st = rc.host_refit(lib, u, v, rc.pack(bits))
    assert st == rc.OK
    assert rc.deviation(H, H_ls, u) <= dev_ref
    A, b = rc.system(u, v)
    scale = np.sqrt((A * A).sum(axis=0))
    B = A / scale
    g = H.ravel()[:8] * scale
    w = np.abs(np.concatenate([u.astype(np.float64), np.ones((4, 1))], axis=1) @ H[2])
    C = 8 * (3 * 8 + 1) + 8 * (4 + 3)
    bound = np.sqrt(8.0) * C * 2.0 ** -53 * np.linalg.cond(B.T @ B) * np.linalg.norm(g) / w.min()
    err = float(np.sqrt(((rc.project(H, u) - v.astype(np.float64)) ** 2).sum(axis=1)).max())
    err_ls = float(np.sqrt(((rc.project(H_ls, u) - v.astype(np.float64)) ** 2).sum(axis=1)).max())
    print("refit host-twin M=4 exact fit: reprojection error %.3e px, float64 lstsq's own %.3e px, worst-case bound %.3e px"
          % (err, err_ls, bound))
    assert err <= err_ls and err <= bound


def test_one_repeated_correspondence(lib):
    """All inliers the same correspondence: A^T A has rank 2.  The call returns; whichever way the rounding of a zero pivot falls,
    H is NaN exactly when the status is not OK."""
    for m in (4, 64, 185):
        u, v = rc.synthetic(m)
        u[:], v[:] = u[0], v[0]
        H, st = rc.host_refit(lib, u, v, rc.pack(np.ones(m, dtype=bool)))
        assert st in (rc.OK, rc.SINGULAR)
        assert np.isnan(H).all() if st != rc.OK else np.isfinite(H).all()
    z = np.zeros((8, 2), dtype=np.float32)          # a zero diagonal entry: certainly singular
    H, st = rc.host_refit(lib, z, z, rc.pack(np.ones(8, dtype=bool)))
    assert st == rc.SINGULAR and np.isnan(H).all()


def test_argument_validation(lib):
    u, v = rc.synthetic(8)
    w, h, st = rc.pack(np.ones(8, dtype=bool)), np.empty(9), np.zeros(1, dtype=np.int32)
    good = [u.ctypes.data, v.ctypes.data, 8, w.ctypes.data, h.ctypes.data, st.ctypes.data]
    assert lib.rwh_host_refit(*good) == 0
    for i in (0, 1, 3, 4, 5):
        bad = list(good)
        bad[i] = rc.null
        assert lib.rwh_host_refit(*bad) == -1
    bad = list(good)
    bad[2] = -1
    assert lib.rwh_host_refit(*bad) == -1
    one = 1         # non-NULL, never dereferenced: validation comes first
    assert lib.rwh_refit_batched(rc.null, one, one, 1, one, 1, one, one, rc.null) == -1
    assert lib.rwh_refit_batched(one, one, one, 0, one, 1, one, one, rc.null) == -1
    assert lib.rwh_refit_batched(one, one, one, 1, one, 0, one, one, rc.null) == -1
    assert lib.rwh_refit_batched(one, one, one, 1, rc.null, 1, one, one, rc.null) == -1


def test_run_batch_rejects_unknown_refit():
    from ransac_with_homography_amd import ransac as rmod
    X = np.zeros((2, 8), dtype=np.float32)
    with pytest.raises(ValueError):
        rmod.run_batch([[X, X]], method="fwd", refit="bogus")
