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


CASES = ["%s %s" % c for c in rc.cases()]


def _case(case):
    name, family = rc.cases()[CASES.index(case)]
    return (*rc.problem(name), rc.family_bits(name, family))


def test_exact_fit_is_the_least_squares_solution():
    """The reference of every test below, checked on its own: the normal-equation residual A^T (A h_x - b), evaluated in
    rational arithmetic for the rounded H_x, is zero to the rounding of the eight results; and a singular A^T A raises."""
    F = rc.fractions.Fraction
    u, v = rc.problem("synthetic M=65")
    bits = rc.family_bits("synthetic M=65", "random half")
    H_x = rc.exact_fit(u, v, bits)
    A, b = rc.system(u[bits], v[bits])
    A, b, h = [[F(t) for t in row] for row in A.tolist()], [F(t) for t in b.tolist()], [F(t) for t in H_x.ravel()[:8].tolist()]
    res = [sum(a * t for a, t in zip(row, h)) - y for row, y in zip(A, b)]
    grad = [sum(row[j] * r for row, r in zip(A, res)) for j in range(8)]
    col = [sum(abs(row[j]) * sum(abs(a * t) for a, t in zip(row, h)) for row in A) for j in range(8)]
    assert all(abs(g) <= 8 * F(2) ** -53 * c for g, c in zip(grad, col))
    for _, ud, vd in rc.rank_deficient():
        with pytest.raises(ZeroDivisionError):
            rc.exact_fit(ud, vd, np.ones(len(ud), dtype=bool))


@pytest.mark.parametrize("case", CASES, ids=[c.replace(" ", "_") for c in CASES])
def test_host_refit_meets_yardstick(lib, case):
    """The host twin is within 1/16 of one inlier's effect of the exact fit (condition A of refit_cases) and no further from it than
    numpy's float64 lstsq (condition B); and, as before, no further from lstsq's solution than the reference's float32 refit is.

    Condition B is what the corrected step of csrc/rwh_refit.h is for.  On "clustered M=300 top bits" -- the 4 correspondences
    63, 127, 191, 255 of the 8K strip, cond of A 6.5e+11, of the equilibrated A 1.3e+05 -- the normal equations alone are
    6.6e-05 px from the exact fit and lstsq 1.4e-06 px; trace(G^-1) is 3.8e+09 there, above the step's threshold of 2^27, and
    with the step the twin is at 2.3e-11 px.  Every other case lies below the threshold (3.4e+06 at most, "clustered M=300
    ends") and keeps the first solution; the 4- and 5-point subsets keep B by the least (a factor 2.3 at "synthetic M=512
    ends", 9.6 at "synthetic M=257 top bits")."""
    u, v, bits = _case(case)
    H_ls, dev_ref = rc.yardstick(u, v, bits)
    H, st = rc.host_refit(lib, u, v, rc.pack(bits))
    assert st == rc.OK and np.isfinite(H).all() and H[2, 2] == 1.0
    assert rc.deviation(H, H_ls, u) <= dev_ref
    rc.hold("host-twin", case, H, u, v, bits)


def test_corrected_step_walks_every_trip(lib):
    """refit_cases.patch(): 700 correspondences whose trace(G^-1) is 128 times and more above the threshold of the corrected
    step, so the second pass over the correspondences is certainly made, through three trips of the stride loop.  A residual
    lost there moves the correction by that inlier's effect, so conditions A and B see it.  And of the cases of
    test_host_refit_meets_yardstick exactly one is above the threshold."""
    u, v = rc.patch()
    for family in rc.PATCH_FAMILIES:
        bits = rc.FAMILIES[family](len(u))
        assert rc.inverse_trace(u, v, bits) >= 2.0 ** 34
        H, st = rc.host_refit(lib, u, v, rc.pack(bits))
        assert st == rc.OK and H[2, 2] == 1.0
        rc.hold("host-twin", "patch M=700 %s" % family, H, u, v, bits)
    above = [c for c in CASES if rc.inverse_trace(*_case(c)) >= 2.0 ** 27]
    assert above == ["clustered M=300 top bits"]


def test_bits_beyond_m_are_ignored(lib):
    """Bits at or past M -- the rest of the last word and every later word of a mask row -- do not enter: the same H and status,
    bit for bit, as with the clean mask, for every problem of the launch."""
    for name in rc.PROBLEMS:
        u, v = rc.problem(name)
        m = len(u)
        bits = rc.family_bits(name, "random half")
        clean, dirty = rc.pack(bits, rc.MASK_WORDS), rc.dirty(bits)
        assert (dirty != clean).sum() == rc.MASK_WORDS - m // 64
        H0, s0 = rc.host_refit(lib, u, v, clean)
        H1, s1 = rc.host_refit(lib, u, v, dirty)
        assert s0 == s1 == (rc.OK if m >= 4 else rc.FEW) and np.array_equal(H0, H1, equal_nan=True)


def test_random_masks_select_the_subset(lib):
    """The mask selects: over a random half of every synthetic size the fit is that subset's least-squares fit.  A fit that lost
    one of the subset's points lies at least `resolution` from the exact fit of the subset (refit_cases, condition A); the twin
    is held to 1/16 of that, so one dropped point -- a lost tail, a lost lane, a misread word -- fails here."""
    for m in rc.SYNTHETIC_SIZES[1:]:
        u, v = rc.problem("synthetic M=%d" % m)
        bits = rc.family_bits("synthetic M=%d" % m, "random half")
        H_ls, dev_ref = rc.yardstick(u, v, bits)
        H, st = rc.host_refit(lib, u, v, rc.pack(bits))
        assert st == rc.OK
        assert rc.deviation(H, H_ls, u) <= dev_ref
        rc.hold("host-twin", "synthetic M=%d random half (subset)" % m, H, u, v, bits)
        if bits.sum() >= 6:
            H_x, _, res = rc.reference(u, v, bits)
            for j in np.flatnonzero(bits)[[0, -1]]:        # the claim itself, on the twin: drop one point and A fails
                less = bits.copy()
                less[j] = False
                H_less, st = rc.host_refit(lib, u, v, rc.pack(less))
                assert st == rc.OK and rc.deviation(H_less, H_x, u) > res / 2


def test_non_finite_coordinates(lib):
    """A NaN or an infinity in a correspondence whose bit is clear leaves every bit of the result as it is with a finite value
    there; in an inlier it makes a moment non-finite, which fails the solve's `diagonal > 0 and finite` test: SINGULAR, H NaN."""
    name = "synthetic M=257"
    u, v = rc.problem(name)
    bits = rc.family_bits(name, "random half")
    words = rc.pack(bits)
    H0, s0 = rc.host_refit(lib, u, v, words)
    assert s0 == rc.OK
    for k, poison in enumerate(rc.POISONS):
        for at, want in ((np.flatnonzero(~bits), (H0, rc.OK)), (np.flatnonzero(bits), (np.full((3, 3), np.nan), rc.SINGULAR))):
            for i in (at[k], at[-1 - k]):
                H, st = rc.host_refit(lib, *rc.poisoned(u, v, i, poison), words)
                assert st == want[1] and np.array_equal(H, want[0], equal_nan=True), (poison, i)


def test_rank_deficient_inlier_sets(lib):
    """All inliers on one line, and 4 inliers of which two are equal: A^T A is singular in exact arithmetic.  The call returns,
    and H is NaN exactly when the status is not OK."""
    for name, u, v in rc.rank_deficient():
        H, st = rc.host_refit(lib, u, v, rc.pack(np.ones(len(u), dtype=bool)))
        assert st in (rc.OK, rc.SINGULAR), name
        assert np.isnan(H).all() if st != rc.OK else np.isfinite(H).all() and H[2, 2] == 1.0


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
