"""The camera rule (include/rwh.h) without a GPU: the host twin of rwh_camera_blocks against the numpy restatement of
tests/camera_cases.py bit for bit, the Jacobian against the exact derivative in rationals within the derived rounding bound, the
host step against a numpy assembly and solve, the Levenberg-Marquardt loop of `sequence_adjust_cameras(on="host")` against an
independent optimiser and the focal length it recovers, the conversions between maps and cameras, and every refusal."""
import inspect
from fractions import Fraction

import numpy as np
import pytest

import bundle_cases as bc
import camera_cases as cc
import sequence_cases as sc

# The reference optimiser's stopping resolution, relative to the cost.  It differentiates forward with a relative step of 1e-7, so
# its gradient is wrong by about 1e-7 of itself and the point it converges to misses the minimum by that much of a step; the cost
# there exceeds the minimum by the square of it, 1e-14, and it stops on a gain below 1e-15 of the cost.  1e-9 leaves five orders
# over that and is seven under the 0.17 % between the cost at the ground truth (2412.905) and the minimum (2408.896).
REL = 1e-9
FOCALS = {"shared": cc.SHARED, "per-image": cc.PER_IMAGE}


@pytest.fixture(scope="module")
def lib():
    return sc.library()


@pytest.fixture(scope="module")
def sized():
    c = cc.size_list_case()
    c["cache"] = {}
    return c


@pytest.fixture(scope="module")
def grid():
    scene, shapes, Rs, f = cc.grid_cameras()
    return dict(scene, shapes=shapes, Rs=Rs, f=f)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def hblocks(lib, *a):
    st, blocks, count, status = cc.host_blocks(lib, *a)
    assert st == 0
    return blocks, count, status


# ---- 1. the host twin is the restatement ----
@pytest.mark.parametrize("which", ["ones", "random", "short", "zero row"])
def test_host_twin_is_the_restatement_bit_for_bit(lib, sized, which):
    """13 edges over 5 turning cameras with focal lengths that differ, the sizes 0 .. 600 that cross the mask word (64), the
    staged chunk (128) and the four partials; "short" has one mask word fewer than the longest edge needs, "zero row" clears the
    whole mask row of edge 11 (257 rows)."""
    c = sized
    sets = bc.mask_sets(c["sizes"])
    masks = sets["random"].copy() if which == "zero row" else sets[which]
    if which == "zero row":
        masks[11] = 0
    want, want_count, want_status = cc.restate(c["pa"], c["pb"], c["offsets"], masks, c["rec"], c["cache"])
    blocks, count, status = hblocks(lib, c["pa"], c["pb"], c["offsets"], masks, c["rec"])
    assert same_bits(blocks, want), "entries that differ: %s" % (np.argwhere(blocks != want)[:8].tolist(),)
    assert np.array_equal(count, want_count) and np.array_equal(status, want_status) and not status.any()
    assert count[0] == 0 and not blocks[0].any()                                    # the edge without rows
    if which == "ones":
        assert count.tolist() == c["sizes"]
    if which == "short":
        assert count[12] <= 64 * masks.shape[1] < c["sizes"][12]
    if which == "zero row":
        assert count[11] == 0 and not blocks[11].any() and count[10] > 0


def test_kernels_entry_is_the_twin(lib, sized):
    from ransac_with_homography_amd import kernels
    c = sized
    masks = bc.mask_sets(c["sizes"])["random"]
    got = kernels.host_camera_blocks(c["pa"], c["pb"], c["offsets"], masks, c["rec"])
    want = hblocks(lib, c["pa"], c["pb"], c["offsets"], masks, c["rec"])
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_behind_is_reported_and_isolated(lib):
    """Row 70 of edge 1 has v2 < 0: BEHIND on that edge alone, 128 of its 129 rows counted, the bits of the run with that row's
    mask bit cleared, the other edges untouched, and the twin is the restatement."""
    c, pa, rec, masks, cleared = cc.behind_case()
    assert cc.row_values(rec[1], pa[c["offsets"][1] + 70], c["pb"][c["offsets"][1] + 70]) is None
    blocks, count, status = hblocks(lib, pa, c["pb"], c["offsets"], masks, rec)
    assert status.tolist() == [cc.OK, cc.BEHIND, cc.OK] and count.tolist() == [65, 128, 5] and np.isfinite(blocks).all()
    blocks2, count2, status2 = hblocks(lib, pa, c["pb"], c["offsets"], cleared, rec)
    assert status2.tolist() == [cc.OK, cc.OK, cc.OK] and same_bits(blocks, blocks2)
    plain, _, _ = hblocks(lib, c["pa"], c["pb"], c["offsets"], masks, c["rec"])
    assert same_bits(blocks[[0, 2]], plain[[0, 2]])
    want, want_count, want_status = cc.restate(pa, c["pb"], c["offsets"], masks, rec)
    assert same_bits(blocks, want) and np.array_equal(count, want_count) and np.array_equal(status, want_status)


def test_blocks_refuse_bad_arguments(lib, sized):
    c = sized
    masks = bc.mask_sets(c["sizes"])["ones"]
    good = [np.ascontiguousarray(c["pa"]), np.ascontiguousarray(c["pb"]), c["offsets"], 13, masks, masks.shape[1], np.ascontiguousarray(c["rec"]),
            np.empty((13, cc.BLOCK)), np.empty(13, dtype=np.int32), np.empty(13, dtype=np.int32)]

    def call(args):
        return lib.rwh_host_camera_blocks(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args])
    assert call(good) == 0
    for at in (0, 1, 2, 4, 6, 7, 8, 9):
        assert call(good[:at] + [None] + good[at + 1:]) == -1
    for at, value in ((3, 0), (3, 2017), (5, 0), (5, -1)):
        assert call(good[:at] + [value] + good[at + 1:]) == -1
    # the device call refuses the same before any launch: no GPU is touched by these
    for at in (0, 1, 2, 4, 6, 7, 8, 9):
        assert call_device(lib, good, at, None) == -1
    for at, value in ((3, 0), (3, 2017), (5, 0)):
        assert call_device(lib, good, at, value) == -1


def call_device(lib, good, at, value):
    args = good[:at] + [value] + good[at + 1:]
    return lib.rwh_camera_blocks(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args], None)


# ---- 2. the Jacobian ----
def test_jacobian_lies_within_the_forward_bound_of_the_exact_derivative(lib):
    """20 random (record, a, b): the residual under the local update is a rational function of (omega, phi); its derivative by a
    central difference with h = 1e-30 in exact rationals is the rule's formula (to the difference's own truncation, h^2 times a
    third derivative: far below 1e-40), and every J entry the twin computes lies within the forward rounding bound of the stated
    operation sequence, propagated from the operands (camera_cases.jacobian_bound; no free constant)."""
    rng = np.random.default_rng(78)
    i0, j0, i1, j1 = cc.entries()
    worst = 0.0
    for case in range(20):
        shapes, Rs, fs = cc.random_cameras(3, 100 + case, yaw=0.25)
        s, d = [(1, 0), (2, 0), (0, 2), (2, 1)][case % 4]
        rec = cc.records(shapes, Rs, fs, [(s, d)])[0]
        a = (rng.uniform(0, 1, 2) * [160.0, 120.0]).astype(np.float32)
        b = (bc.project(cc.transfer(shapes, Rs, fs, s, d), a[None])[0] + rng.normal(0, 0.5, 2)).astype(np.float32)
        blocks, count, status = hblocks(lib, a[None], b[None], np.array([0, 1], dtype=np.int32), np.array([[1]], dtype=np.int64), rec[None])
        assert count[0] == 1 and status[0] == cc.OK
        # one row: S = J^T J, g = J^T r, c = r.r -- the twin's J is read back through the restatement, which equals it bit for bit
        row = cc.row_values(rec, a, b)
        assert same_bits(blocks[0], (row[i0] * row[j0] + row[i1] * row[j1]) + 0.0)
        exact, bound = cc.jacobian_bound(rec, a)
        central = cc.exact_jacobian(rec, a, b)
        for r in range(2):
            for k in range(8):
                assert abs(central[r][k] - exact[r][k]) < Fraction(1, 10 ** 40), (case, r, k)
                err = abs(Fraction(float(row[8 * r + k])) - exact[r][k])
                assert err <= bound[r][k], (case, r, k, float(err), float(bound[r][k]))
                assert bound[r][k] <= Fraction(1, 10 ** 10)       # the bound itself says something: J entries are of order 1 .. 300
                worst = max(worst, float(err / bound[r][k]) if bound[r][k] else 0.0)
    print("largest error over its bound: %.3f" % worst)


# ---- 3. the step ----
@pytest.fixture(scope="module")
def grid_blocks(lib, grid):
    pa, pb, offsets = bc.concatenated(grid["matches"])
    n = grid["n"]
    rec = cc.records(grid["shapes"], grid["Rs"], np.full(n, grid["f"]), grid["pairs"])
    blocks, _, status = hblocks(lib, pa, pb, offsets, bc.mask_sets(grid["sizes"])["ones"], rec)
    assert not status.any()
    return blocks


def check_step(lib, n, anchor, focals, pairs, blocks, lam):
    st, delta, step_status = cc.host_step(lib, n, anchor, focals, pairs, blocks, lam)
    assert st == 0 and step_status == cc.OK
    assert (delta[anchor, :3] == 0.0).all() and delta.any()
    A, g, slot = cc.assemble(n, anchor, focals, pairs, blocks, lam)
    flat = delta.reshape(-1)
    for members in slot:
        assert all(flat[i] == flat[members[0]] for i in members)       # with one focal for all, every phi slot holds one value
    x = np.array([flat[members[0]] for members in slot])
    ref = np.linalg.solve(A, -g)
    bound = bc.solve_bound(A, x)
    assert np.abs(A @ x + g).max() <= bound
    assert np.abs(A @ (x - ref)).max() <= bound + bc.solve_bound(A, ref)
    return delta


@pytest.mark.parametrize("focals", ["shared", "per-image"])
def test_step_solves_the_assembled_system(lib, grid, grid_blocks, focals):
    """rwh_host_camera_step against a numpy assembly over 4 n parameters reduced by a 0/1 matrix (the anchor's omega dropped, with
    one focal for all every phi summed into one unknown, so S[3][7] of an edge reaches that diagonal entry twice) and
    numpy.linalg.solve, within the backward-error bound of a Cholesky solve (bundle_cases.solve_bound); anchors 0, 5 and 7."""
    for anchor, lam in [(0, 1e-3), (5, 0.0), (7, 10.0)]:
        delta = check_step(lib, grid["n"], anchor, FOCALS[focals], grid["pairs"], grid_blocks, lam)
        assert delta.shape == (8, 4)
        if focals == "shared":
            assert (delta[:, 3] == delta[0, 3]).all() and delta[0, 3] != 0.0
        else:
            assert len(set(delta[:, 3].tolist())) == 8                  # the anchor's focal moves too


@pytest.mark.parametrize("focals", ["shared", "per-image"])
@pytest.mark.parametrize("anchor", [0, 1])
def test_step_on_a_two_image_graph(lib, grid, grid_blocks, focals, anchor):
    e = grid["pairs"].index((1, 0))
    check_step(lib, 2, anchor, FOCALS[focals], [(1, 0)], grid_blocks[e:e + 1], 1e-3)


def test_step_reports_an_untouched_image_and_refuses_bad_arguments(lib, grid, grid_blocks):
    blocks, pairs = grid_blocks, grid["pairs"]
    for focals in (cc.SHARED, cc.PER_IMAGE):
        st, delta, step_status = cc.host_step(lib, grid["n"] + 1, 0, focals, pairs, blocks, 1e-3)      # image 8: no edge touches it
        assert st == 0 and step_status == cc.SINGULAR and not delta.any()
        st, delta, step_status = cc.host_step(lib, grid["n"], 0, focals, pairs, np.zeros_like(blocks), 1e-3)
        assert st == 0 and step_status == cc.SINGULAR and not delta.any()
    assert cc.host_step(lib, 1, 0, cc.SHARED, [(0, 0)], blocks[:1], 1e-3)[0] == -1
    for n, anchor, focals, prs, lam in [(0, 0, 0, pairs, 1e-3), (65, 0, 0, pairs, 1e-3), (8, 8, 0, pairs, 1e-3), (8, -1, 0, pairs, 1e-3),
                                        (8, 0, 0, [(1, 8)], 1e-3), (8, 0, 0, [(-1, 2)], 1e-3), (8, 0, 0, [(2, 2)], 1e-3), (8, 0, 0, pairs, -1.0),
                                        (8, 0, 0, pairs, np.nan), (8, 0, 0, pairs, np.inf), (8, 0, 2, pairs, 1e-3), (8, 0, -1, pairs, 1e-3)]:
        assert cc.host_step(lib, n, anchor, focals, prs, blocks[:len(prs)], lam)[0] == -1, (n, anchor, focals, prs, lam)
    edges = np.ascontiguousarray(pairs, dtype=np.int32)
    out, status = np.zeros(32), np.zeros(1, dtype=np.int32)
    good = [8, 0, 0, edges.ctypes.data, len(pairs), blocks.ctypes.data, 1e-3, out.ctypes.data, status.ctypes.data]
    assert lib.rwh_host_camera_step(*good) == 0
    for at in (3, 5, 7, 8):
        assert lib.rwh_host_camera_step(*(good[:at] + [None] + good[at + 1:])) == -1
    for n_edges in (0, 2017):
        assert lib.rwh_host_camera_step(*(good[:4] + [n_edges] + good[5:])) == -1


# ---- 4. the loop ----
def traced(grid, Rs, fs, spoil=None, singular_at=None, **kw):
    """sequence_adjust_cameras(on="host") with kernels.host_camera_step wrapped -> (Rs, fs, info, steps): steps lists (lambda, the
    blocks the step was given) of every step tried; spoil(k, delta) may replace what call k returns, singular_at makes call k
    report RWH_BUNDLE_SINGULAR."""
    import homography as hg
    from ransac_with_homography_amd import kernels
    steps, info, real = [], {}, kernels.host_camera_step

    def step(n, anchor, edges, blocks, lam, focals="shared"):
        assert len(steps) < 200, "the loop does not end"
        delta, st = real(n, anchor, edges, blocks, lam, focals)
        if spoil is not None:
            delta = spoil(len(steps), delta)
        if singular_at == len(steps):
            delta, st = np.zeros_like(delta), cc.SINGULAR
        steps.append((float(lam), np.array(blocks, copy=True)))
        return delta, st

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(kernels, "host_camera_step", step)
        Rs, fs = hg.sequence_adjust_cameras(grid["shapes"], Rs, fs, grid["pairs"], grid["matches"], on="host", info=info, **kw)
    return Rs, fs, info, steps


@pytest.fixture(scope="module")
def outcomes(grid):
    """(focals, starting focal) -> the loop's run and the reference optimiser's from the same start, made once."""
    import homography as hg
    done = {}

    def run(focals, f0):
        if (focals, f0) not in done:
            Rs0, fs0 = hg.sequence_cameras(grid["shapes"], grid["Gs"], f0)
            Rs, fs, info, steps = traced(grid, Rs0, fs0, focals=focals)
            ref = cc.reference_optimum(grid["shapes"], Rs0, fs0, grid["pairs"], grid["matches"], 0, FOCALS[focals])
            done[(focals, f0)] = dict(Rs=Rs, fs=fs, info=info, steps=steps, ref=ref, start=(Rs0, fs0),
                                      cost=cc.reference_cost(grid["shapes"], Rs, fs, grid["pairs"], grid["matches"]))
        return done[(focals, f0)]
    return run


@pytest.mark.parametrize("f0", [120.0, 190.0])
@pytest.mark.parametrize("focals", ["shared", "per-image"])
def test_loop_ends_at_the_reference_optimum_and_recovers_the_focal(grid, outcomes, focals, f0):
    """GRID (8 views, true focal 150, 25 pairs, 4881 correspondences, 0.5 px noise) from `sequence_cameras` of the true maps with
    focal 120 and with 190 -- a focal 20 % and 27 % wrong, and rotations that are the nearest ones to maps that are none.

    Cost: the geometry's cost at what the loop returns does not exceed the reference optimiser's by more than REL of it (that
    optimiser's stopping resolution, stated at the top).  Where this was written: 2408.8960437058 (shared) and 2406.7452447245
    (per image) on both sides from both starts, gaps between -4e-16 and 6e-16, 5 accepted steps each.

    Focal: every recovered focal lies within 4 standard errors of 150, the standard error from the REFERENCE's normal matrix,
    sqrt(cost / (rows - unknowns) * inv(J^T J)_ff).  The reference alone, from the starts used here: 150.3525 +- 0.2173 shared,
    1.62 standard errors off, and 150.2458 .. 150.4654 +- 0.2200 .. 0.2233 per image, 2.09 at most (asserted below as well, so
    the yardstick is seen to hold the bound it sets); the loop's figures are the same to six digits."""
    run = outcomes(focals, f0)
    ref = run["ref"]
    gap = (run["cost"] - ref["cost"]) / ref["cost"]
    z_ref, z = np.abs(ref["fs"] - grid["f"]) / ref["se"], np.abs(run["fs"] - grid["f"]) / ref["se"]
    print("%s from %g: cost %.10f, reference %.10f, gap %.3e, %d accepted; focal %.4f .. %.4f, se %.4f .. %.4f, off by %.3f se (reference %.3f)"
          % (focals, f0, run["cost"], ref["cost"], gap, run["info"]["iters"], run["fs"].min(), run["fs"].max(), ref["se"].min(), ref["se"].max(),
             z.max(), z_ref.max()))
    assert gap <= REL
    assert gap >= -REL                                   # below the reference would be rows that went missing
    assert z_ref.max() < 4.0
    assert z.max() < 4.0 and run["fs"].shape == (8,)
    assert run["cost"] < run["info"]["cost"][0] * 0.01   # the start is far: the cost falls by more than two orders
    if focals == "shared":
        assert (run["fs"] == run["fs"][0]).all()
    else:
        assert len(set(run["fs"].tolist())) == 8
    # what comes back are rotations, the anchor's the identity; the worst rotation error against the truth is a few milliradians
    Rs = run["Rs"]
    assert np.array_equal(Rs[0], np.eye(3))
    assert np.abs(Rs @ Rs.transpose(0, 2, 1) - np.eye(3)).max() <= 16 * bc.U and np.allclose(np.linalg.det(Rs), 1.0, atol=16 * bc.U, rtol=0)
    angle = max(np.linalg.norm(cc.rotation_vector(Rt.T @ R)) for Rt, R in zip(grid["Rs"], Rs))
    print("largest rotation error %.5f rad" % angle)
    assert angle < 0.01


@pytest.mark.parametrize("focals", ["shared", "per-image"])
def test_reported_cost_is_the_cost_of_the_returned_cameras(grid, outcomes, focals):
    """info["cost"][-1] (the rule's sum) against the geometry's cost at the SAME cameras: the plain summation bound (2 rows + 64) u
    relative.  Both starts end at the same minimum (REL)."""
    a, b = outcomes(focals, 120.0), outcomes(focals, 190.0)
    for run in (a, b):
        info = run["info"]
        assert abs(info["cost"][-1] - run["cost"]) <= (2 * sum(grid["sizes"]) + 64) * bc.U * run["cost"]
        assert len(info["cost"]) == info["iters"] + 1 and all(y < x for x, y in zip(info["cost"], info["cost"][1:]))
        assert len(run["steps"]) == info["iters"]                              # no step was rejected on the way
        assert info["lambda"] == pytest.approx(1e-3 / 10.0 ** info["iters"], rel=1e-12)
    assert abs(a["cost"] - b["cost"]) <= REL * b["cost"]


def test_a_rejected_step_raises_lambda_and_keeps_the_blocks(grid, outcomes):
    """A stand-in: the first step's delta comes back multiplied by -40, which raises the cost.  The step is rejected: the next one
    runs at 10 lambda from the same blocks, and the run ends at the same minimum."""
    Rs0, fs0 = outcomes("shared", 120.0)["start"]

    def spoil(k, delta):
        return delta * -40.0 if k == 0 else delta
    Rs, fs, info, steps = traced(grid, Rs0, fs0, spoil=spoil)
    assert steps[0][0] == 1e-3 and steps[1][0] == 1e-3 * 10.0 and same_bits(steps[0][1], steps[1][1])
    assert len(steps) > info["iters"] >= 1 and not same_bits(steps[2][1], steps[1][1])
    cost = cc.reference_cost(grid["shapes"], Rs, fs, grid["pairs"], grid["matches"])
    assert abs(cost - outcomes("shared", 120.0)["cost"]) <= REL * cost
    # a focal that leaves (0, inf) is rejected as well, without raising
    def negative(k, delta):
        if k == 0:
            delta = delta.copy()
            delta[:, 3] = -1.5
        return delta
    Rs, fs, info, steps = traced(grid, Rs0, fs0, spoil=negative)
    assert steps[1][0] == 1e-3 * 10.0 and same_bits(steps[0][1], steps[1][1]) and (fs > 0).all()
    # a singular system raises on the first step tried and is a rejected step after it
    with pytest.raises(ValueError, match="singular"):
        traced(grid, Rs0, fs0, singular_at=0)
    Rs, fs, info, steps = traced(grid, Rs0, fs0, singular_at=1)
    assert steps[1][0] == 1e-3 / 10.0 and steps[2][0] == 1e-3 and same_bits(steps[1][1], steps[2][1])
    cost = cc.reference_cost(grid["shapes"], Rs, fs, grid["pairs"], grid["matches"])
    assert abs(cost - outcomes("shared", 120.0)["cost"]) <= REL * cost


def test_max_iters_gives_a_prefix(grid, outcomes):
    full = outcomes("shared", 120.0)
    Rs0, fs0 = full["start"]
    Rs, fs, info, steps = traced(grid, Rs0, fs0, max_iters=2)
    assert info["iters"] == 2 and info["cost"] == full["info"]["cost"][:3] and info["lambda"] == 1e-3 / 10.0 / 10.0
    Rs, fs, info, steps = traced(grid, Rs0, fs0, max_iters=0)
    assert info["iters"] == 0 and info["cost"] == full["info"]["cost"][:1] and not steps and info["lambda"] == 1e-3
    assert same_bits(Rs, Rs0) and same_bits(fs, fs0)


def test_masks_and_anchor(grid):
    """The "random" masks, and the same rows with two words of ones behind them: the same bits out; anchor 5 ends at the minimum
    of anchor 0 (the cost does not depend on the frame)."""
    import homography as hg
    masks = bc.mask_sets(grid["sizes"])["random"]
    wide = np.concatenate([masks, np.full((len(masks), 2), -1, dtype=np.int64)], axis=1)
    Rs0, fs0 = hg.sequence_cameras(grid["shapes"], grid["Gs"], 150.0)
    a_info, b_info = {}, {}
    a = hg.sequence_adjust_cameras(grid["shapes"], Rs0, fs0, grid["pairs"], grid["matches"], masks=masks, on="host", info=a_info)
    b = hg.sequence_adjust_cameras(grid["shapes"], Rs0, fs0, grid["pairs"], grid["matches"], masks=wide.view(np.uint64), on="host", info=b_info)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a_info == b_info and a_info["iters"] >= 1
    cost = bc.reference_cost(cc.maps(grid["shapes"], a[0], a[1]), grid["pairs"], grid["matches"], masks)
    assert abs(a_info["cost"][-1] - cost) <= (2 * sum(grid["sizes"]) + 64) * bc.U * cost
    G5 = bc.reframed(grid["Gs"], 5)
    R5, f5 = hg.sequence_cameras(grid["shapes"], G5, 150.0, anchor=5)
    info0, info5 = {}, {}
    hg.sequence_adjust_cameras(grid["shapes"], Rs0, fs0, grid["pairs"], grid["matches"], on="host", info=info0)
    R5, f5 = hg.sequence_adjust_cameras(grid["shapes"], R5, f5, grid["pairs"], grid["matches"], anchor=5, on="host", info=info5)
    assert np.array_equal(R5[5], np.eye(3)) and abs(info5["cost"][-1] - info0["cost"][-1]) <= REL * info0["cost"][-1]


# ---- 5. the conversions ----
@pytest.mark.parametrize("anchor", [0, 5])
def test_cameras_and_maps_are_inverse_conversions(grid, anchor):
    """With the true focal, `sequence_cameras` of the GRID maps gives the true rotations to rounding, and `sequence_camera_maps` of
    those the maps up to scale.  1e-13: K and its inverse carry the factor f = 150 in and out, three 3 x 3 products and an SVD,
    each a few u of entries of order 1 after it -- 150 * 16 u = 2.7e-13 would be the coarse figure, 2.4e-16 and 6e-14 were seen."""
    import homography as hg
    Gs = bc.reframed(grid["Gs"], anchor)
    true = np.stack([grid["Rs"][anchor].T @ R for R in grid["Rs"]])
    Rs, fs = hg.sequence_cameras(grid["shapes"], Gs, grid["f"], anchor=anchor)
    assert (fs == grid["f"]).all() and np.array_equal(Rs[anchor], np.eye(3))
    print("rotations within %.2e" % np.abs(Rs - true).max())
    assert np.abs(Rs - true).max() <= 1e-13
    back = hg.sequence_camera_maps(grid["shapes"], Rs, fs, anchor=anchor)
    assert np.array_equal(back[anchor], np.eye(3))
    for G, B in zip(Gs, back):
        assert np.abs(B / B[2, 2] - G / G[2, 2]).max() <= 1e-13 * np.abs(G / G[2, 2]).max()
    assert same_bits(back, cc.maps(grid["shapes"], Rs, fs, anchor))              # the same three products, written twice


def test_cameras_of_flipped_maps(grid):
    """A map with a negative determinant (the same map, scaled by -1) gives the same rotation: the sign is taken out first."""
    import homography as hg
    Gs = grid["Gs"].copy()
    Gs[3] = -Gs[3]
    Rs, _ = hg.sequence_cameras(grid["shapes"], Gs, grid["f"])
    assert np.abs(Rs - grid["Rs"]).max() <= 1e-13


# ---- 6. refusals and surface ----
def test_value_errors_without_a_gpu(grid):
    import homography as hg
    shapes, Gs, pairs, matches = grid["shapes"], grid["Gs"], grid["pairs"], grid["matches"]
    Rs, fs = hg.sequence_cameras(shapes, Gs, 150.0)
    singular = Gs.copy()
    singular[2] = np.ones((3, 3))
    nan = Gs.copy()
    nan[2, 0, 0] = np.nan
    for args, kw in [((shapes, Gs, 0.0), {}), ((shapes, Gs, -3.0), {}), ((shapes, Gs, np.nan), {}), ((shapes, Gs, np.inf), {}),
                     ((shapes, Gs, "auto"), {}), ((shapes, Gs, None), {}), ((shapes, Gs, True), {}), ((shapes, Gs, 150.0), dict(anchor=8)),
                     ((shapes, Gs, 150.0), dict(anchor=-1)), (([], [], 150.0), {}), (([(4, 4)] * 65, [np.eye(3)] * 65, 150.0), {}),
                     ((shapes, singular, 150.0), {}), ((shapes, nan, 150.0), {}), ((shapes, Gs[:7], 150.0), {})]:
        with pytest.raises(ValueError):
            hg.sequence_cameras(*args, **kw)
    turned = Rs.copy()
    turned[0] = Rs[1]
    for bad_Rs, bad_fs, kw in [(turned, fs, {}), (Rs[:7], fs, {}), (Rs, fs[:7], {}), (Rs, np.append(fs[:7], 0.0), {}), (Rs, np.append(fs[:7], np.nan), {}),
                               (Rs, -fs, {}), (Rs, fs, dict(anchor=8))]:
        with pytest.raises(ValueError):
            hg.sequence_camera_maps(shapes, bad_Rs, bad_fs, **kw)
        with pytest.raises(ValueError):
            hg.sequence_adjust_cameras(shapes, bad_Rs, bad_fs, pairs, matches, on="host", **kw)
    uneven = fs.copy()
    uneven[3] = 151.0
    short_masks = np.full((len(pairs) - 1, 7), -1, dtype=np.int64)
    for kw in [dict(on="gpu"), dict(focals="each"), dict(focals=1), dict(max_iters=-1), dict(max_iters=2.5), dict(max_iters=True), dict(pairs=[]),
               dict(pairs=[(1, 1)]), dict(pairs=[(1, 8)]), dict(matches=matches[:-1]), dict(masks=short_masks),
               dict(masks=np.ones((len(pairs), 7), dtype=np.float64)), dict(fs=uneven)]:
        kw = dict(dict(pairs=pairs, matches=matches, fs=fs, on="host"), **kw)
        with pytest.raises(ValueError):
            hg.sequence_adjust_cameras(shapes, Rs, kw.pop("fs"), kw.pop("pairs"), kw.pop("matches"), **kw)
    per = hg.sequence_adjust_cameras(shapes, Rs, uneven, pairs, matches, focals="per-image", on="host", max_iters=1)   # unequal focals: fine per image
    assert per[1].shape == (8,)
    with pytest.raises(ValueError, match="no edge with inliers touches|singular"):
        hg.sequence_adjust_cameras(shapes + [shapes[0]], np.concatenate([Rs, np.eye(3)[None]]), np.append(fs, 150.0), pairs, matches, on="host")
    behind = Rs.copy()
    behind[1] = cc.rodrigues(np.array([0.0, 2.5, 0.0]))
    with pytest.raises(ValueError, match=r"pair \d+ \(images \d and \d\) has an inlier behind the camera at the start"):
        hg.sequence_adjust_cameras(shapes, behind, fs, pairs, matches, on="host")
    spoiled = [(a, b.copy()) for a, b in matches]
    spoiled[6][1][17, 1] = np.nan
    with pytest.raises(ValueError, match=r"pair 6 \(images %d and %d\) has a cost that is not finite" % pairs[6]):
        hg.sequence_adjust_cameras(shapes, Rs, fs, pairs, spoiled, on="host")


def test_stitch_sequence_takes_the_new_adjust_values_before_any_gpu_work():
    """The argument check comes before anything else: with adjust="cameras" the call gets past it and fails on the NEXT check (an
    unknown projection, also made before the GPU is asked for), where adjust="yes" fails on its own.  The signature is the one it
    was."""
    import ransac as rs
    imgs = [np.zeros((40, 40, 3), dtype=np.uint8)] * 2
    for value in ("yes", 1, None, "Cameras", "cameras-shared", ["cameras"]):
        with pytest.raises(ValueError, match="adjust="):
            rs.stitch_sequence(imgs, adjust=value, projection="fisheye", focal=100.0)
    for value in ("cameras", "cameras-per-image", True, False):
        with pytest.raises(ValueError, match="projection="):
            rs.stitch_sequence(imgs, adjust=value, projection="fisheye", focal=100.0)
    for focal in (0.0, -1.0, np.nan, "wide", True):
        with pytest.raises(ValueError, match="focal="):
            rs.stitch_sequence(imgs, adjust="cameras", focal=focal)
    with pytest.raises(ValueError, match="focal=100.0 without a projection"):
        rs.stitch_sequence(imgs, adjust=True, focal=100.0)                       # as it was
    assert list(inspect.signature(rs.stitch_sequence).parameters) == [
        "images", "anchor", "th", "d", "k", "ransacMet", "seed", "blending", "features", "info", "gains", "projection", "focal", "pairs", "adjust",
        "bands"]


def test_new_names_are_exported(lib):
    import homography as hg
    from ransac_with_homography_amd import _lib, homography, kernels
    for name in ("sequence_cameras", "sequence_camera_maps", "sequence_adjust_cameras"):
        assert name in homography.__all__ and getattr(hg, name) is getattr(homography, name)
    for name in ("rwh_camera_blocks", "rwh_host_camera_blocks", "rwh_host_camera_step"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for name in ("camera_blocks", "camera_split", "host_camera_blocks", "host_camera_step"):
        assert callable(getattr(kernels, name))
    assert (kernels.CAMERA_BLOCK, kernels.CAMERA_RECORD) == (45, 15) == (cc.BLOCK, cc.RECORD)
    hdr = open(sc.__file__.replace("tests/sequence_cases.py", "include/rwh.h")).read()
    assert "#define RWH_CAMERA_BLOCK 45" in hdr and "#define RWH_CAMERA_RECORD 15" in hdr and "The camera rule." in hdr
