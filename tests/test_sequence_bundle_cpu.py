"""The bundle rule without a GPU: the host twin of the edge blocks against the numpy restatement of tests/bundle_cases.py (bit for
bit), its Jacobian against exact rationals, the damped step against a numpy assembly and solve, `sequence_adjust(on="host")` on the
GRID scene, `sequence_graph`, and every refusal at the Python level."""
import inspect
from fractions import Fraction

import numpy as np
import pytest

import bundle_cases as bc
import projection_cases as pc
import sequence_cases as sc


@pytest.fixture(scope="module")
def lib():
    return sc.library()


@pytest.fixture(scope="module")
def sized():
    return bc.size_list_case()


@pytest.fixture(scope="module")
def grid():
    return bc.grid_scene()


def hblocks(lib, *a):
    st, blocks, count, status = bc.host_blocks(lib, *a)
    assert st == 0
    return blocks, count, status


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---- 1. the twin is the restatement ----
@pytest.mark.parametrize("which", ["ones", "random", "short"])
def test_twin_is_the_restatement_bit_for_bit(lib, sized, which):
    """One call over the 13 edge sizes that cross the mask word, the staged chunk and the partials."""
    c = sized
    masks = bc.mask_sets(c["sizes"])[which]
    blocks, count, status = hblocks(lib, c["pa"], c["pb"], c["offsets"], masks, c["T"])
    want, want_count, want_status = bc.restate(c["pa"], c["pb"], c["offsets"], masks, c["T"])
    assert same_bits(blocks, want)
    assert np.array_equal(count, want_count) and np.array_equal(status, want_status) and not status.any()
    assert not blocks[0].any() and count[0] == 0                         # the edge without rows: a zero block, status OK
    if which == "ones":
        assert count.tolist() == c["sizes"]
    if which == "short":
        assert count[-1] <= 64 * masks.shape[1] < c["sizes"][-1]         # rows past the mask row are no inliers


def test_twin_through_the_package_is_the_same_call(lib, sized):
    from ransac_with_homography_amd import kernels
    c = sized
    masks = bc.mask_sets(c["sizes"])["random"]
    got = kernels.host_bundle_blocks(c["pa"], c["pb"], c["offsets"], masks, c["T"])
    want = hblocks(lib, c["pa"], c["pb"], c["offsets"], masks, c["T"])
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


# ---- 2. the Jacobian ----
def test_jacobian_lies_within_the_forward_bound_of_the_exact_derivative(lib):
    """20 random (T, a, b): the residual is a rational function of delta; its derivative by a central difference with h = 1e-30 in
    exact rationals is the rule's formula (to the difference's own truncation, h^2 times a third derivative: far below 1e-40), and
    every J entry the twin computes lies within the forward rounding bound of the stated operation sequence, computed from the
    operands (bundle_cases.jacobian_bound; no free constant).  Cases 0 .. 9 have T and a positive throughout, so p has no
    cancellation and the closed form gamma_15 (|dp| + |q| |dp2|) / |p2| holds as well."""
    rng = np.random.default_rng(77)
    i0, j0, i1, j1 = bc.entries()
    gamma15 = Fraction(15, 2 ** 53) / (1 - Fraction(15, 2 ** 53))
    for case in range(20):
        if case < 10:
            T = np.array([[1.0, 0.05, 20.0], [0.03, 1.0, 10.0], [2e-4, 1e-4, 1.0]]) * rng.uniform(0.5, 1.5, (3, 3))
        else:
            T = np.eye(3) + np.array([[0.2, 0.2, 60.0], [0.2, 0.2, 40.0], [8e-4, 8e-4, 0.1]]) * rng.uniform(-1, 1, (3, 3))
        T = T / np.abs(T).max()
        a = (rng.uniform(0, 1, 2) * [160.0, 120.0]).astype(np.float32)
        b = (bc.project(T, a[None])[0] + rng.normal(0, 0.5, 2)).astype(np.float32)
        blocks, count, status = hblocks(lib, a[None], b[None], np.array([0, 1], dtype=np.int32), np.array([[1]], dtype=np.int64), T[None])
        assert count[0] == 1 and status[0] == bc.OK
        # one row: S = J^T J, g = J^T r, c = r.r -- the twin's J is read back through the restatement, which equals it bit for bit
        row = bc.row_values(T, a, b)
        assert same_bits(blocks[0], (row[i0] * row[j0] + row[i1] * row[j1]) + 0.0)
        exact, bound = bc.jacobian_bound(T, a)
        central = bc.exact_jacobian(T, a, b)
        Tf = [[Fraction(float(v)) for v in r] for r in T]
        at = [Fraction(float(a[0])), Fraction(float(a[1])), Fraction(1)]
        p = [sum(Tf[i][k] * at[k] for k in range(3)) for i in range(3)]
        for r in range(2):
            for k in range(16):
                assert abs(central[r][k] - exact[r][k]) < Fraction(1, 10 ** 40), (case, r, k)
                err = abs(Fraction(float(row[16 * r + k])) - exact[r][k])
                assert err <= bound[r][k], (case, r, k, float(err), float(bound[r][k]))
                if case < 10:
                    rho, c = (k % 8) // 3, (k % 8) % 3
                    dp = [at[c] * Tf[i][rho] for i in range(3)] if k < 8 else [-p[c] if i == rho else 0 for i in range(3)]
                    closed = gamma15 * (abs(dp[r]) + abs(p[r] / p[2]) * abs(dp[2])) / abs(p[2])
                    assert err <= closed, (case, r, k, float(err), float(closed))


# ---- 3. exact zeros ----
def test_integer_translations_of_integer_points_leave_no_residual(lib):
    rng = np.random.default_rng(5)
    sizes = [7, 130, 64]
    shifts = [(12.0, -3.0), (-40.0, 25.0), (0.0, 0.0)]
    pa = rng.integers(0, 300, (sum(sizes), 2)).astype(np.float32)
    offsets = np.array([0, 7, 137, 201], dtype=np.int32)
    pb, T = pa.copy(), []
    for e, (tx, ty) in enumerate(shifts):
        pb[offsets[e]:offsets[e + 1]] += np.float32([tx, ty])
        T.append(np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]]))      # as it is: the library takes T as given
    blocks, count, status = hblocks(lib, pa, pb, offsets, bc.mask_sets(sizes)["ones"], np.stack(T))
    assert count.tolist() == sizes and not status.any()
    assert (blocks[:, bc.N_S:] == 0.0).all()                              # every g and c is exactly 0
    assert (blocks[:, :bc.N_S] != 0.0).any()


def test_power_of_two_scaled_translations_leave_no_residual(lib):
    """The transfer is divided by its largest entry: with a shift of 64 that is a power of two, and r stays exactly 0."""
    pa = np.arange(40, dtype=np.float32).reshape(20, 2)
    pb = pa + np.float32([64.0, -8.0])
    T = np.array([[1.0, 0.0, 64.0], [0.0, 1.0, -8.0], [0.0, 0.0, 1.0]]) / 64.0
    blocks, _, status = hblocks(lib, pa, pb, np.array([0, 20], dtype=np.int32), np.array([[-1]], dtype=np.int64), T[None])
    assert status[0] == bc.OK and (blocks[0, bc.N_S:] == 0.0).all()


# ---- 4. BEHIND ----
def test_behind_is_reported_and_isolated(lib):
    c, pa, T, masks, cleared = bc.behind_case()
    blocks, count, status = hblocks(lib, pa, c["pb"], c["offsets"], masks, T)
    assert status.tolist() == [bc.OK, bc.BEHIND, bc.OK] and count.tolist() == [65, 128, 5]
    blocks2, count2, status2 = hblocks(lib, pa, c["pb"], c["offsets"], cleared, T)
    assert status2.tolist() == [bc.OK, bc.OK, bc.OK] and count2.tolist() == [65, 128, 5]
    assert same_bits(blocks, blocks2)                                     # the invalid inlier contributed nothing
    plain, _, _ = hblocks(lib, c["pa"], c["pb"], c["offsets"], masks, c["T"])
    assert same_bits(blocks[[0, 2]], plain[[0, 2]])                       # the other edges keep every bit
    want, want_count, want_status = bc.restate(pa, c["pb"], c["offsets"], masks, T)
    assert same_bits(blocks, want) and np.array_equal(status, want_status) and np.array_equal(count, want_count)


def test_blocks_refuse_bad_arguments(lib):
    c = bc.size_list_case(sizes=[3, 4])
    masks = bc.mask_sets(c["sizes"])["ones"]
    out = np.zeros(2 * bc.BLOCK), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    args = [c["pa"].ctypes.data, c["pb"].ctypes.data, c["offsets"].ctypes.data, 2, masks.ctypes.data, 1, c["T"].ctypes.data,
            out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data]
    assert lib.rwh_host_bundle_blocks(*args) == 0
    for at, bad in [(0, None), (1, None), (2, None), (4, None), (6, None), (7, None), (8, None), (9, None), (3, 0), (3, 2017), (5, 0)]:
        spoiled = list(args)
        spoiled[at] = bad
        assert lib.rwh_host_bundle_blocks(*spoiled) == -1, (at, bad)
        assert lib.rwh_bundle_blocks(*(spoiled + [None])) == -1, (at, bad)   # refused before anything is launched: no GPU needed


# ---- 5. the step ----
def test_step_matches_a_numpy_assembly_and_solve(lib, grid):
    """delta against numpy.linalg.solve of the numpy assembly, each held to the backward-error bound of its own solve: the
    residual A x + g of either is below residual_bound, so the two differ by at most cond-scaled bounds -- compared in the
    residual, where the bound is computed from the operands."""
    pa, pb, offsets = bc.concatenated(grid["matches"])
    T = bc.transfers(grid["Gs"], grid["pairs"])
    blocks, _, status = hblocks(lib, pa, pb, offsets, bc.mask_sets(grid["sizes"])["ones"], T)
    assert not status.any()
    n = grid["n"]
    for anchor, lam in [(0, 1e-3), (5, 0.0), (7, 10.0)]:
        st, delta, step_status = bc.host_step(lib, n, anchor, grid["pairs"], blocks, lam)
        assert st == 0 and step_status == bc.OK
        assert (delta[anchor] == 0.0).all() and delta.any()
        A, g, keep = bc.assemble(n, anchor, grid["pairs"], blocks, lam)
        x = delta.reshape(-1)[keep]
        ref = np.linalg.solve(A, -g)
        bound = bc.solve_bound(A, x)
        assert np.abs(A @ x + g).max() <= bound
        assert np.abs(A @ (x - ref)).max() <= bound + bc.solve_bound(A, ref)


def test_step_reports_an_untouched_image_and_refuses_bad_arguments(lib, grid):
    pa, pb, offsets = bc.concatenated(grid["matches"])
    blocks, _, _ = hblocks(lib, pa, pb, offsets, bc.mask_sets(grid["sizes"])["ones"], bc.transfers(grid["Gs"], grid["pairs"]))
    st, delta, step_status = bc.host_step(lib, grid["n"] + 1, 0, grid["pairs"], blocks, 1e-3)      # image 8: no edge touches it
    assert st == 0 and step_status == bc.SINGULAR and not delta.any()
    zero = np.zeros_like(blocks)
    st, delta, step_status = bc.host_step(lib, grid["n"], 0, grid["pairs"], zero, 1e-3)            # edges without inliers
    assert st == 0 and step_status == bc.SINGULAR and not delta.any()
    st, delta, step_status = bc.host_step(lib, 1, 0, [(0, 0)], blocks[:1], 1e-3)
    assert st == -1
    for n, anchor, pairs, lam in [(0, 0, grid["pairs"], 1e-3), (65, 0, grid["pairs"], 1e-3), (8, 8, grid["pairs"], 1e-3), (8, -1, grid["pairs"], 1e-3),
                                  (8, 0, [(1, 8)], 1e-3), (8, 0, [(-1, 2)], 1e-3), (8, 0, [(2, 2)], 1e-3), (8, 0, grid["pairs"], -1.0),
                                  (8, 0, grid["pairs"], np.inf), (8, 0, grid["pairs"], np.nan)]:
        assert bc.host_step(lib, n, anchor, pairs, blocks[:len(pairs)], lam)[0] == -1, (n, anchor, pairs, lam)
    one = np.zeros((1, 8))
    status = np.zeros(1, dtype=np.int32)
    edges = np.array([[1, 0]], dtype=np.int32)
    for at in range(4):
        args = [edges.ctypes.data, blocks.ctypes.data, one.ctypes.data, status.ctypes.data]
        args[at] = None
        assert lib.rwh_host_bundle_step(1, 0, args[0], 1, args[1], 1e-3, args[2], args[3]) == -1


# ---- 6. the adjustment ----
def edge_rms(lib, grid, Gs, pair):
    e = grid["pairs"].index(pair)
    a, b = grid["matches"][e]
    blocks, count, _ = hblocks(lib, a, b, np.array([0, len(a)], dtype=np.int32), np.full((1, (len(a) + 63) // 64), -1, dtype=np.int64),
                               bc.transfers(Gs, [pair]))
    return float(np.sqrt(blocks[0, 152] / count[0]))


def test_adjust_on_host_closes_the_loop_of_the_grid(lib, grid):
    """GRID from the snake chain of pairwise least-squares homographies.  The four conditions are exact comparisons.  The scene
    has 25 pairs and 4881 correspondences; where this was written the cost went from 2521.8 (chain) to 2398.3 in 5 accepted steps,
    against 2412.9 at the ground truth, and the RMS of the loop-closing edge (4, 0) from 0.775 px to 0.708 px (truth 0.710 px).
    The figures are printed."""
    import homography as hg
    start = bc.snake_start(lib, grid)
    info, at_truth = {}, {}
    Gs = hg.sequence_adjust(start, grid["pairs"], grid["matches"], anchor=0, on="host", info=info)
    hg.sequence_adjust(grid["Gs"], grid["pairs"], grid["matches"], anchor=0, on="host", max_iters=0, info=at_truth)
    cost = info["cost"]
    print("GRID: %d pairs, %d rows; cost chain %.1f, truth %.1f, adjusted %.1f in %d steps; edge (4, 0) RMS %.3f px -> %.3f px (truth %.3f)"
          % (len(grid["pairs"]), sum(grid["sizes"]), cost[0], at_truth["cost"][0], cost[-1], info["iters"],
             edge_rms(lib, grid, start, (4, 0)), edge_rms(lib, grid, Gs, (4, 0)), edge_rms(lib, grid, grid["Gs"], (4, 0))))
    assert len(cost) == info["iters"] + 1 >= 2 and all(b < a for a, b in zip(cost, cost[1:]))     # strictly decreasing
    assert cost[-1] < cost[0]                                                                      # below the chain's
    assert cost[-1] <= at_truth["cost"][0]                                                         # the truth is a feasible point
    assert Gs.shape == (8, 3, 3) and Gs.dtype == np.float64 and np.array_equal(Gs[0], np.eye(3))
    assert at_truth["iters"] == 0 and len(at_truth["cost"]) == 1
    assert all(abs(np.abs(G).max() - 1.0) == 0.0 for G in Gs[1:])                                  # each divided by its largest entry


def test_adjust_takes_masks_and_leaves_an_edge_out(lib, grid):
    import homography as hg
    start = bc.snake_start(lib, grid)
    masks = bc.mask_sets(grid["sizes"])["ones"]
    all_in, info = {}, {}
    a = hg.sequence_adjust(start, grid["pairs"], grid["matches"], masks=masks, on="host", max_iters=2, info=all_in)
    b = hg.sequence_adjust(start, grid["pairs"], grid["matches"], on="host", max_iters=2)
    assert same_bits(a, b) and all_in["iters"] == 2
    e = grid["pairs"].index((4, 0))
    masks[e] = 0
    hg.sequence_adjust(start, grid["pairs"], grid["matches"], masks=masks.view(np.uint64), on="host", max_iters=1, info=info)
    assert info["cost"][0] < all_in["cost"][0]                          # the loop-closing edge no longer counts


# ---- 7. the graph ----
def test_graph_is_sequence_plan_on_adjacent_pairs():
    import homography as hg
    for n in (1, 2, 5):
        images, Hs = pc.sweep(n, 40 + n, f=300.0, yaw=0.1)
        shapes = [im.shape for im in images]
        want = hg.sequence_plan(shapes, Hs, anchor=0)[0]
        Gs, accepted, tree = hg.sequence_graph(n, [(i + 1, i) for i in range(n - 1)], Hs, [100] * (n - 1), [60] * (n - 1), anchor=0)
        assert same_bits(Gs, want) and accepted.all() and tree == [(i, i + 1, i) for i in range(n - 1)]


def test_graph_accepts_by_the_inlier_rule_and_grows_the_heaviest_tree():
    import homography as hg
    rng = np.random.default_rng(9)
    H = {pr: sc.homography(rng, 30.0 * (pr[0] - pr[1]), 2.0) for pr in [(1, 0), (2, 0), (2, 1), (3, 1), (3, 2), (0, 3)]}
    pairs = list(H)
    # 8 + 0.3 * 100 = 38: 38 inliers are not enough, 39 are
    Gs, accepted, tree = hg.sequence_graph(4, pairs, [H[p] for p in pairs], [100] * 6, [39, 38, 50, 50, 60, 45], anchor=0)
    assert accepted.tolist() == [True, False, True, True, True, True]
    # from 0: (1, 0) has 39, (0, 3) has 45 -> image 3 through inv(H); then (3, 2) with 60; then 1 by (2, 1) and (3, 1), both 50: the lower pair
    assert tree == [(0, 3, 5), (3, 2, 4), (2, 1, 2)]
    G3 = np.linalg.inv(H[(0, 3)])
    assert same_bits(Gs[3], np.eye(3) @ G3) and same_bits(Gs[2], Gs[3] @ np.linalg.inv(H[(3, 2)])) and same_bits(Gs[1], Gs[2] @ np.linalg.inv(H[(2, 1)]))
    assert np.array_equal(Gs[0], np.eye(3))
    # another anchor: the tree starts there
    Gs1, _, tree1 = hg.sequence_graph(4, pairs, [H[p] for p in pairs], [100] * 6, [39, 38, 50, 50, 60, 45], anchor=2)
    assert tree1[0] == (2, 3, 4) and np.array_equal(Gs1[2], np.eye(3)) and same_bits(Gs1[3], np.eye(3) @ H[(3, 2)])
    # a non-finite or missing H is not accepted, whatever its count
    bad = [H[p] for p in pairs]
    bad[4] = np.full((3, 3), np.nan)
    bad[5] = None
    _, accepted, tree = hg.sequence_graph(4, pairs, bad, [100] * 6, [39, 38, 50, 50, 60, 45], anchor=0)
    assert accepted.tolist() == [True, False, True, True, False, False] and tree == [(0, 1, 0), (1, 2, 2), (1, 3, 3)]


def test_graph_names_the_image_it_cannot_reach():
    import homography as hg
    H = [np.eye(3)] * 2
    with pytest.raises(ValueError, match="image 3"):
        hg.sequence_graph(4, [(1, 0), (2, 1)], H, [100, 100], [90, 90])
    with pytest.raises(ValueError, match="image 2"):
        hg.sequence_graph(3, [(1, 0), (2, 1)], H, [100, 100], [90, 38])       # the only edge to image 2 is not accepted
    for n, pairs in [(3, [(1, 0), (3, 1)]), (3, [(1, 1), (2, 1)]), (3, [(1, 0), (2.5, 1)]), (3, [(1, 0), 7])]:
        with pytest.raises(ValueError):
            hg.sequence_graph(n, pairs, H, [100, 100], [90, 90])
    with pytest.raises(ValueError):
        hg.sequence_graph(3, [(1, 0), (2, 1)], H, [100], [90, 90])
    with pytest.raises(ValueError):
        hg.sequence_graph(3, [(1, 0), (2, 1)], H, [100, 100], [90, 90], anchor=3)


def test_focal_takes_the_edges_of_a_graph():
    import homography as hg
    images, Hs = pc.sweep(4, 8, f=300.0, yaw=0.2)
    shapes = [im.shape for im in images]
    chainwise = hg.sequence_focal(shapes, Hs)
    assert hg.sequence_focal(shapes, Hs, pairs=[(1, 0), (2, 1), (3, 2)]) == chainwise
    assert hg.sequence_focal(shapes, [Hs[1], Hs[0], Hs[2]], pairs=[(2, 1), (1, 0), (3, 2)]) == chainwise      # a median: any order
    # an edge stored the other way round reads the shapes the other way round
    back = hg.sequence_focal(shapes, [np.linalg.inv(Hs[0])], pairs=[(0, 1)])
    assert back == hg.sequence_focal([shapes[1], shapes[0]], [np.linalg.inv(Hs[0])])
    with pytest.raises(ValueError):
        hg.sequence_focal(shapes, Hs, pairs=[(1, 0), (2, 1)])


# ---- 8. refusals come before the GPU ----
def test_python_refusals_come_before_the_gpu(monkeypatch, grid):
    import homography as hg
    import ransac as rs
    from ransac_with_homography_amd import _lib

    def no_gpu():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    images = [sc.random_image(40, 50, i) for i in range(3)]
    for kw in [dict(pairs="every"), dict(pairs=[(0, 0)]), dict(pairs=[(1, 0), (3, 1)]), dict(pairs=[(1, 0), (1, 0)]), dict(pairs=7),
               dict(pairs=[(1, 0, 2)]), dict(pairs=[(1.5, 0)]), dict(adjust="yes"), dict(adjust=1), dict(adjust=None)]:
        with pytest.raises(ValueError, match="stitch_sequence"):
            rs.stitch_sequence(images, **kw)
    Gs, pairs, matches = grid["Gs"], grid["pairs"], grid["matches"]
    for kw in [dict(on="cpu"), dict(max_iters=-1), dict(max_iters=2.5), dict(anchor=8), dict(masks=np.zeros((3, 1), dtype=np.int64)),
               dict(masks=np.zeros((len(pairs), 1), dtype=np.float64))]:
        with pytest.raises(ValueError, match="sequence"):
            hg.sequence_adjust(Gs, pairs, matches, **kw)
    with pytest.raises(ValueError):
        hg.sequence_adjust(Gs, pairs[:-1], matches)
    with pytest.raises(ValueError):
        hg.sequence_adjust(Gs, pairs + [(8, 0)], matches + [matches[0]])
    with pytest.raises(ValueError):
        hg.sequence_adjust(Gs[::-1], pairs, matches)                   # the anchor's map is not the identity
    with pytest.raises(ValueError):
        hg.sequence_adjust(np.concatenate([Gs[:3], np.zeros((1, 3, 3)), Gs[4:]]), pairs, matches, on="host")


def test_default_signature_still_takes_todays_calls():
    import homography as hg
    import ransac as rs
    sig = inspect.signature(rs.stitch_sequence)
    names = list(sig.parameters)
    assert names == ["images", "anchor", "th", "d", "k", "ransacMet", "seed", "blending", "features", "info", "gains", "projection",
                     "focal", "pairs", "adjust", "bands"]           # every earlier position is unchanged, `bands` stays last
    assert sig.parameters["pairs"].default == "adjacent" and sig.parameters["adjust"].default is False
    assert list(inspect.signature(hg.sequence_focal).parameters) == ["shapes", "Hs", "pairs"]
    assert inspect.signature(hg.sequence_focal).parameters["pairs"].default is None
    from ransac_with_homography_amd import homography as impl
    for name in ("sequence_graph", "sequence_adjust"):
        assert getattr(hg, name) is getattr(impl, name) and name in impl.__all__      # the top-level shim re-exports them
    from ransac_with_homography_amd import _lib, kernels
    for name in ("rwh_bundle_blocks", "rwh_host_bundle_blocks", "rwh_host_bundle_step"):
        assert name in _lib.EXPORTS
    assert hasattr(kernels, "bundle_blocks") and hasattr(kernels, "host_bundle_blocks")
