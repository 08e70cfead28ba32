"""What sits around the bundle rule's arithmetic, on the GPU: rwh_bundle_blocks against its host twin (bit for bit) on every side of
the validity test and at the two ends of a launch, `sequence_adjust` fed the way `stitch_sequence(adjust=True)` feeds it -- a
`DeviceProblems` and an int64 mask tensor on the GPU -- on GRID, where the residuals are not zero, and the pipeline on three views
that are no integer shifts of their scene.  tests/test_bundle_loop_cpu.py holds the twin and the host loop to their references."""
import numpy as np
import pytest

import bundle_cases as bc
import sequence_cases as sc

pytestmark = pytest.mark.gpu
TH = 5
VALIDITY = ["x nan", "x +inf", "y -inf", "x 3e38", "p2 +0", "p2 -0", "p2 negative", "p2 denormal"]


@pytest.fixture(scope="module")
def lib():
    return sc.library(gpu=True)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def twin(lib, *a):
    st, blocks, count, status = bc.host_blocks(lib, *a)
    assert st == 0
    return blocks, count, status


# ---- 1. every side of the validity test ----
@pytest.fixture(scope="module")
def validity(lib):
    c, masks, cleared, cases = bc.validity_cases()
    assert [name for name, _, _ in cases] == VALIDITY
    plain = bc.device_blocks(c["pa"], c["pb"], c["offsets"], masks, c["T"])
    return c, masks, cleared, {name: (pa, T) for name, pa, T in cases}, plain


@pytest.mark.parametrize("name", VALIDITY)
def test_one_invalid_row_on_the_device(lib, validity, name):
    """Row 130 of edge 1 (200 rows: the second staged chunk, wave 2's partial) invalid in one of eight ways: the device reports
    what the twin reports and leaves the twin's bits -- where a device isfinite or float64 divide could part from the host's."""
    c, masks, cleared, cases, plain = validity
    pa, T = cases[name]
    blocks, count, status = bc.device_blocks(pa, c["pb"], c["offsets"], masks, T)
    assert status.tolist() == [bc.OK, bc.BEHIND, bc.OK] and count.tolist() == [70, 199, 9]
    assert np.isfinite(blocks).all()
    blocks2, count2, status2 = bc.device_blocks(pa, c["pb"], c["offsets"], cleared, T)
    assert status2.tolist() == [bc.OK, bc.OK, bc.OK] and count2.tolist() == [70, 199, 9] and same_bits(blocks, blocks2)
    assert same_bits(blocks[[0, 2]], plain[0][[0, 2]])
    want, want_count, want_status = twin(lib, pa, c["pb"], c["offsets"], masks, T)
    assert same_bits(blocks, want), "entries that differ: %s" % (np.argwhere(blocks != want)[:8].tolist(),)
    assert np.array_equal(count, want_count) and np.array_equal(status, want_status)


# ---- 2. the two ends of a launch ----
def test_largest_and_smallest_launch(lib):
    """RWH_BUNDLE_MAX_EDGES = 2016 edges in one launch (33 824 rows; sizes 0, 1, 2, 3, 4, 5, 7, 64, 65 in turn; the "random" masks)
    between the guard words of `device_blocks`, bit for bit the twin; the last and the first edge launched alone (n_edges = 1,
    offsets from 0) give their rows of the big launch."""
    c, masks = bc.launch_case()
    assert len(c["sizes"]) == 2016 and int(c["offsets"][-1]) == 33824
    want, want_count, want_status = twin(lib, c["pa"], c["pb"], c["offsets"], masks, c["T"])
    blocks, count, status = bc.device_blocks(c["pa"], c["pb"], c["offsets"], masks, c["T"])
    assert same_bits(blocks, want), "edges that differ: %s" % (np.unique(np.argwhere(blocks != want)[:, 0])[:8].tolist(),)
    assert np.array_equal(count, want_count) and np.array_equal(status, want_status) and not status.any()
    for e in (2015, 0):
        one, one_count, one_status = bc.device_blocks(*bc.single_edge(c, masks, e))
        assert same_bits(one, blocks[e:e + 1]) and one_count[0] == count[e] and one_status[0] == status[e]
    assert count[0] == 0 and not blocks[0].any() and count[2015] > 0


# ---- 3. the device-resident path on real residuals ----
@pytest.fixture(scope="module")
def grid_on_device(lib):
    import torch
    from ransac_with_homography_amd.features import DeviceProblems
    grid = bc.grid_scene()
    pa, pb, _ = bc.concatenated(grid["matches"])
    problems = DeviceProblems(torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda(), grid["sizes"])
    start = bc.snake_start(lib, grid)
    far = bc.far_start(start, bc.FAR_ONE_REJECT["seed"], bc.FAR_ONE_REJECT["persp"])
    return grid, problems, {"chain": start, "one reject": far}


@pytest.mark.parametrize("which", ["random", "ones"])
def test_adjust_from_tensors_is_adjust_on_host(grid_on_device, which):
    """GRID the way the pipeline hands it over: a `DeviceProblems` and the masks as an int64 tensor on the GPU, two words wider
    than the largest edge needs.  From the chain's start, from the far start that rejects a step, and from the adjusted result
    (with every row an inlier no step is accepted up to the lambda ceiling): on="device" gives the bits of on="host" with the
    same arguments."""
    import torch
    import homography as hg
    grid, problems, begins = grid_on_device
    words = bc.mask_sets(grid["sizes"])[which]
    wide = torch.from_numpy(np.concatenate([words, np.full((len(words), 2), -1, dtype=np.int64)], axis=1)).cuda()
    begins = dict(begins)
    for name in ("chain", "one reject", "adjusted"):
        host, dev = {}, {}
        want = hg.sequence_adjust(begins[name], grid["pairs"], problems, masks=wide, on="host", info=host)
        got = hg.sequence_adjust(begins[name], grid["pairs"], problems, masks=wide, on="device", info=dev)
        print("%s masks, %s: cost %.4f -> %.4f, %d accepted, lambda %.3g" % (which, name, host["cost"][0], host["cost"][-1], host["iters"], host["lambda"]))
        assert same_bits(got, want), name
        assert dev["iters"] == host["iters"] and dev["lambda"] == host["lambda"], name
        assert same_bits(np.array(dev["cost"]), np.array(host["cost"])), name
        if name == "chain":
            begins["adjusted"] = want
            assert host["iters"] >= 1
            # the tensors give what the lists and numpy words give on the host
            again = hg.sequence_adjust(begins[name], grid["pairs"], grid["matches"], masks=words, on="host")
            assert same_bits(want, again)
        if name == "adjusted" and which == "ones":        # (with the random masks one more step of 6e-13 is accepted on the way up)
            assert host["iters"] == 0 and host["lambda"] > 1e12 and same_bits(want, begins["adjusted"])


# ---- 4. the pipeline with residuals that are not zero ----
def corner_deviation(Ga, Gb, shape):
    h, w = shape[0], shape[1]
    corners = np.array([[0, w - 1, w - 1, 0], [0, 0, h - 1, h - 1], [1.0, 1, 1, 1]])
    pa, pb = Ga @ corners, Gb @ corners
    return float(np.abs(pa[:2] / pa[2] - pb[:2] / pb[2]).max())


def test_pipeline_on_three_warped_views(lib):
    """Three views of one scene under known maps that are no integer shifts (bundle_cases.warped_views), so the matches carry
    sub-pixel residuals.  The stages by hand -- extract_batch, match_batch, run_batch(refit="device"), sequence_graph -- and then
    sequence_adjust on the mask rows run_batch left on the device (outliers cleared, as wide as the batch's largest problem):
    on="device" is on="host" bit for bit, and both are what stitch_sequence(pairs="all", adjust=True) reports.  The adjustment
    takes at least one step, lowers the cost strictly, does not raise the cost stated from the geometry (bundle_cases.
    reference_cost over the downloaded points and mask bits), and every view's corners land within th = 5 px (the call's own
    inlier threshold) of the ground truth.  The figures are printed."""
    import homography as hg
    import ransac as rs
    from ransac_with_homography_amd.features import extract_batch, match_batch
    views, truth = bc.warped_views()
    pairs = [(1, 0), (2, 0), (2, 1)]
    search = dict(th=TH, d=70, k=1000, seed=0)
    feats = extract_batch(views)
    problems = match_batch([(feats[s][0], feats[s][1], feats[d][0], feats[d][1]) for s, d in pairs])
    found = {}
    res = rs.run_batch(problems, n=4, method="fwd", refit="device", info=found, **search)
    sizes, inliers = [int(m) for m in problems.sizes], [int(r[2]) for r in res]
    tree_Gs, accepted, tree = hg.sequence_graph(3, pairs, [r[0] for r in res], sizes, inliers, anchor=0)
    print("matches %s, inliers %s, accepted %s, tree %s" % (sizes, inliers, accepted.tolist(), tree))
    assert accepted.all()                                                   # a condition on the fixture: all three pairs register
    masks = found["mask_device"]
    assert masks.is_cuda and tuple(masks.shape) == (3, (max(sizes) + 63) // 64)

    host, dev = {}, {}
    want = hg.sequence_adjust(tree_Gs, pairs, problems, masks=masks, on="host", info=host)
    got = hg.sequence_adjust(tree_Gs, pairs, problems, masks=masks, on="device", info=dev)
    assert same_bits(got, want) and dev["iters"] == host["iters"] and dev["lambda"] == host["lambda"]
    assert same_bits(np.array(dev["cost"]), np.array(host["cost"]))

    info = {}
    rs.stitch_sequence(views, info=info, pairs="all", adjust=True, ransacMet="fwd", **search)
    assert info["pairs"] == pairs and np.array_equal(info["accepted"], accepted) and info["tree"] == tree
    assert same_bits(info["Gs"], got)
    cost = info["adjust"]["cost"]
    assert same_bits(np.array(cost), np.array(dev["cost"])) and info["adjust"]["iters"] == dev["iters"]
    assert cost[0] > 0                                                      # a condition on the fixture: there is something to adjust
    assert info["adjust"]["iters"] >= 1 and all(b < a for a, b in zip(cost, cost[1:]))

    pa, pb, words = problems.pts_a.cpu().numpy(), problems.pts_b.cpu().numpy(), masks.cpu().numpy()
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    matches = [(pa[offsets[e]:offsets[e + 1]], pb[offsets[e]:offsets[e + 1]]) for e in range(3)]
    rows = sum(bc.mask_bit(words[e].view(np.uint64), i) for e in range(3) for i in range(sizes[e]))
    assert rows == sum(inliers)
    before, after = bc.reference_cost(tree_Gs, pairs, matches, words), bc.reference_cost(got, pairs, matches, words)
    worst = max(corner_deviation(got[i], truth[i], views[i].shape) for i in range(3))
    tree_worst = max(corner_deviation(tree_Gs[i], truth[i], views[i].shape) for i in range(3))
    print("cost %s in %d steps; from the geometry %.6f -> %.6f over %d rows; corners within %.3f px of the truth (tree: %.3f px; th = %d)"
          % (", ".join("%.6f" % v for v in cost), info["adjust"]["iters"], before, after, rows, worst, tree_worst, TH))
    assert after <= before
    assert abs(cost[0] - before) <= (2 * rows + 64) * bc.U * before and abs(cost[-1] - after) <= (2 * rows + 64) * bc.U * after
    assert worst <= TH
