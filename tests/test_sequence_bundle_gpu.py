"""The bundle rule on the GPU: rwh_bundle_blocks against its host twin (which tests/test_sequence_bundle_cpu.py holds to the numpy
restatement) bit for bit, `sequence_adjust(on="device")` against on="host", the mask rows `run_batch` leaves on the device, and
the pipeline entry ransac.stitch_sequence with a pair graph on three crops of one synthetic scene."""
import numpy as np
import pytest

import bundle_cases as bc
import sequence_cases as sc

pytestmark = pytest.mark.gpu
TH = 5


@pytest.fixture(scope="module")
def lib():
    return sc.library(gpu=True)


@pytest.fixture(scope="module")
def sized():
    return bc.size_list_case()


@pytest.fixture(scope="module")
def crops():
    scene = sc.scene()
    return [np.ascontiguousarray(scene[:, x:x + 260]) for x in (0, 90, 180)]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


device_blocks = bc.device_blocks


@pytest.mark.parametrize("which", ["ones", "random", "short"])
def test_device_blocks_are_the_twin_bit_for_bit(lib, sized, which):
    """One launch of 13 edges over 5 images, the sizes 0 .. 600 that cross the mask word, the staged chunk and the partials;
    exact, and a second call gives the same bits."""
    c = sized
    masks = bc.mask_sets(c["sizes"])[which]
    st, want, want_count, want_status = bc.host_blocks(lib, c["pa"], c["pb"], c["offsets"], masks, c["T"])
    assert st == 0
    blocks, count, status = device_blocks(c["pa"], c["pb"], c["offsets"], masks, c["T"])
    assert same_bits(blocks, want), "entries that differ: %s" % (np.argwhere(blocks != want)[:8].tolist(),)
    assert np.array_equal(count, want_count) and np.array_equal(status, want_status)
    again = device_blocks(c["pa"], c["pb"], c["offsets"], masks, c["T"])
    assert same_bits(again[0], blocks) and np.array_equal(again[1], count) and np.array_equal(again[2], status)


def test_behind_is_reported_and_isolated_on_the_device(lib):
    c, pa, T, masks, cleared = bc.behind_case()
    blocks, count, status = device_blocks(pa, c["pb"], c["offsets"], masks, T)
    assert status.tolist() == [bc.OK, bc.BEHIND, bc.OK] and count.tolist() == [65, 128, 5]
    blocks2, count2, status2 = device_blocks(pa, c["pb"], c["offsets"], cleared, T)
    assert status2.tolist() == [bc.OK, bc.OK, bc.OK] and same_bits(blocks, blocks2)
    plain, _, _ = device_blocks(c["pa"], c["pb"], c["offsets"], masks, c["T"])
    assert same_bits(blocks[[0, 2]], plain[[0, 2]])
    st, want, _, want_status = bc.host_blocks(lib, pa, c["pb"], c["offsets"], masks, T)
    assert st == 0 and same_bits(blocks, want) and np.array_equal(status, want_status)


def test_adjust_on_device_is_adjust_on_host(lib):
    import homography as hg
    grid = bc.grid_scene()
    start = bc.snake_start(lib, grid)
    host, dev = {}, {}
    want = hg.sequence_adjust(start, grid["pairs"], grid["matches"], on="host", info=host)
    got = hg.sequence_adjust(start, grid["pairs"], grid["matches"], on="device", info=dev)
    assert same_bits(got, want)
    assert dev["iters"] == host["iters"] and dev["lambda"] == host["lambda"]
    assert same_bits(np.array(dev["cost"]), np.array(host["cost"]))


def test_run_batch_leaves_the_winners_mask_rows(lib):
    import ransac as rs
    rng = np.random.default_rng(4)
    datas = []
    for m in (70, 129, 40):
        X = (rng.uniform(0, 1, (2, m)) * [[200.0], [150.0]]).astype(np.float32)
        Y = X + np.float32([[12.0], [-7.0]])
        Y[:, ::5] += rng.uniform(20, 60, (2, len(range(0, m, 5)))).astype(np.float32)       # every fifth is an outlier
        datas.append([X, Y])
    info = {}
    res = rs.run_batch(datas, th=TH, d=50, k=200, method="fwd", seed=1, refit="device", info=info)
    masks, offsets = info["mask_device"].cpu().numpy(), info["offsets_device"].cpu().numpy()
    assert masks.dtype == np.int64 and masks.shape == (3, 3) and offsets.tolist() == [0, 70, 199, 239]
    for p, (_, inliers, count) in enumerate(res):
        bits = np.unpackbits(masks[p].view(np.uint8), bitorder="little")
        assert np.array_equal(np.nonzero(bits)[0], inliers[0]) and int(count) == len(inliers[0]) > 0


def corner_deviation(Ga, Gb, shape):
    h, w = shape[0], shape[1]
    corners = np.array([[0, w - 1, w - 1, 0], [0, 0, h - 1, h - 1], [1.0, 1, 1, 1]])
    pa, pb = Ga @ corners, Gb @ corners
    return float(np.abs(pa[:2] / pa[2] - pb[:2] / pb[2]).max())


def test_pipeline_with_a_pair_graph_on_three_crops(lib, crops):
    """The defaults are today's call; pairs="all", adjust=True composes the Gs it reports, spans the three images and does not
    raise the cost of the tree it starts from; the crops in the order (0, 2, 1) register to within th = 5 px (the call's own inlier
    threshold) of the in-order run.  The measured deviation is printed: 0.000 px where this was written (the crops are integer
    shifts of one scene, so the residuals are 0 before and after the adjustment)."""
    import homography as hg
    import ransac as rs
    base, same = {}, {}
    can = rs.stitch_sequence(crops, th=TH, info=base)
    assert np.array_equal(can, rs.stitch_sequence(crops, th=TH, info=same, pairs="adjacent", adjust=False))
    assert np.array_equal(base["Hs"], same["Hs"]) and np.array_equal(base["Gs"], same["Gs"]) and "pairs" not in same

    info = {}
    full = rs.stitch_sequence(crops, th=TH, info=info, pairs="all", adjust=True)
    assert isinstance(full, np.ndarray) and "Hs" not in info
    assert np.array_equal(full, hg.stitchSequence(crops, Gs=info["Gs"]))
    assert info["pairs"] == [(1, 0), (2, 0), (2, 1)] and len(info["accepted"]) == 3
    assert sorted(child for _, child, _ in info["tree"]) == [1, 2] and info["tree"][0][0] == 0
    cost = info["adjust"]["cost"]
    assert cost[-1] <= cost[0] and all(b < a for a, b in zip(cost, cost[1:]))
    assert np.array_equal(info["Gs"][0], np.eye(3))

    chain = {}
    rs.stitch_sequence(crops, th=TH, info=chain, adjust=True)                # adjacent pairs, adjusted: the chain's Hs are reported
    assert chain["pairs"] == [(1, 0), (2, 1)] and np.array_equal(chain["Hs"], base["Hs"]) and chain["adjust"]["cost"][0] >= chain["adjust"]["cost"][-1]

    graph = {}
    rs.stitch_sequence(crops, th=TH, info=graph, pairs="all")
    assert graph["adjust"] is None and np.array_equal(graph["accepted"], info["accepted"])

    order = [0, 2, 1]
    shuffled = {}
    rs.stitch_sequence([crops[i] for i in order], th=TH, info=shuffled, pairs="all")
    worst = max(corner_deviation(shuffled["Gs"][j], graph["Gs"][i], crops[i].shape) for j, i in enumerate(order))
    print("crops in the order (0, 2, 1): corners within %.3f px of the in-order run (th = %d); adjusted cost %.6g -> %.6g in %d steps"
          % (worst, TH, cost[0], cost[-1], info["adjust"]["iters"]))
    assert worst <= TH
