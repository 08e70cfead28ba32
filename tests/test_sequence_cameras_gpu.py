"""The camera rule on the GPU: rwh_camera_blocks against its host twin (which tests/test_sequence_cameras_cpu.py holds to the numpy
restatement) bit for bit, `sequence_adjust_cameras(on="device")` against on="host", and the pipeline entry
ransac.stitch_sequence(adjust="cameras") on three crops of one synthetic scene."""
import numpy as np
import pytest

import bundle_cases as bc
import camera_cases as cc
import sequence_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return sc.library(gpu=True)


@pytest.fixture(scope="module")
def sized():
    return cc.size_list_case()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def hblocks(lib, *a):
    st, blocks, count, status = cc.host_blocks(lib, *a)
    assert st == 0
    return blocks, count, status


@pytest.mark.parametrize("which", ["ones", "random", "short", "zero row"])
def test_device_blocks_are_the_twin_bit_for_bit(lib, sized, which):
    """One launch of 13 edges over 5 cameras, the sizes 0 .. 600 that cross the mask word, the staged chunk and the partials --
    the smallest shapes that do; exact, and a second call gives the same bits."""
    c = sized
    sets = bc.mask_sets(c["sizes"])
    masks = sets["random"].copy() if which == "zero row" else sets[which]
    if which == "zero row":
        masks[11] = 0
    want, want_count, want_status = hblocks(lib, c["pa"], c["pb"], c["offsets"], masks, c["rec"])
    blocks, count, status = cc.device_blocks(c["pa"], c["pb"], c["offsets"], masks, c["rec"])
    assert same_bits(blocks, want), "entries that differ: %s" % (np.argwhere(blocks != want)[:8].tolist(),)
    assert np.array_equal(count, want_count) and np.array_equal(status, want_status)
    again = cc.device_blocks(c["pa"], c["pb"], c["offsets"], masks, c["rec"])
    assert same_bits(again[0], blocks) and np.array_equal(again[1], count) and np.array_equal(again[2], status)


def test_behind_is_reported_and_isolated_on_the_device(lib):
    c, pa, rec, masks, cleared = cc.behind_case()
    blocks, count, status = cc.device_blocks(pa, c["pb"], c["offsets"], masks, rec)
    assert status.tolist() == [cc.OK, cc.BEHIND, cc.OK] and count.tolist() == [65, 128, 5]
    blocks2, count2, status2 = cc.device_blocks(pa, c["pb"], c["offsets"], cleared, rec)
    assert status2.tolist() == [cc.OK, cc.OK, cc.OK] and same_bits(blocks, blocks2)
    want, _, want_status = hblocks(lib, pa, c["pb"], c["offsets"], masks, rec)
    assert same_bits(blocks, want) and np.array_equal(status, want_status)


def test_the_two_ends_of_a_launch(lib):
    """E = RWH_BUNDLE_MAX_EDGES = 2016 with one row each, and its edges 0 and 2015 alone (E = 1, offsets from 0)."""
    c = cc.launch_case()
    masks = bc.mask_sets(c["sizes"])["ones"]
    assert len(c["sizes"]) == 2016 and int(c["offsets"][-1]) == 2016
    want, want_count, want_status = hblocks(lib, c["pa"], c["pb"], c["offsets"], masks, c["rec"])
    blocks, count, status = cc.device_blocks(c["pa"], c["pb"], c["offsets"], masks, c["rec"])
    assert same_bits(blocks, want) and np.array_equal(count, want_count) and np.array_equal(status, want_status)
    assert (count == 1).all() and not status.any() and np.isfinite(blocks).all()
    for e in (0, 2015):
        one, one_count, one_status = cc.device_blocks(*cc.single_edge(c, masks, e))
        assert same_bits(one, blocks[e:e + 1]) and one_count[0] == 1 and one_status[0] == cc.OK


@pytest.mark.parametrize("focals", ["shared", "per-image"])
def test_adjust_on_device_is_adjust_on_host(lib, focals):
    """GRID from `sequence_cameras` of the true maps with focal 120, the "random" inlier words as an int64 tensor on the GPU."""
    import torch
    import homography as hg
    scene, shapes, _, _ = cc.grid_cameras()
    Rs0, fs0 = hg.sequence_cameras(shapes, scene["Gs"], 120.0)
    masks = bc.mask_sets(scene["sizes"])["random"]
    host, dev = {}, {}
    want = hg.sequence_adjust_cameras(shapes, Rs0, fs0, scene["pairs"], scene["matches"], masks=masks, focals=focals, on="host", info=host)
    got = hg.sequence_adjust_cameras(shapes, Rs0, fs0, scene["pairs"], scene["matches"], masks=torch.from_numpy(masks).cuda(), focals=focals,
                                     on="device", info=dev)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert dev["iters"] == host["iters"] >= 3 and dev["lambda"] == host["lambda"]
    assert same_bits(np.array(dev["cost"]), np.array(host["cost"]))


def test_pipeline_with_cameras_on_three_crops(lib):
    """stitch_sequence(pairs="all", adjust="cameras") with the ratio matcher on the three crops of
    tests/test_sequence_bundle_gpu.py: a canvas comes back, composed from the maps it reports; the reported Rs are rotations
    (orthonormal and of determinant +1 to 16 u: they come out of an SVD's U V^T), the anchor's the identity; the cost never rises.
    The crops are translations of one scene -- no rotation about the camera's centre produces them exactly and the focal length
    is not determined by them --, so nothing is asserted about the focal's value beyond its being one."""
    import homography as hg
    import ransac as rs
    scene = sc.scene()
    crops = [np.ascontiguousarray(scene[:, x:x + 260]) for x in (0, 90, 180)]
    info = {}
    out = rs.stitch_sequence(crops, pairs="all", adjust="cameras", features={"ratio": 0.7}, info=info)
    assert isinstance(out, np.ndarray) and out.ndim == 3 and out.shape[2] == 3 and out.dtype == np.uint8
    assert out.shape[0] >= crops[0].shape[0] and out.shape[1] > crops[0].shape[1]
    adj = info["adjust"]
    Rs, fs, cost = adj["Rs"], adj["focals"], adj["cost"]
    print("cost %s, %d steps, focal %s" % (["%.6g" % c for c in cost], adj["iters"], fs.tolist()))
    assert Rs.shape == (3, 3, 3) and np.array_equal(Rs[0], np.eye(3))
    assert np.abs(Rs @ Rs.transpose(0, 2, 1) - np.eye(3)).max() <= 16 * bc.U
    assert np.abs(np.linalg.det(Rs) - 1.0).max() <= 16 * bc.U
    assert all(b < a for a, b in zip(cost, cost[1:])) and cost[-1] <= cost[0] and len(cost) == adj["iters"] + 1
    assert fs.shape == (3,) and (fs == fs[0]).all() and np.isfinite(fs).all() and fs[0] > 0
    assert info["focal"] is None and info["pairs"] == [(1, 0), (2, 0), (2, 1)]
    assert np.array_equal(info["Gs"], hg.sequence_camera_maps([c.shape for c in crops], Rs, fs))
    assert np.array_equal(out, hg.stitchSequence(crops, Gs=info["Gs"]))
