"""The sequence compositor on the GPU: rwh_stitch_sequence against its host twin (which tests/test_sequence_cpu.py holds to the
numpy restatement of the rule) on canvases that cross every launch edge, the Python layers above it, and the pipeline entry
ransac.stitch_sequence on three crops of one synthetic scene.  Every comparison of canvases is exact."""
import os

import numpy as np
import pytest

import sequence_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return sc.library(gpu=True)


host, device = sc.host, sc.device


EDGES = sc.edge_canvases()


@pytest.mark.parametrize("case", EDGES, ids=["fw%d-fh%d" % (c[0], c[1]) for c in EDGES])
def test_device_is_the_host_twin_across_launch_edges(lib, case):
    fw, fh, images, Gs, order, rows = case
    for blend in (sc.PASTE, sc.FEATHER):
        want = host(lib, images, Gs, 0, blend, order, rows=rows)
        got = device(images, Gs, 0, blend, order, rows=rows)
        assert got.shape[1] == fw and got.shape[0] == max(fh, 2) and (rows is None or rows[1] - rows[0] == fh)
        assert np.array_equal(got, want)              # rows that were not launched keep the fill in both
        launched = got if rows is None else got[rows[0]:rows[1]]
        assert launched.any() and not np.array_equal(launched, np.full_like(launched, 0xA5))


def test_one_image_and_sixty_four(lib):
    img = sc.random_image(9, 11, 1)
    assert np.array_equal(device([img], [np.eye(3)]), img)                      # N = 1: the anchor's bytes
    assert np.array_equal(device([img], [np.eye(3)], blend=sc.FEATHER), img)
    images, Gs = sc.translated_strip(64)
    order = list(range(64))[::-1]
    for blend, od in ((sc.PASTE, None), (sc.PASTE, order), (sc.FEATHER, None)):
        assert np.array_equal(device(images, Gs, 0, blend, od), host(lib, images, Gs, 0, blend, od))


def test_forty_candidates_in_one_tile(lib):
    """40 images over ONE 256 x 4 tile: more than any short fixed candidate list holds."""
    rng = np.random.default_rng(40)
    images = [sc.random_image(6, 30, 400 + i) for i in range(40)]
    Gs = [np.eye(3)] + [sc.homography(rng, 5.0 * i + 0.25, (i % 2) + 0.5, 0.004, 1e-6) for i in range(1, 40)]
    t = sc.tables(images, Gs, 0)
    assert t["size"][1] <= 256 and all(r[1] < 4 for r in t["rects"])           # every rectangle meets rows 0 .. 3 of the one block column
    order = list(range(40))[::-1]
    for blend, od in ((sc.PASTE, order), (sc.PASTE, None), (sc.FEATHER, None)):
        want = host(lib, images, Gs, 0, blend, od)
        assert np.array_equal(device(images, Gs, 0, blend, od), want)
    assert not np.array_equal(host(lib, images, Gs, 0, sc.PASTE, order), host(lib, images, Gs, 0, sc.PASTE, None))


def test_row_tiles_and_a_second_stream(lib):
    import torch
    _, images, Gs, anchor, order = sc.general_cases()[4]
    for blend in (sc.PASTE, sc.FEATHER):
        whole = device(images, Gs, anchor, blend, order)
        assert np.array_equal(whole, host(lib, images, Gs, anchor, blend, order))
        fh = whole.shape[0]
        bounds = [0, 5, fh - 7, fh]
        tiled = np.zeros_like(whole)
        for r0, r1 in zip(bounds[:-1], bounds[1:]):
            part = device(images, Gs, anchor, blend, order, rows=(r0, r1))
            assert (part[:r0] == 0xA5).all() and (part[r1:] == 0xA5).all()
            tiled[r0:r1] = part[r0:r1]
        assert np.array_equal(tiled, whole)
        on = sc.upload(images)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            other = device(images, Gs, anchor, blend, order, on=on)
        assert np.array_equal(other, whole)


def test_stitch_sequence_of_the_homography_module(lib):
    import torch
    import homography as hg
    rng = np.random.default_rng(77)
    images = [sc.random_image(30, 41, 4), sc.random_image(27, 38, 5), sc.random_image(33, 29, 6)]
    Hs = [sc.homography(rng, 22.5, 3.2), sc.homography(rng, 19.1, -5.7)]
    before = [im.copy() for im in images]
    for anchor, blending, blend in ((0, False, sc.PASTE), (1, False, sc.PASTE), (1, "feather", sc.FEATHER)):
        want = host(lib, images, sc.chain(Hs, anchor), anchor, blend)
        got = hg.stitchSequence(images, Hs=Hs, anchor=anchor, blending=blending)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
        tens = [torch.from_numpy(im).cuda() for im in images]
        out = hg.stitchSequence(tens, Gs=sc.chain(Hs, anchor), anchor=anchor, blending=blending)
        assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want)
        assert all(np.array_equal(t.cpu().numpy(), b) for t, b in zip(tens, before))          # texel (0,0) included
    assert all(np.array_equal(a, b) for a, b in zip(images, before))
    got = hg.stitchSequence(images, Hs=Hs, order=[2, 1, 0])
    assert np.array_equal(got, host(lib, images, sc.chain(Hs, 0), 0, sc.PASTE, [2, 1, 0]))
    # N = 2 is stitchPanorama, the reference's four canvas cases among the pairs
    for seed, Q, T, H in sc.oracle_pairs(8):
        assert np.array_equal(hg.stitchSequence([Q, T], Hs=[H]), hg.stitchPanorama(Q, T.copy(), H)), seed


TH = 5


@pytest.fixture(scope="module")
def crops():
    scene = sc.scene()
    return [np.ascontiguousarray(scene[:, x:x + 260]) for x in (0, 90, 180)]


def test_pipeline_on_three_crops_of_one_scene(lib, crops):
    """ransac.stitch_sequence, pixels -> panorama: the canvas is stitchSequence of the homographies it reports; each maps the
    corners of crop i+1 to within th (the call's inlier threshold, 5) of the true shift of 90 columns; no pixel inside the union
    of the true rectangles, shrunk by th, is left uncovered.  The observed corner error goes to profiles/stitch_sequence.txt by
    hand (printed here)."""
    import homography as hg
    import ransac as rs
    info = {}
    before = [c.copy() for c in crops]
    can = rs.stitch_sequence(crops, th=TH, info=info)
    assert isinstance(can, np.ndarray) and all(np.array_equal(a, b) for a, b in zip(crops, before))
    assert info["Hs"].shape == (2, 3, 3) and len(info["sizes"]) == 2 and len(info["inliers"]) == 2 and info["Gs"].shape == (3, 3, 3)
    assert np.array_equal(can, hg.stitchSequence(crops, Hs=info["Hs"]))
    corners = np.array([[0, 259, 259, 0], [0, 0, 199, 199], [1.0, 1, 1, 1]])
    worst = 0.0
    for i in range(2):
        p = info["Hs"][i] @ corners
        err = np.hypot(p[0] / p[2] - (corners[0] + 90), p[1] / p[2] - corners[1])
        print("pair %d: %d matches, %d inliers, corner error max %.4f px" % (i, info["sizes"][i], info["inliers"][i], err.max()))
        worst = max(worst, float(err.max()))
    print("maximum corner error %.4f px (bound: th = %d)" % (worst, TH))
    assert worst <= TH
    ox, oy = info["origin"]
    inner = can[TH - oy:200 - TH - oy, TH - ox:440 - TH - ox]                   # frame x in [th, 440 - th), y in [th, 200 - th)
    assert inner.shape[:2] == (200 - 2 * TH, 440 - 2 * TH)
    assert inner.any(axis=2).all(), "%d uncovered pixels inside the union" % int((~inner.any(axis=2)).sum())


def test_pipeline_names_the_pair_without_a_homography(lib, crops):
    import ransac as rs
    flat = np.full((200, 260, 3), 90, dtype=np.uint8)
    with pytest.raises(ValueError, match="pair 1"):
        rs.stitch_sequence([crops[0], crops[1], flat])
