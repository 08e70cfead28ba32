"""The ring rule on the GPU: the ring forms of the compositor, the overlap statistics and the multi-band blend against their host
twins (which tests/test_sequence_ring_cpu.py holds to the numpy restatement) on canvases of one, two and three tile columns with an
image across the seam, the Python layers above them, and the pipeline entry ransac.stitch_ring (ransac.stitch_sequence with wrap=True, pairs="ring").  Every
comparison is exact, every device canvas lies between canaries, and the multi-band workspace is pre-filled."""
import numpy as np
import pytest

import gain_cases as gc
import projection_cases as pc
import ring_cases as rc
import sequence_cases as sc

pytestmark = pytest.mark.gpu

PERIODS = (256, 512, 768)           # one, two and three columns of 256 x 4 tiles
HEIGHTS = (1, 4, 5, 9)


@pytest.fixture(scope="module")
def lib():
    return sc.library(gpu=True)


def crossing(t):
    return (t["rects"][:, 0] + t["rects"][:, 2] > t["size"][1]).any()


@pytest.mark.parametrize("kind", rc.SURFACES)
@pytest.mark.parametrize("P", (256, 512))
def test_device_is_the_twin(lib, kind, P):
    """The 12-image and the 13-image circle: paste (a permuted order) and feather, with and without gains; the statistics; multi-band
    at bands 1, 2 and 5."""
    n = rc.CASES[P]["n"]
    order = list(np.random.default_rng(P).permutation(n))
    images, t = rc.circle_tables(P, kind, 0, order)
    assert crossing(t)
    on = sc.upload(images)
    for blend in (rc.PASTE, rc.FEATHER):
        for gains in (None, rc.gains_for(n)):
            assert np.array_equal(rc.device(images, t, blend, gains=gains, on=on), rc.host(lib, images, t, blend, gains=gains)), (blend, gains)
    for stride in (1, 3, 4):
        for a, b in zip(rc.device_stats(images, t, stride), rc.host_stats(lib, images, t, stride)):
            assert np.array_equal(a, b), stride
    for bands in (1, 2, 5):
        for gains in (None, rc.gains_for(n)):
            assert np.array_equal(rc.device_multiband(lib, images, t, bands, gains), rc.host_multiband(lib, images, t, bands, gains)), (bands, gains)


@pytest.mark.parametrize("kind", rc.SURFACES)
@pytest.mark.parametrize("P", PERIODS)
def test_launch_edges(lib, kind, P):
    """Canvases of HEIGHTS rows cut out of each circle, the image across the seam wrapping into tile column 0: paste and feather with
    and without gains, the statistics, multi-band."""
    images, whole = rc.circle_tables(P, kind)
    mid = whole["size"][0] // 2 - 4
    for fh in HEIGHTS:
        ims, t = rc.crop_rows(images, whole, mid, fh)
        assert crossing(t)
        on = sc.upload(ims)
        for blend in (rc.PASTE, rc.FEATHER):
            for gains in (None, rc.gains_for(len(ims))):
                want = rc.host(lib, ims, t, blend, gains=gains)
                assert np.array_equal(rc.device(ims, t, blend, gains=gains, on=on), want), (fh, blend, gains)
        assert want.any()
        for a, b in zip(rc.device_stats(ims, t, 3), rc.host_stats(lib, ims, t, 3)):
            assert np.array_equal(a, b), fh
        assert np.array_equal(rc.device_multiband(lib, ims, t, 2), rc.host_multiband(lib, ims, t, 2)), fh


@pytest.mark.parametrize("kind", rc.SURFACES)
def test_row_ranges_that_cut_a_tile(lib, kind):
    images, whole = rc.circle_tables(512, kind)
    ims, t = rc.crop_rows(images, whole, whole["size"][0] // 2 - 4, 9)
    on = sc.upload(ims)
    for rows in ((0, 1), (1, 2), (3, 6), (4, 9), (2, 8), (6, 6)):
        for blend in (rc.PASTE, rc.FEATHER):
            want = rc.host(lib, ims, t, blend, rows=rows)
            assert np.array_equal(rc.device(ims, t, blend, rows=rows, on=on), want), (rows, blend)


@pytest.mark.parametrize("kind", rc.SURFACES)
def test_rolling_the_tables_rolls_the_canvas(lib, kind):
    """Consequence (b) on the device: s = 37 under paste and feather, s = 64 under multi-band at bands 5 and in the statistics at
    stride 4."""
    images, t = rc.circle_tables(256, kind)
    on = sc.upload(images)
    for blend in (rc.PASTE, rc.FEATHER):
        assert np.array_equal(rc.device(images, rc.roll(t, 37), blend, on=on), np.roll(rc.device(images, t, blend, on=on), 37, axis=1))
    assert np.array_equal(rc.device_multiband(lib, images, rc.roll(t, 64), 5), np.roll(rc.device_multiband(lib, images, t, 5), 64, axis=1))
    for a, b in zip(rc.device_stats(images, rc.roll(t, 64), 4), rc.device_stats(images, t, 4)):
        assert np.array_equal(a, b)


def test_device_refusals_come_before_any_launch(lib):
    import torch
    from ransac_with_homography_amd import kernels
    images, t = rc.circle_tables(256, "cylindrical")
    col, row = pc.device_tables(t)
    on = sc.upload(images)
    fh, P = t["size"]
    can, fetch = sc.guarded_device_canvas(fh, P)

    def spoilt(i, j, v):
        rects = t["rects"].copy()
        rects[i, j] = v
        return rects
    for rects in (spoilt(3, 0, -1), spoilt(3, 0, P), spoilt(3, 2, P + 1)):
        with pytest.raises(ValueError):
            kernels.stitch_sequence_ring(on, t["m"], rects, col, row, t["order"], rc.PASTE, t["size"], out=can)
        with pytest.raises(ValueError):
            kernels.stitch_sequence_multiband_ring(on, t["m"], rects, col, row, t["size"], 2, out=can)
        with pytest.raises(ValueError):
            kernels.sequence_overlap_tables_ring(on, t["m"], rects, col, row, t["size"], 1)
    with pytest.raises(ValueError):
        kernels.stitch_sequence_ring(on, t["m"], t["rects"], col[1:], row, t["order"], rc.PASTE, t["size"], out=can)
    ptrs = np.array([d.data_ptr() for d in on], dtype=np.uint64)
    head = (ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, t["n"])
    ws = torch.empty(4096, dtype=torch.int64, device="cuda")
    for c, r in ((0, row.data_ptr()), (col.data_ptr(), 0), (col.data_ptr() + 8, row.data_ptr())):        # NULL, NULL, misaligned
        assert lib.rwh_stitch_sequence_ring(*head, t["order"].ctypes.data, rc.PASTE, c, r, can.data_ptr(), fh, P, 0, fh, ws.data_ptr(), 32768, 0, None) == -1
    for w in (255, 257):                                                                                 # not a whole number of tiles
        assert lib.rwh_stitch_sequence_ring(*head, t["order"].ctypes.data, rc.PASTE, col.data_ptr(), row.data_ptr(), can.data_ptr(), fh, w, 0, fh,
                                            ws.data_ptr(), 32768, 0, None) == -1
    need = rc.workspace_bytes(lib, t, 2)
    big = torch.empty((need + 7) // 8, dtype=torch.int64, device="cuda")
    assert lib.rwh_stitch_multiband_ring(*head, 2, None, col.data_ptr(), row.data_ptr(), can.data_ptr(), fh, P, big.data_ptr(), need - 1, 0) == -1    # too small
    assert lib.rwh_stitch_multiband_ring(*head, 2, None, col.data_ptr(), row.data_ptr(), can.data_ptr(), fh, P, big.data_ptr() + 4, need, 0) == -1    # misaligned
    torch.cuda.synchronize()
    assert (fetch() == 0xA5).all()


@pytest.mark.parametrize("kind", rc.SURFACES)
def test_stitch_sequence_arrays_and_tensors(lib, kind):
    """stitchSequence(wrap=True) and sequence_gains(wrap=True) against the host twins: numpy in -> numpy out, tensor in -> tensor out."""
    import torch
    from ransac_with_homography_amd import homography as hg
    images, Gs, f = rc.circle(256, 2)
    t = rc.tables(images, Gs, 2, kind, f)
    before = [im.copy() for im in images]
    for blending, blend in ((False, rc.PASTE), ("feather", rc.FEATHER)):
        info = {}
        can = hg.stitchSequence(images, Gs=Gs, anchor=2, blending=blending, projection=kind, focal=f, wrap=True, info=info)
        assert isinstance(can, np.ndarray) and np.array_equal(can, rc.host(lib, images, t, blend))
        assert info["period"] == 256 and info["radius"] == 256 / (2.0 * np.pi)
    ten = hg.stitchSequence([torch.from_numpy(im) for im in images], Gs=Gs, anchor=2, blending="feather", projection=kind, focal=f, wrap=True)
    assert isinstance(ten, torch.Tensor) and ten.is_cuda and np.array_equal(ten.cpu().numpy(), can)
    wide = hg.stitchSequence(images, Gs=Gs, anchor=2, projection=kind, focal=f, wrap=512)
    assert wide.shape[1] == 512 and np.array_equal(wide, rc.host(lib, images, rc.tables(images, Gs, 2, kind, f, 512)))
    info, ginfo = {}, {}
    auto = hg.stitchSequence(images, Gs=Gs, anchor=2, blending="multiband", bands=2, gains="auto", info=info, projection=kind, focal=f, wrap=True)
    st, want = gc.host_gains(lib, *rc.host_stats(lib, images, t, 4))
    assert st == 0 and np.array_equal(info["gains"], want)
    assert np.array_equal(info["gains"], hg.sequence_gains(images, Gs=Gs, anchor=2, projection=kind, focal=f, wrap=True, info=ginfo))
    assert ginfo["period"] == 256 and ginfo["count"][0, 11] > 0                                      # the first image meets the last
    assert np.array_equal(hg.sequence_gains([torch.from_numpy(im) for im in images], Gs=Gs, anchor=2, projection=kind, focal=f, wrap=True), want)
    assert np.array_equal(auto, rc.host_multiband(lib, images, t, 2, gains=want))
    assert all(np.array_equal(a, b) for a, b in zip(images, before))


def test_pipeline_closes_the_circle(lib):
    """ransac.stitch_ring on a full circle of 14 views of a texture wrapped round a cylinder: every pair of the ring is accepted,
    the closing one included, the canvas is stitchSequence of what the call reports, and row s = 0 is covered in every column.  How
    close the adjusted focal comes to the true one is printed, not asserted."""
    from ransac_with_homography_amd import homography as hg
    from ransac_with_homography_amd import ransac as rs
    views = rc.cylinder_views()
    n = len(views)
    info = {}
    can = rs.stitch_ring(views, projection="cylindrical", focal="auto", wrap=True, pairs="ring", adjust="cameras", features={"ratio": 0.7},
                             info=info)
    assert info["pairs"] == [(i + 1, i) for i in range(n - 1)] + [(0, n - 1)]
    print("focal %.3f (true 400), period %d, matches %s, inliers %s, canvas %d x %d"
          % (info["focal"], info["period"], info["sizes"], info["inliers"], can.shape[0], can.shape[1]))
    assert np.asarray(info["accepted"]).all()
    assert info["period"] == hg.sequence_period(info["focal"]) == can.shape[1] and info["radius"] == info["period"] / (2.0 * np.pi)
    assert isinstance(can, np.ndarray)
    assert np.array_equal(can, hg.stitchSequence(views, Gs=info["Gs"], projection="cylindrical", focal=info["focal"], wrap=True))
    assert info["origin"][0] == -info["period"] // 2 and 0 <= -info["origin"][1] < can.shape[0]
    assert can[-info["origin"][1]].any(axis=1).all()
