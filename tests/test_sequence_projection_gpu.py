"""The projection rule on the GPU: the projected forms of the compositor, the overlap statistics and the multi-band head against
their host twins (which tests/test_sequence_projection_cpu.py holds to the numpy restatement) on canvases that cross every launch
edge, the Python layers above them, and the pipeline entry ransac.stitch_sequence(projection=...).  Every comparison is exact, and
every device canvas lies between canaries."""
import numpy as np
import pytest

import gain_cases as gc
import projection_cases as pc
import sequence_cases as sc

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 255, 256, 257, 259, 513)      # the 256 x 4 tile with four pixels per lane
HEIGHTS = (1, 4, 5, 9)


@pytest.fixture(scope="module")
def lib():
    return sc.library(gpu=True)


@pytest.fixture(scope="module")
def wide():
    return {kind: pc.wide_case(kind) for kind in pc.SURFACES}


@pytest.mark.parametrize("kind", pc.SURFACES)
@pytest.mark.parametrize("fw", WIDTHS)
def test_launch_edges(lib, wide, kind, fw):
    """Windows of one wide canvas, fw columns by each of HEIGHTS rows: paste and feather, with and without gains."""
    images, whole = wide[kind]
    for fh in HEIGHTS:
        ims, t = pc.crop(images, whole, 200 if fw < 300 else 60, 4, fw, fh)      # (columns 175 .. 263: two images meet)
        on = sc.upload(ims)
        for blend in (pc.PASTE, pc.FEATHER):
            for gains in (None, gc.mixed_gains(len(ims))):
                st, want = pc.host_twin(lib, ims, None, blend=blend, gains=gains, t=t)
                assert st == 0
                assert np.array_equal(pc.device(ims, None, blend=blend, gains=gains, on=on, t=t), want), (fh, blend, gains)
    assert want.any()


@pytest.mark.parametrize("kind", pc.SURFACES)
def test_row_ranges_that_cut_a_tile(lib, wide, kind):
    images, whole = wide[kind]
    ims, t = pc.crop(images, whole, 100, 1, 259, 9)
    on = sc.upload(ims)
    for rows in ((0, 1), (1, 2), (3, 6), (4, 9), (2, 8), (6, 6)):
        for blend in (pc.PASTE, pc.FEATHER):
            st, want = pc.host_twin(lib, ims, None, blend=blend, rows=rows, t=t)
            assert st == 0
            assert np.array_equal(pc.device(ims, None, blend=blend, rows=rows, on=on, t=t), want), (rows, blend)


@pytest.mark.parametrize("kind", pc.SURFACES)
def test_general_cases(lib, kind):
    for _, images, Gs, anchor, order, f in pc.general_cases():
        for blend in (pc.PASTE, pc.FEATHER):
            assert np.array_equal(pc.device(images, Gs, anchor, kind, f, blend, order), pc.host(lib, images, Gs, anchor, kind, f, blend, order))


@pytest.mark.parametrize("kind", pc.SURFACES)
def test_sixty_four_images(lib, kind):
    """64 images of 12 x 16, f = 200, 0.02 rad apart: the descriptor table takes two put launches."""
    images, Gs = pc.strip(64, 12, 16, 200.0, 0.02)
    on = sc.upload(images)
    gains = gc.mixed_gains(64)
    assert np.array_equal(pc.device(images, Gs, 0, kind, 200.0, pc.PASTE, on=on), pc.host(lib, images, Gs, 0, kind, 200.0, pc.PASTE))
    assert np.array_equal(pc.device(images, Gs, 0, kind, 200.0, pc.FEATHER, gains=gains, on=on), pc.host(lib, images, Gs, 0, kind, 200.0, pc.FEATHER, gains=gains))
    count, total = pc.device_stats(images, Gs, 0, kind, 200.0, 4)
    want = pc.host_stats(lib, images, Gs, 0, kind, 200.0, 4)
    assert np.array_equal(count, want[0]) and np.array_equal(total, want[1])


def test_forty_images_meet_one_tile(lib):
    images, Gs = pc.strip(40, 6, 30, 300.0, 5.0 / 300.0, pitch=0.0001)
    t = pc.tables(images, Gs, 0, "cylindrical", 300.0)
    assert t["size"][1] <= 256
    assert ((t["rects"][:, 1] < 4) & (t["rects"][:, 1] + t["rects"][:, 3] > 0)).all()       # every rectangle meets the first tile
    for blend in (pc.PASTE, pc.FEATHER):
        assert np.array_equal(pc.device(images, Gs, 0, "cylindrical", 300.0, blend), pc.host(lib, images, Gs, 0, "cylindrical", 300.0, blend))
    count, total = pc.device_stats(images, Gs, 0, "cylindrical", 300.0, 1)
    want = pc.host_stats(lib, images, Gs, 0, "cylindrical", 300.0, 1)
    assert np.array_equal(count, want[0]) and np.array_equal(total, want[1])
    assert (count > 0).sum() > 40 * 5


@pytest.mark.parametrize("kind", pc.SURFACES)
@pytest.mark.parametrize("stride", (1, 4))
def test_overlap_tables(lib, kind, stride):
    for _, images, Gs, anchor, _, f in pc.general_cases():
        count, total = pc.device_stats(images, Gs, anchor, kind, f, stride)
        want = pc.host_stats(lib, images, Gs, anchor, kind, f, stride)
        assert np.array_equal(count, want[0]) and np.array_equal(total, want[1])


@pytest.mark.parametrize("kind", pc.SURFACES)
@pytest.mark.parametrize("bands", (1, 3))
def test_multiband(lib, kind, bands):
    for _, images, Gs, anchor, _, f in pc.general_cases():
        for gains in (None, gc.mixed_gains(len(images))):
            assert np.array_equal(pc.device_multiband(images, Gs, anchor, kind, f, bands, gains), pc.host_multiband(lib, images, Gs, anchor, kind, f, bands, gains))
    images, Gs = pc.strip(12, 12, 70, 200.0, 0.1)                    # several blocks wide
    assert np.array_equal(pc.device_multiband(images, Gs, 0, kind, 200.0, bands), pc.host_multiband(lib, images, Gs, 0, kind, 200.0, bands))


def test_a_second_stream(lib):
    import torch
    _, images, Gs, anchor, order, f = pc.general_cases()[4]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = pc.device(images, Gs, anchor, "spherical", f, pc.FEATHER, gains=gc.mixed_gains(5))
        band = pc.device_multiband(images, Gs, anchor, "spherical", f, 2)
        count, total = pc.device_stats(images, Gs, anchor, "spherical", f, 1)
    assert np.array_equal(got, pc.host(lib, images, Gs, anchor, "spherical", f, pc.FEATHER, gains=gc.mixed_gains(5)))
    assert np.array_equal(band, pc.host_multiband(lib, images, Gs, anchor, "spherical", f, 2))
    want = pc.host_stats(lib, images, Gs, anchor, "spherical", f, 1)
    assert np.array_equal(count, want[0]) and np.array_equal(total, want[1])


def test_device_refusals_come_before_any_launch(lib):
    import torch
    from ransac_with_homography_amd import kernels
    _, images, Gs, anchor, order, f = pc.general_cases()[1]
    t = pc.tables(images, Gs, anchor, "cylindrical", f)
    col, row = pc.device_tables(t)
    on = sc.upload(images)
    can, fetch = sc.guarded_device_canvas(*t["size"])
    bad = t["m"].copy()
    bad[anchor, 8] = np.inf
    with pytest.raises(ValueError):
        kernels.stitch_sequence_proj(on, bad, t["rects"], col, row, t["order"], pc.PASTE, t["size"], out=can)
    with pytest.raises(ValueError):
        kernels.stitch_sequence_proj(on, t["m"], t["rects"], col[1:], row, t["order"], pc.PASTE, t["size"], out=can)
    with pytest.raises(ValueError):
        kernels.stitch_sequence_proj(on, t["m"], t["rects"], col.float(), row, t["order"], pc.PASTE, t["size"], out=can)
    with pytest.raises(ValueError):
        kernels.stitch_sequence_multiband_proj(on, bad, t["rects"], col, row, t["size"], 2, out=can)
    with pytest.raises(ValueError):
        kernels.sequence_overlap_tables_proj(on, bad, t["rects"], col, row, t["size"], 1)
    ptrs = np.array([d.data_ptr() for d in on], dtype=np.uint64)
    ws = torch.empty(1024, dtype=torch.int64, device="cuda")
    for c, r in ((0, row.data_ptr()), (col.data_ptr(), 0), (col.data_ptr() + 8, row.data_ptr())):        # NULL, NULL, misaligned
        st = lib.rwh_stitch_sequence_proj(ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, 3, t["order"].ctypes.data,
                                          pc.PASTE, c, r, can.data_ptr(), t["size"][0], t["size"][1], 0, t["size"][0], ws.data_ptr(), 8192, 0, None)
        assert st == -1
    torch.cuda.synchronize()
    assert (fetch() == 0xA5).all()


@pytest.mark.parametrize("kind", pc.SURFACES)
def test_stitch_sequence_arrays_and_tensors(lib, kind):
    import torch
    from ransac_with_homography_amd import homography as hg
    images, Hs = pc.sweep(4, 4, f=37.5)
    Gs = sc.chain(Hs, 1)
    before = [im.copy() for im in images]
    for blending, blend in ((False, pc.PASTE), ("feather", pc.FEATHER)):
        can = hg.stitchSequence(images, Hs=Hs, anchor=1, blending=blending, projection=kind, focal=37.5)
        assert isinstance(can, np.ndarray) and np.array_equal(can, pc.host(lib, images, Gs, 1, kind, 37.5, blend))
    ten = hg.stitchSequence([torch.from_numpy(im) for im in images], Gs=Gs, anchor=1, blending="feather", projection=kind, focal=37.5)
    assert isinstance(ten, torch.Tensor) and ten.is_cuda and np.array_equal(ten.cpu().numpy(), can)
    info = {}
    auto = hg.stitchSequence(images, Hs=Hs, anchor=1, blending="multiband", bands=2, gains="auto", info=info, projection=kind, focal=37.5)
    st, want = gc.host_gains(lib, *pc.host_stats(lib, images, Gs, 1, kind, 37.5, 4))
    assert st == 0 and np.array_equal(info["gains"], want)
    assert np.array_equal(info["gains"], hg.sequence_gains(images, Hs=Hs, anchor=1, projection=kind, focal=37.5))
    assert np.array_equal(auto, pc.host_multiband(lib, images, Gs, 1, kind, 37.5, 2, gains=want))
    assert all(np.array_equal(a, b) for a, b in zip(images, before))


def test_pipeline_on_rotated_views_of_one_scene(lib):
    """ransac.stitch_sequence on three rotated views of sc.scene() (true f = 400), cylindrical, focal="auto", gains="auto",
    multi-band: the canvas is stitchSequence of what the call reports.  How close info["focal"] comes to 400 on estimated
    homographies is printed (and kept in profiles/sequence_projection.txt), not asserted: nobody has measured it."""
    from ransac_with_homography_amd import homography as hg
    from ransac_with_homography_amd import ransac as rs
    views, true_hs = pc.scene_views()
    info = {}
    can = rs.stitch_sequence(views, projection="cylindrical", focal="auto", gains="auto", blending="multiband", bands=2, info=info)
    assert isinstance(can, np.ndarray) and info["Hs"].shape == (2, 3, 3) and info["gains"].shape == (3,)
    print("focal: estimated %.3f on the estimated homographies, %.6f on the true ones (true f = 400); matches %s, inliers %s; canvas %d x %d"
          % (info["focal"], hg.sequence_focal([v.shape for v in views], true_hs), info["sizes"], info["inliers"], can.shape[0], can.shape[1]))
    assert np.array_equal(can, hg.stitchSequence(views, Hs=info["Hs"], projection="cylindrical", focal=info["focal"], gains=info["gains"],
                                                 blending="multiband", bands=2))
    assert info["focal"] == hg.sequence_focal([v.shape for v in views], info["Hs"])
    plain = {}
    rs.stitch_sequence(views, info=plain)
    assert plain["focal"] is None
