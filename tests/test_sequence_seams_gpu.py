"""The seam rule on the GPU: rwh_sequence_seams and the two compositors that take labels against their host twins, across the
launch and tile edges, through a corridor that forces the relaxation to carry distances from tile to tile, with 64 images in one
launch, into a dirty workspace and on a second stream, and through the Python layers.  Every comparison is exact; the label plane
and the canvas sit between canaries."""
import numpy as np
import pytest

import gain_cases as gc
import projection_cases as pc
import seam_cases as sm
import sequence_cases as sc

pytestmark = pytest.mark.gpu

TH = 5


@pytest.fixture(scope="module")
def lib():
    return sc.library(gpu=True)


EDGES = sc.edge_canvases()
GENERAL = sc.general_cases()
PROJECTED = [(kind,) + pc.general_cases()[1] for kind in pc.SURFACES]


# ---- device equals host twin ----
@pytest.mark.parametrize("case", EDGES, ids=["fw%d-fh%d" % (c[0], c[1]) for c in EDGES])
def test_device_is_the_host_twin_across_launch_edges(lib, case):
    _, _, images, Gs, _, _ = case
    dev = sc.upload(images)
    for gains in (None, gc.mixed_gains(len(images))):
        assert np.array_equal(sm.device(lib, images, Gs, 0, gains, 2.0, on=dev), sm.host(lib, images, Gs, 0, gains, 2.0))


@pytest.mark.parametrize("case", GENERAL, ids=[c[0].replace(" ", "-") for c in GENERAL])
def test_device_is_the_host_twin_on_general_cases(lib, case):
    _, images, Gs, anchor, _ = case
    dev = sc.upload(images)
    for gains in (None, gc.mixed_gains(len(images))):
        for margin, tau in ((sm.MARGIN, sm.TAU), (2.0, 200), (np.inf, 64)):
            got = sm.device(lib, images, Gs, anchor, gains, margin, tau, on=dev)
            assert np.array_equal(got, sm.host(lib, images, Gs, anchor, gains, margin, tau)), (margin, tau)


@pytest.mark.parametrize("case", PROJECTED, ids=[c[0] for c in PROJECTED])
def test_device_is_the_host_twin_on_a_curved_canvas(lib, case):
    kind, _, images, Gs, anchor, _, f = case
    for gains in (None, gc.mixed_gains(len(images))):
        assert np.array_equal(sm.device_proj(images, Gs, anchor, kind, f, gains, 3.0), sm.host_proj(lib, images, Gs, anchor, kind, f, gains, 3.0))


def test_windows_and_canvases_of_a_tile_plus_minus_one(lib):
    from ransac_with_homography_amd import _lib
    assert (sm.TILE_W, sm.TILE_H) == (_lib.RWH_SEAM_TILE_W, _lib.RWH_SEAM_TILE_H)
    for w, h, images, Gs in sm.tile_window_cases():
        want = sm.host(lib, images, Gs, 0, margin=2.0)
        assert set(np.unique(want)) == {0, 1, sm.NONE}, (w, h)
        assert np.array_equal(sm.device(lib, images, Gs, 0, margin=2.0), want), (w, h)
    for fw, fh, images, Gs in sm.tile_canvas_cases():
        want = sm.host(lib, images, Gs, 0, margin=2.0)
        assert set(np.unique(want)) == {0, 1, sm.NONE}, (fw, fh)          # (the first row's last 10 pixels are nobody's)
        assert np.array_equal(sm.device(lib, images, Gs, 0, margin=2.0), want), (fw, fh)


def test_the_serpentine_is_carried_from_tile_to_tile(lib):
    """Distances have to travel along a corridor of 3040 pixels through 24 tiles, back into tiles that were already done
    (tests/test_sequence_seams_cpu.py checks the scene on the restatement): one pass cannot do it."""
    images, Gs, path = sm.serpentine()
    info = {}
    got = sm.device(lib, images, Gs, 0, margin=0.0, tau=sm.SERPENTINE_TAU, info=info)
    print("serpentine: %d passes" % info["passes"])
    assert np.array_equal(got, sm.host(lib, images, Gs, 0, margin=0.0, tau=sm.SERPENTINE_TAU))
    assert info["passes"] > 1


def test_a_moving_object_and_a_three_way_overlap(lib):
    images, Gs, block = sm.moving_object()
    got = sm.device(lib, images, Gs, 0)
    assert np.array_equal(got, sm.host(lib, images, Gs, 0)) and len(np.unique(got[block])) == 1
    images, Gs = sm.three_way()
    assert np.array_equal(sm.device(lib, images, Gs, 0), sm.host(lib, images, Gs, 0))


def test_sixty_four_images_in_one_launch(lib):
    images, Gs = sc.translated_strip(64)
    for margin in (1.0, sm.MARGIN):
        got = sm.device(lib, images, Gs, 0, margin=margin)
        assert np.array_equal(got, sm.host(lib, images, Gs, 0, margin=margin))
    assert len(np.unique(sm.device(lib, images, Gs, 0, gc.mixed_gains(64), 1.0))) == 65


def test_the_call_does_not_depend_on_what_the_workspace_held(lib):
    """The strip of 64 twice into one workspace, another case's planes left in it in between."""
    import torch
    images, Gs = sc.translated_strip(64)
    other, oG, _ = sm.serpentine()
    want = sm.host(lib, images, Gs, 0, margin=1.0)
    need = max(sm.workspace_bytes(lib, sc.tables(images, Gs, 0)), sm.workspace_bytes(lib, sc.tables(other, oG, 0)))
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    dev = sc.upload(images)
    assert np.array_equal(sm.device(lib, images, Gs, 0, margin=1.0, on=dev, workspace=ws), want)
    assert np.array_equal(sm.device(lib, other, oG, 0, margin=0.0, tau=sm.SERPENTINE_TAU, workspace=ws),
                          sm.host(lib, other, oG, 0, margin=0.0, tau=sm.SERPENTINE_TAU))
    assert np.array_equal(sm.device(lib, images, Gs, 0, margin=1.0, on=dev, workspace=ws), want)
    assert (ws[need:].cpu().numpy() == 0xA5).all(), "a byte beyond the workspace's stated size was written"


def test_on_a_second_stream(lib):
    import torch
    images, Gs = sm.three_way()
    assert np.array_equal(sm.device(lib, images, Gs, 0, stream=torch.cuda.Stream()), sm.host(lib, images, Gs, 0))


def test_both_forms_on_a_second_stream_after_a_dirty_workspace(lib):
    """The two seam entry points synchronise and cannot be captured (tests/stream_contract_cases.py exempts them); what can be held:
    on a side stream, into a workspace that holds another fill and then their own leftovers, the labels are the host twin's."""
    import ctypes
    import torch
    import projection_cases as pc
    side = torch.cuda.Stream()
    images, Gs = sm.three_way()
    need = sm.workspace_bytes(lib, sc.tables(images, Gs, 0))
    ws = torch.full((need + 4096,), 0x3C, dtype=torch.uint8, device="cuda")
    ws[need:].fill_(0xA5)
    torch.cuda.synchronize()
    for _ in range(2):
        assert np.array_equal(sm.device(lib, images, Gs, 0, workspace=ws[:need], stream=side), sm.host(lib, images, Gs, 0))
    assert (ws[need:].cpu().numpy() == 0xA5).all(), "a byte beyond the workspace's stated size was written"
    images, Hs = pc.sweep(3, 3)
    Gs = sc.chain(Hs, 0)
    t = pc.tables(images, Gs, 0, "cylindrical", 40.0)
    fh, fw = t["size"]
    want = sm.host_proj(lib, images, Gs, 0)
    need = lib.rwh_sequence_seams_workspace_bytes(t["rects"].ctypes.data, t["n"], fh, fw, 0, 0)
    assert need > 0
    ws = torch.full((need + 4096,), 0x3C, dtype=torch.uint8, device="cuda")
    ws[need:].fill_(0xA5)
    dev = sc.upload(images)
    ptrs = np.array([d.data_ptr() for d in dev], dtype=np.uint64)
    col, row = pc.device_tables(t)
    for _ in range(2):
        lab, fetch = sm.guarded_device_plane(fh, fw)
        passes = ctypes.c_int32(0)
        torch.cuda.synchronize()
        st = lib.rwh_sequence_seams_proj(ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, t["n"], None,
                                         float(sm.MARGIN), int(sm.TAU), col.data_ptr(), row.data_ptr(), lab.data_ptr(), fh, fw,
                                         ws.data_ptr(), need, side.cuda_stream, ctypes.addressof(passes))
        assert st == 0
        side.synchronize()
        assert np.array_equal(fetch(), want) and passes.value >= 1
    assert (ws[need:].cpu().numpy() == 0xA5).all(), "a byte beyond the workspace's stated size was written"


def test_a_bad_workspace_or_option_is_refused_and_nothing_written(lib):
    import torch
    images, Gs = sc.translated_strip(3)
    t = sc.tables(images, Gs, 0)
    fh, fw = t["size"]
    dev = sc.upload(images)
    ptrs = np.array([d.data_ptr() for d in dev], dtype=np.uint64)
    need = sm.workspace_bytes(lib, t)
    ws = torch.zeros((need + 8,), dtype=torch.uint8, device="cuda")
    lab = torch.full((fh, fw), 0xA5, dtype=torch.uint8, device="cuda")

    def call(wp, wb, margin=8.0, tau=64, lp=lab.data_ptr()):
        return lib.rwh_sequence_seams(ptrs.ctypes.data, t["hw"].ctypes.data, t["inv"].ctypes.data, t["rects"].ctypes.data, 3, 0, None, margin, tau,
                                      lp, fh, fw, 0, 0, wp, wb, torch.cuda.current_stream().cuda_stream, None)
    assert call(ws.data_ptr(), need - 1) == -1 and call(ws.data_ptr() + 4, need) == -1 and call(None, need) == -1
    assert call(ws.data_ptr(), need, tau=0) == -1 and call(ws.data_ptr(), need, tau=767) == -1
    assert call(ws.data_ptr(), need, margin=-1.0) == -1 and call(ws.data_ptr(), need, margin=float("nan")) == -1
    assert call(ws.data_ptr(), need, lp=None) == -1
    torch.cuda.synchronize()
    assert (lab.cpu().numpy() == 0xA5).all(), "a refused call wrote the label plane"
    assert call(ws.data_ptr(), need) == 0                               # (passes may be NULL)
    torch.cuda.synchronize()
    assert np.array_equal(lab.cpu().numpy(), sm.host(lib, images, Gs, 0))


# ---- the compositors that take labels ----
def test_label_paste_and_labelled_multiband_are_their_host_twins(lib):
    from ransac_with_homography_amd import kernels
    for name, images, Gs, anchor, _ in GENERAL[1:5]:
        t = sc.tables(images, Gs, anchor)
        dev = sc.upload(images)
        for gains in (None, gc.mixed_gains(len(images))):
            lab = sm.host(lib, images, Gs, anchor, gains, 2.0)
            can, fetch = sc.guarded_device_canvas(*t["size"])
            kernels.stitch_sequence_labels(dev, t["inv"], t["rects"], anchor, t["origin"], t["size"], lab, gains=gains, out=can)
            assert np.array_equal(fetch(), sm.host_paste(lib, images, Gs, lab, anchor, gains)[1]), name
            can, fetch = sc.guarded_device_canvas(*t["size"])
            kernels.stitch_sequence_multiband_labels(dev, t["inv"], t["rects"], anchor, t["origin"], t["size"], 3, lab, gains=gains, out=can)
            assert np.array_equal(fetch(), sm.host_multiband(lib, images, Gs, lab, anchor, 3, gains)[1]), name
        junk = np.random.default_rng(3).integers(0, 256, t["size"]).astype(np.uint8)      # labels out of range index nothing
        can, fetch = sc.guarded_device_canvas(*t["size"])
        kernels.stitch_sequence_multiband_labels(dev, t["inv"], t["rects"], anchor, t["origin"], t["size"], 2, junk, out=can)
        assert np.array_equal(fetch(), sm.host_multiband(lib, images, Gs, junk, anchor, 2)[1]), name


def test_labelled_compositors_on_a_curved_canvas(lib):
    from ransac_with_homography_amd import kernels
    kind, _, images, Gs, anchor, _, f = PROJECTED[1]
    t = pc.tables(images, Gs, anchor, kind, f)
    col, row = pc.device_tables(t)
    dev = sc.upload(images)
    lab = sm.host_proj(lib, images, Gs, anchor, kind, f, None, 3.0)
    can, fetch = sc.guarded_device_canvas(*t["size"])
    kernels.stitch_sequence_labels_proj(dev, t["m"], t["rects"], col, row, t["size"], lab, out=can)
    assert np.array_equal(fetch(), sm.host_paste_proj(lib, images, Gs, lab, anchor, kind, f))
    can, fetch = sc.guarded_device_canvas(*t["size"])
    kernels.stitch_sequence_multiband_labels_proj(dev, t["m"], t["rects"], col, row, t["size"], 2, lab, out=can)
    assert np.array_equal(fetch(), sm.host_multiband_proj(lib, images, Gs, lab, anchor, kind, f, 2))


# ---- the Python layers ----
def test_stitch_sequence_with_seams_numpy_and_tensors(lib):
    import torch
    import homography as hg
    images, Gs, block = sm.moving_object()
    lab = sm.host(lib, images, Gs, 0)
    g = np.array([1.2, 0.9])
    lab_g = sm.host(lib, images, Gs, 0, g)
    info = {}
    got = hg.sequence_seams(images, Gs=Gs, info=info)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, lab) and info["passes"] >= 1
    for blending, want, want_g in ((False, sm.host_paste(lib, images, Gs, lab)[1], sm.host_paste(lib, images, Gs, lab_g, 0, g)[1]),
                                   ("multiband", sm.host_multiband(lib, images, Gs, lab, 0, 3)[1], sm.host_multiband(lib, images, Gs, lab_g, 0, 3, g)[1])):
        info = {}
        got = hg.stitchSequence(images, Gs=Gs, blending=blending, seams=True, bands=3, info=info)
        assert isinstance(got, np.ndarray) and np.array_equal(got, want), blending
        assert np.array_equal(info["labels"], lab) and info["passes"] >= 1
        dev = sc.upload(images)
        keep = [d.clone() for d in dev]
        out = hg.stitchSequence(dev, Gs=Gs, blending=blending, seams={"margin": 8.0, "tau": 64}, bands=3)
        assert isinstance(out, torch.Tensor) and out.is_cuda and np.array_equal(out.cpu().numpy(), want), blending
        assert all(torch.equal(a, b) for a, b in zip(dev, keep))
        assert np.array_equal(hg.stitchSequence(images, Gs=Gs, blending=blending, seams=lab, bands=3), want)
        assert np.array_equal(hg.stitchSequence(images, Gs=Gs, blending=blending, seams=True, bands=3, gains=g), want_g)
    t = hg.sequence_seams(sc.upload(images), Gs=Gs, margin=np.inf)
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy(), sm.host(lib, images, Gs, 0, margin=np.inf))


def test_stitch_sequence_with_seams_on_a_curved_canvas(lib):
    import homography as hg
    kind, _, images, Gs, anchor, _, f = PROJECTED[0]
    lab = sm.host_proj(lib, images, Gs, anchor, kind, f)
    assert np.array_equal(hg.sequence_seams(images, Gs=Gs, anchor=anchor, projection=kind, focal=f), lab)
    got = hg.stitchSequence(images, Gs=Gs, anchor=anchor, projection=kind, focal=f, blending="multiband", bands=2, seams=True)
    assert np.array_equal(got, sm.host_multiband_proj(lib, images, Gs, lab, anchor, kind, f, 2))
    got = hg.stitchSequence(images, Gs=Gs, anchor=anchor, projection=kind, focal=f, seams=True)
    assert np.array_equal(got, sm.host_paste_proj(lib, images, Gs, lab, anchor, kind, f))


def test_pipeline_on_three_crops_of_one_scene(lib):
    import homography as hg
    import ransac as rs
    scene = sc.scene()
    crops = [np.ascontiguousarray(scene[:, x:x + 260]) for x in (0, 90, 180)]
    info = {}
    can = rs.stitch_sequence(crops, th=TH, blending="multiband+seams", bands=3, info=info)
    assert isinstance(can, np.ndarray) and info["Hs"].shape == (2, 3, 3) and info["passes"] >= 1
    assert np.array_equal(can, hg.stitchSequence(crops, Hs=info["Hs"], blending="multiband", seams=True, bands=3))
    Gs = hg.sequence_plan([c.shape for c in crops], info["Hs"])[0]
    assert np.array_equal(can, sm.host_multiband(lib, crops, Gs, info["labels"], 0, 3)[1])
    pasted = rs.stitch_sequence(crops, th=TH, blending="seams", info=info)
    assert np.array_equal(pasted, hg.stitchSequence(crops, Hs=info["Hs"], seams=True))
