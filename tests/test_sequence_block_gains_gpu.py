"""The block gain rule on the GPU: rwh_sequence_cell_stats and the map-taking compositors against their host twins (which
tests/test_sequence_block_gains_cpu.py holds to the numpy restatement), on the smallest shapes that reach each edge of the cell
kernel and on canvases that cross the compositors' launch edges, then the Python layers above them.  Every comparison is exact."""
import numpy as np
import pytest

import block_gain_cases as bg
import gain_cases as gc
import projection_cases as pc
import sequence_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return sc.library(gpu=True)


def _tables(name):
    if name == "cylinder":
        images, Gs, kind, f = bg.cylinder_case()
        return images, pc.tables(images, Gs, 0, kind, f)
    if name == "wide cylinder":
        return pc.wide_case("cylindrical")
    images, Gs = getattr(bg, name)()
    return images, sc.tables(images, Gs, 0)


# partial cells at B = 16 under strides 1, 3 and 17 (17 > B: cells without a sample); a canvas narrower than one cell; cells without a
# candidate; K = 64 on one cell (the full LDS table); B = 128 on a 130 x 130 canvas (sixteen passes of 1024 samples, the largest
# sums, and cells one pixel wide); a cylindrical canvas; a canvas of more than 32 cells across
CELL_CASES = [("partial_cells", 16, 1), ("partial_cells", 16, 3), ("partial_cells", 16, 17), ("partial_cells", 32, 1), ("partial_cells", 64, 2),
              ("narrow_canvas", 16, 1), ("narrow_canvas", 64, 3), ("empty_cell", 16, 1), ("sixty_four_on_one_cell", 16, 1),
              ("sixty_four_on_one_cell", 32, 3), ("big_cell", 128, 1), ("big_cell", 128, 3), ("big_cell", 16, 1), ("cylinder", 16, 1),
              ("cylinder", 16, 3), ("cylinder", 32, 17), ("wide cylinder", 16, 1)]


@pytest.mark.parametrize("name,B,stride", CELL_CASES, ids=["%s-B%d-s%d" % c for c in CELL_CASES])
def test_device_cells_are_the_host_twin_between_canaries(lib, name, B, stride):
    images, t = _tables(name)
    want = bg.hcells(lib, t, images, B, stride)
    got = bg.device_cells_guarded(lib, t, images, B, stride)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert want[:, :, 0].any()


def test_the_launcher_returns_the_same_table_in_one_tensor(lib):
    import torch
    for name, B, stride in (("partial_cells", 16, 3), ("cylinder", 32, 1), ("sixty_four_on_one_cell", 16, 1)):
        images, t = _tables(name)
        on = sc.upload(images)
        from ransac_with_homography_amd import kernels
        tabs = kernels.sequence_cell_tables_on(on, bg.geometry(t), B, stride)
        K = bg.slots(lib, t, B)
        assert isinstance(tabs, torch.Tensor) and tabs.is_cuda and tabs.dtype == torch.int32 and tuple(tabs.shape) == bg.grid(t["size"], B) + (2, K, K)
        assert np.array_equal(tabs.cpu().numpy().view(np.uint32), bg.hcells(lib, t, images, B, stride))
        assert kernels.sequence_cell_slots(bg.geometry(t), t["n"], B) == K


def test_a_second_call_writes_the_table_whole(lib):
    """The device table starts as 0xA5 bytes in every call of the guarded driver, empty cells and unused ranks included."""
    images, t = _tables("empty_cell")
    got = bg.device_cells_guarded(lib, t, images, 16, 1)
    cands, _ = bg.candidates(t, 16)
    empty = [(gy, gx) for gy, row in enumerate(cands) for gx, c in enumerate(row) if not c]
    assert empty and all(not got[gy, gx].any() for gy, gx in empty)


# ---- the compositors on maps ----
KINDS = [("sequence", sc.PASTE, False), ("sequence", sc.FEATHER, False), ("labels", 0, True), ("multiband", 0, False), ("multiband", 0, True)]
KIND_IDS = ["paste", "feather", "label paste", "multiband", "multiband labels"]
EDGES = sc.edge_canvases()


@pytest.mark.parametrize("what,blend,labelled", KINDS, ids=KIND_IDS)
def test_compositors_with_maps_are_the_host_twin_across_launch_edges(lib, what, blend, labelled):
    """sc.edge_canvases(): canvases of 5 .. 1030 columns and 2 .. 6 rows, with non-constant maps of 16 x 16 cells.  The row-range
    cases (one row launched) belong to paste and feather, which alone take a row range; the others composite the whole canvas."""
    for fw, fh, images, Gs, order, rows in EDGES:
        t = sc.tables(images, Gs, 0, order)
        maps = bg.wavy_maps(t["n"], t["size"], 16, seed=fw + fh)
        labels = bg.stripes(t["size"], t["n"], seed=fw) if labelled else None
        rows = rows if what == "sequence" else None
        want = bg.hcanvas(lib, what, t, images, maps, 16, blend=blend, labels=labels, bands=2, rows=rows)
        got = bg.device_canvas(what, t, images, maps, 16, blend=blend, labels=labels, bands=2, rows=rows)
        assert np.array_equal(got, want), (fw, fh)


@pytest.mark.parametrize("what,blend,labelled", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name,B", [("wide cylinder", 16), ("wide cylinder", 128), ("cylinder", 32), ("partial_cells", 64)])
def test_compositors_with_maps_are_the_host_twin(lib, name, B, what, blend, labelled):
    images, t = _tables(name)
    maps = bg.wavy_maps(t["n"], t["size"], B, seed=B)
    labels = bg.stripes(t["size"], t["n"], seed=9) if labelled else None
    want = bg.hcanvas(lib, what, t, images, maps, B, blend=blend, labels=labels, bands=2)
    got = bg.device_canvas(what, t, images, maps, B, blend=blend, labels=labels, bands=2)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, bg.hcanvas(lib, what, t, images, np.ones_like(maps), B, blend=blend, labels=labels, bands=2))


# ---- the Python layers ----
def _host_tables(hg, images, Hs, anchor=0, projection=None, focal=None):
    """The tables of block_gain_cases' drivers from homography's own geometry (the pinned six-tuple of _sequence_inputs)."""
    rects, origin, size, default, mats, rays = hg._sequence_inputs("test", images, Hs, None, anchor, projection, focal)
    n = len(images)
    t = dict(hw=np.array([[im.shape[0], im.shape[1]] for im in images], dtype=np.int32), rects=np.array(rects, dtype=np.int32),
             order=np.array(default, dtype=np.int32), origin=tuple(origin), size=tuple(int(v) for v in size), n=n, anchor=anchor)
    if rays is None:
        t["inv"] = np.ascontiguousarray(np.asarray(mats).reshape(n, 9))
    else:
        t["m"], t["col"], t["row"] = np.ascontiguousarray(np.asarray(mats).reshape(n, 9)), np.ascontiguousarray(rays[0]), np.ascontiguousarray(rays[1])
    return t


def _host_blocks(lib, t, images, block=32, stride=1, base="auto", smooth=2, sigma_n=10.0):
    """sequence_block_gains on the host twins alone -> (base, maps)."""
    images = [np.ascontiguousarray(im) for im in images]
    n = t["n"]
    if isinstance(base, str):
        _, count, total, _ = gc.guarded_tables(n)
        ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
        st = getattr(lib, "rwh_host_sequence_overlap_stats" + bg.form(t))(*bg.layout(t, ptrs, (), t["size"], (4, count.ctypes.data, total.ctypes.data)))
        assert st == 0
        st, base = gc.host_gains(lib, count, total)
        assert st == 0
    elif base is None:
        base = np.ones(n)
    base = np.asarray(base, dtype=np.float64)
    return base, bg.hmaps(lib, bg.hcells(lib, t, images, block, stride), t, block, base, sigma_n, 0.1, smooth)


def test_sequence_block_gains_is_the_host_path(lib):
    from ransac_with_homography_amd import homography as hg
    images, Gs = bg.vignetted_scene()
    Hs = [sc.translate(80, 0), sc.translate(80, 0)]
    t = _host_tables(hg, images, Hs)
    for kw in (dict(), dict(block=16, stride=3, smooth=0, base=None), dict(block=64, base=[0.9, 1.0, 1.2], sigma_n=5.0, smooth=4)):
        info = {}
        got = hg.sequence_block_gains(images, Hs=Hs, info=info, **kw)
        base, maps = _host_blocks(lib, t, images, **kw)
        assert isinstance(got, hg.BlockGains) and got.block == kw.get("block", 32)
        assert isinstance(got.maps, np.ndarray) and got.maps.dtype == np.float64 and np.array_equal(got.maps, maps)
        assert np.array_equal(got.base, base)
        assert info["slots"] == bg.slots(lib, t, got.block) and np.array_equal(info["tables"], bg.hcells(lib, t, images, got.block, kw.get("stride", 1)))
    # on a cylinder
    views, Hs = pc.scene_views()
    f = hg.sequence_focal([v.shape for v in views], Hs)
    t = _host_tables(hg, views, Hs, 0, "cylindrical", f)
    got = hg.sequence_block_gains(views, Hs=Hs, projection="cylindrical", focal=f)
    base, maps = _host_blocks(lib, t, views)
    assert np.array_equal(got.maps, maps) and np.array_equal(got.base, base)


@pytest.mark.parametrize("blending,seams", [(False, None), ("feather", None), ("multiband", None), (False, True), ("multiband", True)],
                         ids=["paste", "feather", "multiband", "seams", "multiband seams"])
def test_stitch_sequence_with_blocks_is_the_host_path(lib, blending, seams):
    import torch
    import seam_cases as smc
    from ransac_with_homography_amd import homography as hg
    images, _ = bg.vignetted_scene()
    Hs = [sc.translate(80, 0), sc.translate(80, 0)]
    t = _host_tables(hg, images, Hs)
    base, maps = _host_blocks(lib, t, images)
    labels = None
    if seams:
        st, labels = smc.host_twin(lib, images, sc.chain(Hs, 0), 0, gains=base)              # the survey keeps one gain per image: base
        assert st == 0
    what = "multiband" if blending == "multiband" else "labels" if seams else "sequence"
    want = bg.hcanvas(lib, what, t, images, maps, 32, blend=sc.FEATHER if blending == "feather" else sc.PASTE, labels=labels, bands=3)
    info = {}
    got = hg.stitchSequence(images, Hs=Hs, gains="blocks", blending=blending, seams=seams, bands=3, info=info)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    used = info["gains"]
    assert isinstance(used, hg.BlockGains) and used.block == 32 and np.array_equal(used.maps, maps) and np.array_equal(used.base, base)
    if seams:
        assert np.array_equal(info["labels"], labels)
    # the BlockGains given back composites the same canvas, from tensors too
    again = hg.stitchSequence([torch.from_numpy(im).cuda() for im in images], Hs=Hs, gains=used, blending=blending, seams=labels, bands=3)
    assert isinstance(again, torch.Tensor) and np.array_equal(again.cpu().numpy(), want)
    assert not np.array_equal(want, hg.stitchSequence(images, Hs=Hs, gains=used.base, blending=blending, seams=labels, bands=3))


def test_stitch_sequence_with_blocks_on_a_cylinder(lib):
    from ransac_with_homography_amd import homography as hg
    views, Hs = pc.scene_views()
    f = hg.sequence_focal([v.shape for v in views], Hs)
    t = _host_tables(hg, views, Hs, 0, "cylindrical", f)
    _, maps = _host_blocks(lib, t, views)
    for blending, what in ((False, "sequence"), ("multiband", "multiband")):
        got = hg.stitchSequence(views, Hs=Hs, gains="blocks", blending=blending, bands=2, projection="cylindrical", focal=f)
        assert np.array_equal(got, bg.hcanvas(lib, what, t, views, maps, 32, bands=2))


def test_sequence_seams_takes_the_base_of_block_gains(lib):
    from ransac_with_homography_amd import homography as hg
    images, _ = bg.vignetted_scene()
    Hs = [sc.translate(80, 0), sc.translate(80, 0)]
    blocks = hg.sequence_block_gains(images, Hs=Hs)
    assert np.array_equal(hg.sequence_seams(images, Hs=Hs, gains=blocks), hg.sequence_seams(images, Hs=Hs, gains=blocks.base))


def test_pipeline_passes_blocks_through(lib):
    import ransac as rs
    from ransac_with_homography_amd import homography as hg
    scene = sc.scene()
    crops = [np.ascontiguousarray(scene[:, x:x + 260]) for x in (0, 90, 180)]      # test_sequence_gpu's crops: known to register
    before = [c.copy() for c in crops]
    info = {}
    can = rs.stitch_sequence(crops, th=5, gains="blocks", info=info)
    used = info["gains"]
    assert isinstance(can, np.ndarray) and isinstance(used, hg.BlockGains) and used.block == 32
    t = _host_tables(hg, crops, info["Hs"])
    base, maps = _host_blocks(lib, t, crops)
    assert np.array_equal(used.maps, maps) and np.array_equal(used.base, base)
    assert np.array_equal(can, bg.hcanvas(lib, "sequence", t, crops, maps, 32))
    assert np.array_equal(can, hg.stitchSequence(crops, Hs=info["Hs"], gains=used))
    assert all(np.array_equal(a, b) for a, b in zip(crops, before))
