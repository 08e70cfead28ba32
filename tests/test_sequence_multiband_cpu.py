"""The multi-band rule without a GPU: rwh_host_stitch_multiband (the host twin, which works in per-image windows) against the
numpy restatement of tests/multiband_cases.py (which holds every image's planes over the whole padded canvas), the rule's stated
consequences, what the blend is for, the refusals, and the Python layer's checks.  Every comparison is exact."""
import inspect

import numpy as np
import pytest

import gain_cases as gc
import multiband_cases as mc
import sequence_cases as sc


@pytest.fixture(scope="module")
def lib():
    return sc.library()


def paste(lib, images, Gs, anchor=0, gains=None):
    return sc.host_ex(lib, images, Gs, anchor, sc.PASTE, gains=gains)


GENERAL = sc.general_cases()
EDGES = sc.edge_canvases()


# ---- twin equals restatement ----
@pytest.mark.parametrize("bands", (1, 3, 5))
@pytest.mark.parametrize("case", GENERAL, ids=[c[0].replace(" ", "-") for c in GENERAL])
def test_twin_is_the_restatement_on_general_cases(lib, case, bands):
    _, images, Gs, anchor, _ = case
    assert np.array_equal(mc.host(lib, images, Gs, anchor, bands), mc.restate(images, Gs, anchor, bands))


@pytest.mark.parametrize("case", EDGES, ids=["fw%d-fh%d" % (c[0], c[1]) for c in EDGES])
def test_twin_is_the_restatement_on_edge_canvases(lib, case):
    _, _, images, Gs, _, _ = case
    for bands in (1, 2):
        assert np.array_equal(mc.host(lib, images, Gs, 0, bands), mc.restate(images, Gs, 0, bands)), bands


@pytest.mark.parametrize("bands", (1, 2))
def test_twin_is_the_restatement_on_a_strip_of_64(lib, bands):
    """An 18 x 331 canvas of 12 x 16 images: a per-image window that is too small shows here."""
    images, Gs = sc.translated_strip(64)
    assert np.array_equal(mc.host(lib, images, Gs, 0, bands), mc.restate(images, Gs, 0, bands))


def test_twin_is_the_restatement_with_gains(lib):
    for name, images, Gs, anchor, _ in GENERAL:
        g = gc.mixed_gains(len(images))
        assert np.array_equal(mc.host(lib, images, Gs, anchor, 3, g), mc.restate(images, Gs, anchor, 3, g)), name
    images, Gs = sc.translated_strip(64)
    g = gc.mixed_gains(64)
    assert np.array_equal(mc.host(lib, images, Gs, 0, 2, g), mc.restate(images, Gs, 0, 2, g))


def test_unit_gains_change_nothing(lib):
    for name, images, Gs, anchor, _ in GENERAL:
        assert np.array_equal(mc.host(lib, images, Gs, anchor, 3, np.ones(len(images))), mc.host(lib, images, Gs, anchor, 3)), name


def test_twin_is_the_restatement_where_windows_meet_tile_edges(lib):
    """The fixtures of the GPU tile-edge tests, on the host: the windows they aim at are the restatement's planes too."""
    for key, (images, Gs) in sorted(mc.tile_edge_cases().items()):
        assert np.array_equal(mc.host(lib, images, Gs, 0, mc.TILE_BANDS), mc.restate(images, Gs, 0, mc.TILE_BANDS)), key


def test_tile_edge_fixtures_exist():
    """The search finds a window of every tile width +- 1 at levels 1 .. 3 but the even ones that only a clipped window has, and of
    every height the margins allow."""
    found = set(mc.tile_edge_cases())
    for level in (1, 2, 3):
        assert {("x", level, s) for s in (31, 33, 63, 65)} <= found
    assert {("x", 3, s) for s in mc.TILE_WIDTHS} <= found and {("y", 3, s) for s in mc.TILE_HEIGHTS} <= found


# ---- the stated consequences ----
@pytest.mark.parametrize("bands", range(1, 9))
def test_one_image_is_paste(lib, bands):
    for img in (sc.random_image(9, 11, 1), sc.random_image(3, 5, 2), sc.random_image(70, 37, 3)):      # 3 x 5: smaller than 2^K from K = 3 on
        assert np.array_equal(mc.host(lib, [img], [np.eye(3)], 0, bands), paste(lib, [img], [np.eye(3)])), img.shape
        assert np.array_equal(mc.host(lib, [img], [np.eye(3)], 0, bands), img)


def test_identical_overlaps_are_paste(lib):
    images, Gs = gc.identical_overlaps()
    for bands in (1, 2, 3, 5):
        for anchor in (0, 1):
            G = [np.linalg.inv(Gs[anchor]) @ g for g in Gs]
            G[anchor] = np.eye(3)
            assert np.array_equal(mc.host(lib, images, G, anchor, bands), paste(lib, images, G, anchor)), (bands, anchor)


# ---- what the blend is for ----
def test_two_flat_images_give_a_monotone_ramp(lib):
    images, Gs = mc.flat_pair()
    row = paste(lib, images, Gs)[48, :, 0].astype(int)
    paste_step = int(np.abs(np.diff(row)).max())
    assert paste_step == 60
    steps = []
    for bands in (1, 2, 3, 4):
        can = mc.host(lib, images, Gs, 0, bands)
        row = can[48, :, 0].astype(int)
        assert (np.diff(row) >= 0).all() and row[0] == 100 and row[-1] == 160, bands
        assert (can[48] == can[48, :, :1]).all()
        steps.append(int(np.diff(row).max()))
    print("largest column step: paste %d, bands 1 .. 4 %r" % (paste_step, steps))
    assert all(s < paste_step for s in steps)
    assert all(b <= a for a, b in zip(steps, steps[1:]))


def test_a_misregistered_pair_keeps_more_detail_than_feather(lib):
    images, Gs = mc.misregistered_pair()
    multi = mc.gradient_energy(mc.host(lib, images, Gs, 0, 5))
    st, fe = sc.host_twin(lib, images, Gs, 0, sc.FEATHER)
    assert st == 0
    feather = mc.gradient_energy(fe)
    print("gradient energy in the overlap: multiband (5 bands) %.3f, feather %.3f, paste %.3f"
          % (multi, feather, mc.gradient_energy(paste(lib, images, Gs))))
    assert multi > feather


def test_the_images_are_not_written(lib):
    _, images, Gs, anchor, _ = GENERAL[2]
    before = [im.copy() for im in images]
    mc.host(lib, images, Gs, anchor, 3, gc.mixed_gains(len(images)))
    assert all(np.array_equal(a, b) for a, b in zip(images, before))


# ---- refusals ----
def test_c_level_refusals(lib):
    images, Gs = sc.translated_strip(3)
    st, can = mc.host_twin(lib, images, Gs, 0, 2)
    assert st == 0 and can.any()

    def spoiled(tweak, bands=2, gains=None):
        st, can = mc.host_twin(lib, images, Gs, 0, bands, gains, tweak)
        assert (can == 0xA5).all(), "a refused call wrote the canvas"
        return st
    assert spoiled(None, bands=0) == -1 and spoiled(None, bands=9) == -1 and spoiled(None, bands=-1) == -1
    assert spoiled(lambda t, p: p.__setitem__(1, 0)) == -1                                   # a NULL image
    assert spoiled(lambda t, p: t.__setitem__("anchor", 3)) == -1 and spoiled(lambda t, p: t.__setitem__("anchor", -1)) == -1
    for bad in (np.nan, np.inf, 0.0, -1.0):
        assert spoiled(None, gains=[1.0, bad, 1.0]) == -1, bad
    assert spoiled(lambda t, p: t["rects"].__setitem__((2, 0), t["rects"][2, 0] + 1)) == -1     # a rectangle off the canvas
    assert spoiled(lambda t, p: t.__setitem__("origin", (1, 0))) == -1
    assert spoiled(lambda t, p: t.__setitem__("n", 0)) == -1 and spoiled(lambda t, p: t.__setitem__("n", 65)) == -1
    assert spoiled(lambda t, p: t["inv"].__setitem__((2, 4), np.nan)) == -1
    assert spoiled(lambda t, p: t["hw"].__setitem__((1, 0), 1)) == -1
    # the workspace size: positive for what the call takes, <= 0 for what it refuses
    t = sc.tables(images, Gs, 0)
    assert mc.workspace_bytes(lib, t, 2) > 0
    assert mc.workspace_bytes(lib, t, 0) <= 0 and mc.workspace_bytes(lib, t, 9) <= 0
    off = dict(t, rects=t["rects"].copy())
    off["rects"][2, 0] += 1
    assert mc.workspace_bytes(lib, off, 2) <= 0
    assert mc.workspace_bytes(lib, dict(t, n=0), 2) <= 0
    # the sequence entry point has not grown a third blend
    fh, fw = t["size"]
    can = np.zeros((fh, fw, 3), np.uint8)
    keep = [np.ascontiguousarray(im) for im in images]
    ptrs = np.array([im.ctypes.data for im in keep], dtype=np.uint64)
    args = (ptrs.ctypes.data, t["hw"].ctypes.data, t["inv"].ctypes.data, t["rects"].ctypes.data, 3, 0, t["order"].ctypes.data)
    assert lib.rwh_host_stitch_sequence(*args, 2, can.ctypes.data, fh, fw, 0, 0, 0, fh) == -1
    assert lib.rwh_host_stitch_sequence(*args, 1, can.ctypes.data, fh, fw, 0, 0, 0, fh) == 0


def test_exports_and_constants(lib):
    from ransac_with_homography_amd import _lib
    for name in ("rwh_stitch_multiband_workspace_bytes", "rwh_stitch_multiband", "rwh_host_stitch_multiband"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.RWH_SEQ_MAX_BANDS == mc.MAX_BANDS == 8


# ---- the Python layer, without a GPU ----
def test_python_level_refusals_come_before_the_gpu():
    import homography
    import ransac
    from ransac_with_homography_amd import homography as hg
    from ransac_with_homography_amd import ransac as rs
    a, b, c = (sc.random_image(12, 16, i) for i in (1, 2, 3))
    T = sc.translate(8, 0)
    for bad in (0, 9, 2.5, True, -1, None, "5"):
        with pytest.raises(ValueError):
            hg.stitchSequence([a, b, c], Hs=[T, T], blending="multiband", bands=bad)
        with pytest.raises(ValueError, match="bands"):
            rs.stitch_sequence([a, b, c], blending="multiband", bands=bad)
    for bad in ("Rate", "Gradient", "Multiband", "multi", True, 1):
        with pytest.raises(ValueError):
            hg.stitchSequence([a, b, c], Hs=[T, T], blending=bad)
    with pytest.raises(ValueError):
        hg.stitchSequence([a, b, c], Hs=[T, T], blending="multiband", order=[0, 0, 1])       # `order` is still validated
    with pytest.raises(ValueError):
        hg.stitchSequence([a, b, c], Hs=[T, T], blending="multiband", gains=[1.0, 0.0, 1.0])
    assert inspect.signature(hg.stitchSequence).parameters["bands"].default == 5
    assert inspect.signature(rs.stitch_sequence).parameters["bands"].default == 5
    assert list(inspect.signature(hg.stitchSequence).parameters)[-1] == "bands"
    assert list(inspect.signature(rs.stitch_sequence).parameters)[-1] == "bands"
    assert homography.stitchSequence is hg.stitchSequence and ransac.stitch_sequence is rs.stitch_sequence
