"""The block gain rule (include/rwh.h) on the CPU: the host twins against the numpy restatement of tests/block_gain_cases.py --
tables and canvases exactly, maps by the backward-error criterion of tests/test_sequence_gains_cpu.py -- the sum-over-cells
identity, constant and unit maps, every refusal, the exports, and the effect of block gains on a vignetted scene."""
import inspect

import numpy as np
import pytest

import block_gain_cases as bg
import gain_cases as gc
import projection_cases as pc
import sequence_cases as sc


@pytest.fixture(scope="module")
def lib():
    return sc.library()


def _planar(name):
    images, Gs = getattr(bg, name)()
    return (name, images) + bg.planar_planes(images, Gs, 0)


def _curved():
    images, Gs, kind, f = bg.cylinder_case()
    return ("cylinder", images) + bg.curved_planes(images, Gs, 0, kind, f)


@pytest.fixture(scope="module")
def scenes():
    """name -> (images, tables t, cover, val, w): the planes of every case, restated once and never written."""
    out = {}
    for name in ("partial_cells", "narrow_canvas", "empty_cell", "sixty_four_on_one_cell", "big_cell"):
        n, images, t, cover, val, w = _planar(name)
        out[n] = (images, t, cover, val, w)
    n, images, t, cover, val, w = _curved()
    out[n] = (images, t, cover, val, w)
    _, images, Gs, anchor, _ = sc.general_cases()[4]
    out["n5 anchor 2"] = (images,) + bg.planar_planes(images, Gs, anchor)
    return out


TABLE_CASES = [("partial_cells", 16, 1), ("partial_cells", 16, 3), ("partial_cells", 16, 17), ("partial_cells", 32, 1), ("partial_cells", 64, 5),
               ("narrow_canvas", 16, 1), ("narrow_canvas", 32, 3), ("empty_cell", 16, 1), ("empty_cell", 16, 3),
               ("sixty_four_on_one_cell", 16, 1), ("big_cell", 128, 1), ("big_cell", 128, 3), ("cylinder", 16, 1), ("cylinder", 16, 3),
               ("cylinder", 32, 17), ("n5 anchor 2", 16, 1), ("n5 anchor 2", 32, 3)]


# ---- cells and their statistics ----
@pytest.mark.parametrize("name,B,stride", TABLE_CASES, ids=["%s-B%d-s%d" % c for c in TABLE_CASES])
def test_host_tables_are_the_restatement(lib, scenes, name, B, stride):
    images, t, cover, val, _ = scenes[name]
    before = [im.copy() for im in images]
    _, K = bg.candidates(t, B)
    assert bg.slots(lib, t, B) == K
    got = bg.hcells(lib, t, images, B, stride)
    want = bg.cell_tables(t, cover, val, B, stride)
    assert got.shape == want.shape == bg.grid(t["size"], B) + (2, K, K)
    assert np.array_equal(got, want)
    assert all(np.array_equal(a, b) for a, b in zip(images, before))         # the images are never written
    assert got[:, :, 0].any()


def test_shapes_reach_the_edges_they_are_made_for(lib, scenes):
    _, t, _, _, _ = scenes["partial_cells"]
    assert t["size"][0] % 16 and t["size"][1] % 16 and min(t["size"]) > 16
    assert scenes["narrow_canvas"][1]["size"][1] < 16
    cands, K = bg.candidates(scenes["empty_cell"][1], 16)
    assert any(not c for row in cands for c in row) and K == 1
    images, t, _, _, _ = scenes["partial_cells"]
    tabs = bg.hcells(lib, t, images, 16, 17)                                   # stride 17 > B: some cells hold no sample
    assert any(not tabs[gy, gx].any() for gy in range(tabs.shape[0]) for gx in range(tabs.shape[1]))
    images, t, _, _, _ = scenes["sixty_four_on_one_cell"]
    assert bg.slots(lib, t, 16) == 64 and (bg.hcells(lib, t, images, 16, 1)[0, 0, 0] > 0).all()
    images, t, _, _, _ = scenes["big_cell"]
    tabs = bg.hcells(lib, t, images, 128, 1)
    assert tabs.shape[:2] == (2, 2) and tabs[0, 0, 0, 0, 0] == 16384 and tabs[0, 0, 1, 0, 0] == 16384 * 765     # the largest sum of a slot


@pytest.mark.parametrize("name,B,stride", [c for c in TABLE_CASES if c[0] != "cylinder"], ids=["%s-B%d-s%d" % c for c in TABLE_CASES if c[0] != "cylinder"])
def test_cells_sum_to_the_overlap_statistics(lib, scenes, name, B, stride):
    images, t, _, _, _ = scenes[name]
    images = [np.ascontiguousarray(im) for im in images]
    n = t["n"]
    _, count, total, check = gc.guarded_tables(n)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    st = lib.rwh_host_sequence_overlap_stats(*bg.layout(t, ptrs, (), t["size"], (stride, count.ctypes.data, total.ctypes.data)))
    check()
    assert st == 0
    got = bg.scatter(bg.hcells(lib, t, images, B, stride), t, B)
    assert np.array_equal(got[0], count) and np.array_equal(got[1], total)


def test_cells_sum_to_the_overlap_statistics_on_the_cylinder(lib, scenes):
    images, t, _, _, _ = scenes["cylinder"]
    _, Gs, kind, f = bg.cylinder_case()
    for B, stride in ((16, 1), (32, 3)):
        count, total = pc.host_stats(lib, images, Gs, 0, kind, f, stride)
        got = bg.scatter(bg.hcells(lib, t, images, B, stride), t, B)
        assert np.array_equal(got[0], count) and np.array_equal(got[1], total)


# ---- cell gains, smoothing, maps ----
BASES = {"none": None, "dyadic": (0.5, 2.0, 1.0), "general": (1.3, 0.7, 1.1)}


@pytest.mark.parametrize("base", list(BASES), ids=list(BASES))
@pytest.mark.parametrize("name,B", [("partial_cells", 16), ("partial_cells", 32), ("cylinder", 16), ("sixty_four_on_one_cell", 16)])
def test_cell_gains_solve_the_restated_systems(lib, scenes, name, B, base):
    """smooth = 0: the maps are base_i * r.  Every cell's r solves the restated system within the bound of a Cholesky solve; an
    image that is no candidate, or that meets nobody, has r = 1.0 exactly."""
    images, t, _, _, _ = scenes[name]
    n = t["n"]
    base = None if BASES[base] is None else np.array([BASES[base][i % 3] for i in range(n)])
    ones = np.ones(n) if base is None else base
    tabs = bg.hcells(lib, t, images, B, 1)
    maps = bg.hmaps(lib, tabs, t, B, base, iterations=0)
    r = maps / ones[:, None, None]                     # (exact for base None and the dyadic base; one rounding for the general one)
    cands, _ = bg.candidates(t, B)
    seen = 0
    for gy, gx, c, A, b in bg.cell_systems(tabs, t, B, ones):
        g = r[c, gy, gx]
        assert np.abs(A @ g - b).max() <= bg.residual_bound(A, g), (gy, gx)
        ref = np.linalg.solve(A, b)
        assert np.abs(A @ ref - b).max() <= bg.residual_bound(A, ref)
        for k, i in enumerate(c):
            if not tabs[gy, gx, 0, k, :len(c)].any():
                assert maps[i, gy, gx] == ones[i]
        seen += 1
    assert seen
    for gy, row in enumerate(cands):
        for gx, c in enumerate(row):
            rest = [i for i in range(n) if i not in c]
            assert np.array_equal(maps[rest, gy, gx], ones[rest])


@pytest.mark.parametrize("iterations", [1, 2, 8])
def test_smoothing_and_maps_are_the_restated_steps_exactly(lib, scenes, iterations):
    """On the library's own cell gains (smooth = 0, where base is a power of two the division is exact) the smoothing and the
    maps are float64 steps in a stated order: bit for bit the restatement's."""
    for name, B in (("partial_cells", 16), ("cylinder", 16), ("narrow_canvas", 16)):
        images, t, _, _, _ = scenes[name]
        n = t["n"]
        tabs = bg.hcells(lib, t, images, B, 1)
        for base in (None, np.array([(0.5, 2.0, 1.0)[i % 3] for i in range(n)])):
            ones = np.ones(n) if base is None else base
            r = bg.hmaps(lib, tabs, t, B, base, iterations=0) / ones[:, None, None]
            got = bg.hmaps(lib, tabs, t, B, base, iterations=iterations)
            assert np.array_equal(got, bg.maps_of(bg.smooth(r, iterations), ones))
            assert not np.array_equal(got, bg.maps_of(r, ones)) or t["size"][1] < 16


def test_other_sigmas_enter_as_the_rule_says(lib, scenes):
    images, t, _, _, _ = scenes["partial_cells"]
    tabs = bg.hcells(lib, t, images, 16, 1)
    for sn, sg in ((5.0, 0.1), (10.0, 0.5), (2.5, 0.02)):
        maps = bg.hmaps(lib, tabs, t, 16, None, sn, sg, 0)
        for gy, gx, c, A, b in bg.cell_systems(tabs, t, 16, np.ones(3), sn, sg):
            assert np.abs(A @ maps[c, gy, gx] - b).max() <= bg.residual_bound(A, maps[c, gy, gx])


# ---- applying maps ----
def _restated(what, t, cover, val, w, maps, B, blend, order, labels, bands):
    v = bg.compensated(val, bg.gain_planes(maps, B, t["size"]))
    if what == "sequence":
        return bg.composite(cover, v, w, blend, t["order"] if order is None else order)
    if what == "labels":
        return bg.label_paste(cover, v, w, labels)
    return bg.multiband(cover, v, w, bands, labels)


CANVAS_KINDS = [("sequence", sc.PASTE, False), ("sequence", sc.FEATHER, False), ("labels", 0, True), ("multiband", 0, False), ("multiband", 0, True)]


@pytest.mark.parametrize("what,blend,labelled", CANVAS_KINDS, ids=["paste", "feather", "label paste", "multiband", "multiband labels"])
@pytest.mark.parametrize("name,B", [("partial_cells", 16), ("partial_cells", 32), ("cylinder", 16), ("narrow_canvas", 16), ("n5 anchor 2", 16)])
def test_host_compositors_with_maps_are_the_restatement(lib, scenes, name, B, what, blend, labelled):
    images, t, cover, val, w = scenes[name]
    before = [im.copy() for im in images]
    maps = bg.wavy_maps(t["n"], t["size"], B, seed=B)
    labels = bg.stripes(t["size"], t["n"], seed=3) if labelled else None
    got = bg.hcanvas(lib, what, t, images, maps, B, blend=blend, labels=labels, bands=2)
    want = _restated(what, t, cover, val, w, maps, B, blend, None, labels, 2)
    assert np.array_equal(got, want)
    assert all(np.array_equal(a, b) for a, b in zip(images, before))
    assert not np.array_equal(got, bg.hcanvas(lib, what, t, images, np.ones_like(maps), B, blend=blend, labels=labels, bands=2))


def test_row_tiles_with_maps_equal_the_whole_canvas(lib, scenes):
    images, t, _, _, _ = scenes["partial_cells"]
    maps = bg.wavy_maps(3, t["size"], 16)
    for blend in (sc.PASTE, sc.FEATHER):
        whole = bg.hcanvas(lib, "sequence", t, images, maps, 16, blend=blend)
        fh = t["size"][0]
        for r0, r1 in ((0, 7), (7, 30), (30, fh)):
            part = bg.hcanvas(lib, "sequence", t, images, maps, 16, blend=blend, rows=(r0, r1))
            assert np.array_equal(part[r0:r1], whole[r0:r1]) and (part[:r0] == 0xA5).all() and (part[r1:] == 0xA5).all()


def _scalar_canvas(lib, what, t, images, gains, blend, labels, bands):
    """The host twins that take N gains, on the tables `t`."""
    images = [np.ascontiguousarray(im) for im in images]
    fh, fw = t["size"]
    can, check = sc.guarded_canvas(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    g = None if gains is None else np.ascontiguousarray(gains, dtype=np.float64)
    gp = None if g is None else g.ctypes.data
    out = (can.ctypes.data, fh, fw)
    if what == "sequence":
        entry = "rwh_host_stitch_sequence" + (bg.form(t) or "_ex")
        st = getattr(lib, entry)(*bg.layout(t, ptrs, (t["order"].ctypes.data, blend), out, (0, fh, gp)))
    elif what == "labels":
        st = getattr(lib, "rwh_host_stitch_sequence_labels" + bg.form(t))(*bg.layout(t, ptrs, (gp, labels.ctypes.data), out, ()))
    elif labels is None:
        st = getattr(lib, "rwh_host_stitch_multiband" + bg.form(t))(*bg.layout(t, ptrs, (bands, gp), out, ()))
    else:
        st = getattr(lib, "rwh_host_stitch_multiband_labels" + bg.form(t))(*bg.layout(t, ptrs, (bands, gp, labels.ctypes.data), out, ()))
    check()
    assert st == 0
    return can


@pytest.mark.parametrize("what,blend,labelled", CANVAS_KINDS, ids=["paste", "feather", "label paste", "multiband", "multiband labels"])
def test_constant_maps_give_the_gain_rules_canvas_and_unit_maps_the_plain_one(lib, scenes, what, blend, labelled):
    """Gains of at most 53 - (s + 1) significant bits (here float32 values, 24 bits): the lerp of a constant map is then exact, so the
    canvas is the gain rule's byte for byte -- for every block.  Unit maps give the canvas without gains."""
    gains32 = np.array([1.9, 0.5, 1.3], dtype=np.float32).astype(np.float64)
    for name in ("partial_cells", "cylinder"):
        images, t, _, _, _ = scenes[name]
        labels = bg.stripes(t["size"], 3, seed=5) if labelled else None
        with_gains = _scalar_canvas(lib, what, t, images, gains32, blend, labels, 2)
        plain = _scalar_canvas(lib, what, t, images, None, blend, labels, 2)
        assert not np.array_equal(with_gains, plain)
        for B in bg.BLOCKS:
            shape = (3,) + bg.grid(t["size"], B)
            maps = np.broadcast_to(gains32[:, None, None], shape)
            assert np.array_equal(bg.gain_planes(np.ascontiguousarray(maps), B, t["size"]), np.broadcast_to(gains32[:, None, None], (3,) + tuple(t["size"])))
            assert np.array_equal(bg.hcanvas(lib, what, t, images, maps, B, blend=blend, labels=labels, bands=2), with_gains)
            assert np.array_equal(bg.hcanvas(lib, what, t, images, np.ones(shape), B, blend=blend, labels=labels, bands=2), plain)


def test_a_constant_map_of_a_full_width_gain_may_round():
    """Why the identity above is stated for short gains: the lerp of the constant 1.3 (53 significant bits) rounds at t = 3/16."""
    t = 3 / 16
    assert 1.3 * (1 - t) + 1.3 * t != 1.3
    g = float(np.float32(1.3))
    assert all(g * (1 - k / 256) + g * (k / 256) == g for k in range(256))


# ---- refusals ----
def test_c_level_refusals(lib, scenes):
    images, t, _, _, _ = scenes["partial_cells"]
    images = [np.ascontiguousarray(im) for im in images]
    fh, fw = t["size"]
    rects = t["rects"]
    ox, oy = t["origin"]
    INVALID = -1
    # slots
    assert lib.rwh_sequence_cell_slots(rects.ctypes.data, 3, fh, fw, ox, oy, 4) == 2 or lib.rwh_sequence_cell_slots(rects.ctypes.data, 3, fh, fw, ox, oy, 4) == 3
    for shift in (3, 8, 0, -1):
        assert lib.rwh_sequence_cell_slots(rects.ctypes.data, 3, fh, fw, ox, oy, shift) < 0
    assert lib.rwh_sequence_cell_slots(None, 3, fh, fw, ox, oy, 4) < 0
    assert lib.rwh_sequence_cell_slots(rects.ctypes.data, 0, fh, fw, ox, oy, 4) < 0 and lib.rwh_sequence_cell_slots(rects.ctypes.data, 65, fh, fw, ox, oy, 4) < 0
    assert lib.rwh_sequence_cell_slots(rects.ctypes.data, 3, fh, fw - 1, ox, oy, 4) < 0                 # a rectangle off the canvas
    assert lib.rwh_sequence_cell_slots(rects.ctypes.data, 3, 0, fw, ox, oy, 4) < 0
    assert lib.rwh_sequence_cell_stats_workspace_bytes(0) < 0 and lib.rwh_sequence_cell_stats_workspace_bytes(65) < 0
    assert lib.rwh_sequence_cell_stats_workspace_bytes(3) == 384
    K = bg.slots(lib, t, 16)
    gh, gw = bg.grid(t["size"], 16)
    assert lib.rwh_sequence_cell_stats_table_bytes(fh, fw, 4, K) == gh * gw * 2 * K * K * 4
    for bad in ((fh, fw, 3, K), (fh, fw, 8, K), (fh, fw, 4, 0), (fh, fw, 4, 65), (0, fw, 4, K)):
        assert lib.rwh_sequence_cell_stats_table_bytes(*bad) < 0
    # the statistics
    assert bg.host_cell_stats(lib, t, images, 16, 1)[0] == 0
    for stride in (0, 256, -1):
        assert bg.host_cell_stats(lib, t, images, 16, stride)[0] == INVALID
    for K_bad in (K - 1, K + 1, 64):
        assert bg.host_cell_stats(lib, t, images, 16, 1, K=K_bad)[0] == INVALID
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    words = np.zeros(gh * gw * 2 * K * K + 1, dtype=np.uint32)
    call = lambda tt, tail: lib.rwh_host_sequence_cell_stats(*bg.layout(tt, ptrs, (), (fh, fw), tail))
    assert call(t, (4, 1, K, words.ctypes.data)) == 0
    assert call(t, (4, 1, K, None)) == INVALID
    assert call(t, (4, 1, K, words.ctypes.data + 2)) == INVALID                                        # misaligned
    assert call(t, (3, 1, K, words.ctypes.data)) == INVALID and call(t, (8, 1, K, words.ctypes.data)) == INVALID
    assert call(dict(t, anchor=3), (4, 1, K, words.ctypes.data)) == INVALID                            # what the sequence rule refuses
    # cell gains
    tabs = bg.hcells(lib, t, images, 16, 1)
    assert bg.host_block_gains(lib, tabs, t, 16)[0] == 0
    for kw in (dict(sigma_n=0.0), dict(sigma_n=np.nan), dict(sigma_g=-0.1), dict(sigma_g=np.inf), dict(iterations=-1), dict(iterations=9),
               dict(base=[1.0, 0.0, 1.0]), dict(base=[1.0, np.nan, 1.0]), dict(base=[1.0, -2.0, 1.0]), dict(base=[np.inf, 1.0, 1.0]),
               dict(K=K + 1), dict(K=K - 1)):
        assert bg.host_block_gains(lib, tabs, t, 16, **kw)[0] == INVALID, kw
    out = np.zeros(3 * gh * gw)
    args = (t["rects"].ctypes.data, 3, fh, fw, ox, oy, 4, K, None, 10.0, 0.1, 2)
    assert lib.rwh_host_sequence_block_gains(tabs.ctypes.data, *args, out.ctypes.data) == 0
    assert lib.rwh_host_sequence_block_gains(None, *args, out.ctypes.data) == INVALID
    assert lib.rwh_host_sequence_block_gains(tabs.ctypes.data, *args, None) == INVALID
    assert lib.rwh_host_sequence_block_gains(tabs.ctypes.data, None, *args[1:], out.ctypes.data) == INVALID
    # a table that gives a non-positive pivot: two images that meet with means large enough that alpha's terms overflow to inf
    huge = tabs.copy()
    huge[:, :, 1] = 0xFFFFFFFF
    assert bg.host_block_gains(lib, huge, t, 16, base=[1e300, 1e300, 1e300])[0] == INVALID
    # the compositors
    maps = bg.wavy_maps(3, t["size"], 16)
    labels = bg.stripes(t["size"], 3)
    for what, lab in (("sequence", None), ("labels", labels), ("multiband", None), ("multiband", labels)):
        assert bg.host_canvas(lib, what, t, images, maps, 16, labels=lab)[0] == 0
        for bad in (0.0, -1.0, np.nan, np.inf):
            spoiled = maps.copy()
            spoiled[2, -1, -1] = bad
            assert bg.host_canvas(lib, what, t, images, spoiled, 16, labels=lab)[0] == INVALID, (what, bad)
        assert bg.host_canvas(lib, what, t, images, maps, 8, labels=lab)[0] == INVALID                 # shift 3
        assert bg.host_canvas(lib, what, t, images, np.ones((3, 1, 1)), 256, labels=lab)[0] == INVALID  # shift 8
    assert bg.host_canvas(lib, "labels", t, images, maps, 16, labels=None)[0] == INVALID               # label paste takes a plane
    od = t["order"]
    can = np.zeros((fh, fw, 3), dtype=np.uint8)
    seq = lambda m: lib.rwh_host_stitch_sequence_maps(*bg.layout(t, ptrs, (od.ctypes.data, 0), (can.ctypes.data, fh, fw), (0, fh, m, 4)))
    assert seq(maps.ctypes.data) == 0 and seq(None) == INVALID and seq(maps.ctypes.data + 4) == INVALID
    assert all(np.array_equal(a, b) for a, b in zip(images, bg.partial_cells()[0]))


def test_python_level_refusals_come_before_the_gpu():
    """Everything here raises where there is no GPU: the checks come before the device is asked for."""
    from ransac_with_homography_amd import homography as hg
    from ransac_with_homography_amd import ransac as rs
    a, b, c = (sc.random_image(40, 56, i) for i in (1, 2, 3))
    T = sc.translate(30, 0)
    for kw in (dict(block=8), dict(block=48), dict(block=256), dict(block=32.0), dict(block=None), dict(block=True),
               dict(stride=0), dict(stride=256), dict(stride=2.5), dict(sigma_n=0.0), dict(sigma_n=np.nan), dict(sigma_g=-0.1),
               dict(sigma_g=np.inf), dict(smooth=-1), dict(smooth=9), dict(smooth=1.5), dict(smooth=None),
               dict(base="Auto"), dict(base=[1.0, 1.0]), dict(base=[1.0, 0.0, 1.0]), dict(base=[1.0, np.nan, 1.0])):
        with pytest.raises(ValueError):
            hg.sequence_block_gains([a, b, c], Hs=[T, T], **kw)
    with pytest.raises(ValueError):
        hg.sequence_block_gains([a, b])                                        # the same validation of geometry as stitchSequence
    with pytest.raises(NotImplementedError):
        hg.sequence_block_gains([a, b.astype(np.float32)], Hs=[T])
    # stitchSequence: maps that do not fit the canvas and block, bad entries, a bad block, a bad base
    size = (40, 116)
    good = np.ones((3,) + bg.grid(size, 32))
    for bad in (hg.BlockGains(np.ones((3, 1, 1)), 32, np.ones(3)), hg.BlockGains(np.ones((2,) + good.shape[1:]), 32, np.ones(3)),
                hg.BlockGains(good, 16, np.ones(3)), hg.BlockGains(good, 48, np.ones(3)), hg.BlockGains(good * 0.0, 32, np.ones(3)),
                hg.BlockGains(good * np.nan, 32, np.ones(3)), hg.BlockGains(good, 32, np.ones(2)), hg.BlockGains(good, 32, [1.0, -1.0, 1.0])):
        for blending in (False, "feather", "multiband"):
            with pytest.raises(ValueError):
                hg.stitchSequence([a, b, c], Hs=[T, T], gains=bad, blending=blending)
        with pytest.raises(ValueError):
            hg.sequence_seams([a, b, c], Hs=[T, T], gains=bad)
    for bad in ("Blocks", "block", ""):
        with pytest.raises(ValueError):
            hg.stitchSequence([a, b, c], Hs=[T, T], gains=bad)
        with pytest.raises(ValueError):
            rs.stitch_sequence([a, b, c], gains=bad)
    # the ring is out, before the GPU and before the geometry is looked at
    for gains in ("blocks", hg.BlockGains(good, 32, np.ones(3))):
        with pytest.raises(NotImplementedError):
            hg.stitchSequence([a, b, c], Hs=[T, T], gains=gains, projection="cylindrical", focal=300.0, wrap=True)
    with pytest.raises(NotImplementedError):
        rs.stitch_ring([a, b, c], gains="blocks")


def test_kernels_level_refusals_come_before_the_library():
    from ransac_with_homography_amd import kernels
    for bad in (8, 48, 256, 16.0, None, True):
        with pytest.raises(ValueError):
            kernels.sequence_block_shift("who", bad)
    assert [kernels.sequence_block_shift("who", b) for b in bg.BLOCKS] == [4, 5, 6, 7]
    assert kernels.sequence_cell_grid((40, 116), 32) == (2, 4) and kernels.sequence_cell_grid((32, 33), 16) == (2, 3)
    images, Gs = bg.partial_cells()
    t = sc.tables(images, Gs, 0)
    geom = sc.geometry(t)
    for B in (16, 32):
        cands, K = bg.candidates(t, B)
        got = kernels.sequence_cell_candidates(geom, 3, B)
        assert got.shape == bg.grid(t["size"], B) + (3,)
        assert all(list(np.flatnonzero(got[gy, gx])) == c for gy, row in enumerate(cands) for gx, c in enumerate(row))
    ring = kernels.SeqGeometry(t["inv"], t["rects"], t["size"], rays=(None, None), ring=True)
    with pytest.raises(NotImplementedError):
        kernels.sequence_cell_tables_on([], ring, 32, 1)


def test_exports_and_defaults():
    import homography
    import ransac
    from ransac_with_homography_amd import _lib, kernels
    from ransac_with_homography_amd import homography as hg
    from ransac_with_homography_amd import ransac as rs
    assert homography.sequence_block_gains is hg.sequence_block_gains and rs.sequence_block_gains is hg.sequence_block_gains
    assert homography.BlockGains is hg.BlockGains and rs.BlockGains is hg.BlockGains
    assert not hasattr(ransac, "sequence_block_gains")      # the top-level `ransac` shim's name list is pinned (test_orb_pyramid_cpu.py)
    assert "sequence_block_gains" in homography.__all__ and "BlockGains" in homography.__all__
    assert hg.BlockGains._fields == ("maps", "block", "base")
    p = inspect.signature(hg.sequence_block_gains).parameters
    assert list(p) == ["images", "Hs", "Gs", "anchor", "block", "stride", "sigma_n", "sigma_g", "smooth", "base", "info", "projection", "focal"]
    assert [p[k].default for k in ("block", "stride", "sigma_n", "sigma_g", "smooth", "base")] == [32, 1, 10.0, 0.1, 2, "auto"]
    assert inspect.signature(hg.stitchSequence).parameters["gains"].default is None        # no default changes
    assert inspect.signature(rs.stitch_sequence).parameters["gains"].default is None
    assert list(inspect.signature(kernels.sequence_cell_tables_on).parameters) == ["images", "geom", "block", "stride"]
    lib = sc.library()
    for name in ("rwh_sequence_cell_slots", "rwh_sequence_cell_stats", "rwh_sequence_cell_stats_proj", "rwh_host_sequence_cell_stats",
                 "rwh_host_sequence_cell_stats_proj", "rwh_sequence_cell_stats_workspace_bytes", "rwh_host_sequence_block_gains",
                 "rwh_stitch_sequence_maps", "rwh_stitch_sequence_maps_proj", "rwh_stitch_multiband_maps", "rwh_stitch_multiband_maps_proj",
                 "rwh_stitch_sequence_labels_maps", "rwh_stitch_sequence_labels_maps_proj"):
        assert name in _lib.EXPORTS and hasattr(lib, name)


# ---- the effect ----
def test_block_gains_remove_what_one_gain_per_image_cannot(lib, capsys):
    """Three crops of one texture, each with its own exposure and the same radial falloff: the mean absolute difference of the
    compensated bytes where two images meet falls from no gains to one gain per image, and again to block gains."""
    images, Gs = bg.vignetted_scene()
    t, cover, val, _ = bg.planar_planes(images, Gs, 0)
    count, total = gc.hstats(lib, images, Gs, 0, 4)
    st, g = gc.host_gains(lib, count, total)
    assert st == 0
    none = bg.mismatch(cover, val)
    glob = bg.mismatch(cover, bg.compensated(val, np.broadcast_to(g[:, None, None], cover.shape)))
    assert glob < none                                                         # the reference condition: holds without any new code
    maps = bg.hmaps(lib, bg.hcells(lib, t, images, 32, 1), t, 32, g)
    blocks = bg.mismatch(cover, bg.compensated(val, bg.gain_planes(maps, 32, t["size"])))
    with capsys.disabled():
        print("\nvignetted scene, mean |difference| of compensated bytes in the overlaps: none %.3f, global %.3f, blocks %.3f" % (none, glob, blocks))
    assert blocks < glob < none
