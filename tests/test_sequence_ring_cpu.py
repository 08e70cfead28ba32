"""The ring rule (include/rwh.h: the sequence compositor on a canvas that closes the circle) on the CPU: the host twins against the
numpy restatement of tests/ring_cases.py, exactly; the rule's two consequences; the geometry of a full circle of an analytic
texture; the Python layer's plan; and every refusal of the new arguments, before any GPU use."""
import numpy as np
import pytest

import gain_cases as gc
import projection_cases as pc
import ring_cases as rc
import sequence_cases as sc

INVALID = -1


@pytest.fixture(scope="module")
def lib():
    return sc.library()


@pytest.fixture(scope="module")
def hg(lib):
    from ransac_with_homography_amd import homography
    return homography


def settings():
    """(period, anchor, order): the 12-image circle with its default and a permuted order, with another anchor (another image lies
    across the seam), and the 13-image circle."""
    return [(256, 0, None), (256, 0, [7, 2, 11, 0, 5, 9, 1, 4, 10, 3, 8, 6]), (256, 5, None), (512, 0, None)]


SETTINGS = settings()
IDS = ["P%d anchor %d%s" % (p, a, " permuted" if o else "") for p, a, o in SETTINGS]


# ---- the rule against its restatement ----
@pytest.mark.parametrize("kind", rc.SURFACES)
@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_twin_is_the_restatement(lib, setting, kind):
    """Paste (in the case's order) and feather, with and without gains; one rectangle at least passes the canvas's edge and every
    column is covered somewhere."""
    P, anchor, order = setting
    images, t = rc.circle_tables(P, kind, anchor, order)
    assert t["size"][1] == P and t["origin"][0] == -P // 2
    assert (t["rects"][:, 0] + t["rects"][:, 2] > P).any()
    assert rc.planes(images, t)[0].any(axis=(0, 1)).all()
    for blend in (rc.PASTE, rc.FEATHER):
        for gains in (None, rc.gains_for(len(images))):
            got = rc.host(lib, images, t, blend, gains=gains)
            assert np.array_equal(got, rc.restate(images, t, blend, gains)), (blend, gains)
            assert got.any()


@pytest.mark.parametrize("kind", rc.SURFACES)
def test_which_rectangles_cross_the_edge(kind):
    for P, crossing in ((256, 1), (512, 2)):          # 12 images: the one opposite the anchor; 13: the two on either side of the seam
        _, t = rc.circle_tables(P, kind)
        assert ((t["rects"][:, 0] + t["rects"][:, 2]) > P).sum() == crossing
        assert (t["rects"][:, 0] >= 0).all() and (t["rects"][:, 0] < P).all() and (t["rects"][:, 2] <= P).all()


@pytest.mark.parametrize("kind", rc.SURFACES)
@pytest.mark.parametrize("stride", (1, 3, 4))
def test_overlap_tables_are_the_restatements(lib, kind, stride):
    for P, anchor, _ in SETTINGS[1:]:
        images, t = rc.circle_tables(P, kind, anchor)
        count, total = rc.host_stats(lib, images, t, stride)
        want = rc.stats(images, t, stride)
        assert np.array_equal(count, want[0]) and np.array_equal(total, want[1])
        n = len(images)
        assert count[0, 1] > 0 and (stride > 1 or count[0, n - 1] > 0)      # the first image meets the second -- and the last


@pytest.mark.parametrize("kind", rc.SURFACES)
@pytest.mark.parametrize("bands", (1, 2, 5))
def test_multiband_twin_is_the_restatement(lib, kind, bands):
    """At bands 5 the windows of the low levels are the whole ring (256 >> 5 is 8 columns)."""
    for P, anchor, _ in SETTINGS[1:]:
        images, t = rc.circle_tables(P, kind, anchor)
        for gains in (None, rc.gains_for(len(images))):
            assert np.array_equal(rc.host_multiband(lib, images, t, bands, gains), rc.multiband(images, t, bands, gains)), (P, anchor, gains)


@pytest.mark.parametrize("kind", rc.SURFACES)
def test_one_image_multiband_is_paste(lib, kind):
    images, t = rc.circle_tables(256, kind)
    one = dict(t, hw=t["hw"][6:7].copy(), m=t["m"][6:7].copy(), rects=t["rects"][6:7].copy(), order=np.zeros(1, dtype=np.int32), n=1)
    assert one["rects"][0, 0] + one["rects"][0, 2] > 256                  # the image across the seam
    for bands in (1, 3):
        assert np.array_equal(rc.host_multiband(lib, images[6:7], one, bands), rc.host(lib, images[6:7], one, rc.PASTE))


# ---- rectangles ----
@pytest.mark.parametrize("kind", rc.SURFACES)
@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_the_rectangles_contain_every_valid_pixel(lib, setting, kind):
    """No valid pixel of any image lies outside its rectangle, and with every rectangle the whole canvas the twins write what they
    write with the rule's rectangles."""
    P, anchor, order = setting
    images, t = rc.circle_tables(P, kind, anchor, order)
    _, full = rc.circle_tables(P, kind, anchor, order, rects="canvas")
    assert np.array_equal(rc.unbounded_cover(images, t), rc.planes(images, t)[0])
    for blend in (rc.PASTE, rc.FEATHER):
        assert np.array_equal(rc.host(lib, images, full, blend), rc.host(lib, images, t, blend))
    for a, b in zip(rc.host_stats(lib, images, full, 3), rc.host_stats(lib, images, t, 3)):
        assert np.array_equal(a, b)
    assert np.array_equal(rc.host_multiband(lib, images, full, 2), rc.host_multiband(lib, images, t, 2))


# ---- consequence (a): the projection rule's canvas ----
@pytest.mark.parametrize("kind", rc.SURFACES)
def test_at_the_rings_own_focal_the_canvas_is_the_projected_one(lib, kind):
    """f == 256 / (2 pi) as a float64, three images about the anchor: on the columns and rows of the projection= canvas the ring
    canvas is that canvas byte for byte, under paste and feather; the table entries are the same numbers."""
    images, Gs, f = rc.three_views()
    assert rc.period(f) == 256 and 256 / (2.0 * np.pi) == f
    t = rc.tables(images, Gs, 1, kind, f)
    p = pc.tables(images, Gs, 1, kind, f)
    assert not (t["rects"][:, 0] + t["rects"][:, 2] > 256).any()
    dx, dy = p["origin"][0] - t["origin"][0], p["origin"][1] - t["origin"][1]
    fh, fw = p["size"]
    assert dx >= 0 and dy >= 0 and dx + fw <= 256 and dy + fh <= t["size"][0]
    assert np.array_equal(t["col"][dx:dx + fw], p["col"]) and np.array_equal(t["row"][dy:dy + fh], p["row"])
    for blend in (rc.PASTE, rc.FEATHER):
        ring = rc.host(lib, images, t, blend)
        assert np.array_equal(ring[dy:dy + fh, dx:dx + fw], pc.host(lib, images, Gs, 1, kind, f, blend))
        assert ring.any()


# ---- consequence (b): rolling ----
@pytest.mark.parametrize("kind", rc.SURFACES)
@pytest.mark.parametrize("s", (1, 37, 128))
def test_rolling_the_tables_rolls_the_canvas(lib, kind, s):
    images, t = rc.circle_tables(256, kind, 0, [7, 2, 11, 0, 5, 9, 1, 4, 10, 3, 8, 6])
    rolled = rc.roll(t, s)
    for blend in (rc.PASTE, rc.FEATHER):
        assert np.array_equal(rc.host(lib, images, rolled, blend), np.roll(rc.host(lib, images, t, blend), s, axis=1))


@pytest.mark.parametrize("kind", rc.SURFACES)
@pytest.mark.parametrize("s", (32, 64))
def test_rolling_by_a_multiple_rolls_bands_and_keeps_the_statistics(lib, kind, s):
    """Multi-band at bands 5 (s a multiple of 2^5) and the statistics at stride 4 (s a multiple of 4: the same samples)."""
    images, t = rc.circle_tables(256, kind)
    rolled = rc.roll(t, s)
    assert np.array_equal(rc.host_multiband(lib, images, rolled, 5), np.roll(rc.host_multiband(lib, images, t, 5), s, axis=1))
    for a, b in zip(rc.host_stats(lib, images, rolled, 4), rc.host_stats(lib, images, t, 4)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("kind", rc.SURFACES)
def test_a_row_range_writes_its_rows_only(lib, kind):
    images, t = rc.circle_tables(256, kind)
    whole = rc.restate(images, t, rc.FEATHER)
    fh = whole.shape[0]
    for rows in ((0, 1), (3, 9), (fh - 2, fh), (5, 5)):
        got = rc.host(lib, images, t, rc.FEATHER, rows=rows)
        assert np.array_equal(got[rows[0]:rows[1]], whole[rows[0]:rows[1]])
        assert (got[:rows[0]] == 0xA5).all() and (got[rows[1]:] == 0xA5).all()


# ---- geometry: a full circle of an analytic texture ----
@pytest.fixture(scope="module")
def eighteen():
    return rc.eighteen_views()


@pytest.mark.parametrize("kind", rc.SURFACES)
def test_eighteen_views_land_where_their_rays_point(lib, hg, eighteen, kind):
    """18 views of 160 x 120 at f = 300, 20 degrees apart, pitch 0.005 i, roll 0.003 i, through the Python layer's plan and the host
    twin, paste: P = 1792, rho = 285.2.  Every covered canvas pixel is within 2 grey levels of the texture on its own ray (0.5 image
    rounding + < 1 output truncation + 0.002 bilinear error: the bound and derivation of test_seven_views_land_where_their_rays_point),
    except the at most 4 per image whose taps include the image's texel (0,0), which the rule reads as 0; canvas row s = 0 is covered
    in ALL P columns; and the canvas is exactly P wide."""
    images, Hs, Rs = eighteen
    f = rc.EIGHTEEN["f"]
    rects, origin, (fh, fw), order, m, (col, row) = hg._sequence_inputs("test", images, Hs, None, 0, kind, f, True)
    P = hg.sequence_period(f)
    rho = P / (2.0 * np.pi)
    assert P == 1792 == fw and origin[0] == -896 and abs(rho - 285.2) < 0.05
    t = dict(hw=np.array([[im.shape[0], im.shape[1]] for im in images], dtype=np.int32), m=np.ascontiguousarray(m.reshape(-1, 9)),
             rects=np.array(rects, dtype=np.int32), order=np.array(order, dtype=np.int32), origin=origin, size=(fh, fw), n=len(images), col=col, row=row)
    can = rc.host(lib, images, t)
    covered = can.any(axis=2)
    theta = (origin[0] + np.arange(fw)) / rho
    s = (origin[1] + np.arange(fh)) / rho
    want = pc.texture(theta[None, :], (s if kind == "cylindrical" else np.tan(s))[:, None])
    rays = pc.rays_of(col, row).reshape(3, -1)
    zeroed = np.zeros((fh, fw), dtype=bool)
    for i in range(len(images)):
        z = m[i] @ rays
        with np.errstate(all="ignore"):
            sx, sy = z[0] / z[2], z[1] / z[2]
        near = ((z[2] > 0) & (sx >= 0) & (sx < 1) & (sy >= 0) & (sy < 1)).reshape(fh, fw)
        assert near.sum() <= 4
        zeroed |= near
    err = np.abs(can.astype(np.float64) - want).max(axis=2)
    print("%s: canvas %d x %d, %d covered, max error %.3f, %d pixels at a texel (0,0)" % (kind, fh, fw, covered.sum(), err[covered & ~zeroed].max(), zeroed.sum()))
    assert err[covered & ~zeroed].max() <= 2.0
    assert 0 <= -origin[1] < fh
    assert covered[-origin[1]].all()


# ---- the Python layer ----
def test_sequence_period(hg):
    for f, want in ((40.0, 256), (1.0, 256), (60.0, 256), (62.0, 512), (80.0, 512), (300.0, 1792), (256 / (2.0 * np.pi), 256), (10389.0, 65280)):
        assert hg.sequence_period(f) == want == rc.period(f) and isinstance(hg.sequence_period(f), int)
    for bad in (0.0, -3.0, float("nan"), float("inf"), "40", True, None, 10500.0):
        with pytest.raises(ValueError):
            hg.sequence_period(bad)


@pytest.mark.parametrize("kind", rc.SURFACES)
@pytest.mark.parametrize("wrap", (True, 512))
def test_the_plan_is_the_restatements(hg, kind, wrap):
    """sequence_plan and _sequence_inputs with wrap=True (the default period, 256) and wrap=512 on the 12-image circle."""
    for anchor in (0, 5):
        images, _, f = rc.circle(256, anchor)
        _, Hs = pc.sweep(12, rc.CASES[256]["seed"], f=f, yaw=2.0 * np.pi / 12)
        shapes = [im.shape for im in images]
        P = 256 if wrap is True else wrap
        Gs, rects, origin, size, order = hg.sequence_plan(shapes, Hs, anchor, kind, f, wrap=wrap)
        chained = pc.orient(sc.chain(Hs, anchor))
        assert np.array_equal(Gs, np.stack(chained))
        want = rc.rectangles(shapes, chained, anchor, kind, f, P)
        t = rc.tables(images, sc.chain(Hs, anchor), anchor, kind, f, P)
        assert rects == want and origin == t["origin"] and size == t["size"] == (size[0], P) and order == sc.default_order(12, anchor)
        assert any(r[0] < -P // 2 or r[0] + r[2] > P // 2 for r in rects)          # unwrapped: one passes the seam
        for how in (dict(Hs=Hs, Gs=None), dict(Hs=None, Gs=sc.chain(Hs, anchor))):
            own, origin2, size2, order2, m, (col, row) = hg._sequence_inputs("test", images, how["Hs"], how["Gs"], anchor, kind, f, wrap)
            assert np.array_equal(np.array(own, dtype=np.int32), t["rects"]) and (origin2, size2, order2) == (origin, size, order)
            assert np.array_equal(m.reshape(-1, 9), t["m"])
            for a, b in ((col, t["col"]), (row, t["row"])):
                assert a.dtype == np.float64 and a.flags.c_contiguous and np.array_equal(a, b)


BAD_WRAPS = [dict(wrap=True), dict(wrap=256), dict(wrap=True, focal=40.0), dict(wrap=255, projection="cylindrical", focal=40.0),
             dict(wrap=257, projection="cylindrical", focal=40.0), dict(wrap=0, projection="cylindrical", focal=40.0),
             dict(wrap=-256, projection="spherical", focal=40.0), dict(wrap=65536, projection="spherical", focal=40.0),
             dict(wrap=512.0, projection="cylindrical", focal=40.0), dict(wrap="yes", projection="cylindrical", focal=40.0),
             dict(wrap=None, projection="cylindrical", focal=40.0), dict(wrap=True, projection="cylindrical", focal=10500.0)]


@pytest.mark.parametrize("bad", BAD_WRAPS, ids=[str(b) for b in BAD_WRAPS])
def test_bad_wraps_are_refused_before_the_gpu(hg, bad):
    from ransac_with_homography_amd import ransac
    images, Hs = pc.sweep(3, 3)
    shapes = [im.shape for im in images]
    with pytest.raises(ValueError):
        hg.sequence_plan(shapes, Hs, 0, **bad)
    with pytest.raises(ValueError):
        hg.stitchSequence(images, Hs=Hs, **bad)
    with pytest.raises(ValueError):
        hg.sequence_gains(images, Hs=Hs, **bad)
    with pytest.raises(ValueError):
        ransac.stitch_ring(images, pairs="adjacent", adjust=False, **{"projection": None, "focal": None, **bad})
    with pytest.raises(ValueError):
        ransac.stitch_ring(images, **{"projection": None, "focal": None, **bad})


def test_a_ring_of_pairs_takes_three_images():
    from ransac_with_homography_amd import ransac
    with pytest.raises(ValueError, match="ring"):
        ransac.stitch_sequence([sc.random_image(20, 20, 1)] * 2, pairs="ring")
    with pytest.raises(ValueError):
        ransac.stitch_sequence([sc.random_image(20, 20, 1)] * 3, pairs="circle")


@pytest.mark.parametrize("kind", rc.SURFACES)
def test_without_wrap_the_plan_is_what_it_was(hg, kind):
    images, Hs = pc.sweep(3, 3)
    shapes = [im.shape for im in images]
    a, b = hg.sequence_plan(shapes, Hs, 1, kind, 40.0), hg.sequence_plan(shapes, Hs, 1, kind, 40.0, wrap=False)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    assert a[1] == pc.rectangles(shapes, pc.orient(sc.chain(Hs, 1)), 1, kind, 40.0)
    x, y = hg._sequence_inputs("test", images, Hs, None, 1, kind, 40.0), hg._sequence_inputs("test", images, Hs, None, 1, kind, 40.0, False)
    assert x[:4] == y[:4] and np.array_equal(x[4], y[4]) and all(np.array_equal(p, q) for p, q in zip(x[5], y[5]))
    planar = hg.sequence_plan(shapes, Hs, 1, wrap=False)
    assert planar[1][1] == (0, 0, shapes[1][1], shapes[1][0])
    # across the seam: refused without wrap, taken with it
    K = pc.camera((120, 160), 100.0)
    step = K @ pc.rotation(np.deg2rad(30.0)) @ np.linalg.inv(K)
    with pytest.raises(ValueError, match="seam"):
        hg.sequence_plan([(120, 160, 3)] * 6, [step] * 5, 0, kind, 100.0)
    assert hg.sequence_plan([(120, 160, 3)] * 6, [step] * 5, 0, kind, 100.0, wrap=True)[3][1] == 512


@pytest.mark.parametrize("kind", rc.SURFACES)
def test_a_pole_inside_an_image_is_still_refused(hg, kind):
    K = pc.camera((120, 160), 100.0)
    up = K @ pc.rotation(0.0, np.deg2rad(90.0)) @ np.linalg.inv(K)
    with pytest.raises(ValueError, match="pole|finite"):
        hg.sequence_plan([(120, 160, 3)] * 2, [up], 0, kind, 100.0, wrap=True)
    with pytest.raises(ValueError, match="determinant"):
        hg.sequence_plan([(120, 160, 3)] * 2, [np.array([[1.0, 0.0, 5.0], [0.0, 1.0, 0.0], [1.0, 0.0, 5.0]])], 0, kind, 100.0, wrap=True)


# ---- the library's refusals ----
def test_c_level_refusals(lib):
    images, t = rc.circle_tables(256, "spherical")
    fh = t["size"][0]

    def every(tweak=None, size=None, paste=None):
        """The three twins on spoilt tables -> their statuses; nothing is written when one refuses."""
        st, can = rc.host_twin(lib, images, t, tweak=tweak, size=size, **(paste or {}))
        assert st == 0 or (can == 0xA5).all()
        s2, count, total = rc.host_stats_twin(lib, images, t, 1, tweak=tweak, size=size)
        assert s2 == 0 or ((count.view(np.uint8) == 0xA5).all() and (total.view(np.uint8) == 0xA5).all())
        s3, can3 = rc.host_multiband_twin(lib, images, t, 2, tweak=tweak, size=size)
        assert s3 == 0 or (can3 == 0xA5).all()
        return st, s2, s3

    assert every() == (0, 0, 0)
    col255, col257 = np.ascontiguousarray(t["col"][:255]), np.ascontiguousarray(np.concatenate([t["col"], t["col"][:1]]))
    assert every(lambda t, p: t.update(col=col255), size=(fh, 255)) == (INVALID,) * 3
    assert every(lambda t, p: t.update(col=col257), size=(fh, 257)) == (INVALID,) * 3
    assert every(lambda t, p: t["rects"].__setitem__((3, 0), -1)) == (INVALID,) * 3
    assert every(lambda t, p: t["rects"].__setitem__((3, 0), 256)) == (INVALID,) * 3
    assert every(lambda t, p: t["rects"].__setitem__((3, 2), 257)) == (INVALID,) * 3
    assert every(lambda t, p: t["rects"].__setitem__((3, 2), 0)) == (INVALID,) * 3
    assert every(lambda t, p: t["rects"].__setitem__((3, 1), -1)) == (INVALID,) * 3
    assert every(lambda t, p: t["rects"].__setitem__((3, 3), fh + 1)) == (INVALID,) * 3
    # allowed: a rectangle a period wide wherever it starts, and one that ends past the edge
    assert every(lambda t, p: t["rects"].__setitem__((3, slice(0, 3, 2)), (255, 256))) == (0, 0, 0)
    assert every(lambda t, p: t.update(col=None)) == (INVALID,) * 3
    assert every(lambda t, p: t.update(row=None)) == (INVALID,) * 3
    odd = np.zeros(2 * 256 * 8 + 8, dtype=np.uint8)
    off = (4 - odd.ctypes.data) % 8                                              # an address that is 4 modulo 8
    skew = odd[off:off + 2 * 256 * 8].view(np.float64).reshape(256, 2)
    skew[:] = t["col"]
    assert skew.ctypes.data % 8 == 4
    assert every(lambda t, p: t.update(col=skew)) == (INVALID,) * 3
    for bad in (np.nan, np.inf):
        assert every(lambda t, p: t["m"].__setitem__((0, 0), bad)) == (INVALID,) * 3      # no image is exempt: there is no anchor
    assert every(lambda t, p: p.__setitem__(1, 0)) == (INVALID,) * 3
    assert every(lambda t, p: t["hw"].__setitem__((0, 0), 1)) == (INVALID,) * 3
    assert every(lambda t, p: t.update(order=np.zeros(12, dtype=np.int32)))[0] == INVALID
    assert every(paste=dict(rows=(2, 1)))[0] == INVALID and every(paste=dict(blend=2))[0] == INVALID
    assert every(paste=dict(gains=[0.0] * 12))[0] == INVALID
    assert rc.host_stats_twin(lib, images, t, 0)[0] == INVALID and rc.host_stats_twin(lib, images, t, 256)[0] == INVALID
    assert rc.host_multiband_twin(lib, images, t, 0)[0] == INVALID and rc.host_multiband_twin(lib, images, t, 9)[0] == INVALID
    # the size of the multi-band workspace: positive for what the call takes, <= 0 for what it refuses
    assert rc.workspace_bytes(lib, t, 5) > rc.workspace_bytes(lib, t, 1) > 0
    for bad in (dict(bands=0), dict(bands=9), dict(bands=2, size=(fh, 255)), dict(bands=2, size=(fh, 257)), dict(bands=2, size=(fh - 1, 256))):
        assert rc.workspace_bytes(lib, t, **bad) <= 0
    wide = dict(t, rects=t["rects"].copy())
    wide["rects"][3, 2] = 257
    assert rc.workspace_bytes(lib, wide, 2) <= 0
    # the projected and planar entry points go on refusing a rectangle that leaves the canvas
    st, can = pc.host_twin(lib, images, None, t=dict(t, rects=t["rects"].copy(), m=t["m"].copy()))
    assert st == INVALID and (can == 0xA5).all()


def test_exports(lib):
    from ransac_with_homography_amd import _lib
    for name in ("rwh_stitch_sequence_ring", "rwh_host_stitch_sequence_ring", "rwh_sequence_overlap_stats_ring", "rwh_host_sequence_overlap_stats_ring",
                 "rwh_stitch_multiband_ring_workspace_bytes", "rwh_stitch_multiband_ring", "rwh_host_stitch_multiband_ring"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    from ransac_with_homography_amd import homography, kernels, ransac
    assert ransac.sequence_period is homography.sequence_period
    for name in ("stitch_sequence_ring", "sequence_overlap_tables_ring", "stitch_sequence_multiband_ring"):
        assert callable(getattr(kernels, name))
