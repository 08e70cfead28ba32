"""Rules 6 - 8 of the extractor (include/rwh.h: the scale pyramid) without a GPU: the host twins rwh_host_orb_pyramid and
rwh_host_orb_extract_pyramid against the numpy restatement of tests/orb_pyramid_cases.py, exact equality everywhere; the properties
the rules state (level shapes, the edge rule, a level is an image, quotas, the map back to the image); a pair of images that
differs in zoom by 1.5, the reason for the pyramid; argument validation of the tables and of the entry points."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import match_cases as mc
import orb_cases as oc
import orb_pyramid_cases as pc

null = ctypes.c_void_p(0)
one = ctypes.c_void_p(8)             # non-NULL and aligned, never dereferenced: validation comes first


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ransac_with_homography_amd import _lib
    return _lib.load()


def _tables():
    import ransac as rs
    return [rs.orb_scales(4), pc.CALLER_SCALES]


def test_planes_equal_restatement(lib):
    assert _tables()[0].tolist() == [256, 307, 369, 442]
    for name, img in pc.plane_images():
        for scales in _tables():
            st, got = pc.host_planes(lib, img, scales)
            want = pc.planes(img, scales)
            assert st == 0 and len(got) == len(want) == len(scales) - 1
            for s, g, w in zip(scales[1:], got, want):
                assert g.shape == w.shape == (pc.level_side(img.shape[0], s), pc.level_side(img.shape[1], s)) and np.array_equal(g, w), (name, s)
    # the rounding of a level's side: 97 * 256 / 307 = 80.89 -> 81, 131 * 256 / 300 = 111.79 -> 112, 33 * 256 / 1024 = 8.25 -> 8
    assert (pc.level_side(97, 307), pc.level_side(131, 300), pc.level_side(33, 1024)) == (81, 112, 8)


def _direct(gp, X, Y, s):
    """Rule 6's double sum for one pixel on a plane that was padded far enough: no index is clamped."""
    total = 0
    for i in range(Y * s // 256, ((Y + 1) * s - 1) // 256 + 1):
        wy = min((Y + 1) * s, 256 * (i + 1)) - max(Y * s, 256 * i)
        for j in range(X * s // 256, ((X + 1) * s - 1) // 256 + 1):
            total += wy * (min((X + 1) * s, 256 * (j + 1)) - max(X * s, 256 * j)) * int(gp[i, j])
    return (total + s * s // 2) // (s * s)


def test_a_tie_rounds_the_side_up_and_the_overshoot_reads_the_edge(lib):
    """34 x 42 at s = 1024: 256 * 34 + 512 = 9 * 1024 and 256 * 42 + 512 = 11 * 1024 exactly -- 8.5 and 10.5 round up to 9 and 11, so
    the last row and column of the level reach two source pixels, half a footprint, past the image.  They equal the rule on the
    image padded with copies of its last row and column; so do those of 97 x 131 at s = 307 and 300, which overshoot by less."""
    for img, scales in ((oc.random_image(34, 42, 31, channels=1), np.array([256, 1024], dtype=np.int32)),
                        (oc.gray(pc.plane_images()[0][1]), np.array([256, 307], dtype=np.int32)),
                        (oc.gray(pc.plane_images()[0][1]), np.array([256, 300], dtype=np.int32))):
        s = int(scales[1])
        st, (p,) = pc.host_planes(lib, img, scales)
        h, w = img.shape
        hl, wl = p.shape
        assert st == 0 and hl * s > 256 * h and (wl * s > 256 * w or s == 307)          # the last row overshoots, and but for 307 the last column
        if s == 1024:
            assert (hl, wl) == (9, 11) and (256 * h + 512) % 1024 == 0 and (256 * w + 512) % 1024 == 0
            assert lib.rwh_orb_pyramid_bytes(h, w, scales.ctypes.data, 2) == 99
        gp = np.pad(img, ((0, 4), (0, 4)), mode="edge")
        assert all(int(p[Y, wl - 1]) == _direct(gp, wl - 1, Y, s) for Y in range(hl))
        assert all(int(p[hl - 1, X]) == _direct(gp, X, hl - 1, s) for X in range(wl))
        assert int(p[3, 4]) == _direct(gp, 4, 3, s)
        zero = np.pad(img, ((0, 4), (0, 4)))                                          # and they do not equal the rule on zeros
        assert any(int(p[hl - 1, X]) != _direct(zero, X, hl - 1, s) for X in range(wl))


def test_constant_and_checkerboard(lib):
    import ransac as rs
    flat = np.full((50, 61, 3), 77, dtype=np.uint8)
    st, got = pc.host_planes(lib, flat, rs.orb_scales(8))
    assert st == 0 and len(got) == 7 and all(g.size and (g == oc.gray(flat)[0, 0]).all() for g in got)
    # pitch 1, even sides, s = 512 and 1024: every footprint holds as many 255 as 0 -- 127.5, and the rule rounds half up
    yy, xx = np.mgrid[0:40, 0:48]
    board = (255 * ((xx + yy) % 2)).astype(np.uint8)
    st, got = pc.host_planes(lib, board, [256, 512, 1024])
    assert st == 0 and [g.shape for g in got] == [(20, 24), (10, 12)] and all((g == 128).all() for g in got)
    # any other scale: 127 or 128 wherever the footprint is balanced, and never outside what an average of 0 and 255 can be
    st, got = pc.host_planes(lib, board, rs.orb_scales(4))
    assert st == 0 and all(np.array_equal(g, w) for g, w in zip(got, pc.planes(board, rs.orb_scales(4))))


@pytest.fixture(scope="module")
def whole(lib):
    """name -> (image, scales, quotas, restatement, host twin) for the plane images, both tables, quotas of 300 features."""
    import ransac as rs
    out = {}
    for name, img in pc.plane_images():
        for scales in _tables():
            quotas = rs.orb_level_quotas(300, scales)
            st, got = pc.host_extract_pyramid(lib, img, scales, quotas)
            assert st == 0
            out[(name, len(scales))] = (img, scales, quotas, pc.restate_pyramid(img, scales, quotas), got)
    return out


def test_whole_rule_equals_restatement(whole):
    for key, (img, scales, quotas, want, got) in whole.items():
        assert pc.same(got, want), key
        assert (np.diff(got["level"]) >= 0).all() and all((got["level"] == l).sum() == min(f, q) for l, (f, q) in enumerate(zip(got["found"], quotas)))
    rgb = whole[("97x131 rgb", 4)][3]
    assert rgb["found"][0] > rgb["found"][1] > rgb["found"][2] > rgb["found"][3] > 0 and len(rgb["score"]) > 250
    assert sorted(set(rgb["size"].tolist())) == [31.0, 31 * 307 / 256, 31 * 369 / 256, 31 * 442 / 256]
    # 40 x 203: level 1 is 33 x 169, one legal row; levels 2 and 3 are lower than 33 and hold nothing, and nothing is raised;
    # 33 x 33: noise around a single legal centre, and levels of 28, 23 and 19 pixels
    assert whole[("40x203 gray", 4)][3]["found"][2:] == [0, 0] and whole[("40x203 gray", 4)][3]["found"][1] > 0
    assert whole[("33x33", 4)][3]["found"][1:] == [0, 0, 0] and whole[("33x33", 3)][3]["found"][1:] == [0, 0]


def test_one_level_is_the_one_scale_rule(lib):
    for name, img, kw in oc.cpu_cases():
        nf = kw.get("n_features", 500)
        rest = {k: v for k, v in kw.items() if k != "n_features"}
        st0, want = oc.host_extract(lib, img, **kw)
        st, got = pc.host_extract_pyramid(lib, img, [256], [nf], **rest)
        assert st == st0 == 0 and got["found"] == [want["found"]], name
        assert all(got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]) for k in ("kps", "desc", "score", "bin")), name
        assert (got["level"] == 0).all() and (got["size"] == 31).all()


def test_a_level_is_an_image(lib):
    """The level-2 plane of an image, extracted on one scale, is the level-2 slice of the image's pyramid extraction."""
    import ransac as rs
    img = pc.textured(150, 200, seed=5)
    scales = rs.orb_scales(4)
    s = int(scales[2])
    st, (_, P, _) = pc.host_planes(lib, img, scales)
    st1, alone = oc.host_extract(lib, P, n_features=5000)
    st2, pyr = pc.host_extract_pyramid(lib, img, scales, [5000] * 4)
    assert st == st1 == st2 == 0 and max(pyr["found"]) < 5000 and alone["found"] == pyr["found"][2] > 20
    cut = pyr["level"] == 2
    assert all(np.array_equal(pyr[k][cut], alone[k]) for k in ("desc", "score", "bin"))
    k = alone["kps"].astype(np.int64)
    assert np.array_equal(k.astype(np.float32), alone["kps"])
    assert np.array_equal(pyr["kps"][cut], np.stack([pc.back_map(k[:, 0], s), pc.back_map(k[:, 1], s)], axis=1))
    assert (pyr["size"][cut] == np.float32(31 * s / 256)).all()


def test_quotas(lib):
    import ransac as rs
    for n in (0, 1, 7, 500, 5000, 123457):
        for scales in (rs.orb_scales(8), rs.orb_scales(1), pc.CALLER_SCALES, rs.orb_scales(16, 1.09)):
            q = rs.orb_level_quotas(n, scales)
            assert q.dtype == np.int32 and q.shape == scales.shape and int(q.sum()) == n and (q >= 0).all() and (np.diff(q) <= 0).all()
    assert rs.orb_level_quotas(500, rs.orb_scales(8)).tolist() == [112, 90, 75, 62, 52, 43, 36, 30]
    # level 0 finds fewer than its quota and keeps them all; the others are cut at theirs and get nothing of level 0's room
    img = pc.textured()
    scales = rs.orb_scales(4)
    st, got = pc.host_extract_pyramid(lib, img, scales, [1000, 5, 0, 6])
    assert st == 0 and 5 < got["found"][0] < 1000 and min(got["found"][1:]) > 6
    assert np.bincount(got["level"], minlength=4).tolist() == [got["found"][0], 5, 0, 6]
    assert pc.same(got, pc.restate_pyramid(img, scales, [1000, 5, 0, 6]))


def test_back_map(lib):
    """Rule 8: the reported coordinate is np.float32(Fraction((2 x + 1) s - 256, 512)).  The host twin is asked through noise at
    threshold 0, where the first two legal columns, x = 16 and 17, hold keypoints on every level; the widest coordinate, 65519,
    exists only on level 0 (no level of a 65536-wide image is that wide), where the twin is asked through orb_cases.wide_image;
    the package's own map (features._orb_level_to_image, which extract_batch applies on the device) is asked for all three columns
    and every default scale on CPU tensors."""
    import torch
    import ransac as rs
    from ransac_with_homography_amd import features as impl
    scales = rs.orb_scales(8)
    exact = lambda x, s: np.float32(Fraction((2 * int(x) + 1) * int(s) - 256, 512))
    img = oc.random_image(200, 200, 41, channels=1)
    st, got = pc.host_extract_pyramid(lib, img, scales, [4000] * 8, threshold=0)
    want = pc.restate_pyramid(img, scales, [4000] * 8, threshold=0)
    assert st == 0 and pc.same(got, want)
    for l, s in enumerate(scales.tolist()):
        cut = want["level"] == l
        xs = want["xy_level"][cut]
        assert {16, 17} <= set(xs[:, 0].tolist()) and {16, 17} <= set(xs[:, 1].tolist()), l
        rep = got["kps"][cut]
        assert all(rep[i, 0] == exact(xs[i, 0], s) and rep[i, 1] == exact(xs[i, 1], s) for i in range(len(xs)))
    wide, strong, _ = oc.wide_image()
    st, got = pc.host_extract_pyramid(lib, wide, [256, 1024], [100, 100])
    assert st == 0 and [float(oc.WIDE_W - 1 - oc.BORDER), 16.0] in got["kps"].tolist() and exact(65535 - 16, 256) == 65519
    for s in scales.tolist():
        for x in (16, 17, 65535 - 16):
            rep = impl._orb_level_to_image(torch.tensor([[float(x), float(x)]], dtype=torch.float32), torch.tensor([[float(s)]], dtype=torch.float64))
            assert rep.dtype == torch.float32 and rep.numpy()[0, 0] == exact(x, s) == pc.back_map(np.array([x]), s)[0]
    assert exact(16, 256) == 16 and exact(65519, 917) != np.float32(65519 * 917 / 256)   # not the corner of the footprint


def test_scale_change(lib):
    """The reason for the pyramid.  A: 256 x 320 of rectangles and discs; B: A shrunk by 1.5 with a bilinear resampler of the test's
    own.  Features of both with 8 levels and with 1 (n_features 500, threshold 20), matched by rwh_host_match_hamming; a match
    agrees when its pair obeys x_B = (x_A + 0.5) / 1.5 - 0.5 within 3 px.
    Measured when this was written: 8 levels -- 303 matches, 225 agree; 1 level -- 88 matches, 15 agree."""
    import ransac as rs
    A = pc.textured()
    B = pc.shrink_bilinear(A)
    assert A.shape == (256, 320) and B.shape == (170, 213)
    agree = {}
    for levels in (8, 1):
        scales = rs.orb_scales(levels)
        quotas = rs.orb_level_quotas(500, scales)
        (sa, a), (sb, b) = (pc.host_extract_pyramid(lib, im, scales, quotas) for im in (A, B))
        st, train, _ = mc.host_match(lib, a["desc"], b["desc"])
        assert sa == sb == st == 0
        agree[levels] = pc.agreeing(a["kps"], b["kps"], train)
        print("scale change, %d level(s): %d matches, %d agree" % (levels, int((train >= 0).sum()), agree[levels]))
    assert agree[8] > agree[1]
    assert agree[8] >= 113                                                    # half of the 225 measured


def test_table_helpers_and_their_errors():
    import ransac as rs
    assert rs.orb_scales().tolist() == [256, 307, 369, 442, 531, 637, 764, 917] and rs.orb_scales(1).tolist() == [256]
    assert rs.orb_scales(3, 2.0).tolist() == [256, 512, 1024] and rs.orb_scales(3, 2.0).dtype == np.int32
    for bad in ((0,), (17,), (-1,), (9, 1.2), (4, 2.0), (3, 1.0), (3, 0.9), (2, 1.001), (3, float("inf")), (3, float("nan"))):
        with pytest.raises(ValueError):
            rs.orb_scales(*bad)
    for bad in ([], [256] * 2, [255, 300], [256, 1025], [256, 400, 400], [256.0, 300.0], [[256, 300]], list(range(256, 273))):
        with pytest.raises(ValueError):
            rs.orb_level_quotas(10, bad)
    with pytest.raises(ValueError):
        rs.orb_level_quotas(-1, [256, 300])


def test_layout_equals_the_restatement():
    """features.orb_layout -- the buffer and table extract_batch and tools/orb_probe.py hand to the library -- against
    orb_pyramid_cases.layout, which was written from include/rwh.h on its own: the table, where the planes start and where they end;
    gray_bytes is the sum of every level's area.  One level, four, and the caller's table with its level of scale 1024; a 1 x 40
    image whose level at 1024 has no rows, (256 + 512) // 1024 = 0."""
    import ransac as rs
    from ransac_with_homography_amd import features
    shape = lambda im: (im.shape[0], im.shape[1], 1 if im.ndim == 2 else im.shape[2])
    thin = oc.random_image(1, 40, 51, channels=1)
    batch = [img for _, img in pc.plane_images()] + pc.gpu_images() + [thin]
    cases = [(batch, sc) for sc in (np.array([256], dtype=np.int32), rs.orb_scales(4), pc.CALLER_SCALES)]
    cases.append(([thin], np.array([256, 1024], dtype=np.int32)))
    for images, scales in cases:
        table, planes_offset, images_bytes, gray_bytes, full = features.orb_layout([shape(im) for im in images], scales)
        head, want, off, end, _ = pc.layout(images, scales, gap=0)
        assert table.dtype == want.dtype == np.int64 and table.shape == (len(images) * len(scales), 5) and np.array_equal(table, want)
        assert planes_offset == off == head.size and images_bytes == end
        assert gray_bytes == sum(pc.level_side(im.shape[0], s) * pc.level_side(im.shape[1], s) for im in images for s in scales.tolist())
    assert table.tolist() == [[0, 0, 1, 40, 1], [0, 0, 0, 0, 1]] and (planes_offset, images_bytes, gray_bytes, full) == (40, 40, 40, 1)


def test_layout_full_is_a_bound(lib):
    """`full`, the room of the overflow retry, holds every keypoint there can be: no image of the CPU cases finds more, and an image
    without a legal centre (32 x 32) still gets room for one."""
    from ransac_with_homography_amd import features
    one = np.array([256], dtype=np.int32)
    for name, img, kw in oc.cpu_cases():
        st, got = oc.host_extract(lib, img, **kw)
        full = features.orb_layout([(img.shape[0], img.shape[1], 1 if img.ndim == 2 else img.shape[2])], one)[4]
        assert st == 0 and 0 <= got["found"] <= full, name
    assert features.orb_layout([(32, 32, 3)], one)[4] == 1 and features.orb_layout([(32, 32, 3), (33, 35, 1)], one)[4] == 2


def test_import_surface():
    """Every name of the top-level `ransac` module comes from ransac_with_homography_amd.ransac; the names that live in features.py
    are the same objects there, the hand-off type among them."""
    import ransac as shim
    from ransac_with_homography_amd import features
    from ransac_with_homography_amd import ransac as impl
    names = [n for n in vars(shim) if not n.startswith("__")]
    assert len(names) == 25 and all(getattr(shim, n) is getattr(impl, n) for n in names)
    moved = {"DeviceProblems", "match_descriptors", "match_batch", "extract_batch", "detect_and_describe", "default_pattern",
             "rotate_pattern", "orb_bin_table", "orb_scales", "orb_level_quotas"}
    assert moved <= set(names) and all(getattr(impl, n) is getattr(features, n) for n in moved)
    assert impl.DeviceProblems is features.DeviceProblems and impl.run_batch.__module__ == impl.__name__


def test_entry_points_refuse_bad_arguments(lib):
    from ransac_with_homography_amd import _lib
    assert (_lib.RWH_ORB_SCALE_ONE, _lib.RWH_ORB_SCALE_MAX, _lib.RWH_ORB_LEVELS_MAX, _lib.RWH_ORB_PYR_TILE_W, _lib.RWH_ORB_PYR_TILE_H) == (256, 1024, 16, 64, 16)
    arr = lambda v: np.array(v, dtype=np.int32)
    good = arr([256, 300, 1024])
    bad_tables = [arr([255, 300]), arr([256, 256]), arr([256, 300, 299]), arr([256, 1025]), arr([300]), arr(list(range(256, 273)))]
    assert lib.rwh_orb_pyramid_bytes(97, 131, good.ctypes.data, 3) == 83 * 112 + 24 * 33 and lib.rwh_orb_pyramid_bytes(97, 131, good.ctypes.data, 1) == 0
    for t in bad_tables:
        assert lib.rwh_orb_pyramid_bytes(97, 131, t.ctypes.data, len(t)) == _lib.RWH_E_INVALID, t
    assert lib.rwh_orb_pyramid_bytes(97, 131, good.ctypes.data, 0) == -1 and lib.rwh_orb_pyramid_bytes(97, 131, null, 2) == -1
    assert lib.rwh_orb_pyramid_bytes(0, 131, good.ctypes.data, 3) == -1 and lib.rwh_orb_pyramid_bytes(97, 65537, good.ctypes.data, 3) == -1
    # the device entry point: every refusal comes before any device work, so none is needed here
    dev = lambda images=one, nbytes=1000, off=500, table=one, n=2, scales=good, levels=3, ws=one, ws_bytes=56: \
        lib.rwh_orb_pyramid_batched(images, nbytes, off, table, n, scales.ctypes.data if scales is not None else null, levels, ws, ws_bytes, null)
    for kw in (dict(images=null), dict(table=null), dict(ws=null), dict(n=0), dict(scales=None), dict(levels=0), dict(levels=17), dict(off=-1),
               dict(off=1001), dict(ws_bytes=48), dict(ws=ctypes.c_void_p(12)), dict(n=2 ** 30)) + tuple(dict(scales=t, levels=len(t)) for t in bad_tables):
        assert dev(**kw) == _lib.RWH_E_INVALID, kw
    assert dev(scales=arr([256]), levels=1, ws_bytes=24) == 0                   # one level: checked, and nothing to launch
    # the host twins
    img = oc.random_image(40, 48, 1)
    buf = np.zeros(4096, dtype=np.uint8)
    hp = lambda im=img.ctypes.data, h=40, w=48, c=3, scales=good, levels=3, out=buf.ctypes.data, room=4096: \
        lib.rwh_host_orb_pyramid(im, h, w, c, scales.ctypes.data, levels, out, room)
    assert hp() == 0 and hp(room=34 * 41 + 10 * 12) == 0
    for kw in (dict(im=null), dict(h=0), dict(w=65537), dict(levels=0), dict(out=null), dict(room=34 * 41 + 10 * 12 - 1)) + \
            tuple(dict(scales=t, levels=len(t)) for t in bad_tables):
        assert hp(**kw) == _lib.RWH_E_INVALID, kw
    assert hp(c=2) == _lib.RWH_E_UNSUPPORTED
    ok = pc.host_extract_pyramid(lib, img, good, [10, 10, 10])
    assert ok[0] == 0 and len(ok[1]["score"]) == 10 + ok[1]["found"][1] and ok[1]["found"][2] == 0
    assert pc.host_extract_pyramid(lib, img, good, [10, -1, 10])[0] == _lib.RWH_E_INVALID
    out = np.zeros(4, dtype=np.int32)
    raw = lambda quotas, nbytes=32: lib.rwh_host_orb_extract_pyramid(img.ctypes.data, 40, 48, 3, 20, good.ctypes.data, quotas.ctypes.data, 3, one, one,
                                                                     nbytes, one, one, one, one, one, one, out.ctypes.data, null)
    assert raw(arr([2 ** 30, 2 ** 30, 2 ** 30])) == _lib.RWH_E_INVALID          # room for 3 * 2^30 keypoints: refused before anything is read
    assert raw(arr([1, 1, 1]), nbytes=65) == _lib.RWH_E_UNSUPPORTED and raw(arr([1, 1, 1]), nbytes=0) == _lib.RWH_E_UNSUPPORTED
    assert pc.host_extract_pyramid(lib, img, bad_tables[1], [10, 10])[0] == _lib.RWH_E_INVALID
    assert pc.host_extract_pyramid(lib, img, good, [10, 10, 10], threshold=255)[0] == _lib.RWH_E_INVALID
    assert pc.host_extract_pyramid(lib, img[:, :, :2], good, [10, 10, 10])[0] == _lib.RWH_E_UNSUPPORTED
    st, none = pc.host_extract_pyramid(lib, img, good, [0, 0, 0])
    assert st == 0 and len(none["score"]) == 0 and none["found"] == ok[1]["found"]
