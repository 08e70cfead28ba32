"""The seam rule without a GPU: rwh_host_sequence_seams (the host twin: Dijkstra with a binary heap over per-image windows) against
the numpy restatement of tests/seam_cases.py (Jacobi sweeps over whole-canvas planes), the rule's stated consequences, what seam
finding is for, the two compositors that take labels, the refusals, and the Python layer's checks.  Every comparison is exact."""
import inspect

import numpy as np
import pytest

import gain_cases as gc
import multiband_cases as mc
import projection_cases as pc
import seam_cases as sm
import sequence_cases as sc


@pytest.fixture(scope="module")
def lib():
    return sc.library()


GENERAL = sc.general_cases()
EDGES = sc.edge_canvases()
PROJECTED = [(kind,) + pc.general_cases()[1] for kind in pc.SURFACES]       # one cylinder and one sphere case: "n3 anchor 0"


# ---- twin equals restatement ----
@pytest.mark.parametrize("gains", (False, True), ids=("plain", "gains"))
@pytest.mark.parametrize("case", GENERAL, ids=[c[0].replace(" ", "-") for c in GENERAL])
def test_twin_is_the_restatement_on_general_cases(lib, case, gains):
    _, images, Gs, anchor, _ = case
    g = gc.mixed_gains(len(images)) if gains else None
    for margin, tau in ((sm.MARGIN, sm.TAU), (2.0, 200), (0.0, 766)):
        assert np.array_equal(sm.host(lib, images, Gs, anchor, g, margin, tau), sm.restate(images, Gs, anchor, g, margin, tau)), (margin, tau)


@pytest.mark.parametrize("case", EDGES, ids=["fw%d-fh%d" % (c[0], c[1]) for c in EDGES])
def test_twin_is_the_restatement_on_edge_canvases(lib, case):
    _, _, images, Gs, _, _ = case
    for g in (None, gc.mixed_gains(len(images))):
        assert np.array_equal(sm.host(lib, images, Gs, 0, g, 2.0), sm.restate(images, Gs, 0, g, 2.0))


@pytest.mark.parametrize("case", PROJECTED, ids=[c[0] for c in PROJECTED])
def test_twin_is_the_restatement_on_a_curved_canvas(lib, case):
    kind, _, images, Gs, anchor, _, f = case
    for g in (None, gc.mixed_gains(len(images))):
        got = sm.host_proj(lib, images, Gs, anchor, kind, f, g, 3.0)
        assert np.array_equal(got, sm.restate_proj(images, Gs, anchor, kind, f, g, 3.0))
        assert len(np.unique(got[got != sm.NONE])) == len(images)


def test_three_way_overlap_and_a_strip_of_64(lib):
    images, Gs = sm.three_way()
    info = {}
    ref = sm.restate(images, Gs, 0, info=info)
    assert (info["cover"].sum(axis=0) == 3).sum() > 1000                 # all three meet
    assert np.array_equal(sm.host(lib, images, Gs, 0), ref) and set(np.unique(ref)) == {0, 1, 2, sm.NONE}
    images, Gs = sc.translated_strip(64)
    for margin in (1.0, sm.MARGIN):
        ref = sm.restate(images, Gs, 0, margin=margin)
        assert np.array_equal(sm.host(lib, images, Gs, 0, margin=margin), ref)
    assert len(np.unique(sm.restate(images, Gs, 0, margin=1.0))) == 65   # every image of the strip owns something, and 255


# ---- the consequences ----
def test_infinite_margin_is_the_feather_winner(lib):
    for name, images, Gs, anchor, _ in GENERAL:
        info = {}
        sm.restate(images, Gs, anchor, info=info)
        lab = sm.host(lib, images, Gs, anchor, margin=np.inf)
        assert np.array_equal(lab, info["w"]), name
        st, can = sm.host_multiband(lib, images, Gs, lab, anchor, 3)
        assert st == 0 and np.array_equal(can, mc.host(lib, images, Gs, anchor, 3)), name


def test_planes_that_name_nobody_give_the_unlabelled_canvas(lib):
    for name, images, Gs, anchor, _ in GENERAL:
        ref = mc.host(lib, images, Gs, anchor, 3)
        fh, fw = ref.shape[:2]
        rng = np.random.default_rng(5)
        for plane in (np.full((fh, fw), 0xff, dtype=np.uint8), rng.integers(len(images), 256, (fh, fw)).astype(np.uint8)):
            st, can = sm.host_multiband(lib, images, Gs, plane, anchor, 3)
            assert st == 0 and np.array_equal(can, ref), name


def test_a_label_of_an_image_that_does_not_cover_is_ignored(lib):
    """Every label valid as an index, few of them covering: where the named image does not cover, the feather winner stands."""
    _, images, Gs, anchor, _ = GENERAL[4]
    _, _, cover, byt, gw = mc.image_planes(images, Gs, anchor)
    w = sm.survey(cover, byt, gw)[0]
    plane = np.random.default_rng(6).integers(0, len(images), w.shape).astype(np.uint8)
    named = np.take_along_axis(cover, plane[None].astype(np.int64), axis=0)[0]
    assert named.any() and (~named & cover.any(axis=0)).any()
    owner = np.where(named, plane, w)
    st, can = sm.host_paste(lib, images, Gs, plane, anchor)
    want = np.where(cover.any(axis=0)[..., None], np.take_along_axis(byt, np.minimum(owner, len(images) - 1)[None, :, :, None].astype(np.int64), axis=0)[0], 0)
    assert st == 0 and np.array_equal(can, want.astype(np.uint8))
    st, a = sm.host_multiband(lib, images, Gs, plane, anchor, 2)
    st2, b = sm.host_multiband(lib, images, Gs, owner.astype(np.uint8), anchor, 2)
    assert st == 0 and st2 == 0 and np.array_equal(a, b)


def test_tau_one_is_the_nearest_seed_by_breadth_first_search(lib):
    for name, images, Gs, anchor, _ in GENERAL[1:5]:
        info = {}
        ref = sm.restate(images, Gs, anchor, margin=2.0, tau=1, info=info)
        assert (info["c"] == 1).all()
        hops = sm.nearest_seed_bfs(info["cover"], info["seed"])
        assert np.array_equal(hops, info["dist"]), name
        assert np.array_equal(sm.labels_of(info["cover"], info["w"], hops), ref)
        assert np.array_equal(sm.host(lib, images, Gs, anchor, margin=2.0, tau=1), ref), name


def test_one_image_owns_what_it_covers(lib):
    lab = sm.host(lib, [sc.random_image(9, 11, 1)], [np.eye(3)])
    assert (lab == 0).all()
    images, Gs = [sc.random_image(20, 30, 2)], [np.eye(3)]
    assert (sm.host(lib, images, Gs, margin=0.0, tau=766) == 0).all()


def test_an_image_inside_another_with_margin_zero_labels_nothing(lib):
    images, Gs = [sc.random_image(40, 50, 3), sc.random_image(12, 14, 4)], [np.eye(3), sc.translate(15, 11)]
    info = {}
    ref = sm.restate(images, Gs, 0, margin=0.0, info=info)
    assert info["cover"][1].sum() > 100 and not info["seed"][1].any()
    assert (ref == 0).all() and np.array_equal(sm.host(lib, images, Gs, 0, margin=0.0), ref)


def test_a_label_always_covers_its_pixel(lib):
    cases = [(images, Gs, anchor) for _, images, Gs, anchor, _ in GENERAL] + [sm.three_way() + (0,), sm.moving_object()[:2] + (0,)]
    for images, Gs, anchor in cases:
        _, _, cover, _, _ = mc.image_planes(images, Gs, anchor)
        for margin, tau in ((sm.MARGIN, sm.TAU), (0.0, 5)):
            lab = sm.host(lib, images, Gs, anchor, margin=margin, tau=tau)
            anyone = cover.any(axis=0)
            assert (lab[~anyone] == sm.NONE).all() and (lab[anyone] < len(images)).all()
            assert np.take_along_axis(cover, np.minimum(lab, len(images) - 1)[None].astype(np.int64), axis=0)[0][anyone].all()


# ---- what seam finding is for ----
def test_a_moving_object_is_swept_whole(lib, capsys):
    """The scene of the issue through the real sampler: a block that only view 0 shows, across the midline of the overlap.  The
    feather winner cuts it in two; the seam rule gives it to one image, and its seam runs where the views agree.  Measured on the
    restatement: the block's labels are {1} against {0, 1} (308 / 352 pixels), the summed disagreement along the seam 0 against 18689."""
    images, Gs, block = sm.moving_object()
    info = {}
    ref = sm.restate(images, Gs, 0, info=info)
    lab = sm.host(lib, images, Gs, 0)
    assert np.array_equal(lab, ref)
    w, d = info["w"], info["d"]
    seam, feather = sm.seam_disagreement(lab, d), sm.seam_disagreement(w, d)
    with capsys.disabled():
        print("\nmoving object: summed d along the seam %d (seam rule) against %d (feather winner); %d sweeps" % (seam, feather, info["sweeps"]))
    assert len(np.unique(lab[block])) == 1 and len(np.unique(w[block])) == 2
    assert (d[block] >= sm.TAU).all() and feather > 0
    assert seam < feather / 2
    st, pasted = sm.host_paste(lib, images, Gs, lab)
    assert st == 0
    owner = int(lab[block][0, 0])
    assert (pasted[block] == 250).all() if owner == 0 else not (pasted[block] == 250).any()


def test_the_serpentine_is_walked_along_its_corridor(lib):
    """The GPU suite's serpentine, checked here first: image 0's seeds reach the corridor's far end only along it -- one step of
    cost 1 per corridor pixel from the end of the first run on, and cutting the corridor anywhere makes the far end dearer."""
    images, Gs, path = sm.serpentine()
    tau = sm.SERPENTINE_TAU
    info = {}
    ref = sm.restate(images, Gs, 0, margin=0.0, tau=tau, info=info)
    assert np.array_equal(sm.host(lib, images, Gs, 0, margin=0.0, tau=tau), ref)
    ys, xs = (np.array(v) for v in zip(*path))
    along = info["dist"][0][ys, xs]
    run = images[0].shape[1] - 2
    assert (info["c"][ys, xs] == 1).all() and (info["c"] == 1).sum() == len(path)
    assert (along[:run] == 1).all() and (np.diff(along[run - 1:]) == 1).all() and along[-1] == len(path) - run + 1
    assert (ref[ys, xs] == 0).all() and (ref == 1).any()
    tw, th = 64, 16
    assert len(set(xs // tw)) >= 3 and len(set(ys // th)) >= 3
    tiles = [(int(y) // th, int(x) // tw) for y, x in path]
    visits = [t for k, t in enumerate(tiles) if k == 0 or tiles[k - 1] != t]
    assert len(visits) > len(set(visits))                                  # it re-enters tiles it has left
    cut = info["c"].copy()
    cut[path[len(path) // 2]] = tau
    assert sm.distances(info["cover"], info["seed"], cut)[0][path[-1]] > along[-1]


# ---- label paste ----
def test_label_paste_with_first_in_order_labels_is_paste(lib):
    for name, images, Gs, anchor, order in GENERAL:
        order = sc.default_order(len(images), anchor) if order is None else order
        for g in (None, gc.mixed_gains(len(images))):
            _, _, cover, _, _ = mc.image_planes(images, Gs, anchor, g)
            st, can = sm.host_paste(lib, images, Gs, sm.first_in_order_labels(cover, order), anchor, g)
            assert st == 0 and np.array_equal(can, sc.host_ex(lib, images, Gs, anchor, sc.PASTE, order, gains=g)), name


def test_label_paste_and_labelled_multiband_on_a_curved_canvas(lib):
    kind, _, images, Gs, anchor, order, f = PROJECTED[0]
    _, cover, _, _ = pc.planes(images, Gs, anchor, kind, f)
    order = sc.default_order(len(images), anchor) if order is None else order
    can = sm.host_paste_proj(lib, images, Gs, sm.first_in_order_labels(cover, order), anchor, kind, f)
    assert np.array_equal(can, pc.host(lib, images, Gs, anchor, kind, f, sc.PASTE, order))
    none = np.full(cover.shape[1:], sm.NONE, dtype=np.uint8)
    assert np.array_equal(sm.host_multiband_proj(lib, images, Gs, none, anchor, kind, f, 2), pc.host_multiband(lib, images, Gs, anchor, kind, f, 2))


# ---- refusals ----
def test_the_library_refuses(lib):
    images, Gs = [sc.random_image(20, 30, 1), sc.random_image(20, 30, 2)], [np.eye(3), sc.translate(12, 3)]
    assert sm.host_twin(lib, images, Gs)[0] == 0
    for margin in (np.nan, -1.0, -np.inf):
        assert sm.host_twin(lib, images, Gs, margin=margin)[0] == -1
    for tau in (0, 767, -5):
        assert sm.host_twin(lib, images, Gs, tau=tau)[0] == -1
    assert sm.host_twin(lib, images, Gs, tau=766, margin=np.inf)[0] == 0
    assert sm.host_twin(lib, images, Gs, gains=[1.0, 0.0])[0] == -1

    def beyond(t, ptrs):
        t["rects"][1, 2] += 1
    assert sm.host_twin(lib, images, Gs, tweak=beyond)[0] == -1
    assert sm.host_multiband(lib, images, Gs, None)[0] == -1 and sm.host_paste(lib, images, Gs, None)[0] == -1
    t = sc.tables(images, Gs, 0)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    st = lib.rwh_host_sequence_seams(ptrs.ctypes.data, t["hw"].ctypes.data, t["inv"].ctypes.data, t["rects"].ctypes.data, 2, 0, None, 8.0, 64,
                                     None, t["size"][0], t["size"][1], 0, 0)
    assert st == -1                                                      # a NULL label plane


def test_the_overflow_bound_is_refused_by_validation_alone(lib):
    """A 65535 x 65535 rectangle with tau 2: 2 wt ht > 2^32 - 3.  Nothing of that size is allocated: the size function and both
    twins refuse on the numbers."""
    rects = np.array([[0, 0, 65535, 65535]], dtype=np.int32)
    assert lib.rwh_sequence_seams_workspace_bytes(rects.ctypes.data, 1, 65535, 65535, 0, 0) <= 0
    img = sc.random_image(4, 4, 1)
    hw, inv, ptrs = np.array([[65535, 65535]], dtype=np.int32), np.eye(3).reshape(1, 9).copy(), np.array([img.ctypes.data], dtype=np.uint64)
    lab = np.zeros(16, dtype=np.uint8)
    assert lib.rwh_host_sequence_seams(ptrs.ctypes.data, hw.ctypes.data, inv.ctypes.data, rects.ctypes.data, 1, 0, None, 8.0, 2,
                                       lab.ctypes.data, 65535, 65535, 0, 0) == -1
    assert lib.rwh_sequence_seams(ptrs.ctypes.data, hw.ctypes.data, inv.ctypes.data, rects.ctypes.data, 1, 0, None, 8.0, 2,
                                  lab.ctypes.data, 65535, 65535, 0, 0, lab.ctypes.data, 16, None, None) == -1
    # the bound itself, on a canvas the other checks take: 20000 x 30000 pixels, tau 7 fits and tau 8 does not
    rects = np.array([[0, 0, 30000, 20000]], dtype=np.int32)
    hw = np.array([[20000, 30000]], dtype=np.int32)
    assert 20000 * 30000 * 7 <= 2 ** 32 - 3 < 20000 * 30000 * 8
    assert lib.rwh_sequence_seams_workspace_bytes(rects.ctypes.data, 1, 20000, 30000, 0, 0) > 0
    assert lib.rwh_sequence_seams(ptrs.ctypes.data, hw.ctypes.data, inv.ctypes.data, rects.ctypes.data, 1, 0, None, 8.0, 8,
                                  lab.ctypes.data, 20000, 30000, 0, 0, lab.ctypes.data, 16, None, None) == -1


def test_the_python_layer_refuses_before_the_gpu():
    import homography as hg
    from ransac_with_homography_amd.ransac import stitch_ring as ring
    images, Hs = [sc.random_image(20, 30, 1), sc.random_image(20, 30, 2)], [sc.translate(12, 3)]
    with pytest.raises(ValueError, match="feather"):
        hg.stitchSequence(images, Hs=Hs, blending="feather", seams=True)
    with pytest.raises(NotImplementedError, match="wrap"):
        hg.stitchSequence(images, Hs=Hs, projection="cylindrical", focal=300.0, wrap=True, seams=True)
    with pytest.raises(NotImplementedError, match="wrap"):
        ring(images, blending="multiband+seams", pairs="adjacent", focal=300.0)
    for bad in ({"tau": 0}, {"tau": 767}, {"tau": 64.0}, {"margin": -1.0}, {"margin": float("nan")}, {"radius": 3}, "yes", np.zeros((3, 3), np.uint8),
                np.zeros((23, 42), np.float32)):
        with pytest.raises(ValueError):
            hg.stitchSequence(images, Hs=Hs, seams=bad)
    for kw in (dict(margin=-1.0), dict(margin=float("nan")), dict(tau=0), dict(tau=767)):
        with pytest.raises(ValueError):
            hg.sequence_seams(images, Hs=Hs, **kw)


def test_the_launchers_refuse_a_ring_geometry_before_the_gpu():
    from ransac_with_homography_amd import kernels
    images = [sc.random_image(20, 30, 1), sc.random_image(20, 30, 2)]          # numpy: a launcher that looked at them would not get past them
    m, rects = np.stack([np.eye(3)] * 2), [(0, 0, 30, 20), (12, 3, 30, 20)]
    ring = kernels.SeqGeometry(m, rects, (24, 256), rays=(np.zeros((256, 2)), np.zeros((24, 2))), ring=True)
    assert ring.form == "_ring" and ring._replace(ring=False).form == "_proj" and kernels.SeqGeometry(m, rects, (24, 256)).form == ""
    lab = np.zeros((24, 256), np.uint8)
    for call in (lambda: kernels.sequence_seams_on(images, ring), lambda: kernels.stitch_sequence_labels_on(images, ring, lab),
                 lambda: kernels.stitch_sequence_multiband_on(images, ring, 2, labels=lab)):
        with pytest.raises(NotImplementedError, match="seam rule"):
            call()


def test_the_signatures_are_pinned():
    import homography as hg
    import ransac as rs
    sig = inspect.signature(hg.stitchSequence)
    assert sig.parameters["seams"].default is None and list(sig.parameters)[-2:] == ["seams", "bands"]
    assert list(inspect.signature(hg.sequence_seams).parameters) == ["images", "Hs", "Gs", "anchor", "gains", "margin", "tau", "info", "projection",
                                                                     "focal"]
    assert inspect.signature(hg.sequence_seams).parameters["margin"].default == 8.0
    assert inspect.signature(hg.sequence_seams).parameters["tau"].default == 64
    assert list(inspect.signature(rs.stitch_sequence).parameters) == [
        "images", "anchor", "th", "d", "k", "ransacMet", "seed", "blending", "features", "info", "gains", "projection", "focal", "pairs", "adjust",
        "bands"]
    from ransac_with_homography_amd import ransac as impl
    assert "sequence_seams" in hg.__all__ and impl.sequence_seams is hg.sequence_seams
    from ransac_with_homography_amd import _lib, kernels
    assert kernels.SEAM_TILE == (_lib.RWH_SEAM_TILE_W, _lib.RWH_SEAM_TILE_H) == (64, 16)
