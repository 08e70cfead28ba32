"""The extractor's rule without a GPU: the host twin (rwh_host_orb_extract) against the numpy restatement of tests/orb_cases.py --
keypoints, their order, scores, bins and descriptor bytes, exact equality -- on every case of orb_cases.cpu_cases; the properties
each case was built for; argument validation of the entry points; the default pattern's invariants."""
import ctypes

import numpy as np
import pytest

import orb_cases as oc

null = ctypes.c_void_p(0)
one = ctypes.c_void_p(8)             # non-NULL and aligned, never dereferenced: validation comes first


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ransac_with_homography_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def results(lib):
    """name -> (image, kwargs, restatement, host twin's result), computed once."""
    out = {}
    for name, img, kw in oc.cpu_cases():
        st, got = oc.host_extract(lib, img, **kw)
        assert st == 0, name
        out[name] = (img, kw, oc.restate(img, **kw), got)
    return out


def test_host_twin_equals_restatement(results):
    for name, (img, kw, want, got) in results.items():
        assert oc.same(got, want), name
    assert sum(len(want["score"]) for _, _, want, _ in results.values()) > 100        # there were keypoints to get right


def test_what_the_cases_were_built_for(results):
    _, _, r, _ = results["random 40x48"]
    x, y = r["kps"][:, 0], r["kps"][:, 1]
    assert x.min() == 16 and x.max() == 31 and y.min() == 16 and y.max() == 23          # first and last legal column and row
    assert (np.diff(-r["score"].astype(np.int64)) >= 0).all() and len(set(r["score"].tolist())) < len(r["score"])
    # RGBA: alpha ignored; gray in: taken as gray
    assert oc.same(results["rgba"][2], r) and oc.same(results["gray"][2], r) and oc.same(results["rgba"][3], r) and oc.same(results["gray"][3], r)
    one_c = results["one centre 33x33"][2]
    assert one_c["kps"].tolist() == [[16.0, 16.0]] and one_c["score"].tolist() == [255] and one_c["bin"].tolist() == [0]    # zero moments: bin 0
    for name in ("too small 32x40", "flat", "threshold 254"):
        assert results[name][2]["found"] == 0 and results[name][2]["kps"].shape == (0, 2), name
    # saturated differences: hundreds of pixels score 255, each beside an equal -- the suppression is strict, so none survives
    S = oc.scores(results["checkerboard"][0])
    assert (S == 255).sum() > 300 and S.max() == 255 and results["checkerboard"][2]["found"] == 0 and len(oc.keypoints(S - (S == 255), 20)[0]) == 0
    t0 = results["threshold 0"][2]
    assert t0["found"] > r["found"] and t0["score"].min() >= 1
    # the order is total: equal scores either side of the cut, the kept ones are the first by (y, x)
    img, kw, tie, _ = results["tie at the cut"]
    full = oc.restate(img, n_features=100)
    assert full["found"] == tie["found"] == 12 and kw["n_features"] == 7 and len(tie["score"]) == 7
    assert full["score"][6] == full["score"][7] == 200 and oc.same(dict(full, **{k: full[k][:7] for k in ("kps", "desc", "score", "bin")}), tie)
    assert tie["kps"][3:].tolist() == [[20.0, 30.0], [28.0, 30.0], [36.0, 30.0], [44.0, 30.0]]
    # a moment vector exactly on a sector boundary belongs to the sector it opens
    b = results["boundary"][2]
    where = {tuple(k): int(v) for k, v in zip(b["kps"].astype(int).tolist(), b["bin"])}
    g = oc.gray(results["boundary"][0])
    bins, m10, m01 = oc.orientation_bins(g, np.array([20, 50]), np.array([24, 24]), oc.tables()[0])
    assert m10.tolist() == [0, 0] and m01.tolist() == [500, -500] and bins.tolist() == [8, 23]
    assert where[(20, 24)] == 8 and where[(50, 24)] == 23
    table = oc.tables()[0]
    assert table[8].tolist() == [0, 32768] and table[23].tolist() == [0, -32768] and table[0].tolist() == [32588, -3425]
    # descriptor lengths: a shorter descriptor is the head of a longer one (the default pattern is a prefix)
    for nb in (1, 61):
        assert np.array_equal(results["nbytes %d" % nb][2]["desc"], results["nbytes 64"][2]["desc"][:, :nb])
    assert np.array_equal(r["desc"], results["nbytes 64"][2]["desc"][:, :32]) and r["desc"].any()
    cp = results["caller's pattern"][2]
    assert cp["desc"].shape == (r["found"], 4) and not np.array_equal(cp["desc"], r["desc"][:, :4]) and np.array_equal(cp["kps"], r["kps"])
    crop = results["foto crop"][2]
    assert crop["found"] > 100 and len(set(crop["bin"].tolist())) > 15                     # real texture, most sectors


def test_default_pattern_invariants():
    import ransac as rs
    p = rs.default_pattern(64)
    assert p.dtype == np.int8 and p.shape == (512, 4) and np.array_equal(p, rs.default_pattern(64))
    q = p.astype(int)
    assert (q[:, 0] ** 2 + q[:, 1] ** 2 <= 169).all() and (q[:, 2] ** 2 + q[:, 3] ** 2 <= 169).all()
    assert ((q[:, 0] != q[:, 2]) | (q[:, 1] != q[:, 3])).all()
    for nb in (1, 32, 61):
        assert np.array_equal(rs.default_pattern(nb), p[:8 * nb])
    assert rs.default_pattern().shape == (256, 4)
    rot = rs.rotate_pattern(p)
    assert rot.dtype == np.int8 and rot.shape == (30, 512, 4) and np.abs(rot.astype(int)).max() <= 13 and np.array_equal(rot[0], p)
    assert np.array_equal(rot[15], -p)                                                      # half a turn
    for bad in (0, 65):
        with pytest.raises(NotImplementedError):
            rs.default_pattern(bad)
    far = p.copy(); far[3] = (13, 1, 0, 0)
    with pytest.raises(ValueError):
        rs.rotate_pattern(far)
    with pytest.raises(ValueError):
        rs.rotate_pattern(p[:12])


def test_argument_validation_without_gpu(lib):
    from ransac_with_homography_amd import _lib
    assert (_lib.RWH_ORB_BORDER, _lib.RWH_ORB_BINS, _lib.RWH_ORB_TILE_W, _lib.RWH_ORB_TILE_H) == (16, 30, 64, 16)
    assert lib.rwh_orb_workspace_bytes(3) == 32 and lib.rwh_orb_workspace_bytes(0) == -1
    det = lambda images=one, table=one, n=2, thr=20, gray=one, keys=one, cap=64, counts=one, ws=one, ws_bytes=24: \
        lib.rwh_orb_detect_batched(images, 100, table, n, thr, gray, 100, keys, cap, counts, ws, ws_bytes, null)
    for kw in (dict(images=null), dict(table=null), dict(gray=null), dict(keys=null), dict(counts=null), dict(ws=null), dict(n=0),
               dict(cap=0), dict(thr=-1), dict(thr=255), dict(ws_bytes=16), dict(ws=ctypes.c_void_p(12))):
        assert det(**kw) == _lib.RWH_E_INVALID, kw
    des = lambda gray=one, table=one, n=2, keys=one, stride=8, counts=one, nf=8, bt=one, pat=one, nbytes=32, kps=one, desc=one, sc=one, bn=one: \
        lib.rwh_orb_describe_batched(gray, 100, table, n, keys, stride, counts, nf, bt, pat, nbytes, kps, desc, sc, bn, null)
    for kw in (dict(gray=null), dict(table=null), dict(keys=null), dict(counts=null), dict(bt=null), dict(pat=null), dict(kps=null),
               dict(desc=null), dict(sc=null), dict(bn=null), dict(n=0), dict(nf=0), dict(stride=0)):
        assert des(**kw) == _lib.RWH_E_INVALID, kw
    assert des(nbytes=0) == _lib.RWH_E_UNSUPPORTED and des(nbytes=65) == _lib.RWH_E_UNSUPPORTED
    # the host twin
    img = oc.random_image(40, 48, 1)
    assert oc.host_extract(lib, img, threshold=255)[0] == _lib.RWH_E_INVALID and oc.host_extract(lib, img, threshold=-1)[0] == _lib.RWH_E_INVALID
    assert oc.host_extract(lib, img, n_features=-1)[0] == _lib.RWH_E_INVALID
    assert oc.host_extract(lib, img[:, :, :2])[0] == _lib.RWH_E_UNSUPPORTED
    rot = oc.tables(32)[1].copy(); rot[29, 255, 3] = 14
    assert oc.host_extract(lib, img, rotated=rot)[0] == _lib.RWH_E_INVALID
    table, rot = oc.tables(32)
    out = np.zeros(64, dtype=np.int32)
    call = lambda nbytes: lib.rwh_host_orb_extract(img.ctypes.data, 40, 48, 3, 20, 0, table.ctypes.data, rot.ctypes.data, nbytes, null, null,
                                                   null, null, out.ctypes.data, null)
    assert call(65) == _lib.RWH_E_UNSUPPORTED and call(0) == _lib.RWH_E_UNSUPPORTED
    assert call(32) == 0 and out[0] == 0                     # n_features = 0: nothing written, no arrays needed
    st, none = oc.host_extract(lib, img, n_features=0)
    assert st == 0 and none["found"] == oc.restate(img)["found"] and len(none["score"]) == 0
    assert lib.rwh_host_orb_extract(null, 40, 48, 3, 20, 0, table.ctypes.data, rot.ctypes.data, 32, null, null, null, null, out.ctypes.data, null) == -1


def test_pattern_check_and_bin_table():
    """The table helpers and the pattern check of extract_batch need no device."""
    import ransac as rs
    from ransac_with_homography_amd import features as impl
    with pytest.raises(ValueError):
        impl._check_pattern(rs.default_pattern(4), 32)       # 32 tests for 32 bytes
    with pytest.raises(ValueError):
        impl._check_pattern(np.zeros((8, 4), dtype=np.float32), 1)
    assert impl._check_pattern(oc.caller_pattern(4), 4).shape == (32, 4)
    t = rs.orb_bin_table()
    assert t.dtype == np.int32 and t.shape == (30, 2) and (np.abs((t.astype(float) ** 2).sum(axis=1) - 2.0 ** 30) < 2.0 ** 17).all()
