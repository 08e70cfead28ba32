"""The extractor on the MI355X: features.extract_batch (rwh_orb_detect_batched -> one sort -> rwh_orb_describe_batched) against the host
twin and the numpy restatement of tests/orb_cases.py -- exact equality, everything is an integer -- on one batch that holds every
image of the CPU suite plus one that spans several tiles with corners planted on the seams; the parameter variants; the overflow
status; determinism; alone == in the batch; tensors in == numpy in; descriptors independent of n_features; displaced crops through
match_batch; the real pair through match_batch and run_batch; stitching(features="extract")."""
import numpy as np
import pytest

import match_cases as mc
import orb_cases as oc

pytestmark = pytest.mark.gpu
KEY_NONE = 0x7F7F7F7F7F7F7F7F


@pytest.fixture(scope="module")
def gpu():
    return oc.gpu_torch()


def _seams_image():
    """55 x 150 gray, noise of 0 .. 10 under planted dots.  The detector's tiles are TILE_W x TILE_H = 64 x 16: the legal centres
    16 .. 133 x 16 .. 38 span three tile columns and two tile rows, neither side a multiple of the tile.  Pairs of neighbouring dots
    of different value sit across a vertical seam, a horizontal seam and a tile corner (the weaker one is suppressed through the
    halo), lone dots sit on seams, and a row of dots four pixels apart gives a wave many survivors to append at once."""
    from ransac_with_homography_amd import kernels
    tw, th = kernels.ORB_TILE_W, kernels.ORB_TILE_H
    assert (tw, th) == (64, 16)
    img = np.random.RandomState(8).randint(0, 11, (55, 150)).astype(np.uint8)
    strong = [(2 * tw, 20), (70, 2 * th - 1), (tw - 1, 2 * th - 1), (tw, 36), (2 * tw - 1, 37)] + [(16 + 4 * i, 24) for i in range(10)] + [(133, 38), (16, 16)]
    weak = [(2 * tw - 1, 20), (70, 2 * th), (tw, 2 * th)]
    for x, y in strong:
        img[y, x] = 250
    for x, y in weak:
        img[y, x] = 200
    return img, strong, weak


@pytest.fixture(scope="module")
def batch(gpu):
    """Every image of the CPU cases and the seams image in one call with the default parameters; restatement computed once."""
    images = [img for _, img, _ in oc.cpu_cases()[:13]] + [_seams_image()[0]]
    return dict(images=images, want=[oc.restate(img) for img in images], first=oc.extract(images))


def test_batch_equals_host_twin_and_restatement(batch):
    from ransac_with_homography_amd import _lib
    lib = _lib.load()
    shapes = set()
    for i, (img, want, got) in enumerate(zip(batch["images"], batch["want"], batch["first"])):
        assert oc.same(got, want), (i, img.shape)
        st, host = oc.host_extract(lib, img)
        assert st == 0 and oc.same(got, host), (i, img.shape)
        shapes.add(img.shape)
    assert len(shapes) > 8 and sum(w["found"] for w in batch["want"]) > 400
    _, strong, weak = _seams_image()
    kept = set(map(tuple, batch["want"][-1]["kps"].astype(int).tolist()))
    assert set(strong) <= kept and not set(weak) & kept and batch["want"][-1]["found"] == len(strong)


def test_parameter_variants(gpu):
    from ransac_with_homography_amd import _lib
    lib = _lib.load()
    variants = [(name, img, kw) for name, img, kw in oc.cpu_cases() if kw]
    assert len(variants) == 7
    for name, img, kw in variants:
        got, = oc.extract([img], **kw)
        assert oc.same(got, oc.restate(img, **kw)) and oc.same(got, oc.host_extract(lib, img, **kw)[1]), name


def test_second_call_is_bit_identical(batch):
    again = oc.extract(batch["images"])
    assert all(oc.same(a, b) for a, b in zip(again, batch["first"]))


def test_alone_equals_in_the_batch(batch):
    for i in (0, 3, 4, 12, 13):
        alone, = oc.extract([batch["images"][i]])
        assert oc.same(alone, batch["first"][i]), i


def test_tensors_in_equal_numpy_in(gpu, batch):
    pick = [0, 1, 2, 13]
    got = oc.extract([gpu.from_numpy(batch["images"][i]).cuda() if i % 2 else gpu.from_numpy(batch["images"][i]) for i in pick])
    assert all(oc.same(g, batch["first"][i]) for g, i in zip(got, pick))
    import ransac as rs
    kps, desc = rs.detect_and_describe(batch["images"][12])
    assert isinstance(kps, np.ndarray) and np.array_equal(kps, batch["want"][12]["kps"]) and np.array_equal(desc, batch["want"][12]["desc"])
    for bad in (batch["images"][0].astype(np.float32), batch["images"][0].astype(np.int8)):
        with pytest.raises(TypeError):
            rs.extract_batch([bad])
    with pytest.raises(ValueError):
        rs.extract_batch([batch["images"][0][:, :, :2]])
    with pytest.raises(ValueError):
        rs.extract_batch([batch["images"][0]], threshold=255)
    with pytest.raises(NotImplementedError):
        rs.extract_batch([batch["images"][0]], nbytes=65)


def test_descriptors_do_not_depend_on_n_features(batch):
    crop, full = batch["images"][12], batch["first"][12]
    few, = oc.extract([crop], n_features=40)
    assert full["found"] > 40 and few["found"] == full["found"] and len(few["score"]) == 40
    assert all(np.array_equal(few[k], full[k][:40]) for k in ("kps", "desc", "score", "bin"))


def test_overflow_status_and_nothing_past_the_list(gpu, batch, monkeypatch):
    """Twelve keypoints into a list of four: counts says twelve, four of them are stored, the next image's list and the words
    behind the buffer are untouched; extract_batch meets the same status and repeats the call with room for all."""
    torch = gpu
    from ransac_with_homography_amd import kernels
    from ransac_with_homography_amd import features as impl
    tie, _ = oc.tie_image()
    one = oc.dots(33, 33, [(16, 16, 255)])
    src = torch.from_numpy(np.concatenate([tie.reshape(-1), one.reshape(-1)])).cuda()
    table = torch.tensor([[0, 0, 60, 90, 1], [tie.size, tie.size, 33, 33, 1]], dtype=torch.int64, device="cuda")
    guard = torch.full((2 * 4 + 64,), -12345, dtype=torch.int64, device="cuda")
    gray, keys, counts = kernels.orb_detect_batched(src, table, tie.size + one.size, 20, 4, out_keys=guard[:8].view(2, 4))
    x, y, s = oc.keypoints(oc.scores(tie), 20)
    true_keys = set(((255 - s.astype(np.int64)) << 32 | y.astype(np.int64) << 16 | x).tolist())
    g = guard.cpu().numpy()
    assert counts.cpu().tolist() == [12, 1] and len(true_keys) == 12
    assert len(set(g[:4].tolist())) == 4 and set(g[:4].tolist()) <= true_keys
    assert g[4:8].tolist() == [16 << 16 | 16, KEY_NONE, KEY_NONE, KEY_NONE] and (g[8:] == -12345).all()
    assert np.array_equal(gray.cpu().numpy(), np.concatenate([tie.reshape(-1), one.reshape(-1)]))
    monkeypatch.setattr(impl, "_ORB_DEFAULT_CAPACITY", 4)
    got = oc.extract([tie, batch["images"][12], one])
    assert got[1]["found"] > 4 and oc.same(got[1], batch["first"][12]) and oc.same(got[0], oc.restate(tie)) and got[2]["found"] == 1


def test_displaced_crops_match_at_distance_zero_exactly(gpu):
    """Two 300 x 400 crops of img_foto1 A displaced by (33, 12), nothing cut: every match at distance 0 is exactly the displacement,
    and the matches are the CPU pipeline's (restatement + match_cases.oracle: 790 matches, 787 at distance 0)."""
    import ransac as rs
    A = oc.foto("A")
    c1, c2 = np.ascontiguousarray(A[100:400, 200:600]), np.ascontiguousarray(A[112:412, 233:633])
    info, minfo = {}, {}
    (k1, d1), (k2, d2) = rs.extract_batch([c1, c2], n_features=4096, info=info)
    assert max(info["found"]) < 4096 and info["counts"] == info["found"]
    r1, r2 = oc.restate(c1, n_features=4096), oc.restate(c2, n_features=4096)
    assert np.array_equal(d1.cpu().numpy(), r1["desc"]) and np.array_equal(d2.cpu().numpy(), r2["desc"])
    dp = rs.match_batch([(k1, d1, k2, d2)], info=minfo)
    q, t, d = (minfo[k].cpu().numpy() for k in ("query_idx", "train_idx", "distance"))
    wq, wt, wd = mc.oracle(r1["desc"], r2["desc"])
    assert np.array_equal(q, wq) and np.array_equal(t, wt) and np.array_equal(d, wd)
    zero = d == 0
    assert len(d) == 790 and int(zero.sum()) == 787
    shift = (dp.pts_a.cpu().numpy() - dp.pts_b.cpu().numpy())[zero]
    assert shift.dtype == np.float32 and (shift == np.float32([33, 12])).all()


@pytest.fixture(scope="module")
def real_pair(gpu):
    import ransac as rs
    A, B = oc.foto("A"), oc.foto("B")
    ra, rb = oc.restate(A), oc.restate(B)
    feats = rs.extract_batch([A, B])
    return dict(A=A, B=B, ra=ra, rb=rb, feats=feats, oracle=mc.oracle(ra["desc"], rb["desc"]))


def test_real_pair_through_match_batch_and_run_batch(gpu, real_pair):
    """img_foto1 A / B at threshold 20, n_features = 500: keypoints, descriptors and matches equal the CPU restatement's; run_batch on
    the DeviceProblems equals run_batch on the host lists.  Sanity floor: the winner's inliers are at least 25 % of the matches.
    On the CPU (restatement, match_cases.oracle, the oracle's RANSAC with th = 5, d = 70, k = 1000, 'fwd', numpy seeds 0 .. 3): 285
    matches, 118 or 119 inliers (41 - 42 %), an H that shifts by about 440 px; a broken extractor gives a few percent."""
    import ransac as rs
    ra, rb, ((ka, da), (kb, db)) = real_pair["ra"], real_pair["rb"], real_pair["feats"]
    assert len(ra["score"]) == len(rb["score"]) == 500
    for got_k, got_d, want in ((ka, da, ra), (kb, db, rb)):
        assert np.array_equal(got_k.cpu().numpy(), want["kps"]) and np.array_equal(got_d.cpu().numpy(), want["desc"])
    qi, ti, dist = real_pair["oracle"]
    info = {}
    dp = rs.match_batch([(ka, da, kb, db)], info=info)
    assert dp.sizes == [len(qi)] and len(qi) > 200
    assert np.array_equal(info["query_idx"].cpu().numpy(), qi) and np.array_equal(info["train_idx"].cpu().numpy(), ti)
    assert np.array_equal(info["distance"].cpu().numpy(), dist)
    host = [[ra["kps"][qi].T.copy(), rb["kps"][ti].T.copy()]]
    kw = dict(seed=3, k=1000, d=70, th=5, method="fwd")
    for refit in (True, "device"):
        i_dp, i_host = {}, {}
        got = rs.run_batch(dp, refit=refit, info=i_dp, **kw)
        want = rs.run_batch(host, refit=refit, info=i_host, **kw)
        assert got[0][0] is not None and np.array_equal(got[0][0], want[0][0])
        assert np.array_equal(got[0][1][0], want[0][1][0]) and int(got[0][2]) == int(want[0][2])
        assert int(got[0][2]) >= 0.25 * len(qi), (int(got[0][2]), len(qi))
        if refit == "device":
            assert np.array_equal(i_dp["H_device"].cpu().numpy(), i_host["H_device"].cpu().numpy(), equal_nan=True)


def test_stitching_extracts_on_the_gpu(gpu, real_pair):
    import ransac as rs
    A, B, ra, rb = real_pair["A"], real_pair["B"], real_pair["ra"], real_pair["rb"]
    qi, ti, _ = real_pair["oracle"]
    kw = dict(ransacMet="fwd", th=5, d=70, k=300)
    np.random.seed(4)
    want = rs.stitching(A.copy(), B.copy(), matches=(ra["kps"][qi], rb["kps"][ti]), **kw)
    np.random.seed(4)
    got = rs.stitching(A.copy(), B.copy(), features="extract", **kw)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    np.random.seed(4)
    both = rs.stitching(A.copy(), B.copy(), matches=(ra["kps"][qi], rb["kps"][ti]), features="extract", **kw)
    assert np.array_equal(both, want)
    with pytest.raises(ValueError):
        rs.stitching(A, B, features="orb")
