"""The ratio matcher on the MI355X: kernels.match_ratio_graph (rwh_match_ratio_graph) against the numpy restatement of
tests/match_ratio_cases.py and the host twin -- exact equality, everything is an integer -- on one pair graph per descriptor length
whose images cross every edge of the block shape; determinism; alone == in the batch; pairs that name no image; match_graph
feeding run_batch; stitch_sequence(features={"ratio": ...}) on the three crops."""
import ctypes

import numpy as np
import pytest

import match_cases as mc
import match_ratio_cases as rc
import orb_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return oc.gpu_torch()


def _tables(images):
    off = np.zeros(len(images) + 1, dtype=np.int32)
    off[1:] = np.cumsum([im.shape[0] for im in images])
    return off


def _call(torch, images, pairs, ratio=(7, 10)):
    from ransac_with_homography_amd import kernels
    desc = torch.from_numpy(np.concatenate(images)).cuda()
    return [t.cpu().numpy() for t in kernels.match_ratio_graph(desc, _tables(images), np.array(pairs, dtype=np.int32), ratio)]


@pytest.fixture(scope="module", params=[32, 61, 1])
def batch(gpu, request):
    """The graph of one descriptor length, the restatement of every distinct pair (computed once) and the first call's results."""
    from ransac_with_homography_amd import kernels
    nbytes = request.param
    images, pairs, planted = rc.graph(nbytes, kernels.MATCH2_TILE_QUERY, kernels.MATCH2_CHUNK_TRAIN, kernels.MATCH2_SEG_TRAIN)
    want = {pr: rc.per_query(images[pr[0]], images[pr[1]]) for pr in set(pairs)}
    rows = np.zeros(len(pairs) + 1, dtype=np.int64)
    rows[1:] = np.cumsum([images[s].shape[0] for s, _ in pairs])
    return dict(nbytes=nbytes, images=images, pairs=pairs, planted=planted, want=want, rows=rows, first=_call(gpu, images, pairs))


def test_graph_covers_the_block_shape(batch):
    from ransac_with_homography_amd import kernels
    T, C, S = kernels.MATCH2_TILE_QUERY, kernels.MATCH2_CHUNK_TRAIN, kernels.MATCH2_SEG_TRAIN
    sizes = [im.shape[0] for im in batch["images"]]
    assert sizes[:7] == [0, 1, 2, 63, 65, 70, 257] and sizes[7] == 2 * max(T, S) + C + 5 and sizes[8] not in sizes[:8] and sizes[8] > 2 * max(T, S)
    pairs = batch["pairs"]
    assert (7, 8) in pairs and (8, 7) in pairs and pairs.count((7, 8)) == 2 and (7, 7) in pairs
    assert all(pr in pairs for pr in ((0, 8), (8, 0), (1, 8), (8, 1)))


def test_batch_equals_restatement_and_host_twin(batch):
    from ransac_with_homography_amd import _lib
    lib = _lib.load()
    rows, images = batch["rows"], batch["images"]
    assert all(o.dtype == np.int32 and o.shape == (rows[-1],) for o in batch["first"])
    twins = {}
    for p, (s, d) in enumerate(batch["pairs"]):
        got = [o[rows[p]:rows[p + 1]] for o in batch["first"]]
        assert all(np.array_equal(g, w) for g, w in zip(got, batch["want"][(s, d)])), (p, s, d)
        if (s, d) not in twins:
            twins[(s, d)] = rc.host_match(lib, images[s], images[d])
        assert twins[(s, d)][0] == 0 and all(np.array_equal(g, w) for g, w in zip(got, twins[(s, d)][1:])), (p, s, d)
    matched = sum(int((w[0] >= 0).sum()) for w in batch["want"].values())
    assert matched > (len(batch["pairs"]) if batch["nbytes"] > 1 else 0)                # there were matches to get right
    # what was planted in the pair (7, 8) is what the restatement -- and so the device -- gives
    train = batch["want"][(7, 8)][0]
    assert batch["planted"] or batch["nbytes"] == 1
    for i, j in batch["planted"].items():
        assert train[i] == j, (i, j, train[i])


def test_second_call_is_bit_identical(gpu, batch):
    again = _call(gpu, batch["images"], batch["pairs"])
    assert all(np.array_equal(a, b) for a, b in zip(again, batch["first"]))


def test_alone_equals_in_the_batch(gpu, batch):
    rows = batch["rows"]
    alone = {}
    for p, pr in enumerate(batch["pairs"]):
        if pr not in alone:
            alone[pr] = _call(gpu, batch["images"], [pr])
        assert all(np.array_equal(a, o[rows[p]:rows[p + 1]]) for a, o in zip(alone[pr], batch["first"])), (p, pr)


def test_other_ratios(gpu, batch):
    images = batch["images"]
    pairs = [(7, 8), (6, 5), (8, 7)]
    for ratio in ((1, 1), (1, 1024), (4, 5)):
        got = _call(gpu, images, pairs, ratio)
        want = [np.concatenate(c) for c in zip(*[rc.per_query(images[s], images[d], *ratio) for s, d in pairs])]
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), ratio


def test_pairs_that_name_no_rows_and_canaries(gpu):
    """The raw call on device pointers: a pair naming image N, one naming image -1 and images whose offsets leave [0, total_rows]
    have no matches, the legal pairs between them are unharmed, and the rows behind total_query are not written."""
    torch = gpu
    from ransac_with_homography_amd import _lib
    lib = _lib.load()
    A, B = mc.random_pair(70, 65, 32, seed=9)
    desc = torch.from_numpy(np.concatenate([A, B])).cuda()
    # images 0 and 1 are A and B; image 2 ends behind total_rows, image 3 starts before 0 (its successor's range is broken with it)
    off = np.array([0, 70, 135, 200, -5, 60], dtype=np.int32)
    n_images, total_rows = 5, 135
    pairs = np.array([(0, 1), (0, 5), (5, 0), (-1, 1), (0, -1), (0, 2), (2, 0), (0, 3), (4, 1), (1, 0)], dtype=np.int32)
    na = [70, 70, 0, 0, 70, 70, 0, 70, 0, 65]
    nb = [65, 0, 70, 65, 0, 0, 70, 0, 65, 70]
    total_query, total_train = sum(na), sum(nb)
    spare = 64
    outs = [torch.full((total_query + spare,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    ws_bytes = lib.rwh_match_ratio_workspace_bytes(len(pairs), total_query, total_train, max(nb))
    ws = torch.zeros((ws_bytes // 8,), dtype=torch.int64, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    off_dev, pairs_dev = torch.from_numpy(off).cuda(), torch.from_numpy(pairs).cuda()
    st = lib.rwh_match_ratio_graph(ptr(desc), 32, ptr(off_dev), n_images, total_rows, ptr(pairs_dev), len(pairs), total_query, total_train,
                                   7, 10, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(ws), ws_bytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert st == 0
    got = [o.cpu().numpy() for o in outs]
    assert all((g[total_query:] == -7).all() for g in got)                              # the canaries
    rows = np.concatenate([[0], np.cumsum(na)])
    for p in range(len(pairs)):
        part = [g[rows[p]:rows[p + 1]] for g in got]
        want = rc.per_query(A, B) if p == 0 else rc.per_query(B, A) if p == 9 else [np.full(na[p], -1, dtype=np.int32)] * 3
        assert all(np.array_equal(g, w) for g, w in zip(part, want)), p
    assert (got[0][:70] >= 0).any() and (got[0][rows[9]:rows[10]] >= 0).any()


def test_unsupported_length_and_bad_tables_raise(gpu):
    from ransac_with_homography_amd import kernels
    off, pairs = np.array([0, 4], dtype=np.int32), np.array([[0, 0]], dtype=np.int32)
    for nbytes in (0, 65):
        with pytest.raises(NotImplementedError):
            kernels.match_ratio_graph(gpu.zeros((4, nbytes), dtype=gpu.uint8, device="cuda"), off, pairs)
    d = gpu.zeros((4, 32), dtype=gpu.uint8, device="cuda")
    for bad in ((d.cpu(), off, pairs), (d.to(gpu.int32), off, pairs), (d, off.astype(np.int64), pairs), (d, off, pairs.reshape(-1)),
                (d, off[:1], pairs)):
        with pytest.raises(ValueError):
            kernels.match_ratio_graph(*bad)
    for ratio in ((0, 1), (2, 1), (1, 1025), (0.7, 1), 0.7):
        with pytest.raises(ValueError):
            kernels.match_ratio_graph(d, off, pairs, ratio)
    # tables on the device are taken as well
    got = kernels.match_ratio_graph(d, gpu.from_numpy(off).cuda(), gpu.from_numpy(pairs).cuda())
    assert all(g.is_cuda and g.dtype == gpu.int32 and g.cpu().tolist() == [-1] * 4 for g in got)


def _same_results(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g[0] is None) == (w[0] is None) and (g[0] is None or np.array_equal(g[0], w[0]))
        assert np.array_equal(g[1][0], w[1][0]) and int(g[2]) == int(w[2])


def test_match_graph_feeds_run_batch(gpu, matches):
    from ransac_with_homography_amd import ransac as rs
    torch = gpu
    kps_a, desc_a, kps_b, desc_b, truth = rc.planted_features(matches)
    # image 2: three of A's rows, image 3: no rows; tensors and numpy arrays mixed
    feats = [(kps_a, desc_a), (torch.from_numpy(kps_b).cuda(), torch.from_numpy(desc_b)), (kps_a[:3] + np.float32(10), desc_a[:3][::-1].copy()),
             (kps_a[:0], desc_a[:0])]
    host = [(kps_a, desc_a), (kps_b, desc_b), (kps_a[:3] + np.float32(10), desc_a[:3][::-1].copy()), (kps_a[:0], desc_a[:0])]
    pairs = [(0, 1), (2, 0), (0, 3), (3, 0), (1, 0), (0, 1), (0, 0)]
    want = [rc.oracle(host[s][1], host[d][1]) for s, d in pairs]
    # on the CPU: the planted pairs; three exact copies; an image against itself matches every row with itself
    assert set(zip(want[0][0].tolist(), want[0][1].tolist())) == truth and len(want[1][0]) == 3
    assert np.array_equal(want[6][0], want[6][1]) and len(want[6][0]) == 300
    before = {}
    cross = rs.match_batch([(kps_a, desc_a, kps_b, desc_b)], info=before)
    info = {}
    dp = rs.match_graph(feats, pairs, ratio=0.7, info=info)
    assert isinstance(dp, rs.DeviceProblems) and dp.sizes == [len(w[0]) for w in want] == [185, 3, 0, 0, len(want[4][0]), 185, 300]
    assert dp.pts_a.is_cuda and dp.pts_a.dtype == torch.float32 and dp.pts_b.is_cuda
    arrays = [[host[s][0][w[0]].T.copy(), host[d][0][w[1]].T.copy()] for (s, d), w in zip(pairs, want)]
    assert np.array_equal(dp.pts_a.cpu().numpy(), np.concatenate([X.T for X, _ in arrays]))
    assert np.array_equal(dp.pts_b.cpu().numpy(), np.concatenate([Y.T for _, Y in arrays]))
    for k, name in enumerate(("query_idx", "train_idx", "distance", "second")):
        assert info[name].is_cuda and info[name].dtype == torch.int32
        assert np.array_equal(info[name].cpu().numpy(), np.concatenate([w[k] for w in want])), name
    assert rs.match_graph(feats, pairs, ratio=(7, 10)).sizes == dp.sizes
    for got, w in zip(rs.match_descriptors_ratio(desc_a, torch.from_numpy(desc_b).cuda()), want[0]):
        assert got.dtype == np.int32 and np.array_equal(got, w)
    # run_batch takes the hand-over as it takes the same correspondences from the host
    kw = dict(seed=3, k=256, d=70, th=5, method="fwd")
    got = rs.run_batch(dp, refit=True, **kw)
    _same_results(got, rs.run_batch(arrays, refit=True, **kw))
    assert got[0][0] is not None and int(got[0][2]) > 100 and got[2][0] is None and int(got[2][2]) == 0
    # match_batch on the same features still returns what it returned
    qi, ti, dd = mc.oracle(desc_a, desc_b)
    after = {}
    again = rs.match_batch([(kps_a, desc_a, kps_b, desc_b)], info=after)
    assert again.sizes == cross.sizes == [len(qi)] and len(qi) > 185
    assert np.array_equal(again.pts_a.cpu().numpy(), kps_a[qi]) and np.array_equal(again.pts_b.cpu().numpy(), kps_b[ti])
    for k, name in enumerate(("query_idx", "train_idx", "distance")):
        assert np.array_equal(after[name].cpu().numpy(), (qi, ti, dd)[k]) and np.array_equal(before[name].cpu().numpy(), (qi, ti, dd)[k])


def test_pipeline_on_three_crops(gpu):
    """stitch_sequence with the ratio key: the matcher's counts are the restatement's on extract_batch's own features, all three
    pairs of the graph are accepted -- the 80-pixel overlap (2, 0) included, which cross-check's ballast costs -- and the canvas is
    the compositor's on the reported Gs.  Without the key the call is the one it was."""
    import homography as hg
    from ransac_with_homography_amd import ransac as rs
    crops = rc.crops()
    feats = [(k.cpu().numpy(), d.cpu().numpy()) for k, d in rs.extract_batch(crops)]
    counts = rc.crop_counts(feats)
    for pair in rc.CROP_PAIRS:
        print("crops %s: cross-check %d matches / %d true, ratio 7/10 %d / %d" % ((pair,) + counts[pair]["cross"] + counts[pair]["ratio"]))
    info = {}
    can = rs.stitch_sequence(crops, th=5, pairs="all", features={"ratio": 0.7}, info=info)
    assert info["pairs"] == list(rc.CROP_PAIRS)
    assert info["sizes"] == [counts[pr]["ratio"][0] for pr in rc.CROP_PAIRS]
    print("ratio 7/10: sizes %s inliers %s accepted %s" % (info["sizes"], info["inliers"], list(info["accepted"])))
    assert all(info["accepted"])
    assert isinstance(can, np.ndarray) and np.array_equal(can, hg.stitchSequence(crops, Gs=info["Gs"]))
    # the adjacent path takes the key too
    chain = {}
    rs.stitch_sequence(crops, th=5, features={"ratio": (7, 10)}, info=chain)
    assert chain["sizes"] == [counts[(1, 0)]["ratio"][0], counts[(2, 1)]["ratio"][0]] and chain["Hs"].shape == (2, 3, 3)
    # the defaults: the same call with and without a features dict that has no ratio, and cross-check's counts
    base, same = {}, {}
    want = rs.stitch_sequence(crops, th=5, info=base)
    assert np.array_equal(want, rs.stitch_sequence(crops, th=5, features={}, info=same))
    assert base["sizes"] == same["sizes"] == [counts[(1, 0)]["cross"][0], counts[(2, 1)]["cross"][0]]
    assert np.array_equal(base["Hs"], same["Hs"]) and np.array_equal(base["Gs"], same["Gs"])
    graph = {}
    rs.stitch_sequence(crops, th=5, pairs="all", info=graph)
    assert graph["sizes"] == [counts[pr]["cross"][0] for pr in rc.CROP_PAIRS]
