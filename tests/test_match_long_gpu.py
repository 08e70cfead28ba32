"""The two Hamming matchers on the MI355X where production runs them and the sibling files (test_match_gpu.py,
test_match_ratio_gpu.py) do not: pair lists whose block list is longer than the grid, so that a block walks through several items
with one LDS buffer and one set of registers; more than 256 pairs, so that the setup kernels' scans carry between runs and the
binary searches walk long tables with runs of equal entries; every template instance (1, 2, 4, 8, 16 dwords) at its shortest and
longest length and at one that is no multiple of 4, aligned and not; the largest distance, 8 * 64 = 512; the three safety
statements in the argument list of rwh_match_ratio_graph (include/rwh.h) in guarded buffers; and the Python layer on the
pipeline's largest graph, 64 images and 2016 pairs.  The fixtures are tests/match_long_cases.py's; everything is an integer and
every comparison is exact equality against the numpy restatements of match_cases.py and match_ratio_cases.py."""
import ctypes

import numpy as np
import pytest

import match_cases as mc
import match_long_cases as lc
import match_ratio_cases as rc
import orb_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    return oc.gpu_torch()


@pytest.fixture(scope="module")
def pool(gpu):
    """The pool at 32 bytes: its images (once on the device, as the ratio matcher reads them), their sizes and the restatements of
    all 144 ordered pairs under both rules."""
    images, ratio, cross = lc.restated(32)
    return dict(images=images, sizes=[im.shape[0] for im in images], ratio=ratio, cross=cross,
                desc=gpu.from_numpy(np.concatenate(images)).cuda(), off=lc.offsets([im.shape[0] for im in images]))


def _ratio(pool, pairs):
    from ransac_with_homography_amd import kernels
    got = kernels.match_ratio_graph(pool["desc"], pool["off"], np.array(pairs, dtype=np.int32).reshape(-1, 2), (7, 10))
    return [t.cpu().numpy() for t in got]


def _cross(torch, probs):
    """kernels.match_hamming_batched on problems (A, B): the descriptors concatenated per side, as match_batch does."""
    from ransac_with_homography_amd import kernels
    da = torch.from_numpy(np.concatenate([A for A, _ in probs])).cuda()
    db = torch.from_numpy(np.concatenate([B for _, B in probs])).cuda()
    oa = torch.from_numpy(lc.offsets([A.shape[0] for A, _ in probs])).cuda()
    ob = torch.from_numpy(lc.offsets([B.shape[0] for _, B in probs])).cuda()
    return [t.cpu().numpy() for t in kernels.match_hamming_batched(da, db, oa, ob)]


def _assert_list(got, want, pairs, rows):
    assert all(g.dtype == np.int32 and g.shape == (rows[-1],) for g in got)
    wrong = lc.first_wrong_pair(got, want, pairs, rows)
    assert wrong is None, "pair %d = %s of %d: got %s, the restatement has %s" % (wrong[0], wrong[1], len(pairs), wrong[2], wrong[3])


@pytest.mark.parametrize("P", lc.LONG_P)
def test_long_list_ratio(pool, P):
    """match2_setup_kernel's scans over runs of ceil(P / 256) pairs, match2_owner on the long tables, and from P = 2016 on the
    walk of match2_query_kernel: at 2016 some blocks of the grid take a second item, at 4500 every block takes a third."""
    from ransac_with_homography_amd import kernels
    pairs = lc.long_list(P)
    blocks = lc.blocks_ratio(pool["sizes"], pairs)
    assert (blocks > kernels.MATCH2_GRID_MAX) == (P >= 2016) and (blocks >= 3 * kernels.MATCH2_GRID_MAX) == (P == 4500)
    rows = lc.offsets([pool["sizes"][s] for s, _ in pairs])
    got = _ratio(pool, pairs)
    _assert_list(got, pool["ratio"], pairs, rows)
    assert sum(int((pool["ratio"][pr][0] >= 0).sum()) for pr in pairs) > P            # there were matches to get right
    if P == 4500:
        again = _ratio(pool, pairs)
        assert all(np.array_equal(a, g) for a, g in zip(again, got))                 # a second call is bit-identical
        alone = _ratio(pool, pairs[:300])                                            # ... and the head of the list alone == in the list
        assert all(a.shape == (rows[300],) and np.array_equal(a, g[:rows[300]]) for a, g in zip(alone, got))


@pytest.mark.parametrize("P", lc.LONG_P)
def test_long_list_cross_check(gpu, pool, P):
    """The same lists as problems of the cross-check matcher: match_setup_kernel's scan, match_train_kernel's walk and its search
    in the block prefix, match_cross_kernel's search in an offsets table with runs of equal entries (problems without train rows)."""
    from ransac_with_homography_amd import kernels
    pairs = lc.long_list(P)
    blocks = lc.blocks_cross(pool["sizes"], pairs)
    assert (blocks > kernels.MATCH_GRID_MAX) == (P >= 2016) and (blocks >= 3 * kernels.MATCH_GRID_MAX) == (P == 4500)
    images = pool["images"]
    probs = [(images[s], images[d]) for s, d in pairs]
    rows = lc.offsets([A.shape[0] for A, _ in probs])
    got = _cross(gpu, probs)
    _assert_list(got, pool["cross"], pairs, rows)
    assert sum(int((pool["cross"][pr][0] >= 0).sum()) for pr in pairs) > P
    if P == 4500:
        again = _cross(gpu, probs)
        assert all(np.array_equal(a, g) for a, g in zip(again, got))
        alone = _cross(gpu, probs[:300])
        assert all(a.shape == (rows[300],) and np.array_equal(a, g[:rows[300]]) for a, g in zip(alone, got))


def _odd_start(torch, rows):
    """`rows` [n, nbytes] (nbytes odd) as buf[1:] of a device buffer with one spare leading row: the array starts at an odd address,
    and every row lies at another address modulo 4 than in a buffer of its own."""
    buf = torch.zeros((rows.shape[0] + 1, rows.shape[1]), dtype=torch.uint8, device="cuda")
    buf[1:] = torch.from_numpy(rows).cuda()
    view = buf[1:]
    assert view.is_contiguous() and view.data_ptr() % 2 == 1
    return view


@pytest.mark.parametrize("nbytes", lc.WIDTHS)
def test_every_width_both_matchers(gpu, nbytes):
    """match2_query_kernel<NW> and match_train_kernel<NW> for NW = 1 (2 .. 4 bytes), 2 (5 .. 8), 4 (9 .. 16), 8 (17 .. 32) and 16
    (33 .. 64), and desc_dword's tail branch at 2, 3, 5, 7, 9, 13, 17, 31, 33 and 63 bytes, on a block-crossing pair and three small
    ones; at the odd lengths once more from an array that starts at an odd address."""
    from ransac_with_homography_amd import kernels
    torch = gpu
    ratio_probs, cross_probs = lc.width_problems(nbytes)
    assert [(A.shape, B.shape) for A, B in ratio_probs] == [(A.shape, B.shape) for A, B in cross_probs] == \
        [((2 * 256 + 69, nbytes), (2 * 256 + 37, nbytes)), ((70, nbytes), (65, nbytes)), ((1, nbytes), (70, nbytes)), ((65, nbytes), (2, nbytes))]
    # ratio: eight images, pair p = (2 p, 2 p + 1)
    images = [im for pr in ratio_probs for im in pr]
    pairs = np.array([(2 * p, 2 * p + 1) for p in range(4)], dtype=np.int32)
    off = lc.offsets([im.shape[0] for im in images])
    want = [np.concatenate(c) for c in zip(*[rc.per_query(A, B) for A, B in ratio_probs])]
    host = np.concatenate(images)
    got = [t.cpu().numpy() for t in kernels.match_ratio_graph(torch.from_numpy(host).cuda(), off, pairs, (7, 10))]
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), nbytes
    want_cross = [np.concatenate(c) for c in zip(*[mc.per_query(A, B) for A, B in cross_probs])]
    got_cross = _cross(torch, cross_probs)
    assert all(np.array_equal(g, w) for g, w in zip(got_cross, want_cross)), nbytes
    assert int((want_cross[0] >= 0).sum()) > 4 and int((want[0] >= 0).sum()) > 4       # there were matches to get right
    if nbytes % 2:
        odd = [t.cpu().numpy() for t in kernels.match_ratio_graph(_odd_start(torch, host), off, pairs, (7, 10))]
        assert all(np.array_equal(o, g) for o, g in zip(odd, got)), nbytes
        da = _odd_start(torch, np.concatenate([A for A, _ in cross_probs]))
        db = _odd_start(torch, np.concatenate([B for _, B in cross_probs]))
        oa = torch.from_numpy(lc.offsets([A.shape[0] for A, _ in cross_probs])).cuda()
        ob = torch.from_numpy(lc.offsets([B.shape[0] for _, B in cross_probs])).cuda()
        odd = [t.cpu().numpy() for t in kernels.match_hamming_batched(da, db, oa, ob)]
        assert all(np.array_equal(o, g) for o, g in zip(odd, got_cross)), nbytes


def test_the_largest_distance(gpu):
    """8 * 64 = 512: the top of the packed keys' distance field and the value features._ordered_matches sizes its sort key for
    ("distance <= 512 < 2^10").  The four problems of match_long_cases.extreme_problems: all distances 512; one query at distance 1
    among queries at 512; and the ratio rule's d1 = 1 with d2 = 511 and d1 = 0 with d2 = 512.  (With B all 0xFF the ratio rule can
    give no match, whatever A holds: B's rows are equal, so every query ties.  Problems 2 and 3 give it something to get right.)"""
    from ransac_with_homography_amd import kernels
    from ransac_with_homography_amd import ransac as rs
    torch = gpu
    probs = lc.extreme_problems()
    rows = lc.offsets([A.shape[0] for A, _ in probs])
    want = [mc.per_query(A, B) for A, B in probs]
    got = _cross(torch, probs)
    for p in range(4):
        assert all(np.array_equal(g[rows[p]:rows[p + 1]], w) for g, w in zip(got, want[p])), p
    lists = [[tuple(int(v) for v in m) for m in zip(*mc.ordered(*w))] for w in want]
    assert lists[0] == [(0, 0, 512)] and lists[1] == [(37, 0, 1)] and lists[2] == [(0, 0, 0), (37, 5, 1)]
    assert 512 in got[1].tolist() and 1 in got[1].tolist()
    # ratio: the images once each, the pairs name them
    images = [probs[0][0], probs[0][1], probs[1][0], probs[2][1], probs[3][0]]
    pairs = [(0, 1), (2, 1), (2, 3), (4, 3)]
    assert all(images[s] is probs[p][0] and images[d] is probs[p][1] for p, (s, d) in enumerate(pairs))
    want2 = [rc.per_query(A, B) for A, B in probs]
    got2 = [t.cpu().numpy() for t in kernels.match_ratio_graph(torch.from_numpy(np.concatenate(images)).cuda(),
                                                               lc.offsets([im.shape[0] for im in images]), np.array(pairs, dtype=np.int32))]
    for p in range(4):
        assert all(np.array_equal(g[rows[p]:rows[p + 1]], w) for g, w in zip(got2, want2[p])), p
    assert all((g[:rows[2]] == -1).all() for g in got2)                               # every query ties: no match
    assert [int(g[rows[2] + 37]) for g in got2] == [5, 1, 511] and [int(g[rows[3] + 37]) for g in got2] == [5, 0, 512]
    # the Python layer: the sort on the packed (problem, distance, i) key holds 512
    rng = np.random.RandomState(5)
    kps = [((rng.rand(A.shape[0], 2) * 300).astype(np.float32), (rng.rand(B.shape[0], 2) * 300).astype(np.float32)) for A, B in probs]
    info = {}
    dp = rs.match_batch([(ka, A, kb, B) for (ka, kb), (A, B) in zip(kps, probs)], info=info)
    oracle = [mc.oracle(A, B) for A, B in probs]
    assert dp.sizes == [1, 1, 2, 2]
    for k, name in enumerate(("query_idx", "train_idx", "distance")):
        assert np.array_equal(info[name].cpu().numpy(), np.concatenate([o[k] for o in oracle])), name
    assert info["distance"].cpu().tolist() == [512, 1, 0, 1, 0, 0]
    assert np.array_equal(dp.pts_a.cpu().numpy(), np.concatenate([ka[o[0]] for (ka, _), o in zip(kps, oracle)]))
    assert np.array_equal(dp.pts_b.cpu().numpy(), np.concatenate([kb[o[1]] for (_, kb), o in zip(kps, oracle)]))
    info2 = {}
    feats = [(kps[0][0], images[0]), (kps[0][1], images[1]), (kps[1][0], images[2]), (kps[2][1], images[3]), (kps[3][0], images[4])]
    dp2 = rs.match_graph(feats, pairs, ratio=(7, 10), info=info2)
    oracle2 = [rc.oracle(A, B) for A, B in probs]
    assert dp2.sizes == [0, 0, 1, 1]
    for k, name in enumerate(("query_idx", "train_idx", "distance", "second")):
        assert np.array_equal(info2[name].cpu().numpy(), np.concatenate([o[k] for o in oracle2])), name
    assert info2["second"].cpu().tolist() == [511, 512]


CANARY, GUARD_BYTES, SPARE_ROWS = 0xA5, 4096, 64


def _guarded_ratio_call(torch, images, pairs, total_query, total_train, ws_bytes, rows_held):
    """The raw rwh_match_ratio_graph with the workspace as a slice of a larger buffer of 0xA5, GUARD_BYTES of it in front and
    behind, and each output as a slice of a larger int32 tensor of -7 with SPARE_ROWS rows in front and `rows_held - total_query`
    + SPARE_ROWS behind: a write outside what the call was given lands in the test's own memory and is seen.  Returns (status,
    the three outputs from their first row to the end of the spare rows, workspace guards intact, rows in front intact)."""
    from ransac_with_homography_amd import _lib
    lib = _lib.load()
    assert ws_bytes % 8 == 0 and GUARD_BYTES % 8 == 0
    desc = torch.from_numpy(np.concatenate(images)).cuda()
    off = torch.from_numpy(lc.offsets([im.shape[0] for im in images])).cuda()
    pr = torch.from_numpy(np.array(pairs, dtype=np.int32)).cuda()
    arena = torch.full((ws_bytes + 2 * GUARD_BYTES,), CANARY, dtype=torch.uint8, device="cuda")
    ws = arena[GUARD_BYTES:GUARD_BYTES + ws_bytes]
    assert ws.data_ptr() % 8 == 0
    outs = [torch.full((rows_held + 2 * SPARE_ROWS,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lib.rwh_match_ratio_graph(ptr(desc), images[0].shape[1], ptr(off), len(images), desc.shape[0], ptr(pr), len(pairs), total_query,
                                   total_train, 7, 10, ptr(outs[0][SPARE_ROWS:]), ptr(outs[1][SPARE_ROWS:]), ptr(outs[2][SPARE_ROWS:]),
                                   ptr(ws), ws_bytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    guards = bool((arena[:GUARD_BYTES] == CANARY).all()) and bool((arena[GUARD_BYTES + ws_bytes:] == CANARY).all())
    front = all(bool((o[:SPARE_ROWS] == -7).all()) for o in outs)
    return st, [o[SPARE_ROWS:].cpu().numpy() for o in outs], guards, front


def _modelled(images, pairs, live):
    """Per output the pairs' slices: the restatement for a live pair, -1 for every row of one that is not."""
    per = [rc.per_query(images[s], images[d]) if ok else [np.full(images[s].shape[0], -1, dtype=np.int32)] * 3 for (s, d), ok in zip(pairs, live)]
    return [np.concatenate(c) for c in zip(*per)]


def _safety_images():
    """70, 65 and 600 rows of 32 bytes; every row of the first has a partner at distance 1 in the last, so that a pair against it
    has matches to lose."""
    A, B = mc.random_pair(70, 65, 32, seed=9)
    rng = np.random.RandomState(19)
    C = rng.randint(0, 256, (600, 32)).astype(np.uint8)
    for i in range(70):
        C[300 + i] = mc.flip(A[i], [int(rng.randint(256))])
    return [A, B, C]


def test_starved_workspace_costs_matches_never_a_write_outside(gpu):
    """include/rwh.h: "a pair whose partial results would not fit into the workspace given has no matches -- never a write outside
    it", and none behind it either.  The smallest workspace the call accepts holds total_query = 205 partials; pair 1 (70 x 600,
    three segments) needs 70 + 210 with pair 0's, so pairs 1 and 2 have no matches although pair 2 would fit by itself."""
    from ransac_with_homography_amd import _lib
    lib = _lib.load()
    images, pairs = _safety_images(), [(0, 1), (0, 2), (1, 0)]
    na, nb = [70, 70, 65], [65, 600, 70]
    total_query, total_train = sum(na), sum(nb)
    small = lib.rwh_match_ratio_workspace_bytes(3, total_query, total_train, 0)
    assert lc.partial_capacity(lib, 3, total_train, small) == 205
    live = lc.live_prefix(na, nb, total_query, total_train, 205)
    assert live == [True, False, False]
    st, got, guards, front = _guarded_ratio_call(gpu, images, pairs, total_query, total_train, small, total_query)
    assert st == 0 and guards and front
    want = _modelled(images, pairs, live)
    assert all(np.array_equal(g[:total_query], w) for g, w in zip(got, want))
    assert all((g[70:total_query] == -1).all() and (g[total_query:] == -7).all() for g in got) and (got[0][:70] >= 0).any()
    # one entry less is refused before the device is touched
    assert _guarded_ratio_call(gpu, images, pairs, total_query, total_train, small - 8, total_query)[0] == _lib.RWH_E_INVALID
    # sized for the longest train side, the same call gives the restatement for all three pairs
    full = lib.rwh_match_ratio_workspace_bytes(3, total_query, total_train, 600)
    assert lc.live_prefix(na, nb, total_query, total_train, lc.partial_capacity(lib, 3, total_train, full)) == [True, True, True]
    st, got, guards, front = _guarded_ratio_call(gpu, images, pairs, total_query, total_train, full, total_query)
    assert st == 0 and guards and front
    want = _modelled(images, pairs, [True, True, True])
    assert all(np.array_equal(g[:total_query], w) and (g[total_query:] == -7).all() for g, w in zip(got, want))
    assert int((want[0][70:140] >= 0).sum()) > 35 and (want[0][140:] >= 0).any()     # what the starved call lost


def test_understated_totals_cost_matches_never_a_write_outside(gpu):
    """include/rwh.h: "Rows at or beyond total_query are never written; a pair whose rows would pass total_query or total_train
    (totals smaller than the tables say) has no matches"."""
    from ransac_with_homography_amd import _lib
    lib = _lib.load()
    images, pairs = _safety_images()[:2], [(0, 1), (1, 0), (0, 1)]
    na, nb = [70, 65, 70], [65, 70, 65]
    true_query, true_train = sum(na), sum(nb)
    ws_bytes = lib.rwh_match_ratio_workspace_bytes(3, true_query, true_train, 70)        # no bound but the one under test binds
    # total_query = 145: pairs 0 and 1 own rows 0 .. 134, pair 2 would end at 205
    live = lc.live_prefix(na, nb, 145, true_train, lc.partial_capacity(lib, 3, true_train, ws_bytes))
    assert live == [True, True, False]
    st, got, guards, front = _guarded_ratio_call(gpu, images, pairs, 145, true_train, ws_bytes, true_query)
    assert st == 0 and guards and front
    want = _modelled(images, pairs, live)
    for g, w in zip(got, want):
        assert np.array_equal(g[:135], w[:135]) and (g[135:145] == -1).all() and (g[145:] == -7).all() and g.shape == (true_query + SPARE_ROWS,)
    assert (got[0][:70] >= 0).any() and (got[0][70:135] >= 0).any()
    # total_train one row short of what the tables say: pair 2's owner slots would end at 200
    short = 65 + 70 + 64
    live = lc.live_prefix(na, nb, true_query, short, lc.partial_capacity(lib, 3, short, ws_bytes))
    assert live == [True, True, False]
    st, got, guards, front = _guarded_ratio_call(gpu, images, pairs, true_query, short, ws_bytes, true_query)
    assert st == 0 and guards and front
    for g, w in zip(got, want):
        assert np.array_equal(g[:135], w[:135]) and (g[135:true_query] == -1).all() and (g[true_query:] == -7).all()
    # with the true totals pair 2 is pair 0 again
    st, got, guards, front = _guarded_ratio_call(gpu, images, pairs, true_query, true_train, ws_bytes, true_query)
    assert st == 0 and guards and front
    want = _modelled(images, pairs, [True, True, True])
    assert all(np.array_equal(g[:true_query], w) and np.array_equal(g[135:true_query], g[:70]) and (g[true_query:] == -7).all()
               for g, w in zip(got, want))


def test_python_layer_on_the_largest_graph(gpu):
    """ransac.match_graph on the 2016 pairs (i, j), i > j, of 64 images -- stitch_sequence(pairs="all") at RWH_SEQ_MAX_IMAGES --
    and ransac.match_batch on the first 300 of them as explicit problems: sizes, the ordered index lists, the distances and the
    gathered keypoints are the restatements'."""
    from ransac_with_homography_amd import ransac as rs
    torch = gpu
    feats = lc.sequence_features()
    assert len(feats) == 64 and all(24 <= d.shape[0] <= 60 and d.shape[1] == 32 and k.shape == (d.shape[0], 2) for k, d in feats)
    pairs = [(i, j) for i in range(64) for j in range(i)]
    assert len(pairs) == 2016
    want = [rc.oracle(feats[s][1], feats[d][1]) for s, d in pairs]
    adjacent = [len(w[0]) for (s, d), w in zip(pairs, want) if s == d + 1]
    assert min(adjacent) >= 8 and any(len(w[0]) == 0 for w in want)
    info = {}
    dp = rs.match_graph(feats, pairs, ratio=0.7, info=info)
    assert isinstance(dp, rs.DeviceProblems) and dp.sizes == [len(w[0]) for w in want]
    for k, name in enumerate(("query_idx", "train_idx", "distance", "second")):
        assert info[name].is_cuda and info[name].dtype == torch.int32
        assert np.array_equal(info[name].cpu().numpy(), np.concatenate([w[k] for w in want])), name
    assert np.array_equal(dp.pts_a.cpu().numpy(), np.concatenate([feats[s][0][w[0]] for (s, d), w in zip(pairs, want)]))
    assert np.array_equal(dp.pts_b.cpu().numpy(), np.concatenate([feats[d][0][w[1]] for (s, d), w in zip(pairs, want)]))
    # match_batch: the first 300 pairs as explicit (kpsA, descA, kpsB, descB)
    head = pairs[:300]
    cross = [mc.oracle(feats[s][1], feats[d][1]) for s, d in head]
    info = {}
    dp = rs.match_batch([(feats[s][0], feats[s][1], feats[d][0], feats[d][1]) for s, d in head], info=info)
    assert isinstance(dp, rs.DeviceProblems) and dp.sizes == [len(w[0]) for w in cross] and min(dp.sizes) > 0
    for k, name in enumerate(("query_idx", "train_idx", "distance")):
        assert info[name].is_cuda and info[name].dtype == torch.int32
        assert np.array_equal(info[name].cpu().numpy(), np.concatenate([w[k] for w in cross])), name
    assert np.array_equal(dp.pts_a.cpu().numpy(), np.concatenate([feats[s][0][w[0]] for (s, d), w in zip(head, cross)]))
    assert np.array_equal(dp.pts_b.cpu().numpy(), np.concatenate([feats[d][0][w[1]] for (s, d), w in zip(head, cross)]))
