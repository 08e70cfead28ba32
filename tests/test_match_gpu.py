"""The Hamming matcher on the MI355X: kernels.match_hamming_batched (rwh_match_hamming_batched) against the numpy oracle of
tests/match_cases.py and the host twin -- exact equality, everything is an integer -- on one batch that holds every shape of the
suite, two empty sides and a problem that crosses train tiles, query chunks and query segments; determinism; alone == in the
batch; match_descriptors; match_batch feeding run_batch; stitching(features=)."""
import numpy as np
import pytest

import match_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch


def _big_pair(nbytes):
    """Sized from the exported block shape: more than two train tiles, query segments and query chunks on either side, with
    duplicate rows planted across a chunk boundary, a segment boundary (both in A) and a tile boundary (in B)."""
    from ransac_with_homography_amd import kernels
    T, C, S = kernels.MATCH_TILE_TRAIN, kernels.MATCH_CHUNK_QUERY, kernels.MATCH_SEG_QUERY
    n = 2 * max(T, S)
    A, B = mc.random_pair(n + C + 5, n + 37, nbytes, seed=77)
    A[C] = A[C - 1]                                  # equal queries either side of a chunk boundary: the lower index wins
    B[3] = mc.flip(A[C], [2])
    A[S] = A[S - 1]                                  # ... and of a segment boundary: two blocks' minima tie on the distance
    B[T + 9] = mc.flip(A[S], [5, 6])
    B[T] = B[T - 1] = mc.flip(A[2 * S + 1], [1])     # equal train rows either side of a tile boundary pick the same query
    return A, B


def _problems(nbytes, small_only):
    shapes = [s for s in mc.SHAPES if not small_only or s != (500, 500)] + [(0, 5), (5, 0)]
    probs = [mc.random_pair(max(na, 1), max(nb, 1), nbytes, seed=31 * na + nb) for na, nb in shapes]
    probs = [(A[:na], B[:nb]) for (A, B), (na, nb) in zip(probs, shapes)]
    probs.insert(2, mc.separating_case(nbytes))
    probs.insert(4, mc.identical_pair(70, 9, nbytes))
    if not small_only:
        probs.append(_big_pair(nbytes))
    return probs


def _upload(torch, probs):
    dev = torch.device("cuda")
    oa = np.zeros(len(probs) + 1, dtype=np.int32)
    ob = np.zeros(len(probs) + 1, dtype=np.int32)
    oa[1:] = np.cumsum([A.shape[0] for A, _ in probs])
    ob[1:] = np.cumsum([B.shape[0] for _, B in probs])
    return (torch.from_numpy(np.concatenate([A for A, _ in probs])).to(dev), torch.from_numpy(np.concatenate([B for _, B in probs])).to(dev),
            torch.from_numpy(oa).to(dev), torch.from_numpy(ob).to(dev), oa, ob)


@pytest.fixture(scope="module", params=[32, 61, 1])
def batch(gpu, request):
    """The problems of one descriptor length, their oracle (computed once) and the first call's results."""
    from ransac_with_homography_amd import kernels
    nbytes = request.param
    probs = _problems(nbytes, small_only=nbytes != 32)
    da, db, offa, offb, oa, ob = _upload(gpu, probs)
    train, dist = kernels.match_hamming_batched(da, db, offa, offb)
    return dict(nbytes=nbytes, probs=probs, dev=(da, db, offa, offb), oa=oa, ob=ob, want=[mc.per_query(A, B) for A, B in probs],
                first=(train.cpu().numpy(), dist.cpu().numpy()))


def test_batch_equals_oracle_and_host_twin(batch):
    from ransac_with_homography_amd import _lib
    lib = _lib.load()
    train, dist = batch["first"]
    oa, ob = batch["oa"], batch["ob"]
    assert train.dtype == np.int32 and dist.dtype == np.int32 and train.shape == dist.shape == (oa[-1],)
    assert (oa[1:-1] % 64 != 0).all() and (ob[1:-1] % 64 != 0).all()          # the problems start at no tile boundary
    for p, ((A, B), (want_t, want_d)) in enumerate(zip(batch["probs"], batch["want"])):
        got_t, got_d = train[oa[p]:oa[p + 1]], dist[oa[p]:oa[p + 1]]
        assert np.array_equal(got_t, want_t) and np.array_equal(got_d, want_d), (p, A.shape, B.shape)
        st, host_t, host_d = mc.host_match(lib, A, B)
        assert st == 0 and np.array_equal(host_t, got_t) and np.array_equal(host_d, got_d), (p, A.shape, B.shape)
    assert sum(int((t >= 0).sum()) for t, _ in batch["want"]) > len(batch["probs"])       # there were matches to get right


def test_second_call_is_bit_identical(gpu, batch):
    from ransac_with_homography_amd import kernels
    train, dist = kernels.match_hamming_batched(*batch["dev"])
    assert np.array_equal(train.cpu().numpy(), batch["first"][0]) and np.array_equal(dist.cpu().numpy(), batch["first"][1])


def test_alone_equals_in_the_batch(gpu, batch):
    from ransac_with_homography_amd import kernels
    oa = batch["oa"]
    alone = []
    for A, B in batch["probs"]:
        da, db, offa, offb, _, _ = _upload(gpu, [(A, B)])
        alone.append(kernels.match_hamming_batched(da, db, offa, offb))
    train = gpu.cat([t for t, _ in alone]).cpu().numpy()
    dist = gpu.cat([d for _, d in alone]).cpu().numpy()
    assert train.shape == (oa[-1],)
    assert np.array_equal(train, batch["first"][0]) and np.array_equal(dist, batch["first"][1])


def test_unsupported_length_raises(gpu):
    from ransac_with_homography_amd import kernels
    off = gpu.tensor([0, 4], dtype=gpu.int32, device="cuda")
    for nbytes in (0, 65):
        d = gpu.zeros((4, nbytes), dtype=gpu.uint8, device="cuda")
        with pytest.raises(NotImplementedError):
            kernels.match_hamming_batched(d, d, off, off)


def test_match_descriptors_returns_the_oracles_triple(gpu):
    import ransac as rs
    for A, B in (mc.separating_case(32), mc.random_pair(130, 257, 32, seed=5), mc.random_pair(70, 1, 61, seed=6)):
        want = mc.oracle(A, B)
        for got in (rs.match_descriptors(A, B), rs.match_descriptors(gpu.from_numpy(A).cuda(), gpu.from_numpy(B))):
            assert all(g.dtype == np.int32 for g in got)
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
    q, t, d = rs.match_descriptors(*mc.separating_case(32))
    assert list(zip(q.tolist(), t.tolist(), d.tolist())) == [(1, 1, 1), (0, 0, 3)]


def _planted_features(matches):
    """The 185 matchespoints with each side independently permuted; descriptors: random 256-bit rows for A, B's row of the true
    partner = A's row with (i % 20) bits flipped, so there are many distance ties."""
    ptsA, ptsB = matches
    n = len(ptsA)
    rng = np.random.RandomState(11)
    perm_a, perm_b = rng.permutation(n), rng.permutation(n)
    kps_a, kps_b = ptsA[perm_a], ptsB[perm_b]
    pos_b = np.argsort(perm_b)                       # original pair k sits at row pos_b[k] of B
    desc_a = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    desc_b = np.empty_like(desc_a)
    truth = set()
    for i in range(n):
        j = int(pos_b[perm_a[i]])
        desc_b[j] = mc.flip(desc_a[i], rng.choice(256, i % 20, replace=False))
        truth.add((i, j))
    return kps_a, desc_a, kps_b, desc_b, truth


def _same_results(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g[0] is None) == (w[0] is None) and (g[0] is None or np.array_equal(g[0], w[0]))
        assert np.array_equal(g[1][0], w[1][0]) and int(g[2]) == int(w[2])


def test_match_batch_feeds_run_batch(gpu, matches):
    import ransac as rs
    torch = gpu
    kps_a, desc_a, kps_b, desc_b, truth = _planted_features(matches)
    qi, ti, d = mc.oracle(desc_a, desc_b)
    assert set(zip(qi.tolist(), ti.tolist())) == truth and len(qi) == 185 and int(d.max()) <= 19      # on the CPU: the true pairs
    assert len(set(d.tolist())) < len(d)
    # problem 1: no train rows, so no matches; problem 2: three rows a side, three matches
    none = (kps_a[:5], desc_a[:5], kps_b[:0], desc_b[:0])
    few = (kps_a[:3], desc_a[:3], kps_a[:3] + np.float32(10), desc_a[:3][::-1].copy())
    feats = [(kps_a, desc_a, kps_b, desc_b), none, (torch.from_numpy(few[0]).cuda(), torch.from_numpy(few[1]), few[2], torch.from_numpy(few[3]).cuda())]
    want_idx = [(qi, ti), (qi[:0], ti[:0]), mc.oracle(few[1], few[3])[:2]]
    assert len(want_idx[2][0]) == 3
    host = [[f[0][q].T.copy(), f[2][t].T.copy()] for f, (q, t) in zip([feats[0], none, few], want_idx)]
    info = {}
    dp = rs.match_batch(feats, info=info)
    assert isinstance(dp, rs.DeviceProblems) and dp.sizes == [185, 0, 3]
    assert dp.pts_a.is_cuda and dp.pts_a.dtype == torch.float32
    assert np.array_equal(dp.pts_a.cpu().numpy(), np.concatenate([X.T for X, _ in host]))
    assert np.array_equal(dp.pts_b.cpu().numpy(), np.concatenate([Y.T for _, Y in host]))
    assert info["query_idx"].is_cuda and info["query_idx"].dtype == torch.int32 and info["train_idx"].dtype == torch.int32
    assert np.array_equal(info["query_idx"].cpu().numpy(), np.concatenate([q for q, _ in want_idx]))
    assert np.array_equal(info["train_idx"].cpu().numpy(), np.concatenate([t for _, t in want_idx]))
    kw = dict(seed=3, k=256, d=70, th=5, method="fwd")
    # run_batch as it stands: a problem of 0 or 3 correspondences gives (None, no inliers / its count, ...) on either route
    got = rs.run_batch(dp, refit=True, **kw)
    want = rs.run_batch(host, refit=True, **kw)
    _same_results(got, want)
    assert got[0][0] is not None and int(got[0][2]) > 100 and got[1][0] is None and int(got[1][2]) == 0 and got[2][0] is None
    i_dp, i_host = {}, {}
    got = rs.run_batch(dp, refit="device", info=i_dp, **kw)
    want = rs.run_batch(host, refit="device", info=i_host, **kw)
    _same_results(got, want)
    assert i_dp["H_device"].is_cuda
    assert np.array_equal(i_dp["H_device"].cpu().numpy(), i_host["H_device"].cpu().numpy(), equal_nan=True)
    assert np.array_equal(i_dp["refit_status"].cpu().numpy(), i_host["refit_status"].cpu().numpy())


def _small_pair():
    """A 96 x 128 uint8 RGB pair and 60 keypoints related by a mild homography, with planted descriptors."""
    rng = np.random.RandomState(21)
    img_a = rng.randint(0, 256, (96, 128, 3)).astype(np.uint8)
    img_b = rng.randint(0, 256, (96, 128, 3)).astype(np.uint8)
    H = np.array([[1.01, 0.02, 31.0], [-0.01, 0.99, 4.0], [1e-5, 2e-5, 1.0]])
    pa = (rng.rand(60, 2) * [120, 90] + 3).astype(np.float32)
    w = np.concatenate([pa.astype(np.float64), np.ones((60, 1))], axis=1) @ H.T
    pb = (w[:, :2] / w[:, 2:]).astype(np.float32)
    perm = rng.permutation(60)
    desc_a = rng.randint(0, 256, (60, 32)).astype(np.uint8)
    desc_b = np.stack([mc.flip(desc_a[i], rng.choice(256, i % 7, replace=False)) for i in perm])
    return img_a, img_b, (pa, desc_a, pb[perm], desc_b)


def test_stitching_with_features(gpu):
    import ransac as rs
    img_a, img_b, feats = _small_pair()
    qi, ti, _ = mc.oracle(feats[1], feats[3])
    assert len(qi) == 60
    oracle_matches = (feats[0][qi], feats[2][ti])
    kw = dict(ransacMet="fwd", th=5, d=70, k=200)
    np.random.seed(4)
    want = rs.stitching(img_a.copy(), img_b.copy(), matches=oracle_matches, **kw)
    np.random.seed(4)
    got = rs.stitching(img_a.copy(), img_b.copy(), features=feats, **kw)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    # matches= wins over features=: descriptors that would raise if they were looked at
    np.random.seed(4)
    both = rs.stitching(img_a.copy(), img_b.copy(), matches=oracle_matches, features=(None, None, None, None), **kw)
    assert np.array_equal(both, want)
