"""rwh_host_match_hamming, the host twin of the GPU matcher (include/rwh.h states the rule), without a GPU: exact equality with
the numpy oracle of tests/match_cases.py on the case that separates the rule from mutual nearest neighbour, on ties, on every
shape and descriptor length of the suite; empty sides; argument validation of both entry points."""
import re
import os

import numpy as np
import pytest

import match_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ransac_with_homography_amd import _lib
    return _lib.load()


def _same(lib, A, B):
    st, train, dist = mc.host_match(lib, A, B)
    want_t, want_d = mc.per_query(A, B)
    assert st == 0 and np.array_equal(train, want_t) and np.array_equal(dist, want_d)
    return train, dist


@pytest.mark.parametrize("nbytes", mc.NBYTES)
def test_separating_case(lib, nbytes):
    """The rule keeps (0, 0, 3), which mutual nearest neighbour drops: query 0's own nearest is train 1."""
    A, B = mc.separating_case(nbytes)
    train, dist = _same(lib, A, B)
    assert train.tolist() == [0, 1] and dist.tolist() == [3, 1]
    assert [tuple(int(v) for v in m) for m in zip(*mc.oracle(A, B))] == [(1, 1, 1), (0, 0, 3)]
    assert mc.mutual_nearest(A, B) == [(1, 1, 1)]


def test_ties_take_the_lowest_index(lib):
    """Duplicates on both sides: train rows 0 and 2 are equal and equally near queries 1 and 3 (equal): both pick query 1, and
    query 1 keeps train 0."""
    rng = np.random.RandomState(3)
    A = rng.randint(0, 256, (5, 32)).astype(np.uint8)
    B = rng.randint(0, 256, (4, 32)).astype(np.uint8)
    A[3] = A[1]
    B[0] = B[2] = mc.flip(A[1], [9])
    train, dist = _same(lib, A, B)
    assert train[1] == 0 and dist[1] == 1 and train[3] == -1
    A, B = mc.identical_pair(9, 11, 32)
    train, dist = _same(lib, A, B)
    assert train.tolist() == [0] + [-1] * 8 and dist.tolist() == [0] + [-1] * 8


@pytest.mark.parametrize("nbytes", mc.NBYTES)
@pytest.mark.parametrize("na,nb", mc.SHAPES)
def test_host_twin_equals_oracle(lib, na, nb, nbytes):
    _same(lib, *mc.random_pair(na, nb, nbytes, seed=1000 * na + nb + nbytes))


def test_oracle_order_is_a_stable_sort_by_distance():
    A, B = mc.random_pair(130, 257, 32, seed=5)
    qi, ti, d = mc.oracle(A, B)
    assert len(qi) > 10 and len(set(d.tolist())) < len(d)               # there are distance ties to order
    assert sorted(zip(d.tolist(), qi.tolist())) == list(zip(d.tolist(), qi.tolist()))
    D = mc.distances(A, B)
    assert all(D[i, j] == dd for i, j, dd in zip(qi, ti, d))


def test_empty_sides_give_no_matches(lib):
    B = np.zeros((5, 32), dtype=np.uint8)
    st, train, dist = mc.host_match(lib, np.zeros((0, 32), dtype=np.uint8), B)
    assert st == 0 and train.size == 0
    st, train, dist = mc.host_match(lib, B, np.zeros((0, 32), dtype=np.uint8))
    assert st == 0 and train.tolist() == [-1] * 5 and dist.tolist() == [-1] * 5
    assert [a.size for a in mc.oracle(B[:0], B)] == [0, 0, 0] and [a.size for a in mc.oracle(B, B[:0])] == [0, 0, 0]


def test_unsupported_lengths(lib):
    buf = np.zeros(4 * 65, dtype=np.uint8)
    out = np.zeros(4, dtype=np.int32)
    one = 8                 # non-NULL, 8-byte aligned, never dereferenced: validation comes first
    for nbytes in (0, 65, -1):
        assert lib.rwh_host_match_hamming(buf.ctypes.data, 4, buf.ctypes.data, 4, nbytes, out.ctypes.data, out.ctypes.data) == -2
        assert lib.rwh_match_hamming_batched(one, one, nbytes, one, one, 1, 4, 4, one, one, one, 1 << 20, mc.null) == -2
    for nbytes in (1, 64):
        assert lib.rwh_host_match_hamming(buf.ctypes.data, 4, buf.ctypes.data, 4, nbytes, out.ctypes.data, out.ctypes.data) == 0


def test_argument_validation(lib):
    """NULL pointers and negative sizes: RWH_E_INVALID before any device is touched (this runs without one)."""
    A = np.zeros((4, 32), dtype=np.uint8)
    out = np.zeros(4, dtype=np.int32)
    good = [A.ctypes.data, 4, A.ctypes.data, 4, 32, out.ctypes.data, out.ctypes.data]
    assert lib.rwh_host_match_hamming(*good) == 0
    for i in (0, 2, 5, 6):
        bad = list(good)
        bad[i] = mc.null
        assert lib.rwh_host_match_hamming(*bad) == -1
    for i in (1, 3):
        bad = list(good)
        bad[i] = -1
        assert lib.rwh_host_match_hamming(*bad) == -1
    one = 8
    need = lib.rwh_match_workspace_bytes(2, 4, 4)
    assert need == 8 * (4 + 4 + 2 + 1)
    assert lib.rwh_match_workspace_bytes(0, 4, 4) == -1 and lib.rwh_match_workspace_bytes(1, -1, 4) == -1
    good = [one, one, 32, one, one, 2, 4, 4, one, one, one, need, mc.null]
    for i in (0, 1, 3, 4, 8, 9, 10):
        bad = list(good)
        bad[i] = mc.null
        assert lib.rwh_match_hamming_batched(*bad) == -1, i
    for i, v in ((5, 0), (5, -1), (6, -1), (7, -1), (11, need - 1), (10, 12)):      # P, totals, workspace size and alignment
        bad = list(good)
        bad[i] = v
        assert lib.rwh_match_hamming_batched(*bad) == -1, (i, v)
    # no query rows: nothing to do, whatever the other side holds, and no device is touched
    assert lib.rwh_match_hamming_batched(mc.null, one, 32, one, one, 1, 0, 4, mc.null, mc.null, one, 1 << 10, mc.null) == 0


def test_python_constants_match_the_header():
    from ransac_with_homography_amd import _lib, kernels
    hdr = open(os.path.join(ROOT, "include", "rwh.h")).read()
    for name in ("RWH_MATCH_MAX_BYTES", "RWH_MATCH_TILE_TRAIN", "RWH_MATCH_CHUNK_QUERY", "RWH_MATCH_SEG_QUERY", "RWH_MATCH_GRID_MAX"):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == getattr(_lib, name)
    assert (kernels.MATCH_TILE_TRAIN, kernels.MATCH_CHUNK_QUERY, kernels.MATCH_SEG_QUERY, kernels.MATCH_GRID_MAX) == \
        (_lib.RWH_MATCH_TILE_TRAIN, _lib.RWH_MATCH_CHUNK_QUERY, _lib.RWH_MATCH_SEG_QUERY, _lib.RWH_MATCH_GRID_MAX)
    assert kernels.MATCH_SEG_QUERY % kernels.MATCH_CHUNK_QUERY == 0


def test_match_entry_points_need_a_gpu():
    import torch
    if torch.cuda.is_available():
        return              # with a GPU these calls succeed: tests/test_match_gpu.py
    import ransac as rs
    from ransac_with_homography_amd import RwhUnavailable
    A = np.zeros((4, 32), dtype=np.uint8)
    with pytest.raises(RwhUnavailable):
        rs.match_descriptors(A, A)
    with pytest.raises(RwhUnavailable):
        rs.match_batch([(np.zeros((4, 2), np.float32), A, np.zeros((4, 2), np.float32), A)])
