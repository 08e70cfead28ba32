"""Helpers of the matcher's tests (test_match_cpu.py, test_match_gpu.py) -- not a test module.

`oracle` restates the rule of include/rwh.h (rwh_match_hamming_batched) in numpy: a per-byte popcount table for the distance
matrix, argmin (first index on ties) for both reductions, a stable sort for the order.  Everything is an integer: every comparison
in the tests is exact equality."""
import ctypes

import numpy as np

POPCOUNT = np.array([bin(v).count("1") for v in range(256)], dtype=np.int32)

# (Na, Nb) every suite runs, and the descriptor lengths: ORB 32, AKAZE 61 (no multiple of 4), BRISK 64, and the shortest
SHAPES = ((1, 1), (1, 70), (70, 1), (63, 65), (64, 64), (130, 257), (500, 500))
NBYTES = (1, 32, 61, 64)
null = ctypes.c_void_p(0)


def distances(A, B):
    """D[i, j] = popcount(A[i] xor B[j]), int32 [Na, Nb]; in row blocks, so that 500 x 500 x 64 stays small."""
    D = np.empty((A.shape[0], B.shape[0]), dtype=np.int32)
    for i0 in range(0, A.shape[0], 64):
        D[i0:i0 + 64] = POPCOUNT[A[i0:i0 + 64, None, :] ^ B[None, :, :]].sum(axis=2)
    return D


def per_query(A, B):
    """Rules 1 and 2: (train_idx, distance), int32 [Na] each, -1 / -1 for a query without a match."""
    na, nb = A.shape[0], B.shape[0]
    train = np.full(na, -1, dtype=np.int32)
    dist = np.full(na, -1, dtype=np.int32)
    if na == 0 or nb == 0:
        return train, dist
    D = distances(A, B)
    q = D.argmin(axis=0)                    # rule 1: per train row the nearest query, the lowest i on ties
    dT = D[q, np.arange(nb)]
    for i in np.unique(q):                  # rule 2: per chosen query the nearest of its train rows, the lowest j on ties
        js = np.nonzero(q == i)[0]
        j = js[dT[js].argmin()]
        train[i], dist[i] = j, dT[j]
    return train, dist


def ordered(train, dist):
    """Rule 3: the surviving (i, j, distance) by (distance, i) -- a stable sort by distance of the list in query order."""
    i = np.nonzero(train >= 0)[0]
    o = np.argsort(dist[i], kind="stable")
    i = i[o]
    return i.astype(np.int32), train[i].astype(np.int32), dist[i].astype(np.int32)


def oracle(A, B):
    """(queryIdx, trainIdx, distance) in the order of rule 3."""
    return ordered(*per_query(A, B))


def mutual_nearest(A, B):
    """The textbook rule the code must NOT implement: (i, j) with i nearest to j and j nearest to i (first index on ties)."""
    D = distances(A, B)
    q, t = D.argmin(axis=0), D.argmin(axis=1)
    return [(int(i), int(t[i]), int(D[i, t[i]])) for i in range(A.shape[0]) if q[t[i]] == i]


def flip(row, bits):
    out = row.copy()
    for b in bits:
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def separating_case(nbytes=32):
    """The 2 x 2 case of the issue: D[0,0] = 3, D[1,0] = 6, D[0,1] = 2, D[1,1] = 1.  The rule gives (0, 0, 3) and (1, 1, 1);
    mutual nearest neighbour gives (1, 1, 1) alone.  Needs 6 bits, so nbytes >= 1."""
    rng = np.random.RandomState(99)
    b1 = rng.randint(0, 256, nbytes).astype(np.uint8)
    a1 = flip(b1, [0])
    a0 = flip(b1, [1, 2])
    b0 = flip(a0, [3, 4, 5])
    A, B = np.stack([a0, a1]), np.stack([b0, b1])
    assert distances(A, B).tolist() == [[3, 2], [6, 1]]
    return A, B


def random_pair(na, nb, nbytes, seed):
    """Seeded random descriptors with planted structure: exact duplicates on both sides (ties, resolved by the lowest index),
    rows copied across the sides (distance 0), near-duplicates (a few flipped bits)."""
    rng = np.random.RandomState(seed)
    A = rng.randint(0, 256, (na, nbytes)).astype(np.uint8)
    B = rng.randint(0, 256, (nb, nbytes)).astype(np.uint8)
    nbits = 8 * nbytes
    for _ in range(max(1, min(na, nb) // 4)):
        i, j = rng.randint(na), rng.randint(nb)
        kind = rng.randint(4)
        if kind == 0:                       # B's row is A's row
            B[j] = A[i]
        elif kind == 1:                     # ... with a few bits flipped
            B[j] = flip(A[i], rng.randint(0, nbits, rng.randint(1, 4)))
        elif kind == 2:                     # a duplicate inside A (and its copy in B): a tie between two query rows
            A[rng.randint(na)] = A[i]
            B[j] = flip(A[i], rng.randint(0, nbits, 1))
        else:                               # a duplicate inside B: two train rows pick the same query at the same distance
            B[rng.randint(nb)] = B[j] = flip(A[i], rng.randint(0, nbits, 2))
    return A, B


def identical_pair(na, nb, nbytes):
    """Every row the same descriptor: all distances 0, every train row picks query 0, query 0 keeps train 0."""
    row = np.arange(7, 7 + nbytes, dtype=np.uint8)
    return np.tile(row, (na, 1)), np.tile(row, (nb, 1))


def host_match(lib, A, B):
    """rwh_host_match_hamming on one pair -> (status, train_idx, distance)."""
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    train = np.full(max(A.shape[0], 1), -7, dtype=np.int32)
    dist = np.full(max(A.shape[0], 1), -7, dtype=np.int32)
    st = lib.rwh_host_match_hamming(A.ctypes.data if A.size else null, A.shape[0], B.ctypes.data if B.size else null, B.shape[0],
                                    A.shape[1], train.ctypes.data, dist.ctypes.data)
    return st, train[:A.shape[0]], dist[:A.shape[0]]
