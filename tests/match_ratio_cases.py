"""Helpers of the ratio matcher's tests (test_match_ratio_cpu.py, test_match_ratio_gpu.py) -- not a test module.

`per_query` restates rules 1 - 3 of the ratio rule (include/rwh.h, rwh_match_ratio_graph) in numpy on `match_cases.distances`:
argmin for the nearest row, the minimum over the other rows for the runner-up, an integer comparison for the ratio, and per train
row the first minimum of d1 among its candidates; `ordered` is rule 4.  Everything is an integer: every comparison in the tests is
exact equality.  The generators: unrelated sets, planted partners among distractors, the pair graph of the GPU tests, and the three
crops of the sequence tests with their known shifts."""
import numpy as np

import match_cases as mc

RATIOS = ((7, 10), (1, 1), (1, 1024))
CROP_COLUMNS, CROP_WIDTH = (0, 90, 180), 260
CROP_PAIRS = ((1, 0), (2, 0), (2, 1))


def per_query(A, B, num=7, den=10):
    """Rules 1 - 3: (train_idx, distance, second), int32 [Na] each, -1 / -1 / -1 for a query without a match."""
    na, nb = A.shape[0], B.shape[0]
    train, dist, second = (np.full(na, -1, dtype=np.int32) for _ in range(3))
    if na == 0 or nb < 2:                   # rule 1: no second distance, no candidate
        return train, dist, second
    D = mc.distances(A, B).astype(np.int64)
    rows = np.arange(na)
    j1 = D.argmin(axis=1)
    d1 = D[rows, j1]
    D[rows, j1] = np.iinfo(np.int64).max
    d2 = D.min(axis=1)                      # the smallest over j != j1: equal to d1 when two rows tie
    cand = den * d1 < num * d2              # rule 2: integers, strict
    for j in np.unique(j1[cand]):           # rule 3: per train row the candidate with the smallest d1, the lowest i on ties
        idx = np.nonzero(cand & (j1 == j))[0]
        i = idx[d1[idx].argmin()]
        train[i], dist[i], second[i] = j, d1[i], d2[i]
    return train, dist, second


def candidates(A, B, num=7, den=10):
    """What the branches of the rule see on one pair: (candidates, queries with d1 == d2, candidates dropped by rule 3)."""
    if A.shape[0] == 0 or B.shape[0] < 2:
        return 0, 0, 0
    D = np.sort(mc.distances(A, B).astype(np.int64), axis=1)
    cand = int((den * D[:, 0] < num * D[:, 1]).sum())
    return cand, int((D[:, 0] == D[:, 1]).sum()), cand - int((per_query(A, B, num, den)[0] >= 0).sum())


def ordered(train, dist, second):
    """Rule 4: the surviving (i, j1, d1, d2) by (d1, i) -- a stable sort by distance of the list in query order."""
    i = np.nonzero(train >= 0)[0]
    i = i[np.argsort(dist[i], kind="stable")]
    return i.astype(np.int32), train[i].astype(np.int32), dist[i].astype(np.int32), second[i].astype(np.int32)


def oracle(A, B, num=7, den=10):
    """(queryIdx, trainIdx, distance, second) in the order of rule 4."""
    return ordered(*per_query(A, B, num, den))


def host_match(lib, A, B, num=7, den=10):
    """rwh_host_match_ratio on one pair -> (status, train_idx, distance, second)."""
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    out = [np.full(max(A.shape[0], 1), -7, dtype=np.int32) for _ in range(3)]
    st = lib.rwh_host_match_ratio(A.ctypes.data if A.size else mc.null, A.shape[0], B.ctypes.data if B.size else mc.null, B.shape[0],
                                  A.shape[1], num, den, *[o.ctypes.data for o in out])
    return (st,) + tuple(o[:A.shape[0]] for o in out)


def flipped(row, rng, count):
    """`row` with `count` distinct bits flipped."""
    return mc.flip(row, rng.choice(8 * row.shape[0], count, replace=False))


def unrelated_sets(n=300, nbytes=32, seed=41):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (n, nbytes)).astype(np.uint8), rng.randint(0, 256, (n, nbytes)).astype(np.uint8)


def planted_features(matches, distractors=115, seed=11):
    """The 185 matchespoints with each side independently permuted among `distractors` unrelated rows per side (built as
    test_match_gpu.py builds its planted features): random 256-bit rows for A; B's row of the true partner = A's row with (k % 20)
    bits flipped, so there are many distance ties; the distractors are random rows with random keypoints.  Returns
    (kps_a, desc_a, kps_b, desc_b, truth), truth = the set of planted (i, j)."""
    ptsA, ptsB = matches
    m, n = len(ptsA), len(ptsA) + distractors
    rng = np.random.RandomState(seed)
    kps_a = np.concatenate([ptsA, (rng.rand(distractors, 2) * 400).astype(np.float32)]).astype(np.float32)
    kps_b = np.concatenate([ptsB, (rng.rand(distractors, 2) * 400).astype(np.float32)]).astype(np.float32)
    desc_a = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    desc_b = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    for k in range(m):
        desc_b[k] = flipped(desc_a[k], rng, k % 20)
    perm_a, perm_b = rng.permutation(n), rng.permutation(n)
    pos_a, pos_b = np.argsort(perm_a), np.argsort(perm_b)           # original row k sits at row pos[k]
    truth = set((int(pos_a[k]), int(pos_b[k])) for k in range(m))
    return kps_a[perm_a], desc_a[perm_a], kps_b[perm_b], desc_b[perm_b], truth


def plant_block_edges(A, B, T, C, S):
    """Plants, in a pair of at least 2 T + 1 query and 2 S + 4 train rows of at least 32 bytes, the cases that separate a correct
    split of the work from a wrong one at ratio 7 / 10, and returns {query row: its train row, or -1 for no match}.  T: query rows per
    block, C: train rows staged at a time, S: train rows per block.  Every query row used is drawn afresh first, so that nothing
    else in B is near it."""
    rng = np.random.RandomState(1234)
    want = {}
    fresh = lambda: rng.randint(0, 256, A.shape[1]).astype(np.uint8)
    # the nearest train row duplicated across a chunk boundary, and across a segment boundary: d1 == d2, no match -- a runner-up
    # lost between chunks or between blocks would accept them
    A[5] = fresh()
    B[C - 1] = B[C] = flipped(A[5], rng, 1)
    want[5] = -1
    A[T + 44] = fresh()
    B[S - 1] = B[S] = flipped(A[T + 44], rng, 2)
    want[T + 44] = -1
    # the runner-up in another segment, at a distance that just fails (7 and 10: 70 < 70 is false) and one that just passes (7 and 11)
    A[7] = fresh()
    B[10], B[S + 20] = flipped(A[7], rng, 7), flipped(A[7], rng, 10)
    want[7] = -1
    A[2 * T + 8] = fresh()
    B[12], B[S + 22] = flipped(A[2 * T + 8], rng, 7), flipped(A[2 * T + 8], rng, 11)
    want[2 * T + 8] = 12
    # two identical queries either side of a query-tile boundary claim one train row: the lower index keeps it
    A[T - 1] = A[T] = fresh()
    B[2 * S + 3] = flipped(A[T], rng, 3)
    want[T - 1], want[T] = 2 * S + 3, -1
    return want


GRAPH_SMALL = (0, 1, 2, 63, 65, 70, 257)


def graph(nbytes, T, C, S):
    """The pair graph of the GPU tests for one descriptor length: images of 0, 1, 2, 63, 65, 70 and 257 rows (near copies of rows of
    the large ones, so there are matches), one of 2 max(T, S) + C + 5 rows (image 7) and one of 2 max(T, S) + 37 (image 8), the
    large two made by `match_cases.random_pair` with `plant_block_edges` on top where the rows have the bits for it.  The pair
    list uses the large images both as query and as train, lists (s, d) and (d, s), one pair twice, one (s, s), and pairs with the
    empty and the 1-row image on either side.  Returns (images, pairs, planted) -- planted: `plant_block_edges`' expectations for
    the pair (7, 8), empty for short rows."""
    big = 2 * max(T, S)
    A, B = mc.random_pair(big + C + 5, big + 37, nbytes, seed=177 + nbytes)
    planted = plant_block_edges(A, B, T, C, S) if nbytes >= 32 else {}
    rng = np.random.RandomState(nbytes)
    images = []
    for k, n in enumerate(GRAPH_SMALL):
        src = (A if k % 2 else B)[:n]
        images.append(np.stack([flipped(r, rng, min(rng.randint(0, 4), 8 * nbytes)) for r in src]) if n else np.zeros((0, nbytes), dtype=np.uint8))
    images += [A, B]
    pairs = [(7, 8), (8, 7), (3, 4), (7, 8), (7, 7), (0, 8), (8, 0), (1, 8), (8, 1), (4, 3), (2, 5), (5, 2), (6, 5), (5, 6), (6, 7),
             (0, 0), (1, 0), (0, 1), (1, 1), (2, 2)]
    return images, pairs, planted


def crops():
    """The three crops of the sequence tests (test_sequence_bundle_gpu.py): columns 0, 90 and 180 of `sequence_cases.scene()`, 260
    wide.  A point (x, y) of crop s lies at (x + CROP_COLUMNS[s] - CROP_COLUMNS[d], y) in crop d."""
    import sequence_cases as sc
    scene = sc.scene()
    return [np.ascontiguousarray(scene[:, x:x + CROP_WIDTH]) for x in CROP_COLUMNS]


def true_matches(kps_s, kps_d, s, d, qi, ti):
    """How many of the matches (qi, ti) of the crop pair (s, d) lie within 1 px of the known shift."""
    shift = np.array([CROP_COLUMNS[s] - CROP_COLUMNS[d], 0], dtype=np.float64)
    err = np.abs(kps_s[qi].astype(np.float64) + shift - kps_d[ti].astype(np.float64)).max(axis=1) if len(qi) else np.zeros(0)
    return int((err <= 1.0).sum())


def crop_counts(feats, num=7, den=10):
    """Per crop pair (s, d): (matches, true) under cross-check and under the ratio rule, on feats = [(kps, desc)] per crop (numpy)."""
    out = {}
    for s, d in CROP_PAIRS:
        (ks, ds), (kd, dd) = feats[s], feats[d]
        qi, ti, _ = mc.oracle(ds, dd)
        rq, rt, _, _ = oracle(ds, dd, num, den)
        out[(s, d)] = dict(cross=(len(qi), true_matches(ks, kd, s, d, qi, ti)), ratio=(len(rq), true_matches(ks, kd, s, d, rq, rt)))
    return out
