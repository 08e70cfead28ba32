"""Helpers of the matchers' long-list tests (test_match_long_cpu.py, test_match_long_gpu.py) -- not a test module.

Both main kernels run a grid of at most GRID_MAX blocks that strides over a block list built on the device from prefix sums over
the pairs, 256 threads scanning a run of ceil(P / 256) pairs each.  The fixtures here make that list long: one POOL of twelve small
images and pair lists of P = 256 .. 4500 drawn from the pool's 144 ordered pairs, so that the restatements (`match_cases.per_query`,
`match_ratio_cases.per_query`) are computed once per distinct pair, whatever P.  `blocks_ratio` / `blocks_cross` count the block
list as include/rwh.h states the split, and `live_prefix` is the model of the header's three bounds on a pair's rows (total_query,
total_train, the workspace).  Everything is an integer: every comparison in the tests is exact equality."""
import numpy as np

import match_cases as mc
import match_ratio_cases as rc

LONG_P = (256, 257, 513, 2016, 4500)
# every template instance (1, 2, 4, 8, 16 dwords; 1 byte runs in the sibling files): its shortest length, its longest, and one
# that is no multiple of 4
WIDTHS = (2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 31, 33, 60, 63, 64)
POOL_SEED = 600


def block_shape():
    """(ratio: TILE_QUERY, CHUNK_TRAIN, SEG_TRAIN, GRID_MAX), (cross-check: TILE_TRAIN, CHUNK_QUERY, SEG_QUERY, GRID_MAX) as exported."""
    from ransac_with_homography_amd import kernels as k
    return ((k.MATCH2_TILE_QUERY, k.MATCH2_CHUNK_TRAIN, k.MATCH2_SEG_TRAIN, k.MATCH2_GRID_MAX),
            (k.MATCH_TILE_TRAIN, k.MATCH_CHUNK_QUERY, k.MATCH_SEG_QUERY, k.MATCH_GRID_MAX))


def pool_sizes():
    """Rows of the twelve images: none, 1 .. 3, either side of the staging chunk, 70, 130, one past the block, 300, and more than two
    blocks on either side of either kernel (2 * 256 + 69 with the shape as it stands, as `match_ratio_cases.graph` sizes its largest)."""
    (T2, C2, S2, _), (T1, C1, S1, _) = block_shape()
    C, B = max(C1, C2), max(T1, S1, T2, S2)
    return [0, 1, 2, 3, C - 1, C, C + 1, 70, 130, B + 1, 300, 2 * B + 69]


def pool(nbytes, seed=POOL_SEED):
    """The twelve images, cut from the two sides of ONE match_cases.random_pair(600, 600), alternating sides and at different
    rows: images of one side overlap (exact copies, and that side's planted duplicates: ties), images of different sides hold the
    planted cross-copies and near-duplicates."""
    sizes = pool_sizes()
    rows = max(600, max(sizes))
    A, B = mc.random_pair(rows, rows, nbytes, seed)
    images = []
    for k, n in enumerate(sizes):
        src = A if k % 2 else B
        start = (37 * k) % (rows - n + 1)
        images.append(np.ascontiguousarray(src[start:start + n]))
    return images


def long_list(P, seed=None):
    """P ordered pairs (s, d) drawn with replacement from the 144 of the pool: repeats, (s, s) and the empty and the 1-row image on
    either side all occur.  The seed defaults to P."""
    n = len(pool_sizes())
    draw = np.random.RandomState(P if seed is None else seed).randint(0, n * n, P)
    return [(int(k) // n, int(k) % n) for k in draw]


def ceil_div(a, b):
    return (a + b - 1) // b


def blocks_ratio(sizes, pairs):
    """Blocks of match2_query_kernel: per pair ceil(na / TILE_QUERY) * ceil(nb / SEG_TRAIN), none where nb < 2."""
    (T, _, S, _), _ = block_shape()
    return sum(ceil_div(sizes[s], T) * ceil_div(sizes[d], S) for s, d in pairs if sizes[d] >= 2)


def blocks_cross(sizes, pairs):
    """Blocks of match_train_kernel: per problem ceil(na / SEG_QUERY) * ceil(nb / TILE_TRAIN)."""
    _, (T, _, S, _) = block_shape()
    return sum(ceil_div(sizes[s], S) * ceil_div(sizes[d], T) for s, d in pairs)


def live_prefix(na, nb, total_query, total_train, capacity):
    """Which pairs of the ratio rule are worked on (include/rwh.h, the argument list of rwh_match_ratio_graph): pair p is live iff
    the sums over the pairs 0 .. p of na, of nb and of the partials na * ceil(nb / SEG_TRAIN) stay within total_query, total_train
    and `capacity` (the partials the workspace holds); behind the first pair that is not live none is.  -> list of bool."""
    (_, _, S, _), _ = block_shape()
    live, q, t, part, ok = [], 0, 0, 0, True
    for a, b in zip(na, nb):
        q, t, part = q + int(a), t + int(b), part + int(a) * ceil_div(int(b), S)
        ok = ok and q <= total_query and t <= total_train and part <= capacity
        live.append(ok)
    return live


def partial_capacity(lib, n_pairs, total_train, workspace_bytes):
    """The partials a workspace of `workspace_bytes` holds, as the header sizes it: what is left behind owner[total_train] and the
    four tables of P + 1, in 8-byte entries."""
    return (workspace_bytes - lib.rwh_match_ratio_workspace_bytes(n_pairs, 0, total_train, 0)) // 8


_RESTATED = {}


def restated(nbytes=32):
    """(images, ratio, cross): the pool and, per ordered pair (s, d) of it, rc.per_query (7 / 10) and mc.per_query of image s against
    image d.  Computed once per descriptor length and shared: nobody writes into it."""
    if nbytes not in _RESTATED:
        images = pool(nbytes)
        every = [(s, d) for s in range(len(images)) for d in range(len(images))]
        _RESTATED[nbytes] = (images, {pr: rc.per_query(images[pr[0]], images[pr[1]]) for pr in every},
                             {pr: mc.per_query(images[pr[0]], images[pr[1]]) for pr in every})
    return _RESTATED[nbytes]


def offsets(counts):
    off = np.zeros(len(counts) + 1, dtype=np.int32)
    off[1:] = np.cumsum(counts)
    return off


def expected(want, pairs, n_out):
    """The restatement of a pair list: per output array the pairs' slices concatenated in pair order."""
    return [np.concatenate([want[pr][k] for pr in pairs]) for k in range(n_out)]


def first_wrong_pair(got, want, pairs, rows):
    """The first pair whose slice of some output differs from the restatement's, as (index, pair, got, want), or None."""
    for p, pr in enumerate(pairs):
        for g, w in zip(got, want[pr]):
            if not np.array_equal(g[rows[p]:rows[p + 1]], w):
                return p, pr, g[rows[p]:rows[p + 1]], w
    return None


def big_cross(nbytes):
    """The chunk-, segment- and tile-crossing pair of the cross-check matcher as test_match_gpu.py builds it: more than two train
    tiles and query segments, equal queries either side of a chunk and of a segment boundary, equal train rows either side of a tile
    boundary."""
    _, (T, C, S, _) = block_shape()
    n = 2 * max(T, S)
    A, B = mc.random_pair(n + C + 5, n + 37, nbytes, seed=77 + nbytes)
    A[C] = A[C - 1]
    B[3] = mc.flip(A[C], [2])
    A[S] = A[S - 1]
    B[T + 9] = mc.flip(A[S], [5, 6])
    B[T] = B[T - 1] = mc.flip(A[2 * S + 1], [1])
    return A, B


def width_problems(nbytes):
    """The four problems of the every-width test, as (ratio's, cross-check's): the block-crossing pair of 2 * 256 + 69 by
    2 * 256 + 37 rows (`match_ratio_cases.graph`'s images 7 and 8, with `plant_block_edges` from 32 bytes on; `big_cross`), (70, 65),
    (1, 70) and (65, 2)."""
    (T, C, S, _), _ = block_shape()
    images, _, _ = rc.graph(nbytes, T, C, S)
    small = [mc.random_pair(na, nb, nbytes, seed=900 + 31 * na + nb + nbytes) for na, nb in ((70, 65), (1, 70), (65, 2))]
    return [(images[7], images[8])] + small, [big_cross(nbytes)] + small


def extreme_problems():
    """64-byte rows at the ends of the distance range, four problems (A, B):
      0. A: 70 rows of 0x00, B: 65 rows of 0xFF -- every distance is 8 * 64 = 512, the top of the packed keys' distance field.
         Cross-check: every train row picks query 0, which keeps train row 0: the one match (0, 0, 512).  Ratio: every query ties,
         no match.
      1. A's row 37 is 0xFF with one bit cleared.  Cross-check: every train row now picks query 37 at distance 1: (37, 0, 1) alone.
         Ratio: B's rows are all equal, so query 37 ties at 1 as the others tie at 512: still no match.
      2. The same A against 65 rows of 0x00 with 0xFF at row 5.  Ratio: (37, 5, 1, 511), the rows of 0x00 tie at 0.  Cross-check:
         (0, 0, 0) and (37, 5, 1).
      3. A's row 37 is 0xFF itself, the same B: the ratio rule's (37, 5, 0, 512) -- the largest SECOND distance."""
    A0 = np.zeros((70, 64), dtype=np.uint8)
    B0 = np.full((65, 64), 0xFF, dtype=np.uint8)
    A1 = A0.copy()
    A1[37] = mc.flip(B0[0], [100])
    B2 = np.zeros((65, 64), dtype=np.uint8)
    B2[5] = 0xFF
    A3 = A0.copy()
    A3[37] = 0xFF
    return [(A0, B0), (A1, B0), (A1, B2), (A3, B2)]


def sequence_features(n_images=64, nbytes=32, seed=64):
    """The pipeline's largest graph: `n_images` images of 24 .. 60 keypoints with seeded positions; image k's descriptors are rows
    of image k - 1 with 0 .. 3 bits flipped (fresh rows where it has more than its neighbour), so adjacent pairs have matches and
    distant ones a few.  -> [(kps float32 [n, 2], desc uint8 [n, nbytes])]."""
    rng = np.random.RandomState(seed)
    feats, prev = [], None
    for _ in range(n_images):
        n = int(rng.randint(24, 61))
        desc = rng.randint(0, 256, (n, nbytes)).astype(np.uint8)
        if prev is not None:
            take = rng.permutation(prev.shape[0])[:n]
            for r, src in enumerate(take):
                desc[r] = rc.flipped(prev[src], rng, int(rng.randint(0, 4)))
            desc = desc[rng.permutation(n)]
        feats.append(((rng.rand(n, 2) * 400).astype(np.float32), desc))
        prev = desc
    return feats
