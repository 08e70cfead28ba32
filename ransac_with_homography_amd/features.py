"""The feature front end of the pipeline on the MI355X: the stage of the reference's ransac.py:252-267 (ORB_create().detectAndCompute
on both images, BFMatcher(NORM_HAMMING, crossCheck=True).match) in front of the RANSAC search, batched over many images and pairs.

    extract_batch    FAST-9 corners + steered BRIEF, on one scale or on a scale pyramid (rules 1 - 8 of include/rwh.h):
                     rwh_orb_pyramid_batched (more than one level only) -> rwh_orb_detect_batched -> one sort -> rwh_orb_describe_batched
    match_batch      brute-force Hamming matches with cross-check (rwh_match_hamming_batched), handed over as `DeviceProblems`,
                     the correspondences `ransac.run_batch` takes without a visit to the host
    match_graph      Hamming matches under the 2-nearest ratio test for the pairs of a pair graph (rwh_match_ratio_graph), every
                     image's descriptors held once; the same hand-off

`orb_layout` is the one statement of the extractor's buffer and table; `orb_bin_table`, `orb_scales`, `orb_level_quotas`,
`default_pattern` and `rotate_pattern` make the library calls' tables on the host; `detect_and_describe` and `match_descriptors`
are the one-image / one-pair forms with numpy out.  Both stages follow the rules as include/rwh.h states them, NOT OpenCV's code.
`ransac.py` imports the public names, so `from ransac_with_homography_amd.ransac import extract_batch, ...` keeps working.
There is no CPU implementation here: without librwh_hip.so and a GPU both stages raise `RwhUnavailable`.
"""
import numpy as np

from . import _lib, kernels


class DeviceProblems(object):
    """Correspondences that already live on the GPU (the hand-off of SURVEY.md 8f row f-3): the problems' matches
    concatenated, pts_a / pts_b float32 [total, 2] torch tensors on the device (the `matchespoints` layout, points in rows),
    `sizes` = correspondences per problem (host ints).  `run_batch` takes it in place of the list of [X, Y] arrays."""

    def __init__(self, pts_a, pts_b, sizes):
        import torch
        self.sizes = [int(m) for m in sizes]
        assert pts_a.is_cuda and pts_b.is_cuda and pts_a.dtype == torch.float32 and pts_b.dtype == torch.float32
        assert tuple(pts_a.shape) == tuple(pts_b.shape) == (sum(self.sizes), 2)
        self.pts_a, self.pts_b = pts_a.contiguous(), pts_b.contiguous()

    def __len__(self):
        return len(self.sizes)


def _to_device(x, dtype, dev, what):
    """numpy array or tensor -> contiguous tensor of `dtype` on the GPU; a wrong dtype is refused, not cast."""
    import torch
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype != dtype:
        raise TypeError("%s: expected %s, got %s" % (what, dtype, t.dtype))
    return t.to(dev).contiguous()


def _host_rows(kps):
    return kps.cpu().numpy() if hasattr(kps, "cpu") else np.asarray(kps)


def match_batch(features, info=None):
    """Brute-force Hamming matches with cross-check for MANY image pairs in one GPU submission, handed over as the
    `DeviceProblems` that `run_batch` takes: the stage of ransac.py:258-267 (BFMatcher(NORM_HAMMING, crossCheck=True).match,
    sorted by distance, keypoints gathered) in front of the batched search, without a visit to the host.

    features: list of (kpsA float32 [Na, 2], descA uint8 [Na, nbytes], kpsB float32 [Nb, 2], descB uint8 [Nb, nbytes]) per pair,
    numpy arrays or tensors; A is the "query" side, B the "train" side; one nbytes (1 .. 64) for the whole list.  Any binary
    extractor (ORB, BRIEF, BRISK, AKAZE, ...) serves; `extract_batch` is the package's own.

    The rule (include/rwh.h, rwh_match_hamming_batched): D[i, j] = popcount(A[i] xor B[j]); every train row j picks its nearest
    query q[j] (lowest i on ties); every query i keeps, of the train rows that picked it, the nearest (lowest j on ties); the
    matches are ordered by (distance, i), and problem p's correspondences are kpsA[i], kpsB[j] in that order.  This is how the
    crossCheck path of OpenCV 4's BFMatcher reads -- NOT the textbook mutual nearest neighbour -- and parity with OpenCV is NOT
    verified (OpenCV is not a dependency); the code is held to the rule as stated.

    Returns a `DeviceProblems`.  The distances come from one library call; compaction, the ordering (one sort on a packed
    (problem, distance, i) key) and the keypoint gather are tensor operations on the device, and the one download is the P match
    counts that `DeviceProblems.sizes` holds.  `info`: optional dict, receives "query_idx" and "train_idx" (int32 device tensors,
    indices inside each problem, in the order of the correspondences) and "distance".

    A pair may have no matches (an empty side): its size is 0.  `run_batch` scores nothing for such a problem and returns
    (None, no inliers, 0), as it does for a problem of fewer than four correspondences."""
    import torch
    dev = _lib.require_gpu()
    P = len(features)
    if P == 0:
        raise ValueError("match_batch: no image pairs")
    ka = [_to_device(f[0], torch.float32, dev, "kpsA").reshape(-1, 2) for f in features]
    da = [_to_device(f[1], torch.uint8, dev, "descA") for f in features]
    kb = [_to_device(f[2], torch.float32, dev, "kpsB").reshape(-1, 2) for f in features]
    db = [_to_device(f[3], torch.uint8, dev, "descB") for f in features]
    widths = set(int(t.shape[1]) for t in da + db if t.dim() == 2)
    if any(t.dim() != 2 for t in da + db) or len(widths) != 1:
        raise ValueError("match_batch: descriptors must be uint8 [rows, nbytes] with one nbytes for every pair")
    for p in range(P):
        if ka[p].shape[0] != da[p].shape[0] or kb[p].shape[0] != db[p].shape[0]:
            raise ValueError("match_batch: pair %d has %d / %d keypoints for %d / %d descriptors"
                             % (p, ka[p].shape[0], kb[p].shape[0], da[p].shape[0], db[p].shape[0]))
    off_a = np.zeros(P + 1, dtype=np.int64)
    off_b = np.zeros(P + 1, dtype=np.int64)
    off_a[1:] = np.cumsum([t.shape[0] for t in da])
    off_b[1:] = np.cumsum([t.shape[0] for t in db])
    if off_a[-1] >= 2 ** 31 or off_b[-1] >= 2 ** 31 or P >= 2 ** 21:
        raise ValueError("match_batch: too many rows or pairs for one submission")
    off_a_dev = torch.from_numpy(off_a).to(dev)
    off_b_dev = torch.from_numpy(off_b).to(dev)
    train, dist = kernels.match_hamming_batched(torch.cat(da), torch.cat(db), off_a_dev.to(torch.int32), off_b_dev.to(torch.int32))
    ka_all, kb_all = torch.cat(ka), torch.cat(kb)
    order, q_local, t_local, p_of, sizes = _ordered_matches(train, dist, off_a_dev, int(off_a[-1]), P)
    if info is not None:
        info["query_idx"], info["train_idx"], info["distance"] = q_local.to(torch.int32), t_local.to(torch.int32), dist[order]
    return _device_problems(ka_all[order], kb_all[off_b_dev[p_of] + t_local], sizes)


def _ordered_matches(train, dist, off_q_dev, total_q, P):
    """The tail both matchers share: the library's per-query records (train, dist: int32 [total_q], -1 for no match; problem p owns
    rows off_q_dev[p] .. off_q_dev[p + 1] - 1, int64 [P + 1] on the device) -> the match lists in the rules' order.  Returns
    (order, q_local, t_local, p_of, sizes): the rows of the records that hold a match, ordered by (problem, distance, i) with ONE
    sort on a packed key; the query and train index inside the problem and the problem of each; matches per problem (numpy; the
    one download)."""
    import torch
    row = torch.arange(total_q, device=train.device)
    prob = torch.searchsorted(off_q_dev[1:].contiguous(), row, right=True)      # the problem of every query row
    local = row - off_q_dev[prob]
    found = train >= 0
    # (problem, distance, i) in one int64: i < 2^31, distance <= 512 < 2^10, problem < 2^21; rows without a match sort last
    key = ((prob << 10) + dist.to(torch.int64).clamp(min=0) << 31) + local
    key = torch.where(found, key, torch.full_like(key, torch.iinfo(torch.int64).max))
    order = torch.sort(key, stable=True).indices
    sizes = torch.bincount(prob[found], minlength=P).cpu().numpy()              # the one download
    order = order[:int(sizes.sum())]
    return order, local[order], train[order].to(torch.int64), prob[order], sizes


def _device_problems(rows_a, rows_b, sizes):
    """The gathered keypoints of the ordered matches -> `DeviceProblems`, with one spare row behind the correspondences: the
    4-point kernel reads row 0 of a problem that has none."""
    import torch
    n = rows_a.shape[0]
    pts_a = torch.zeros((n + 1, 2), dtype=torch.float32, device=rows_a.device)
    pts_b = torch.zeros((n + 1, 2), dtype=torch.float32, device=rows_a.device)
    pts_a[:n] = rows_a
    pts_b[:n] = rows_b
    return DeviceProblems(pts_a[:n], pts_b[:n], sizes)


def match_ratio(ratio, who="match_graph"):
    """`ratio` of the ratio rule -> integers (num, den), 0 < num <= den <= 1024.  A float in (0, 1] is taken as
    Fraction(ratio).limit_denominator(1024), so 0.7 is 7 / 10; a pair of integers (num, den) is taken as it stands.  ValueError for
    anything else.  No GPU is needed."""
    from fractions import Fraction
    top = _lib.RWH_MATCH2_RATIO_MAX
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if isinstance(ratio, (float, np.floating)) and 0.0 < float(ratio) <= 1.0:      # (a NaN fails both comparisons)
        f = Fraction(float(ratio)).limit_denominator(top)
        if f > 0:
            return f.numerator, f.denominator
    elif isinstance(ratio, (tuple, list)) and len(ratio) == 2 and is_int(ratio[0]) and is_int(ratio[1]) and 0 < ratio[0] <= ratio[1] <= top:
        return int(ratio[0]), int(ratio[1])
    raise ValueError("%s: ratio=%r; a float in (0, 1] that is at least 1 / %d, or integers (num, den) with 0 < num <= den <= %d"
                     % (who, ratio, 2 * top, top))


def _check_graph_pairs(pairs, n, who):
    """`match_graph`'s pair list -> int32 [P, 2] of (s, d), both inside 0 .. n - 1; s == d and repeats are allowed here."""
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    try:
        rows = [tuple(pr) for pr in pairs]
    except TypeError:
        rows = None
    if not rows or any(len(pr) != 2 or not is_int(pr[0]) or not is_int(pr[1]) for pr in rows):
        raise ValueError("%s: pairs=%r; a non-empty list of (s, d)" % (who, pairs))
    if any(not (0 <= s < n and 0 <= d < n) for s, d in rows):
        raise ValueError("%s: pairs=%r names an image outside 0 .. %d" % (who, pairs, n - 1))
    if len(rows) >= 2 ** 21:
        raise ValueError("%s: too many pairs for one submission" % who)
    return np.array(rows, dtype=np.int32).reshape(-1, 2)


def match_graph(features, pairs, ratio=0.7, info=None):
    """Hamming matches under Lowe's 2-nearest ratio test for the pairs of a PAIR GRAPH in one GPU submission, handed over as the
    `DeviceProblems` that `run_batch` takes: the matcher in front of `sequence_graph`, where most proposed pairs do not overlap.
    `match_batch`'s cross-check gives nearly every train row a partner, overlap or not, and `sequence_graph`'s
    inliers > 8 + 0.3 matches pays for that ballast; the ratio test leaves the matches that have support.

    features: the list `extract_batch` returns, one (kps float32 [N_k, 2], desc uint8 [N_k, nbytes]) per IMAGE, numpy arrays or
    tensors, one nbytes (1 .. 64) throughout.  pairs: a list of (s, d): image s is the query side, image d the train side, H will
    map s into d; s == d and repeats are allowed.  ratio: a float in (0, 1], taken as Fraction(ratio).limit_denominator(1024) (0.7
    is 7 / 10), or integers (num, den) (`match_ratio`).  ValueError for another ratio or pair list, before the GPU is asked for.

    The ratio rule (include/rwh.h, rwh_match_ratio_graph): D[i, j] = popcount(A[i] xor B[j]); d1[i], j1[i] the nearest train row of
    query i and d2[i] the nearest of the others; i is a candidate iff den d1 < num d2 (integers, strict: a tie for the nearest is
    never a candidate); of the candidates of one train row the one with the smallest d1 survives (lowest i on ties); the matches
    are ordered by (d1, i).  Lowe's ratio test plus a uniqueness step; held to this statement, NOT to OpenCV.

    The descriptors are concatenated ONCE PER IMAGE and every pair reads them in place (`match_batch` copies them per pair).
    Ordering, compaction and the keypoint gather are `match_batch`'s tensor operations, and the one download is the P match counts.
    `info`: optional dict, receives "query_idx", "train_idx" (int32 device tensors, indices inside the pair's images, in the order of
    the correspondences), "distance" and "second" (d1 and d2)."""
    num, den = match_ratio(ratio)
    n = len(features)
    if n == 0:
        raise ValueError("match_graph: no images")
    pr = _check_graph_pairs(pairs, n, "match_graph")
    import torch
    dev = _lib.require_gpu()
    kps = [_to_device(f[0], torch.float32, dev, "kps").reshape(-1, 2) for f in features]
    desc = [_to_device(f[1], torch.uint8, dev, "desc") for f in features]
    if any(t.dim() != 2 for t in desc) or len(set(int(t.shape[1]) for t in desc)) != 1:
        raise ValueError("match_graph: descriptors must be uint8 [rows, nbytes] with one nbytes for every image")
    for k in range(n):
        if kps[k].shape[0] != desc[k].shape[0]:
            raise ValueError("match_graph: image %d has %d keypoints for %d descriptors" % (k, kps[k].shape[0], desc[k].shape[0]))
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([t.shape[0] for t in desc])
    P = pr.shape[0]
    off_q = np.zeros(P + 1, dtype=np.int64)
    off_q[1:] = np.cumsum((off[1:] - off[:-1])[pr[:, 0]])
    if off[-1] >= 2 ** 31 or off_q[-1] >= 2 ** 31:
        raise ValueError("match_graph: too many rows for one submission")
    train, dist, second = kernels.match_ratio_graph(torch.cat(desc), off.astype(np.int32), pr, (num, den))
    order, q_local, t_local, p_of, sizes = _ordered_matches(train, dist, torch.from_numpy(off_q).to(dev), int(off_q[-1]), P)
    kps_all = torch.cat(kps)
    first = torch.from_numpy(off[:-1][pr.astype(np.int64)]).to(dev)            # [P, 2]: the first row of the pair's images
    if info is not None:
        info["query_idx"], info["train_idx"] = q_local.to(torch.int32), t_local.to(torch.int32)
        info["distance"], info["second"] = dist[order], second[order]
    return _device_problems(kps_all[first[p_of, 0] + q_local], kps_all[first[p_of, 1] + t_local], sizes)


def match_descriptors_ratio(descA, descB, ratio=0.7):
    """One pair through `match_graph`'s matcher: descA [Na, nbytes], descB [Nb, nbytes] uint8 (numpy or tensors; query and train
    side) -> (queryIdx, trainIdx, distance, second), int32 numpy arrays ordered by (distance, queryIdx), under the ratio rule stated
    at `match_graph`."""
    import torch
    info = {}
    na, nb = int(descA.shape[0]), int(descB.shape[0])
    match_graph([(torch.zeros((na, 2), dtype=torch.float32), descA), (torch.zeros((nb, 2), dtype=torch.float32), descB)], [(0, 1)],
                ratio=ratio, info=info)
    both = torch.stack([info["query_idx"], info["train_idx"], info["distance"], info["second"]]).cpu().numpy()
    return both[0].copy(), both[1].copy(), both[2].copy(), both[3].copy()


def match_descriptors(descA, descB):
    """One pair through `match_batch`'s matcher: descA [Na, nbytes], descB [Nb, nbytes] uint8 (numpy or tensors; "query" and
    "train" side) -> (queryIdx, trainIdx, distance), int32 numpy arrays ordered by (distance, queryIdx): the fields of
    `sorted(bf.match(descA, descB), key=lambda m: m.distance)` (ransac.py:258-261) under the rule stated at `match_batch`
    (parity with OpenCV not verified)."""
    import torch
    info = {}
    na, nb = int(descA.shape[0]), int(descB.shape[0])
    match_batch([(torch.zeros((na, 2), dtype=torch.float32), descA, torch.zeros((nb, 2), dtype=torch.float32), descB)], info=info)
    both = torch.stack([info["query_idx"], info["train_idx"], info["distance"]]).cpu().numpy()
    return both[0].copy(), both[1].copy(), both[2].copy()


# ---- the feature extractor (include/rwh.h, rwh_orb_detect_batched / rwh_orb_describe_batched): its tables, made on the host ----
ORB_BINS, ORB_BORDER, ORB_TEST_RADIUS = _lib.RWH_ORB_BINS, _lib.RWH_ORB_BORDER, _lib.RWH_ORB_TEST_RADIUS
ORB_PATTERN_SEED = 2011
_ORB_DEFAULT_CAPACITY = 1 << 16


def orb_bin_table():
    """The 30 sector boundaries of the orientation rule: int32 [30, 2], row k = round(2^15 (cos, sin)((k - 1/2) 12 degrees))."""
    a = np.deg2rad((np.arange(ORB_BINS) - 0.5) * (360.0 / ORB_BINS))
    return np.rint(32768.0 * np.stack([np.cos(a), np.sin(a)], axis=1)).astype(np.int32)


ORB_SCALE_ONE, ORB_SCALE_MAX, ORB_LEVELS_MAX = _lib.RWH_ORB_SCALE_ONE, _lib.RWH_ORB_SCALE_MAX, _lib.RWH_ORB_LEVELS_MAX


def _check_scales(scales):
    """Rule 6's table: int32 [n_levels], 1 .. 16 levels, 256 first, strictly increasing, <= 1024."""
    sc = np.asarray(scales)
    if sc.dtype.kind not in "iu" or sc.ndim != 1:
        raise ValueError("orb: scales must be a list of integers in Q8 (256 = the image's own scale), got %s %s" % (sc.dtype, sc.shape))
    if not 1 <= sc.shape[0] <= ORB_LEVELS_MAX:
        raise ValueError("orb: %d levels; the pyramid takes 1 .. %d" % (sc.shape[0], ORB_LEVELS_MAX))
    sc = sc.astype(np.int64)
    if sc[0] != ORB_SCALE_ONE or (np.diff(sc) <= 0).any() or sc[-1] > ORB_SCALE_MAX:
        raise ValueError("orb: scales %s; the table starts at %d, increases strictly and stays <= %d" % (sc.tolist(), ORB_SCALE_ONE, ORB_SCALE_MAX))
    return sc.astype(np.int32)


def orb_scales(n_levels=8, scale=1.2):
    """The scales of a pyramid of n_levels levels (rule 6 of include/rwh.h): int32 [n_levels] in Q8, entry l = rint(256 scale ** l).
    ValueError where n_levels leaves 1 .. 16 or the table leaves 256 .. 1024 or does not increase strictly (scale 1.2 reaches 8
    levels: 256 307 369 442 531 637 764 917)."""
    n_levels = int(n_levels)
    if not 1 <= n_levels <= ORB_LEVELS_MAX:
        raise ValueError("orb: %d levels; the pyramid takes 1 .. %d" % (n_levels, ORB_LEVELS_MAX))
    with np.errstate(over="ignore"):
        t = np.rint(ORB_SCALE_ONE * np.float64(scale) ** np.arange(n_levels))
    if not np.isfinite(t).all() or (np.abs(t) > 2 ** 30).any():
        raise ValueError("orb: scale %r gives a table outside %d .. %d" % (scale, ORB_SCALE_ONE, ORB_SCALE_MAX))
    return _check_scales(t.astype(np.int64))


def orb_level_quotas(n_features, scales):
    """How many keypoints each level may keep (rule 7): int32 [n_levels], q_l = floor(n_features (1 / s_l) / sum_j (1 / s_j)) in exact
    rationals, the remainder added to level 0 -- a share that falls geometrically with the level, as OpenCV's does, stated in
    integers (no parity claimed).  Sums to n_features and never increases with the level."""
    from fractions import Fraction
    sc = _check_scales(scales)
    n_features = int(n_features)
    if n_features < 0:
        raise ValueError("orb: n_features must not be negative")
    total = sum(Fraction(1, int(v)) for v in sc)
    q = [int(n_features * Fraction(1, int(v)) / total) for v in sc]           # int() of a non-negative Fraction is its floor
    q[0] += n_features - sum(q)
    return np.array(q, dtype=np.int32)


def default_pattern(nbytes=32):
    """The default BRIEF test pattern: int8 [8 * nbytes, 4], rows (x1, y1, x2, y2).  The recipe: numpy's legacy
    RandomState(ORB_PATTERN_SEED); per test four draws normal(0, 31 / 5) rounded with rint; a test is rejected (and drawn again)
    when a point lies outside radius 13 or the two points coincide.  The same table on every call, and a shorter pattern is a
    prefix of a longer one.  It is NOT OpenCV's learned ORB pattern; a caller who owns that one passes it as `pattern=`."""
    nbytes = int(nbytes)
    if not 1 <= nbytes <= _lib.RWH_MATCH_MAX_BYTES:
        raise NotImplementedError("orb: descriptors of %d bytes; the extractor takes 1 .. %d" % (nbytes, _lib.RWH_MATCH_MAX_BYTES))
    rng = np.random.RandomState(ORB_PATTERN_SEED)
    out = np.empty((8 * nbytes, 4), dtype=np.int8)
    t = 0
    while t < out.shape[0]:
        x1, y1, x2, y2 = (int(v) for v in np.rint(rng.normal(0.0, 31.0 / 5.0, 4)))
        if x1 * x1 + y1 * y1 > ORB_TEST_RADIUS ** 2 or x2 * x2 + y2 * y2 > ORB_TEST_RADIUS ** 2 or (x1, y1) == (x2, y2):
            continue
        out[t] = (x1, y1, x2, y2)
        t += 1
    return out


def _check_pattern(pattern, nbytes):
    pat = np.asarray(pattern)
    if pat.dtype.kind not in "iu" or pat.ndim != 2 or pat.shape[1] != 4 or pat.shape[0] == 0 or pat.shape[0] % 8:
        raise ValueError("orb: pattern must be an integer [8 * nbytes, 4] table of (x1, y1, x2, y2), got %s %s" % (pat.dtype, pat.shape))
    if nbytes is not None and pat.shape[0] != 8 * int(nbytes):
        raise ValueError("orb: pattern has %d tests, nbytes = %d needs %d" % (pat.shape[0], nbytes, 8 * int(nbytes)))
    if pat.shape[0] // 8 > _lib.RWH_MATCH_MAX_BYTES:
        raise NotImplementedError("orb: descriptors of %d bytes; the extractor takes 1 .. %d" % (pat.shape[0] // 8, _lib.RWH_MATCH_MAX_BYTES))
    p = pat.astype(np.int64)
    if ((p[:, 0] ** 2 + p[:, 1] ** 2 > ORB_TEST_RADIUS ** 2) | (p[:, 2] ** 2 + p[:, 3] ** 2 > ORB_TEST_RADIUS ** 2)).any():
        raise ValueError("orb: a pattern point lies outside radius %d" % ORB_TEST_RADIUS)
    return p


def rotate_pattern(pattern):
    """The 30 steered copies of a test pattern: int8 [30, nbits, 4], copy k = every point rotated by k 12 degrees in float64,
    (x cos - y sin, x sin + y cos), and rounded with rint; a point within radius 13 keeps every coordinate within +-13."""
    p = _check_pattern(pattern, None).astype(np.float64)
    a = np.deg2rad(np.arange(ORB_BINS) * (360.0 / ORB_BINS))[:, None]
    c, s = np.cos(a), np.sin(a)
    out = np.empty((ORB_BINS, p.shape[0], 4), dtype=np.float64)
    for o in (0, 2):
        out[:, :, o] = p[None, :, o] * c - p[None, :, o + 1] * s
        out[:, :, o + 1] = p[None, :, o] * s + p[None, :, o + 1] * c
    out = np.rint(out)
    assert np.abs(out).max() <= ORB_TEST_RADIUS
    return out.astype(np.int8)


def orb_layout(shapes, scales):
    """The buffer and the table of one extraction, on the host: what rwh_orb_pyramid_batched, rwh_orb_detect_batched and
    rwh_orb_describe_batched are handed.  shapes: the images' (h, w, c); scales: the checked Q8 table of rule 6.  Returns
    (table, planes_offset, images_bytes, gray_bytes, full): table int64 [n * n_levels, 5], row i * n_levels + l = (byte offset of
    the pixels, byte offset of the gray plane, h, w, c) of level l of image i -- level 0 the image itself, level l >= 1 its plane
    of (256 h + s // 2) // s by (256 w + s // 2) // s pixels, one channel, and (0, 0, 0, 0, 1) for a level without pixels; the
    images lie back to back in [0, planes_offset), the planes behind them in (image, level) order up to images_bytes (equal to
    planes_offset with one level); gray_bytes holds every row's gray plane; full is the largest number of keypoints one row can
    hold (no two are neighbours, and level 0 is an image's largest)."""
    sc = [int(s) for s in scales]
    planes_offset = sum(h * w * c for h, w, c in shapes)
    table, src_off, plane_off, gray_off, full = [], 0, planes_offset, 0, 1
    for h, w, c in shapes:
        full = max(full, ((max(w - 2 * ORB_BORDER, 0) + 1) // 2) * ((max(h - 2 * ORB_BORDER, 0) + 1) // 2))
        table.append((src_off, gray_off, h, w, c))
        src_off += h * w * c
        gray_off += h * w
        for s in sc[1:]:
            hl, wl = (256 * h + s // 2) // s, (256 * w + s // 2) // s
            if hl == 0 or wl == 0:
                table.append((0, 0, 0, 0, 1))
                continue
            table.append((plane_off, gray_off, hl, wl, 1))
            plane_off += hl * wl
            gray_off += hl * wl
    return np.array(table, dtype=np.int64).reshape(-1, 5), planes_offset, plane_off, gray_off, full


def _orb_image(img, dev, i):
    """numpy array or tensor -> (flat uint8 tensor on the GPU, h, w, c); uint8 [h, w], [h, w, 3] or [h, w, 4] only."""
    import torch
    t = img if isinstance(img, torch.Tensor) else (torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else None)
    if t is None:
        raise TypeError("extract_batch: image %d is a %s; numpy arrays and tensors are taken" % (i, type(img).__name__))
    if t.dtype != torch.uint8:
        raise TypeError("extract_batch: image %d is %s; the extractor takes uint8" % (i, t.dtype))
    if t.dim() == 2:
        c = 1
    elif t.dim() == 3 and t.shape[2] in (3, 4):
        c = int(t.shape[2])
    else:
        raise ValueError("extract_batch: image %d has shape %s; [h, w], [h, w, 3] or [h, w, 4]" % (i, tuple(t.shape)))
    h, w = int(t.shape[0]), int(t.shape[1])
    if not (1 <= h <= 65536 and 1 <= w <= 65536):
        raise ValueError("extract_batch: image %d is %d x %d; sides of 1 .. 65536" % (i, h, w))
    return t.to(dev).contiguous().reshape(-1), h, w, c


def _orb_level_to_image(xy, s):
    """Rule 8: pixel coordinates on a level of scale s (Q8) -> float32 coordinates in the image, the centre of the pixel's footprint,
    ((2 x + 1) s - 256) / 512.  xy: tensor of whole numbers, s: float64 tensor that broadcasts against it.  Every step is exact in
    float64 (the numerator is an integer below 2^27), so the one rounding is the conversion to float32."""
    import torch
    return (((2.0 * xy.to(torch.float64) + 1.0) * s - 256.0) / 512.0).to(torch.float32)


def extract_batch(images, n_features=500, threshold=20, nbytes=32, pattern=None, info=None, n_levels=1, scale=1.2, scales=None,
                  quotas=None):
    """Keypoints and binary descriptors of MANY images in one GPU submission: the stage of ransac.py:252-257
    (cvtColor(RGB2GRAY) + ORB_create().detectAndCompute) in front of `match_batch`, by the rule stated in include/rwh.h --
    FAST-9 corners with 3 x 3 non-maximum suppression, ordered by (score descending, y, x) and cut at n_features;
    intensity-centroid orientation in 30 bins of 12 degrees; BRIEF steered by the bin, 5 x 5 box tests; on ONE scale by default, on
    the levels of a scale pyramid with n_levels > 1.  It follows the ORB paper (Rublee et al. 2011), NOT OpenCV's code: not its
    pyramid's resampling, no Harris ranking, not OpenCV's learned pattern, no sub-pixel refinement; parity with OpenCV's ORB is
    neither claimed nor verified.  Everything is an integer: results are exact and a rerun is identical.

    images: list of uint8 numpy arrays or tensors, [h, w, 3] RGB, [h, w, 4] RGBA (alpha ignored) or [h, w] gray; shapes may differ.
    threshold: 0 .. 254; nbytes: 1 .. 64; pattern: an integer [8 * nbytes, 4] table of tests (x1, y1, x2, y2) within radius 13
    (default: `default_pattern(nbytes)`).  Returns a list of (kps float32 [N, 2] as (x, y), desc uint8 [N, nbytes]) device tensors,
    N <= n_features, ready to be paired into `match_batch`'s `features`.  `info`: optional dict, receives "score" and "bin" (lists
    of int32 device tensors), "counts" (keypoints kept per image) and "found" (before the cut), "level" (int32) and "size"
    (float32, the patch's side in image pixels: 31 on level 0) as lists of device tensors, and "found_levels" (per image, the
    keypoints found on each level before its quota; "found" is their sum).

    The pyramid (rules 6 - 8 of include/rwh.h; ORB paper, section 6.1).  n_levels: 1 .. 16; level l is the image's gray plane
    shrunk by scales[l] / 256 -- an exact area average made from level 0 -- and is searched and described as an image of its own.
    scales: int32 [n_levels] in Q8 (default `orb_scales(n_levels, scale)`: rint(256 scale ** l)); quotas: how many keypoints each
    level keeps (default `orb_level_quotas(n_features, scales)`; a level's shortfall is not handed to another).  An image's
    keypoints are its levels' in level order, each at the image's own coordinates: the centre of its footprint,
    ((2 x + 1) s - 256) / 512.  One level (the default) is the pyramid of the image alone, through the same body; there that map
    is the identity, so its results are handed out as slices of the describe call's rows (the gather costs a one-image call
    170 us of 1060: profiles/extract_refactor.txt).

    Every level is a row of `orb_layout`'s table, row i * n_levels + l = level l of image i, and detect, the sort of the keys and
    describe run ONCE over the n_images * n_levels rows: three library launches (detect, describe and their setup).  More than one
    level: two more in front (the level planes of the whole batch, written behind the images in the same buffer, and their setup).
    The one download is the per-row keypoint counts."""
    import torch
    dev = _lib.require_gpu()
    n = len(images)
    if n == 0:
        raise ValueError("extract_batch: no images")
    n_features, threshold = int(n_features), int(threshold)
    if n_features < 1:
        raise ValueError("extract_batch: n_features must be positive")
    if not 0 <= threshold <= 254:
        raise ValueError("extract_batch: threshold %d outside 0 .. 254" % threshold)
    sc = orb_scales(n_levels, scale) if scales is None else _check_scales(scales)
    levels = int(sc.shape[0])
    if scales is not None and int(n_levels) not in (1, levels):
        raise ValueError("extract_batch: n_levels = %d but %d scales" % (int(n_levels), levels))
    if quotas is None:
        qt = orb_level_quotas(n_features, sc)
    else:
        qt = np.asarray(quotas)
        if qt.dtype.kind not in "iu" or qt.shape != (levels,) or (qt.astype(np.int64) < 0).any() or (qt.astype(np.int64) >= 2 ** 31).any():
            raise ValueError("extract_batch: quotas must be %d non-negative integers, one per level" % levels)
        qt = qt.astype(np.int32)
    pat = default_pattern(nbytes) if pattern is None else _check_pattern(pattern, nbytes)
    if levels == 1 and qt[0] < 1:
        raise ValueError("extract_batch: the quota of the only level must be positive")
    nf = max(int(qt.max()), 1)
    packed = [_orb_image(img, dev, i) for i, img in enumerate(images)]
    flat, shapes = [p[0] for p in packed], [p[1:] for p in packed]
    if n * levels * nf >= 2 ** 31:
        raise ValueError("extract_batch: too many images x n_features for one submission" if levels == 1 else
                         "extract_batch: too many images x levels x quota for one submission")
    rot = torch.from_numpy(rotate_pattern(pat)).to(dev)
    bins_t = torch.from_numpy(orb_bin_table()).to(dev)
    table, planes_offset, images_bytes, gray_bytes, full = orb_layout(shapes, sc)
    table_dev = torch.from_numpy(table).to(dev)
    if levels > 1:
        src = torch.cat(flat + [torch.empty((images_bytes - planes_offset,), dtype=torch.uint8, device=dev)])
        kernels.orb_pyramid_batched(src, planes_offset, table_dev, sc)
    else:
        src = torch.cat(flat)
    capacity = min(full, _ORB_DEFAULT_CAPACITY)
    gray, keys, counts = kernels.orb_detect_batched(src, table_dev, gray_bytes, threshold, capacity)
    found = counts.cpu().numpy()                                               # the one download
    if (found > capacity).any():                 # more keypoints than the usual room: once more with room for every one there can be
        gray, keys, counts = kernels.orb_detect_batched(src, table_dev, gray_bytes, threshold, full)
    keys = torch.sort(keys, dim=1).values
    quota_rows = np.tile(qt, n)
    if (qt < nf).any():                          # rule 7: a level's quota below the row length nf, which the describe call cuts at itself
        counts = torch.minimum(counts, torch.from_numpy(quota_rows).to(dev))
    kps, desc, score, bins = kernels.orb_describe_batched(gray, gray_bytes, table_dev, keys, counts, nf, bins_t, rot)
    kept = np.minimum(found, quota_rows)
    per_image = [int(v) for v in kept.reshape(n, levels).sum(axis=1)]
    patch = float(2 * _lib.RWH_ORB_PATCH_RADIUS + 1)
    if info is not None:
        info["counts"] = per_image
        info["found_levels"] = [[int(v) for v in r] for r in found.reshape(n, levels)]
        info["found"] = [sum(r) for r in info["found_levels"]]
    if levels == 1:                              # rule 8 at scale 256 is the identity and a row is an image: slices, no gather
        if info is not None:
            info["score"], info["bin"] = [score[i, :kept[i]] for i in range(n)], [bins[i, :kept[i]] for i in range(n)]
            info["level"] = [torch.zeros((k,), dtype=torch.int32, device=dev) for k in per_image]
            info["size"] = [torch.full((k,), patch, dtype=torch.float32, device=dev) for k in per_image]
        return [(kps[i, :kept[i]], desc[i, :kept[i]]) for i in range(n)]
    # rule 8: one gather of the kept slots of every row, in row order = (image, level); the map to the image's own coordinates
    rows = np.repeat(np.arange(n * levels), kept)
    slots = np.arange(int(kept.sum())) - np.repeat(np.cumsum(kept) - kept, kept)
    pick = torch.from_numpy(rows.astype(np.int64) * nf + slots).to(dev)
    s_of = torch.from_numpy(np.tile(sc, n)[rows].astype(np.float64)).to(dev)
    xy = _orb_level_to_image(kps.reshape(-1, 2).index_select(0, pick), s_of[:, None])
    split = lambda t: list(torch.split(t, per_image))
    if info is not None:
        info["score"], info["bin"] = split(score.reshape(-1).index_select(0, pick)), split(bins.reshape(-1).index_select(0, pick))
        info["level"] = split(torch.from_numpy((rows % levels).astype(np.int32)).to(dev))
        info["size"] = split((s_of * patch / 256.0).to(torch.float32))
    return list(zip(split(xy), split(desc.reshape(-1, desc.shape[2]).index_select(0, pick))))


def detect_and_describe(img, n_features=500, threshold=20, nbytes=32, pattern=None, n_levels=1, scale=1.2, scales=None, quotas=None):
    """One image through `extract_batch`, numpy in and out: (kps float32 [N, 2] as (x, y), desc uint8 [N, nbytes]) -- what stands
    for `ORB_create().detectAndCompute` (ransac.py:254-257) under the rule stated at `extract_batch` (not OpenCV's ORB)."""
    (kps, desc), = extract_batch([img], n_features=n_features, threshold=threshold, nbytes=nbytes, pattern=pattern, n_levels=n_levels,
                                 scale=scale, scales=scales, quotas=quotas)
    return kps.cpu().numpy(), desc.cpu().numpy()
