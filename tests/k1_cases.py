"""Problems and the exact reference for K1 (`dlt4_kernel`, ransac_with_homography_amd/csrc/rwh_ransac.hip) -- numpy and the standard
library only, so the CPU suite (test_k1_cpu.py) and the GPU suite (test_k1_gpu.py) share one statement of everything:

  exact_h            the null vector of the float32 8 x 9 DLT matrix in rational arithmetic, rounded the way the kernel and the
                     reference round theirs;
  FAMILIES           seven deterministic problems (M <= 256 correspondences, 256 samples each);
  edge_table         hand-built samples with the flag byte each must get, derived from the kernel's rules and not from any output;
  k2i_box            the perturbation box of rwh_score_interval (include/rwh.h) -- its one statement in the tests;
  borderline         the rows on which a last-bit difference of a float64 intermediate may legitimately change a flag, defined
                     from the emulation's intermediates (tests/k1_emulation.py, return_ratios=True) alone;
  EMULATION_BIT_EQUAL  per family, the share of the emulation's unflagged / ILLCOND rows whose float32 H equals the exact one bit
                     for bit (measured on the CPU, asserted current by test_k1_cpu.py): what the kernel is measured against."""
import decimal
import functools
import os
from fractions import Fraction

import numpy as np

import k1_emulation as k1e

REPEATED, SINGULAR, ILLCOND, DEGENERATE = k1e.RWH_HYP_REPEATED, k1e.RWH_HYP_SINGULAR, k1e.RWH_HYP_ILLCOND, k1e.RWH_HYP_DEGENERATE
HOST_BITS = REPEATED | SINGULAR | DEGENERATE          # rows the settle rule always hands to the host: no box is claimed for them
N_SAMPLES = 256
INT32_MAX = 2 ** 31 - 1

_CTX = decimal.Context(prec=80)


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact reference
# ---------------------------------------------------------------------------------------------------------------------------------
def dlt_matrix32(pa, pb, idx4):
    """The float32 8 x 9 matrix of one sample, as the reference builds it (homography.py:4-14): the four products per pair are
    rounded to float32.  Rows [-x -y -1 0 0 0 x*x' y*x' x'] and [0 0 0 -x -y -1 x*y' y*y' y']."""
    A = np.asarray(pa, np.float32)[np.asarray(idx4)]
    B = np.asarray(pb, np.float32)[np.asarray(idx4)]
    x, y, xp, yp = A[:, 0], A[:, 1], B[:, 0], B[:, 1]
    m = np.zeros((8, 9), np.float32)
    with np.errstate(all="ignore"):
        m[0::2, 0], m[0::2, 1], m[0::2, 2] = -x, -y, -1
        m[0::2, 6], m[0::2, 7], m[0::2, 8] = x * xp, y * xp, xp
        m[1::2, 3], m[1::2, 4], m[1::2, 5] = -x, -y, -1
        m[1::2, 6], m[1::2, 7], m[1::2, 8] = x * yp, y * yp, yp
    return m


def exact_null_vector(mat32):
    """The null vector of a float32 8 x 9 matrix as nine Fractions (Gauss-Jordan elimination over the rationals, the free
    component set to 1), or None when the rank is below 8 or an entry is not finite."""
    if not np.isfinite(mat32).all():
        return None
    rows = [[Fraction(float(v)) for v in r] for r in mat32]
    pivots = []
    r = 0
    for c in range(9):
        p = next((i for i in range(r, 8) if rows[i][c] != 0), None)
        if p is None:
            continue
        rows[r], rows[p] = rows[p], rows[r]
        inv = 1 / rows[r][c]
        rows[r] = [v * inv for v in rows[r]]
        for i in range(8):
            if i != r and rows[i][c] != 0:
                f = rows[i][c]
                rows[i] = [a - f * b for a, b in zip(rows[i], rows[r])]
        pivots.append(c)
        r += 1
        if r == 8:
            break
    if r < 8:
        return None
    free = next(c for c in range(9) if c not in pivots)
    h = [Fraction(0)] * 9
    h[free] = Fraction(1)
    for i, c in enumerate(pivots):
        h[c] = -rows[i][free]
    return h


def _round_f32(q):
    """The float32 nearest to the Fraction q (an exact comparison among the candidates: no double rounding)."""
    c = np.float32(float(q))
    if not np.isfinite(c):
        return c
    cands = [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    return min(cands, key=lambda v: abs(Fraction(float(v)) - q) if np.isfinite(v) else Fraction(10) ** 60)


def exact_h(pa, pb, idx4):
    """float32 [9]: the exact null vector of the sample's float32 DLT matrix, scaled to unit 2-norm (80 significant digits), each
    component rounded to float32 and then divided by the 9th in float32 -- the roundings the kernel and the reference apply to
    their float64 vectors.  None when the matrix has rational rank below 8 (or a non-finite entry)."""
    h = exact_null_vector(dlt_matrix32(pa, pb, idx4))
    if h is None:
        return None
    ss = sum(v * v for v in h)
    norm = _CTX.sqrt(_CTX.divide(decimal.Decimal(ss.numerator), decimal.Decimal(ss.denominator)))
    n = np.zeros(9, np.float32)
    for i, v in enumerate(h):
        d = _CTX.divide(_CTX.divide(decimal.Decimal(v.numerator), decimal.Decimal(v.denominator)), norm)
        n[i] = _round_f32(Fraction(d))
    with np.errstate(all="ignore"):
        return n / n[8]


def residual_is_zero(pa, pb, idx4):
    """M h == 0 exactly, in rationals, for the vector exact_null_vector returns (the reference checked on its own terms)."""
    m = dlt_matrix32(pa, pb, idx4)
    h = exact_null_vector(m)
    return h is not None and any(v != 0 for v in h) and all(sum(Fraction(float(a)) * b for a, b in zip(r, h)) == 0 for r in m)


# ---------------------------------------------------------------------------------------------------------------------------------
# the box (rwh_score_interval) and the borderline rows
# ---------------------------------------------------------------------------------------------------------------------------------
def k2i_box(h, illcond, C, delta0, delta1):
    """The perturbation box of rwh_score_interval (include/rwh.h), plainly in float64: entry i may move by delta x max(|h_i|, its
    natural scale) -- s, s, s C / s, s, s C / s / C, s / C, s, with s the largest scale-free entry and C = coord_scale."""
    a = np.abs(np.asarray(h, np.float64))
    s = max(a[0], a[1], a[3], a[4], a[8], max(a[2], a[5]) / C, max(a[6], a[7]) * C)
    nat = np.array([s, s, s * C, s, s, s * C, s / C, s / C, s])
    return (delta1 if illcond else delta0) * np.maximum(a, nat)


def coord_scale(pa):
    """coord_scale as the settle step passes it: the largest source coordinate, at least 1."""
    return max(1.0, float(np.abs(np.asarray(pa, np.float64)).max()))


def box_fraction(h_exact, h, flag, C, delta0, delta1):
    """max_i |h_exact_i - h_i| / box_i of the box around h for h's flag class: <= 1 means inside."""
    D = k2i_box(h, bool(flag & ILLCOND), C, delta0, delta1)
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(np.asarray(h_exact, np.float64) - np.asarray(h, np.float64)) / D))


def _near(v, t, rel):
    return (v > t * (1 - rel)) & (v < t * (1 + rel))


def borderline(inter, near_singular=True):
    """bool [K] from the emulation's intermediates (k1e.dlt4(..., return_ratios=True)): a pivot ratio within a factor 1 +- 1e-3 of
    1e-3 or 1e-7, ss within that factor of 1e14, a pivot near-tie (the second candidate within 1e-9 relative of the first and not
    exactly equal), and -- for launches that flag nearly singular H -- a determinant ratio within a factor 2 of 1e-6 (it is taken
    from the float32 H, where one ulp moves it by percent)."""
    with np.errstate(all="ignore"):
        r = inter["ratios"]
        b = (_near(r, 1e-3, 1e-3) | _near(r, 1e-7, 1e-3)).any(axis=1) | _near(inter["ss"], 1e14, 1e-3)
        f, s = inter["piv_first"], inter["piv_second"]
        b |= ((s != f) & (s >= f * (1 - 1e-9))).any(axis=1)
        if near_singular:
            d = inter["det_ratio"]
            b |= (d > 0.5e-6) & (d < 2e-6)
    return b


def repeated_rule(idx, m):
    """REPEATED as the integer rule states it (include/rwh.h): an index outside [0, m) counts as 0 and raises the flag; then any
    two equal indices raise it."""
    idx = np.asarray(idx, np.int64)
    bad = (idx < 0) | (idx >= m)
    z = np.where(bad, 0, idx)
    rep = np.zeros(len(idx), bool)
    for i in range(4):
        for j in range(i + 1, 4):
            rep |= z[:, i] == z[:, j]
    return rep | bad.any(axis=1)


def clamp_idx(idx, m):
    idx = np.asarray(idx, np.int64)
    return np.where((idx < 0) | (idx >= m), 0, idx).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# problem families
# ---------------------------------------------------------------------------------------------------------------------------------
_HS = np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]])
_HSMALL = np.array([[0.9, 0.05, 0.1], [-0.03, 1.1, 0.05], [0.02, -0.01, 1.0]])

FAMILIES = ("uniform", "cloud", "two_clusters", "lattice", "uniform_x100", "below2", "matchespoints")
_SEED = {n: 9100 + i for i, n in enumerate(FAMILIES)}


def _targets(G, Hm, noise, rng, outliers):
    """Targets of the source points G under Hm, with Gaussian noise and a share of gross outliers anywhere in 0..1000."""
    P = np.c_[G, np.ones(len(G))] @ Hm.T
    B = P[:, :2] / P[:, 2:3] + rng.normal(0, noise, (len(G), 2))
    o = rng.random(len(G)) < outliers
    B[o] = rng.uniform(0, 1000, (int(o.sum()), 2)) * (B.max() / 1000.0 if B.max() < 10 else 1.0)
    return B


@functools.lru_cache(maxsize=None)
def family(name):
    """-> (pa float32 [M, 2], pb float32 [M, 2], idx int32 [256, 4]); samples drawn with replacement like the reference draws.

    The dense cloud, the clusters and the lattice carry exact targets (float32 rounding is their only noise) and ~3 % gross outliers,
    and the golden matches are sampled among the consensus set of the golden run: on noisy targets the hypotheses of such problems
    spread their determinant ratio evenly over 1e-12 .. 1e-2 and 5-10 % of them land within a factor 2 of the 1e-6 threshold, where
    nothing can be asserted (test_k1_cpu.py caps the borderline rows at 2 %).  This way the ratio is bimodal -- ~1 without an outlier
    in the sample, anything with one -- and both sides of the threshold stay populated."""
    rng = np.random.default_rng(_SEED[name])
    M = 256
    pool = None
    if name == "matchespoints":
        here = os.path.dirname(os.path.abspath(__file__))
        z = np.load(os.path.join(here, "golden", "matchespoints.npz"), allow_pickle=False)
        A, B = z["ptsA"].astype(np.float32), z["ptsB"].astype(np.float32)
        pool = np.load(os.path.join(here, "golden", "g2_hyp_seed0.npz"), allow_pickle=False)["winner_inliers"].astype(np.int64)
    elif name in ("uniform", "uniform_x100"):
        rng = np.random.default_rng(_SEED["uniform"])
        G = rng.uniform(0, 1000, (M, 2))
        B = _targets(G, _HS, 1.0, rng, 0.3)
        s = 100.0 if name == "uniform_x100" else 1.0
        A, B = (G * s).astype(np.float32), (B * s).astype(np.float32)
    elif name == "below2":
        G = rng.uniform(0, 1.99, (M, 2))
        A, B = G.astype(np.float32), _targets(G, _HSMALL, 0.002, rng, 0.3).astype(np.float32)
    else:
        if name == "cloud":
            G = rng.normal(500, 3, (M, 2))
        elif name == "two_clusters":
            G = np.array([[400., 450.], [620., 560.]])[rng.integers(0, 2, M)] + rng.normal(0, 5, (M, 2))
        else:
            G = np.stack([rng.integers(0, 16, M) * 37.0, rng.integers(0, 16, M) * 53.0], 1)
        A, B = G.astype(np.float32), _targets(G, _HS, 0.0, rng, 0.03).astype(np.float32)
    A.setflags(write=False); B.setflags(write=False)
    idx = np.random.default_rng(_SEED[name] + 50).integers(0, A.shape[0] if pool is None else len(pool), (N_SAMPLES, 4))
    idx = (idx if pool is None else pool[idx]).astype(np.int32)
    idx.setflags(write=False)
    return A, B, idx


@functools.lru_cache(maxsize=None)
def family_exact(name):
    """The exact H of every sample of a family (None where rank < 8), computed once per process."""
    A, B, idx = family(name)
    return tuple(exact_h(A, B, r) for r in idx)


@functools.lru_cache(maxsize=None)
def family_emulation(name, near_singular=False):
    A, B, idx = family(name)
    return k1e.dlt4(A, B, idx, near_singular=near_singular, return_ratios=True)


def launch_edge_table():
    """The uniform family's points with 1024 samples (its own 256 first): the reference launch of the launch-edge test."""
    A, B, idx = family("uniform")
    more = np.random.default_rng(_SEED["uniform"] + 51).integers(0, A.shape[0], (1024 - N_SAMPLES, 4)).astype(np.int32)
    return A, B, np.concatenate([idx, more])


# measured on the CPU (test_k1_cpu.py asserts it is current): per family, (rows of the emulation without REPEATED / SINGULAR /
# DEGENERATE whose float32 H is bit-identical to exact_h's, those rows).  The exact-target families sit lower: their hypotheses are
# close to one H whose entries 5.0 and 7.0 put many unit-vector components near float32 rounding boundaries.
EMULATION_BIT_EQUAL = {
    "uniform": (253, 253),
    "cloud": (228, 251),
    "two_clusters": (247, 252),
    "lattice": (233, 237),
    "uniform_x100": (249, 249),
    "below2": (251, 251),
    "matchespoints": (243, 243),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# the edge table
# ---------------------------------------------------------------------------------------------------------------------------------
def edge_table():
    """-> (pa, pb float32 [14, 2], rows): rows = [(name, idx4, expected flag byte, twin idx4 or None)]; a row with a twin must have the
    twin's H bit for bit.  The flag bytes follow from the kernel's stated rules (include/rwh.h, dlt4_kernel), not from an output:

      clean        a plain quadrilateral, every pivot ratio 0.3 .. 1: no flag.
      repeated     index 5 twice.  Point 5 has the largest |x| of the sample, 512: it is the first pivot, 1 / 512 is exact, the
                   factor of its twin row is exactly 1 and the twin row becomes exactly zero; it ends as the row of the 2 x 2
                   system: 0 * (1 / 0) = NaN everywhere -> REPEATED | SINGULAR | ILLCOND | DEGENERATE.
      bad_*        an index outside [0, m) counts as 0 and raises REPEATED, nothing else: H and the other bits are those of the
                   row with 0 in its place, (0, 1, 2, 3) in some order: clean.
      two_bad      both become 0: the flags and H of (0, 2, 0, 3), which repeats 0 itself.
      same_coords  points 1 and 6 are equal in both images at different indices: the matrix has rank 7, the elimination leaves a
                   rounding residue (400.25 * (1 / 400.25) != 1) for the 2 x 2 system, ~1e-16 of its scale: below 1e-7 -> ILLCOND |
                   DEGENERATE; finite, so no SINGULAR; the indices differ, so no REPEATED.
      collinear    three lattice points on y = 53 / 37 x and a fourth elsewhere: no homography maps them onto three targets in
                   general position, the last pivot of the 2 x 2 system is rounding residue -> ILLCOND | DEGENERATE.
      nan / inf    a NaN source coordinate / an infinite target coordinate: NaN reaches ss and every entry of H (inf * 0, inf - inf)
                   -> SINGULAR | ILLCOND | DEGENERATE.
      illcond      four source points within 0.003 px of one line 300 px long: the third pivot of the shared block (the column of
                   ones) is 1.4e-5 of its scale by construction -- a factor 70 from 1e-3 and 140 from 1e-7, test_k1_cpu.py checks
                   it with the emulation's ratios -- the others are 0.2 .. 1 -> ILLCOND alone."""
    A = [(100.5, 200.25), (400.25, 150.5), (350.75, 420.5), (120.25, 380.75), (250.5, 60.25), (512.0, 300.5), (400.25, 150.5),
         (np.nan, 10.5), (200.5, 300.25), (37.0, 53.0), (111.0, 159.0), (259.0, 371.0)]
    B = [(110.75, 215.5), (415.5, 160.25), (372.25, 440.75), (131.5, 401.25), (262.75, 71.5), (530.25, 310.75), (415.5, 160.25),
         (20.5, 30.25), (np.inf, 5.0), (45.5, 66.25), (120.25, 170.5), (280.75, 390.25)]
    p0, p1 = np.array(A[0]), np.array(A[1])
    d = p1 - p0
    nrm = np.array([-d[1], d[0]]) / np.hypot(d[0], d[1])
    A += [tuple(p0 + 0.37 * d + 0.003 * nrm), tuple(p0 + 0.71 * d - 0.0018 * nrm)]
    B += [(230.5, 190.25), (322.25, 175.5)]
    pa, pb = np.array(A, np.float32), np.array(B, np.float32)
    m = len(pa)
    ALL = SINGULAR | ILLCOND | DEGENERATE
    rows = [("clean", (0, 1, 2, 3), 0, None),
            ("repeated", (5, 5, 1, 2), REPEATED | ALL, None),
            ("bad_minus_one", (-1, 1, 2, 3), REPEATED, (0, 1, 2, 3)),
            ("bad_m", (1, m, 2, 3), REPEATED, (1, 0, 2, 3)),
            ("bad_int32_max", (1, 2, 3, INT32_MAX), REPEATED, (1, 2, 3, 0)),
            ("two_bad", (m, 2, -1, 3), None, (0, 2, 0, 3)),
            ("same_coords", (1, 6, 2, 3), ILLCOND | DEGENERATE, None),
            ("collinear", (9, 10, 11, 3), ILLCOND | DEGENERATE, None),
            ("nan", (7, 1, 2, 3), ALL, None),
            ("inf", (1, 2, 8, 3), ALL, None),
            ("illcond", (0, 1, 12, 13), ILLCOND, None)]
    return pa, pb, rows


def edge_launch(rows):
    """The edge table as one index table: every row, then every twin.  -> (idx int32 [n, 4], {row number: its twin's row number})."""
    idx = [r[1] for r in rows]
    twins = {}
    for i, r in enumerate(rows):
        if r[3] is not None:
            twins[i] = len(idx)
            idx.append(r[3])
    return np.array(idx, np.int64).astype(np.int32), twins


def check_edge_rows(rows, twins, H, flags):
    """The assertions of the edge table on one implementation's output (H float32 [n, 9], flags uint8 [n])."""
    for i, (name, _, expect, twin) in enumerate(rows):
        if expect is not None:
            assert int(flags[i]) == expect, (name, int(flags[i]), expect)
        if twin is not None:
            t = twins[i]
            assert int(flags[i]) == int(flags[t]) | REPEATED, (name, int(flags[i]), int(flags[t]))
            assert np.array_equal(H[i].view(np.uint32), H[t].view(np.uint32)), (name, H[i], H[t])
