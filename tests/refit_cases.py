"""Shared by tests/test_refit_cpu.py and tests/test_refit_gpu.py: the inputs of the device-refit tests and their yardstick.

Yardstick: for a problem's inlier subset, A and b of the reference's least-squares problem (calc_correspLinearCollective) are
built in float64 and solved by numpy.linalg.lstsq -> H_ls.  The DEVIATION of a matrix H is the largest distance in pixels, over
ALL of the problem's correspondences, between H (x, y, 1) and H_ls (x, y, 1), both dehomogenised, in float64.  A refit passes
when its deviation is no larger than that of the project's calcHomographyLinear(u, v, True) on the same subset -- the
reference's float32 normal equations, pinned by the golden fixtures.  tests/stream_contract_cases.py still measures with it.

That yardstick is orders of magnitude looser than the float64 refit, and its centre H_ls is less accurate than the refit itself, so
the refit tests hold a result to two tighter conditions around the EXACT fit H_x = exact_fit(u, v, bits) -- the same least-squares
problem solved in rational arithmetic on the float32 inputs, only the eight results rounded:
  (A, resolution)  deviation(H, H_x) <= resolution / 16, for n >= 5 inliers, where resolution = the smallest deviation from H_x of
                   the lstsq fit of the subset with ONE inlier left out.  A fit that lost an inlier lies at least `resolution` from
                   H_x, so any bar below half of that tells it apart; 16 leaves room for lstsq's own error inside `resolution`
                   (each case first asserts deviation(H_ls, H_x) <= resolution / 16, so that the scale can be trusted).
  (B, precision)   deviation(H, H_x) <= deviation(H_ls, H_x): no further from the exact fit than numpy's float64 lstsq.
PROBLEMS and FAMILIES are the shapes and masks that end the kernel's 256-stride loop on every side of a trip and single out a
wave, a lane, the top bit of every mask word and the first and last correspondences."""
import ctypes
import fractions
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, FEW, SINGULAR = 0, 1, 2
SYNTHETIC_SIZES = (4, 5, 63, 64, 65, 185, 1000)


def matchespoints():
    z = np.load(os.path.join(ROOT, "tests", "golden", "matchespoints.npz"))
    return np.ascontiguousarray(z["ptsA"], dtype=np.float32), np.ascontiguousarray(z["ptsB"], dtype=np.float32)


def synthetic(m, seed=1234):
    """m correspondences of a 1920 x 1080 frame under a mild projective H, 1 px Gaussian noise on the targets."""
    rng = np.random.default_rng([seed, m])
    H = np.array([[1.03, 0.02, 40.0], [-0.015, 0.98, 25.0], [2e-5, -1e-5, 1.0]])
    u = np.stack([rng.uniform(0, 1920, m), rng.uniform(0, 1080, m)], axis=1)
    w = np.concatenate([u, np.ones((m, 1))], axis=1) @ H.T
    v = w[:, :2] / w[:, 2:] + rng.normal(0.0, 1.0, (m, 2))
    return u.astype(np.float32), v.astype(np.float32)


def random_bits(m, seed, at_least=4):
    """A pseudo-random half of m bits (at least `at_least` of them set, where m allows)."""
    bits = np.random.default_rng([seed, m]).random(m) < 0.5
    bits[:min(at_least, m)] = True
    return bits


def pack(bits, n_words=None):
    """bool [m] -> uint64 words, bit i of word i // 64 (the layout rwh_ransac_batched writes)."""
    n_words = n_words if n_words is not None else max(1, (len(bits) + 63) // 64)
    padded = np.zeros(64 * n_words, dtype=np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view(np.uint64)


def system(u, v):
    """(2N x 8 A, 2N b) in float64 from float32 correspondences; every entry is exact."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    x, y, xp, yp = u[:, 0], u[:, 1], v[:, 0], v[:, 1]
    o, z = np.ones_like(x), np.zeros_like(x)
    r1 = np.stack([x, y, o, z, z, z, -x * xp, -y * xp], axis=1)
    r2 = np.stack([z, z, z, x, y, o, -x * yp, -y * yp], axis=1)
    A = np.empty((2 * len(x), 8))
    A[0::2], A[1::2] = r1, r2
    b = np.empty(2 * len(x))
    b[0::2], b[1::2] = xp, yp
    return A, b


def h_lstsq(u, v):
    A, b = system(u, v)
    h = np.linalg.lstsq(A, b, rcond=None)[0]
    return np.append(h, 1.0).reshape(3, 3)


def project(H, pts):
    w = np.concatenate([np.asarray(pts, dtype=np.float64), np.ones((len(pts), 1))], axis=1) @ np.asarray(H, dtype=np.float64).T
    return w[:, :2] / w[:, 2:]


def deviation(H, H_ls, pts):
    return float(np.sqrt(((project(H, pts) - project(H_ls, pts)) ** 2).sum(axis=1)).max())


def yardstick(u, v, bits):
    """(H_ls, deviation of the reference's float32 refit) for the inlier subset `bits` of the problem (u, v)."""
    import homography as hg
    bits = np.asarray(bits, dtype=bool)
    H_ls = h_lstsq(u[bits], v[bits])
    return H_ls, deviation(hg.calcHomographyLinear(u[bits], v[bits], True), H_ls, u)


def host_refit(lib, u, v, words):
    """rwh_host_refit -> (H 3x3 float64, status)."""
    u, v, words = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32), np.ascontiguousarray(words, np.uint64)
    h, st = np.empty(9), np.zeros(1, dtype=np.int32)
    rc = lib.rwh_host_refit(u.ctypes.data, v.ctypes.data, len(u), words.ctypes.data, h.ctypes.data, st.ctypes.data)
    assert rc == 0, rc
    return h.reshape(3, 3), int(st[0])


def clustered(m=300, seed=1234):
    """m correspondences of the right-hand strip of an 8K frame that overlaps its neighbour: x in [7000, 7679], y in [0, 4319],
    targets about 6990 px to the left, 1 px Gaussian noise.  Far from the origin and narrow, so the moments are large and the
    columns of A nearly dependent."""
    rng = np.random.default_rng([seed, m, 8])
    H = np.array([[1.01, 0.004, -7060.0], [-0.003, 0.995, 30.0], [1.5e-6, -1e-6, 1.0]])
    u = np.stack([rng.uniform(7000, 7679, m), rng.uniform(0, 4319, m)], axis=1)
    w = np.concatenate([u, np.ones((m, 1))], axis=1) @ H.T
    v = w[:, :2] / w[:, 2:] + rng.normal(0.0, 1.0, (m, 2))
    return u.astype(np.float32), v.astype(np.float32)


def patch(m=700, seed=1234):
    """m correspondences of a 40 x 30 px patch at (7600, 2000) of the 8K frame, 0.05 px noise: the equilibrated A^T A has
    trace(G^-1) = 2^34.8 (inverse_trace), far above the 2^27 from which csrc/rwh_refit.h corrects its solution, so every subset
    of some size takes the refit's second pass, through three trips of the 256-stride loop."""
    rng = np.random.default_rng([seed, m, 9])
    H = np.array([[1.01, 0.004, -7060.0], [-0.003, 0.995, 30.0], [1.5e-6, -1e-6, 1.0]])
    u = np.stack([rng.uniform(7600, 7640, m), rng.uniform(2000, 2030, m)], axis=1)
    w = np.concatenate([u, np.ones((m, 1))], axis=1) @ H.T
    v = w[:, :2] / w[:, 2:] + rng.normal(0.0, 0.05, (m, 2))
    return u.astype(np.float32), v.astype(np.float32)


PATCH_FAMILIES = ("all", "random half", "wave 3")


def inverse_trace(u, v, bits):
    """trace(G^-1) for G = the inlier subset's A^T A scaled to a unit diagonal, in float64: what the refit compares with 2^27."""
    A, _ = system(u[bits], v[bits])
    G = A.T @ A
    d = 1.0 / np.sqrt(np.diag(G))
    return float(np.trace(np.linalg.inv(G * d[:, None] * d[None, :])))


def exact_fit(u, v, bits):
    """H_x: the least-squares problem of system() on the inlier subset, solved without rounding.  Every float32 coordinate becomes
    a Fraction, A^T A and A^T b are exact sums over the rows of system(), the 8 x 8 system is solved by Gaussian elimination in
    Fraction, and only the eight results are rounded, to float64.  ZeroDivisionError when A^T A is singular."""
    F = fractions.Fraction
    bits = np.asarray(bits, dtype=bool)
    one, n = F(1), 8
    G = [[F(0)] * (n + 1) for _ in range(n)]           # upper triangle of A^T A | A^T b
    for (x, y), (xp, yp) in zip(np.asarray(u)[bits].tolist(), np.asarray(v)[bits].tolist()):
        x, y, xp, yp = F(x), F(y), F(xp), F(yp)
        for row, b in ((((0, x), (1, y), (2, one), (6, -x * xp), (7, -y * xp)), xp),
                       (((3, x), (4, y), (5, one), (6, -x * yp), (7, -y * yp)), yp)):
            for k, (i, ai) in enumerate(row):
                G[i][n] += ai * b
                for j, aj in row[k:]:
                    G[i][j] += ai * aj
    for i in range(n):
        for j in range(i):
            G[i][j] = G[j][i]
    for c in range(n):
        piv = next((r for r in range(c, n) if G[r][c] != 0), None)
        if piv is None:
            raise ZeroDivisionError("exact_fit: A^T A is singular")
        G[c], G[piv] = G[piv], G[c]
        for r in range(c + 1, n):
            if G[r][c] != 0:
                f = G[r][c] / G[c][c]
                G[r] = [a - f * t for a, t in zip(G[r], G[c])]
    h = [F(0)] * n
    for c in range(n - 1, -1, -1):
        h[c] = (G[c][n] - sum(G[c][j] * h[j] for j in range(c + 1, n))) / G[c][c]
    return np.array([float(t) for t in h] + [1.0]).reshape(3, 3)


def resolution(u, v, bits, H_x):
    """The smallest move of the fit that one lost inlier causes: the minimum, over the inliers j, of the deviation from H_x of the
    lstsq fit of the subset without j.  Defined for n >= 5 inliers."""
    idx = np.flatnonzero(np.asarray(bits, dtype=bool))
    assert len(idx) >= 5, len(idx)
    return min(deviation(h_lstsq(u[np.delete(idx, k)], v[np.delete(idx, k)]), H_x, u) for k in range(len(idx)))


# ---- the problems of one launch, in launch order, and the mask families ----
# 185 = matchespoints, 300 = clustered(), the others synthetic(m); "three" gives FEW and "empty" (two equal offsets) sits in the
# middle of the batch.  No offset but the first is a multiple of 64.
PROBLEMS = ("synthetic M=4", "synthetic M=5", "synthetic M=63", "synthetic M=64", "synthetic M=65", "synthetic M=130", "matchespoints",
            "synthetic M=1000", "three", "synthetic M=255", "synthetic M=256", "empty", "synthetic M=257", "synthetic M=511",
            "synthetic M=512", "synthetic M=513", "synthetic M=1281", "clustered M=300", "synthetic M=185")
RANDOM_SEED = 11


def _five(m):
    bits = np.zeros(m, dtype=bool)
    bits[[i for i in (0, 1, m // 2, m - 2, m - 1) if 0 <= i < m]] = True
    return bits


FAMILIES = {"all": lambda m: np.ones(m, dtype=bool),
            "random half": lambda m: random_bits(m, RANDOM_SEED),
            "wave 3": lambda m: np.arange(m) % 256 >= 192,              # lanes 192 .. 255 only
            "top bits": lambda m: np.arange(m) % 64 == 63,              # bit 63 of every mask word
            "lane 255": lambda m: np.arange(m) % 256 == 255,            # one lane, one correspondence per trip of the stride loop
            "ends": _five}                                              # {0, 1, M/2, M-2, M-1}


@functools.lru_cache(maxsize=None)
def problem(name):
    """(u, v) float32 [m, 2] of a problem of PROBLEMS; shared and read-only."""
    if name == "matchespoints":
        u, v = matchespoints()
    elif name == "three":
        u, v = synthetic(3)
    elif name == "empty":
        u, v = synthetic(3)
        u, v = u[:0].copy(), v[:0].copy()
    else:
        kind, m = name.split(" M=")
        u, v = (clustered if kind == "clustered" else synthetic)(int(m))
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


@functools.lru_cache(maxsize=None)
def family_bits(name, family):
    bits = FAMILIES[family](len(problem(name)[0]))
    bits.setflags(write=False)
    return bits


@functools.lru_cache(maxsize=None)
def cases():
    """Every (problem, family) that leaves at least 4 bits, as (problem, family) names; a family that sets every bit of a problem
    is the problem's "all" and listed once."""
    out = []
    for name in PROBLEMS:
        for family in FAMILIES:
            bits = family_bits(name, family)
            if bits.sum() >= 4 and (family == "all" or not bits.all()):
                out.append((name, family))
    return tuple(out)


MASK_WORDS = (max(len(problem(name)[0]) for name in PROBLEMS) + 63) // 64       # a mask row of the launch: what the largest problem needs


def dirty(bits, n_words=MASK_WORDS):
    """pack(bits, n_words) with every bit at or past len(bits) set: the rest of the last word and every later word of the row."""
    words = pack(bits, n_words)
    garbage = np.ones(64 * n_words, dtype=np.uint8)
    garbage[:len(bits)] = 0
    return words | np.packbits(garbage, bitorder="little").view(np.uint64)


# non-finite coordinates: (0 = source / 1 = target, coordinate, value), one in each slot of a correspondence
POISONS = ((0, 0, np.nan), (0, 1, np.inf), (1, 0, -np.inf), (1, 1, np.nan))


def poisoned(u, v, i, poison):
    """Copies of (u, v) with one coordinate of correspondence i made non-finite."""
    which, coordinate, value = poison
    out = [u.copy(), v.copy()]
    out[which][i, coordinate] = value
    return out


def rank_deficient():
    """Inlier sets whose A^T A is singular in exact arithmetic, as (name, u, v), every bit set: 70 correspondences on one line
    (source points on y = x / 2 + 10, exact in float32) and 4 correspondences of which two are equal.  Which way the rounding of a
    zero pivot falls is the solver's; kernel and host twin must fall the same way."""
    H = np.array([[1.03, 0.02, 40.0], [-0.015, 0.98, 25.0], [2e-5, -1e-5, 1.0]])
    x = np.arange(70, dtype=np.float64) * 24.0 + 3.0
    u = np.stack([x, 0.5 * x + 10.0], axis=1)
    w = np.concatenate([u, np.ones((70, 1))], axis=1) @ H.T
    line = u.astype(np.float32), (w[:, :2] / w[:, 2:]).astype(np.float32)
    u4, v4 = (a.copy() for a in synthetic(4))
    u4[3], v4[3] = u4[0], v4[0]
    return (("70 on one line", *line), ("4 with two equal", u4, v4))


_references = {}


def reference(u, v, bits):
    """(H_x, deviation of H_ls from H_x, resolution or None below 5 inliers) of an inlier subset; computed once per subset."""
    bits = np.asarray(bits, dtype=bool)
    key = (u.tobytes(), v.tobytes(), bits.tobytes())
    if key not in _references:
        H_x = exact_fit(u, v, bits)
        res = resolution(u, v, bits, H_x) if bits.sum() >= 5 else None
        _references[key] = (H_x, deviation(h_lstsq(u[bits], v[bits]), H_x, u), res)
    return _references[key]


def hold(side, case, H, u, v, bits):
    """Conditions A and B (module docstring) on a refit H of the inlier subset `bits`; prints the case's line first.  Returns the
    deviation from H_x."""
    H_x, dev_ls, res = reference(u, v, bits)
    dev = deviation(H, H_x, u)
    report(side, case, dev, dev_ls, res)
    if res is not None:
        assert dev_ls <= res / 16, "%s: lstsq is %.3e px from the exact fit, resolution %.3e px: no scale to judge by" % (case, dev_ls, res)
        assert dev <= res / 16, "%s %s (A): %.3e px from the exact fit, resolution / 16 = %.3e px" % (side, case, dev, res / 16)
    assert dev <= dev_ls, "%s %s (B): %.3e px from the exact fit, lstsq %.3e px" % (side, case, dev, dev_ls)
    return dev


def report(side, case, dev, dev_lstsq, res):
    """One line per case, printed (run with -s to collect the figures that profiles/refit_device.txt records)."""
    print("refit %-9s %-30s from exact fit %.3e px   lstsq %.3e px   resolution %s"
          % (side, case, dev, dev_lstsq, "%.3e px (1/16 used: %.1e)" % (res, 16 * dev / res) if res is not None else "-- (n = 4)"))


null = ctypes.c_void_p(0)
