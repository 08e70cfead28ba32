"""The gain rule (include/rwh.h: overlap statistics, gains) restated in numpy on top of tests/sequence_cases.py (which restates
the compositor with gains and drives it), the ctypes drivers of the statistics' and the solver's host twins, and the fixtures that
tests/test_sequence_gains_cpu.py and tests/test_sequence_gains_gpu.py share."""
import numpy as np

import sequence_cases as sc

U = 2.0 ** -53


# ---- the rule ----
def planes(images, Gs, anchor):
    """-> (rects, (ox, oy), (fh, fw), cover bool [n, fh, fw], L int64 [n, fh, fw]): where each image covers the canvas, and the sum
    of the three bytes paste would write for it there."""
    n = len(images)
    rects = sc.rectangles([im.shape for im in images], Gs, anchor)
    (ox, oy), (fh, fw) = sc.canvas_of(rects)
    cover, L = np.zeros((n, fh, fw), dtype=bool), np.zeros((n, fh, fw), dtype=np.int64)
    for i in range(n):
        v, valid, _ = sc.sample(images[i], Gs[i], rects[i], i == anchor)
        r = rects[i]
        win = (slice(r[1] - oy, r[1] - oy + r[3]), slice(r[0] - ox, r[0] - ox + r[2]))
        cover[i][win] = valid
        L[i][win] = np.where(valid, v.astype(np.int32).astype(np.uint8).astype(np.int64).sum(axis=2), 0)
    return rects, (ox, oy), (fh, fw), cover, L


def stats(images, Gs, anchor, stride):
    """-> (count, sum) uint64 [n, n] over the canvas pixels with cx % stride == 0 and cy % stride == 0."""
    _, _, _, cover, L = planes(images, Gs, anchor)
    cover, L = cover[:, ::stride, ::stride], L[:, ::stride, ::stride]
    n = len(images)
    count, total = np.zeros((n, n), dtype=np.uint64), np.zeros((n, n), dtype=np.uint64)
    for i in range(n):
        for j in range(n):
            both = cover[i] & cover[j]
            count[i, j], total[i, j] = both.sum(), L[i][both].sum()
    return count, total


def system(count, total, sigma_n=10.0, sigma_g=0.1):
    """-> (A, b, I) of the rule, built in its order."""
    n = len(count)
    alpha, beta = 1.0 / (sigma_n * sigma_n), 1.0 / (sigma_g * sigma_g)
    N = count.astype(np.float64)
    I = np.zeros((n, n))
    I[count > 0] = total[count > 0].astype(np.float64) / (3.0 * N[count > 0])
    A, b = np.zeros((n, n)), np.zeros(n)
    for i in range(n):
        if count[i, i] == 0:
            A[i, i], b[i] = 1.0, 1.0
            continue
        for j in range(n):
            A[i, i] += beta * N[i, j]
            b[i] += beta * N[i, j]
            if j != i:
                A[i, i] += 2 * alpha * I[i, j] * I[i, j] * N[i, j]
                A[i, j] -= 2 * alpha * I[i, j] * I[j, i] * N[i, j]
    return A, b, I


def gains(count, total, sigma_n=10.0, sigma_g=0.1):
    A, b, _ = system(count, total, sigma_n, sigma_g)
    return np.linalg.solve(A, b)


def residual_bound(A, g):
    """The backward-error bound of a Cholesky solve: 4 n^2 u |A|_inf |g|_inf."""
    n = len(g)
    return 4 * n * n * U * np.abs(A).sum(axis=1).max() * np.abs(g).max()


def mismatch(count, I, g):
    """sum over i != j of N_ij (g_i I_ij - g_j I_ji)^2."""
    n = len(g)
    return sum(float(count[i, j]) * (g[i] * I[i, j] - g[j] * I[j, i]) ** 2 for i in range(n) for j in range(n) if i != j)


# ---- the host twins ----
def guarded_tables(n):
    """Two uint64 [n, n] tables pre-filled with 0xA5 bytes, each between two 64-byte canaries: -> (buffer uint8, count, sum, check)."""
    size = n * n * 8
    buf = np.full(2 * (size + 128), 0xA5, dtype=np.uint8)
    tabs = [buf[k * (size + 128) + 64:k * (size + 128) + 64 + size].view(np.uint64).reshape(n, n) for k in range(2)]

    def check(flat=buf):
        for k in range(2):
            at = k * (size + 128)
            assert (flat[at:at + 64] == 0xA5).all() and (flat[at + 64 + size:at + 128 + size] == 0xA5).all(), "a byte outside the tables was written"
    return buf, tabs[0], tabs[1], check


def host_stats(lib, images, Gs, anchor=0, stride=1):
    """rwh_host_sequence_overlap_stats -> (status, count, sum); the tables start as 0xA5 bytes between canaries that are checked here."""
    images = [np.ascontiguousarray(im) for im in images]
    t = sc.tables(images, Gs, anchor)
    fh, fw = t["size"]
    _, count, total, check = guarded_tables(t["n"])
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    st = lib.rwh_host_sequence_overlap_stats(ptrs.ctypes.data, t["hw"].ctypes.data, t["inv"].ctypes.data, t["rects"].ctypes.data, t["n"], anchor,
                                             fh, fw, t["origin"][0], t["origin"][1], stride, count.ctypes.data, total.ctypes.data)
    check()
    return st, count.copy(), total.copy()


def host_gains(lib, count, total, sigma_n=10.0, sigma_g=0.1):
    """rwh_host_sequence_gains -> (status, gains float64 [n]), the gains between two canaries that are checked here."""
    n = len(count)
    count, total = np.ascontiguousarray(count, dtype=np.uint64), np.ascontiguousarray(total, dtype=np.uint64)
    buf = np.full(n + 16, -7.0)
    st = lib.rwh_host_sequence_gains(count.ctypes.data, total.ctypes.data, n, sigma_n, sigma_g, buf[8:].ctypes.data)
    assert (buf[:8] == -7.0).all() and (buf[-8:] == -7.0).all()
    return st, buf[8:8 + n].copy()


def hstats(lib, *a, **k):
    st, count, total = host_stats(lib, *a, **k)
    assert st == 0
    return count, total


# ---- the cases ----
def mixed_gains(n):
    """1.9, 0.5, 1.0, ... : bright enough to clip at 255, darker, and as it is."""
    return np.array([(1.9, 0.5, 1.0)[i % 3] for i in range(n)])


def forty_in_one_tile():
    """The fixture of test_sequence_gpu.test_forty_candidates_in_one_tile: 40 images over one 256 x 4 tile."""
    rng = np.random.default_rng(40)
    images = [sc.random_image(6, 30, 400 + i) for i in range(40)]
    Gs = [np.eye(3)] + [sc.homography(rng, 5.0 * i + 0.25, (i % 2) + 0.5, 0.004, 1e-6) for i in range(1, 40)]
    return images, Gs


def sixty_four_half_steps():
    """64 images of 6 x 40, image i half a pixel right of image i - 1: every one of the 4096 pairs meets, in one tile."""
    return [sc.random_image(6, 40, 600 + i) for i in range(64)], [sc.translate(0.5 * i, 0) for i in range(64)]


def exposure_fixture():
    """Three 200 x 260 crops of scene() at columns 0 / 90 / 180, scaled by 0.7 / 1.0 / 1.3, rounded and clipped; their translations."""
    scene = sc.scene().astype(np.float64)
    crops = [np.clip(np.rint(scene[:, x:x + 260] * e), 0, 255).astype(np.uint8) for x, e in zip((0, 90, 180), (0.7, 1.0, 1.3))]
    return crops, [sc.translate(90 * i, 0) for i in range(3)]


def identical_overlaps():
    """Three 50 x 70 crops of one small scene, each 20 columns right of and 3 rows above the one before: integer translations, and
    no image's texel (0,0) (which a warped image reads as 0) lies inside another image -- where two meet, their bytes are equal."""
    scene = sc.scene(60, 120, seed=6)
    at = [(0, 6), (20, 3), (40, 0)]
    images = [np.ascontiguousarray(scene[y:y + 50, x:x + 70]) for x, y in at]
    return images, [sc.translate(x - at[0][0], y - at[0][1]) for x, y in at]


def between_samples():
    """A 2 x 2 image at canvas (1, 1) of a 9 x 11 anchor: at stride 7 no sample falls on it."""
    return [sc.random_image(9, 11, 70), sc.random_image(2, 2, 71)], [np.eye(3), sc.translate(1, 1)]
