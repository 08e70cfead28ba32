"""Shared by tests/test_refit_cpu.py and tests/test_refit_gpu.py: the inputs of the device-refit tests and their yardstick.

Yardstick: for a problem's inlier subset, A and b of the reference's least-squares problem (calc_correspLinearCollective) are
built in float64 and solved by numpy.linalg.lstsq -> H_ls.  The DEVIATION of a matrix H is the largest distance in pixels, over
ALL of the problem's correspondences, between H (x, y, 1) and H_ls (x, y, 1), both dehomogenised, in float64.  A refit passes
when its deviation is no larger than that of the project's calcHomographyLinear(u, v, True) on the same subset -- the
reference's float32 normal equations, pinned by the golden fixtures."""
import ctypes
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


def report(side, case, dev_refit, dev_reference):
    """One line per case, printed (run with -s to collect the figures that profiles/refit_device.txt records)."""
    print("refit %-9s %-34s deviation %.3e px   reference float32 refit %.3e px" % (side, case, dev_refit, dev_reference))


null = ctypes.c_void_p(0)
