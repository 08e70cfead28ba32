"""Helpers of the extractor's tests (test_orb_cpu.py, test_orb_gpu.py) -- not a test module.

`restate` restates the rule of include/rwh.h (rwh_orb_detect_batched / rwh_orb_describe_batched) in numpy, written from that text:
whole planes, shifted views for the circle and the neighbours, a lexsort for the order, fancy indexing for the patches, an integral
image for the boxes.  Everything is an integer: every comparison in the tests is exact equality."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BORDER, BINS, PATCH_RADIUS, TEST_RADIUS = 16, 30, 15, 13
CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
          (-2, -2), (-1, -3))


def tables(nbytes=32, pattern=None):
    """(bin table int32 [30, 2], rotated pattern int8 [30, 8 * nbytes, 4]) as the package makes them."""
    import ransac as rs
    return rs.orb_bin_table(), rs.rotate_pattern(rs.default_pattern(nbytes) if pattern is None else pattern)


def gray(img):
    """Rule 1."""
    if img.ndim == 2:
        return img.copy()
    v = img.astype(np.int64)
    return ((4899 * v[:, :, 0] + 9617 * v[:, :, 1] + 1868 * v[:, :, 2] + 8192) >> 14).astype(np.uint8)


def scores(g):
    """Rule 2: int32 [h, w]."""
    h, w = g.shape
    S = np.zeros((h, w), dtype=np.int32)
    if h < 7 or w < 7:
        return S
    c = g[3:h - 3, 3:w - 3].astype(np.int16)
    d = np.stack([g[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx].astype(np.int16) - c for dx, dy in CIRCLE])
    best = np.zeros(c.shape, dtype=np.int16)
    for a in range(16):
        arc = d[[(a + j) % 16 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(axis=0), -arc.max(axis=0)))
    S[3:h - 3, 3:w - 3] = best
    return S


def keypoints(S, threshold):
    """Rule 3 without the cut: (x, y, s) int arrays ordered by (s descending, y, x)."""
    h, w = S.shape
    P = np.zeros((h + 2, w + 2), dtype=np.int32)
    P[1:-1, 1:-1] = S
    nb = np.max(np.stack([P[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]), axis=0)
    ok = (S > threshold) & (S > nb)
    yy, xx = np.mgrid[0:h, 0:w]
    ok &= (xx >= BORDER) & (xx <= w - 1 - BORDER) & (yy >= BORDER) & (yy <= h - 1 - BORDER)
    y, x = np.nonzero(ok)
    s = S[y, x]
    o = np.lexsort((x, y, -s))
    return x[o], y[o], s[o]


def orientation_bins(g, x, y, bin_table):
    """Rule 4: (bin int32 [N], m10, m01)."""
    dy, dx = np.mgrid[-PATCH_RADIUS:PATCH_RADIUS + 1, -PATCH_RADIUS:PATCH_RADIUS + 1]
    disc = dx * dx + dy * dy <= PATCH_RADIUS * PATCH_RADIUS
    dx, dy = dx[disc].astype(np.int64), dy[disc].astype(np.int64)
    v = g[y[:, None] + dy[None, :], x[:, None] + dx[None, :]].astype(np.int64)
    m10, m01 = (v * dx).sum(axis=1), (v * dy).sum(axis=1)
    b = bin_table.astype(np.int64)
    cross = b[None, :, 0] * m01[:, None] - b[None, :, 1] * m10[:, None]          # [N, 30]
    hit = (cross >= 0) & (np.roll(cross, -1, axis=1) < 0)
    assert (hit.sum(axis=1) == ((m10 != 0) | (m01 != 0))).all()                  # exactly one sector, none for the zero vector
    return np.where(hit.any(axis=1), hit.argmax(axis=1), 0).astype(np.int32), m10, m01


def descriptors(g, x, y, bins, rotated):
    """Rule 5: uint8 [N, nbytes]."""
    h, w = g.shape
    I = np.zeros((h + 1, w + 1), dtype=np.int64)
    I[1:, 1:] = g.astype(np.int64).cumsum(axis=0).cumsum(axis=1)

    def box(u, v):                           # the 5 x 5 window centred on (u, v): columns u - 2 .. u + 2, rows v - 2 .. v + 2
        return I[v + 3, u + 3] - I[v - 2, u + 3] - I[v + 3, u - 2] + I[v - 2, u - 2]
    t = rotated[bins].astype(np.int64)       # [N, nbits, 4]
    bits = box(x[:, None] + t[:, :, 0], y[:, None] + t[:, :, 1]) < box(x[:, None] + t[:, :, 2], y[:, None] + t[:, :, 3])
    return np.packbits(bits, axis=1, bitorder="little")


def restate(img, n_features=500, threshold=20, nbytes=32, pattern=None):
    """The whole rule for one image -> dict(kps float32 [N, 2], desc uint8 [N, nbytes], score, bin int32 [N], found)."""
    bin_table, rotated = tables(nbytes, pattern)
    g = gray(img)
    x, y, s = keypoints(scores(g), threshold)
    found = len(x)
    x, y, s = x[:n_features], y[:n_features], s[:n_features]
    bins, _, _ = orientation_bins(g, x, y, bin_table)
    desc = descriptors(g, x, y, bins, rotated) if len(x) else np.zeros((0, nbytes), dtype=np.uint8)
    return dict(kps=np.stack([x, y], axis=1).astype(np.float32).reshape(-1, 2), desc=desc, score=s.astype(np.int32), bin=bins, found=found)


def host_extract(lib, img, n_features=500, threshold=20, nbytes=32, pattern=None, rotated=None):
    """rwh_host_orb_extract on one image -> (status, dict as `restate` gives it)."""
    bin_table, rot = tables(nbytes, pattern)
    rot = np.ascontiguousarray(rot if rotated is None else rotated)
    img = np.ascontiguousarray(img)
    c = 1 if img.ndim == 2 else img.shape[2]
    room = max(n_features, 1)
    kps = np.full((room, 2), -7, dtype=np.float32)
    desc = np.full((room, nbytes), 0xAA, dtype=np.uint8)
    score, bins = np.full(room, -7, dtype=np.int32), np.full(room, -7, dtype=np.int32)
    count, found = np.full(1, -7, dtype=np.int32), np.full(1, -7, dtype=np.int32)
    st = lib.rwh_host_orb_extract(img.ctypes.data, img.shape[0], img.shape[1], c, threshold, n_features, bin_table.ctypes.data,
                                  rot.ctypes.data, nbytes, kps.ctypes.data, desc.ctypes.data, score.ctypes.data, bins.ctypes.data,
                                  count.ctypes.data, found.ctypes.data)
    n = max(int(count[0]), 0)
    return st, dict(kps=kps[:n], desc=desc[:n], score=score[:n], bin=bins[:n], found=int(found[0]))


def same(a, b):
    return (a["found"] == b["found"] and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k])
                                             for k in ("kps", "desc", "score", "bin")))


# ---- the cases ----
def random_image(h, w, seed, channels=3):
    shape = (h, w) if channels == 1 else (h, w, channels)
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def dots(h, w, points, background=0):
    """A gray plane with single bright pixels (x, y, value): each is a corner of score value - background with an empty ring."""
    img = np.full((h, w), background, dtype=np.uint8)
    for x, y, v in points:
        img[y, x] = v
    return img


def checkerboard(h=64, w=80, block=4, pitch=10):
    """Blocks of 255 on 0 (a full checkerboard has X-junctions only, which no arc of 9 spans): every block corner saturates."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((xx % pitch < block) & (yy % pitch < block), 255, 0).astype(np.uint8)


def tie_image():
    """60 x 90 gray: three dots of score 255 and nine of score 200, eight pixels apart; n_features = 7 cuts inside the 200s."""
    pts = [(20 + 8 * i, 20, 255) for i in range(3)] + [(20 + 8 * (i % 5), 30 + 8 * (i // 5), 200) for i in range(9)]
    return dots(60, 90, pts), 7


def boundary_image():
    """48 x 80 gray: a dot at (20, 24) with one pixel straight below it -- moment vector (0, +) on boundary 8 (90 degrees), the lower
    boundary of bin 8 -- and, out of the first one's patch, a dot at (50, 24) with one pixel straight above it: (0, -) on boundary
    23 (270 degrees), bin 23."""
    return dots(48, 80, [(20, 24, 255), (20, 29, 100), (50, 24, 255), (50, 19, 100)])


def foto(name="A"):
    return np.load(os.path.join(GOLDEN, "img_foto1.npz"), allow_pickle=False)[name]


def caller_pattern(nbytes=4):
    """A pattern that is not the default: axis-aligned and diagonal pairs on rings of radius 3 .. 13."""
    rng = np.random.RandomState(5)
    out = []
    while len(out) < 8 * nbytes:
        p = rng.randint(-13, 14, 4)
        if p[0] ** 2 + p[1] ** 2 <= 169 and p[2] ** 2 + p[3] ** 2 <= 169 and tuple(p[:2]) != tuple(p[2:]):
            out.append(p)
    return np.array(out, dtype=np.int8)


def cpu_cases():
    """(name, image, kwargs) of every case the CPU suite runs and the GPU batch repeats."""
    rgb = random_image(40, 48, 1)
    rgba = np.concatenate([rgb, random_image(40, 48, 2, channels=1)[:, :, None]], axis=2)
    tie, cut = tie_image()
    crop = np.ascontiguousarray(foto("A")[200:400, 300:600])
    cases = [("random 40x48", rgb, {}), ("rgba", rgba, {}), ("gray", gray(rgb), {}),
             ("one centre 33x33", dots(33, 33, [(16, 16, 255)]), {}), ("too small 32x40", random_image(32, 40, 3), {}),
             ("flat", np.full((50, 60, 3), 77, dtype=np.uint8), {}), ("checkerboard", checkerboard(), {}),
             ("tie at the cut", tie, dict(n_features=cut)), ("boundary", boundary_image(), {}),
             ("threshold 0", rgb, dict(threshold=0)), ("threshold 254", checkerboard(), dict(threshold=254)),
             ("caller's pattern", rgb, dict(nbytes=4, pattern=caller_pattern(4))), ("foto crop", crop, {})]
    cases += [("nbytes %d" % nb, rgb, dict(nbytes=nb)) for nb in (1, 61, 64)]
    return cases
