"""Helpers of the extractor's tests (test_orb_cpu.py, test_orb_gpu.py, the edge and pyramid files) -- not a test module.

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


def gpu_torch():
    """torch, with the GPU in sight and the package built: the body of every GPU file's `gpu` fixture."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch


def extract(images, per_level=False, **kw):
    """extract_batch on the GPU -> one dict per image as `restate` gives it, with level and size besides (what
    orb_pyramid_cases.restate_pyramid adds); found is the image's total, with per_level the list of its levels' counts."""
    import ransac as rs
    info = {}
    feats = rs.extract_batch(images, info=info, **kw)
    assert all(k.is_cuda and d.is_cuda and k.shape[0] == d.shape[0] == c for (k, d), c in zip(feats, info["counts"]))
    assert info["found"] == [sum(f) for f in info["found_levels"]]
    return [dict(kps=k.cpu().numpy(), desc=d.cpu().numpy(), score=s.cpu().numpy(), bin=b.cpu().numpy(), level=l.cpu().numpy(),
                 size=z.cpu().numpy(), found=f)
            for (k, d), s, b, l, z, f in zip(feats, info["score"], info["bin"], info["level"], info["size"],
                                             info["found_levels" if per_level else "found"])]


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


# ---- the edge cases (test_orb_edges_cpu.py, test_orb_edges_gpu.py): built for branches that texture reaches only by chance ----
CELL = 33                                    # the smallest image with a legal centre, (16, 16): cells of a mosaic are that size


def _arc_cell(background, start, length, value):
    """A 33 x 33 cell of `background` whose centre's circle pixels start .. start + length - 1 (modulo 16) hold `value`."""
    cell = np.full((CELL, CELL), background, dtype=np.uint8)
    for j in range(length):
        dx, dy = CIRCLE[(start + j) % 16]
        cell[16 + dy, 16 + dx] = value
    return cell


def arc_mosaic(threshold):
    """(gray image of 8 x 12 cells = 264 x 396, must, must_not): for each polarity (brighter, darker) and each of the 16 arc starts
    three cells -- exactly 9 consecutive circle pixels at background +- (threshold + 1): the centre is a keypoint of score
    threshold + 1; the same at +- threshold: score == threshold, none; only 8 consecutive pixels at the largest difference a byte
    holds: no arc of 9, none.  `must` lists (x, y, score) of the centres that are keypoints, `must_not` (x, y) of those that are
    not.  The brighter arcs sit in the upper four cell rows on a background of min(128, 254 - threshold), the darker ones in the
    lower four on max(128, threshold + 1): one flat 128 up to threshold 126; at threshold 254, 255 on 0 above 0 on 255."""
    t = int(threshold)
    assert 1 <= t <= 254
    rows, cols = 8, 12
    img = np.zeros((rows * CELL, cols * CELL), dtype=np.uint8)
    must, must_not = [], []
    n = 0
    for sign, background in ((1, min(128, 254 - t)), (-1, max(128, t + 1))):
        for start in range(16):
            for kind in range(3):
                value = background + sign * (t + 1) if kind == 0 else background + sign * t if kind == 1 else (255 if sign > 0 else 0)
                r, c = divmod(n, cols)
                img[r * CELL:(r + 1) * CELL, c * CELL:(c + 1) * CELL] = _arc_cell(background, start, 8 if kind == 2 else 9, value)
                centre = (c * CELL + 16, r * CELL + 16)
                if kind == 0:
                    must.append(centre + (t + 1,))
                else:
                    must_not.append(centre)
                n += 1
    assert n == rows * cols == 96
    return img, must, must_not


def bin_wheel():
    """(gray 165 x 198, centres): 5 x 6 cells, cell k a dot of 255 at its centre with one satellite pixel of 100 at radius 10 in
    direction 12 k degrees (y downwards) -- moment vector 100 (dx, dy), within 3 degrees of the middle of sector k.  The 30 centres
    are the 30 strongest keypoints, in cell order: bins 0, 1, ..., 29."""
    rows, cols = 5, 6
    img = np.zeros((rows * CELL, cols * CELL), dtype=np.uint8)
    centres = []
    for k in range(BINS):
        r, c = divmod(k, cols)
        x, y = c * CELL + 16, r * CELL + 16
        a = np.deg2rad(12.0 * k)
        img[y, x] = 255
        img[y + int(np.rint(10 * np.sin(a))), x + int(np.rint(10 * np.cos(a)))] = 100
        centres.append((x, y))
    return img, centres


WIDE_W = 65536
_wide = {}


def wide_image():
    """(gray 33 x 65536, strong, weak), read-only and built once: noise of 0 .. 10 under dots of 250 at x = 16 and x = 65519 -- the
    first and the last legal column, row 16 being the only legal row -- and, astride the tile seams at x = 64, 32768 and 65472, a
    dot of 250 on one side with a dot of 200 as its neighbour on the other: the weaker one is suppressed through the halo.
    x = 65519 and 65472 need all 16 bits of a key's field."""
    if not _wide:
        img = np.random.RandomState(77).randint(0, 11, (CELL, WIDE_W)).astype(np.uint8)
        strong = [(16, 16), (WIDE_W - 1 - BORDER, 16), (63, 16), (32767, 16), (65472, 16)]
        weak = [(64, 16), (32768, 16), (65471, 16)]
        for x, y in strong:
            img[y, x] = 250
        for x, y in weak:
            img[y, x] = 200
        img.flags.writeable = False
        _wide["v"] = (img, strong, weak)
    return _wide["v"]


def tall_image():
    """The transpose of `wide_image`, 65536 x 33: the same dots at (16, y), y up to 65519, the seams between tile rows."""
    img, strong, weak = wide_image()
    return np.ascontiguousarray(img.T), [(y, x) for x, y in strong], [(y, x) for x, y in weak]


def narrow(seed):
    """One 33 x 65 image -- 2 x 3 tiles, legal centres (16 .. 48, 16): gray, RGB or RGBA by seed % 3; seeds 0 .. 2 are random texture,
    the others noise of 0 .. 10 under one to four planted dots on the legal row, every third of them under a stronger dot in the
    row above (no legal centre, but it suppresses)."""
    c = (1, 3, 4)[seed % 3]
    if seed < 3:
        return random_image(CELL, 65, 100 + seed, channels=c)
    rng = np.random.RandomState(1000 + seed)
    plane = rng.randint(0, 11, (CELL, 65))
    for j, col in enumerate(rng.permutation(9)[:1 + seed % 4]):
        x, v = 16 + 4 * int(col), 60 + int(rng.randint(0, 160))
        plane[16, x] = v
        if (seed + j) % 3 == 0:
            plane[15, x] = v + 30
    if c == 1:
        return plane.astype(np.uint8)
    img = np.clip(plane[:, :, None] + rng.randint(-5, 6, (CELL, 65, c)), 0, 255)
    if c == 4:
        img[:, :, 3] = rng.randint(0, 256, (CELL, 65))
    return img.astype(np.uint8)


def strip(w, c, seed):
    """1 x w random uint8 with c channels: too flat for a keypoint, but its gray plane is an output and its tiles are work."""
    return random_image(1, w, seed, channels=c)


def numbered(i):
    """Image i of a long batch: gray, 33 .. 40 x 33 .. 48, one to three dots whose position and value are functions of i -- a batch
    whose per-image tile counts were summed in the wrong order shows as wrong keypoints."""
    h, w = CELL + i % 8, CELL + (5 * i) % 16
    pts = [(16 + (3 * i + 5 * j) % (w - 32), 16 + (i + 3 * j) % (h - 32), 60 + (7 * i + 31 * j) % 190) for j in range(1 + i % 3)]
    return dots(h, w, pts)


def key_set(img, threshold=20):
    """The keys (255 - S) << 32 | y << 16 | x of rule 3 for one image, as a set of ints."""
    x, y, s = keypoints(scores(gray(img)), threshold)
    return set(((255 - s.astype(np.int64)) << 32 | y.astype(np.int64) << 16 | x.astype(np.int64)).tolist())


def edge_cases():
    """(name, image, kwargs) of the edge cases that hold keypoints: the CPU module runs each through the host twin and the restatement."""
    cases = [("arcs at threshold 20", arc_mosaic(20)[0], dict(threshold=20)), ("arcs at threshold 254", arc_mosaic(254)[0], dict(threshold=254)),
             ("bin wheel", bin_wheel()[0], {}), ("wide", wide_image()[0], {}), ("tall", tall_image()[0], {})]
    cases += [("narrow %d" % s, narrow(s), {}) for s in range(12)]
    cases += [("strip %d x %d" % (w, c), strip(w, c, 40 + c), {}) for w, c in ((4097, 1), (4097, 3), (65, 4))]
    return cases
