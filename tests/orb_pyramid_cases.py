"""Helpers of the pyramid extractor's tests (test_orb_pyramid_cpu.py, test_orb_pyramid_gpu.py) -- not a test module.

`plane` and `restate_pyramid` restate rules 6 - 8 of include/rwh.h in numpy, written from that text; rules 1 - 5 come from
tests/orb_cases.py.  The area average is two integer matrix products (overlap lengths on y, the gray plane, overlap lengths on x)
and one rounding -- neither the host twin's double loop nor the kernel's tiles.  Everything is an integer: every comparison in the
tests is exact equality."""
import numpy as np

import orb_cases as oc

ONE, SCALE_MAX, LEVELS_MAX, PATCH = 256, 1024, 16, 31
CALLER_SCALES = np.array([256, 300, 1024], dtype=np.int32)


def level_side(n, s):
    return (256 * int(n) + int(s) // 2) // int(s)


def overlaps(n, s):
    """int64 [n_l, n]: row X holds the overlap lengths of [X s, (X + 1) s) with the source pixels [256 j, 256 (j + 1)); what lies
    beyond the last source pixel is added to the last one (the edge rule)."""
    nl = level_side(n, s)
    W = np.zeros((nl, n), dtype=np.int64)
    for X in range(nl):
        a, b = X * s, (X + 1) * s
        for j in range(a // 256, (b - 1) // 256 + 1):
            W[X, min(j, n - 1)] += min(b, 256 * (j + 1)) - max(a, 256 * j)
    assert (W.sum(axis=1) == s).all()
    return W


def plane(g, s):
    """Rule 6: level s of the gray plane g, uint8 [h_l, w_l]."""
    s = int(s)
    h, w = g.shape
    if level_side(h, s) == 0 or level_side(w, s) == 0:
        return np.zeros((level_side(h, s), level_side(w, s)), dtype=np.uint8)
    acc = overlaps(h, s) @ g.astype(np.int64) @ overlaps(w, s).T
    assert acc.max() < 2 ** 31
    return ((acc + s * s // 2) // (s * s)).astype(np.uint8)


def planes(img, scales):
    """The planes of levels 1 .. of an image (rule 1 first)."""
    g = oc.gray(img)
    return [plane(g, s) for s in np.asarray(scales).tolist()[1:]]


def back_map(x, s):
    """Rule 8: level coordinates (integer array) -> float32 level-0 coordinates."""
    num = (2 * x.astype(np.int64) + 1) * int(s) - 256
    return (num.astype(np.float64) / 512.0).astype(np.float32)             # num / 512 is exact in float64: one rounding


def restate_pyramid(img, scales, quotas, threshold=20, nbytes=32, pattern=None):
    """Rules 1 - 8 for one image -> dict(kps, desc, score, bin, level, size, found = per-level list; xy_level = the keypoints in
    their level's own pixels, int64, before rule 8's map)."""
    scales = np.asarray(scales).tolist()
    levels = [img] + planes(img, scales)
    parts, found = [], []
    for l, (s, lv) in enumerate(zip(scales, levels)):
        if lv.shape[0] == 0 or lv.shape[1] == 0:
            found.append(0)
            continue
        r = oc.restate(lv, n_features=int(quotas[l]), threshold=threshold, nbytes=nbytes, pattern=pattern)
        found.append(r["found"])
        k = r["kps"].astype(np.int64)
        r["xy_level"] = k
        r["kps"] = np.stack([back_map(k[:, 0], s), back_map(k[:, 1], s)], axis=1).reshape(-1, 2)
        r["level"] = np.full(len(k), l, dtype=np.int32)
        r["size"] = np.full(len(k), np.float32(PATCH * s) / np.float32(256), dtype=np.float32)
        parts.append(r)
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("kps", "desc", "score", "bin", "level", "size", "xy_level")}
    out["found"] = found
    return out


def host_planes(lib, img, scales):
    """rwh_host_orb_pyramid on one image -> (status, list of the planes of levels 1 ..), with a canary behind the last plane."""
    img = np.ascontiguousarray(img)
    sc = np.ascontiguousarray(scales, dtype=np.int32)
    c = 1 if img.ndim == 2 else img.shape[2]
    need = lib.rwh_orb_pyramid_bytes(img.shape[0], img.shape[1], sc.ctypes.data, len(sc))
    if need < 0:
        return int(need), []
    buf = np.full(need + 16, 0xA5, dtype=np.uint8)
    st = lib.rwh_host_orb_pyramid(img.ctypes.data, img.shape[0], img.shape[1], c, sc.ctypes.data, len(sc), buf.ctypes.data, need)
    assert (buf[need:] == 0xA5).all()
    out, at = [], 0
    for s in sc.tolist()[1:]:
        hl, wl = level_side(img.shape[0], s), level_side(img.shape[1], s)
        out.append(buf[at:at + hl * wl].reshape(hl, wl).copy())
        at += hl * wl
    assert at == need
    return st, out


def host_extract_pyramid(lib, img, scales, quotas, threshold=20, nbytes=32, pattern=None):
    """rwh_host_orb_extract_pyramid on one image -> (status, dict as `restate_pyramid` gives it)."""
    bin_table, rot = oc.tables(nbytes, pattern)
    rot = np.ascontiguousarray(rot)
    img = np.ascontiguousarray(img)
    sc, qt = np.ascontiguousarray(scales, dtype=np.int32), np.ascontiguousarray(quotas, dtype=np.int32)
    c = 1 if img.ndim == 2 else img.shape[2]
    room = max(int(np.maximum(qt, 0).sum()), 1)
    kps, size = np.full((room, 2), -7, dtype=np.float32), np.full(room, -7, dtype=np.float32)
    desc = np.full((room, nbytes), 0xAA, dtype=np.uint8)
    score, bins, level = (np.full(room, -7, dtype=np.int32) for _ in range(3))
    count, found = np.full(1, -7, dtype=np.int32), np.full(len(sc), -7, dtype=np.int32)
    st = lib.rwh_host_orb_extract_pyramid(img.ctypes.data, img.shape[0], img.shape[1], c, threshold, sc.ctypes.data, qt.ctypes.data, len(sc),
                                          bin_table.ctypes.data, rot.ctypes.data, nbytes, kps.ctypes.data, desc.ctypes.data,
                                          score.ctypes.data, bins.ctypes.data, level.ctypes.data, size.ctypes.data, count.ctypes.data,
                                          found.ctypes.data)
    n = max(int(count[0]), 0)
    return st, dict(kps=kps[:n], desc=desc[:n], score=score[:n], bin=bins[:n], level=level[:n], size=size[:n], found=found.tolist())


KEYS = ("kps", "desc", "score", "bin", "level", "size")


def same(a, b):
    return (list(a["found"]) == list(b["found"]) and
            all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in KEYS))


# ---- the cases ----
def plane_images():
    """(name, image) of the CPU plane cases."""
    return [("97x131 rgb", oc.random_image(97, 131, 11)), ("40x203 gray", oc.random_image(40, 203, 12, channels=1)),
            ("33x33", oc.random_image(33, 33, 13, channels=1))]


def gpu_images():
    """The GPU batch: level widths that are no multiple of the tile or of 4, windows that cross the right and the bottom edge, a
    level that falls below 33 px."""
    return [oc.random_image(150, 203, 21), oc.random_image(67, 90, 22, channels=1), oc.random_image(33, 300, 23, channels=4)]


def textured(h=256, w=320, seed=3):
    """A gray image of seeded random rectangles and discs on a mid-gray ground: corners at many sizes."""
    rng = np.random.RandomState(seed)
    img = np.full((h, w), 110, dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for k in range(160):
        x, y, v = int(rng.randint(0, w)), int(rng.randint(0, h)), int(rng.randint(0, 256))
        a, b = int(rng.randint(4, 30)), int(rng.randint(4, 30))
        if k % 2:
            img[max(y - b, 0):y + b, max(x - a, 0):x + a] = v
        else:
            img[(xx - x) ** 2 + (yy - y) ** 2 <= a * a] = v
    return img


def shrink_bilinear(img, factor=1.5):
    """img resampled by 1 / factor, plain bilinear at pixel centres: output pixel X samples the source at (X + 0.5) factor - 0.5.
    Not the rule's area average, and off the level grid."""
    h, w = img.shape
    H, W = int(h / factor), int(w / factor)
    sy = np.clip((np.arange(H) + 0.5) * factor - 0.5, 0, h - 1)
    sx = np.clip((np.arange(W) + 0.5) * factor - 0.5, 0, w - 1)
    y0, x0 = np.minimum(sy.astype(int), h - 2), np.minimum(sx.astype(int), w - 2)
    fy, fx = (sy - y0)[:, None], (sx - x0)[None, :]
    f = img.astype(np.float64)
    top = f[y0][:, x0] * (1 - fx) + f[y0][:, x0 + 1] * fx
    bot = f[y0 + 1][:, x0] * (1 - fx) + f[y0 + 1][:, x0 + 1] * fx
    return np.rint(top * (1 - fy) + bot * fy).astype(np.uint8)


def agreeing(kps_a, kps_b, train, factor=1.5, tol=3.0):
    """How many matches (query i -> train[i]) agree with the known map x_B = (x_A + 0.5) / factor - 0.5 within tol px."""
    q = np.nonzero(train >= 0)[0]
    want = (kps_a[q].astype(np.float64) + 0.5) / factor - 0.5
    d = want - kps_b[train[q]].astype(np.float64)
    err = np.hypot(d[:, 0], d[:, 1])
    return int((err <= tol).sum())


def layout(images, scales, gap=0):
    """The buffer and table of rwh_orb_pyramid_batched for a list of images: (head uint8 [bytes] = the images concatenated, table
    int64 [n * n_levels, 5], planes_offset, images_bytes, spans) -- the planes follow the head after `gap` unused bytes, in (image,
    level) order; spans[i][l - 1] = (offset, h_l, w_l) of level l of image i; a level without pixels is the row (0, 0, 0, 0, 1)."""
    scales = np.asarray(scales).tolist()
    head = np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images])
    rows, spans, src, gray, at = [], [], 0, 0, head.size + gap
    for im in images:
        h, w, c = im.shape[0], im.shape[1], 1 if im.ndim == 2 else im.shape[2]
        rows.append((src, gray, h, w, c))
        src += im.size
        gray += h * w
        spans.append([])
        for s in scales[1:]:
            hl, wl = level_side(h, s), level_side(w, s)
            spans[-1].append((at, hl, wl))
            rows.append((at, gray, hl, wl, 1) if hl and wl else (0, 0, 0, 0, 1))
            at += hl * wl
            gray += hl * wl
    return head, np.array(rows, dtype=np.int64), head.size, at, spans
