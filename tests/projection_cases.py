"""The projection rule (include/rwh.h: the sequence compositor on a cylindrical or spherical canvas) restated in numpy -- its
rectangles, ray tables, Sample and Coverage, and on top of them paste, feather, the overlap statistics and the multi-band blend --,
the drivers of the host twins and of the device calls, and the cases that tests/test_sequence_projection_cpu.py and
tests/test_sequence_projection_gpu.py share.  The restatement forms X, Y and W as `M @ rays`: the BLAS product of a 3 x 3 matrix
runs k in order with fused multiply-adds, which is the rule's one contraction; `exact_rows` restates it with exact rationals and a
CPU test holds the product to it."""
from fractions import Fraction

import numpy as np

import multiband_cases as mc
import sequence_cases as sc

PASTE, FEATHER = sc.PASTE, sc.FEATHER
SURFACES = ("cylindrical", "spherical")


# ---- the rule ----
def camera(shape, f):
    return np.array([[f, 0.0, (shape[1] - 1) / 2.0], [0.0, f, (shape[0] - 1) / 2.0], [0.0, 0.0, 1.0]])


def orient(Gs):
    return [np.asarray(G, dtype=np.float64) * np.sign(np.linalg.det(G)) for G in Gs]


def perimeter(h, w):
    pts = [(x, 0) for x in range(w - 1)] + [(w - 1, y) for y in range(h - 1)] + [(x, h - 1) for x in range(w - 1, 0, -1)]
    pts += [(0, y) for y in range(h - 1, 0, -1)]
    return np.array([[x, y, 1.0] for x, y in pts]).T


def surface(rays, kind, f):
    theta = np.arctan2(rays[0], rays[2])
    hyp = np.hypot(rays[0], rays[2])
    return f * theta, f * (rays[1] / hyp if kind == "cylindrical" else np.arctan2(rays[1], hyp))


def rectangles(shapes, Gs, anchor, kind, f):
    """The rule's rectangles in surface pixels (no refusals: the cases are made to be taken)."""
    kinv = np.linalg.inv(camera(shapes[anchor], f))
    out = []
    for s, G in zip(shapes, Gs):
        u, v = surface(kinv @ (G @ perimeter(s[0], s[1])), kind, f)
        mx, my = int(np.floor(u.min())) - 1, int(np.floor(v.min())) - 1
        out.append((mx, my, int(np.ceil(u.max())) + 1 - mx + 1, int(np.ceil(v.max())) + 1 - my + 1))
    return out


def ray_tables(kind, f, origin, size):
    u = (origin[0] + np.arange(size[1], dtype=np.float64)) / f
    t = (origin[1] + np.arange(size[0], dtype=np.float64)) / f
    col = np.stack([np.sin(u), np.cos(u)], axis=1)
    row = np.stack([t, np.ones_like(t)], axis=1) if kind == "cylindrical" else np.stack([np.sin(t), np.cos(t)], axis=1)
    return np.ascontiguousarray(col), np.ascontiguousarray(row)


def matrices(shapes, Gs, anchor, f):
    K = camera(shapes[anchor], f)
    return np.stack([K if i == anchor else np.linalg.inv(G) @ K for i, G in enumerate(Gs)])


def rays_of(col, row):
    """[3, fh, fw]: r0 = col.sin * row[1], r1 = row[0], r2 = col.cos * row[1]."""
    return np.stack([col[None, :, 0] * row[:, None, 1], np.broadcast_to(row[:, None, 0], (len(row), len(col))), col[None, :, 1] * row[:, None, 1]])


def exact_rows(M, rays):
    """X, Y, W of the rule with exact rationals: fma(m2, r2, fma(m1, r1, m0 * r0)), every step rounded once.  rays [3, k]."""
    out = np.zeros((3, rays.shape[1]))
    for r in range(3):
        m = [Fraction(float(v)) for v in M[r]]
        for k in range(rays.shape[1]):
            a = float(m[0] * Fraction(float(rays[0, k])))
            a = float(m[1] * Fraction(float(rays[1, k])) + Fraction(a))
            out[r, k] = float(m[2] * Fraction(float(rays[2, k])) + Fraction(a))
    return out


def geometry(images, Gs, anchor, kind, f, rects=None):
    """-> (rects in CANVAS coordinates, origin, (fh, fw), M, col, row).  rects: "canvas" makes every rectangle the whole canvas."""
    shapes = [im.shape for im in images]
    Gs = orient(Gs)
    surf = rectangles(shapes, Gs, anchor, kind, f)
    origin, size = sc.canvas_of(surf)
    own = [(r[0] - origin[0], r[1] - origin[1], r[2], r[3]) for r in surf]
    if rects == "canvas":
        own = [(0, 0, size[1], size[0])] * len(images)
    col, row = ray_tables(kind, f, origin, size)
    return own, origin, size, matrices(shapes, Gs, anchor, f), col, row


def planes(images, Gs, anchor, kind, f, gains=None, rects=None):
    """Every image over the whole canvas: -> ((fh, fw), cover bool [n, fh, fw], v float64 [n, fh, fw, 3], g float64 [n, fh, fw])."""
    own, _, (fh, fw), M, col, row = geometry(images, Gs, anchor, kind, f, rects)
    n = len(images)
    rays = rays_of(col, row).reshape(3, -1)
    cover, val, gw = np.zeros((n, fh, fw), dtype=bool), np.zeros((n, fh, fw, 3)), np.zeros((n, fh, fw))
    cy, cx = np.mgrid[0:fh, 0:fw]
    for i, img in enumerate(images):
        h, w, _ = img.shape
        with np.errstate(all="ignore"):
            z = M[i] @ rays
            sx, sy, W = (z[0] / z[2]).reshape(fh, fw), (z[1] / z[2]).reshape(fh, fw), z[2].reshape(fh, fw)
            valid = (W > 0) & (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
        r = own[i]
        valid &= (cx >= r[0]) & (cx < r[0] + r[2]) & (cy >= r[1]) & (cy < r[1] + r[3])
        sx, sy = np.where(valid, sx, 0.0), np.where(valid, sy, 0.0)
        ix, iy = sx.astype(np.int32), sy.astype(np.int32)
        ix1, iy1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
        src = img.astype(np.float64)
        src[0, 0] = 0.0
        fx, fy = (sx - ix)[:, :, None], (sy - iy)[:, :, None]
        top = src[iy, ix] * (1 - fx) + src[iy, ix1] * fx
        bot = src[iy1, ix] * (1 - fx) + src[iy1, ix1] * fx
        v = top * (1 - fy) + bot * fy
        if gains is not None:
            v = np.minimum(v * float(gains[i]), 255.0)
        cover[i], val[i] = valid, v
        gw[i] = np.minimum(np.minimum(sx, (w - 1) - sx), np.minimum(sy, (h - 1) - sy)) + 1.0
    return (fh, fw), cover, val, gw


def restate(images, Gs, anchor=0, kind="cylindrical", f=40.0, blend=PASTE, order=None, gains=None, rects=None):
    """-> canvas uint8 [fh, fw, 3] of the projection rule under paste or feather."""
    n = len(images)
    (fh, fw), cover, val, gw = planes(images, Gs, anchor, kind, f, gains, rects)
    can = np.zeros((fh, fw, 3), dtype=np.uint8)
    if blend == PASTE:
        for i in reversed(sc.default_order(n, anchor) if order is None else list(order)):
            can[cover[i]] = val[i][cover[i]].astype(np.int32).astype(np.uint8)
        return can
    num, den = np.zeros((fh, fw, 3)), np.zeros((fh, fw))
    for i in range(n):
        num[cover[i]] += gw[i][cover[i]][:, None] * val[i][cover[i]]
        den[cover[i]] += gw[i][cover[i]]
    hit = den > 0
    can[hit] = (num[hit] / den[hit][:, None]).astype(np.int32).astype(np.uint8)
    return can


def stats(images, Gs, anchor, kind, f, stride, rects=None):
    """The gain rule's two tables on the curved canvas -> (count, sum) uint64 [n, n]."""
    _, cover, val, _ = planes(images, Gs, anchor, kind, f, rects=rects)
    L = val.astype(np.int32).astype(np.uint8).astype(np.int64).sum(axis=3)
    cover, L = cover[:, ::stride, ::stride], L[:, ::stride, ::stride]
    n = len(images)
    count, total = np.zeros((n, n), dtype=np.uint64), np.zeros((n, n), dtype=np.uint64)
    for i in range(n):
        for j in range(n):
            both = cover[i] & cover[j]
            count[i, j], total[i, j] = both.sum(), L[i][both].sum()
    return count, total


def multiband(images, Gs, anchor=0, kind="cylindrical", f=40.0, bands=2, gains=None):
    """The multi-band rule on the planes of the projection rule (tests/multiband_cases.py's restatement from the planes onward)."""
    K, n = bands, len(images)
    (fh, fw), cover, val, gw = planes(images, Gs, anchor, kind, f, gains)
    byt = np.where(cover[:, :, :, None], val.astype(np.int32).astype(np.uint8).astype(np.int64), 0)
    gw = np.where(cover, gw, -np.inf)
    PH, PW = -(-fh // 2 ** K) * 2 ** K, -(-fw // 2 ** K) * 2 ** K
    anyone = cover.any(axis=0)
    winner = np.where(anyone, np.argmax(gw, axis=0), -1)
    P = np.zeros((PH, PW, 3), dtype=np.int64)
    P[:fh, :fw] = np.where(anyone[:, :, None], np.take_along_axis(byt, np.maximum(winner, 0)[None, :, :, None], axis=0)[0], 0)
    num = [np.zeros((PH >> l, PW >> l, 3), dtype=np.int64) for l in range(K + 1)]
    den = [np.zeros((PH >> l, PW >> l, 1), dtype=np.int64) for l in range(K + 1)]
    for i in range(n):
        I = P.copy()
        I[:fh, :fw][cover[i]] = byt[i][cover[i]]
        Wt = np.zeros((PH, PW, 1), dtype=np.int64)
        Wt[:fh, :fw, 0][winner == i] = mc.ONE
        G, Ws = [I], [Wt]
        for l in range(K):
            G.append(mc.down(G[l]))
            Ws.append(mc.down(Ws[l]))
        for l in range(K + 1):
            L = G[l] - mc.up(G[l + 1]) if l < K else G[l]
            num[l] += L * Ws[l]
            den[l] += Ws[l]
    R = None
    for l in range(K, -1, -1):
        B = np.where(den[l] > 0, np.sign(num[l]) * ((np.abs(num[l]) + den[l] // 2) // np.maximum(den[l], 1)), 0)
        R = B if R is None else B + mc.up(R)
    can = np.zeros((fh, fw, 3), dtype=np.uint8)
    can[anyone] = np.clip(R[:fh, :fw], 0, 255)[anyone].astype(np.uint8)
    return can


# ---- the library's entry points ----
def tables(images, Gs, anchor, kind, f, order=None, rects=None):
    own, origin, size, M, col, row = geometry(images, Gs, anchor, kind, f, rects)
    n = len(images)
    hw = np.array([[im.shape[0], im.shape[1]] for im in images], dtype=np.int32)
    order = np.array(sc.default_order(n, anchor) if order is None else order, dtype=np.int32)
    return dict(hw=hw, m=np.ascontiguousarray(M.reshape(n, 9)), rects=np.array(own, dtype=np.int32), order=order, origin=origin, size=size,
                n=n, col=col, row=row)


def _gains_ptr(gains):
    g = None if gains is None else np.ascontiguousarray(gains, dtype=np.float64)
    return g, (None if g is None else g.ctypes.data)


def host_twin(lib, images, Gs, anchor=0, kind="cylindrical", f=40.0, blend=PASTE, order=None, rows=None, gains=None, rects=None, tweak=None,
              t=None):
    """rwh_host_stitch_sequence_proj -> (status, canvas), the canvas guarded.  tweak(t, ptrs): may spoil the tables before the call;
    t: tables to use as they are (Gs, anchor, kind, f, order and rects are then not read)."""
    images = [np.ascontiguousarray(im) for im in images]
    t = tables(images, Gs, anchor, kind, f, order, rects) if t is None else t
    fh, fw = t["size"]
    can, check = sc.guarded_canvas(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    if tweak is not None:
        tweak(t, ptrs)
    r0, r1 = (0, fh) if rows is None else rows
    g, gp = _gains_ptr(gains)
    st = lib.rwh_host_stitch_sequence_proj(ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, t["n"],
                                           t["order"].ctypes.data, blend, None if t["col"] is None else t["col"].ctypes.data,
                                           None if t["row"] is None else t["row"].ctypes.data, can.ctypes.data, fh, fw, r0, r1, gp)
    check()
    return st, can


def host(lib, *a, **k):
    st, can = host_twin(lib, *a, **k)
    assert st == 0
    return can


def host_stats(lib, images, Gs, anchor=0, kind="cylindrical", f=40.0, stride=1, rects=None):
    import gain_cases as gc
    images = [np.ascontiguousarray(im) for im in images]
    t = tables(images, Gs, anchor, kind, f, rects=rects)
    fh, fw = t["size"]
    _, count, total, check = gc.guarded_tables(t["n"])
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    st = lib.rwh_host_sequence_overlap_stats_proj(ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, t["n"],
                                                  t["col"].ctypes.data, t["row"].ctypes.data, fh, fw, stride, count.ctypes.data, total.ctypes.data)
    check()
    assert st == 0
    return count.copy(), total.copy()


def host_multiband(lib, images, Gs, anchor=0, kind="cylindrical", f=40.0, bands=2, gains=None):
    images = [np.ascontiguousarray(im) for im in images]
    t = tables(images, Gs, anchor, kind, f)
    fh, fw = t["size"]
    can, check = sc.guarded_canvas(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    g, gp = _gains_ptr(gains)
    st = lib.rwh_host_stitch_multiband_proj(ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, t["n"], bands, gp,
                                            t["col"].ctypes.data, t["row"].ctypes.data, can.ctypes.data, fh, fw)
    check()
    assert st == 0
    return can


def device_tables(t):
    import torch
    return torch.from_numpy(t["col"]).cuda(), torch.from_numpy(t["row"]).cuda()


def device(images, Gs, anchor=0, kind="cylindrical", f=40.0, blend=PASTE, order=None, rows=None, gains=None, on=None, t=None):
    """kernels.stitch_sequence on a curved canvas, into a guarded device canvas -> the canvas in numpy.  t: as host_twin's."""
    from ransac_with_homography_amd import kernels
    t = tables(images, Gs, anchor, kind, f, order) if t is None else t
    can, fetch = sc.guarded_device_canvas(*t["size"])
    kernels.stitch_sequence_on(sc.upload(images) if on is None else on, sc.geometry(t, device_tables(t)), t["order"], blend,
                            rows=rows, out=can, gains=gains)
    return fetch()


def device_stats(images, Gs, anchor=0, kind="cylindrical", f=40.0, stride=1):
    from ransac_with_homography_amd import kernels
    t = tables(images, Gs, anchor, kind, f)
    tabs = kernels.sequence_overlap_tables_on(sc.upload(images), sc.geometry(t, device_tables(t)), stride).cpu().numpy().view(np.uint64)
    return tabs[0], tabs[1]


def device_multiband(images, Gs, anchor=0, kind="cylindrical", f=40.0, bands=2, gains=None):
    from ransac_with_homography_amd import kernels
    t = tables(images, Gs, anchor, kind, f)
    can, fetch = sc.guarded_device_canvas(*t["size"])
    kernels.stitch_sequence_multiband_on(sc.upload(images), sc.geometry(t, device_tables(t)), bands, gains=gains, out=can)
    return fetch()


# ---- the cases ----
def rotation(yaw, pitch=0.0, roll=0.0):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    Rz = np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]])
    return Ry @ Rx @ Rz


def pair_homography(shape_i, shape_j, f, R, persp=None):
    """Image j into image i for a camera turned by R between them: K_i R inv(K_j), plus a small perspective part."""
    H = camera(shape_i, f) @ R @ np.linalg.inv(camera(shape_j, f))
    if persp is not None:
        H = H @ (np.eye(3) + np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [persp[0], persp[1], 0.0]]))
    return H


def sweep(n, seed, f=40.0, yaw=0.33, h=24, w=32):
    """n images of about h x w (sizes differ), turned by about `yaw` per image with some pitch and roll and a small perspective
    perturbation -> (images, Hs): at f = 40 the curvature is strong."""
    rng = np.random.default_rng(seed)
    images = [sc.random_image(h + int(rng.integers(-2, 3)), w + int(rng.integers(-3, 4)), seed * 100 + i) for i in range(n)]
    Hs = [pair_homography(images[i].shape, images[i + 1].shape, f,
                          rotation(yaw + rng.uniform(-0.03, 0.03), rng.uniform(-0.06, 0.06), rng.uniform(-0.05, 0.05)), rng.uniform(-2e-4, 2e-4, 2))
          for i in range(n - 1)]
    return images, Hs


def general_cases():
    """(name, images, Gs, anchor, order, f)."""
    out = [("n1", [sc.random_image(9, 11, 1)], [np.eye(3)], 0, None, 40.0)]
    im3, hs3 = sweep(3, 3)
    out.append(("n3 anchor 0", im3, sc.chain(hs3, 0), 0, None, 40.0))
    out.append(("n3 anchor 1 reversed", im3, sc.chain(hs3, 1), 1, sc.default_order(3, 1)[::-1], 40.0))
    im4, hs4 = sweep(4, 4, f=37.5)
    out.append(("n4 negated", im4, [G if i != 2 else -G for i, G in enumerate(sc.chain(hs4, 1))], 1, None, 37.5))
    im5, hs5 = sweep(5, 5, yaw=0.3)
    out.append(("n5 order", im5, sc.chain(hs5, 2), 2, [4, 0, 2, 3, 1], 40.0))
    return out


def antipodal_pair(f=40.0):
    """Two images 170 degrees apart in yaw, the far one narrow enough to end before the seam: its mirrored ghost (rays with
    W <= 0) lies 10 degrees off the anchor's axis, inside the anchor's image."""
    images = [sc.random_image(24, 32, 170), sc.random_image(24, 12, 171)]
    return images, [np.eye(3), pair_homography(images[0].shape, images[1].shape, f, rotation(np.deg2rad(170.0)))]


SEVEN = dict(n=7, h=120, w=160, f=300.0, yaw=np.deg2rad(20.0))


def texture(theta, t):
    """[..., 3] float64: the analytic texture of the geometry test, 128 + 60 sin(3 theta + phi_k) cos(2 t)."""
    return np.stack([128.0 + 60.0 * np.sin(3.0 * theta + phi) * np.cos(2.0 * t) for phi in (0.0, 1.0, 2.0)], axis=-1)


def seven_views():
    """The issue's setup: seven 160 x 120 views of a camera with f = 300 turning 20 degrees per image, pitch 0.01 i and roll 0.005 i;
    image bytes are rint(T(theta, t)) on each pixel's ray (t the cylinder's height).  -> (images, Hs, Rs): Hs[i] maps image i + 1
    into image i exactly, Rs[i] is camera i's rotation in the anchor's (camera 0's) frame."""
    n, h, w, f = SEVEN["n"], SEVEN["h"], SEVEN["w"], SEVEN["f"]
    K = camera((h, w), f)
    Rs = [rotation(SEVEN["yaw"] * i, 0.01 * i, 0.005 * i) for i in range(n)]
    yy, xx = np.mgrid[0:h, 0:w]
    pix = np.stack([xx.ravel(), yy.ravel(), np.ones(h * w)]).astype(np.float64)
    images = []
    for R in Rs:
        r = R @ (np.linalg.inv(K) @ pix)
        theta, t = np.arctan2(r[0], r[2]), r[1] / np.hypot(r[0], r[2])
        images.append(np.rint(texture(theta, t)).astype(np.uint8).reshape(h, w, 3))
    Hs = [K @ Rs[i].T @ Rs[i + 1] @ np.linalg.inv(K) for i in range(n - 1)]
    return images, Hs, Rs


def wide_case(kind):
    """Three 10 x 260 images at f = 300, 0.6 rad apart: a canvas more than 513 columns wide and more than 9 rows high -> (images,
    tables): the whole canvas, of which `crop` cuts the launch-edge canvases."""
    f = 300.0
    images = [sc.random_image(10, 260, 900 + i) for i in range(3)]
    Hs = [pair_homography(images[i].shape, images[i + 1].shape, f, rotation(0.6, 0.004 * (i + 1), 0.003)) for i in range(2)]
    return images, tables(images, sc.chain(Hs, 1), 1, kind, f)


def crop(images, t, x0, y0, fw, fh):
    """Canvas columns [x0, x0 + fw) and rows [y0, y0 + fh) of tables `t` as a canvas of its own: the tables' slices, the rectangles
    clipped to the window (Coverage is "inside the rectangle and valid", so the window shows what the whole canvas shows there),
    images that do not meet it dropped -> (images, tables)."""
    keep, rects = [], []
    for i, (mx, my, wt, ht) in enumerate(t["rects"].tolist()):
        a, b, c, d = max(mx, x0), max(my, y0), min(mx + wt, x0 + fw), min(my + ht, y0 + fh)
        if a < c and b < d:
            keep.append(i)
            rects.append((a - x0, b - y0, c - a, d - b))
    assert keep
    return [images[i] for i in keep], dict(hw=np.ascontiguousarray(t["hw"][keep]), m=np.ascontiguousarray(t["m"][keep]),
                                          rects=np.array(rects, dtype=np.int32), order=np.arange(len(keep), dtype=np.int32)[::-1].copy(),
                                          origin=(t["origin"][0] + x0, t["origin"][1] + y0), size=(fh, fw), n=len(keep),
                                          col=np.ascontiguousarray(t["col"][x0:x0 + fw]), row=np.ascontiguousarray(t["row"][y0:y0 + fh]))


def strip(n, h, w, f, step, pitch=0.0007):
    """n images of h x w from a camera with focal f turning `step` radians per image (a little pitch and roll with it) -> (images, Gs)
    with anchor 0."""
    images = [sc.random_image(h, w, 7000 + 10 * n + i) for i in range(n)]
    H = pair_homography((h, w), (h, w), f, rotation(step, pitch, 0.0005))
    return images, sc.chain([H] * (n - 1), 0)


def scene_views(f=400.0, yaws=(-0.15, 0.0, 0.15), h=160, w=200):
    """Rotated views of sc.scene(): the scene is what a camera with focal f sees straight ahead, view i what it sees turned by
    yaws[i] (and a little pitch and roll), resampled bilinearly -> (views uint8 [h, w, 3], Hs true pairwise, view i + 1 into view i)."""
    scene = sc.scene().astype(np.float64)
    Ks, Kv = camera(scene.shape, f), camera((h, w), f)
    Rs = [rotation(y, 0.01 * i, 0.008 * i) for i, y in enumerate(yaws)]
    yy, xx = np.mgrid[0:h, 0:w]
    pix = np.stack([xx.ravel(), yy.ravel(), np.ones(h * w)]).astype(np.float64)
    views = []
    for R in Rs:
        q = Ks @ R @ np.linalg.inv(Kv) @ pix
        sx, sy = q[0] / q[2], q[1] / q[2]
        assert sx.min() >= 0 and sx.max() <= scene.shape[1] - 1 and sy.min() >= 0 and sy.max() <= scene.shape[0] - 1
        ix, iy = np.minimum(sx.astype(np.int64), scene.shape[1] - 2), np.minimum(sy.astype(np.int64), scene.shape[0] - 2)
        fx, fy = (sx - ix)[:, None], (sy - iy)[:, None]
        top = scene[iy, ix] * (1 - fx) + scene[iy, ix + 1] * fx
        bot = scene[iy + 1, ix] * (1 - fx) + scene[iy + 1, ix + 1] * fx
        views.append(np.rint(top * (1 - fy) + bot * fy).astype(np.uint8).reshape(h, w, 3))
    return views, [Kv @ Rs[i].T @ Rs[i + 1] @ np.linalg.inv(Kv) for i in range(len(yaws) - 1)]
