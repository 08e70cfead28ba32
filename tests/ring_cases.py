"""The ring rule (include/rwh.h: the sequence compositor on a cylindrical or spherical canvas that closes the circle) restated in
numpy on top of tests/projection_cases.py -- the period, the rectangles on the unwrapped angle, Coverage modulo the period, and on
top of them paste, feather, the overlap statistics and the multi-band blend with periodic reduce and expand --, the drivers of the
host twins and of the device calls, and the cases that tests/test_sequence_ring_cpu.py and tests/test_sequence_ring_gpu.py share.
Everything works on TABLES (the dict of `tables`): rolled and cropped tables are restated by the same code."""
import numpy as np

import multiband_cases as mc
import projection_cases as pc
import sequence_cases as sc

PASTE, FEATHER = sc.PASTE, sc.FEATHER
SURFACES = pc.SURFACES
TILE = 256


# ---- the rule ----
def period(f):
    return TILE * max(1, int(np.rint(2.0 * np.pi * f / TILE)))


def wrapped(x):
    return (x + np.pi) % (2.0 * np.pi) - np.pi


def rectangles(shapes, Gs, anchor, kind, f, P):
    """The rule's rectangles (lo, my, wt, ht) in UNWRAPPED surface pixels (no refusals: the cases are made to be taken)."""
    rho = P / (2.0 * np.pi)
    kinv = np.linalg.inv(pc.camera(shapes[anchor], f))
    out = []
    for s, G in zip(shapes, Gs):
        rays = kinv @ (G @ pc.perimeter(s[0], s[1]))
        theta = np.arctan2(rays[0], rays[2])
        tu = [theta[0]]
        for k in range(len(theta) - 1):
            tu.append(tu[-1] + wrapped(theta[k + 1] - theta[k]))
        u, v = rho * np.array(tu), pc.surface(rays, kind, rho)[1]
        lo, my = int(np.floor(u.min())) - 1, int(np.floor(v.min())) - 1
        out.append((lo, my, min(int(np.ceil(u.max())) + 1 - lo + 1, P), int(np.ceil(v.max())) + 1 - my + 1))
    return out


def tables(images, Gs, anchor, kind, f, P=None, order=None, rects=None):
    """The tables of a ring call: rects in CANVAS coordinates (mx in [0, P), mx + wt may pass P), origin (-P / 2, oy), size (fh, P),
    M with the focal f, the ray tables with the radius P / (2 pi).  rects: "canvas" makes every rectangle the whole canvas."""
    n = len(images)
    shapes = [im.shape for im in images]
    P = period(f) if P is None else P
    Gs = pc.orient(Gs)
    surf = rectangles(shapes, Gs, anchor, kind, f, P)
    ox, oy = -(P // 2), min(r[1] for r in surf)
    fh = max(r[1] + r[3] for r in surf) - oy
    own = [(0 if r[2] == P else (r[0] - ox) % P, r[1] - oy, r[2], r[3]) for r in surf]
    if rects == "canvas":
        own = [(0, 0, P, fh)] * n
    col, row = pc.ray_tables(kind, P / (2.0 * np.pi), (ox, oy), (fh, P))
    hw = np.array([[s[0], s[1]] for s in shapes], dtype=np.int32)
    order = np.array(sc.default_order(n, anchor) if order is None else order, dtype=np.int32)
    return dict(hw=hw, m=np.ascontiguousarray(pc.matrices(shapes, Gs, anchor, f).reshape(n, 9)), rects=np.array(own, dtype=np.int32),
                order=order, origin=(ox, oy), size=(fh, P), n=n, col=col, row=row)


def roll(t, s):
    """Consequence (b): the column table rolled by s columns and every mx moved to (mx + s) mod P."""
    P = t["size"][1]
    rects = t["rects"].copy()
    rects[:, 0] = (rects[:, 0] + s) % P
    return dict(t, rects=rects, col=np.ascontiguousarray(np.roll(t["col"], s, axis=0)))


def crop_rows(images, t, y0, fh):
    """Canvas rows [y0, y0 + fh) of tables `t` as a ring canvas of its own (projection_cases.crop, rows only: the ring keeps all
    its columns) -> (images, tables)."""
    keep, rects = [], []
    for i, (mx, my, wt, ht) in enumerate(t["rects"].tolist()):
        b, d = max(my, y0), min(my + ht, y0 + fh)
        if b < d:
            keep.append(i)
            rects.append((mx, b - y0, wt, d - b))
    assert keep
    return [images[i] for i in keep], dict(hw=np.ascontiguousarray(t["hw"][keep]), m=np.ascontiguousarray(t["m"][keep]),
                                          rects=np.array(rects, dtype=np.int32), order=np.arange(len(keep), dtype=np.int32)[::-1].copy(),
                                          origin=(t["origin"][0], t["origin"][1] + y0), size=(fh, t["size"][1]), n=len(keep),
                                          col=t["col"], row=np.ascontiguousarray(t["row"][y0:y0 + fh]))


def planes(images, t, gains=None):
    """Every image over the whole canvas: -> (cover bool [n, fh, P], v float64 [n, fh, P, 3], g float64 [n, fh, P]).  Coverage is
    the ring rule's: ((cx - mx) mod P) < wt, the rows and `valid` as in the projection rule."""
    fh, P = t["size"]
    n = len(images)
    rays = pc.rays_of(t["col"], t["row"]).reshape(3, -1)
    cover, val, gw = np.zeros((n, fh, P), dtype=bool), np.zeros((n, fh, P, 3)), np.zeros((n, fh, P))
    cy, cx = np.mgrid[0:fh, 0:P]
    for i, img in enumerate(images):
        h, w, _ = img.shape
        with np.errstate(all="ignore"):
            z = t["m"][i].reshape(3, 3) @ rays
            sx, sy, W = (z[0] / z[2]).reshape(fh, P), (z[1] / z[2]).reshape(fh, P), z[2].reshape(fh, P)
            valid = (W > 0) & (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
        mx, my, wt, ht = (int(v) for v in t["rects"][i])
        valid &= (np.mod(cx - mx, P) < wt) & (cy >= my) & (cy < my + ht)
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
    return cover, val, gw


def unbounded_cover(images, t):
    """`valid` of every image over the whole canvas, no rectangle: what the rectangles have to contain."""
    return planes(images, dict(t, rects=np.array([(0, 0, t["size"][1], t["size"][0])] * t["n"], dtype=np.int32)))[0]


def restate(images, t, blend=PASTE, gains=None):
    """-> canvas uint8 [fh, P, 3] of the ring rule under paste (in t["order"]) or feather."""
    n = len(images)
    fh, P = t["size"]
    cover, val, gw = planes(images, t, gains)
    can = np.zeros((fh, P, 3), dtype=np.uint8)
    if blend == PASTE:
        for i in reversed([int(v) for v in t["order"]]):
            can[cover[i]] = val[i][cover[i]].astype(np.int32).astype(np.uint8)
        return can
    num, den = np.zeros((fh, P, 3)), np.zeros((fh, P))
    for i in range(n):
        num[cover[i]] += gw[i][cover[i]][:, None] * val[i][cover[i]]
        den[cover[i]] += gw[i][cover[i]]
    hit = den > 0
    can[hit] = (num[hit] / den[hit][:, None]).astype(np.int32).astype(np.uint8)
    return can


def stats(images, t, stride):
    """The gain rule's two tables on the ring -> (count, sum) uint64 [n, n]."""
    cover, val, _ = planes(images, t)
    L = val.astype(np.int32).astype(np.uint8).astype(np.int64).sum(axis=3)
    cover, L = cover[:, ::stride, ::stride], L[:, ::stride, ::stride]
    n = len(images)
    count, total = np.zeros((n, n), dtype=np.uint64), np.zeros((n, n), dtype=np.uint64)
    for i in range(n):
        for j in range(n):
            both = cover[i] & cover[j]
            count[i, j], total[i, j] = both.sum(), L[i][both].sum()
    return count, total


def down(S):
    """The periodic reduce: the plane three times side by side, multiband_cases.down, the middle third.  The width is even at every
    level below K, and the zero padding reaches only the outer copies."""
    w = S.shape[1] // 2
    return mc.down(np.concatenate([S, S, S], axis=1))[:, w:2 * w]


def up(S):
    w = 2 * S.shape[1]
    return mc.up(np.concatenate([S, S, S], axis=1))[:, w:2 * w]


def multiband(images, t, bands=2, gains=None):
    """The multi-band rule on the planes of the ring rule: PW = P, every plane periodic in x, zero above and below."""
    K, n = bands, len(images)
    fh, P = t["size"]
    cover, val, gw = planes(images, t, gains)
    byt = np.where(cover[:, :, :, None], val.astype(np.int32).astype(np.uint8).astype(np.int64), 0)
    gw = np.where(cover, gw, -np.inf)
    PH = -(-fh // 2 ** K) * 2 ** K
    anyone = cover.any(axis=0)
    winner = np.where(anyone, np.argmax(gw, axis=0), -1)
    Pl = np.zeros((PH, P, 3), dtype=np.int64)
    Pl[:fh] = np.where(anyone[:, :, None], np.take_along_axis(byt, np.maximum(winner, 0)[None, :, :, None], axis=0)[0], 0)
    num = [np.zeros((PH >> l, P >> l, 3), dtype=np.int64) for l in range(K + 1)]
    den = [np.zeros((PH >> l, P >> l, 1), dtype=np.int64) for l in range(K + 1)]
    for i in range(n):
        I = Pl.copy()
        I[:fh][cover[i]] = byt[i][cover[i]]
        Wt = np.zeros((PH, P, 1), dtype=np.int64)
        Wt[:fh, :, 0][winner == i] = mc.ONE
        G, Ws = [I], [Wt]
        for l in range(K):
            G.append(down(G[l]))
            Ws.append(down(Ws[l]))
        for l in range(K + 1):
            L = G[l] - up(G[l + 1]) if l < K else G[l]
            num[l] += L * Ws[l]
            den[l] += Ws[l]
    R = None
    for l in range(K, -1, -1):
        B = np.where(den[l] > 0, np.sign(num[l]) * ((np.abs(num[l]) + den[l] // 2) // np.maximum(den[l], 1)), 0)
        R = B if R is None else B + up(R)
    can = np.zeros((fh, P, 3), dtype=np.uint8)
    can[anyone] = np.clip(R[:fh], 0, 255)[anyone].astype(np.uint8)
    return can


# ---- the library's entry points ----
def _gains_ptr(gains):
    g = None if gains is None else np.ascontiguousarray(gains, dtype=np.float64)
    return g, (None if g is None else g.ctypes.data)


def _ptr(a):
    return None if a is None else a.ctypes.data


def host_twin(lib, images, t, blend=PASTE, rows=None, gains=None, tweak=None, size=None):
    """rwh_host_stitch_sequence_ring -> (status, canvas), the canvas guarded.  tweak(t, ptrs): may spoil (a copy of) the tables before
    the call; size: the (canvas_h, canvas_w) to pass in place of the tables'."""
    images = [np.ascontiguousarray(im) for im in images]
    t = dict(t, rects=t["rects"].copy(), m=t["m"].copy())
    fh, fw = t["size"] if size is None else size
    can, check = sc.guarded_canvas(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    if tweak is not None:
        tweak(t, ptrs)
    r0, r1 = (0, fh) if rows is None else rows
    g, gp = _gains_ptr(gains)
    st = lib.rwh_host_stitch_sequence_ring(ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, t["n"],
                                           t["order"].ctypes.data, blend, _ptr(t["col"]), _ptr(t["row"]), can.ctypes.data, fh, fw, r0, r1, gp)
    check()
    return st, can


def host(lib, *a, **k):
    st, can = host_twin(lib, *a, **k)
    assert st == 0
    return can


def host_stats_twin(lib, images, t, stride=1, tweak=None, size=None):
    import gain_cases as gc
    images = [np.ascontiguousarray(im) for im in images]
    t = dict(t, rects=t["rects"].copy(), m=t["m"].copy())
    fh, fw = t["size"] if size is None else size
    _, count, total, check = gc.guarded_tables(t["n"])
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    if tweak is not None:
        tweak(t, ptrs)
    st = lib.rwh_host_sequence_overlap_stats_ring(ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, t["n"],
                                                  _ptr(t["col"]), _ptr(t["row"]), fh, fw, stride, count.ctypes.data, total.ctypes.data)
    check()
    return st, count.copy(), total.copy()


def host_stats(lib, images, t, stride=1):
    st, count, total = host_stats_twin(lib, images, t, stride)
    assert st == 0
    return count, total


def host_multiband_twin(lib, images, t, bands=2, gains=None, tweak=None, size=None):
    images = [np.ascontiguousarray(im) for im in images]
    t = dict(t, rects=t["rects"].copy(), m=t["m"].copy())
    fh, fw = t["size"] if size is None else size
    can, check = sc.guarded_canvas(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    if tweak is not None:
        tweak(t, ptrs)
    g, gp = _gains_ptr(gains)
    st = lib.rwh_host_stitch_multiband_ring(ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, t["n"], bands, gp,
                                            _ptr(t["col"]), _ptr(t["row"]), can.ctypes.data, fh, fw)
    check()
    return st, can


def host_multiband(lib, *a, **k):
    st, can = host_multiband_twin(lib, *a, **k)
    assert st == 0
    return can


def workspace_bytes(lib, t, bands, size=None):
    fh, fw = t["size"] if size is None else size
    return lib.rwh_stitch_multiband_ring_workspace_bytes(t["rects"].ctypes.data, t["n"], fh, fw, bands)


def device(images, t, blend=PASTE, rows=None, gains=None, on=None):
    """kernels.stitch_sequence on the ring, into a guarded device canvas -> the canvas in numpy."""
    from ransac_with_homography_amd import kernels
    can, fetch = sc.guarded_device_canvas(*t["size"])
    kernels.stitch_sequence_on(sc.upload(images) if on is None else on, sc.geometry(t, pc.device_tables(t), ring=True), t["order"], blend,
                            rows=rows, out=can, gains=gains)
    return fetch()


def device_stats(images, t, stride=1):
    from ransac_with_homography_amd import kernels
    tabs = kernels.sequence_overlap_tables_on(sc.upload(images), sc.geometry(t, pc.device_tables(t), ring=True), stride).cpu().numpy().view(np.uint64)
    return tabs[0], tabs[1]


def device_multiband(lib, images, t, bands=2, gains=None):
    """rwh_stitch_multiband_ring into a guarded canvas, the workspace of the size function's bytes pre-filled with 0xA5 (the call may
    not depend on what it held) -> numpy."""
    import torch
    fh, fw = t["size"]
    dev = sc.upload(images)
    ptrs = np.array([d.data_ptr() for d in dev], dtype=np.uint64)
    need = workspace_bytes(lib, t, bands)
    assert need > 0
    workspace = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    assert workspace.data_ptr() % 8 == 0
    col, row = pc.device_tables(t)
    g, gp = _gains_ptr(gains)
    can, fetch = sc.guarded_device_canvas(fh, fw)
    s = torch.cuda.current_stream()
    st = lib.rwh_stitch_multiband_ring(ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, t["n"], bands, gp,
                                       col.data_ptr(), row.data_ptr(), can.data_ptr(), fh, fw, workspace.data_ptr(), workspace.numel(),
                                       s.cuda_stream)
    assert st == 0, st
    s.synchronize()
    return fetch()


# ---- the cases ----
CASES = {256: dict(n=12, f=40.0, h=24, w=32, seed=12), 512: dict(n=13, f=80.0, h=20, w=60, seed=13), 768: dict(n=12, f=120.0, h=22, w=90, seed=14)}


def circle(P, anchor=0):
    """A sweep that closes the circle on a period of P columns: n images 360 / n degrees apart with a little pitch, roll and
    perspective (projection_cases.sweep) -> (images, Gs, f).  P = 256: 12 images of about 24 x 32 at f = 40; P = 512: 13 of about
    20 x 60 at f = 80; P = 768: 12 of about 22 x 90 at f = 120."""
    c = CASES[P]
    assert period(c["f"]) == P
    images, Hs = pc.sweep(c["n"], c["seed"], f=c["f"], yaw=2.0 * np.pi / c["n"], h=c["h"], w=c["w"])
    return images, sc.chain(Hs, anchor), c["f"]


def circle_tables(P, kind, anchor=0, order=None, rects=None):
    images, Gs, f = circle(P, anchor)
    return images, tables(images, Gs, anchor, kind, f, order=order, rects=rects)


def gains_for(n):
    return 0.8 + 0.05 * np.arange(n)


def three_views(f=TILE / (2.0 * np.pi)):
    """Consequence (a): three images about the anchor at f == 256 / (2 pi), none near the seam -> (images, Gs, f)."""
    images, Hs = pc.sweep(3, 33, f=f, yaw=0.33)
    return images, sc.chain(Hs, 1), f


EIGHTEEN = dict(n=18, h=120, w=160, f=300.0, yaw=np.deg2rad(20.0))


def eighteen_views():
    """18 views of 160 x 120 of projection_cases.texture (periodic in theta) at f = 300, 20 degrees apart, pitch 0.005 i and roll
    0.003 i: a full circle.  -> (images, Hs, Rs) as projection_cases.seven_views gives them."""
    n, h, w, f = EIGHTEEN["n"], EIGHTEEN["h"], EIGHTEEN["w"], EIGHTEEN["f"]
    K = pc.camera((h, w), f)
    Rs = [pc.rotation(EIGHTEEN["yaw"] * i, 0.005 * i, 0.003 * i) for i in range(n)]
    yy, xx = np.mgrid[0:h, 0:w]
    pix = np.stack([xx.ravel(), yy.ravel(), np.ones(h * w)]).astype(np.float64)
    images = []
    for R in Rs:
        r = R @ (np.linalg.inv(K) @ pix)
        theta, t = np.arctan2(r[0], r[2]), r[1] / np.hypot(r[0], r[2])
        images.append(np.rint(pc.texture(theta, t)).astype(np.uint8).reshape(h, w, 3))
    Hs = [K @ Rs[i].T @ Rs[i + 1] @ np.linalg.inv(K) for i in range(n - 1)]
    return images, Hs, Rs


def cylinder_views(n=14, f=400.0, h=200, w=400, scenes=16):
    """A full circle of n views of a feature-rich texture wrapped round a cylinder of radius f about the camera: `scenes`
    sequence_cases.scene() of different seeds side by side make one turn, view i looks along yaw 2 pi i / n (a little pitch and roll
    with it) and is resampled bilinearly -> views uint8 [h, w, 3].  At f = 400 a 400-pixel view spans 53 degrees, so neighbours
    26 degrees apart share half their width: on the MI355X every pair of the ring had 69 to 104 ratio-test matches at 0.7 and 63 to
    94 inliers; views of 200 columns at f = 250 had 10 to 32 matches and lost pairs to the graph's acceptance rule."""
    wide = int(np.ceil(2.0 * np.pi * f / scenes))
    tex = np.concatenate([sc.scene(h=300, w=wide, seed=5 + k) for k in range(scenes)], axis=1).astype(np.float64)
    th, tw = tex.shape[:2]
    Kv = pc.camera((h, w), f)
    yy, xx = np.mgrid[0:h, 0:w]
    pix = np.stack([xx.ravel(), yy.ravel(), np.ones(h * w)]).astype(np.float64)
    views = []
    for i in range(n):
        r = pc.rotation(2.0 * np.pi * i / n, 0.004 * np.sin(i), 0.003 * np.cos(i)) @ (np.linalg.inv(Kv) @ pix)
        sx = (np.arctan2(r[0], r[2]) + np.pi) / (2.0 * np.pi) * tw
        sy = r[1] / np.hypot(r[0], r[2]) * f + (th - 1) / 2.0
        assert sy.min() >= 0 and sy.max() <= th - 1
        ix, iy = np.floor(sx).astype(np.int64), np.minimum(sy.astype(np.int64), th - 2)
        fx, fy = (sx - ix)[:, None], (sy - iy)[:, None]
        a, b = ix % tw, (ix + 1) % tw
        top = tex[iy, a] * (1 - fx) + tex[iy, b] * fx
        bot = tex[iy + 1, a] * (1 - fx) + tex[iy + 1, b] * fx
        views.append(np.rint(top * (1 - fy) + bot * fy).astype(np.uint8).reshape(h, w, 3))
    return views
