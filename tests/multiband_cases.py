"""The multi-band rule (include/rwh.h, rwh_stitch_multiband) restated in numpy on top of tests/sequence_cases.py -- every image's
planes over the WHOLE padded canvas, no windows --, the ctypes drivers of the host twin and of the device call, and the fixtures
that tests/test_sequence_multiband_cpu.py and tests/test_sequence_multiband_gpu.py share."""
import numpy as np

import sequence_cases as sc

ONE = 16384
W5 = (1, 4, 6, 4, 1)
MAX_BANDS = 8


# ---- the rule ----
def down(S):
    """Reduce: S int64 [H, W, C] (H, W even) -> [H / 2, W / 2, C]."""
    H, W = S.shape[:2]
    P = np.pad(S, ((2, 2), (2, 2), (0, 0)))
    out = np.zeros((H // 2, W // 2, S.shape[2]), dtype=np.int64)
    for ky in range(5):
        for kx in range(5):
            out += W5[ky] * W5[kx] * P[ky:ky + H:2, kx:kx + W:2]
    return (out + 128) >> 8


def up(S):
    """Expand: S int64 [h, w, C] -> [2h, 2w, C].  S sits on the even coordinates of a zero plane: the taps with y + ky and x + kx
    even are the non-zero ones, S[(y + ky) / 2][(x + kx) / 2]; `>>` floors."""
    h, w = S.shape[:2]
    U = np.zeros((2 * h + 4, 2 * w + 4, S.shape[2]), dtype=np.int64)
    U[2:2 + 2 * h:2, 2:2 + 2 * w:2] = S
    out = np.zeros((2 * h, 2 * w, S.shape[2]), dtype=np.int64)
    for ky in range(5):
        for kx in range(5):
            out += W5[ky] * W5[kx] * U[ky:ky + 2 * h, kx:kx + 2 * w]
    return (out + 32) >> 6


def image_planes(images, Gs, anchor, gains=None):
    """-> ((ox, oy), (fh, fw), cover bool [n, fh, fw], bytes int64 [n, fh, fw, 3], g float64 [n, fh, fw] (-inf where not covered))."""
    n = len(images)
    gains = np.ones(n) if gains is None else np.asarray(gains, dtype=np.float64)
    rects = sc.rectangles([im.shape for im in images], Gs, anchor)
    (ox, oy), (fh, fw) = sc.canvas_of(rects)
    cover = np.zeros((n, fh, fw), dtype=bool)
    byt = np.zeros((n, fh, fw, 3), dtype=np.int64)
    gw = np.full((n, fh, fw), -np.inf)
    for i in range(n):
        v, valid, g = sc.sample(images[i], Gs[i], rects[i], i == anchor)
        v = np.minimum(v * gains[i], 255.0)                            # (v <= 255: a unit gain changes nothing)
        r = rects[i]
        win = (slice(r[1] - oy, r[1] - oy + r[3]), slice(r[0] - ox, r[0] - ox + r[2]))
        cover[i][win] = valid
        byt[i][win] = np.where(valid[:, :, None], v.astype(np.int32).astype(np.uint8).astype(np.int64), 0)
        gw[i][win] = np.where(valid, g, -np.inf)
    return (ox, oy), (fh, fw), cover, byt, gw


def restate(images, Gs, anchor=0, bands=5, gains=None):
    """-> canvas uint8 [fh, fw, 3] of the multi-band rule."""
    K, n = bands, len(images)
    _, (fh, fw), cover, byt, gw = image_planes(images, Gs, anchor, gains)
    PH, PW = -(-fh // 2 ** K) * 2 ** K, -(-fw // 2 ** K) * 2 ** K
    anyone = cover.any(axis=0)
    winner = np.where(anyone, np.argmax(gw, axis=0), -1)               # argmax: the first (lowest index) of equal weights
    P = np.zeros((PH, PW, 3), dtype=np.int64)
    P[:fh, :fw] = np.where(anyone[:, :, None], np.take_along_axis(byt, np.maximum(winner, 0)[None, :, :, None], axis=0)[0], 0)
    num = [np.zeros((PH >> l, PW >> l, 3), dtype=np.int64) for l in range(K + 1)]
    den = [np.zeros((PH >> l, PW >> l, 1), dtype=np.int64) for l in range(K + 1)]
    for i in range(n):
        I = P.copy()
        I[:fh, :fw][cover[i]] = byt[i][cover[i]]
        Wt = np.zeros((PH, PW, 1), dtype=np.int64)
        Wt[:fh, :fw, 0][winner == i] = ONE
        G, Ws = [I], [Wt]
        for l in range(K):
            G.append(down(G[l]))
            Ws.append(down(Ws[l]))
        for l in range(K + 1):
            L = G[l] - up(G[l + 1]) if l < K else G[l]
            assert np.abs(L).max() <= 255
            num[l] += L * Ws[l]
            den[l] += Ws[l]
    R = None
    for l in range(K, -1, -1):
        d = np.maximum(den[l], 1)
        B = np.where(den[l] > 0, np.sign(num[l]) * ((np.abs(num[l]) + den[l] // 2) // d), 0)
        R = B if R is None else B + up(R)
        assert np.abs(R).max() <= 255 * (K + 1)
    can = np.zeros((fh, fw, 3), dtype=np.uint8)
    can[anyone] = np.clip(R[:fh, :fw], 0, 255)[anyone].astype(np.uint8)
    return can


# ---- the library's entry points ----
def _gains_ptr(gains):
    g = None if gains is None else np.ascontiguousarray(gains, dtype=np.float64)
    return g, (None if g is None else g.ctypes.data)


def host_twin(lib, images, Gs, anchor=0, bands=5, gains=None, tweak=None):
    """rwh_host_stitch_multiband -> (status, canvas), the canvas between two 64-byte canaries that are checked here.  tweak(t, ptrs):
    may spoil the tables before the call (the refusal tests)."""
    images = [np.ascontiguousarray(im) for im in images]
    t = sc.tables(images, Gs, anchor)
    fh, fw = t["size"]
    can, check = sc.guarded_canvas(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    if tweak is not None:
        tweak(t, ptrs)
    g, gp = _gains_ptr(gains)
    st = lib.rwh_host_stitch_multiband(ptrs.ctypes.data, t["hw"].ctypes.data, t["inv"].ctypes.data, t["rects"].ctypes.data, t["n"], t["anchor"],
                                       bands, gp, can.ctypes.data, fh, fw, t["origin"][0], t["origin"][1])
    check()
    return st, can


def host(lib, *a, **k):
    st, can = host_twin(lib, *a, **k)
    assert st == 0
    return can


def workspace_bytes(lib, t, bands):
    fh, fw = t["size"]
    return lib.rwh_stitch_multiband_workspace_bytes(t["rects"].ctypes.data, t["n"], fh, fw, t["origin"][0], t["origin"][1], bands)


def device(lib, images, Gs, anchor=0, bands=5, gains=None, on=None, workspace=None, stream=None):
    """rwh_stitch_multiband into a canvas pre-filled with 0xA5 between two 64-byte canaries -> numpy (status 0 and canaries checked).
    workspace: a uint8 device tensor to use (else one of the size function's bytes, filled with 0xA5: the call may not depend on what
    it held); stream: a torch stream (else the current one)."""
    import torch
    t = sc.tables(images, Gs, anchor)
    fh, fw = t["size"]
    dev = sc.upload(images) if on is None else on
    ptrs = np.array([d.data_ptr() for d in dev], dtype=np.uint64)
    need = workspace_bytes(lib, t, bands)
    assert need > 0
    if workspace is None:
        workspace = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    assert workspace.numel() >= need and workspace.data_ptr() % 8 == 0
    s = torch.cuda.current_stream() if stream is None else stream
    g, gp = _gains_ptr(gains)
    torch.cuda.synchronize()                    # (the uploads and the workspace fill ran on the current stream)
    with torch.cuda.stream(s):
        can, fetch = sc.guarded_device_canvas(fh, fw)
        st = lib.rwh_stitch_multiband(ptrs.ctypes.data, t["hw"].ctypes.data, t["inv"].ctypes.data, t["rects"].ctypes.data, t["n"], anchor, bands, gp,
                                      can.data_ptr(), fh, fw, t["origin"][0], t["origin"][1], workspace.data_ptr(), workspace.numel(),
                                      s.cuda_stream)
        assert st == 0, st
        s.synchronize()
        return fetch()


# ---- the cases ----
def flat_pair():
    """Two flat 96 x 200 images, values 100 and 160, the second 80 columns right of the first."""
    return [np.full((96, 200, 3), 100, dtype=np.uint8), np.full((96, 200, 3), 160, dtype=np.uint8)], [np.eye(3), sc.translate(80, 0)]


def misregistered_pair():
    """Crops of sc.scene() at columns 0 and 90, each 260 wide, placed with translate(93, 2): 3 columns and 2 rows off."""
    scene = sc.scene()
    return [np.ascontiguousarray(scene[:, 0:260]), np.ascontiguousarray(scene[:, 90:350])], [np.eye(3), sc.translate(93, 2)]


def gradient_energy(can):
    """Mean |horizontal| + |vertical| gradient of the channel mean over rows 20:180 and columns 110:240."""
    m = can.astype(np.float64).mean(axis=2)[20:180, 110:240]
    return float(np.abs(np.diff(m, axis=1)).mean() + np.abs(np.diff(m, axis=0)).mean())


def one_by_one_top():
    """A 9 x 11 canvas: at bands 4 the padded canvas is 16 x 16 and its top level one pixel."""
    return [sc.random_image(9, 11, 90)], [np.eye(3)]


def axis_windows(a, b, P, K):
    """"Working in windows" of the rule, one axis: the rectangle's canvas interval [a, b), the padded side P -> [(lo, hi)] per level,
    inclusive, clipped to the level's plane."""
    d = [(a, b - 1)]
    for l in range(K):
        d.append(((d[l][0] - 1) >> 1, (d[l][1] + 2) >> 1))
    n = [None] * (K + 1)
    for l in range(K, -1, -1):
        lo, hi = d[l]
        if l > 0:
            lo, hi = min(lo, (d[l - 1][0] >> 1) - 1), max(hi, (d[l - 1][1] >> 1) + 1)
        if l < K:
            lo, hi = min(lo, 2 * n[l + 1][0] - 2), max(hi, 2 * n[l + 1][1] + 2)
        n[l] = (lo, hi)
    return [(max(lo, 0), min(hi, (P >> l) - 1)) for l, (lo, hi) in enumerate(n)]


TILE_BANDS = 3
TILE_WIDTHS = (31, 32, 33, 63, 64, 65)      # the reduce kernel makes 32 x 8 outputs per block, the other kernels take 64 x 4 pixels
TILE_HEIGHTS = (3, 4, 5, 7, 8, 9)


def tile_edge_cases():
    """{(axis, level, size): (images, Gs)} for a 3-band run: an anchor that spans the canvas (6 x 704, or 704 x 6 for the rows) and
    a second image whose window at `level` is exactly `size` wide (high), for every tile width (height) +- 1 -- found by search with
    axis_windows.  A window reaches 6 * 2^(K - level) pixels and more beyond its rectangle, so the small sizes do not exist at the
    low levels (tests/test_sequence_multiband_cpu.py asserts what is found); the level-0 edges of the launches are met by plane_edge_cases()."""
    K, long = TILE_BANDS, 704
    out = {}
    for axis, sizes in (("x", TILE_WIDTHS), ("y", TILE_HEIGHTS)):
        for level in range(K + 1):
            for size in sizes:
                hit = None
                for at in (0, 3, 150, None):                # None: flush with the far edge, the window clipped by the plane there
                    for ext in range(2, 540):
                        a = long - ext if at is None else at
                        lo, hi = axis_windows(a, a + ext, long, K)[level]
                        if hi - lo + 1 == size:
                            hit = (a, ext)
                            break
                    if hit:
                        break
                if hit is None:
                    continue
                at, ext = hit
                seed = 1000 * level + size
                if axis == "x":
                    images, Gs = [sc.random_image(6, long, seed), sc.random_image(5, ext, seed + 1)], [np.eye(3), sc.translate(at, 1)]
                else:
                    images, Gs = [sc.random_image(long, 6, seed), sc.random_image(ext, 5, seed + 1)], [np.eye(3), sc.translate(1, at)]
                out[(axis, level, size)] = (images, Gs)
    return out


def plane_edge_cases():
    """(fw, fh, images, Gs): two-image canvases of exactly fw x fh, fw and fh at the 64 x 4 and 32 x 8 tiles +- 1: the edges of the
    launches over the canvas, the padded canvas and the level-0 windows."""
    out = []
    for fw, fh in ((31, 3), (32, 4), (33, 5), (63, 7), (64, 8), (65, 9)):
        wa = fw - 7
        images = [sc.random_image(fh, wa, 50 + fw), sc.random_image(fh - 1, fw - 9, 51 + fw)]
        Gs = [np.eye(3), sc.translate(9, 1)]
        rects = sc.rectangles([im.shape for im in images], Gs, 0)
        assert sc.canvas_of(rects) == ((0, 0), (fh, fw)), (fw, fh, rects)
        out.append((fw, fh, images, Gs))
    return out
