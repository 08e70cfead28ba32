"""The seam rule (include/rwh.h, rwh_sequence_seams) restated in numpy -- every image's distances over the WHOLE canvas, relaxed by
Jacobi sweeps to the fixed point --, the ctypes drivers of the host twins and of the device calls, and the scenes that
tests/test_sequence_seams_cpu.py and tests/test_sequence_seams_gpu.py share.  It builds on tests/sequence_cases.py,
tests/multiband_cases.py (the planes) and tests/projection_cases.py (the planes of a curved canvas)."""
import collections

import numpy as np

import multiband_cases as mc
import projection_cases as pc
import sequence_cases as sc

NONE = 255
INF = np.int64(2) ** 62
MARGIN, TAU = 8.0, 64           # the defaults of the rule: conventions, not measured optima


# ---- the rule ----
def survey(cover, byt, gw, margin=MARGIN, tau=TAU):
    """cover bool [n, fh, fw], byt int [n, fh, fw, 3], gw float64 [n, fh, fw] -> (w uint8 [fh, fw] (255: nobody), d, c int64 [fh, fw],
    seed bool [n, fh, fw])."""
    n = len(cover)
    anyone = cover.any(axis=0)
    gw = np.where(cover, gw, -np.inf)
    w = np.where(anyone, np.argmax(gw, axis=0), NONE)                  # argmax: the lowest index of equal weights
    hi = np.where(cover[..., None], byt, -1).max(axis=0)
    lo = np.where(cover[..., None], byt, 256).min(axis=0)
    d = np.where(anyone, (hi - lo).sum(axis=-1), 0).astype(np.int64)
    c = np.maximum(1, tau - d)
    seed = np.zeros(cover.shape, dtype=bool)
    for i in range(n):
        rest = np.delete(gw, i, axis=0).max(axis=0) if n > 1 else np.full(anyone.shape, -np.inf)
        seed[i] = cover[i] & (w == i) & (rest <= margin)
    return w.astype(np.uint8), d, c, seed


def distances(cover, seed, c, info=None):
    """dist int64 [n, fh, fw] by Jacobi sweeps: INF where unreached or not covered.  info: receives "sweeps"."""
    dist = np.where(seed, 0, INF)
    free = cover & ~seed
    sweeps = 0
    while True:
        pad = np.pad(dist, ((0, 0), (1, 1), (1, 1)), constant_values=INF)
        near = np.minimum(np.minimum(pad[:, :-2, 1:-1], pad[:, 2:, 1:-1]), np.minimum(pad[:, 1:-1, :-2], pad[:, 1:-1, 2:]))
        new = np.where(free & (near < INF), np.minimum(dist, near + c[None]), dist)
        if np.array_equal(new, dist):
            break
        dist, sweeps = new, sweeps + 1
    if info is not None:
        info["sweeps"] = sweeps
    return dist


def labels_of(cover, w, dist):
    anyone = cover.any(axis=0)
    first = np.argmin(dist, axis=0)                                    # argmin: the lowest index of equal distances
    reached = dist.min(axis=0) < INF
    return np.where(anyone, np.where(reached, first, w), NONE).astype(np.uint8)


def restate_planes(cover, byt, gw, margin=MARGIN, tau=TAU, info=None):
    w, d, c, seed = survey(cover, byt, gw, margin, tau)
    dist = distances(cover, seed, c, info)
    if info is not None:
        info.update(w=w, d=d, c=c, seed=seed, dist=dist, cover=cover)
    return labels_of(cover, w, dist)


def restate(images, Gs, anchor=0, gains=None, margin=MARGIN, tau=TAU, info=None):
    """-> labels uint8 [fh, fw] of the seam rule on the anchor's plane."""
    _, _, cover, byt, gw = mc.image_planes(images, Gs, anchor, gains)
    return restate_planes(cover, byt, gw, margin, tau, info)


def restate_proj(images, Gs, anchor=0, kind="cylindrical", f=40.0, gains=None, margin=MARGIN, tau=TAU, info=None):
    """-> labels uint8 [fh, fw] of the seam rule on a curved canvas."""
    _, cover, val, gw = pc.planes(images, Gs, anchor, kind, f, gains)
    byt = np.where(cover[..., None], val.astype(np.int32).astype(np.uint8).astype(np.int64), 0)
    return restate_planes(cover, byt, gw, margin, tau, info)


def nearest_seed_bfs(cover, seed):
    """tau = 1 stated independently: per image a breadth-first search from its seeds inside its coverage -> hops int64 [n, fh, fw]."""
    n, fh, fw = cover.shape
    hops = np.full(cover.shape, INF)
    for i in range(n):
        todo = collections.deque((int(y), int(x)) for y, x in zip(*np.nonzero(seed[i])))
        hops[i][seed[i]] = 0
        while todo:
            y, x = todo.popleft()
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < fh and 0 <= xx < fw and cover[i, yy, xx] and hops[i, yy, xx] == INF:
                    hops[i, yy, xx] = hops[i, y, x] + 1
                    todo.append((yy, xx))
    return hops


def seam_disagreement(labels, d):
    """The summed disagreement along the seam: d(p) + d(q) over the 4-neighbour pairs (p, q) of covered pixels with two labels."""
    total = 0
    for a, b, da, db in ((labels[:, :-1], labels[:, 1:], d[:, :-1], d[:, 1:]), (labels[:-1], labels[1:], d[:-1], d[1:])):
        cut = (a != b) & (a != NONE) & (b != NONE)
        total += int(da[cut].sum() + db[cut].sum())
    return total


# ---- the library's entry points ----
def _gains_ptr(gains):
    g = None if gains is None else np.ascontiguousarray(gains, dtype=np.float64)
    return g, (None if g is None else g.ctypes.data)


def guarded_plane(fh, fw):
    """A host label plane uint8 [fh, fw] of 0xA5 bytes between two 64-byte canaries -> (plane, check)."""
    buf = np.full(fh * fw + 128, 0xA5, dtype=np.uint8)

    def check():
        assert (buf[:64] == 0xA5).all() and (buf[-64:] == 0xA5).all(), "a byte outside the label plane was written"
    return buf[64:-64].reshape(fh, fw), check


def guarded_device_plane(fh, fw):
    import torch
    buf = torch.full((fh * fw + 128,), 0xA5, dtype=torch.uint8, device="cuda")

    def fetch():
        flat = buf.cpu().numpy()
        assert (flat[:64] == 0xA5).all() and (flat[-64:] == 0xA5).all(), "a byte outside the label plane was written"
        return flat[64:-64].reshape(fh, fw)
    return buf[64:-64].view(fh, fw), fetch


def host_twin(lib, images, Gs, anchor=0, gains=None, margin=MARGIN, tau=TAU, tweak=None):
    """rwh_host_sequence_seams -> (status, labels), the plane guarded.  tweak(t, ptrs): may spoil the tables before the call."""
    images = [np.ascontiguousarray(im) for im in images]
    t = sc.tables(images, Gs, anchor)
    fh, fw = t["size"]
    lab, check = guarded_plane(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    if tweak is not None:
        tweak(t, ptrs)
    g, gp = _gains_ptr(gains)
    st = lib.rwh_host_sequence_seams(ptrs.ctypes.data, t["hw"].ctypes.data, t["inv"].ctypes.data, t["rects"].ctypes.data, t["n"], t["anchor"],
                                     gp, float(margin), int(tau), lab.ctypes.data, fh, fw, t["origin"][0], t["origin"][1])
    check()
    return st, lab


def host(lib, *a, **k):
    st, lab = host_twin(lib, *a, **k)
    assert st == 0
    return lab


def host_proj(lib, images, Gs, anchor=0, kind="cylindrical", f=40.0, gains=None, margin=MARGIN, tau=TAU):
    """rwh_host_sequence_seams_proj -> labels."""
    images = [np.ascontiguousarray(im) for im in images]
    t = pc.tables(images, Gs, anchor, kind, f)
    fh, fw = t["size"]
    lab, check = guarded_plane(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    g, gp = _gains_ptr(gains)
    st = lib.rwh_host_sequence_seams_proj(ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, t["n"], gp,
                                          float(margin), int(tau), t["col"].ctypes.data, t["row"].ctypes.data, lab.ctypes.data, fh, fw)
    check()
    assert st == 0
    return lab


def host_multiband(lib, images, Gs, labels, anchor=0, bands=3, gains=None):
    """rwh_host_stitch_multiband_labels -> (status, canvas); labels None passes NULL."""
    images = [np.ascontiguousarray(im) for im in images]
    t = sc.tables(images, Gs, anchor)
    fh, fw = t["size"]
    can, check = sc.guarded_canvas(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    g, gp = _gains_ptr(gains)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint8)
    st = lib.rwh_host_stitch_multiband_labels(ptrs.ctypes.data, t["hw"].ctypes.data, t["inv"].ctypes.data, t["rects"].ctypes.data, t["n"],
                                              t["anchor"], bands, gp, None if lab is None else lab.ctypes.data, can.ctypes.data, fh, fw,
                                              t["origin"][0], t["origin"][1])
    check()
    return st, can


def host_paste(lib, images, Gs, labels, anchor=0, gains=None):
    """rwh_host_stitch_sequence_labels -> (status, canvas); labels None passes NULL."""
    images = [np.ascontiguousarray(im) for im in images]
    t = sc.tables(images, Gs, anchor)
    fh, fw = t["size"]
    can, check = sc.guarded_canvas(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    g, gp = _gains_ptr(gains)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint8)
    st = lib.rwh_host_stitch_sequence_labels(ptrs.ctypes.data, t["hw"].ctypes.data, t["inv"].ctypes.data, t["rects"].ctypes.data, t["n"],
                                             t["anchor"], gp, None if lab is None else lab.ctypes.data, can.ctypes.data, fh, fw,
                                             t["origin"][0], t["origin"][1])
    check()
    return st, can


def host_multiband_proj(lib, images, Gs, labels, anchor=0, kind="cylindrical", f=40.0, bands=2, gains=None):
    images = [np.ascontiguousarray(im) for im in images]
    t = pc.tables(images, Gs, anchor, kind, f)
    fh, fw = t["size"]
    can, check = sc.guarded_canvas(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    g, gp = _gains_ptr(gains)
    lab = np.ascontiguousarray(labels, dtype=np.uint8)
    st = lib.rwh_host_stitch_multiband_labels_proj(ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, t["n"], bands,
                                                   gp, lab.ctypes.data, t["col"].ctypes.data, t["row"].ctypes.data, can.ctypes.data, fh, fw)
    check()
    assert st == 0
    return can


def host_paste_proj(lib, images, Gs, labels, anchor=0, kind="cylindrical", f=40.0, gains=None):
    images = [np.ascontiguousarray(im) for im in images]
    t = pc.tables(images, Gs, anchor, kind, f)
    fh, fw = t["size"]
    can, check = sc.guarded_canvas(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    g, gp = _gains_ptr(gains)
    lab = np.ascontiguousarray(labels, dtype=np.uint8)
    st = lib.rwh_host_stitch_sequence_labels_proj(ptrs.ctypes.data, t["hw"].ctypes.data, t["m"].ctypes.data, t["rects"].ctypes.data, t["n"], gp,
                                                  lab.ctypes.data, t["col"].ctypes.data, t["row"].ctypes.data, can.ctypes.data, fh, fw)
    check()
    assert st == 0
    return can


def workspace_bytes(lib, t):
    fh, fw = t["size"]
    return lib.rwh_sequence_seams_workspace_bytes(t["rects"].ctypes.data, t["n"], fh, fw, t["origin"][0], t["origin"][1])


def device(lib, images, Gs, anchor=0, gains=None, margin=MARGIN, tau=TAU, on=None, workspace=None, stream=None, info=None):
    """rwh_sequence_seams into a label plane pre-filled with 0xA5 between two 64-byte canaries -> numpy (status 0 and canaries checked).
    workspace: a uint8 device tensor to use (else one of the size function's bytes, filled with 0xA5: the call may not depend on what
    it held); stream: a torch stream (else the current one); info: receives "passes"."""
    import ctypes
    import torch
    t = sc.tables(images, Gs, anchor)
    fh, fw = t["size"]
    dev = sc.upload(images) if on is None else on
    ptrs = np.array([d.data_ptr() for d in dev], dtype=np.uint64)
    need = workspace_bytes(lib, t)
    assert need > 0
    if workspace is None:
        workspace = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    assert workspace.numel() >= need and workspace.data_ptr() % 8 == 0
    s = torch.cuda.current_stream() if stream is None else stream
    g, gp = _gains_ptr(gains)
    passes = ctypes.c_int32(-1)
    torch.cuda.synchronize()                    # (the uploads and the workspace fill ran on the current stream)
    with torch.cuda.stream(s):
        lab, fetch = guarded_device_plane(fh, fw)
        st = lib.rwh_sequence_seams(ptrs.ctypes.data, t["hw"].ctypes.data, t["inv"].ctypes.data, t["rects"].ctypes.data, t["n"], anchor, gp,
                                    float(margin), int(tau), lab.data_ptr(), fh, fw, t["origin"][0], t["origin"][1], workspace.data_ptr(),
                                    workspace.numel(), s.cuda_stream, ctypes.addressof(passes))
        assert st == 0, st
        s.synchronize()
        if info is not None:
            info["passes"] = passes.value
        return fetch()


def device_proj(images, Gs, anchor=0, kind="cylindrical", f=40.0, gains=None, margin=MARGIN, tau=TAU):
    """kernels.sequence_seams on a curved canvas, into a guarded plane -> numpy."""
    from ransac_with_homography_amd import kernels
    t = pc.tables(images, Gs, anchor, kind, f)
    lab, fetch = guarded_device_plane(*t["size"])
    kernels.sequence_seams_on(sc.upload(images), sc.geometry(t, pc.device_tables(t)), gains=gains, margin=margin, tau=tau, out=lab)
    return fetch()


# ---- the scenes ----
def smooth_noise(h, w, seed, lo=60, hi=160, cell=8):
    """Smooth noise uint8 [h, w, 3]: seeded values on a coarse grid, interpolated bilinearly."""
    rng = np.random.default_rng(seed)
    gh, gw = h // cell + 2, w // cell + 2
    grid = rng.uniform(lo, hi, (gh, gw, 3))
    y, x = np.arange(h) / cell, np.arange(w) / cell
    iy, ix = y.astype(int), x.astype(int)
    fy, fx = (y - iy)[:, None, None], (x - ix)[None, :, None]
    top = grid[iy][:, ix] * (1 - fx) + grid[iy][:, ix + 1] * fx
    bot = grid[iy + 1][:, ix] * (1 - fx) + grid[iy + 1][:, ix + 1] * fx
    return np.rint(top * (1 - fy) + bot * fy).astype(np.uint8)


MOVING = dict(h=96, w=130, shift=70, x0=86, y0=37, bw=30, bh=22)


def moving_object():
    """Two 96 x 130 views of one 96 x 200 scene of smooth noise, the second 70 columns right of the first; a 30 x 22 block of value
    250 that only view 0 shows sits across the midline of the overlap (canvas columns 70 .. 129) -> (images, Gs, block slices)."""
    m = MOVING
    scene = smooth_noise(m["h"], m["shift"] + m["w"], 77)
    a, b = scene[:, :m["w"]].copy(), scene[:, m["shift"]:].copy()
    a[m["y0"]:m["y0"] + m["bh"], m["x0"]:m["x0"] + m["bw"]] = 250
    return [a, b], [np.eye(3), sc.translate(m["shift"], 0)], (slice(m["y0"], m["y0"] + m["bh"]), slice(m["x0"], m["x0"] + m["bw"]))


SERPENTINE_TAU = 255


def serpentine_path(y_end, w, step=6):
    """The corridor's canvas pixels, in order: row 1 from column 1 to the right, down `step` rows along the last column, back to the
    left, and so on while the run's row is at most y_end."""
    path, y, going_right = [], 1, True
    while True:
        path += [(y, x) for x in (range(1, w - 1) if going_right else range(w - 2, 0, -1))]
        if y + step > y_end:
            return path
        path += [(yy, w - 2 if going_right else 1) for yy in range(y + 1, y + step)]
        y, going_right = y + step, not going_right


def serpentine(h=100, w=200):
    """Two h x w images, the second one row below the first, for margin 0 and tau = SERPENTINE_TAU: canvas row 0 is image 0's
    alone (its seeds), row h image 1's alone (its seeds), and everything between is covered by both.  The images are equal, red 0,
    except along a one-pixel corridor where image 1's red byte is 255, so c = 1 on the corridor and tau off it.  The corridor starts
    under image 0's seeds and snakes row by row down to 15 rows above image 1's seeds.  A run is w - 2 pixels long and the runs lie
    6 rows apart, so leaving the corridor (5 tau) never pays (2 (w - 2) at most is saved): image 0 takes the whole corridor along it,
    long before image 1 arrives from below.  With the relaxation tile of 64 x 16 every run crosses all tile columns and the next run
    re-enters the tiles the last one left.  -> (images, Gs, path in canvas coordinates)."""
    a = np.full((h, w, 3), 100, dtype=np.uint8)
    a[:, :, 0] = 0
    b = a.copy()
    path = serpentine_path(h - 15, w)
    for y, x in path:
        b[y - 1, x, 0] = 255
    return [a, b], [np.eye(3), sc.translate(0, 1)], path


def three_way():
    """Three images of sc.scene() crops that all meet in one region."""
    scene = sc.scene()
    images = [np.ascontiguousarray(scene[0:90, 0:120]), np.ascontiguousarray(scene[10:100, 60:180]), np.ascontiguousarray(scene[40:130, 30:150])]
    return images, [np.eye(3), sc.translate(60.3, 10.2), sc.translate(30.6, 40.4)]


def first_in_order_labels(cover, order):
    """The label plane "first covering image in `order`"."""
    lab = np.full(cover.shape[1:], NONE, dtype=np.uint8)
    for i in reversed(list(order)):
        lab[cover[i]] = i
    return lab


TILE_W, TILE_H = 64, 16                      # the relaxation tile (RWH_SEAM_TILE_W x RWH_SEAM_TILE_H; the tests assert the export)


def tile_window_cases(tw=TILE_W, th=TILE_H):
    """(w, h, images, Gs): an anchor of 3 tw x 3 th (more than one tile each way) and a second image whose window -- its rectangle
    -- is w x h, for every w and h of the tile's size - 1, the size and the size + 1, placed off the tile grid: its first 20 columns
    lie on the anchor, the rest beyond it, so both images have seeds and the overlap is contested."""
    out = []
    for w in (tw - 1, tw, tw + 1):
        for h in (th - 1, th, th + 1):
            images = [random_pair_image(3 * th, 3 * tw, 10 * w + h), random_pair_image(h, w, 10 * w + h + 1)]
            out.append((w, h, images, [np.eye(3), sc.translate(3 * tw - 20, th + 1)]))
    return out


def tile_canvas_cases(tw=TILE_W, th=TILE_H):
    """(fw, fh, images, Gs): canvases of one tile - 1, one tile and one tile + 1 each way: the anchor holds all columns but the
    last 10, a second image all but the first 10 and the first row."""
    out = []
    for fw, fh in ((tw - 1, th - 1), (tw, th), (tw + 1, th + 1), (tw - 1, th + 1), (tw + 1, th - 1)):
        images = [random_pair_image(fh, fw - 10, fw + fh), random_pair_image(fh - 1, fw - 10, fw + fh + 1)]
        Gs = [np.eye(3), sc.translate(10, 1)]
        assert sc.canvas_of(sc.rectangles([im.shape for im in images], Gs, 0)) == ((0, 0), (fh, fw))
        out.append((fw, fh, images, Gs))
    return out


def random_pair_image(h, w, seed):
    """Smooth noise with a seeded sprinkle of outliers: the two images of a pair agree in places and disagree in others."""
    img = smooth_noise(h, w, seed, 40, 215, 5)
    rng = np.random.default_rng(seed + 99)
    hit = rng.random((h, w)) < 0.2
    img[hit] = rng.integers(0, 256, (int(hit.sum()), 3), dtype=np.uint8)
    return img
