"""The block gain rule (include/rwh.h: cells, cell statistics, cell gains, smoothing, maps, applying maps) restated in numpy from the
rule's text, on top of the planes that tests/sequence_cases.py and tests/projection_cases.py restate; the ctypes drivers of the host
twins, the device drivers, and the fixtures that tests/test_sequence_block_gains_cpu.py and _gpu.py share."""
import numpy as np

import multiband_cases as mc
import projection_cases as pc
import sequence_cases as sc

U = 2.0 ** -53
BLOCKS = (16, 32, 64, 128)


def shift_of(B):
    return int(B).bit_length() - 1


# ---- the planes: every image over the whole canvas ----
def planar_planes(images, Gs, anchor):
    """-> (t, cover bool [n, fh, fw], val float64 [n, fh, fw, 3], w float64 [n, fh, fw]); t: sc.tables."""
    t = sc.tables(images, Gs, anchor)
    (ox, oy), (fh, fw), n = t["origin"], t["size"], len(images)
    cover, val, w = np.zeros((n, fh, fw), dtype=bool), np.zeros((n, fh, fw, 3)), np.zeros((n, fh, fw))
    for i in range(n):
        v, valid, g = sc.sample(images[i], Gs[i], tuple(t["rects"][i]), i == anchor)
        r = t["rects"][i]
        win = (slice(r[1] - oy, r[1] - oy + r[3]), slice(r[0] - ox, r[0] - ox + r[2]))
        cover[i][win], val[i][win], w[i][win] = valid, np.where(valid[:, :, None], v, 0.0), g
    return t, cover, val, w


def curved_planes(images, Gs, anchor, kind, f):
    t = pc.tables(images, Gs, anchor, kind, f)
    _, cover, val, w = pc.planes(images, Gs, anchor, kind, f)
    return t, cover, np.where(cover[:, :, :, None], val, 0.0), w


def canvas_rects(t):
    """The rectangles in canvas coordinates (a curved canvas has them so already)."""
    ox, oy = (0, 0) if "m" in t else t["origin"]
    return [(int(r[0]) - ox, int(r[1]) - oy, int(r[2]), int(r[3])) for r in t["rects"]]


# ---- the rule ----
def grid(size, B):
    return -(-size[0] // B), -(-size[1] // B)


def candidates(t, B):
    """-> (cands [gh][gw] lists of image indices in index order, K)."""
    fh, fw = t["size"]
    gh, gw = grid(t["size"], B)
    rects = canvas_rects(t)
    out = [[[i for i, (rx, ry, wt, ht) in enumerate(rects)
             if rx < min(gx * B + B, fw) and rx + wt > gx * B and ry < min(gy * B + B, fh) and ry + ht > gy * B]
            for gx in range(gw)] for gy in range(gh)]
    return out, max(len(c) for row in out for c in row)


def cell_tables(t, cover, val, B, stride):
    """-> uint32 [gh, gw, 2, K, K]: count and sum of the gain rule over each cell's samples, by candidate rank."""
    fh, fw = t["size"]
    gh, gw = grid(t["size"], B)
    cands, K = candidates(t, B)
    L = np.where(cover, val.astype(np.int32).astype(np.uint8).astype(np.int64).sum(axis=3), 0)
    sample = np.zeros((fh, fw), dtype=bool)
    sample[::stride, ::stride] = True
    out = np.zeros((gh, gw, 2, K, K), dtype=np.uint32)
    for gy in range(gh):
        for gx in range(gw):
            win = (slice(gy * B, min(gy * B + B, fh)), slice(gx * B, min(gx * B + B, fw)))
            for a, i in enumerate(cands[gy][gx]):
                for b, j in enumerate(cands[gy][gx]):
                    both = cover[i][win] & cover[j][win] & sample[win]
                    out[gy, gx, 0, a, b], out[gy, gx, 1, a, b] = both.sum(), L[i][win][both].sum()
    return out


def scatter(tables, t, B):
    """The cell tables scattered back to image indices and summed over the cells -> (count, sum) uint64 [n, n]."""
    n = t["n"]
    cands, _ = candidates(t, B)
    count, total = np.zeros((n, n), dtype=np.uint64), np.zeros((n, n), dtype=np.uint64)
    for gy, row in enumerate(cands):
        for gx, c in enumerate(row):
            k = len(c)
            count[np.ix_(c, c)] += tables[gy, gx, 0, :k, :k].astype(np.uint64)
            total[np.ix_(c, c)] += tables[gy, gx, 1, :k, :k].astype(np.uint64)
    return count, total


def cell_system(cnt, tot, base, sigma_n=10.0, sigma_g=0.1):
    """A and b of one cell, built in the gain rule's order with I_ij = sum / (3 N_ij) * base_i."""
    n = len(cnt)
    alpha, beta = 1.0 / (sigma_n * sigma_n), 1.0 / (sigma_g * sigma_g)
    N = cnt.astype(np.float64)
    I = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            if cnt[i, j]:
                I[i, j] = float(tot[i, j]) / (3.0 * N[i, j]) * base[i]
    A, b = np.zeros((n, n)), np.zeros(n)
    for i in range(n):
        if cnt[i, i] == 0:
            A[i, i], b[i] = 1.0, 1.0
            continue
        for j in range(n):
            A[i, i] += beta * N[i, j]
            b[i] += beta * N[i, j]
            if j != i:
                A[i, i] += 2 * alpha * I[i, j] * I[i, j] * N[i, j]
                A[i, j] -= 2 * alpha * I[i, j] * I[j, i] * N[i, j]
    return A, b


def cell_systems(tables, t, B, base, sigma_n=10.0, sigma_g=0.1):
    """Every cell with a candidate: (gy, gx, candidates, A, b)."""
    cands, _ = candidates(t, B)
    for gy, row in enumerate(cands):
        for gx, c in enumerate(row):
            if c:
                k = len(c)
                A, b = cell_system(tables[gy, gx, 0, :k, :k], tables[gy, gx, 1, :k, :k], np.asarray(base, dtype=np.float64)[c], sigma_n, sigma_g)
                yield gy, gx, c, A, b


def cell_gains(tables, t, B, base, sigma_n=10.0, sigma_g=0.1):
    """r float64 [n, gh, gw] by numpy's solver: 1.0 where an image is no candidate."""
    r = np.ones((t["n"],) + grid(t["size"], B))
    for gy, gx, c, A, b in cell_systems(tables, t, B, base, sigma_n, sigma_g):
        r[c, gy, gx] = np.linalg.solve(A, b)
    return r


def smooth(r, iterations):
    """out = ((a + 2.0 * b) + c) * 0.25 along x, then along y, edges replicated; float64, in that order."""
    r = np.array(r, dtype=np.float64)
    for _ in range(iterations):
        a, c = np.concatenate([r[:, :, :1], r[:, :, :-1]], axis=2), np.concatenate([r[:, :, 1:], r[:, :, -1:]], axis=2)
        r = ((a + 2.0 * r) + c) * 0.25
        a, c = np.concatenate([r[:, :1], r[:, :-1]], axis=1), np.concatenate([r[:, 1:], r[:, -1:]], axis=1)
        r = ((a + 2.0 * r) + c) * 0.25
    return r


def maps_of(r, base):
    return np.asarray(base, dtype=np.float64)[:, None, None] * r


def block_gains(tables, t, B, base=None, sigma_n=10.0, sigma_g=0.1, iterations=2):
    base = np.ones(t["n"]) if base is None else base
    return maps_of(smooth(cell_gains(tables, t, B, base, sigma_n, sigma_g), iterations), base)


def _axis(count, cells, B):
    u = (np.arange(count, dtype=np.float64) + 0.5) / B - 0.5
    lo, hi = u <= 0, u >= cells - 1
    c0 = np.where(lo, 0, np.where(hi, cells - 1, np.floor(u))).astype(np.int64)
    c1 = np.where(lo | hi, c0, c0 + 1)
    return c0, c1, np.where(lo | hi, 0.0, u - c0)


def gain_planes(maps, B, size):
    """g float64 [n, fh, fw]: "Applying maps", the two-step lerp with every product and sum rounded on its own."""
    fh, fw = size
    gh, gw = grid(size, B)
    assert maps.shape[1:] == (gh, gw)
    x0, x1, tx = _axis(fw, gw, B)
    y0, y1, q = _axis(fh, gh, B)
    q = q[:, None]
    top = maps[:, y0][:, :, x0] * (1 - tx) + maps[:, y0][:, :, x1] * tx
    bot = maps[:, y1][:, :, x0] * (1 - tx) + maps[:, y1][:, :, x1] * tx
    return top * (1 - q) + bot * q


def compensated(val, g):
    return np.minimum(val * g[:, :, :, None], 255.0)


def composite(cover, val, w, blend, order):
    """Paste or feather of the sequence rule from the planes -> canvas uint8."""
    n, fh, fw = cover.shape
    can = np.zeros((fh, fw, 3), dtype=np.uint8)
    if blend == sc.PASTE:
        for i in reversed(list(order)):
            can[cover[i]] = val[i][cover[i]].astype(np.int32).astype(np.uint8)
        return can
    num, den = np.zeros((fh, fw, 3)), np.zeros((fh, fw))
    for i in range(n):
        num[cover[i]] += w[i][cover[i]][:, None] * val[i][cover[i]]
        den[cover[i]] += w[i][cover[i]]
    hit = den > 0
    can[hit] = (num[hit] / den[hit][:, None]).astype(np.int32).astype(np.uint8)
    return can


def winners(cover, w, labels=None):
    """The multi-band rule's Winner (-1 where nobody covers), with a label plane the seam rule's: the labelled image where it covers."""
    n = len(cover)
    win = np.where(cover.any(axis=0), np.argmax(np.where(cover, w, -np.inf), axis=0), -1)
    if labels is not None:
        lab = np.asarray(labels).astype(np.int64)
        named = (lab < n) & np.take_along_axis(cover, np.minimum(lab, n - 1)[None], axis=0)[0]
        win = np.where(named, lab, win)
    return win


def label_paste(cover, val, w, labels):
    win = winners(cover, w, labels)
    byt = val.astype(np.int32).astype(np.uint8)
    can = np.take_along_axis(byt, np.maximum(win, 0)[None, :, :, None], axis=0)[0]
    return np.where((win >= 0)[:, :, None], can, 0).astype(np.uint8)


def multiband(cover, val, w, bands, labels=None):
    """The multi-band rule from the planes (tests/multiband_cases.py's restatement from there on), the winner from `winners`."""
    K, (n, fh, fw) = bands, cover.shape
    byt = np.where(cover[:, :, :, None], val.astype(np.int32).astype(np.uint8).astype(np.int64), 0)
    PH, PW = -(-fh // 2 ** K) * 2 ** K, -(-fw // 2 ** K) * 2 ** K
    winner = winners(cover, w, labels)
    anyone = winner >= 0
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
            Lp = G[l] - mc.up(G[l + 1]) if l < K else G[l]
            num[l] += Lp * Ws[l]
            den[l] += Ws[l]
    R = None
    for l in range(K, -1, -1):
        Bl = np.where(den[l] > 0, np.sign(num[l]) * ((np.abs(num[l]) + den[l] // 2) // np.maximum(den[l], 1)), 0)
        R = Bl if R is None else Bl + mc.up(R)
    can = np.zeros((fh, fw, 3), dtype=np.uint8)
    can[anyone] = np.clip(R[:fh, :fw], 0, 255)[anyone].astype(np.uint8)
    return can


def residual_bound(A, g):
    """The backward-error bound of a Cholesky solve, as tests/gain_cases.py has it: 4 n^2 u |A|_inf |g|_inf."""
    n = len(g)
    return 4 * n * n * U * np.abs(A).sum(axis=1).max() * np.abs(g).max()


# ---- the library's entry points on host tables ----
def layout(t, ptrs, own, canvas, tail):
    """An entry point's argument list for the tables of sc.tables (the plane) or pc.tables (a curved canvas)."""
    curved = "m" in t
    head = (ptrs.ctypes.data, t["hw"].ctypes.data, (t["m"] if curved else t["inv"]).ctypes.data, t["rects"].ctypes.data, t["n"])
    if curved:
        return head + own + (t["col"].ctypes.data, t["row"].ctypes.data) + canvas + tail
    return head + (t["anchor"],) + own + canvas + (t["origin"][0], t["origin"][1]) + tail


def form(t):
    return "_proj" if "m" in t else ""


def origin_of(t):
    return (0, 0) if "m" in t else t["origin"]


def slots(lib, t, B):
    fh, fw = t["size"]
    return lib.rwh_sequence_cell_slots(t["rects"].ctypes.data, t["n"], fh, fw, origin_of(t)[0], origin_of(t)[1], shift_of(B))


def guarded_words(count, dtype, fill=0xA5):
    """`count` words of `dtype` pre-filled with 0xA5 bytes between two 64-byte canaries -> (the words, check)."""
    size = count * np.dtype(dtype).itemsize
    buf = np.full(size + 128, fill, dtype=np.uint8)

    def check():
        assert (buf[:64] == fill).all() and (buf[-64:] == fill).all(), "a byte outside the table was written"
    return buf[64:64 + size].view(dtype), check


def host_cell_stats(lib, t, images, B, stride, K=None):
    """rwh_host_sequence_cell_stats / _proj -> (status, tables uint32 [gh, gw, 2, K, K]); the table starts as 0xA5 bytes between canaries."""
    images = [np.ascontiguousarray(im) for im in images]
    fh, fw = t["size"]
    gh, gw = grid(t["size"], B)
    K = slots(lib, t, B) if K is None else K
    words, check = guarded_words(gh * gw * 2 * max(K, 1) ** 2, np.uint32)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    st = getattr(lib, "rwh_host_sequence_cell_stats" + form(t))(*layout(t, ptrs, (), (fh, fw), (shift_of(B), stride, K, words.ctypes.data)))
    check()
    return st, words.reshape(gh, gw, 2, max(K, 1), max(K, 1)).copy()


def hcells(lib, t, images, B, stride):
    st, tabs = host_cell_stats(lib, t, images, B, stride)
    assert st == 0
    return tabs


def host_block_gains(lib, tables, t, B, base=None, sigma_n=10.0, sigma_g=0.1, iterations=2, K=None):
    """rwh_host_sequence_block_gains -> (status, maps float64 [n, gh, gw]), the maps between canaries."""
    fh, fw = t["size"]
    gh, gw = grid(t["size"], B)
    tables = np.ascontiguousarray(tables, dtype=np.uint32)
    K = tables.shape[-1] if K is None else K
    base = None if base is None else np.ascontiguousarray(base, dtype=np.float64)
    maps, check = guarded_words(t["n"] * gh * gw, np.float64)
    st = lib.rwh_host_sequence_block_gains(tables.ctypes.data, t["rects"].ctypes.data, t["n"], fh, fw, origin_of(t)[0], origin_of(t)[1],
                                           shift_of(B), K, None if base is None else base.ctypes.data, sigma_n, sigma_g, iterations,
                                           maps.ctypes.data)
    check()
    return st, maps.reshape(t["n"], gh, gw).copy()


def hmaps(lib, *a, **k):
    st, maps = host_block_gains(lib, *a, **k)
    assert st == 0
    return maps


def host_canvas(lib, what, t, images, maps, B, blend=sc.PASTE, order=None, bands=2, labels=None, rows=None):
    """The host twin of a map-taking compositor -> (status, canvas), the canvas guarded.  what: "sequence" (paste / feather),
    "labels" (label paste) or "multiband" (labels None or a plane)."""
    images = [np.ascontiguousarray(im) for im in images]
    fh, fw = t["size"]
    can, check = sc.guarded_canvas(fh, fw)
    ptrs = np.array([im.ctypes.data for im in images], dtype=np.uint64)
    maps = np.ascontiguousarray(maps, dtype=np.float64)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint8)
    labp = None if lab is None else lab.ctypes.data
    out = (can.ctypes.data, fh, fw)
    if what == "sequence":
        od = np.ascontiguousarray(t["order"] if order is None else order, dtype=np.int32)
        r0, r1 = (0, fh) if rows is None else rows
        st = getattr(lib, "rwh_host_stitch_sequence_maps" + form(t))(*layout(t, ptrs, (od.ctypes.data, blend), out,
                                                                              (r0, r1, maps.ctypes.data, shift_of(B))))
    elif what == "labels":
        st = getattr(lib, "rwh_host_stitch_sequence_labels_maps" + form(t))(*layout(t, ptrs, (maps.ctypes.data, shift_of(B), labp), out, ()))
    else:
        st = getattr(lib, "rwh_host_stitch_multiband_maps" + form(t))(*layout(t, ptrs, (bands, maps.ctypes.data, shift_of(B), labp), out, ()))
    check()
    return st, can


def hcanvas(lib, *a, **k):
    st, can = host_canvas(lib, *a, **k)
    assert st == 0
    return can


# ---- the device ----
def geometry(t):
    return sc.geometry(t, pc.device_tables(t)) if "m" in t else sc.geometry(t)


def device_cells(t, images, B, stride, on=None):
    """kernels.sequence_cell_tables_on -> uint32 [gh, gw, 2, K, K] in numpy."""
    from ransac_with_homography_amd import kernels
    return kernels.sequence_cell_tables_on(sc.upload(images) if on is None else on, geometry(t), B, stride).cpu().numpy().view(np.uint32)


def device_cells_guarded(lib, t, images, B, stride, on=None):
    """rwh_sequence_cell_stats / _proj called directly, into a device table pre-filled with 0xA5 bytes between two 64-byte canaries
    -> uint32 [gh, gw, 2, K, K] in numpy, the canaries checked."""
    import torch
    from ransac_with_homography_amd import _lib
    fh, fw = t["size"]
    gh, gw = grid(t["size"], B)
    K = slots(lib, t, B)
    size = gh * gw * 2 * K * K * 4
    buf = torch.full((size + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    dev = sc.upload(images) if on is None else on
    ptrs = np.array([d.data_ptr() for d in dev], dtype=np.uint64)
    need = lib.rwh_sequence_cell_stats_workspace_bytes(t["n"])
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda")
    td = t
    if "m" in t:
        col, row = pc.device_tables(t)
        td = dict(t, col=_Addr(col.data_ptr()), row=_Addr(row.data_ptr()))
    st = getattr(lib, "rwh_sequence_cell_stats" + form(t))(*layout(td, ptrs, (), (fh, fw), (shift_of(B), stride, K, buf[64:].data_ptr(),
                                                                                            ws.data_ptr(), need, _lib.stream_ptr())))
    assert st == 0
    flat = buf.cpu().numpy()
    assert (flat[:64] == 0xA5).all() and (flat[-64:] == 0xA5).all(), "a byte outside the table was written"
    return flat[64:-64].view(np.uint32).reshape(gh, gw, 2, K, K).copy()


class _Addr(object):
    """A device address where `layout` reads `.ctypes.data` of a host table."""
    def __init__(self, data):
        self.ctypes = self
        self.data = data


def device_canvas(what, t, images, maps, B, blend=sc.PASTE, order=None, bands=2, labels=None, rows=None, on=None):
    """The map-taking compositor on the device, into a guarded canvas -> the canvas in numpy."""
    import torch
    from ransac_with_homography_amd import kernels
    can, fetch = sc.guarded_device_canvas(*t["size"])
    on = sc.upload(images) if on is None else on
    gains = kernels.SeqGainMaps(torch.from_numpy(np.ascontiguousarray(maps, dtype=np.float64)).cuda(), B)
    if what == "sequence":
        kernels.stitch_sequence_on(on, geometry(t), t["order"] if order is None else order, blend, rows=rows, out=can, gains=gains)
    elif what == "labels":
        kernels.stitch_sequence_labels_on(on, geometry(t), labels, gains=gains, out=can)
    else:
        kernels.stitch_sequence_multiband_on(on, geometry(t), bands, gains=gains, out=can, labels=labels)
    return fetch()


# ---- the cases ----
def wavy_maps(n, size, B, seed=0):
    """Non-constant maps, float64 [n, gh, gw] in 0.5 .. 1.9: bright enough to clip, dark, and everything between."""
    gh, gw = grid(size, B)
    return np.random.default_rng(seed).uniform(0.5, 1.9, (n, gh, gw))


def stripes(size, n, seed=0):
    """A label plane of random labels 0 .. n (n names nobody), in 5 x 7 patches."""
    fh, fw = size
    rng = np.random.default_rng(seed)
    small = rng.integers(0, n + 1, (-(-fh // 5), -(-fw // 7)), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(small, np.ones((5, 7), dtype=np.uint8))[:fh, :fw])


def partial_cells():
    """Three images of about 40 x 56, properly warped, on a canvas whose sides are no multiples of 16 -> (images, Gs)."""
    rng = np.random.default_rng(77)
    images = [sc.random_image(40, 56, 700), sc.random_image(38, 53, 701), sc.random_image(41, 50, 702)]
    return images, sc.chain([sc.homography(rng, 30.4, 3.3), sc.homography(rng, 27.7, -5.2)], 0)


def narrow_canvas():
    """Two 24 x 11 images one column apart: a canvas narrower than one cell of 16."""
    return [sc.random_image(24, 11, 710), sc.random_image(24, 11, 711)], [np.eye(3), sc.translate(1, 0)]


def empty_cell():
    """Two 14 x 14 images at the opposite corners of a 50 x 50 canvas: the cells between them have no candidate."""
    return [sc.random_image(14, 14, 720), sc.random_image(14, 14, 721)], [np.eye(3), sc.translate(36, 36)]


def sixty_four_on_one_cell():
    """64 images of 8 x 8 stacked on one cell, image i a sixteenth of a pixel right of image i - 1: K = 64, every pair meets."""
    return [sc.random_image(8, 8, 800 + i) for i in range(64)], [sc.translate(i / 16.0, 0) for i in range(64)]


def big_cell():
    """One white 130 x 130 image and a second over all of it but the last column and row: B = 128 gives one full cell of 16384 samples
    whose sum is the largest a slot can hold, and partial cells one pixel wide."""
    return [np.full((130, 130, 3), 255, dtype=np.uint8), sc.random_image(129, 129, 731)], [np.eye(3), np.eye(3) + 0.0]


def cylinder_case():
    """Three images on a cylindrical canvas (tests/projection_cases.py's sweep) -> (images, Gs, kind, f)."""
    images, Hs = pc.sweep(3, seed=11, f=40.0, yaw=0.33, h=40, w=56)
    return images, sc.chain(Hs, 0), "cylindrical", 40.0


def vignetted_scene():
    """The effect test's scene: three 120 x 160 crops of one smooth synthetic texture, 80 columns apart, each multiplied by its own
    exposure (0.8, 1.0, 1.25) and by the radial falloff 1 - 0.35 r^2 (r = 1 at the crop's corners), rounded -> (images, Gs)."""
    h, w, step = 120, 160, 80
    yy, xx = np.mgrid[0:h, 0:w + 2 * step].astype(np.float64)
    tex = np.stack([120 + 45 * np.sin(xx / 23.0 + k) * np.cos(yy / 17.0 - k) + 25 * np.sin((xx + yy) / 9.0 + 2 * k) for k in range(3)], axis=2)
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    fall = 1.0 - 0.35 * (((x - cx) / cx) ** 2 + ((y - cy) / cy) ** 2) / 2.0
    images = [np.clip(np.rint(tex[:, i * step:i * step + w] * e * fall[:, :, None]), 1, 255).astype(np.uint8)
              for i, e in enumerate((0.8, 1.0, 1.25))]
    return images, [sc.translate(step * i, 0) for i in range(3)]


def mismatch(cover, val):
    """The mean absolute difference of the compensated bytes of the two covering images, over the pixels that exactly two cover."""
    byt = val.astype(np.int32).astype(np.uint8).astype(np.float64)
    total, count = 0.0, 0
    n = len(cover)
    for i in range(n):
        for j in range(i + 1, n):
            both = cover[i] & cover[j] & (cover.sum(axis=0) == 2)
            total += np.abs(byt[i][both] - byt[j][both]).sum()
            count += 3 * int(both.sum())
    return total / count
