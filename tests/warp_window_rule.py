"""The block rule of the batch form of the uint8 bilinear warp (fast8mb_body in csrc/rwh_warp_rgb8.h), restated in numpy: which 128 x 16
tiles of a launch walk through their frames with one block window, which store zeros, which fall back to the one-frame body, and how
many rows and 16-byte chunks a walking tile's window has.  float64 division stands in for the kernel's reciprocal + Newton step, so a
corner whose coordinate lies within an ulp of an integer may be counted one row off; the tests that use this assert counts, not tiles.

    python tests/warp_window_rule.py      the two bench grids (32 x 4K and 512 x 1080p under H_S), for candidate window sizes
"""
import collections

import numpy as np

BROWS, BCH = 21, 36              # the kernel's block window: rows x 16-byte chunks (4 texels each)
STRIP_MAX = 16                   # a ragged right edge of 1 .. 16 columns (of 256 or more) goes to the strip kernel

# per tile (ty, tx), int arrays.  kind: 0 = some wave blends (the tile walks if its window fits), 1 = no wave blends (zeros, no loads),
# 2 = a horizon wave (falls back whatever the window).  nrows x chunks from source row ymin: the window.  blending: waves that blend;
# owning: waves that own a column of the tile; masked: some owning wave is not strictly interior.
Windows = collections.namedtuple("Windows", "kind nrows chunks ymin blending owning masked src_h")


def tile_windows(inv, grid, src_hw, bound, shape=6, rows=None):
    """`grid` = (x0, x_last, out_w, y0, y_last, out_h) as kernels.Grid takes them; `shape`: log2 of the patch width (5, 6, 7)."""
    x0, x_last, out_w, y0, y_last, out_h = grid
    step_x = (x_last - x0) / (out_w - 1) if out_w > 1 else 0.0
    step_y = (y_last - y0) / (out_h - 1) if out_h > 1 else 0.0
    r0, r1 = rows if rows is not None else (0, out_h)
    nrow = r1 - r0
    if out_w >= 256 and 1 <= out_w % 128 <= STRIP_MAX:
        out_w -= out_w % 128
    pw = 1 << shape
    ph, wx = 512 // pw, 128 // pw
    tiles_x, tiles_y = (out_w + 127) // 128, (nrow + 15) // 16
    bound_h, bound_w = bound
    src_h = src_hw[0]
    z = lambda: np.zeros((tiles_y, tiles_x), dtype=np.int64)
    win = Windows(z(), z(), z(), z(), z(), z(), z(), src_h)
    clamp = lambda v, hi: min(max(v, 0), hi)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            tcol0 = tx * 128
            tcol = min(tcol0, out_w - 128)
            tshift = tcol0 - tcol
            boxes, horizon = [], False
            for wave in range(4):
                wave_x, wave_y = (wave % wx) * pw, (wave // wx) * ph
                owns = (wave % wx + 1) * pw > tshift
                rr = [min(ty * 16 + wave_y + p, nrow - 1) for p in (0, ph - 1)]
                cc = [tcol + wave_x, tcol + wave_x + pw - 1]
                gx = np.array([x0 + step_x * c for c in cc])[None, :]
                gy = np.array([y0 + step_y * (r0 + r) for r in rr])[:, None]
                X = inv[0, 0] * gx + inv[0, 1] * gy + inv[0, 2]
                Y = inv[1, 0] * gx + inv[1, 1] * gy + inv[1, 2]
                W = inv[2, 0] * gx + inv[2, 1] * gy + inv[2, 2]
                if not (W > 1e-60).all():
                    horizon = True
                    continue
                fx, fy = np.floor(X / W).astype(np.int64), np.floor(Y / W).astype(np.int64)
                bxmn, bxmx, bymn, bymx = int(fx.min()) & ~3, int(fx.max()), int(fy.min()), int(fy.max())
                outside = bxmx < 0 or bxmn >= bound_w or bymx < 0 or bymn >= bound_h
                interior = bxmn >= 0 and bxmx < bound_w - 1 and bymn >= 0 and bymx < min(bound_h - 1, src_h - 2)
                win.owning[ty, tx] += owns
                win.masked[ty, tx] |= owns and not interior
                if owns and not outside:
                    boxes.append((clamp(bxmn, bound_w - 1), clamp(bxmx, bound_w - 1), clamp(bymn, bound_h - 1), clamp(bymx, bound_h - 1)))
            win.blending[ty, tx] = len(boxes)
            if horizon:
                win.kind[ty, tx] = 2
            elif not boxes:
                win.kind[ty, tx] = 1
            else:
                xmn = min(b[0] for b in boxes) & ~3
                xmx = max(b[1] for b in boxes)
                ymn = min(b[2] for b in boxes)
                ymx = max(b[3] for b in boxes)
                win.nrows[ty, tx], win.chunks[ty, tx], win.ymin[ty, tx] = ymx - ymn + 2, (xmx - xmn + 5) >> 2, ymn
    return win


def falls_back(win, brows=BROWS, bch=BCH):
    """Boolean per tile: the tile runs the one-frame body frame by frame."""
    fits = (win.nrows <= brows) & (win.chunks <= bch) & (win.ymin + win.nrows - 1 <= win.src_h - 2)
    return (win.kind == 2) | ((win.kind == 0) & ~fits)


def walks(win, brows=BROWS, bch=BCH):
    """Boolean per tile: the tile walks through its frames with one block window (the blocks that have loads in flight)."""
    return (win.kind == 0) & ~falls_back(win, brows, bch)


if __name__ == "__main__":
    H_S = np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]])

    def bounds(h, w):
        b = H_S @ np.array([[0, w - 1, w - 1, 0], [0, 0, h - 1, h - 1], [1., 1, 1, 1]])
        b /= b[-1]
        mx, my = int(b[0].min()), int(b[1].min())
        return mx, my, int(b[0].max()) - mx + 1, int(b[1].max()) - my + 1

    for name, (h, w) in (("32 x 4K", (2160, 3840)), ("512 x 1080p", (1080, 1920))):
        mx, my, ow, oh = bounds(h, w)
        win = tile_windows(np.linalg.inv(H_S), (mx, mx + ow - 1, ow, my, my + oh - 1, oh), (h, w), (h, w))
        some = win.kind == 0
        hist = lambda a: " ".join("%d:%d" % (v, n) for v, n in zip(*np.unique(a[some], return_counts=True)))
        print("%s: %d x %d output, %d tiles, %d of them wholly outside" % (name, ow, oh, win.kind.size, int((win.kind == 1).sum())))
        print("    rows of the windows (rows:tiles)   %s" % hist(win.nrows))
        print("    chunks of the windows              %s" % hist(win.chunks))
        for brows, bch in ((22, 36), (21, 36), (20, 36), (22, 34)):
            print("    window %2d x %2d: %d tiles fall back" % (brows, bch, int(falls_back(win, brows, bch).sum())))
