"""The sequence compositor (rwh_stitch_sequence) on strips of N = 2, 4, 8 frames of 1080p and 4K that overlap their neighbour by
30 %: resident tensors, HIP events after warm-up, paste and feather.  Beside each: a device copy of the canvas bytes (the floor of
anything that writes the canvas once) and, for N = 2, the exact two-image compositor (kernels.stitch_panorama(fast=False)) on the
same pair.  Each frame maps into its left neighbour by a translation of 70 % of the width plus a small affine and perspective part,
so every frame is properly resampled.  The canvases are checked against each other at N = 2 (paste) before anything is timed.

    python tools/sequence_probe.py [reps]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ransac_with_homography_amd import _lib, homography as hg, kernels      # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def pair_h(w):
    return np.array([[1.01, 0.004, 0.7 * w], [0.003, 0.995, 6.5], [2e-6, 1e-6, 1.0]])


print("%-6s %2s %-8s %13s %9s %9s %9s %9s" % ("frames", "N", "mode", "canvas", "med ms", "min ms", "MB out", "GB/s out"))
for name, (h, w) in (("1080p", (1080, 1920)), ("4K", (2160, 3840))):
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for _ in range(8)]
    for n in (2, 4, 8):
        imgs = frames[:n]
        Gs, rects, origin, (fh, fw), order = hg.sequence_plan([(h, w, 3)] * n, [pair_h(w)] * (n - 1))
        inv = np.stack([np.eye(3) if i == 0 else np.linalg.inv(Gs[i]) for i in range(n)])
        geom = kernels.SeqGeometry(inv, rects, (fh, fw), 0, origin)
        out = torch.empty((fh, fw, 3), dtype=torch.uint8, device="cuda")
        src = torch.empty_like(out)
        mb = fh * fw * 3 / 1e6
        for mode, blend in (("paste", _lib.RWH_SEQ_PASTE), ("feather", _lib.RWH_SEQ_FEATHER)):
            med, mn = timed(lambda: kernels.stitch_sequence_on(imgs, geom, order, blend, out=out))
            print("%-6s %2d %-8s %6d x %-5d %9.3f %9.3f %9.1f %9.0f" % (name, n, mode, fw, fh, med, mn, mb, mb / med))
        med, mn = timed(lambda: out.copy_(src))
        print("%-6s %2d %-8s %6d x %-5d %9.3f %9.3f %9.1f %9.0f" % (name, n, "copy", fw, fh, med, mn, mb, mb / med))
        if n == 2:
            H = pair_h(w)
            mx, my, wt, ht = hg._bounds(h, w, H, 0)
            (tsx, tsy, _, _), (qsx, qsy, _, _), (pw, ph) = hg._stitch_geometry(wt, ht, w, h, mx, my)
            T = imgs[1].clone()
            T[0, 0] = 0

            def two():
                return kernels.stitch_panorama(T, imgs[0], np.linalg.inv(H), (mx, my), (wt, ht), (tsx, tsy), (qsx, qsy), (ph, pw), 0, 0.2,
                                               zero_origin=False, fast=False)
            same = (ph, pw) == (fh, fw) and bool((two() == kernels.stitch_sequence_on(imgs, geom, order, 0)).all())
            med, mn = timed(two)
            print("%-6s %2d %-8s %6d x %-5d %9.3f %9.3f %9.1f %9.0f   (stitch_panorama exact; same bytes as the sequence paste: %s)"
                  % (name, n, "pair", pw, ph, med, mn, mb, mb / med, same))
    del frames
    torch.cuda.empty_cache()
