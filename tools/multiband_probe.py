"""The multi-band compositor (rwh_stitch_multiband) on tools/sequence_probe.py's strips (N = 2, 4, 8 frames of 1080p and 4K that
overlap their neighbour by 30 %) beside the feather pass on the same inputs, for bands 1, 3 and 5, without gains and with them.
Resident tensors, HIP events after warm-up; the times of kernels.stitch_sequence_multiband include its workspace allocation (a
cached torch block after the first call).  The canvas is checked against a second run before anything is timed, and the workspace
size is printed: it is what the per-image windows cost.

    python tools/multiband_probe.py [reps]
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


lib = _lib.load()
print("%-6s %2s %-20s %13s %9s %9s %10s %10s" % ("frames", "N", "pass", "canvas", "med ms", "min ms", "Mpixel/s", "workspace"))
for name, (h, w) in (("1080p", (1080, 1920)), ("4K", (2160, 3840))):
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for _ in range(8)]
    for n in (2, 4, 8):
        imgs = frames[:n]
        Hs = [pair_h(w)] * (n - 1)
        Gs, rects, origin, (fh, fw), order = hg.sequence_plan([(h, w, 3)] * n, Hs)
        inv = np.stack([np.eye(3) if i == 0 else np.linalg.inv(Gs[i]) for i in range(n)])
        geom = kernels.SeqGeometry(inv, rects, (fh, fw), 0, origin)
        rc = np.ascontiguousarray(rects, dtype=np.int32)
        out = torch.empty((fh, fw, 3), dtype=torch.uint8, device="cuda")
        gains = hg.sequence_gains(imgs, Hs=Hs)

        def line(what, med, mn, ws=""):
            print("%-6s %2d %-20s %6d x %-5d %9.3f %9.3f %10.0f %10s" % (name, n, what, fw, fh, med, mn, fw * fh / med / 1e3, ws))
        for g in (None, gains):
            med, mn = timed(lambda: kernels.stitch_sequence_on(imgs, geom, order, _lib.RWH_SEQ_FEATHER, out=out, gains=g))
            line("feather" + (" + gains" if g is not None else ""), med, mn)
        for bands in (1, 3, 5):
            one = kernels.stitch_sequence_multiband_on(imgs, geom, bands).clone()
            two = kernels.stitch_sequence_multiband_on(imgs, geom, bands)
            assert bool((one == two).all()), "the canvas is not reproducible"
            need = lib.rwh_stitch_multiband_workspace_bytes(rc.ctypes.data, n, fh, fw, int(origin[0]), int(origin[1]), bands)
            for g in (None, gains):
                med, mn = timed(lambda: kernels.stitch_sequence_multiband_on(imgs, geom, bands, gains=g, out=out))
                line("multiband %d" % bands + (" + gains" if g is not None else ""), med, mn, "%d MiB" % (need >> 20))
    del frames
    torch.cuda.empty_cache()
