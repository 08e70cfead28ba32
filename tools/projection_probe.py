"""The sequence compositor on the anchor's plane, on a cylinder and on a sphere (the projection rule of include/rwh.h), on sweeps
of N = 4 and 8 frames of 1080p from a camera with f = 1500 px that turns 15 degrees per frame: resident tensors, HIP events after
warm-up.  Passes: paste, feather, the overlap statistics at stride 4, multi-band with 5 bands.  The planar runs take the middle
frame as their anchor (with the first frame the plane does not hold 8 frames); the curved runs take it too, so the three canvases
show the same sweep.  The canvases differ in size, so every time is also given per canvas megapixel.

    python tools/projection_probe.py [reps]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ransac_with_homography_amd import _lib, homography as hg, kernels      # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
H, W, F, YAW = 1080, 1920, 1500.0, np.deg2rad(15.0)


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


def pair_h():
    """Frame i + 1 into frame i: K R inv(K) for a yaw of 15 degrees with a little pitch and roll."""
    K = np.array([[F, 0.0, (W - 1) / 2.0], [0.0, F, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    cy, sy, cp, sp, cr, sr = np.cos(YAW), np.sin(YAW), np.cos(0.004), np.sin(0.004), np.cos(0.002), np.sin(0.002)
    R = (np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]) @ np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
         @ np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]]))
    return K @ R @ np.linalg.inv(K)


print("%-6s %2s %-12s %-12s %13s %9s %9s %9s %11s" % ("frames", "N", "canvas", "pass", "size", "med ms", "min ms", "Mpix", "ms / Mpix"))
rng = np.random.default_rng(0)
frames = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(8)]
for n in (4, 8):
    imgs, anchor = frames[:n], n // 2
    Hs = [pair_h()] * (n - 1)
    for projection in (None, "cylindrical", "spherical"):
        try:
            rects, origin, (fh, fw), order, mats, rays = hg._sequence_inputs("projection_probe", imgs, Hs, None, anchor, projection,
                                                                             None if projection is None else F)
        except ValueError as e:
            print("%-6s %2d %-12s refused: %s" % ("1080p", n, projection or "planar", e))
            continue
        out = torch.empty((fh, fw, 3), dtype=torch.uint8, device="cuda")
        if rays is None:
            geom = kernels.SeqGeometry(mats, rects, (fh, fw), anchor, origin)
        else:
            geom = kernels.SeqGeometry(mats, rects, (fh, fw), rays=rays).on_device(imgs[0].device)
        passes = [(mode, lambda blend=blend: kernels.stitch_sequence_on(imgs, geom, order, blend, out=out))
                  for mode, blend in (("paste", _lib.RWH_SEQ_PASTE), ("feather", _lib.RWH_SEQ_FEATHER))]
        passes.append(("stats 4", lambda: kernels.sequence_overlap_tables_on(imgs, geom, 4)))
        passes.append(("multiband 5", lambda: kernels.stitch_sequence_multiband_on(imgs, geom, 5, out=out)))
        mpix = fh * fw / 1e6
        for mode, fn in passes:
            med, mn = timed(fn)
            print("%-6s %2d %-12s %-12s %6d x %-5d %9.3f %9.3f %9.2f %11.4f" % ("1080p", n, projection or "planar", mode, fw, fh, med, mn, mpix, med / mpix))
        del out
        torch.cuda.empty_cache()
