"""The any-dtype compositor (rwh_stitch_panorama_ex) on config 4's geometry: two 8192 x 5464 images, the homography of the x8
problem (tests/golden/g13_config4_x8.npz) -> a 13 181 x 6 313 canvas; resident tensors, HIP events after warm-up.  Paste and
'Rate' for float32 RGB, float64 RGB, uint16 RGB and uint8 RGBA, and the uint8 RGB exact kernel (rwh_stitch_panorama) beside
them.  Algorithmic bytes: both images read once, the canvas written once; against the 8 TB/s HBM roofline.

    python tools/stitch_dtype_probe.py [reps]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import rwh_oracle as orc                        # noqa: E402  (geometry only)
from ransac_with_homography_amd import kernels              # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
H = np.load(os.path.join(ROOT, "tests", "golden", "g13_config4_x8.npz"))["H"]
h, w = 5464, 8192
mx, my, wt, ht = orc.output_bounds(h, w, H, 0)
(tsx, tsy, _, _), (qsx, qsy, _, _), (fw, fh) = orc.stitch_geometry(wt, ht, w, h, mx, my)
ih = np.linalg.inv(H)
rng = np.random.default_rng(0)


def image(np_dtype, c):
    v = rng.uniform(-20.0, 280.0, (h, w, c)).astype(np.float32)
    if np.dtype(np_dtype).kind in "ui":
        v = np.clip(v, 0, None)
    return torch.from_numpy(v.astype(np_dtype)).cuda()


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


print("canvas %d x %d, imgT / imgQ %d x %d, reps %d" % (fw, fh, w, h, REPS))
print("%-14s %-6s %9s %9s %10s %9s %7s" % ("images", "mode", "med ms", "min ms", "alg MB", "GB/s", "of 8TB/s"))
for name, dtype, c in (("float32 RGB", np.float32, 3), ("float64 RGB", np.float64, 3), ("uint16 RGB", np.uint16, 3),
                       ("uint8 RGBA", np.uint8, 4), ("uint8 RGB", np.uint8, 3)):
    T = image(dtype, c)
    Q = T.flip(0).contiguous()
    for mode, blend in (("paste", 0), ("Rate", 1)):
        cc = 3 if blend else c
        out = torch.empty((fh, fw, cc), dtype=torch.uint8, device="cuda")
        if name == "uint8 RGB":        # the uint8 exact kernel the any-dtype one generalises
            def fn():
                kernels.stitch_panorama(T, Q, ih, (mx, my), (wt, ht), (tsx, tsy), (qsx, qsy), (fh, fw), blend, 0.2, zero_origin=False)
            name_ = "uint8 RGB (u8)"
        else:
            def fn():
                kernels.stitch_panorama_ex(T, Q, ih, (mx, my), (wt, ht), (tsx, tsy), (qsx, qsy), (fh, fw), blend, 0.2,
                                           zero_origin=False, out=out)
            name_ = name
        med, mn = timed(fn)
        nbytes = 2 * T.numel() * T.element_size() + fh * fw * cc
        print("%-14s %-6s %9.3f %9.3f %10.1f %9.0f %6.1f%%" % (name_, mode, med, mn, nbytes / 1e6, nbytes / med / 1e6, 100 * nbytes / med / 1e6 / 8000))
    del T, Q
    torch.cuda.empty_cache()
