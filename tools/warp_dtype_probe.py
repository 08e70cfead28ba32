"""The any-dtype exact warp (warp_any, rwh_warp_backward with RWH_WARP_EXACT) on a 4K RGB frame: 2160 x 3840 x 3 resident tensors,
a mild perspective homography, nearest and bilinear (float64 out) for float64, uint16 and float16 sources, the float32 exact
kernel (warp_exact) beside them; HIP events after warm-up.  GB/s counts the source read once plus the destination written once.
Then the end-to-end numpy call for a uint16 image (upload, warp, download, as wrapPerspective does): the image as it is, and the
path the package took before (a host cast to float32, the float32 kernel on twice the bytes, the nearest result cast back).

    python tools/warp_dtype_probe.py [reps] [--kernels-only]     (--kernels-only: no end-to-end leg, for a kernel trace)
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import homography as hg                                      # noqa: E402
from oracle import rwh_oracle as orc                        # noqa: E402  (geometry only)
from ransac_with_homography_amd import kernels              # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REPS = int(ARGS[0]) if ARGS else 20
h, w, c = 2160, 3840, 3
H = np.array([[0.97, 0.02, 40.5], [-0.015, 1.01, 30.25], [-3e-6, 2e-6, 1.0]])
mx, my, wt, ht = orc.output_bounds(h, w, H, 0)
grid = kernels.Grid(mx, mx + wt - 1, wt, my, my + ht - 1, ht)
ih = np.linalg.inv(H)
rng = np.random.default_rng(0)
base = rng.uniform(0.0, 255.0, (h, w, c))


def timed(fn, reps=REPS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def wall(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


print("source %d x %d x %d, output %d x %d, reps %d" % (h, w, c, wt, ht, REPS))
print("%-9s %-9s %-34s %8s %8s %9s %7s" % ("source", "interp", "kernel", "med ms", "min ms", "alg MB", "GB/s"))
for name, dt in (("float64", torch.float64), ("uint16", torch.uint16), ("float16", torch.float16), ("float32", torch.float32)):
    src = torch.from_numpy(base).to(torch.float32).cuda()
    src = src.to(dt) if dt != torch.uint16 else torch.from_numpy(base.astype(np.uint16)).cuda()
    for interp in ("nn", "bilinear"):
        out_dtype = src.dtype if interp == "nn" else torch.float64
        out = torch.empty((ht, wt, c), dtype=out_dtype, device="cuda")
        kname = kernels.warp_plan(tuple(src.shape), src.dtype, ih, grid, (h, w), interp, out_dtype, exact=True)

        def fn():
            kernels.warp_backward(src, ih, grid, (h, w), interp, out_dtype, zero_origin=False, out=out, exact=True)
        med, mn = timed(fn)
        nbytes = src.numel() * src.element_size() + out.numel() * out.element_size()
        print("%-9s %-9s %-34s %8.3f %8.3f %9.1f %7.0f" % (name, interp, kname, med, mn, nbytes / 1e6, nbytes / med / 1e6))
    del src, out
    torch.cuda.empty_cache()

if "--kernels-only" in sys.argv:
    sys.exit(0)
print()
print("end to end, numpy uint16 image in (wrapPerspective, upload + warp + download), ms: median / min of %d calls" % REPS)
img16 = base.astype(np.uint16)
for conv in ("nn", "bilinear"):
    now = wall(lambda: hg.wrapPerspective(img16, H, conv))

    def before():       # what the package did before: the host cast to float32, the float32 kernel, the nearest result cast back
        r = hg.wrapPerspective(img16.astype(np.float32), H, conv)[0]
        return r.astype(np.uint16) if conv == "nn" else r
    prev = wall(before)
    print("  %-9s own dtype %8.2f / %8.2f    before (float32 cast) %8.2f / %8.2f" % (conv, now[0], now[1], prev[0], prev[1]))
