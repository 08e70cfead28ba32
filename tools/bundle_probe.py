"""The bundle rule's GPU pass and a whole adjustment, timed at two sizes: the GRID scene of tests/bundle_cases.py (N = 8, its 25
pairs of 35 .. 400 rows) and N = 64 with all 2016 pairs of 300 rows.  Per size: rwh_bundle_blocks alone (resident tensors, HIP
events after warm-up, the upload of the E x 9 transfers included: `kernels.bundle_blocks` is the unit the driver calls), the host
twin on the same input beside it for scale (wall clock), and `homography.sequence_adjust` on the device and on the host (wall
clock per call, everything included).  The device blocks are checked against the twin's, bit for bit, before anything is timed.

    python tools/bundle_probe.py [reps]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bundle_cases as bc                                                   # noqa: E402
from ransac_with_homography_amd import _lib, homography as hg, kernels      # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def device_ms(fn):
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


def wall_ms(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def all_pairs_case(n=64, rows=300, seed=64):
    """n images on a line, 12 px apart with a small affine and perspective part; every pair (s > d) with `rows` matches."""
    rng = np.random.default_rng(seed)
    Gs = [np.eye(3)]
    for i in range(1, n):
        G = np.eye(3) + np.array([[0.02, 0.02, 0.0], [0.02, 0.02, 0.0], [1e-5, 1e-5, 0.0]]) * rng.uniform(-1, 1, (3, 3))
        G[0, 2], G[1, 2] = 12.0 * i, rng.uniform(-4, 4)
        Gs.append(G)
    Gs = np.stack(Gs)
    pairs = [(s, d) for d in range(n) for s in range(d + 1, n)]
    T = bc.transfers(Gs, pairs)
    matches = []
    for e in range(len(pairs)):
        a = (rng.uniform(0, 1, (rows, 2)) * [1919.0, 1079.0]).astype(np.float32)
        matches.append((a, (bc.project(T[e], a) + rng.normal(0, 0.5, (rows, 2))).astype(np.float32)))
    # the start of the adjustment: the truth, every map but the anchor's disturbed by about a pixel
    start = Gs.copy()
    start[1:, :2, 2] += rng.normal(0, 1.0, (n - 1, 2))
    return dict(n=n, Gs=Gs, pairs=pairs, matches=matches, start=start)


def probe(name, case, start):
    pa, pb, offsets = bc.concatenated(case["matches"])
    E, rows = len(case["pairs"]), len(pa)
    masks = np.full((E, max((int(np.diff(offsets).max()) + 63) // 64, 1)), -1, dtype=np.int64)
    T = bc.transfers(start, case["pairs"])
    dev = [torch.from_numpy(x).cuda() for x in (pa, pb, offsets, masks)]
    got = kernels.bundle_split(kernels.bundle_blocks(*dev, T).cpu().numpy())
    want = kernels.host_bundle_blocks(pa, pb, offsets, masks, T)
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(got[1], want[1]), "device blocks differ from the twin's"
    med, mn = device_ms(lambda: kernels.bundle_blocks(*dev, T))
    host = wall_ms(lambda: kernels.host_bundle_blocks(pa, pb, offsets, masks, T), max(REPS // 4, 2))
    print("%-12s N %2d  E %4d  rows %6d  bundle_blocks   device %8.3f ms median %8.3f min  (%7.1f Mrows/s)   host twin %9.3f ms"
          % (name, case["n"], E, rows, med, mn, rows / med / 1e3, host))
    for on in ("device", "host"):
        info = {}
        ms = wall_ms(lambda: hg.sequence_adjust(start, case["pairs"], case["matches"], on=on, info=info), 2 if on == "host" else max(REPS // 4, 2))
        print("%-12s N %2d  E %4d  rows %6d  sequence_adjust on=%-6s %9.2f ms per call   cost %.1f -> %.1f in %d accepted steps"
              % (name, case["n"], E, rows, on, ms, info["cost"][0], info["cost"][-1], info["iters"]))


lib = _lib.load()
_lib.require_gpu()
grid = bc.grid_scene()
probe("GRID", grid, bc.snake_start(lib, grid))
big = all_pairs_case()
probe("all pairs", big, big["start"])
