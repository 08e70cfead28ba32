"""The camera rule's GPU pass beside the bundle rule's, and both adjustments, timed on the same edges at two sizes: the GRID scene of
tests/bundle_cases.py (N = 8, its 25 pairs of 35 .. 400 rows) and N = 64 turning cameras with all 2016 pairs of 300 rows.  Per
size: rwh_camera_blocks and rwh_bundle_blocks alone (resident tensors, HIP events after warm-up, the upload of the E x 15 records or
E x 9 transfers included: `kernels.camera_blocks` / `kernels.bundle_blocks` are the units the drivers call), the camera rule's host
twin beside them for scale (wall clock), and `homography.sequence_adjust_cameras` (both focal models) and `sequence_adjust` from the
same start (wall clock per call, everything included).  The device blocks are checked against the twin's, bit for bit, before
anything is timed.

    python tools/cameras_probe.py [reps]
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
import camera_cases as cc                                                   # noqa: E402
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
    """n cameras of 1920 x 1080, focal 1500, 0.008 rad apart with a little pitch and roll; every pair (s > d) with `rows` matches
    spread over image s, 0.5 px noise on b.  The start: the true rotations, every one but the anchor's turned by about 1 mrad, and
    a focal 5 % off."""
    rng = np.random.default_rng(seed)
    shapes = [(1080, 1920)] * n
    Rs = np.stack([np.eye(3)] + [cc.rodrigues(np.array([rng.uniform(-0.01, 0.01), 0.008 * i, rng.uniform(-0.01, 0.01)])) for i in range(1, n)])
    fs = np.full(n, 1500.0)
    pairs = [(s, d) for d in range(n) for s in range(d + 1, n)]
    matches = []
    for s, d in pairs:
        a = (rng.uniform(0, 1, (rows, 2)) * [1919.0, 1079.0]).astype(np.float32)
        matches.append((a, (bc.project(cc.transfer(shapes, Rs, fs, s, d), a) + rng.normal(0, 0.5, (rows, 2))).astype(np.float32)))
    start = np.stack([Rs[0]] + [R @ cc.rodrigues(rng.normal(0, 1e-3, 3)) for R in Rs[1:]])
    return dict(n=n, shapes=shapes, pairs=pairs, matches=matches, Rs=start, fs=np.full(n, 1575.0))


def probe(name, case):
    shapes, pairs, Rs, fs = case["shapes"], case["pairs"], case["Rs"], case["fs"]
    pa, pb, offsets = bc.concatenated(case["matches"])
    E, rows = len(pairs), len(pa)
    masks = np.full((E, max((int(np.diff(offsets).max()) + 63) // 64, 1)), -1, dtype=np.int64)
    rec = hg._camera_records(shapes, Rs, fs, pairs)
    Gs = hg.sequence_camera_maps(shapes, Rs, fs)
    T = hg._bundle_transfers(Gs, pairs)
    dev = [torch.from_numpy(x).cuda() for x in (pa, pb, offsets, masks)]
    got = kernels.camera_split(kernels.camera_blocks(*dev, rec).cpu().numpy())
    want = kernels.host_camera_blocks(pa, pb, offsets, masks, rec)
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and np.array_equal(got[1], want[1]), "device blocks differ from the twin's"
    cam = device_ms(lambda: kernels.camera_blocks(*dev, rec))
    bun = device_ms(lambda: kernels.bundle_blocks(*dev, T))
    host = wall_ms(lambda: kernels.host_camera_blocks(pa, pb, offsets, masks, rec), max(REPS // 4, 2))
    for what, (med, mn) in (("camera_blocks", cam), ("bundle_blocks", bun)):
        print("%-10s N %2d  E %4d  rows %6d  %s  device %8.3f ms median %8.3f min  (%7.1f Mrows/s)"
              % (name, case["n"], E, rows, what, med, mn, rows / med / 1e3))
    print("%-10s N %2d  E %4d  rows %6d  camera_blocks  host twin %9.3f ms" % (name, case["n"], E, rows, host))
    reps = max(REPS // 4, 2)
    for focals in ("shared", "per-image"):
        info = {}
        ms = wall_ms(lambda: hg.sequence_adjust_cameras(shapes, Rs, fs, pairs, case["matches"], focals=focals, on="device", info=info), reps)
        print("%-10s sequence_adjust_cameras focals=%-9s %9.2f ms per call   cost %.1f -> %.1f in %d accepted steps"
              % (name, focals, ms, info["cost"][0], info["cost"][-1], info["iters"]))
    info = {}
    ms = wall_ms(lambda: hg.sequence_adjust(Gs, pairs, case["matches"], on="device", info=info), reps)
    print("%-10s sequence_adjust (8 per image)            %9.2f ms per call   cost %.1f -> %.1f in %d accepted steps"
          % (name, ms, info["cost"][0], info["cost"][-1], info["iters"]))


_lib.load()
_lib.require_gpu()
scene, shapes, _, _ = cc.grid_cameras()
Rs0, fs0 = hg.sequence_cameras(shapes, scene["Gs"], 120.0)
probe("GRID", dict(scene, shapes=shapes, Rs=Rs0, fs=fs0))
probe("all pairs", all_pairs_case())
