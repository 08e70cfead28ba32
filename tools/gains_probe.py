"""The gain rule's GPU passes on tools/sequence_probe.py's strips (N = 2, 4, 8 frames of 1080p and 4K that overlap their neighbour
by 30 %): the overlap statistics (rwh_sequence_overlap_stats) at stride 1 and 4 beside the paste and feather passes of the same
strip, without gains and with them (rwh_stitch_sequence_ex), and the whole of homography.sequence_gains (statistics, one download,
the host solve).  Resident tensors, HIP events after warm-up.  The device tables are checked against each other (stride 1 twice)
before anything is timed; the gains are printed.

    python tools/gains_probe.py [reps]
"""
import os
import sys
import time

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


print("%-6s %2s %-16s %13s %9s %9s %12s" % ("frames", "N", "pass", "canvas", "med ms", "min ms", "Msamples/s"))
for name, (h, w) in (("1080p", (1080, 1920)), ("4K", (2160, 3840))):
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for _ in range(8)]
    for n in (2, 4, 8):
        imgs = frames[:n]
        Hs = [pair_h(w)] * (n - 1)
        Gs, rects, origin, (fh, fw), order = hg.sequence_plan([(h, w, 3)] * n, Hs)
        inv = np.stack([np.eye(3) if i == 0 else np.linalg.inv(Gs[i]) for i in range(n)])
        geom = kernels.SeqGeometry(inv, rects, (fh, fw), 0, origin)
        out = torch.empty((fh, fw, 3), dtype=torch.uint8, device="cuda")
        one = kernels.sequence_overlap_tables_on(imgs, geom, 1)
        two = kernels.sequence_overlap_tables_on(imgs, geom, 1)
        assert bool((one == two).all()) and int(one[0, 0, 0]) == h * w, "the statistics are not reproducible"
        gains = hg.sequence_gains(imgs, Hs=Hs)

        def line(what, med, mn, samples):
            print("%-6s %2d %-16s %6d x %-5d %9.3f %9.3f %12.0f" % (name, n, what, fw, fh, med, mn, samples / med / 1e3))
        for stride in (1, 4):
            med, mn = timed(lambda: kernels.sequence_overlap_tables_on(imgs, geom, stride))
            line("stats stride %d" % stride, med, mn, -(-fw // stride) * -(-fh // stride))
        for mode, blend in (("paste", _lib.RWH_SEQ_PASTE), ("feather", _lib.RWH_SEQ_FEATHER)):
            for g in (None, gains):
                med, mn = timed(lambda: kernels.stitch_sequence_on(imgs, geom, order, blend, out=out, gains=g))
                line(mode + (" + gains" if g is not None else ""), med, mn, fw * fh)
        t0 = time.perf_counter()
        for _ in range(REPS):
            hg.sequence_gains(imgs, Hs=Hs)
        wall = (time.perf_counter() - t0) / REPS * 1e3
        print("%-6s %2d %-16s %6d x %-5d %9.3f   (wall clock per call: statistics at stride 4, download, host solve)   gains %s"
              % (name, n, "sequence_gains", fw, fh, wall, np.round(gains, 4).tolist()))
    del frames
    torch.cuda.empty_cache()
