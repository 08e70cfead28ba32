"""The seam finder (rwh_sequence_seams) on tools/multiband_probe.py's strips (N = 2, 4, 8 frames of 1080p and 4K that overlap their
neighbour by 30 %): the time of kernels.sequence_seams and its pass count, and stitchSequence's two compositors beside their
labelled forms -- multi-band with 5 bands without seams, with a label plane given, and with the seams found in the call -- in the
same run.  Resident tensors, HIP events after warm-up; every time includes the launcher's workspace allocation (a cached torch
block after the first call), and sequence_seams' includes the host's reads of the flag, which synchronise the stream.  The labels
are checked against a second run before anything is timed.  The frames are independent noise, so their overlaps disagree nearly
everywhere (c = 1): fronts cross them at one cost unit per pixel.  The second table repeats the 1080p rows on frames cut from
one smooth scene, which agree in their overlaps (c = tau): the case seam finding is for.  The shader clock under each load is
printed (rwh_lab_clock_probe beside the timed calls).

    python tools/seams_probe.py [reps]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ransac_with_homography_amd import _lib, homography as hg, kernels      # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    probe = kernels.ClockProbe(20.0)
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), probe.mhz()


def pair_h(w):
    return np.array([[1.01, 0.004, 0.7 * w], [0.003, 0.995, 6.5], [2e-6, 1e-6, 1.0]])


def smooth_scene(h, w, seed, cell=24):
    """Seeded values on a coarse grid, interpolated bilinearly: uint8 [h, w, 3]."""
    rng = np.random.default_rng(seed)
    grid = rng.uniform(30, 225, (h // cell + 2, w // cell + 2, 3))
    y, x = np.arange(h) / cell, np.arange(w) / cell
    iy, ix = y.astype(int), x.astype(int)
    fy, fx = (y - iy)[:, None, None], (x - ix)[None, :, None]
    top = grid[iy][:, ix] * (1 - fx) + grid[iy][:, ix + 1] * fx
    bot = grid[iy + 1][:, ix] * (1 - fx) + grid[iy + 1][:, ix + 1] * fx
    return np.rint(top * (1 - fy) + bot * fy).astype(np.uint8)


def run(name, frames, Hs, h, w):
    n = len(frames)
    Gs, rects, origin, (fh, fw), order = hg.sequence_plan([(h, w, 3)] * n, Hs)
    inv = np.stack([np.eye(3) if i == 0 else np.linalg.inv(Gs[i]) for i in range(n)])
    rc = np.ascontiguousarray(rects, dtype=np.int32)
    out = torch.empty((fh, fw, 3), dtype=torch.uint8, device="cuda")
    lab = torch.empty((fh, fw), dtype=torch.uint8, device="cuda")
    info = {}
    geom = kernels.SeqGeometry(inv, rects, (fh, fw), 0, origin)
    one = kernels.sequence_seams_on(frames, geom, info=info).clone()
    two = kernels.sequence_seams_on(frames, geom)
    assert bool((one == two).all()), "the labels are not reproducible"
    need = _lib.load().rwh_sequence_seams_workspace_bytes(rc.ctypes.data, n, fh, fw, int(origin[0]), int(origin[1]))

    def line(what, t, extra=""):
        print("%-7s %2d %-26s %6d x %-5d %9.3f %9.3f %8.0f %10.0f  %s" % (name, n, what, fw, fh, t[0], t[1], t[2], fw * fh / t[0] / 1e3, extra))
    line("sequence_seams", timed(lambda: kernels.sequence_seams_on(frames, geom, out=lab)),
         "%d passes, workspace %d MiB" % (info["passes"], need >> 20))
    line("paste", timed(lambda: kernels.stitch_sequence_on(frames, geom, order, _lib.RWH_SEQ_PASTE, out=out)))
    line("label paste (plane given)", timed(lambda: kernels.stitch_sequence_labels_on(frames, geom, lab, out=out)))
    line("multiband 5", timed(lambda: kernels.stitch_sequence_multiband_on(frames, geom, 5, out=out)))
    line("multiband 5 (plane given)", timed(lambda: kernels.stitch_sequence_multiband_on(frames, geom, 5, out=out, labels=lab)))
    line("stitchSequence multiband", timed(lambda: hg.stitchSequence(frames, Hs=Hs, blending="multiband")))
    line("stitchSequence mb + seams", timed(lambda: hg.stitchSequence(frames, Hs=Hs, blending="multiband", seams=True)))


print("%-7s %2s %-26s %14s %9s %9s %8s %10s" % ("frames", "N", "call", "canvas", "med ms", "min ms", "MHz", "Mpixel/s"))
for name, (h, w) in (("1080p", (1080, 1920)), ("4K", (2160, 3840))):
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for _ in range(8)]
    for n in (2, 4, 8):
        run(name, frames[:n], [pair_h(w)] * (n - 1), h, w)
    del frames
    torch.cuda.empty_cache()
print("frames cut from one smooth scene, integer steps of 0.7 w: the overlaps agree")
h, w = 1080, 1920
for n in (2, 4):
    step = int(0.7 * w)
    scene = smooth_scene(h, step * (n - 1) + w, 11)
    frames = [torch.from_numpy(np.ascontiguousarray(scene[:, i * step:i * step + w])).cuda() for i in range(n)]
    Hs = [np.array([[1.0, 0.0, float(step)], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])] * (n - 1)
    run("smooth", frames, Hs, h, w)
