"""The block gain rule's passes on tools/gains_probe.py's strips (N = 2, 4, 8 frames of 1080p and 4K that overlap their neighbour by
30 %), on the anchor's plane and on a cylinder: the cell statistics (rwh_sequence_cell_stats, block 32, stride 1) beside the overlap
statistics of the gain rule at the same stride and geometry (rwh_sequence_overlap_stats, a kernel this rule leaves as it was), the
download size of the cell table, the host solve (rwh_host_sequence_block_gains, wall clock), and every map-taking compositor beside
its form with one gain per image (the label plane is n vertical stripes).  Resident tensors, HIP events after warm-up, medians and minima of `reps` runs.  Before anything is
timed the cell table is checked against the overlap tables (scattered to image indices and summed over the cells it must equal them).

    python tools/block_gains_probe.py [reps] [out.txt]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ransac_with_homography_amd import _lib, homography as hg, kernels      # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
OUT = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
BLOCK, STRIDE, BANDS = 32, 1, 5


def say(text):
    print(text, flush=True)
    if OUT is not None:
        OUT.write(text + "\n")
        OUT.flush()


def timed(fn):
    for _ in range(2):
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


def strip(canvas, n, h, w):
    """-> (Hs, anchor, stitchSequence's projection arguments).  plane: tools/gains_probe.py's strip, frame i + 1 lies 70 % of a frame
    right of frame i, anchor 0.  cylinder: tools/projection_probe.py's sweep scaled to the frame, a camera with f = 1500 px at 1080p
    that turns 15 degrees per frame with a little pitch and roll, the middle frame the anchor."""
    if canvas == "plane":
        return [np.array([[1.01, 0.004, 0.7 * w], [0.003, 0.995, 6.5], [2e-6, 1e-6, 1.0]])] * (n - 1), 0, {}
    f = 1500.0 * w / 1920.0
    K = np.array([[f, 0.0, (w - 1) / 2.0], [0.0, f, (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    cy, sy, cp, sp, cr, sr = np.cos(np.deg2rad(15.0)), np.sin(np.deg2rad(15.0)), np.cos(0.004), np.sin(0.004), np.cos(0.002), np.sin(0.002)
    R = (np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]) @ np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
         @ np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]]))
    return [K @ R @ np.linalg.inv(K)] * (n - 1), n // 2, dict(projection="cylindrical", focal=f)


def scattered(tabs, geom, n):
    """The cell table scattered back to image indices and summed over the cells -> (count, sum) int64 [n, n]."""
    cand = kernels.sequence_cell_candidates(geom, n, BLOCK)
    count, total = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    for gy, gx in zip(*np.nonzero(cand.any(axis=2))):
        c = np.flatnonzero(cand[gy, gx])
        count[np.ix_(c, c)] += tabs[gy, gx, 0, :len(c), :len(c)]
        total[np.ix_(c, c)] += tabs[gy, gx, 1, :len(c), :len(c)]
    return count, total


say("%-6s %-8s %2s %-26s %13s %9s %9s" % ("frames", "canvas", "N", "pass", "canvas", "med ms", "min ms"))
for name, (h, w) in (("1080p", (1080, 1920)), ("4K", (2160, 3840))):
    rng = np.random.default_rng(0)
    frames = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for _ in range(8)]
    for canvas in ("plane", "cylinder"):
        for n in (2, 4, 8):
            imgs = frames[:n]
            Hs, anchor, kw = strip(canvas, n, h, w)
            order, geom = hg._sequence_geometry("block_gains_probe", imgs, Hs, None, anchor, kw.get("projection"), kw.get("focal"))
            geom = geom.on_device(imgs[0].device)
            fh, fw = geom.size
            out = torch.empty((fh, fw, 3), dtype=torch.uint8, device="cuda")

            def line(what, med, mn):
                say("%-6s %-8s %2d %-26s %6d x %-5d %9.3f %9.3f" % (name, canvas, n, what, fw, fh, med, mn))
            cells = kernels.sequence_cell_tables_on(imgs, geom, BLOCK, STRIDE)
            tabs = cells.cpu().numpy().view(np.uint32)
            flat = kernels.sequence_overlap_tables_on(imgs, geom, STRIDE).cpu().numpy()
            got = scattered(tabs.astype(np.int64), geom, n)
            assert np.array_equal(got[0], flat[0]) and np.array_equal(got[1], flat[1]), "the cells do not sum to the overlap statistics"
            line("overlap stats stride %d" % STRIDE, *timed(lambda: kernels.sequence_overlap_tables_on(imgs, geom, STRIDE)))
            line("cell stats B %d stride %d" % (BLOCK, STRIDE), *timed(lambda: kernels.sequence_cell_tables_on(imgs, geom, BLOCK, STRIDE)))
            base = hg.sequence_gains(imgs, Hs=Hs, anchor=anchor, **kw)
            t0 = time.perf_counter()
            for _ in range(REPS):
                status, maps = kernels.host_sequence_block_gains(tabs, geom, n, BLOCK, base)
            solve = (time.perf_counter() - t0) / REPS * 1e3
            assert status == 0
            say("%-6s %-8s %2d %-26s %6d x %-5d %9.3f   (wall clock; table %d x %d cells, K = %d, %.2f MB to download)"
                % (name, canvas, n, "host solve", fw, fh, solve, tabs.shape[1], tabs.shape[0], tabs.shape[-1], tabs.nbytes / 1e6))
            by_maps = kernels.SeqGainMaps(torch.from_numpy(maps).cuda(), BLOCK)
            labels = (torch.arange(fw, device="cuda") * n // fw).to(torch.uint8).expand(fh, fw).contiguous()     # n vertical stripes
            for g, tag in ((base, "gains"), (by_maps, "maps")):
                line("paste + " + tag, *timed(lambda: kernels.stitch_sequence_on(imgs, geom, order, _lib.RWH_SEQ_PASTE, out=out, gains=g)))
                line("feather + " + tag, *timed(lambda: kernels.stitch_sequence_on(imgs, geom, order, _lib.RWH_SEQ_FEATHER, out=out, gains=g)))
                line("label paste + " + tag, *timed(lambda: kernels.stitch_sequence_labels_on(imgs, geom, labels, gains=g, out=out)))
                line("multiband %d + %s" % (BANDS, tag), *timed(lambda: kernels.stitch_sequence_multiband_on(imgs, geom, BANDS, gains=g, out=out)))
                line("multiband %d labels + %s" % (BANDS, tag),
                     *timed(lambda: kernels.stitch_sequence_multiband_on(imgs, geom, BANDS, gains=g, out=out, labels=labels)))
            del out, cells, labels, by_maps
            torch.cuda.empty_cache()
    del frames
    torch.cuda.empty_cache()
