"""The ring forms of the sequence compositor (the ring rule of include/rwh.h) beside the projected forms, on the same images, the
same tables and the same canvas: 8 frames of 1080p from a camera with f = 1500 px that turns 15 degrees per frame, anchor in the
middle, on the wrap-around cylinder of period P = sequence_period(1500).  No frame of that sweep lies across the seam, so the
projected entry points take the ring's tables as they are and both forms write the same bytes (checked here); the ring form does
the projected form's work plus one compare and add per candidate.  Every pass is timed twice per form, interleaved
(proj, ring, proj, ring), so the table shows the probe's own run-to-run spread beside the difference.  Then the ring forms alone on
24 frames, the full circle.  Resident tensors, HIP events after warm-up.  Passes: paste, feather, the overlap statistics at stride
4, multi-band with 5 bands.

    python tools/ring_probe.py [reps]
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
    cy, sy, cp, sp, cr, sr = np.cos(YAW), np.sin(YAW), np.cos(0.0004), np.sin(0.0004), np.cos(0.0002), np.sin(0.0002)
    R = (np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]]) @ np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
         @ np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]]))
    return K @ R @ np.linalg.inv(K)


def passes(imgs, geom, order, out):
    return [("paste", lambda: kernels.stitch_sequence_on(imgs, geom, order, _lib.RWH_SEQ_PASTE, out=out)),
            ("feather", lambda: kernels.stitch_sequence_on(imgs, geom, order, _lib.RWH_SEQ_FEATHER, out=out)),
            ("stats 4", lambda: kernels.sequence_overlap_tables_on(imgs, geom, 4)),
            ("multiband 5", lambda: kernels.stitch_sequence_multiband_on(imgs, geom, 5, out=out))]


rng = np.random.default_rng(0)
frames = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(24)]
print("%-2s %-12s %13s %7s | %9s %9s | %9s %9s | %s" % ("N", "pass", "canvas", "Mpix", "proj ms", "ring ms", "proj ms", "ring ms", "ring / proj (medians of both rounds)"))
for n in (8, 24):
    imgs, anchor = frames[:n], 0 if n == 24 else n // 2
    rects, origin, (fh, fw), order, mats, rays = hg._sequence_inputs("ring_probe", imgs, [pair_h()] * (n - 1), None, anchor, "cylindrical", F, True)
    ring = kernels.SeqGeometry(mats, rects, (fh, fw), rays=rays, ring=True).on_device(imgs[0].device)
    geoms = {"ring": ring, "proj": ring._replace(ring=False)}
    both = not any(r[0] + r[2] > fw for r in rects)        # no rectangle passes the edge: the projected forms take these tables too
    outs = {form: torch.zeros((fh, fw, 3), dtype=torch.uint8, device="cuda") for form in ("proj", "ring")}
    forms = {form: passes(imgs, geoms[form], order, outs[form]) for form in (("proj", "ring") if both else ("ring",))}
    for k, (mode, ring_fn) in enumerate(forms["ring"]):
        if both:
            proj_fn = forms["proj"][k][1]
            rounds = [(timed(proj_fn)[0], timed(ring_fn)[0]) for _ in range(2)]
            got_p, got_r = proj_fn(), ring_fn()
            torch.cuda.synchronize()
            same = torch.equal(got_p, got_r) if mode == "stats 4" else torch.equal(outs["proj"], outs["ring"])
            ratio = np.median([r[1] for r in rounds]) / np.median([r[0] for r in rounds])
            print("%-2d %-12s %6d x %-5d %7.2f | %9.3f %9.3f | %9.3f %9.3f | %.3f%s"
                  % (n, mode, fw, fh, fh * fw / 1e6, rounds[0][0], rounds[0][1], rounds[1][0], rounds[1][1], ratio, "" if same else "  OUTPUTS DIFFER"))
        else:
            rounds = [timed(ring_fn)[0] for _ in range(2)]
            print("%-2d %-12s %6d x %-5d %7.2f | %9s %9.3f | %9s %9.3f | full circle: %d rectangles pass the edge"
                  % (n, mode, fw, fh, fh * fw / 1e6, "-", rounds[0], "-", rounds[1], sum(r[0] + r[2] > fw for r in rects)))
    del outs
    torch.cuda.empty_cache()
