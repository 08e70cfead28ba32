"""The ratio matcher over a pair graph (rwh_match_ratio_graph) beside the cross-check matcher (rwh_match_hamming_batched) at the
three sizes profiles/match_ratio.txt records, in ONE process: tools/match_probe.py's two shapes -- 512 pairs of 500 x 500
descriptors of 32 bytes, one pair of 8192 x 8192 -- and a graph: 64 images of 500 rows, all 2016 pairs.

Per shape and matcher: the results are checked against the host twin first (all of the 8192 x 8192 pair, the last pair of the
others); then the library call (its four launches, outputs and workspace from torch's caching allocator, the tables already on
the device) is timed with device events over windows of CALLS back-to-back calls after warm-up, the two matchers' windows
ALTERNATING, median and minimum of WINDOWS windows each; the shader clock held meanwhile (kernels.ClockProbe beside a stretch of
the same calls); and the fraction of the VALU bound reached: descriptor pairs x the vector instructions the main kernel's loop
issues per pair (counted in the disassembly: INSTR below), each a 4-cycle issue per wave of 64 on one of the chip's CUs x 4 SIMDs
-- tools/match_probe.py's formula, so the figures stand beside profiles/match_hamming.txt's.  For the graph shape also: the
per-pair concatenation of the descriptors that `match_batch` pays before the cross-check call can start, and the descriptor
bytes resident either way.

    python tools/match_ratio_probe.py [windows] [calls] [shapes]

shapes: which of the three to run, e.g. "2" or "0,1" (default all) -- one shape per process keeps a kernel trace's rows apart
(rocprofv3 --kernel-trace --stats -- python tools/match_ratio_probe.py 3 20 2).
"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ransac_with_homography_amd import _lib, kernels        # noqa: E402

WINDOWS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
NBYTES = 32
RATIO = (7, 10)
SHAPES = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0, 1, 2]
# vector instructions per descriptor pair in the unrolled loops at 32 bytes, from the disassembly: cross-check 149 per 8 pairs
# (64 xor, 64 popcount, 8 add-shift, 8 or, 4 three-way minima, 1 move), ratio 79 per 4 pairs (32 xor, 32 popcount, 4 shift-or,
# 4 maxima, 4 minima, 2 three-way minima, 1 move)
INSTR = {"cross": 149.0 / 8.0, "ratio": 79.0 / 4.0}
dev = _lib.require_gpu()
lib = _lib.load()
CUS = torch.cuda.get_device_properties(dev).multi_processor_count
ptr = lambda t: ctypes.c_void_p(t.data_ptr())


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def alternating(fns, calls):
    """{name: (median, minimum) ms per call}: WINDOWS windows each, the functions taking turns."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            ts[k].append(window(fn, calls))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in ts.items()}


def clock_under(fn, ms_per_call):
    probe = kernels.ClockProbe(200.0)
    for _ in range(max(1, int(200.0 / max(ms_per_call, 1e-3)))):
        fn()
    torch.cuda.synchronize()
    return probe.mhz()


def cross_call(da, db, off_a, off_b):
    """rwh_match_hamming_batched with the tables on the device, as kernels.match_hamming_batched calls it."""
    P, total_a, total_b = off_a.shape[0] - 1, da.shape[0], db.shape[0]
    ws_bytes = int(lib.rwh_match_workspace_bytes(P, total_a, total_b))

    def fn():
        out = [torch.empty((total_a,), dtype=torch.int32, device=dev) for _ in range(2)]
        ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
        assert lib.rwh_match_hamming_batched(ptr(da), ptr(db), NBYTES, ptr(off_a), ptr(off_b), P, total_a, total_b, ptr(out[0]), ptr(out[1]),
                                             ptr(ws), ws_bytes, _lib.stream_ptr()) == 0
        return out
    return fn


def ratio_call(desc, off, pairs, total_query, total_train, max_train):
    """rwh_match_ratio_graph with the tables on the device, as kernels.match_ratio_graph calls it."""
    n_images, P = off.shape[0] - 1, pairs.shape[0]
    ws_bytes = int(lib.rwh_match_ratio_workspace_bytes(P, total_query, total_train, max_train))

    def fn():
        out = [torch.empty((total_query,), dtype=torch.int32, device=dev) for _ in range(3)]
        ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
        assert lib.rwh_match_ratio_graph(ptr(desc), NBYTES, ptr(off), n_images, desc.shape[0], ptr(pairs), P, total_query, total_train,
                                         RATIO[0], RATIO[1], ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(ws), ws_bytes, _lib.stream_ptr()) == 0
        return out
    return fn


def host_cross(A, B):
    t, d = np.empty(len(A), dtype=np.int32), np.empty(len(A), dtype=np.int32)
    assert lib.rwh_host_match_hamming(A.ctypes.data, len(A), B.ctypes.data, len(B), NBYTES, t.ctypes.data, d.ctypes.data) == 0
    return t, d


def host_ratio(A, B):
    o = [np.empty(len(A), dtype=np.int32) for _ in range(3)]
    assert lib.rwh_host_match_ratio(A.ctypes.data, len(A), B.ctypes.data, len(B), NBYTES, RATIO[0], RATIO[1], *[x.ctypes.data for x in o]) == 0
    return o


def report(name, which, med, mn, mhz, pairs, matches):
    bound_ms = pairs * INSTR[which] / (CUS * 64.0 * mhz * 1e6) * 1e3      # 64 lane-instructions per CU per clock (4 SIMDs x 16 lanes)
    print("%-24s %-11s matches %7d  call %.4f ms median / %.4f min  %.3e descriptor pairs/s  sclk %.0f MHz  VALU bound (%.3f instr/pair) "
          "%.4f ms  -> %.1f %% of the VALU bound" % (name, which, matches, med, mn, pairs / med * 1e3, mhz, INSTR[which], bound_ms,
                                                    100.0 * bound_ms / med))


def images_of(rng, n_images, rows):
    """Random rows; a third of every image's rows have a near partner at the same row of every other image (a common base)."""
    base = rng.integers(0, 256, (rows, NBYTES), dtype=np.uint8)
    out = rng.integers(0, 256, (n_images, rows, NBYTES), dtype=np.uint8)
    out[:, ::3] = base[None, ::3] ^ (rng.integers(0, 16, (n_images, len(base[::3]), NBYTES), dtype=np.uint8) == 0).astype(np.uint8)
    return out


def run(name, imgs, pair_list):
    """imgs: [n_images, rows, NBYTES]; pair_list: [(s, d)].  Both matchers on the same descriptor pairs."""
    n_images, rows = imgs.shape[:2]
    P = len(pair_list)
    pr = np.array(pair_list, dtype=np.int32)
    desc = torch.from_numpy(imgs.reshape(-1, NBYTES)).to(dev)
    off = torch.arange(0, n_images * rows + 1, rows, dtype=torch.int32, device=dev)
    ratio = ratio_call(desc, off, torch.from_numpy(pr).to(dev), P * rows, P * rows, rows)

    def concat():       # what match_batch does before its call: one copy of both sides per pair
        return torch.cat([desc[s * rows:(s + 1) * rows] for s, _ in pair_list]), torch.cat([desc[d * rows:(d + 1) * rows] for _, d in pair_list])
    da, db = concat()
    off_p = torch.arange(0, P * rows + 1, rows, dtype=torch.int32, device=dev)
    cross = cross_call(da, db, off_p, off_p)
    got_r = [x.cpu().numpy() for x in ratio()]
    got_c = [x.cpu().numpy() for x in cross()]
    for p in (range(P) if P == 1 else (P - 1,)):
        s, d = pair_list[p]
        sl = slice(p * rows, (p + 1) * rows)
        assert all(np.array_equal(g[sl], w) for g, w in zip(got_r, host_ratio(imgs[s], imgs[d]))), "ratio: GPU result differs from the host twin"
        assert all(np.array_equal(g[sl], w) for g, w in zip(got_c, host_cross(imgs[s], imgs[d]))), "cross-check: GPU result differs from the host twin"
    t = alternating({"ratio": ratio, "cross": cross}, CALLS)
    pairs = float(P) * rows * rows
    for which, fn, got in (("ratio", ratio, got_r), ("cross", cross, got_c)):
        med, mn = t[which]
        report(name, which, med, mn, clock_under(fn, med), pairs, int((got[0] >= 0).sum()))
    if n_images != 2 * P:                                   # the graph shape: what sharing the descriptors saves
        cm, cn = alternating({"concat": concat}, max(1, CALLS // 10))["concat"]
        print("%-24s per-pair concatenation in front of the cross-check call: %.4f ms median / %.4f min; descriptor bytes resident: %d "
              "once per image (ratio), %d once per pair (cross-check)" % (name, cm, cn, desc.numel(), da.numel() + db.numel()))
    del da, db, desc
    torch.cuda.empty_cache()


print("MI355X ratio matcher probe: %d CUs, %d windows of %d calls per matcher, alternating; descriptors of %d bytes, ratio %d / %d"
      % ((CUS, WINDOWS, CALLS, NBYTES) + RATIO))
rng = np.random.default_rng(0)
if 0 in SHAPES:
    A, B = images_of(rng, 2, 512 * 500).reshape(2, 512, 500, NBYTES)
    run("512 pairs of 500 x 500", np.stack([A, B], axis=1).reshape(1024, 500, NBYTES), [(2 * p, 2 * p + 1) for p in range(512)])
if 1 in SHAPES:
    run("one pair of 8192 x 8192", images_of(rng, 2, 8192), [(0, 1)])
if 2 in SHAPES:
    run("64 images x 500, 2016 pairs", images_of(rng, 64, 500), [(s, d) for d in range(64) for s in range(d + 1, 64)])
