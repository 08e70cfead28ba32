"""The feature extractor (features.extract_batch: rwh_orb_detect_batched -> one sort -> rwh_orb_describe_batched) at the two sizes
profiles/extract_orb.txt records: one 683 x 1024 RGB image (tests/golden/img_foto1.npz A), and a batch of 64 (A and B alternating,
each shifted by a few rows so that no two are the same), threshold 20, n_features 500, 32-byte descriptors.

Per case, by device events over windows of CALLS back-to-back calls after warm-up, median and minimum of WINDOWS windows: the
detect call (two memsets, the tile prefix, the tiled kernel), the describe call (one launch) and the whole extract_batch (upload of
nothing -- the images are device tensors --, both calls, the sort, and the one download of the counts, which synchronises).  Each
is set against two numbers measured in the same run: the host twin (rwh_host_orb_extract_pyramid, one core, per image) on the same
input, and a plain device copy of the buffer's bytes (torch's copy kernel: the floor for a kernel that reads every pixel once).  The
results are checked against the host twin first.

--levels N (default 1): the scale pyramid (rules 6 - 8 of include/rwh.h, `extract_batch(n_levels=N)`).  With N > 1 the pyramid call
(rwh_orb_pyramid_batched: its tile prefix and the kernel that makes levels 1 .. N - 1 of the whole batch) is timed too, detect, the
sort and describe run over the n * N rows of the table, and the copy set beside the pyramid call moves as many bytes as it reads
and writes.  The buffer and the table of the separate calls are features.orb_layout's, as extract_batch's are.

    python tools/orb_probe.py [windows] [calls] [--levels N]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ransac_with_homography_amd import _lib, kernels        # noqa: E402
from ransac_with_homography_amd import features as ft       # noqa: E402

ARGS = list(sys.argv[1:])
LEVELS = 1
if "--levels" in ARGS:
    at = ARGS.index("--levels")
    LEVELS = int(ARGS[at + 1])
    del ARGS[at:at + 2]
WINDOWS = int(ARGS[0]) if len(ARGS) > 0 else 11
CALLS = int(ARGS[1]) if len(ARGS) > 1 else 20
N_FEATURES, THRESHOLD, NBYTES = 500, 20, 32
dev = _lib.require_gpu()
lib = _lib.load()


def windows(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / calls * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def case(name, images):
    """One of the two sizes with LEVELS levels: scales and quotas are extract_batch's defaults, buffer and table features.orb_layout's."""
    table, rot = ft.orb_bin_table(), np.ascontiguousarray(ft.rotate_pattern(ft.default_pattern(NBYTES)))
    scales = ft.orb_scales(LEVELS)
    quotas = ft.orb_level_quotas(N_FEATURES, scales)
    room = int(quotas.sum())
    dev_images = [torch.from_numpy(im).to(dev) for im in images]
    extract = lambda: ft.extract_batch(dev_images, n_features=N_FEATURES, threshold=THRESHOLD, nbytes=NBYTES, n_levels=LEVELS)
    feats = extract()
    host_s, picks = 0.0, sorted(set((0, len(images) - 1)))
    for i in picks:
        im = images[i]
        kps, desc = np.empty((room, 2), np.float32), np.empty((room, NBYTES), np.uint8)
        score, bins, level = (np.empty(room, np.int32) for _ in range(3))
        size, count = np.empty(room, np.float32), np.zeros(1, np.int32)
        t = time.perf_counter()
        st = lib.rwh_host_orb_extract_pyramid(im.ctypes.data, im.shape[0], im.shape[1], 3, THRESHOLD, scales.ctypes.data, quotas.ctypes.data,
                                              LEVELS, table.ctypes.data, rot.ctypes.data, NBYTES, kps.ctypes.data, desc.ctypes.data,
                                              score.ctypes.data, bins.ctypes.data, level.ctypes.data, size.ctypes.data, count.ctypes.data, None)
        host_s += time.perf_counter() - t
        assert st == 0
        assert np.array_equal(feats[i][0].cpu().numpy(), kps[:count[0]]) and np.array_equal(feats[i][1].cpu().numpy(), desc[:count[0]]), "device != host twin"
    # the library calls on their own, on the buffer and table extract_batch would hand them
    rows, head, po, go, _ = ft.orb_layout([im.shape for im in images], scales)
    src = torch.cat([t.reshape(-1) for t in dev_images] + [torch.empty((po - head,), dtype=torch.uint8, device=dev)])
    tab = torch.from_numpy(rows).to(dev)
    cap = 1 << 16
    if LEVELS > 1:
        kernels.orb_pyramid_batched(src, head, tab, scales)
    gray, keys, counts = kernels.orb_detect_batched(src, tab, go, THRESHOLD, cap)
    assert int(counts.max()) <= cap
    keys = torch.sort(keys, dim=1).values
    clamped = torch.minimum(counts, torch.from_numpy(np.tile(quotas, len(images))).to(dev))
    bt, pt = torch.from_numpy(table).to(dev), torch.from_numpy(rot).to(dev)
    out_keys, nf = torch.empty_like(keys), int(quotas.max())
    if LEVELS > 1:
        t_pyr = windows(lambda: kernels.orb_pyramid_batched(src, head, tab, scales), CALLS)
    t_detect = windows(lambda: kernels.orb_detect_batched(src, tab, go, THRESHOLD, cap, out_keys=out_keys), CALLS)
    t_describe = windows(lambda: kernels.orb_describe_batched(gray, go, tab, keys, clamped, nf, bt, pt), CALLS)
    t_sort = windows(lambda: torch.sort(out_keys, dim=1), CALLS)
    t_all = windows(extract, max(CALLS // 4, 2))
    if LEVELS > 1:
        half = (po + 1) // 2                                                   # a copy of half the bytes reads and writes head + planes in all
        a, b = torch.empty((half,), dtype=torch.uint8, device=dev), torch.empty((half,), dtype=torch.uint8, device=dev)
        t_copy_pyr = windows(lambda: a.copy_(b), CALLS)
    dst = torch.empty_like(src)
    t_copy = windows(lambda: dst.copy_(src), CALLS)
    n, base_px, kept = len(images), sum(im.shape[0] * im.shape[1] for im in images), sum(f[0].shape[0] for f in feats)
    host_us, pyr = host_s / len(picks) * 1e6, LEVELS > 1
    if pyr:
        print("%s, %d levels: %d image(s), %.2f Mpx on level 0, %.2f Mpx on levels 1 .. (%.2fx), %d keypoints found, %d kept"
              % (name, LEVELS, n, base_px / 1e6, (po - head) / 1e6, (po - head) / base_px, int(counts.sum()), kept))
    else:
        print("%s: %d image(s), %.2f Mpx, %d keypoints found, %d kept" % (name, n, base_px / 1e6, int(counts.sum()), kept))
    lines = [("pyramid call", t_pyr), ("copy moving the pyramid's bytes", t_copy_pyr)] if pyr else []
    lines += [("detect call, %d rows" % len(rows) if pyr else "detect call", t_detect), ("describe call", t_describe),
              ("sort of the keys [%s, 65536]" % (len(rows) if pyr else "n"), t_sort), ("extract_batch, whole", t_all),
              ("device copy of images + planes" if pyr else "device copy of the image bytes", t_copy)]
    for what, (med, mn) in lines:
        print("  %-34s median %9.1f us   min %9.1f us   (%.1f us / image)" % (what, med, mn, med / n))
    print("  %-34s %9.1f us / image on one host core;  extract_batch is %.0fx faster per image" % ("host twin", host_us, host_us / (t_all[0] / n))
          + ("" if pyr else ", detect is %.1fx the copy" % (t_detect[0] / t_copy[0])))
    if pyr:
        print("  the pyramid call reads %.1f MB and writes %.1f MB: %.0f GB/s; per output pixel %.2f ns, detect per pixel of its rows %.2f ns"
              % (head / 1e6, (po - head) / 1e6, po / t_pyr[0] / 1e3, t_pyr[0] * 1e3 / (po - head), t_detect[0] * 1e3 / go))
    else:
        print("  detect reads %.1f MB and writes %.1f MB of gray: %.0f GB/s" % (src.numel() / 1e6, go / 1e6, (src.numel() + go) / t_detect[0] / 1e3))


z = np.load(os.path.join(ROOT, "tests", "golden", "img_foto1.npz"), allow_pickle=False)
A, B = np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["B"])
print("orb_probe: %s, windows %d x %d calls" % (torch.cuda.get_device_name(dev), WINDOWS, CALLS))
case("one image", [A])
case("batch of 64", [np.ascontiguousarray(np.roll(A if i % 2 == 0 else B, 3 * i, axis=0)) for i in range(64)])
