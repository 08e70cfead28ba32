"""The feature extractor (ransac.extract_batch: rwh_orb_detect_batched -> one sort -> rwh_orb_describe_batched) at the two sizes
profiles/extract_orb.txt records: one 683 x 1024 RGB image (tests/golden/img_foto1.npz A), and a batch of 64 (A and B alternating,
each shifted by a few rows so that no two are the same), threshold 20, n_features 500, 32-byte descriptors.

Per case, by device events over windows of CALLS back-to-back calls after warm-up, median and minimum of WINDOWS windows: the
detect call (two memsets, the tile prefix, the tiled kernel), the describe call (one launch) and the whole extract_batch (upload of
nothing -- the images are device tensors --, both calls, the sort, and the one download of the counts, which synchronises).  Each
is set against two numbers measured in the same run: the host twin (rwh_host_orb_extract, one core, per image) on the same input,
and a plain device copy of the images' bytes (torch's copy kernel: the floor for a kernel that reads every pixel once).  The
results are checked against the host twin first.

    python tools/orb_probe.py [windows] [calls]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ransac_with_homography_amd import _lib, kernels        # noqa: E402
from ransac_with_homography_amd import ransac as rs         # noqa: E402

WINDOWS = int(sys.argv[1]) if len(sys.argv) > 1 else 11
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
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


def host_twin(img, table, rot):
    kps = np.empty((N_FEATURES, 2), np.float32)
    desc = np.empty((N_FEATURES, NBYTES), np.uint8)
    score, bins, count = np.empty(N_FEATURES, np.int32), np.empty(N_FEATURES, np.int32), np.zeros(1, np.int32)
    t = time.perf_counter()
    st = lib.rwh_host_orb_extract(img.ctypes.data, img.shape[0], img.shape[1], 3, THRESHOLD, N_FEATURES, table.ctypes.data, rot.ctypes.data,
                                  NBYTES, kps.ctypes.data, desc.ctypes.data, score.ctypes.data, bins.ctypes.data, count.ctypes.data, None)
    dt = time.perf_counter() - t
    assert st == 0
    return dt, kps[:count[0]].copy(), desc[:count[0]].copy()


def case(name, images):
    table, rot = rs.orb_bin_table(), np.ascontiguousarray(rs.rotate_pattern(rs.default_pattern(NBYTES)))
    dev_images = [torch.from_numpy(im).to(dev) for im in images]
    feats = rs.extract_batch(dev_images, n_features=N_FEATURES, threshold=THRESHOLD, nbytes=NBYTES)
    host_s = 0.0
    for i in sorted(set((0, len(images) - 1))):
        dt, kps, desc = host_twin(images[i], table, rot)
        host_s += dt
        assert np.array_equal(feats[i][0].cpu().numpy(), kps) and np.array_equal(feats[i][1].cpu().numpy(), desc), "device != host twin"
    host_per_image = host_s / len(set((0, len(images) - 1)))
    # the two library calls on their own, on the tensors extract_batch would hand them
    src = torch.cat([t.reshape(-1) for t in dev_images])
    rows, so, go = [], 0, 0
    for im in images:
        rows.append((so, go, im.shape[0], im.shape[1], 3)); so += im.size; go += im.shape[0] * im.shape[1]
    tab = torch.tensor(rows, dtype=torch.int64, device=dev)
    cap = 1 << 16
    gray, keys, counts = kernels.orb_detect_batched(src, tab, go, THRESHOLD, cap)
    assert int(counts.max()) <= cap
    keys = torch.sort(keys, dim=1).values
    bt, pt = torch.from_numpy(table).to(dev), torch.from_numpy(rot).to(dev)
    out_keys = torch.empty_like(keys)
    t_detect = windows(lambda: kernels.orb_detect_batched(src, tab, go, THRESHOLD, cap, out_keys=out_keys), CALLS)
    t_describe = windows(lambda: kernels.orb_describe_batched(gray, go, tab, keys, counts, N_FEATURES, bt, pt), CALLS)
    t_sort = windows(lambda: torch.sort(out_keys, dim=1), CALLS)
    t_all = windows(lambda: rs.extract_batch(dev_images, n_features=N_FEATURES, threshold=THRESHOLD, nbytes=NBYTES), max(CALLS // 4, 2))
    dst = torch.empty_like(src)
    t_copy = windows(lambda: dst.copy_(src), CALLS)
    n, px = len(images), go
    print("%s: %d image(s), %.2f Mpx, %d keypoints found, %d kept" % (name, n, px / 1e6, int(counts.sum()), sum(f[0].shape[0] for f in feats)))
    for what, (med, mn) in (("detect call", t_detect), ("describe call", t_describe), ("sort of the keys [n, 65536]", t_sort),
                            ("extract_batch, whole", t_all), ("device copy of the image bytes", t_copy)):
        print("  %-34s median %9.1f us   min %9.1f us   (%.1f us / image)" % (what, med, mn, med / n))
    print("  %-34s %9.1f us / image on one host core;  extract_batch is %.0fx faster per image, detect is %.1fx the copy"
          % ("host twin", host_per_image * 1e6, host_per_image * 1e6 / (t_all[0] / n), t_detect[0] / t_copy[0]))
    print("  detect reads %.1f MB and writes %.1f MB of gray: %.0f GB/s" % (src.numel() / 1e6, go / 1e6, (src.numel() + go) / t_detect[0] / 1e3))


z = np.load(os.path.join(ROOT, "tests", "golden", "img_foto1.npz"), allow_pickle=False)
A, B = np.ascontiguousarray(z["A"]), np.ascontiguousarray(z["B"])
print("orb_probe: %s, windows %d x %d calls" % (torch.cuda.get_device_name(dev), WINDOWS, CALLS))
case("one image", [A])
case("batch of 64", [np.ascontiguousarray(np.roll(A if i % 2 == 0 else B, 3 * i, axis=0)) for i in range(64)])
