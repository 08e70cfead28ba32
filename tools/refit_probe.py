"""tools/refit_probe.py [reps] [--kernels-only]: what run_batch(refit="device") costs beside refit=True (profiles/refit_device.txt).

P = 512 copies of the matchespoints pair as DeviceProblems, k = 1000, th 5, d 70, 'fwd', device sampling.  3 warm-up calls per
mode, then `reps` calls per mode, alternating, each timed by the host clock around a call that ends synchronised; median and
minimum.  The refit kernel alone (kernels.refit_batched on the winners' masks): HIP events around single launches.
--kernels-only: a few calls of each and nothing else, for `rocprofv3 --kernel-trace --stats -- python3 tools/refit_probe.py 5
--kernels-only` (kernel time belongs to a run of its own)."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ransac_with_homography_amd import kernels, ransac as rmod   # noqa: E402

P, K = 512, 1000
KW = dict(th=5, d=70, k=K, method="fwd", seed=0)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 20
    kernels_only = "--kernels-only" in sys.argv
    z = np.load(os.path.join(ROOT, "tests", "golden", "matchespoints.npz"))
    a, b = z["ptsA"].astype(np.float32), z["ptsB"].astype(np.float32)
    m = len(a)
    dp = rmod.DeviceProblems(torch.from_numpy(np.tile(a, (P, 1))).cuda(), torch.from_numpy(np.tile(b, (P, 1))).cuda(), [m] * P)

    def call(mode):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = rmod.run_batch(dp, refit=mode, **KW)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    modes = (True, "device", False)
    for mode in modes:
        for _ in range(1 if kernels_only else 3):
            call(mode)
    # the refit kernel alone, on the masks of the winners the search found
    info = {}
    res = rmod.run_batch(dp, refit="device", info=info, **KW)
    words = (m + 63) // 64
    masks = np.zeros((P, words), dtype=np.uint64)
    for p, r in enumerate(res):
        bits = np.zeros(64 * words, dtype=np.uint8)
        bits[r[1][0]] = 1
        masks[p] = np.packbits(bits, bitorder="little").view(np.uint64)
    masks = torch.from_numpy(masks.view(np.int64)).cuda()
    offsets = torch.arange(0, (P + 1) * m, m, dtype=torch.int32, device="cuda")
    H, st = kernels.refit_batched(dp.pts_a, dp.pts_b, offsets, masks)
    assert torch.equal(H, info["H_device"]) and torch.equal(st, info["refit_status"])
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        kernels.refit_batched(dp.pts_a, dp.pts_b, offsets, masks)
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    if kernels_only:
        return
    times = {mode: [] for mode in modes}
    for _ in range(reps):
        for mode in modes:
            times[mode].append(call(mode)[0])
    host = call(True)[1]
    same = all(np.array_equal(h[1][0], d[1][0]) and int(h[2]) == int(d[2]) for h, d in zip(host, res))
    inl = [int(r[2]) for r in res]
    print("P = %d x M = %d, k = %d, %d timed calls per mode; inliers per problem %d .. %d; inlier sets of the two modes equal: %s; "
          "refit status OK for %d of %d" % (P, m, K, reps, min(inl), max(inl), same, int((st == 0).sum()), P))
    for mode in modes:
        t = times[mode]
        print("run_batch refit=%-8r  median %8.2f ms   min %8.2f ms" % (mode, statistics.median(t), min(t)))
    print("rwh_refit_batched alone (HIP events around one launch, launch overhead included): median %.4f ms   min %.4f ms"
          % (statistics.median(ev), min(ev)))


if __name__ == "__main__":
    main()
