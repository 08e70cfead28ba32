"""The Hamming matcher (kernels.match_hamming_batched, rwh_match_hamming_batched) at the two sizes profiles/match_hamming.txt
records: 512 pairs of 500 x 500 descriptors of 32 bytes in one submission, and one pair of 8192 x 8192.

Per case: the call (its four launches) timed with device events over windows of CALLS back-to-back calls after warm-up, median
and minimum of WINDOWS windows; descriptor pairs per second; the shader clock held meanwhile (kernels.ClockProbe beside a
stretch of the same calls); and the fraction of the VALU bound: 2 * dwords + 2 vector instructions per descriptor pair (one
xor and one popcount-accumulate per dword, one shift-or and one minimum for the key), each a 4-cycle issue per wave of 64 on one
of the chip's CUs x 4 SIMDs.  The results are checked against the host twin first (all of case 2, one pair of case 1).  For
context, not as a pass mark: the same batch through a plain torch formulation (bits unpacked to float16, two batched matrix
products for the distances, argmin / amin reductions for the two rules).

    python tools/match_probe.py [windows] [calls]
"""
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
dev = _lib.require_gpu()
lib = _lib.load()
CUS = torch.cuda.get_device_properties(dev).multi_processor_count


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
        b.synchronize()
        ts.append(a.elapsed_time(b) / calls)
    return float(np.median(ts)), float(np.min(ts))


def clock_under(fn, ms_per_call):
    probe = kernels.ClockProbe(200.0)
    for _ in range(max(1, int(200.0 / max(ms_per_call, 1e-3)))):
        fn()
    torch.cuda.synchronize()
    return probe.mhz()


def host_twin(A, B):
    t = np.empty(len(A), dtype=np.int32)
    d = np.empty(len(A), dtype=np.int32)
    assert lib.rwh_host_match_hamming(A.ctypes.data, len(A), B.ctypes.data, len(B), A.shape[1], t.ctypes.data, d.ctypes.data) == 0
    return t, d


def torch_formulation(bits_a, bits_b):
    """bits_*: [P, N, 8 * nbytes] float16 of 0 / 1.  Distances by two batched products, rule 1 by min over the query axis, rule 2 by
    a scatter-amin of the packed key.  (torch's argmin does not promise the first index on ties: context, not an oracle.)"""
    D = torch.bmm(bits_a, (1 - bits_b).transpose(1, 2)) + torch.bmm(1 - bits_a, bits_b.transpose(1, 2))      # [P, Na, Nb]
    dT, q = D.min(dim=1)                                                                                      # per train row
    P, na, nb = D.shape
    key = (dT.to(torch.int64) << 32) + torch.arange(nb, device=D.device)
    best = torch.full((P, na), torch.iinfo(torch.int64).max, dtype=torch.int64, device=D.device)
    return best.scatter_reduce(1, q, key, reduce="amin")


print("MI355X matcher probe: %d CUs, %d windows of %d calls, descriptors of %d bytes" % (CUS, WINDOWS, CALLS, NBYTES))
rng = np.random.default_rng(0)
for name, P, n, calls in (("512 pairs of 500 x 500", 512, 500, CALLS), ("one pair of 8192 x 8192", 1, 8192, CALLS)):
    A = rng.integers(0, 256, (P * n, NBYTES), dtype=np.uint8)
    B = rng.integers(0, 256, (P * n, NBYTES), dtype=np.uint8)
    B[::3] = A[::3] ^ rng.integers(0, 2, (len(B[::3]), NBYTES), dtype=np.uint8)      # a third of the rows have a near partner
    off = torch.arange(0, P * n + 1, n, dtype=torch.int32, device=dev)
    da, db = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)

    def fn():
        return kernels.match_hamming_batched(da, db, off, off)
    train, dist = (x.cpu().numpy() for x in fn())
    for p in (range(P) if P == 1 else (P - 1,)):
        t, d = host_twin(A[p * n:(p + 1) * n], B[p * n:(p + 1) * n])
        assert np.array_equal(train[p * n:(p + 1) * n], t) and np.array_equal(dist[p * n:(p + 1) * n], d), "GPU result differs from the host twin"
    med, mn = windows(fn, calls)
    mhz = clock_under(fn, med)
    pairs = float(P) * n * n
    instr = 2 * (NBYTES // 4) + 2
    bound_ms = pairs * instr / (CUS * 64.0 * mhz * 1e6) * 1e3        # 64 lane-instructions per CU per clock (4 SIMDs x 16 lanes)
    print("%-24s matches %d  call %.4f ms median / %.4f min  %.3e descriptor pairs/s  sclk %.0f MHz  VALU bound (%d instr/pair) %.4f ms"
          "  -> %.1f %% of the VALU bound" % (name, int((train >= 0).sum()), med, mn, pairs / med * 1e3, mhz, instr, bound_ms, 100.0 * bound_ms / med))
    bits_a = torch.from_numpy(np.unpackbits(A, axis=1)).to(dev).to(torch.float16).reshape(P, n, 8 * NBYTES)
    bits_b = torch.from_numpy(np.unpackbits(B, axis=1)).to(dev).to(torch.float16).reshape(P, n, 8 * NBYTES)
    tmed, tmn = windows(lambda: torch_formulation(bits_a, bits_b), max(1, calls // 10))
    print("%-24s plain torch formulation (bits already unpacked): %.4f ms median / %.4f min" % ("", tmed, tmn))
    del bits_a, bits_b, da, db
    torch.cuda.empty_cache()
