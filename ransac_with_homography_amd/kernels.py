"""Tensor-level wrappers over the C ABI (include/rwh.h): torch-ROCm tensors in,
torch-ROCm tensors out, work enqueued on torch's current HIP stream.

torch is plumbing here (device memory, streams); every computation below happens
inside librwh_hip.so.
"""
import ctypes
import threading
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, _xfer
from ._lib import (RWH_BILINEAR, RWH_F32, RWH_F64, RWH_LOSS, RWH_NEAREST, RWH_U8, RWH_WARP_EXACT, RWH_WARP_ZERO_ORIGIN, check)

_DTYPE = {torch.uint8: RWH_U8, torch.float32: RWH_F32, torch.float64: RWH_F64}
# element type codes of the exact warps (exact=True, sample_points) and rwh_stitch_panorama_ex (a bool plane is read as uint8: numpy
# and torch store it as one 0 / 1 byte)
STITCH_DTYPE = {torch.uint8: RWH_U8, torch.bool: RWH_U8, torch.int8: _lib.RWH_I8, torch.uint16: _lib.RWH_U16, torch.int16: _lib.RWH_I16,
                torch.int32: _lib.RWH_I32, torch.uint32: _lib.RWH_U32, torch.int64: _lib.RWH_I64, torch.uint64: _lib.RWH_U64,
                torch.float16: _lib.RWH_F16, torch.float32: RWH_F32, torch.float64: RWH_F64}
INTERP = {"nn": RWH_NEAREST, "bilinear": RWH_BILINEAR}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev_check(*tensors):
    for t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()):
            raise ValueError("expected contiguous tensors on the GPU")


class Grid:
    """Output sampling grid with numpy.linspace semantics on both axes
    (reference homography.py:166-167 and 197-198)."""

    __slots__ = ("x0", "step_x", "x_last", "out_w", "y0", "step_y", "y_last", "out_h")

    def __init__(self, x_start, x_stop, out_w, y_start, y_stop, out_h):
        self.out_w, self.out_h = int(out_w), int(out_h)
        self.x0, self.x_last = float(x_start), float(x_stop)
        self.y0, self.y_last = float(y_start), float(y_stop)
        # numpy.linspace: step = (stop - start) / (num - 1)
        self.step_x = (self.x_last - self.x0) / (self.out_w - 1) if self.out_w > 1 else 0.0
        self.step_y = (self.y_last - self.y0) / (self.out_h - 1) if self.out_h > 1 else 0.0
        if self.out_w == 1:
            self.x_last = self.x0
        if self.out_h == 1:
            self.y_last = self.y0


def _warp_marshal(src_shape, src_dtype, inv_h, grid, bound_hw, interp, out_dtype, rows, exact):
    """The arguments rwh_warp_backward and rwh_warp_plan share, marshalled once: the plan is the same call without the buffers.
    src_shape (B, H, W, C) -> (source description, B, warp description, dst dtype code, (row_begin, row_end, flags), ih, n_h);
    a dtype without a code in this mode is a KeyError."""
    B, H, W, C = src_shape
    codes = STITCH_DTYPE if exact else _DTYPE
    ih = np.ascontiguousarray(inv_h, dtype=np.float64).reshape(-1)
    n_h = 1 if ih.size == 9 else ih.size // 9          # one inverse for the batch, or [B,3,3]: one per image
    r0, r1 = (0, grid.out_h) if rows is None else rows
    warp = (ih.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n_h,
            grid.x0, grid.step_x, grid.x_last, grid.y0, grid.step_y, grid.y_last,
            grid.out_h, grid.out_w, int(bound_hw[0]), int(bound_hw[1]), INTERP[interp])
    return (H, W, C, codes[src_dtype]), B, warp, codes[out_dtype], (r0, r1, RWH_WARP_EXACT if exact else 0), ih, n_h


def warp_backward(src, inv_h, grid, bound_hw, interp, out_dtype, zero_origin=True, rows=None, out=None, exact=False):
    """Launch K3.  `src`: [B,H,W,C] or [H,W,C] uint8/float32 GPU tensor (with exact=True: any dtype of STITCH_DTYPE, C 1..64).
    Returns a tensor [B,rows,out_w,C] (or without B) of `out_dtype` holding
    output rows `rows=(begin,end)` (default: all).  `inv_h`: inv(H) 3x3 for the whole batch, or [B,3,3] with one
    inverse per image (same output grid for all).  `exact=True` selects the float64 kernel that
    reproduces the reference's arithmetic bit for bit (out_dtype float64 / uint8 for bilinear, src.dtype for nn)."""
    lib = _lib.load()
    _dev_check(src)
    squeeze = src.dim() == 3
    if squeeze:
        src = src.unsqueeze(0)
    B, H, W, C = src.shape
    codes = STITCH_DTYPE if exact else _DTYPE
    if src.dtype not in codes or out_dtype not in codes:
        raise ValueError("unsupported image dtype")
    src_desc, B, warp, dst_code, (r0, r1, flags), ih, n_h = _warp_marshal(src.shape, src.dtype, inv_h, grid, bound_hw, interp, out_dtype,
                                                                          rows, exact)
    if out is None:
        out = torch.empty((B, r1 - r0, grid.out_w, C), dtype=out_dtype, device=src.device)
    else:
        _dev_check(out)
        assert out.dtype == out_dtype and out.numel() == B * (r1 - r0) * grid.out_w * C
    assert ih.size == 9 * n_h and n_h in (1, B), "inv_h: 3x3, or one 3x3 per image of the batch"
    st = lib.rwh_warp_backward(
        _ptr(src), *src_desc, src.stride(0) * src.element_size(), B, *warp,
        _ptr(out), dst_code, (r1 - r0) * grid.out_w * C * out.element_size(),
        r0, r1, flags | (RWH_WARP_ZERO_ORIGIN if zero_origin else 0), _lib.stream_ptr())
    check(st, "rwh_warp_backward")
    return out[0] if squeeze else out


def sample_points(img, xs, ys, bound_hw, interp, zero_origin=True):
    """Launch the interpolator on precomputed coordinates (rwh_sample_points): img [H,W,C] GPU tensor of a STITCH_DTYPE type, xs / ys
    [N] float64 GPU tensors -> [N, C] (image dtype for 'nn', float64 for 'bilinear')."""
    lib = _lib.load()
    _dev_check(img, xs, ys)
    assert xs.dtype == torch.float64 and ys.dtype == torch.float64 and xs.numel() == ys.numel()
    H, W, C = img.shape
    n = xs.numel()
    out_dtype = img.dtype if interp == "nn" else torch.float64
    out = torch.empty((n, C), dtype=out_dtype, device=img.device)
    check(lib.rwh_sample_points(_ptr(img), H, W, C, STITCH_DTYPE[img.dtype], _ptr(xs), _ptr(ys), n, int(bound_hw[0]), int(bound_hw[1]),
                                INTERP[interp], _ptr(out), STITCH_DTYPE[out_dtype], RWH_WARP_ZERO_ORIGIN if zero_origin else 0,
                                _lib.stream_ptr()), "rwh_sample_points")
    return out


def warp_index_check(src_hw, inv_h, grid, bound_hw, interp, device):
    """rwh_warp_index_check: enqueue the test "would the reference raise IndexError on this warp?" and return the device flag
    (int32 [1]; read it after the warp: 1 = an index past the last column, 2 = past the last row, 4 = a NaN coordinate)."""
    lib = _lib.load()
    ih = np.ascontiguousarray(inv_h, dtype=np.float64).reshape(9)
    flag = torch.empty(1, dtype=torch.int32, device=device)
    check(lib.rwh_warp_index_check(int(src_hw[0]), int(src_hw[1]), ih.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                   grid.x0, grid.step_x, grid.x_last, grid.y0, grid.step_y, grid.y_last, grid.out_h, grid.out_w,
                                   int(bound_hw[0]), int(bound_hw[1]), INTERP[interp], _ptr(flag), _lib.stream_ptr()), "rwh_warp_index_check")
    return flag


def raise_like_reference(bits, src_hw):
    """The IndexError numpy raises inside the reference's interpolators (homography.py:117-121, 133-135) for these flag bits."""
    if bits & 4:
        raise IndexError("index -2147483648 is out of bounds for axis 0 with size %d" % src_hw[0])
    if bits & 2:
        raise IndexError("index %d is out of bounds for axis 0 with size %d" % (src_hw[0], src_hw[0]))
    if bits & 1:
        raise IndexError("index %d is out of bounds for axis 1 with size %d" % (src_hw[1], src_hw[1]))


def warp_plan(src_shape, src_dtype, inv_h, grid, bound_hw, interp, out_dtype, rows=None, exact=False):
    """Name of the kernel `warp_backward` launches for this configuration (rwh_warp_plan: the library's own dispatch,
    nothing is launched and no GPU is needed).  src_shape: (B, H, W, C) or (H, W, C)."""
    lib = _lib.load()
    shape4 = (1,) + tuple(src_shape) if len(src_shape) == 3 else tuple(src_shape)
    src_desc, B, warp, dst_code, (r0, r1, flags), _, _ = _warp_marshal(shape4, src_dtype, inv_h, grid, bound_hw, interp, out_dtype, rows, exact)
    buf = ctypes.create_string_buffer(128)
    check(lib.rwh_warp_plan(*src_desc, B, *warp, dst_code, r0, r1, flags, buf, 128), "rwh_warp_plan")
    return buf.value.decode()


def dlt4_batched(pts_a, pts_b, idx):
    """Launch K1.  pts_*: [M,2] float32, idx: [K,4] int32 -> (H [K,9] float32, flags [K] uint8)."""
    lib = _lib.load()
    _dev_check(pts_a, pts_b, idx)
    assert pts_a.dtype == torch.float32 and pts_b.dtype == torch.float32 and idx.dtype == torch.int32
    M, K = pts_a.shape[0], idx.shape[0]
    assert pts_a.shape == (M, 2) and pts_b.shape == (M, 2) and idx.shape == (K, 4)
    H = torch.empty((K, 9), dtype=torch.float32, device=idx.device)
    flags = torch.empty((K,), dtype=torch.uint8, device=idx.device)
    check(lib.rwh_dlt4_batched(_ptr(pts_a), _ptr(pts_b), M, _ptr(idx), K, _ptr(H), _ptr(flags), _lib.stream_ptr()),
          "rwh_dlt4_batched")
    return H, flags


def new_best(device):
    """Zeroed accumulator for rwh_score_count's packed argmax keys (2 x int64)."""
    return torch.zeros(2, dtype=torch.int64, device=device)


_scratch_best = {}


def scratch_best(device):
    """A 2 x int64 accumulator nobody reads (settle-step calls of K2 want counts and masks only): allocated once per device,
    never cleared -- saves the zero-fill launch of `new_best` per call."""
    key = (device.type, device.index)
    if key not in _scratch_best:
        _scratch_best[key] = torch.zeros(2, dtype=torch.int64, device=device)
    return _scratch_best[key]


def score_count(H, pts_a, pts_b, th, loss, need, best, hyp_base=0, want_masks=True, want_err=False, hinv=None):
    """Launch K2.  Returns (counts [K] int32, masks [K,ceil(M/64)] int64 or None, err [K,M] float32 or None);
    `best` (from new_best) is updated in place with atomic max.  hinv: [K, 9] float32 on the device, numpy.linalg.inv of every
    row of H as the reference would compute it ('backward' / 'reproj': rwh_score_count_inv), or None (the kernel's own)."""
    lib = _lib.load()
    _dev_check(H, pts_a, pts_b, best)
    K, M = H.shape[0], pts_a.shape[0]
    words = (M + 63) // 64
    counts = torch.empty((K,), dtype=torch.int32, device=H.device)
    masks = torch.empty((K, words), dtype=torch.int64, device=H.device) if want_masks else None
    err = torch.empty((K, M), dtype=torch.float32, device=H.device) if want_err else None
    if hinv is not None:
        assert hinv.dtype == torch.float32 and hinv.is_contiguous() and tuple(hinv.shape) == (K, 9) and hinv.device == H.device
    check(lib.rwh_score_count_inv(_ptr(H), _ptr(hinv) if hinv is not None else None, _ptr(pts_a), _ptr(pts_b), M, K, float(th),
                                  RWH_LOSS[loss], int(need), int(hyp_base), _ptr(counts), _ptr(masks) if want_masks else None,
                                  _ptr(best), _ptr(err) if want_err else None, _lib.stream_ptr()), "rwh_score_count_inv")
    return counts, masks, err


def score_interval(H, rows, flags, pts_a, pts_b, th, coord_scale, delta0, delta1):
    """rwh_score_interval: count intervals [lo, hi] of the listed rows of H ([K, 9] float32 on the GPU) under 'fwd' -- the pairs that
    are inliers for every / for some H within the perturbation budget (delta0, or delta1 for rows flagged RWH_HYP_ILLCOND in
    `flags`, uint8 [K] on the GPU or None).  rows: host int array.  -> (lo, hi) host int64 arrays."""
    lib = _lib.load()
    _dev_check(H, pts_a, pts_b)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    n = int(rows.shape[0])
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    d_rows = torch.from_numpy(rows).to(H.device)
    out = torch.empty((2, n), dtype=torch.int32, device=H.device)
    check(lib.rwh_score_interval(_ptr(H), _ptr(d_rows), n, _ptr(flags) if flags is not None else None, _ptr(pts_a), _ptr(pts_b),
                                 int(pts_a.shape[0]), float(th), float(coord_scale), float(delta0), float(delta1), _ptr(out[0]), _ptr(out[1]),
                                 _lib.stream_ptr()), "rwh_score_interval")
    o = out.cpu().numpy().astype(np.int64)
    return o[0], o[1]


def host_inverses(H_rows):
    """numpy.linalg.inv of every float32 3 x 3 in `H_rows` ([n, 9] host array) exactly as the reference computes it inside its
    loop (ransac.py:74: float64 LAPACK, cast to float32); a singular matrix gives NaNs instead of numpy's LinAlgError."""
    H3 = np.ascontiguousarray(H_rows, dtype=np.float32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        try:
            return np.linalg.inv(H3).reshape(-1, 9)
        except np.linalg.LinAlgError:
            out = np.full((H3.shape[0], 9), np.nan, dtype=np.float32)
            for i in range(H3.shape[0]):
                try:
                    out[i] = np.linalg.inv(H3[i]).reshape(9)
                except np.linalg.LinAlgError:
                    pass
            return out


class SearchWorkspace:
    """Device buffers of one RANSAC search (K hypotheses over M correspondences), reusable across runs."""

    def __init__(self, k, m, device, want_masks=True):
        self.k, self.m = k, m
        self.H = torch.empty((k, 9), dtype=torch.float32, device=device)
        # counts (int32) and flags (uint8) share one buffer so that the host reads both back with ONE copy (`counts_flags`)
        self.cf = torch.empty((5 * k + 16,), dtype=torch.uint8, device=device)
        self.counts = self.cf[:4 * k].view(torch.int32)
        self.flags = self.cf[4 * k:5 * k]
        self.masks = torch.empty((k, (m + 63) // 64), dtype=torch.int64, device=device) if want_masks else None
        self.best = torch.zeros(2, dtype=torch.int64, device=device)

    def counts_flags(self):
        """-> (counts int32 [k], flags uint8 [k]) as host arrays, one device-to-host copy."""
        raw = self.cf.cpu().numpy()
        return raw[:4 * self.k].view(np.int32), raw[4 * self.k:5 * self.k]


def ransac_search(pts_a, pts_b, idx, th, loss, need, ws, hyp_base=0, reset_best=True):
    """K1 + K2 in one library call (rwh_ransac_search); results land in the workspace `ws`."""
    lib = _lib.load()
    _dev_check(pts_a, pts_b, idx)
    K, M = idx.shape[0], pts_a.shape[0]
    assert K <= ws.k and M == ws.m and idx.dtype == torch.int32
    check(lib.rwh_ransac_search(_ptr(pts_a), _ptr(pts_b), M, _ptr(idx), K, float(th), RWH_LOSS[loss], int(need), int(hyp_base),
                                _ptr(ws.H), _ptr(ws.flags), _ptr(ws.counts), _ptr(ws.masks) if ws.masks is not None else None,
                                _ptr(ws.best), 1 if reset_best else 0, _lib.stream_ptr()), "rwh_ransac_search")
    return ws


_pinned_run_ws = threading.local()      # per thread: two threads inside rwh_ransac_run (ctypes drops the GIL) must not share a host workspace


class RunWorkspace:
    """Buffers of one `rwh_ransac_run` call: a device workspace (fresh per run: `RANSAC.last_run` keeps views into it) and a
    page-locked host workspace (cached per (m, k): page-locking is the expensive part), laid out by rwh_ransac_run_layout."""
    D_H, D_COUNTS, D_FLAGS, D_MASKS, D_END, H_COUNTS, H_FLAGS, H_CNTSET, H_END = 3, 4, 5, 6, 11, 13, 14, 15, 19

    def __init__(self, m, k, device):
        lib = _lib.load()
        self.m, self.k, self.words = int(m), int(k), (int(m) + 63) // 64
        off = (ctypes.c_longlong * 27)()
        n = lib.rwh_ransac_run_layout(self.m, self.k, off, 27)
        if n != 27:
            check(n if n < 0 else _lib_invalid(), "rwh_ransac_run_layout")
        self.off = list(off)
        self.dev = torch.empty(self.off[self.D_END], dtype=torch.uint8, device=device)
        key = (self.m, self.k)
        cache = _pinned_run_ws.__dict__.setdefault("ws", {})
        if key not in cache:
            if len(cache) > 8:
                cache.clear()
            cache[key] = torch.empty(self.off[self.H_END], dtype=torch.uint8, pin_memory=True)
        self.host = cache[key]

    def _dview(self, which, nbytes, dtype):
        return self.dev[self.off[which]:self.off[which] + nbytes].view(dtype)

    @property
    def H(self):
        return self._dview(self.D_H, 36 * self.k, torch.float32).reshape(self.k, 9)

    @property
    def counts(self):
        return self._dview(self.D_COUNTS, 4 * self.k, torch.int32)

    @property
    def flags(self):
        return self._dview(self.D_FLAGS, self.k, torch.uint8)

    @property
    def masks(self):
        return self._dview(self.D_MASKS, 8 * self.words * self.k, torch.int64).reshape(self.k, self.words)

    def host_counts(self, settled=False):
        """K2's raw counts (or, settled=True, the counts after the settle step) as a host int32 array (a copy)."""
        o = self.off[self.H_CNTSET if settled else self.H_COUNTS]
        return self.host[o:o + 4 * self.k].numpy().view(np.int32).copy()

    def host_flags(self):
        o = self.off[self.H_FLAGS]
        return self.host[o:o + self.k].numpy().copy()


def _lib_invalid():
    return -1


def ransac_run(pts_a, pts_b, idx, th, loss, need, margin_cap, ws, dgesdd, threads, dgesv=None, hyp_base=0, want_keys=False):
    """rwh_ransac_run: upload + search + settle + accept rules in ONE native call.  pts_a / pts_b: float32 [M, 2] HOST arrays,
    idx: int32 [K, 4] host array (hyp_base: the global index of its first row when it is a slice of a sharded search).
    -> (winner | None, early, count, host_solved, rounds, flagged, mask_words uint64 [words]); want_keys: + (the slice's two
    packed keys as int64 [2], hypotheses given a count interval)."""
    lib = _lib.load()
    assert pts_a.dtype == np.float32 and pts_b.dtype == np.float32 and idx.dtype == np.int32
    assert pts_a.flags.c_contiguous and pts_b.flags.c_contiguous and idx.flags.c_contiguous
    assert pts_a.shape == (ws.m, 2) and pts_b.shape == (ws.m, 2) and idx.shape == (ws.k, 4)
    out = np.zeros(8, dtype=np.int32)
    keys = np.zeros(2, dtype=np.uint64)
    mask = np.zeros(ws.words, dtype=np.uint64)
    check(lib.rwh_ransac_run(pts_a.ctypes.data, pts_b.ctypes.data, ws.m, idx.ctypes.data, ws.k, float(th), RWH_LOSS[loss], int(need),
                             int(margin_cap), ctypes.c_void_p(dgesdd), ctypes.c_void_p(dgesv or 0), int(threads), _ptr(ws.dev),
                             ctypes.c_void_p(ws.host.data_ptr()), int(hyp_base),
                             out.ctypes.data, keys.ctypes.data, mask.ctypes.data, _lib.stream_ptr()), "rwh_ransac_run")
    winner = int(out[0])
    res = ((winner if winner >= 0 else None), bool(out[1]), int(out[2]), int(out[3]), int(out[4]), int(out[5]), mask)
    return res + (keys.view(np.int64), int(out[6])) if want_keys else res


class BatchWorkspace:
    """Device buffers of one batched search: P problems x K hypotheses (rwh_ransac_batched)."""

    def __init__(self, n_problems, k, m_max, device, want_masks=True):
        self.p, self.k, self.m_max = n_problems, k, m_max
        self.words = (m_max + 63) // 64
        n = n_problems * k
        self.idx = torch.empty((n_problems, k, 4), dtype=torch.int32, device=device)
        self.H = torch.empty((n_problems, k, 9), dtype=torch.float32, device=device)
        self.flags = torch.empty((n_problems, k), dtype=torch.uint8, device=device)
        self.counts = torch.empty((n_problems, k), dtype=torch.int32, device=device)
        self.masks = torch.empty((n_problems, k, self.words), dtype=torch.int64, device=device) if want_masks else None
        self.best = torch.zeros((n_problems, 2), dtype=torch.int64, device=device)


def ransac_batched(pts_a, pts_b, offsets, needs, th, loss, ws, seed=None, idx=None, problem_base=0, early_stop=False):
    """P independent RANSAC searches in one library call (rwh_ransac_batched, include/rwh.h).

    pts_a/pts_b: [total,2] float32 (the problems' correspondences concatenated), offsets: [P+1] int32,
    needs: [P] int32 -- all on the GPU.  Either `idx` ([P,K,4] int32, problem-local indices, the caller's
    sampler: parity with `ransac_search`) or `seed` (device Philox sampling, non-parity; `problem_base` = global
    index of the first problem when a longer list is sharded over calls) must be given.
    Results land in `ws` (ws.idx holds the samples actually used)."""
    lib = _lib.load()
    _dev_check(pts_a, pts_b, offsets, needs)
    assert (seed is None) != (idx is None), "give exactly one of seed= (device sampling) and idx= (caller's samples)"
    P = offsets.shape[0] - 1
    assert P == ws.p and needs.shape[0] == P and offsets.dtype == torch.int32 and needs.dtype == torch.int32
    flags = _lib.RWH_BATCH_EARLY_STOP if early_stop else 0     # hypotheses after a problem's early exit are skipped (count -1)
    if idx is None:
        flags |= _lib.RWH_BATCH_DEVICE_SAMPLING
    else:
        assert tuple(idx.shape) == (P, ws.k, 4) and idx.dtype == torch.int32
        ws.idx.copy_(idx)
    check(lib.rwh_ransac_batched(_ptr(pts_a), _ptr(pts_b), _ptr(offsets), P, ws.m_max, ws.k, _ptr(ws.idx),
                                 int(seed or 0) & 0xFFFFFFFFFFFFFFFF, int(problem_base), float(th), RWH_LOSS[loss], _ptr(needs), _ptr(ws.H),
                                 _ptr(ws.flags), _ptr(ws.counts), _ptr(ws.masks) if ws.masks is not None else None,
                                 _ptr(ws.best), flags, _lib.stream_ptr()), "rwh_ransac_batched")
    return ws


def refit_batched(pts_a, pts_b, offsets, masks):
    """The N-point refit of P problems in one launch (rwh_refit_batched, include/rwh.h): float64 normal equations over each
    problem's inliers -- the reference's least-squares problem, NOT its float32 bits.

    pts_a/pts_b: [total,2] float32, offsets: [P+1] int32, masks: [P,words] int64 (bit i of word i/64 of row p = correspondence
    offsets[p] + i; words >= ceil(M_p/64) for every problem) -- all on the GPU.  Returns (H [P,3,3] float64, status [P] int32:
    RWH_REFIT_OK / _FEW / _SINGULAR, H all NaN unless OK), both on the GPU, enqueued on torch's current stream."""
    lib = _lib.load()
    _dev_check(pts_a, pts_b, offsets, masks)
    P = offsets.shape[0] - 1
    assert pts_a.dtype == torch.float32 and pts_b.dtype == torch.float32 and offsets.dtype == torch.int32
    assert masks.dtype == torch.int64 and masks.dim() == 2 and masks.shape[0] == P and tuple(pts_a.shape) == tuple(pts_b.shape)
    H = torch.empty((P, 3, 3), dtype=torch.float64, device=pts_a.device)
    status = torch.empty((P,), dtype=torch.int32, device=pts_a.device)
    check(lib.rwh_refit_batched(_ptr(pts_a), _ptr(pts_b), _ptr(offsets), P, _ptr(masks), masks.shape[1], _ptr(H), _ptr(status),
                                _lib.stream_ptr()), "rwh_refit_batched")
    return H, status


BUNDLE_BLOCK, BUNDLE_MAX_EDGES = _lib.RWH_BUNDLE_BLOCK, _lib.RWH_BUNDLE_MAX_EDGES
CAMERA_BLOCK, CAMERA_RECORD = _lib.RWH_CAMERA_BLOCK, _lib.RWH_CAMERA_RECORD
CAMERA_FOCALS = {"shared": _lib.RWH_CAMERA_FOCAL_SHARED, "per-image": _lib.RWH_CAMERA_FOCAL_PER_IMAGE}


# ---- the registration rules (include/rwh.h): one marshalling per call shape, a rule gives its entry point, block width and records ----
def _bundle_transfers(transfers, n_edges):
    t = np.ascontiguousarray(transfers, dtype=np.float64).reshape(-1, 9)
    if t.shape[0] != n_edges or not 1 <= n_edges <= BUNDLE_MAX_EDGES:
        raise ValueError("bundle_blocks: %d transfers for %d edges; 1 .. %d edges, a 3 x 3 transfer each" % (t.shape[0], n_edges, BUNDLE_MAX_EDGES))
    return t


def _camera_records(records, n_edges):
    r = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, CAMERA_RECORD)
    if r.shape[0] != n_edges or not 1 <= n_edges <= BUNDLE_MAX_EDGES:
        raise ValueError("camera_blocks: %d records for %d edges; 1 .. %d edges, a record of %d doubles each"
                         % (r.shape[0], n_edges, BUNDLE_MAX_EDGES, CAMERA_RECORD))
    return r


def _edge_blocks(entry, width, checked, pts_a, pts_b, offsets, masks, records, out):
    """The blocks of every edge on the device: library entry point `entry`, blocks of `width` values, `checked(records, E)` the
    rule's per-edge records as a float64 [E, record] host array -> the packed [E, width + 2] tensor."""
    lib = _lib.load()
    _dev_check(pts_a, pts_b, offsets, masks)
    E = offsets.shape[0] - 1
    assert pts_a.dtype == torch.float32 and pts_b.dtype == torch.float32 and offsets.dtype == torch.int32
    assert masks.dtype == torch.int64 and masks.dim() == 2 and masks.shape[0] == E and tuple(pts_a.shape) == tuple(pts_b.shape)
    r_dev = torch.from_numpy(checked(records, E)).to(pts_a.device)
    if pts_a.shape[0] == 0:
        # edges without a single correspondence: an empty tensor has no address and the library refuses a null pointer, where the
        # host twin gives zero blocks.  One row that no edge's offsets reach stands in; nothing of it is read.
        pts_a = pts_b = torch.zeros((1, 2), dtype=torch.float32, device=pts_a.device)
    if out is None:
        blocks = torch.empty((E, width), dtype=torch.float64, device=pts_a.device)
        count, status = torch.empty((2, E), dtype=torch.int32, device=pts_a.device)
    else:
        blocks, count, status = out
        _dev_check(blocks, count, status)
        assert blocks.dtype == torch.float64 and tuple(blocks.shape) == (E, width)
        assert count.dtype == torch.int32 and status.dtype == torch.int32 and tuple(count.shape) == (E,) and tuple(status.shape) == (E,)
    check(getattr(lib, entry)(_ptr(pts_a), _ptr(pts_b), _ptr(offsets), E, _ptr(masks), masks.shape[1], _ptr(r_dev), _ptr(blocks),
                              _ptr(count), _ptr(status), _lib.stream_ptr()), entry)
    return torch.cat([blocks, count.to(torch.float64)[:, None], status.to(torch.float64)[:, None]], dim=1)


def _split(packed, width):
    """(blocks float64 [E, width], count int32 [E], status int32 [E]) of a downloaded packed result (numpy)."""
    packed = np.asarray(packed)
    return np.ascontiguousarray(packed[:, :width]), packed[:, width].astype(np.int32), packed[:, width + 1].astype(np.int32)


def _host_edge_blocks(entry, width, checked, pts_a, pts_b, offsets, masks, records):
    """The host twin `entry` ("rwh_host_<rule>_blocks") of `_edge_blocks`: numpy in, (blocks, count, status) numpy out."""
    lib = _lib.load()
    pts_a, pts_b = np.ascontiguousarray(pts_a, dtype=np.float32).reshape(-1, 2), np.ascontiguousarray(pts_b, dtype=np.float32).reshape(-1, 2)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    E = offsets.shape[0] - 1
    masks = np.ascontiguousarray(masks).view(np.uint64).reshape(E, -1)
    r = checked(records, E)
    if pts_a.shape != pts_b.shape or E < 1 or int(offsets[0]) != 0 or int(offsets[-1]) != pts_a.shape[0] or (np.diff(offsets) < 0).any():
        raise ValueError("%s: offsets must run from 0 to the %d correspondences without decreasing" % (entry[len("rwh_"):], pts_a.shape[0]))
    blocks = np.empty((E, width), dtype=np.float64)
    count, status = np.empty(E, dtype=np.int32), np.empty(E, dtype=np.int32)
    check(getattr(lib, entry)(pts_a.ctypes.data, pts_b.ctypes.data, offsets.ctypes.data, E, masks.ctypes.data, masks.shape[1],
                              r.ctypes.data, blocks.ctypes.data, count.ctypes.data, status.ctypes.data), entry)
    return blocks, count, status


def bundle_blocks(pts_a, pts_b, offsets, masks, transfers, out=None):
    """The normal-equation blocks of every edge of a pair graph in one launch (rwh_bundle_blocks; the bundle rule of include/rwh.h).

    pts_a/pts_b: [total, 2] float32, offsets: [E+1] int32, masks: [E, words] int64 (the layout of `refit_batched`) -- on the GPU;
    transfers: [E, 3, 3] float64 on the HOST (one upload of E x 9 doubles).  Returns one [E, 155] float64 tensor on the GPU: the
    153 values of each block, then the edge's count and status as float64 -- so that ONE download brings everything to the host
    (`bundle_split` takes it apart).  out: optionally the three tensors the library writes -- blocks [E, 153] float64, count [E]
    and status [E] int32, contiguous, on the GPU -- instead of fresh ones.  Edges without any correspondence ([0, 2] points) give
    zero blocks, as the host twin's.  Enqueued on torch's current stream."""
    return _edge_blocks("rwh_bundle_blocks", BUNDLE_BLOCK, _bundle_transfers, pts_a, pts_b, offsets, masks, transfers, out)


def bundle_split(packed):
    """(blocks float64 [E, 153], count int32 [E], status int32 [E]) of a downloaded `bundle_blocks` result (numpy)."""
    return _split(packed, BUNDLE_BLOCK)


def host_bundle_blocks(pts_a, pts_b, offsets, masks, transfers):
    """The host twin of `bundle_blocks` (rwh_host_bundle_blocks): numpy arrays in, (blocks, count, status) numpy out, the same
    operations in the same order.  Uses no device and works without a GPU."""
    return _host_edge_blocks("rwh_host_bundle_blocks", BUNDLE_BLOCK, _bundle_transfers, pts_a, pts_b, offsets, masks, transfers)


def host_bundle_step(n, anchor, edges, blocks, lam):
    """One damped step from the edge blocks (rwh_host_bundle_step, host only): -> (delta float64 [n, 8], status)."""
    lib = _lib.load()
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    blocks = np.ascontiguousarray(blocks, dtype=np.float64).reshape(len(edges), BUNDLE_BLOCK)
    delta, status = np.empty((int(n), 8), dtype=np.float64), np.zeros(1, dtype=np.int32)
    check(lib.rwh_host_bundle_step(int(n), int(anchor), edges.ctypes.data, len(edges), blocks.ctypes.data, float(lam), delta.ctypes.data,
                                   status.ctypes.data), "rwh_host_bundle_step")
    return delta, int(status[0])


def camera_blocks(pts_a, pts_b, offsets, masks, records, out=None):
    """The normal-equation blocks of every edge over rotations and focal lengths in one launch (rwh_camera_blocks; the camera rule of
    include/rwh.h).

    pts_a/pts_b, offsets, masks: as `bundle_blocks`', on the GPU; records: [E, 15] float64 on the HOST -- R_d^T R_s row-major, then
    f_s, cx_s, cy_s, f_d, cx_d, cy_d (one upload of E x 15 doubles).  Returns one [E, 47] float64 tensor on the GPU: the 45 values of
    each block, then the edge's count and status as float64, for ONE download (`camera_split` takes it apart).  out: optionally the
    three tensors the library writes -- blocks [E, 45] float64, count [E] and status [E] int32, contiguous, on the GPU.  Edges
    without any correspondence give zero blocks, as the host twin's.  Enqueued on torch's current stream."""
    return _edge_blocks("rwh_camera_blocks", CAMERA_BLOCK, _camera_records, pts_a, pts_b, offsets, masks, records, out)


def camera_split(packed):
    """(blocks float64 [E, 45], count int32 [E], status int32 [E]) of a downloaded `camera_blocks` result (numpy)."""
    return _split(packed, CAMERA_BLOCK)


def host_camera_blocks(pts_a, pts_b, offsets, masks, records):
    """The host twin of `camera_blocks` (rwh_host_camera_blocks): numpy arrays in, (blocks, count, status) numpy out, the same
    operations in the same order.  Uses no device and works without a GPU."""
    return _host_edge_blocks("rwh_host_camera_blocks", CAMERA_BLOCK, _camera_records, pts_a, pts_b, offsets, masks, records)


def host_camera_step(n, anchor, edges, blocks, lam, focals="shared"):
    """One damped step from the edge blocks (rwh_host_camera_step, host only): -> (delta float64 [n, 4], status); a row of delta is
    (omega_0, omega_1, omega_2, phi).  focals: "shared" (one focal unknown for all images) or "per-image"."""
    lib = _lib.load()
    if not (isinstance(focals, str) and focals in CAMERA_FOCALS):
        raise ValueError("host_camera_step: focals=%r; 'shared' or 'per-image'" % (focals,))
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    blocks = np.ascontiguousarray(blocks, dtype=np.float64).reshape(len(edges), CAMERA_BLOCK)
    delta, status = np.empty((int(n), 4), dtype=np.float64), np.zeros(1, dtype=np.int32)
    check(lib.rwh_host_camera_step(int(n), int(anchor), CAMERA_FOCALS[focals], edges.ctypes.data, len(edges), blocks.ctypes.data, float(lam),
                                   delta.ctypes.data, status.ctypes.data), "rwh_host_camera_step")
    return delta, int(status[0])


# the matcher's block shape, for callers and tests that size problems across it: train rows per block, query rows staged in LDS at
# a time, query rows per block (include/rwh.h)
MATCH_TILE_TRAIN, MATCH_CHUNK_QUERY, MATCH_SEG_QUERY = _lib.RWH_MATCH_TILE_TRAIN, _lib.RWH_MATCH_CHUNK_QUERY, _lib.RWH_MATCH_SEG_QUERY
MATCH_MAX_BYTES = _lib.RWH_MATCH_MAX_BYTES
MATCH_GRID_MAX = _lib.RWH_MATCH_GRID_MAX    # the most blocks of the main kernel; a longer block list is walked with that stride


def match_hamming_batched(desc_a, desc_b, offsets_a, offsets_b):
    """Brute-force Hamming matches with cross-check of P descriptor pairs in one library call (rwh_match_hamming_batched; the
    rule, and the caveat that parity with OpenCV's BFMatcher is not verified, in include/rwh.h).

    desc_a [total_a, nbytes] / desc_b [total_b, nbytes] uint8 (the problems' descriptors concatenated; query / train side),
    offsets_a / offsets_b [P+1] int32 -- all on the GPU.  Returns (train_idx, distance), [total_a] int32 each on the GPU: per query
    row its match's train row inside its problem and the distance, -1 / -1 for no match.  nbytes outside 1 .. MATCH_MAX_BYTES:
    NotImplementedError."""
    lib = _lib.load()
    _dev_check(desc_a, desc_b, offsets_a, offsets_b)
    if not (desc_a.dtype == torch.uint8 and desc_b.dtype == torch.uint8 and desc_a.dim() == 2 and desc_b.dim() == 2 and
            desc_a.shape[1] == desc_b.shape[1]):
        raise ValueError("descriptors: two uint8 [rows, nbytes] tensors of one row length, got %s %s and %s %s"
                         % (desc_a.dtype, tuple(desc_a.shape), desc_b.dtype, tuple(desc_b.shape)))
    if not (offsets_a.dtype == torch.int32 and offsets_b.dtype == torch.int32 and offsets_a.dim() == 1 and
            offsets_a.shape == offsets_b.shape and offsets_a.shape[0] >= 2):
        raise ValueError("offsets: two int32 [P + 1] tensors, P >= 1")
    P, (total_a, nbytes), total_b = offsets_a.shape[0] - 1, desc_a.shape, desc_b.shape[0]
    train_idx = torch.empty((total_a,), dtype=torch.int32, device=desc_a.device)
    distance = torch.empty((total_a,), dtype=torch.int32, device=desc_a.device)
    if nbytes == 0:         # rows without bytes have no address to hand over: the library's answer for this length, given here
        raise NotImplementedError("match: descriptors of 0 bytes; the matcher takes 1 .. %d" % MATCH_MAX_BYTES)
    ws_bytes = int(lib.rwh_match_workspace_bytes(P, total_a, total_b))
    if ws_bytes < 0:
        check(ws_bytes, "rwh_match_workspace_bytes")
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=desc_a.device)
    status = lib.rwh_match_hamming_batched(_ptr(desc_a), _ptr(desc_b), nbytes, _ptr(offsets_a), _ptr(offsets_b), P, total_a, total_b,
                                           _ptr(train_idx), _ptr(distance), _ptr(ws), ws_bytes, _lib.stream_ptr())
    if status == _lib.RWH_E_UNSUPPORTED:
        raise NotImplementedError("match: descriptors of %d bytes; the matcher takes 1 .. %d" % (nbytes, MATCH_MAX_BYTES))
    check(status, "rwh_match_hamming_batched")
    return train_idx, distance


# the ratio matcher's block shape (include/rwh.h, the ratio rule): query rows per block, train rows staged in LDS at a time, train
# rows per block
MATCH2_TILE_QUERY, MATCH2_CHUNK_TRAIN, MATCH2_SEG_TRAIN = _lib.RWH_MATCH2_TILE_QUERY, _lib.RWH_MATCH2_CHUNK_TRAIN, _lib.RWH_MATCH2_SEG_TRAIN
MATCH2_RATIO_MAX = _lib.RWH_MATCH2_RATIO_MAX
MATCH2_GRID_MAX = _lib.RWH_MATCH2_GRID_MAX  # the most blocks of the main kernel; a longer block list is walked with that stride


def match_ratio_rows(image_offsets, pairs, total_rows):
    """The rows of every pair of a graph, on the host, as rwh_match_ratio_graph counts them: image_offsets int [N + 1], pairs int
    [P, 2] of (s, d) -> (na, nb), int64 [P] each.  An image outside 0 .. N - 1, or one whose range is not inside [0, total_rows], has
    no rows."""
    off = np.asarray(image_offsets, dtype=np.int64)
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n = off.shape[0] - 1
    o0, o1 = off[:-1], off[1:]
    rows = np.where((o0 >= 0) & (o1 >= o0) & (o1 <= total_rows), o1 - o0, 0)
    inside = (pr >= 0) & (pr < n)
    both = np.where(inside, rows[np.clip(pr, 0, n - 1)], 0)
    return both[:, 0], both[:, 1]


def match_ratio_graph(desc, image_offsets, pairs, ratio=(7, 10)):
    """Hamming matches under the 2-nearest ratio test for the P pairs of a pair graph in one library call (rwh_match_ratio_graph;
    the ratio rule and its provenance in include/rwh.h).  Every image's descriptors are read where they lie: nothing is copied per pair.

    desc [total_rows, nbytes] uint8 on the GPU (the images' descriptors concatenated); image_offsets [N + 1] int32, image k owns rows
    image_offsets[k] .. image_offsets[k + 1] - 1; pairs [P, 2] int32 of (s, d): query image, train image.  The two tables are numpy
    arrays or tensors; the output's length is counted from them on the host, so tables that live on the GPU are downloaded for
    that.  ratio = (num, den), integers with 0 < num <= den <= MATCH2_RATIO_MAX.  Returns (train_idx, distance, second), int32
    [sum of the pairs' query rows] each on the GPU: per (pair, query row), in pair order, its match's row inside image d, the
    distance and the second-nearest distance, -1 / -1 / -1 for no match.  nbytes outside 1 .. MATCH_MAX_BYTES: NotImplementedError."""
    lib = _lib.load()
    _dev_check(desc)
    if not (desc.dtype == torch.uint8 and desc.dim() == 2):
        raise ValueError("descriptors: a uint8 [rows, nbytes] tensor, got %s %s" % (desc.dtype, tuple(desc.shape)))
    tables = []
    for t, what in ((image_offsets, "image_offsets"), (pairs, "pairs")):
        t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
        if t.dtype != torch.int32:
            raise ValueError("%s: an int32 table, got %s" % (what, t.dtype))
        tables.append(t)
    off, pr = tables
    if not (off.dim() == 1 and off.shape[0] >= 2 and pr.dim() == 2 and pr.shape[1] == 2 and pr.shape[0] >= 1):
        raise ValueError("image_offsets: int32 [N + 1], N >= 1; pairs: int32 [P, 2], P >= 1; got %s and %s" % (tuple(off.shape), tuple(pr.shape)))
    try:
        num, den = (int(v) for v in ratio)
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in ratio) and 0 < num <= den <= MATCH2_RATIO_MAX
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("ratio=%r; two integers (num, den) with 0 < num <= den <= %d" % (ratio, MATCH2_RATIO_MAX))
    total_rows, nbytes = desc.shape
    if nbytes == 0:         # rows without bytes have no address to hand over: the library's answer for this length, given here
        raise NotImplementedError("match: descriptors of 0 bytes; the matcher takes 1 .. %d" % MATCH_MAX_BYTES)
    na, nb = match_ratio_rows(off.cpu().numpy(), pr.cpu().numpy(), total_rows)
    total_query, total_train, max_train = int(na.sum()), int(nb.sum()), int(nb.max())
    if total_query >= 2 ** 31 or total_train >= 2 ** 31:
        raise ValueError("match: too many rows for one submission")
    dev = desc.device
    off, pr = off.to(dev).contiguous(), pr.to(dev).contiguous()
    n_images, n_pairs = off.shape[0] - 1, pr.shape[0]
    out = [torch.empty((total_query,), dtype=torch.int32, device=dev) for _ in range(3)]
    ws_bytes = int(lib.rwh_match_ratio_workspace_bytes(n_pairs, total_query, total_train, max_train))
    if ws_bytes < 0:
        check(ws_bytes, "rwh_match_ratio_workspace_bytes")
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
    status = lib.rwh_match_ratio_graph(_ptr(desc), nbytes, _ptr(off), n_images, total_rows, _ptr(pr), n_pairs, total_query, total_train,
                                       num, den, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(ws), ws_bytes, _lib.stream_ptr())
    if status == _lib.RWH_E_UNSUPPORTED:
        raise NotImplementedError("match: descriptors of %d bytes; the matcher takes 1 .. %d" % (nbytes, MATCH_MAX_BYTES))
    check(status, "rwh_match_ratio_graph")
    return tuple(out)


# the extractor's constants (include/rwh.h): border of a keypoint's centre, orientation bins, radius of the test points, the
# detector's tile -- for callers and tests that plant corners across tile seams
ORB_BORDER, ORB_BINS, ORB_TEST_RADIUS = _lib.RWH_ORB_BORDER, _lib.RWH_ORB_BINS, _lib.RWH_ORB_TEST_RADIUS
ORB_TILE_W, ORB_TILE_H = _lib.RWH_ORB_TILE_W, _lib.RWH_ORB_TILE_H


def orb_detect_batched(images, table, gray_bytes, threshold, capacity, out_keys=None, out_gray=None):
    """FAST-9 corners with non-maximum suppression of a batch of images in one library call (rwh_orb_detect_batched; the rule,
    and the caveat that this is not OpenCV's ORB, in include/rwh.h).

    images: uint8 [bytes], the images' pixels concatenated; table: int64 [n, 5], row i = (byte offset of image i, byte offset of
    its gray plane, h, w, c) -- both on the GPU.  Returns (gray uint8 [gray_bytes], keys int64 [n, capacity], counts int32 [n]) on
    the GPU: the gray planes, per image its keypoints as keys (255 - S) << 32 | y << 16 | x in no particular order (unused entries
    0x7F7F7F7F7F7F7F7F, which sort last), and the number of keypoints found.  counts[i] > capacity: only
    `capacity` of them were stored (overflow; call again with more room).  out_keys: an int64 [n, capacity] tensor to fill instead
    of a new one; out_gray: likewise a uint8 [>= gray_bytes] tensor for the gray planes (bytes outside every plane are not written)."""
    lib = _lib.load()
    _dev_check(images, table)
    if not (images.dtype == torch.uint8 and images.dim() == 1 and table.dtype == torch.int64 and table.dim() == 2 and
            table.shape[1] == 5 and table.shape[0] >= 1):
        raise ValueError("orb_detect_batched: images uint8 [bytes] and table int64 [n, 5], got %s %s and %s %s"
                         % (images.dtype, tuple(images.shape), table.dtype, tuple(table.shape)))
    n = table.shape[0]
    gray = out_gray if out_gray is not None else torch.empty((max(int(gray_bytes), 1),), dtype=torch.uint8, device=images.device)
    _dev_check(gray)
    if gray.dtype != torch.uint8 or gray.dim() != 1 or gray.shape[0] < max(int(gray_bytes), 1):
        raise ValueError("orb_detect_batched: out_gray must be uint8 [>= %d]" % max(int(gray_bytes), 1))
    keys = out_keys if out_keys is not None else torch.empty((n, int(capacity)), dtype=torch.int64, device=images.device)
    _dev_check(keys)
    if keys.dtype != torch.int64 or tuple(keys.shape) != (n, int(capacity)):
        raise ValueError("orb_detect_batched: out_keys must be int64 [%d, %d]" % (n, capacity))
    counts = torch.empty((n,), dtype=torch.int32, device=images.device)
    ws_bytes = int(lib.rwh_orb_workspace_bytes(n))
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=images.device)
    check(lib.rwh_orb_detect_batched(_ptr(images), images.shape[0], _ptr(table), n, int(threshold), _ptr(gray), int(gray_bytes), _ptr(keys),
                                     int(capacity), _ptr(counts), _ptr(ws), ws_bytes, _lib.stream_ptr()), "rwh_orb_detect_batched")
    return gray, keys, counts


def orb_pyramid_batched(images, planes_offset, table, scales):
    """The level planes of a scale pyramid for a batch of images in one library call (rwh_orb_pyramid_batched; rule 6 of
    include/rwh.h): every level an exact area average of the image's gray plane, all levels of all images in one launch.

    images: uint8 [bytes] on the GPU, the images' pixels concatenated in [0, planes_offset) and room for the planes behind them;
    table: int64 [n * n_levels, 5] on the GPU, row i * n_levels + l = level l of image i in the layout of orb_detect_batched --
    level 0 the image itself, level l >= 1 (byte offset of its plane, gray offset, h_l, w_l, 1); scales: n_levels ints in Q8 on the
    HOST (256 first, strictly increasing, <= 1024).  The planes are written into `images` in place (nothing else of it is), so
    that one orb_detect_batched call takes every row; a row that does not fit its image or the tail is not written.  Returns
    `images`."""
    lib = _lib.load()
    _dev_check(images, table)
    sc = np.ascontiguousarray(np.asarray(scales, dtype=np.int32).reshape(-1))
    n_levels = int(sc.shape[0])
    if not (images.dtype == torch.uint8 and images.dim() == 1 and images.is_contiguous() and table.dtype == torch.int64 and table.dim() == 2 and
            table.shape[1] == 5 and table.is_contiguous() and n_levels >= 1 and table.shape[0] >= n_levels and table.shape[0] % n_levels == 0):
        raise ValueError("orb_pyramid_batched: images uint8 [bytes] and table int64 [n * %d, 5], got %s %s and %s %s"
                         % (n_levels, images.dtype, tuple(images.shape), table.dtype, tuple(table.shape)))
    rows = table.shape[0]
    ws_bytes = int(lib.rwh_orb_workspace_bytes(rows))
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=images.device)
    status = lib.rwh_orb_pyramid_batched(_ptr(images), images.shape[0], int(planes_offset), _ptr(table), rows // n_levels, sc.ctypes.data, n_levels,
                                         _ptr(ws), ws_bytes, _lib.stream_ptr())
    if status == _lib.RWH_E_INVALID:
        raise ValueError("orb_pyramid_batched: scales %s (Q8: 256 first, strictly increasing, <= 1024, at most 16) or planes_offset %d "
                         "outside 0 .. %d" % (sc.tolist(), int(planes_offset), images.shape[0]))
    check(status, "rwh_orb_pyramid_batched")
    return images


def orb_describe_batched(gray, gray_bytes, table, keys, counts, n_features, bin_table, pattern):
    """Orientation bin and steered BRIEF descriptor of the first min(counts[i], n_features) keys of every row of `keys`
    (rwh_orb_describe_batched, include/rwh.h), one wavefront per keypoint.

    gray, table: as orb_detect_batched gave / took them; keys: int64 [n, stride], every row SORTED ascending; counts: int32 [n];
    bin_table: int32 [30, 2]; pattern: int8 [30, 8 * nbytes, 4] -- all on the GPU.  Returns (kps float32 [n, n_features, 2] as
    (x, y), desc uint8 [n, n_features, nbytes], score int32 [n, n_features], bin int32 [n, n_features]) on the GPU; rows past an
    image's count are zero.  nbytes outside 1 .. MATCH_MAX_BYTES: NotImplementedError."""
    lib = _lib.load()
    _dev_check(gray, table, keys, counts, bin_table, pattern)
    n = table.shape[0]
    if not (keys.dtype == torch.int64 and keys.dim() == 2 and keys.shape[0] == n and counts.dtype == torch.int32 and
            tuple(counts.shape) == (n,) and bin_table.dtype == torch.int32 and tuple(bin_table.shape) == (ORB_BINS, 2) and
            pattern.dtype == torch.int8 and pattern.dim() == 3 and pattern.shape[0] == ORB_BINS and pattern.shape[2] == 4 and
            pattern.shape[1] % 8 == 0):
        raise ValueError("orb_describe_batched: keys int64 [n, stride], counts int32 [n], bin_table int32 [30, 2], pattern int8 [30, nbits, 4]")
    nbytes = pattern.shape[1] // 8
    if nbytes < 1 or nbytes > MATCH_MAX_BYTES:
        raise NotImplementedError("orb: descriptors of %d bytes; the extractor takes 1 .. %d" % (nbytes, MATCH_MAX_BYTES))
    dev, nf = gray.device, int(n_features)
    kps = torch.zeros((n, nf, 2), dtype=torch.float32, device=dev)
    desc = torch.zeros((n, nf, nbytes), dtype=torch.uint8, device=dev)
    score = torch.zeros((n, nf), dtype=torch.int32, device=dev)
    bins = torch.zeros((n, nf), dtype=torch.int32, device=dev)
    check(lib.rwh_orb_describe_batched(_ptr(gray), int(gray_bytes), _ptr(table), n, _ptr(keys), keys.shape[1], _ptr(counts), nf, _ptr(bin_table),
                                       _ptr(pattern), nbytes, _ptr(kps), _ptr(desc), _ptr(score), _ptr(bins), _lib.stream_ptr()),
          "rwh_orb_describe_batched")
    return kps, desc, score, bins


def project_points(h9, pts, inverse):
    """Launch the projection kernel: h9 [9] float32, pts [M,2] float32 -> [3,M] float32."""
    lib = _lib.load()
    _dev_check(h9, pts)
    M = pts.shape[0]
    out = torch.empty((3, M), dtype=torch.float32, device=pts.device)
    check(lib.rwh_project_points(_ptr(h9), _ptr(pts), M, 1 if inverse else 0, _ptr(out), _lib.stream_ptr()),
          "rwh_project_points")
    return out


def project_points_ex(h9, pts3):
    """General projection (rwh_project_points_ex): h9 [9], pts3 [3,M], both float32 or both float64 -> [3,M] same dtype."""
    lib = _lib.load()
    _dev_check(h9, pts3)
    assert h9.dtype == pts3.dtype and h9.dtype in (torch.float32, torch.float64) and pts3.shape[0] == 3
    out = torch.empty_like(pts3)
    check(lib.rwh_project_points_ex(_ptr(h9), _ptr(pts3), pts3.shape[1], _DTYPE[h9.dtype], _ptr(out), _lib.stream_ptr()),
          "rwh_project_points_ex")
    return out


def stitch_panorama(img_t, img_q, inv_h, grid_origin, warp_wh, t_origin, q_origin, canvas_hw, blend, rate, zero_origin=True, fast=False):
    """Launch the fused compositor: img_t / img_q [H,W,3] uint8 GPU tensors -> canvas [fh,fw,3] uint8.  fast=True: the
    staged warp kernel with the compositor epilogue (within 1 LSB); False: the exact float64 kernel (bit-identical).
    blend: 0 / False paste, 1 / True 'Rate', 2 'Gradient' (exact kernel only)."""
    lib = _lib.load()
    _dev_check(img_t, img_q)
    assert img_t.dtype == torch.uint8 and img_q.dtype == torch.uint8 and img_t.shape[2] == 3 and img_q.shape[2] == 3
    fh, fw = canvas_hw
    out = torch.empty((fh, fw, 3), dtype=torch.uint8, device=img_t.device)
    ih = np.ascontiguousarray(inv_h, dtype=np.float64).reshape(9)
    check(lib.rwh_stitch_panorama(_ptr(img_t), img_t.shape[0], img_t.shape[1], _ptr(img_q), img_q.shape[0], img_q.shape[1],
                                  ih.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(grid_origin[0]), int(grid_origin[1]),
                                  int(warp_wh[0]), int(warp_wh[1]), int(t_origin[0]), int(t_origin[1]), int(q_origin[0]),
                                  int(q_origin[1]), int(fh), int(fw), int(blend), float(rate), _ptr(out),
                                  (RWH_WARP_ZERO_ORIGIN if zero_origin else 0) | (_lib.RWH_STITCH_FAST if fast else 0),
                                  _lib.stream_ptr()), "rwh_stitch_panorama")
    return out


def stitch_panorama_rows(img_t, img_q, inv_h, grid_origin, warp_wh, t_origin, q_origin, out, rows, blend, rate, zero_origin=False):
    """Canvas rows [rows[0], rows[1]) of the exact compositor into `out` ([fh, fw, 3] uint8 on the device): rwh_stitch_panorama_rows,
    on torch's current stream."""
    lib = _lib.load()
    _dev_check(img_t, img_q, out)
    fh, fw = int(out.shape[0]), int(out.shape[1])
    ih = np.ascontiguousarray(inv_h, dtype=np.float64).reshape(9)
    check(lib.rwh_stitch_panorama_rows(_ptr(img_t), img_t.shape[0], img_t.shape[1], _ptr(img_q), img_q.shape[0], img_q.shape[1],
                                       ih.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(grid_origin[0]), int(grid_origin[1]),
                                       int(warp_wh[0]), int(warp_wh[1]), int(t_origin[0]), int(t_origin[1]), int(q_origin[0]),
                                       int(q_origin[1]), fh, fw, int(blend), float(rate), _ptr(out), int(rows[0]), int(rows[1]),
                                       RWH_WARP_ZERO_ORIGIN if zero_origin else 0, _lib.stream_ptr()), "rwh_stitch_panorama_rows")



def stitch_panorama_ex(img_t, img_q, inv_h, grid_origin, warp_wh, t_origin, q_origin, canvas_hw, blend, rate, zero_origin=True,
                       rows=None, out=None):
    """The exact compositor on images of any element type of STITCH_DTYPE (rwh_stitch_panorama_ex): img_t [H,W,3|4], img_q
    [H,W,1|3|4] GPU tensors -> uint8 canvas [fh, fw, 3] (blend) or [fh, fw, C_T] (paste).  rows=(r0, r1): only those canvas rows,
    into `out` (the whole canvas tensor) when given.  zero_origin: paste blanks texel (0,0) of img_t in place (pass it with the
    first row tile only); blend reads that texel blanked and never writes img_t (pass it with every tile)."""
    lib = _lib.load()
    _dev_check(img_t, img_q)
    if img_t.dtype not in STITCH_DTYPE or img_q.dtype not in STITCH_DTYPE:
        raise TypeError("stitch_panorama_ex: no element type code for %s / %s" % (img_t.dtype, img_q.dtype))
    fh, fw = (int(v) for v in canvas_hw)
    cc = 3 if blend else int(img_t.shape[2])
    if out is None:
        out = torch.empty((fh, fw, cc), dtype=torch.uint8, device=img_t.device)
    else:
        _dev_check(out)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (fh, fw, cc)
    r0, r1 = (0, fh) if rows is None else (int(rows[0]), int(rows[1]))
    ih = np.ascontiguousarray(inv_h, dtype=np.float64).reshape(9)
    check(lib.rwh_stitch_panorama_ex(_ptr(img_t), img_t.shape[0], img_t.shape[1], img_t.shape[2], STITCH_DTYPE[img_t.dtype],
                                     _ptr(img_q), img_q.shape[0], img_q.shape[1], img_q.shape[2], STITCH_DTYPE[img_q.dtype],
                                     ih.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(grid_origin[0]), int(grid_origin[1]),
                                     int(warp_wh[0]), int(warp_wh[1]), int(t_origin[0]), int(t_origin[1]), int(q_origin[0]),
                                     int(q_origin[1]), fh, fw, cc, int(blend), float(rate), _ptr(out), r0, r1,
                                     RWH_WARP_ZERO_ORIGIN if zero_origin else 0, _lib.stream_ptr()), "rwh_stitch_panorama_ex")
    return out


SEQ_MAX_IMAGES = _lib.RWH_SEQ_MAX_IMAGES
SEQ_BLEND = {False: _lib.RWH_SEQ_PASTE, "feather": _lib.RWH_SEQ_FEATHER}


class SeqGeometry(NamedTuple):
    """Where a sequence call composites: what every launcher of the family takes beside the images, in one of three forms -- the
    anchor's plane (the sequence rule of include/rwh.h), a curved canvas (the projection rule) or a wrap-around one (the ring rule).
    mats: n matrices, inv(G_i) on the plane and M_i = inv(G_i) @ K on a curved canvas; rects: n (mx, my, wt, ht), off the plane in
    CANVAS coordinates (on the ring 0 <= mx < P, wt <= P and mx + wt allowed past the edge); size: (fh, fw), on the ring (fh, P);
    anchor and origin (ox, oy): of the plane, where alone the library takes them; rays: None on the plane, else the two ray tables
    (homography.sequence_ray_tables), which a launcher takes as float64 GPU tensors [fw, 2] and [fh, 2]; ring: the canvas wraps."""
    mats: object
    rects: object
    size: tuple
    anchor: int = 0
    origin: tuple = (0, 0)
    rays: object = None
    ring: bool = False

    @property
    def form(self):
        """What the names of this form's entry points end in."""
        return "" if self.rays is None else "_ring" if self.ring else "_proj"

    def on_device(self, dev):
        """A copy with the ray tables (numpy arrays or tensors) on `dev`; the plane has none and is returned as it is."""
        if self.rays is None:
            return self
        return self._replace(rays=tuple(t.to(dev) if isinstance(t, torch.Tensor) else _xfer.to_device(t, dev) for t in self.rays))

    def layout(self, tables, n, own, rays, canvas, tail):
        """The argument list of an entry point of this form -- the one place that knows where anchor, ray tables and origin go:
            images hw mats rects n [anchor] | own | [col row] | canvas = [out] h w | [origin_x origin_y] | tail
        tables: the four arrays of `_sequence_marshal`; own: the operation's own arguments; rays: `_sequence_rays`'s addresses."""
        head = (tables[0].ctypes.data, tables[1].ctypes.data, tables[2].ctypes.data, tables[3].ctypes.data, n)
        if self.rays is None:
            return head + (int(self.anchor),) + own + canvas + (int(self.origin[0]), int(self.origin[1])) + tail
        return head + own + rays + canvas + tail


def sequence_tables(shapes, inv_g, rects, order):
    """The host tables of rwh_stitch_sequence / rwh_host_stitch_sequence as contiguous arrays: (hw int32 [n, 2], inv_g float64
    [n, 9], rects int32 [n, 4], order int32 [n])."""
    n = len(shapes)
    hw = np.ascontiguousarray([[int(s[0]), int(s[1])] for s in shapes], dtype=np.int32).reshape(n, 2)
    return (hw, np.ascontiguousarray(inv_g, dtype=np.float64).reshape(n, 9), np.ascontiguousarray(rects, dtype=np.int32).reshape(n, 4),
            np.ascontiguousarray(order, dtype=np.int32).reshape(-1))


def sequence_gains_array(gains, n, who="stitch_sequence"):
    """`gains` of the gain rule as a contiguous float64 [n] array; ValueError for another length, a non-finite value or one <= 0."""
    g = np.ascontiguousarray(gains.detach().cpu().numpy() if isinstance(gains, torch.Tensor) else gains, dtype=np.float64)
    if g.shape != (n,) or not (np.isfinite(g).all() and (g > 0).all()):
        raise ValueError("%s: gains takes %d finite values > 0, got %r" % (who, n, g.tolist() if g.size <= 64 else g.shape))
    return g


class SeqGainMaps(NamedTuple):
    """Gain maps as a launcher takes them in place of N gains (the block gain rule of include/rwh.h, "Applying maps"): maps, float64
    [n, gh, gw] (a GPU tensor, or numpy, which is uploaded) for cells of `block` x `block` canvas pixels."""
    maps: object
    block: int


def sequence_block_shift(who, block):
    """s of the block gain rule for `block` = 2^s; ValueError unless block is 16, 32, 64 or 128."""
    if not (isinstance(block, (int, np.integer)) and not isinstance(block, bool) and block in _lib.RWH_SEQ_BLOCKS):
        raise ValueError("%s: block %r; one of %s" % (who, block, ", ".join(str(b) for b in _lib.RWH_SEQ_BLOCKS)))
    return int(block).bit_length() - 1


def sequence_cell_grid(size, block):
    """(gh, gw): the cells of a canvas of `size` = (fh, fw)."""
    return -(-int(size[0]) // int(block)), -(-int(size[1]) // int(block))


def _sequence_no_ring_maps(who, geom):
    if geom.ring:
        raise NotImplementedError("%s: a wrap-around canvas; the block gain rule (include/rwh.h) has no ring form" % who)


def _sequence_gain_maps(who, gains, n, fh, fw, dev):
    """A SeqGainMaps as the library takes it -> (the maps on `dev`, held by the caller until its call has returned; shift).
    ValueError: another block, maps that are not float64 [n, gh, gw] for this canvas; a numpy array is also read: every entry
    finite and > 0."""
    shift = sequence_block_shift(who, gains.block)
    maps = gains.maps
    want = (n,) + sequence_cell_grid((fh, fw), gains.block)
    if not isinstance(maps, torch.Tensor):
        maps = np.ascontiguousarray(maps, dtype=np.float64)
        if maps.shape == want and not (np.isfinite(maps).all() and (maps > 0).all()):
            raise ValueError("%s: a gain map entry is not finite and > 0" % who)
        maps = torch.from_numpy(maps)
    if maps.dtype != torch.float64 or tuple(maps.shape) != want:
        raise ValueError("%s: gain maps are %s %s; float64 %s for a %d x %d canvas and block %d"
                         % (who, maps.dtype, tuple(maps.shape), want, fh, fw, gains.block))
    return maps.to(dev).contiguous(), shift


def sequence_bands_check(who, bands):
    """ValueError unless `bands` of the multi-band rule is an integer of 1 .. 8."""
    if not (isinstance(bands, (int, np.integer)) and not isinstance(bands, bool) and 1 <= bands <= _lib.RWH_SEQ_MAX_BANDS):
        raise ValueError("%s: bands %r; an integer of 1 .. %d" % (who, bands, _lib.RWH_SEQ_MAX_BANDS))


def _sequence_marshal(who, images, geom, order=None, own=None):
    """What every launcher of the sequence family checks and lays out -> (n, fh, fw, tables, order): tables the four arrays
    (image addresses, hw, mats, rects), `order` the index order when none is given.  own(): the launcher's own refusals, which come
    before the canvas's.  The library gets raw addresses: the caller holds the arrays until its call has returned."""
    _dev_check(*images)
    n = len(images)
    for t in images:
        assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3
    fh, fw = (int(v) for v in geom.size)
    if not (1 <= n <= SEQ_MAX_IMAGES) or (order is not None and len(order) != n) or len(geom.rects) != n or len(geom.mats) != n:
        raise ValueError("%s: %d images (1 .. %d), %d rectangles, %d matrices%s"
                         % (who, n, SEQ_MAX_IMAGES, len(geom.rects), len(geom.mats), "" if order is None else ", order of %d" % len(order)))
    if own is not None:
        own()
    if not (1 <= fh <= 65535 and 1 <= fw <= 65535 and fh * fw * 3 <= 2 ** 31 - 1):
        raise ValueError("%s: a %d x %d canvas; sides of 1 .. 65535 and at most 2^31 - 1 bytes" % (who, fh, fw))
    hw, mats, rc, od = sequence_tables([t.shape for t in images], geom.mats, geom.rects, list(range(n)) if order is None else order)
    return n, fh, fw, (np.array([t.data_ptr() for t in images], dtype=np.uint64), hw, mats, rc), od


def _sequence_canvas(images, fh, fw, out):
    """`out` when given, else a new tensor: uint8 [fh, fw, 3] on the device."""
    if out is None:
        return torch.empty((fh, fw, 3), dtype=torch.uint8, device=images[0].device)
    _dev_check(out)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (fh, fw, 3)
    return out


def _sequence_status(status, what, refused):
    """RWH_E_INVALID -> ValueError(refused()), the text made only when it is needed; any other status through `check`."""
    if status == _lib.RWH_E_INVALID:
        raise ValueError(refused())
    check(status, what)


def _sequence_rays(who, geom, fh, fw):
    """The addresses of a curved canvas's ray tables as the library takes them, float64 GPU tensors of exactly [fw, 2] and [fh, 2];
    () on the plane."""
    if geom.rays is None:
        return ()
    col, row = geom.rays
    _dev_check(col, row)
    for name, t, side in (("col", col, fw), ("row", row, fh)):
        if t.dtype != torch.float64 or tuple(t.shape) != (side, 2) or not t.is_contiguous():
            raise ValueError("%s: %s is %s %s; a contiguous float64 [%d, 2] table" % (who, name, t.dtype, tuple(t.shape), side))
    return _ptr(col), _ptr(row)


def _sequence_labels(who, labels, fh, fw, dev):
    """A label plane as the library takes it: a contiguous uint8 [fh, fw] GPU tensor (a numpy plane is uploaded)."""
    if not isinstance(labels, torch.Tensor):
        labels = torch.from_numpy(np.ascontiguousarray(labels))
    if labels.dtype != torch.uint8 or tuple(labels.shape) != (fh, fw):
        raise ValueError("%s: labels are %s %s; a uint8 [%d, %d] plane" % (who, labels.dtype, tuple(labels.shape), fh, fw))
    return labels.to(dev).contiguous()


def _sequence_label_plane(images, fh, fw, out):
    if out is None:
        return torch.empty((fh, fw), dtype=torch.uint8, device=images[0].device)
    _dev_check(out)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (fh, fw) and out.is_contiguous()
    return out


def _sequence_workspace(need, dev, refused):
    """A workspace of `need` bytes, allocated per call -> (the tensor, its three arguments: workspace bytes stream).  A size <= 0
    is the size function's refusal: ValueError(refused())."""
    if need <= 0:
        raise ValueError(refused())
    ws = torch.empty(((int(need) + 7) // 8,), dtype=torch.int64, device=dev)
    return ws, (_ptr(ws), ws.numel() * 8, _lib.stream_ptr())


def _addr(array):
    return None if array is None else array.ctypes.data


_REFUSED = {"": "anchor, rectangles on the canvas, finite inv(G)",
            "_proj": "rectangles on the canvas, finite M, the tables",
            "_ring": "a period that is a multiple of 256, rectangles that start on the canvas and are at most one period wide, finite M, the tables"}
_SEAM_REFUSED = ("%s: the library refused the arguments (include/rwh.h, the seam rule: anchor, rectangles on the canvas, finite matrices, "
                 "margin >= 0, tau of 1 .. 766, wt * ht * tau <= 2^32 - 3, the label plane)")


def _sequence_refused(who, geom, entry, what):
    """What a launcher says when the library refuses its arguments: the rule of the form (on the plane the entry point's), and
    what it refuses -- `what` the operation adds; on the plane its last item closes the list, as the texts always had it."""
    if geom.form == "":
        *first, last = what.split(", ")
        return "%s: the library refused the arguments (include/rwh.h, %s: %s)" % (who, entry, ", ".join(first + [_REFUSED[""], last]))
    rule = {"_proj": "the projection rule", "_ring": "the ring rule"}[geom.form]
    return "%s: the library refused the arguments (include/rwh.h, %s: %s, %s)" % (who, rule, what, _REFUSED[geom.form])


def _sequence_no_ring(who, geom):
    if geom.ring:
        raise NotImplementedError("%s: a wrap-around canvas; the seam rule (include/rwh.h) has no ring form" % who)


SEAM_TILE = (_lib.RWH_SEAM_TILE_W, _lib.RWH_SEAM_TILE_H)


def sequence_seam_options(who, margin, tau):
    """ValueError unless `margin` of the seam rule is a number >= 0 (inf included) and `tau` an integer of 1 .. 766."""
    if not (isinstance(margin, (int, float, np.integer, np.floating)) and not isinstance(margin, bool) and margin >= 0):
        raise ValueError("%s: margin %r; a number >= 0 (inf included)" % (who, margin))
    if not (isinstance(tau, (int, np.integer)) and not isinstance(tau, bool) and 1 <= tau <= 766):
        raise ValueError("%s: tau %r; an integer of 1 .. 766" % (who, tau))


# The six launchers, named for their operation with `_on` (a geometry).  Each takes the images (n [h, w, 3] uint8 GPU tensors)
# and a SeqGeometry, finds its entry point by name -- operation plus the geometry's form -- and runs on torch's current stream.
# They refuse in one order: the device check and the image asserts, the counts, the launcher's own option, the canvas bound, the
# ray tables, the label plane, the output tensor, a workspace size <= 0, the library's status (RWH_E_INVALID raises ValueError).
def stitch_sequence_on(images, geom, order, blend, rows=None, out=None, gains=None):
    """The sequence compositor (rwh_stitch_sequence_ex / _proj / _ring): order: a permutation of 0 .. n-1; blend: RWH_SEQ_PASTE /
    RWH_SEQ_FEATHER -> canvas [fh, fw, 3] uint8.  rows=(r0, r1): only those canvas rows, into `out` (the whole canvas tensor) when
    given.  gains: None, or n gains of the gain rule (every sample value v of image i enters as min(v * gains[i], 255.0)), or a
    SeqGainMaps (the block gain rule: the gain is read from image i's map at the pixel; rwh_stitch_sequence_maps / _proj, not on
    the ring)."""
    lib = _lib.load()
    who = "stitch_sequence"
    by_maps = isinstance(gains, SeqGainMaps)
    if by_maps:
        _sequence_no_ring_maps(who, geom)
    elif gains is not None:
        gains = sequence_gains_array(gains, len(images), who)
    n, fh, fw, tables, od = _sequence_marshal(who, images, geom, order)
    rays = _sequence_rays(who, geom, fh, fw)
    if by_maps:
        maps, shift = _sequence_gain_maps(who, gains, n, fh, fw, images[0].device)
    out = _sequence_canvas(images, fh, fw, out)
    r0, r1 = (0, fh) if rows is None else (int(rows[0]), int(rows[1]))
    refused = lambda: _sequence_refused(who, geom, "rwh_stitch_sequence", "order, row range")
    ws, ws_args = _sequence_workspace(lib.rwh_stitch_sequence_workspace_bytes(n), out.device, refused)
    entry = "rwh_stitch_sequence" + ("_maps" + geom.form if by_maps else geom.form or "_ex")
    status = getattr(lib, entry)(*geom.layout(tables, n, (od.ctypes.data, int(blend)), rays, (_ptr(out), fh, fw),
                                              (r0, r1) + ws_args + ((_ptr(maps), shift) if by_maps else (_addr(gains),))))
    _sequence_status(status, entry, refused)
    return out


def sequence_overlap_tables_on(images, geom, stride):
    """The overlap statistics of the gain rule (rwh_sequence_overlap_stats / _proj / _ring): stride: 1 .. 255, every stride-th canvas
    pixel each way is a sample -> ONE int64 [2, n, n] GPU tensor (count, sum), so that one copy brings both down (the library's
    uint64 tables: count[i][j] samples where i and j both cover, sum[i][j] the byte sums of i there)."""
    lib = _lib.load()
    who = "sequence_overlap_tables"

    def own():
        if not (isinstance(stride, (int, np.integer)) and 1 <= stride <= _lib.RWH_SEQ_MAX_STRIDE):
            raise ValueError("%s: stride %r; 1 .. %d" % (who, stride, _lib.RWH_SEQ_MAX_STRIDE))
    n, fh, fw, tables, _ = _sequence_marshal(who, images, geom, own=own)
    rays = _sequence_rays(who, geom, fh, fw)
    dev = images[0].device
    tabs = torch.empty((2, n, n), dtype=torch.int64, device=dev)
    refused = lambda: _sequence_refused(who, geom, "rwh_sequence_overlap_stats", "stride")
    ws, ws_args = _sequence_workspace(lib.rwh_sequence_overlap_stats_workspace_bytes(n, fh, fw, int(stride)), dev, refused)
    entry = "rwh_sequence_overlap_stats" + geom.form
    status = getattr(lib, entry)(*geom.layout(tables, n, (), rays, (fh, fw), (int(stride), _ptr(tabs[0]), _ptr(tabs[1])) + ws_args))
    _sequence_status(status, entry, refused)
    return tabs


def sequence_cell_slots(geom, n, block):
    """K of the block gain rule (rwh_sequence_cell_slots): the most candidates of any cell, from the rectangles alone."""
    who = "sequence_cell_slots"
    shift = sequence_block_shift(who, block)
    rects = np.ascontiguousarray(geom.rects, dtype=np.int32).reshape(-1, 4)
    k = _lib.load().rwh_sequence_cell_slots(rects.ctypes.data, int(n), int(geom.size[0]), int(geom.size[1]), int(geom.origin[0]),
                                            int(geom.origin[1]), shift)
    if k < 1:
        raise ValueError("%s: the library refused the arguments (include/rwh.h, the block gain rule: 1 .. %d rectangles on the canvas)"
                         % (who, SEQ_MAX_IMAGES))
    return int(k)


def sequence_cell_candidates(geom, n, block):
    """The candidates of every cell of the block gain rule, in index order: bool [gh, gw, n] (the images whose rectangles meet the
    clipped cell)."""
    gh, gw = sequence_cell_grid(geom.size, block)
    fh, fw = int(geom.size[0]), int(geom.size[1])
    r = np.asarray(geom.rects, dtype=np.int64).reshape(n, 4)
    rx, ry = r[:, 0] - int(geom.origin[0]), r[:, 1] - int(geom.origin[1])
    x0, y0 = np.arange(gw) * block, np.arange(gh) * block
    x1, y1 = np.minimum(x0 + block, fw), np.minimum(y0 + block, fh)
    cols = (rx[None, :] < x1[:, None]) & (rx[None, :] + r[None, :, 2] > x0[:, None])
    rows = (ry[None, :] < y1[:, None]) & (ry[None, :] + r[None, :, 3] > y0[:, None])
    return rows[:, None, :] & cols[None, :, :]


def sequence_cell_tables_on(images, geom, block, stride):
    """The cell statistics of the block gain rule (rwh_sequence_cell_stats / _proj): block: 16, 32, 64 or 128; stride: as
    `sequence_overlap_tables_on`'s -> ONE int32 [gh, gw, 2, K, K] GPU tensor holding the library's uint32 table (count, sum per
    cell, by candidate rank; K = `sequence_cell_slots`), so that one copy brings it down.  Not on the ring."""
    lib = _lib.load()
    who = "sequence_cell_tables"
    _sequence_no_ring_maps(who, geom)

    def own():
        sequence_block_shift(who, block)
        if not (isinstance(stride, (int, np.integer)) and 1 <= stride <= _lib.RWH_SEQ_MAX_STRIDE):
            raise ValueError("%s: stride %r; 1 .. %d" % (who, stride, _lib.RWH_SEQ_MAX_STRIDE))
    n, fh, fw, tables, _ = _sequence_marshal(who, images, geom, own=own)
    shift = sequence_block_shift(who, block)
    rays = _sequence_rays(who, geom, fh, fw)
    slots = sequence_cell_slots(geom, n, block)
    gh, gw = sequence_cell_grid((fh, fw), block)
    dev = images[0].device
    assert lib.rwh_sequence_cell_stats_table_bytes(fh, fw, shift, slots) == gh * gw * 2 * slots * slots * 4
    tabs = torch.empty((gh, gw, 2, slots, slots), dtype=torch.int32, device=dev)
    refused = lambda: _sequence_refused(who, geom, "rwh_sequence_cell_stats", "block, stride, slots")
    ws, ws_args = _sequence_workspace(lib.rwh_sequence_cell_stats_workspace_bytes(n), dev, refused)
    entry = "rwh_sequence_cell_stats" + geom.form
    status = getattr(lib, entry)(*geom.layout(tables, n, (), rays, (fh, fw), (shift, int(stride), slots, _ptr(tabs)) + ws_args))
    _sequence_status(status, entry, refused)
    return tabs


def host_sequence_block_gains(tables, geom, n, block, base=None, sigma_n=10.0, sigma_g=0.1, smooth=2):
    """Cell gains, smoothing and maps of the block gain rule (rwh_host_sequence_block_gains; host only): tables: the uint32
    [gh, gw, 2, K, K] table of `sequence_cell_tables_on`, brought down; base: None or n gains -> (status, maps float64 [n, gh, gw])."""
    shift = sequence_block_shift("sequence_block_gains", block)
    gh, gw = sequence_cell_grid(geom.size, block)
    tables = np.ascontiguousarray(tables).view(np.uint32)
    slots = int(tables.shape[-1])
    assert tables.shape == (gh, gw, 2, slots, slots)
    rects = np.ascontiguousarray(geom.rects, dtype=np.int32).reshape(-1, 4)
    base = None if base is None else np.ascontiguousarray(base, dtype=np.float64)
    assert base is None or base.shape == (n,)
    maps = np.empty((n, gh, gw), dtype=np.float64)
    status = _lib.load().rwh_host_sequence_block_gains(tables.ctypes.data, rects.ctypes.data, int(n), int(geom.size[0]), int(geom.size[1]),
                                                       int(geom.origin[0]), int(geom.origin[1]), shift, slots, _addr(base), float(sigma_n),
                                                       float(sigma_g), int(smooth), maps.ctypes.data)
    return status, maps


def stitch_sequence_multiband_on(images, geom, bands, gains=None, out=None, labels=None):
    """The multi-band compositor (rwh_stitch_multiband / _proj / _ring; the multi-band rule of include/rwh.h): bands: 1 .. 8 pyramid
    levels below the top; gains: as `stitch_sequence_on`'s (a SeqGainMaps: rwh_stitch_multiband_maps / _proj) -> canvas [fh, fw, 3] uint8 (`out` when given).  labels: None, or a uint8
    [fh, fw] plane (a GPU tensor or numpy) that takes the Winner's place (rwh_stitch_multiband_labels / _labels_proj; the seam rule,
    "Using labels"): a label that names no covering image leaves the multi-band rule's Winner; not on the ring."""
    who = "stitch_sequence_multiband"
    if labels is not None:
        _sequence_no_ring(who, geom)
    lib = _lib.load()
    by_maps = isinstance(gains, SeqGainMaps)
    if by_maps:
        _sequence_no_ring_maps(who, geom)
    elif gains is not None:
        gains = sequence_gains_array(gains, len(images), who)
    n, fh, fw, tables, _ = _sequence_marshal(who, images, geom, own=lambda: sequence_bands_check(who, bands))
    rays = _sequence_rays(who, geom, fh, fw)
    if by_maps:
        maps, shift = _sequence_gain_maps(who, gains, n, fh, fw, images[0].device)
    if labels is not None:
        labels = _sequence_labels(who, labels, fh, fw, images[0].device)
    out = _sequence_canvas(images, fh, fw, out)
    refused = lambda: _sequence_refused(who, geom, "rwh_stitch_multiband", "bands") if labels is None else _SEAM_REFUSED % who
    if geom.ring:
        need = lib.rwh_stitch_multiband_ring_workspace_bytes(tables[3].ctypes.data, n, fh, fw, int(bands))
    else:
        need = lib.rwh_stitch_multiband_workspace_bytes(tables[3].ctypes.data, n, fh, fw, int(geom.origin[0]), int(geom.origin[1]), int(bands))
    ws, ws_args = _sequence_workspace(need, out.device, refused)
    if by_maps:
        entry = "rwh_stitch_multiband_maps" + geom.form
        own = (int(bands), _ptr(maps), shift, None if labels is None else _ptr(labels))
    else:
        entry = "rwh_stitch_multiband" + ("" if labels is None else "_labels") + geom.form
        own = (int(bands), _addr(gains)) + (() if labels is None else (_ptr(labels),))
    status = getattr(lib, entry)(*geom.layout(tables, n, own, rays, (_ptr(out), fh, fw), ws_args))
    _sequence_status(status, entry, refused)
    return out


def stitch_sequence_labels_on(images, geom, labels, gains=None, out=None):
    """Label paste (rwh_stitch_sequence_labels / _proj; the seam rule, "Using labels"): every canvas pixel takes the bytes of the image
    its label names where that image covers it, of the covering image with the greatest feather weight elsewhere.  labels: as
    `stitch_sequence_multiband_on`'s.  Not on the ring."""
    who = "stitch_sequence_labels"
    _sequence_no_ring(who, geom)
    lib = _lib.load()
    by_maps = isinstance(gains, SeqGainMaps)
    if gains is not None and not by_maps:
        gains = sequence_gains_array(gains, len(images), who)
    n, fh, fw, tables, _ = _sequence_marshal(who, images, geom)
    rays = _sequence_rays(who, geom, fh, fw)
    if by_maps:
        maps, shift = _sequence_gain_maps(who, gains, n, fh, fw, images[0].device)
    labels = _sequence_labels(who, labels, fh, fw, images[0].device)
    out = _sequence_canvas(images, fh, fw, out)
    refused = lambda: _SEAM_REFUSED % who
    ws, ws_args = _sequence_workspace(lib.rwh_stitch_sequence_workspace_bytes(n), out.device, refused)
    entry = "rwh_stitch_sequence_labels" + ("_maps" if by_maps else "") + geom.form
    own = (_ptr(maps), shift, _ptr(labels)) if by_maps else (_addr(gains), _ptr(labels))
    status = getattr(lib, entry)(*geom.layout(tables, n, own, rays, (_ptr(out), fh, fw), ws_args))
    _sequence_status(status, entry, refused)
    return out


def sequence_seams_on(images, geom, gains=None, margin=8.0, tau=64, out=None, info=None):
    """The seam finder (rwh_sequence_seams / _proj; the seam rule of include/rwh.h): gains: as `stitch_sequence_on`'s; margin (8.0) and
    tau (64): the rule's two conventions -> labels [fh, fw] uint8 (`out` when given).  The call SYNCHRONISES the stream between its
    relaxation passes.  `info`: optional dict, receives "passes".  Not on the ring."""
    who = "sequence_seams"
    _sequence_no_ring(who, geom)
    lib = _lib.load()
    if gains is not None:
        gains = sequence_gains_array(gains, len(images), who)
    n, fh, fw, tables, _ = _sequence_marshal(who, images, geom, own=lambda: sequence_seam_options(who, margin, tau))
    rays = _sequence_rays(who, geom, fh, fw)
    out = _sequence_label_plane(images, fh, fw, out)
    need = lib.rwh_sequence_seams_workspace_bytes(tables[3].ctypes.data, n, fh, fw, int(geom.origin[0]), int(geom.origin[1]))
    refused = lambda: _SEAM_REFUSED % who
    ws, ws_args = _sequence_workspace(need, out.device, refused)
    passes = ctypes.c_int32(0)
    entry = "rwh_sequence_seams" + geom.form
    status = getattr(lib, entry)(*geom.layout(tables, n, (_addr(gains), float(margin), int(tau)), rays, (_ptr(out), fh, fw),
                                              ws_args + (ctypes.addressof(passes),)))
    _sequence_status(status, entry, refused)
    if info is not None:
        info["passes"] = int(passes.value)
    return out


# The launchers under their earlier names, one per canvas form, with the argument lists that callers of this module know (the
# planar five are named in README.md and INTEGRATION.md as the family's Python surface).  Each makes the geometry from its loose
# arguments and calls the `_on` launcher of its operation; nothing else happens here.
def _plane(inv_g, rects, anchor, origin, canvas_hw):
    return SeqGeometry(inv_g, rects, canvas_hw, anchor, origin)


def _curved(m, rects, col, row, canvas_hw, ring=False):
    return SeqGeometry(m, rects, canvas_hw, rays=(col, row), ring=ring)


def stitch_sequence(images, inv_g, rects, anchor, order, blend, origin, canvas_hw, rows=None, out=None, gains=None):
    return stitch_sequence_on(images, _plane(inv_g, rects, anchor, origin, canvas_hw), order, blend, rows, out, gains)


def stitch_sequence_proj(images, m, rects, col, row, order, blend, canvas_hw, rows=None, out=None, gains=None):
    return stitch_sequence_on(images, _curved(m, rects, col, row, canvas_hw), order, blend, rows, out, gains)


def stitch_sequence_ring(images, m, rects, col, row, order, blend, canvas_hw, rows=None, out=None, gains=None):
    return stitch_sequence_on(images, _curved(m, rects, col, row, canvas_hw, True), order, blend, rows, out, gains)


def sequence_overlap_tables(images, inv_g, rects, anchor, origin, canvas_hw, stride):
    return sequence_overlap_tables_on(images, _plane(inv_g, rects, anchor, origin, canvas_hw), stride)


def sequence_overlap_tables_proj(images, m, rects, col, row, canvas_hw, stride):
    return sequence_overlap_tables_on(images, _curved(m, rects, col, row, canvas_hw), stride)


def sequence_overlap_tables_ring(images, m, rects, col, row, canvas_hw, stride):
    return sequence_overlap_tables_on(images, _curved(m, rects, col, row, canvas_hw, True), stride)


def sequence_overlap_stats(images, inv_g, rects, anchor, origin, canvas_hw, stride):
    """`sequence_overlap_tables` as (count, sum), two int64 [n, n] GPU tensors."""
    tabs = sequence_overlap_tables(images, inv_g, rects, anchor, origin, canvas_hw, stride)
    return tabs[0], tabs[1]


def stitch_sequence_multiband(images, inv_g, rects, anchor, origin, canvas_hw, bands, gains=None, out=None):
    return stitch_sequence_multiband_on(images, _plane(inv_g, rects, anchor, origin, canvas_hw), bands, gains, out)


def stitch_sequence_multiband_proj(images, m, rects, col, row, canvas_hw, bands, gains=None, out=None):
    return stitch_sequence_multiband_on(images, _curved(m, rects, col, row, canvas_hw), bands, gains, out)


def stitch_sequence_multiband_ring(images, m, rects, col, row, canvas_hw, bands, gains=None, out=None):
    return stitch_sequence_multiband_on(images, _curved(m, rects, col, row, canvas_hw, True), bands, gains, out)


def stitch_sequence_multiband_labels(images, inv_g, rects, anchor, origin, canvas_hw, bands, labels, gains=None, out=None):
    return stitch_sequence_multiband_on(images, _plane(inv_g, rects, anchor, origin, canvas_hw), bands, gains, out, labels)


def stitch_sequence_multiband_labels_proj(images, m, rects, col, row, canvas_hw, bands, labels, gains=None, out=None):
    return stitch_sequence_multiband_on(images, _curved(m, rects, col, row, canvas_hw), bands, gains, out, labels)


def stitch_sequence_labels(images, inv_g, rects, anchor, origin, canvas_hw, labels, gains=None, out=None):
    return stitch_sequence_labels_on(images, _plane(inv_g, rects, anchor, origin, canvas_hw), labels, gains, out)


def stitch_sequence_labels_proj(images, m, rects, col, row, canvas_hw, labels, gains=None, out=None):
    return stitch_sequence_labels_on(images, _curved(m, rects, col, row, canvas_hw), labels, gains, out)


def sequence_seams(images, inv_g, rects, anchor, origin, canvas_hw, gains=None, margin=8.0, tau=64, out=None, info=None):
    return sequence_seams_on(images, _plane(inv_g, rects, anchor, origin, canvas_hw), gains, margin, tau, out, info)


def sequence_seams_proj(images, m, rects, col, row, canvas_hw, gains=None, margin=8.0, tau=64, out=None, info=None):
    return sequence_seams_on(images, _curved(m, rects, col, row, canvas_hw), gains, margin, tau, out, info)


def decode_best(best_words, k_total):
    """Unpack the two argmax words (host ints) -> (winner_index, count, early_exit).
    Word 1 (first index reaching `need`) takes precedence, like the reference's
    `break` (ransac.py:186-190); otherwise word 0 = max count, lowest index."""
    w0, w1 = int(best_words[0]), int(best_words[1])
    if w1 != 0:
        return 0xFFFFFFFF - w1, None, True
    if (w0 >> 32) == 0:  # nothing ever scored > 0: the reference keeps no model (ransac.py:199)
        return None, 0, False
    return 0xFFFFFFFF - (w0 & 0xFFFFFFFF), w0 >> 32, False


def need_count(m, d, n):
    """ransac.py:169,186: count >= m*d/100 + n, as an integer threshold."""
    return int(math.ceil(m * d / 100 + n))


class ClockProbe:
    """Shader clock held while other kernels run (rwh_lab_clock_probe): one wavefront on a side stream that stays resident
    for `ms` milliseconds of the 100 MHz constant clock and counts shader cycles meanwhile.
        p = ClockProbe(ms); ... enqueue the kernels being measured ...; mhz = p.mhz()"""

    def __init__(self, ms):
        lib = _lib.load()
        self.out = torch.zeros(2, dtype=torch.int64, device=_lib.require_gpu())
        self.stream = torch.cuda.Stream()
        self.stream.wait_stream(torch.cuda.current_stream())        # the zero fill above
        check(lib.rwh_lab_clock_probe(_ptr(self.out), float(ms), ctypes.c_void_p(self.stream.cuda_stream)), "rwh_lab_clock_probe")

    def mhz(self):
        self.stream.synchronize()
        cyc, ticks = (int(v) for v in self.out.cpu())
        return 100.0 * cyc / ticks if ticks else float("nan")


def power_node(device_index=None):
    """Path of the amdgpu hwmon file holding this device's board power in microwatts (power1_average / power1_input), or
    None.  Read it with open(): a process that has initialised the GPU must not fork + exec a tool like rocm-smi."""
    import glob
    try:
        idx = torch.cuda.current_device() if device_index is None else int(device_index)
        bus = torch.cuda.get_device_properties(idx).pci_bus_id
        dom = getattr(torch.cuda.get_device_properties(idx), "pci_domain_id", 0)
        dev = getattr(torch.cuda.get_device_properties(idx), "pci_device_id", 0)
        pci = "%04x:%02x:%02x.0" % (dom, bus, dev)
    except Exception:
        return None
    for leaf in ("power1_average", "power1_input"):
        hits = glob.glob("/sys/bus/pci/devices/%s/hwmon/hwmon*/%s" % (pci, leaf))
        if hits:
            return hits[0]
    return None


def power_cap_node(device_index=None):
    """The same device's power cap (microwatts), or None."""
    node = power_node(device_index)
    if not node:
        return None
    import os
    cap = os.path.join(os.path.dirname(node), "power1_cap")
    return cap if os.path.exists(cap) else None
