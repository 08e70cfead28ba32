"""MI355X-backed mirror of the reference's `homography.py` call surface.

Same names, argument meaning, defaults, return types and error behaviour as
choice17/ransac_with_homography `homography.py`; the per-pixel work (grid ->
inverse homography -> divide -> mask -> gather -> lerp, homography.py:108-209)
runs in the hand-written HIP kernel K3 behind `rwh_warp_backward` (include/rwh.h).

numpy arrays in -> numpy arrays out (uploaded / downloaded around the kernel);
torch-ROCm tensors in -> torch-ROCm tensors out (no host round trip: bilinear
results are float32 instead of the reference's float64, nn keeps the dtype).

What stays on the host, as in SURVEY.md 8(a) row a3: the O(1) 3x3 / 8x8 solves
(`calcHomographyLinear`, `inv(H)`, output bounding box) in numpy, exactly the
reference's arithmetic.  There is no CPU implementation of the warp here: without
librwh_hip.so and a GPU the warps raise `RwhUnavailable`.

Documented divergences from the reference:
  * numpy arrays in: a coordinate exactly on the last column / row, or a scan-mode `res` beyond the image, raises the
    reference's IndexError (`rwh_warp_index_check` tells where the reference would index past the image; fixture g15).
    Tensors in (the fast kernels): the +1 bilinear tap is clamped instead (its weight is 0 there) and scan-mode bounds
    larger than the source are clipped to the source;
  * with the fast kernels (torch tensors in, or EXACT = False) the bilinear blend is float32 on
    float64-derived weights (<= 1e-4 relative to the reference's float64 blend, typically 3e-7) and
    uint8 results can differ by 1 LSB where the float64 value sits within ~1e-5 of an integer; with the
    exact kernel (numpy arrays in, the default) results are bit-identical to the reference's;
  * numpy images of every numeric dtype and 3 .. 64 channels are warped in their own dtype (uint8 / float32 with 3 or 4 channels by
    the exact kernel above, every other one by the any-dtype exact kernel): 'nn' copies texels bit for bit, 'bilinear' converts
    each tap to float64 as numpy does.  A NaN that the bilinear arithmetic produces (inf * 0, inf - inf) is NaN here too, but
    with the GPU's sign and payload (x86 gives a negative NaN); every other value is bit-identical.  1 or 2 channels: the
    reference's IndexError after channel 0 (and 1) of texel (0,0) is zeroed; non-numeric dtypes (complex, longdouble, object,
    strings, datetimes): NotImplementedError, before anything is touched;
  * the exact kernel of uint8 / float32 images with 3 or 4 channels returns 0 for a bilinear pixel outside the bounds, where the
    reference interpolates at (0, 0): the two differ when a texel next to the origin is not finite (0 * inf).  Its uint8 output
    (transformImage) converts through a saturating int32 cast: float32 values beyond int32 give 255 / 0 where numpy gives 0.
    The any-dtype kernel does both as the reference does;
  * `cylindericlMap` / `cylindricalWarp` / `cylindericalTransform` (dead code in
    the reference, needs OpenCV) are not provided beyond an import-compatible stub.
"""
import os
from typing import NamedTuple

import numpy as np

from . import _lib, _xfer, kernels

# Which warp kernels serve this module:
#   EXACT = None (default)  numpy arrays in  -> the float64 "exact" kernel: results bit-identical to the reference's
#                                               float64 arrays and truncated uint8 images (a host round trip dominates
#                                               the call anyway);
#                           torch tensors in -> the fast float32-blend kernels (<= 1e-4 relative, uint8 within 1 LSB);
#   EXACT = True / False    force one or the other (environment: RWH_EXACT=1 / RWH_EXACT=0).
EXACT = {"1": True, "0": False}.get(os.environ.get("RWH_EXACT", ""), None)

__all__ = [
    "calc_corresp", "calc_correspLinear", "calc_correspCollective", "calc_correspLinearCollective",
    "calcHomography", "calcHomographyLinear", "calcH", "nearestNeighbor", "bilinear", "convertfunc",
    "wrapPerspective", "wrapPerspectiveScan", "perspectiveTransform", "transformImage", "transformImageH",
    "BLENDDIR", "addAlpha", "stitchPanorama", "cylindericlMap", "sequence_plan", "stitchSequence", "sequence_gains", "sequence_seams",
    "sequence_block_gains", "BlockGains",
    "sequence_ray_tables", "sequence_focal", "sequence_graph", "sequence_adjust",
    "sequence_cameras", "sequence_camera_maps", "sequence_adjust_cameras",
]


# ------------------------------------------------------------------ design matrices (host, O(N)) ----
def _pair_rows(u, v, sign):
    """Shared builder.  sign=-1: DLT rows [-x,-y,-1,0,0,0, x*x', y*x', x'] (homography.py:4-14, 30-46);
    sign=+1: linear rows [x,y,1,0,0,0,-x*x',-y*x'] with b = (x', y') (homography.py:16-28, 48-69).
    Products are formed in the input dtype, storage is float32, as in the reference."""
    u = np.asarray(u)
    v = np.asarray(v)
    n = u.shape[0]
    x, y, xp, yp = u[:, 0], u[:, 1], v[:, 0], v[:, 1]
    if sign < 0:
        a = np.zeros((n, 18), dtype=np.float32)
        a[:, 0] = -x; a[:, 1] = -y; a[:, 2] = -1
        a[:, 6] = x * xp; a[:, 7] = y * xp; a[:, 8] = xp
        a[:, 12] = -x; a[:, 13] = -y; a[:, 14] = -1
        a[:, 15] = x * yp; a[:, 16] = y * yp; a[:, 17] = yp
        return a.reshape(2 * n, 9)
    a = np.zeros((n, 16), dtype=np.float32)
    b = np.zeros((n, 2), dtype=np.float32)
    a[:, 0] = x; a[:, 1] = y; a[:, 2] = 1
    a[:, 6] = -x * xp; a[:, 7] = -y * xp
    a[:, 11] = x; a[:, 12] = y; a[:, 13] = 1
    a[:, 14] = -x * yp; a[:, 15] = -y * yp
    b[:, 0] = xp; b[:, 1] = yp
    return a.reshape(2 * n, 8), b.reshape(2 * n, 1)


def _four_rows(u, v):
    """The 4-point builders index rows 0..3 of both arrays by hand (homography.py:6-13, 18-27): with fewer rows they fail at
    the first index that is not there."""
    u, v = np.asarray(u), np.asarray(v)
    for a in (u, v):
        if a.shape[0] < 4:
            raise IndexError("index %d is out of bounds for axis 0 with size %d" % (a.shape[0], a.shape[0]))
    return u[:4], v[:4]


def calc_corresp(u, v):
    """8 x 9 DLT matrix of 4 pairs, float32 (homography.py:4-14)."""
    return _pair_rows(*_four_rows(u, v), -1)


def calc_correspLinear(u, v):
    """(8 x 8 A, 8 x 1 b), float32 (homography.py:16-28)."""
    return _pair_rows(*_four_rows(u, v), +1)


def calc_correspCollective(u, v):
    """2N x 9 DLT matrix (homography.py:30-46)."""
    return _pair_rows(u, v, -1)


def calc_correspLinearCollective(u, v):
    """(2N x 8 A, 2N x 1 b) (homography.py:48-69)."""
    return _pair_rows(u, v, +1)


# ------------------------------------------------------------------------------------- solvers ----
def calcHomography(u, v, collective=False):
    """DLT homography, float32 3x3 with h33 == 1 (homography.py:71-88): the reference's own arithmetic on the host --
    float32 DLT matrix -> numpy.linalg.svd -> last right-singular vector / its 9th element.  One 8 x 9 SVD costs less than
    the upload + launch + download a GPU solve of a single sample would, and it IS the reference's solver: samples with
    a repeated index return LAPACK's null vector like the reference does.  (The batched GPU generator K1 serves
    `RANSAC.run`'s thousands of samples per call, with this solver as its arbiter: ransac._settle_on_host.)"""
    u = np.asarray(u)
    v = np.asarray(v)
    mat = calc_correspCollective(u, v) if collective else calc_corresp(u, v)
    _, _, vt = np.linalg.svd(mat)
    h = vt[-1].reshape(3, 3)
    return h / h.item(8)


def calcHomographyLinear(u, v, collective=False):
    """Normal-equation homography with h33 == 1, float64 3x3 (homography.py:90-105).
    O(1) host work (called once per scanner apply / RANSAC run)."""
    A, b = calc_correspLinearCollective(u, v) if collective else calc_correspLinear(u, v)
    h = np.linalg.inv(A.T @ A) @ (A.T @ b)
    return np.array([[h.item(0), h.item(1), h.item(2)],
                     [h.item(3), h.item(4), h.item(5)],
                     [h.item(6), h.item(7), 1]])


calcH = calcHomographyLinear  # name used by BASELINE.json's north_star


# ------------------------------------------------------------------------------- warp plumbing ----
def _is_tensor(x):
    return type(x).__module__.startswith("torch")


def _blank_origin(img):
    """Mirror homography.py:112-116 / 126-130 on the caller's HOST array (the kernel does the
    same to the device copy): channels 0..2, and 3 when there are exactly 4 (not beyond: 5+ channels keep channel 3 on)."""
    img[0, 0, 0] = 0
    img[0, 0, 1] = 0
    img[0, 0, 2] = 0
    if img.shape[2] == 4:
        img[0, 0, 3] = 0


def _to_device(img, host):
    """-> (GPU tensor [H,W,C], was_numpy, result dtype for nn).  Tensors in: uint8 | float32 (other dtypes are cast to float32);
    numpy arrays in: `host`, what _host_src returned for this image, uploaded as it is."""
    import torch
    dev = _lib.require_gpu()
    if _is_tensor(img):
        t = img
        if not t.is_cuda:
            t = t.to(dev)
        if t.dtype not in (torch.uint8, torch.float32):
            t = t.to(torch.float32)
        return t.contiguous(), False, None
    src, np_dtype = host
    return _xfer.to_device(src, dev), True, np_dtype


def _host_src(img, exact):
    """numpy image -> (the array the kernels read, the caller's dtype); no device work.

    exact (the float64 kernels): uint8 / float32 images with 3 or 4 channels as they are; every other numeric dtype (bool read as
    uint8, int8 .. int64, uint16 .. uint64, float16, float64) and channel count 3 .. RWH_WARP_MAX_CHANNELS in its own type, for the
    any-dtype kernel.  1 or 2 channels: the reference's interpolators blank channel 0 (and 1) of the caller's texel (0,0) and then
    raise IndexError at the next channel (homography.py:112-114 / 126-128); so does this.  Non-numeric dtypes (complex,
    longdouble, object, ...) raise NotImplementedError before anything is touched.
    Not exact (RWH_EXACT=0): the fast kernels' uint8 / float32 with 3 or 4 channels, other dtypes cast to float32."""
    a = np.asarray(img)
    if a.ndim != 3:
        raise ValueError("not enough values to unpack (expected 3, got %d)" % a.ndim)  # img.shape unpack
    if not exact:
        if a.shape[2] not in (3, 4):
            raise IndexError("index out of bounds: the warp supports 3 or 4 channels")
        return (a if a.dtype in (np.uint8, np.float32) else a.astype(np.float32)), a.dtype
    native = a.dtype.newbyteorder("=") if a.dtype.kind in "biuf" else a.dtype
    if native not in _STITCH_NP:
        raise NotImplementedError("warp: %s images are not warped here: the exact kernels take numeric images (bool, int8 .. int64, "
                                  "uint8 .. uint64, float16 / 32 / 64)" % a.dtype)
    c = a.shape[2]
    if c < 3:
        for k in range(c):
            img[0, 0, k] = 0
        raise IndexError("index %d is out of bounds for axis 2 with size %d" % (c, c))
    if c > _lib.RWH_WARP_MAX_CHANNELS:
        raise NotImplementedError("warp: %d channels; the exact kernels take up to %d" % (c, _lib.RWH_WARP_MAX_CHANNELS))
    if a.dtype in (np.uint8, np.float32) and c in (3, 4):
        return a, a.dtype
    if native != a.dtype:
        a = a.astype(native)
    return a.view(_STITCH_NP[native]), a.dtype


def _torch_dtype(np_dtype):
    import torch
    return torch.from_numpy(np.empty(0, np_dtype)).dtype


def _warp(img, H, grid, bound_hw, convert, u8_out):
    """Common body of wrapPerspective / wrapPerspectiveScan from `invH = inv(H)` on."""
    import torch
    if convert not in kernels.INTERP:
        raise KeyError(convert)  # convertfunc[convert], homography.py:179 / 208
    inv_h = np.linalg.inv(np.asarray(H, dtype=np.float64))  # homography.py:172 / 203 (raises LinAlgError)
    host = None if _is_tensor(img) else _host_src(img, True if EXACT is None else bool(EXACT))
    if host is not None and PIPELINE_MIN_BYTES is not None:
        # a large host array through the exact kernels: upload, kernel by output-row tiles and download overlapped (_warp_pipelined)
        a, np_dtype = host
        exact = True if EXACT is None else bool(EXACT)
        t_dtype = _torch_dtype(a.dtype)
        out_dtype = t_dtype if convert == "nn" else (torch.uint8 if u8_out else torch.float64 if exact else torch.float32)
        out_bytes = grid.out_h * grid.out_w * a.shape[2] * torch.empty(0, dtype=out_dtype).element_size()
        # (the result of a pipelined call is ONE page-locked block: capped like _xfer.to_host's, beyond it the plain path)
        if a.shape[0] >= 3 and a.shape[1] >= 3 and a.nbytes + out_bytes >= PIPELINE_MIN_BYTES * PIPELINE_WARP_FACTOR and grid.out_h >= 64 \
                and out_bytes <= _xfer.PINNED_RESULT_MAX:
            dev = _lib.require_gpu()
            a = np.ascontiguousarray(a)
            flag = kernels.warp_index_check(a.shape[:2], inv_h, grid, bound_hw, convert, dev)
            res = _warp_pipelined(a, inv_h, grid, bound_hw, convert, out_dtype, exact, dev)
            if res is not None:       # (None: page-locked memory for the result could not be had -- the plain path below)
                _blank_origin(img)
                bits = int(flag.item())
                if bits:
                    kernels.raise_like_reference(bits, a.shape[:2])
                if convert == "nn":
                    return res if res.dtype == np_dtype else res.astype(np_dtype)
                return res if (u8_out or res.dtype == np.float64) else res.astype(np.float64)
            host = (a, np_dtype)
    src, was_numpy, np_dtype = _to_device(img, host)
    true_hw = (int(src.shape[0]), int(src.shape[1]))
    if true_hw[0] < 3 or true_hw[1] < 3:      # the kernels want 3 x 3 texels at least: zero rows / columns beyond the bounds, which
        pad = torch.zeros((max(true_hw[0], 3), max(true_hw[1], 3), src.shape[2]), dtype=src.dtype, device=src.device)   # stay (h, w)
        pad[:true_hw[0], :true_hw[1]] = src
        src = pad
    exact = was_numpy if EXACT is None else bool(EXACT)
    if convert == "nn":
        out_dtype = src.dtype
    elif exact:
        out_dtype = torch.uint8 if u8_out else torch.float64
    else:
        out_dtype = torch.uint8 if u8_out else torch.float32
    # numpy arrays in (the reference's own callers): where the reference's interpolator would index past the image -- a coordinate
    # exactly on the last column / row, a scan `res` beyond the image, a NaN coordinate -- raise its IndexError (rwh.h)
    flag = kernels.warp_index_check(true_hw, inv_h, grid, bound_hw, convert, src.device) if was_numpy else None
    out = kernels.warp_backward(src, inv_h, grid, bound_hw, convert, out_dtype, zero_origin=True, exact=exact)
    if not was_numpy:
        return out
    _blank_origin(img)
    res = _xfer.to_host(out)
    bits = int(flag.item())
    if bits:
        kernels.raise_like_reference(bits, true_hw)
    if convert == "nn":
        return res if res.dtype == np_dtype else res.astype(np_dtype)
    return res if (u8_out or res.dtype == np.float64) else res.astype(np.float64)  # the reference's bilinear yields float64


def _bounds(h, w, H, boundary):
    """Output bounding box, homography.py:143-163 (host numpy, 4 points)."""
    bnd = np.array([[0, w - 1, w - 1, 0],
                    [0, 0, h - 1, h - 1],
                    [1., 1, 1, 1]])
    bnd_n = np.asarray(H) @ bnd
    bnd_n /= bnd_n[-1, :]
    max_x = int(np.max(bnd_n[0, :])); min_x = int(np.min(bnd_n[0, :]))
    max_y = int(np.max(bnd_n[1, :])); min_y = int(np.min(bnd_n[1, :]))
    if boundary:
        min_x = max(min_x, 0)
        min_y = max(min_y, 0)
    return min_x, min_y, max_x - min_x + 1, max_y - min_y + 1


def _wrap_perspective(img, H, convert, boundary, u8_out):
    h, w, _ = img.shape
    min_x, min_y, max_w, max_h = _bounds(h, w, H, boundary)
    if max_w <= 0 or max_h <= 0:
        raise ValueError("Number of samples, %d, must be non-negative." % min(max_w, max_h))  # np.linspace
    grid = kernels.Grid(min_x, min_x + max_w - 1, max_w, min_y, min_y + max_h - 1, max_h)
    return _warp(img, H, grid, (h, w), convert, u8_out), min_x, min_y


def wrapPerspective(img, H, convert='nn', boundary=0, crop=True):
    """Auto-bounds backward warp (homography.py:142-184).  Returns (img_n, min_x, min_y);
    img_n is float64 for 'bilinear' and keeps the image dtype for 'nn'."""
    if not crop:
        raise NotImplementedError("crop=False is dead, shape-inconsistent code in the reference (homography.py:180-183)")
    return _wrap_perspective(img, H, convert, boundary, False)


def wrapPerspectiveScan(img, H, res, convert='nn'):
    """Fixed-resolution backward warp (homography.py:186-209): grid linspace(0,w,w) x
    linspace(0,h,h); the bounds test uses `res` (clipped to the source here)."""
    h, w = res
    grid = kernels.Grid(0, w, w, 0, h, h)
    return _warp(img, H, grid, (h, w), convert, False), 0, 0


perspectiveTransform = wrapPerspective  # name used by BASELINE.json's north_star


def _sample(z_t, img, h, w, mh, mw, convert):
    """Common body of the two interpolators on caller-computed coordinates: `rwh_sample_points` (the reference's float64
    arithmetic, bit-identical results).  Like the reference it blanks texel (0,0) of the caller's image and, for
    'bilinear', writes 0 into the masked columns of the caller's z_t (homography.py:131-132: `z_t = z_t.T` is a view)."""
    import torch
    host = None if _is_tensor(img) else _host_src(img, True)     # (1 or 2 channels: the reference's IndexError, before z_t is touched)
    dev = _lib.require_gpu()
    chn = img.shape[2]
    if _is_tensor(z_t):
        zx, zy = z_t[0].to(dev, torch.float64).contiguous(), z_t[1].to(dev, torch.float64).contiguous()
    else:
        z_t = np.asarray(z_t)
        zx = torch.from_numpy(np.ascontiguousarray(z_t[0], dtype=np.float64)).to(dev)
        zy = torch.from_numpy(np.ascontiguousarray(z_t[1], dtype=np.float64)).to(dev)
    src, was_numpy, np_dtype = _to_device(img, host)
    out = kernels.sample_points(src, zx, zy, (h, w), convert, zero_origin=True).reshape(mh, mw, chn)
    if convert == 'bilinear' and not _is_tensor(z_t) and z_t.dtype.kind == 'f':
        mask = (z_t[0] > w - 1) | (z_t[0] < 0) | (z_t[1] > h - 1) | (z_t[1] < 0)
        z_t[0:2, mask] = 0
    if not was_numpy:
        return out
    _blank_origin(img)
    res = out.cpu().numpy()
    # the reference indexes the image with every coordinate its mask lets through: raise where it would (see _warp, rwh.h)
    ih_, iw_ = int(img.shape[0]), int(img.shape[1])
    if convert == 'nn':
        xi, yi = (zx + 0.5).to(torch.int64), (zy + 0.5).to(torch.int64)
        u = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1) & ~torch.isnan(zx) & ~torch.isnan(zy)
        bits = (1 if bool((u & (xi > iw_ - 1)).any()) else 0) | (2 if bool((u & (yi > ih_ - 1)).any()) else 0)
    else:
        u = ~((zx > w - 1) | (zx < 0) | (zy > h - 1) | (zy < 0))
        nan = u & (torch.isnan(zx) | torch.isnan(zy))
        fin = u & ~nan
        bits = (4 if bool(nan.any()) else 0) | (1 if bool((fin & (zx.floor() + 1 > iw_ - 1)).any()) else 0) | \
               (2 if bool((fin & (zy.floor() + 1 > ih_ - 1)).any()) else 0)
    if bits:
        kernels.raise_like_reference(bits, (ih_, iw_))
    return res if (convert == 'bilinear' or res.dtype == np_dtype) else res.astype(np_dtype)


def nearestNeighbor(z_t, img, h, w, mh, mw):
    """homography.py:108-121 on caller-computed coordinates z_t (3 x N, dehomogenised): (z_t + 0.5) truncated to int32,
    mask on the integers, gather; returns mh x mw x C in the image's dtype."""
    return _sample(z_t, img, h, w, mh, mw, 'nn')


def bilinear(z_t, img, h, w, mh, mw):
    """homography.py:123-138 on caller-computed coordinates: mask on the float64 coordinates, truncation, float64 lerps;
    returns mh x mw x C float64."""
    return _sample(z_t, img, h, w, mh, mw, 'bilinear')


convertfunc = {'nn': nearestNeighbor, 'bilinear': bilinear}


def transformImage(img, u, v, box=None, method='bilinear'):
    """Homography from 4 corner pairs + warp + uint8 + crop (homography.py:211-228).
    u, v: 3 x 4 homogeneous corners; `box=(h,w)` selects the scanner's fixed-resolution mode.
    The uint8 truncation is fused into the kernel (dst_dtype U8)."""
    u = np.asarray(u)
    v = np.asarray(v)
    H = calcHomographyLinear(u.T[:, :2], v.T[:, :2])
    if box is None:
        imgn, mx, my = _wrap_perspective(img, H, method, 0, True)
    else:
        h, w = box
        imgn = _warp(img, H, kernels.Grid(0, w, w, 0, h, h), (h, w), method, True)
        mx = my = 0
    if not _is_tensor(imgn) and imgn.dtype != np.uint8:
        imgn = imgn.astype(np.uint8)
    sx = int(v[0, 0] - mx); sy = int(v[1, 0] - my)
    ex = int(v[0, 2] - mx); ey = int(v[1, 2] - my)
    return imgn[sy:ey + 1, sx:ex + 1, :]


def transformImageH(img, H, method='bilinear'):
    """Warp by a given H (homography.py:230-242): uint8 for 3-channel results, 4-channel
    results stay floating point.  Returns (img, mx, my)."""
    if img.shape[2] == 3:
        imgn, mx, my = _wrap_perspective(img, H, method, 0, True)
        if not _is_tensor(imgn) and imgn.dtype != np.uint8:
            imgn = imgn.astype(np.uint8)
        return imgn, mx, my
    return _wrap_perspective(img, H, method, 0, False)


# ------------------------------------------------------------------------- alpha + compositor ----
class BLENDDIR(object):
    LEFT = 0
    RIGHT = 1
    TOP = 2
    DOWN = 3


def addAlpha(img, method="Rate", rate=0.2, direction=BLENDDIR.LEFT, alphaOnly=False):
    """Append (or return) an alpha plane, float32 (homography.py:250-286).  'Rate' is the only
    mode the reference finishes; its 'Gradient' branch (half-implemented, prints
    'not implement yet') is reproduced for the LEFT/RIGHT ramps it defines."""
    h, w, c = img.shape
    rate += 1e-10

    def ramp():
        if direction == BLENDDIR.RIGHT and alphaOnly:
            x = np.linspace(w - 1, 0, w); y = np.linspace(h - 1, 0, h)
        elif direction == BLENDDIR.LEFT:
            x = np.linspace(0, w - 1, w); y = np.linspace(0, h - 1, h)
        else:
            raise UnboundLocalError("local variable 'br' referenced before assignment")
        xx, yy = np.meshgrid(x, y)
        return (xx + yy) / (w + h) * 0.5

    if not alphaOnly:
        imgn = np.zeros((h, w, c + 1), dtype=np.float32)
        imgn[:, :, :c] = img
        if method == 'Rate':
            print(rate)
            imgn[:, :, c] = rate
        elif method == 'Gradient':
            imgn[:, :, c] = ramp()
            print('not implement yet')
        return imgn
    alpha = np.zeros((h, w, 1), dtype=np.float32)
    if method == 'Rate':
        print(rate)
        alpha[:, :, 0] = rate
    elif method == 'Gradient':
        alpha[:, :, 0] = ramp()
        print('not implement yet')
    return alpha


def _stitch_geometry(wt, ht, wq, hq, mx, my):
    """Paste rectangles and canvas size, homography.py:303-321."""
    tsx = 0; tsy = 0; tex = wt - 1; tey = ht - 1
    qsx = 0; qsy = 0; qex = wq - 1; qey = hq - 1
    if mx < 0 and my < 0:
        qsx = -mx; qsy = -my; qex = -mx + wq - 1; qey = -my + hq - 1
    elif mx < 0:
        tsy = my; tey = my + ht - 1
        qsx = -mx; qex = -mx + wq - 1
    elif my < 0:
        tsx = mx; tex = mx + wt - 1
        qsy = -my; qey = -my + hq - 1
    else:
        tsx = mx; tsy = my; tex = mx + wt - 1; tey = my + ht - 1
    return (tsx, tsy, tex, tey), (qsx, qsy, qex, qey), (max(tex + 1, qex + 1), max(tey + 1, qey + 1))


def _as_uint8_image(img, what):
    """stitchPanorama's kernels take uint8 RGB -- what cv2.imread hands the reference's own pipeline (ransac.py:236-243).  An image
    of another dtype whose values ARE uint8 values (a uint8 photograph converted to float) gives the reference the same canvas as its
    uint8 form -- the warp interpolates the same numbers, numpy's assignment into the uint8 canvas truncates the same way -- and is
    converted; anything else (fractions, values outside 0..255) is refused loudly rather than composited on the host."""
    if _is_tensor(img):
        import torch
        if img.dtype == torch.uint8:
            return img
        u = img.to(torch.uint8)
        # (int8 survives the round trip through uint8 for every value: a negative int8 is no uint8 value -- the blend reads it as
        #  a negative float)
        if bool((u.to(img.dtype) == img).all()) and not (img.dtype == torch.int8 and bool((img < 0).any())):
            return u
    else:
        a = np.asarray(img)
        if a.dtype == np.uint8:
            return img
        with np.errstate(invalid="ignore"):
            u = a.astype(np.uint8)
            if np.array_equal(u.astype(a.dtype), a) and not (a.dtype == np.int8 and (a < 0).any()):
                return u
    raise NotImplementedError("stitchPanorama: %s is not uint8 and holds values that are not uint8 values; the MI355X compositor takes "
                              "uint8 RGB images (the reference composites such images in numpy, homography.py:296-338)" % what)


# host arrays: below this many bytes (inputs + result) the plain upload / kernel / download (None: never pipelined).  Measured: a stitch
# gains from ~90 MB on (two 4K frames 3.0 -> 2.8 ms, two 12 MP photographs 4.2 -> 3.8, two 8K frames 9.4 -> 6.4, config 4's 8192 x 5464 pair
# 11.4 -> 7.7); a single warp only from 8K frames on (4.7 -> 3.8 ms; 4K: 1.5 ms plain against 2.4 -- two dozen tiles cost more than they hide)
PIPELINE_MIN_BYTES = 64 << 20
PIPELINE_WARP_FACTOR = 2.5         # a single warp is pipelined from PIPELINE_MIN_BYTES x this on


def _rows_needed(ih, xs, y_lo, y_hi, src_h):
    """Source rows [0, n) a warp samples for output rows y_lo .. y_hi (grid coordinates) and columns xs[0] .. xs[1]: the four
    corners through inv(H) -- a projective map with W > 0 on a convex region takes its extremes at the vertices -- plus the
    +1 tap and a margin; all rows when the horizon touches the region."""
    X = np.array([xs[0], xs[1], xs[0], xs[1]], dtype=np.float64)
    Y = np.array([y_lo, y_lo, y_hi, y_hi], dtype=np.float64)
    W = ih[2, 0] * X + ih[2, 1] * Y + ih[2, 2]
    if not (W > 0).all():
        return src_h
    ymax = float(np.max((ih[1, 0] * X + ih[1, 1] * Y + ih[1, 2]) / W))
    return src_h if not np.isfinite(ymax) else int(min(src_h, max(0.0, np.floor(ymax) + 3)))


def _pipeline(dev, uploads, need, bounds, compose, result, host):
    """The three PCIe legs of a host-array call overlapped (full duplex).  `uploads`: {tag: (flat uint8 host array, flat uint8
    device tensor)}; `need`[i]: {tag: bytes of that array row tile i reads}; `bounds`: the tiles' row boundaries in `result`
    (a device tensor whose rows go down into `host`, a page-locked tensor of the same shape); compose(i, r0, r1) enqueues tile
    i's kernel on the current stream.  The arrays go up interleaved in the order the tiles need them, a tile is composed as
    soon as its bytes have landed, finished tiles go down in 8 MB pieces issued BETWEEN the upload chunks: this runtime
    overlaps the two directions only when their copies alternate in the queues (two 256 MB copies on two streams: 9.4 ms; the
    same bytes as alternating 8 MB pieces: 5.9 ms)."""
    import torch
    from collections import deque
    cur = torch.cuda.current_stream(dev)
    comp, down = _xfer.side_stream(dev, "compose"), _xfer.side_stream(dev, "download")
    comp.wait_stream(cur)
    down.wait_stream(cur)
    nt = len(bounds) - 1
    size = {t: u[0].size for t, u in uploads.items()}
    need = [{t: min(int(n.get(t, 0)), size[t]) for t in uploads} for n in need]
    for i in range(1, nt):                      # tiles launch in order: what an earlier tile needed has arrived
        for t in uploads:
            need[i][t] = max(need[i][t], need[i - 1][t])
    C = _xfer.CHUNK if max(size.values()) >= (64 << 20) else (2 << 20)      # finer pieces for single frames
    tasks, sent = [], {t: 0 for t in uploads}

    def push(tag, upto):
        while sent[tag] < upto:
            m = min(C, size[tag] - sent[tag])
            tasks.append((uploads[tag][0], uploads[tag][1], sent[tag], m, tag))
            sent[tag] += m
    for i in range(nt):
        for t in uploads:
            push(t, need[i][t])
    for t in uploads:
        push(t, size[t])
    have = {t: 0 for t in uploads}
    last_ev = {t: None for t in uploads}
    state = {"next": 0}
    pieces = deque()                            # (row0, row1, event of the tile's kernel) still to go down
    row_bytes = result[0].numel() * result.element_size() if result.shape[0] else 1

    def launch_ready():
        while state["next"] < nt and all(have[t] >= need[state["next"]][t] for t in uploads):
            i = state["next"]
            r0, r1 = int(bounds[i]), int(bounds[i + 1])
            with torch.cuda.stream(comp):
                for ev in last_ev.values():
                    if ev is not None:
                        comp.wait_event(ev)
                compose(i, r0, r1)
                done = torch.cuda.Event()
                done.record(comp)
            step = max(1, C // row_bytes)
            for a0 in range(r0, r1, step):
                pieces.append((a0, min(r1, a0 + step), done))
            state["next"] += 1

    def send_down(n):
        with torch.cuda.stream(down):
            while n > 0 and pieces:
                a0, a1, done = pieces.popleft()
                down.wait_event(done)
                host[a0:a1].copy_(result[a0:a1], non_blocking=True)
                n -= 1

    def got(tag, nbytes, ev):
        have[tag] = nbytes
        last_ev[tag] = ev
        launch_ready()
        send_down(2)                            # two pieces down per chunk up: the directions alternate in the DMA queues
    _xfer.upload_tasks(tasks, dev, on_chunk=got, join=False)
    launch_ready()
    send_down(1 << 30)
    down.synchronize()
    cur.wait_stream(comp)
    cur.wait_stream(down)
    return host.numpy()


def _stitch_pipelined(imgQ, imgT, inv_h, mx, my, wt, ht, tsx, tsy, qsx, qsy, fh, fw, mode, blendrate, dev):
    """stitchPanorama from host arrays through `_pipeline`: the canvas by row tiles (rwh_stitch_panorama_rows, the exact kernel), a
    tile as soon as the rows of imgT it samples and the rows of imgQ it covers have arrived.  -> the canvas as a host array
    (page-locked, like _xfer.to_host's)."""
    import torch
    tT = np.ascontiguousarray(imgT).reshape(-1).view(np.uint8)
    tQ = np.ascontiguousarray(imgQ).reshape(-1).view(np.uint8)
    h, w = int(imgT.shape[0]), int(imgT.shape[1])
    hq, wq = int(imgQ.shape[0]), int(imgQ.shape[1])
    canvas = torch.empty((fh, fw, 3), dtype=torch.uint8, device=dev)
    try:
        host = torch.empty((fh, fw, 3), dtype=torch.uint8, pin_memory=True)
    except RuntimeError:          # no page-locked memory for the canvas: the caller takes the plain path
        return None
    t_flat = torch.empty(tT.size, dtype=torch.uint8, device=dev)
    q_flat = torch.empty(tQ.size, dtype=torch.uint8, device=dev)
    t_dev, q_dev = t_flat.view(h, w, 3), q_flat.view(hq, wq, 3)
    nt = int(max(1, min(24, fh // 128)))
    bounds = np.linspace(0, fh, nt + 1).astype(np.int64)
    ih = np.asarray(inv_h, dtype=np.float64)
    need = []
    for i in range(nt):
        r0, r1 = int(bounds[i]), int(bounds[i + 1])
        lo, hi = max(r0, tsy), min(r1, tsy + ht)
        rows_t = _rows_needed(ih, (mx, mx + wt - 1), my + lo - tsy, my + hi - 1 - tsy, h) if lo < hi else 0
        rows_q = int(max(0, min(hq, r1 - qsy))) if (r1 > qsy and r0 < qsy + hq) else 0
        need.append({"t": rows_t * w * 3, "q": rows_q * wq * 3})
    need[0]["t"] = max(need[0]["t"], 3)         # the first tile blanks texel (0,0) of imgT: behind the chunk that carries it

    def compose(i, r0, r1):
        kernels.stitch_panorama_rows(t_dev, q_dev, inv_h, (mx, my), (wt, ht), (tsx, tsy), (qsx, qsy), canvas, (r0, r1), mode, blendrate,
                                     zero_origin=(i == 0))
    return _pipeline(dev, {"t": (tT, t_flat), "q": (tQ, q_flat)}, need, bounds, compose, canvas, host)


def _warp_pipelined(a, inv_h, grid, bound_hw, convert, out_dtype, exact, dev):
    """One warp from a host array through `_pipeline`: output row tiles (rwh_warp_backward's row_begin / row_end), a tile as soon
    as the source rows it samples have arrived.  a: contiguous H x W x C host array as _host_src returns it.  -> host array."""
    import torch
    flat = a.reshape(-1).view(np.uint8)
    h, w, c = (int(v) for v in a.shape)
    t_dtype = _torch_dtype(a.dtype)
    s_flat = torch.empty(flat.size, dtype=torch.uint8, device=dev)
    src = s_flat.view(t_dtype).view(h, w, c)
    oh, ow = grid.out_h, grid.out_w
    result = torch.empty((oh, ow, c), dtype=out_dtype, device=dev)
    try:
        host = torch.empty((oh, ow, c), dtype=out_dtype, pin_memory=True)
    except RuntimeError:          # no page-locked memory for a result of this size: the caller takes the plain path
        return None
    nt = int(max(1, min(24, oh // 64)))
    bounds = np.linspace(0, oh, nt + 1).astype(np.int64)
    ih = np.asarray(inv_h, dtype=np.float64)
    row_b = w * c * a.itemsize

    def gy(r):
        return grid.y_last if r == oh - 1 else grid.y0 + r * grid.step_y
    need = [{"s": _rows_needed(ih, (grid.x0, grid.x_last), gy(int(bounds[i])), gy(int(bounds[i + 1]) - 1), h) * row_b} for i in range(nt)]
    need[0]["s"] = max(need[0]["s"], c * a.itemsize)      # the first tile blanks texel (0,0)

    def compose(i, r0, r1):
        kernels.warp_backward(src, inv_h, grid, bound_hw, convert, out_dtype, zero_origin=(i == 0), rows=(r0, r1), out=result[r0:r1], exact=exact)
    return _pipeline(dev, {"s": (flat, s_flat)}, need, bounds, compose, result, host)


def stitchPanorama(imgQ, imgT, H, method='bilinear', blending=False, blendrate=0.2):
    """Warp imgT by H and composite it with imgQ on a common canvas (homography.py:288-338).  `method` is ignored
    exactly as in the reference (always bilinear).

    ONE fused kernel (`rwh_stitch_panorama`): alpha plane, warp, paste / alpha blend per canvas pixel; nothing intermediate (RGBA
    float32 image, float64 warp, float32 canvas) is materialised.  `blending` False / 'Rate' / 'Gradient' / any other truthy value
    (for which the reference's addAlpha leaves the alpha plane at 0: blend mode 3) on uint8 RGB images -- or images of another
    dtype that hold uint8 values, converted.  numpy arrays in (or EXACT = True): the reference's float64 arithmetic, canvas
    bit-identical to the reference's; torch tensors in (or EXACT = False): the staged fast warp kernel with the compositor as its
    epilogue, canvas within 1 LSB.

    Every other input goes to the any-dtype compositor (`rwh_stitch_panorama_ex`, exact for numpy arrays and tensors alike): images
    of any numeric dtype (bool, int8 .. int64, uint8 .. uint64, float16 / 32 / 64), imgT with 3 or 4 channels, imgQ with 1, 3 or 4
    (paste: as many as imgT, or 1); canvas, exceptions (IndexError from the warp before a ValueError from a channel mismatch) and
    side effects on the caller's imgT as the reference's.  imgT with 1 or 2 channels raises the reference's IndexError.  Images
    with 5 or more channels and non-numeric dtypes (bfloat16 tensors among them: numpy has no such type) raise
    NotImplementedError."""
    import torch
    paste = not blending                                     # homography.py:298 / 322: `if blending:`
    u8 = None
    if imgQ.shape[2] == 3 and imgT.shape[2] == 3:
        try:
            u8 = _as_uint8_image(imgQ, "imgQ"), _as_uint8_image(imgT, "imgT")
        except NotImplementedError:
            pass
    if u8 is None:                # not uint8 RGB (nor uint8 values in 3 channels): the any-dtype compositor
        return _stitch_any(imgQ, imgT, H, blending, blendrate)
    tens = _is_tensor(imgQ) or _is_tensor(imgT)
    caller_imgT = imgT
    imgQ, imgT = u8
    if blending == 'Rate':
        print(blendrate + 1e-10)   # addAlpha prints the rate it stores (homography.py:257)
    elif blending == 'Gradient':
        print('not implement yet')  # homography.py:266
    h, w, _ = imgT.shape
    mx, my, wt, ht = _bounds(h, w, H, 0)
    if wt <= 0 or ht <= 0:
        raise ValueError("Number of samples, %d, must be non-negative." % min(wt, ht))
    hq, wq, _ = imgQ.shape
    (tsx, tsy, tex, tey), (qsx, qsy, qex, qey), (fw, fh) = _stitch_geometry(wt, ht, wq, hq, mx, my)
    inv_h = np.linalg.inv(np.asarray(H, dtype=np.float64))
    dev = _lib.require_gpu()
    exact = (not tens) if EXACT is None else bool(EXACT)    # numpy in: the bit-identical float64 kernel; tensors in: the fast one
    # 'Gradient': the alpha ramp, exact kernel only; any other truthy value: addAlpha leaves the alpha plane at 0 (mode 3)
    mode = 0 if paste else 1 if blending == 'Rate' else 2 if blending == 'Gradient' else 3
    # large host arrays through the exact kernel: uploads, composition by row tiles and the download overlapped (_stitch_pipelined)
    pipelined = (not tens) and exact and PIPELINE_MIN_BYTES is not None and fh * fw * 3 <= _xfer.PINNED_RESULT_MAX and \
        (np.asarray(imgT).nbytes + np.asarray(imgQ).nbytes + fh * fw * 3) >= PIPELINE_MIN_BYTES
    if tens:
        t_dev = imgT.to(dev).contiguous()
        q_dev = imgQ.to(dev).contiguous()
        if blending:
            t_dev = t_dev.clone()      # addAlpha copies: the caller's imgT keeps its texel (0,0)
    elif not pipelined:
        t_dev = _xfer.to_device(imgT, dev)      # staged through page-locked buffers by several host threads (_xfer)
        q_dev = _xfer.to_device(imgQ, dev)
    # (numpy in: transformImageH's bilinear warp of imgT raises IndexError in the reference where it indexes past the image)
    flag = None if tens else kernels.warp_index_check((h, w), inv_h, kernels.Grid(mx, mx + wt - 1, wt, my, my + ht - 1, ht), (h, w), "bilinear", dev)
    if pipelined:
        res = _stitch_pipelined(imgQ, imgT, inv_h, mx, my, wt, ht, tsx, tsy, qsx, qsy, fh, fw, mode, blendrate, dev)
        if res is not None:
            if not blending:
                _blank_origin(caller_imgT)
            bits = int(flag.item())
            if bits:
                kernels.raise_like_reference(bits, (h, w))
            return res
        t_dev = _xfer.to_device(imgT, dev)      # (no page-locked memory for the canvas: upload / kernel / download)
        q_dev = _xfer.to_device(imgQ, dev)
    out = kernels.stitch_panorama(t_dev, q_dev, inv_h, (mx, my), (wt, ht), (tsx, tsy), (qsx, qsy), (fh, fw),
                                  mode, blendrate, zero_origin=True, fast=not exact)
    if tens:
        return out
    if not blending:
        _blank_origin(caller_imgT)     # transformImageH -> bilinear blanks the caller's texel (0,0) in the paste path
    res = _xfer.to_host(out)
    bits = int(flag.item())
    if bits:
        kernels.raise_like_reference(bits, (h, w))
    return res


# ------------------------------------------------------------------- sequences of N images ----
def _sequence_canvas(shapes, Gs, anchor):
    """Rectangles, canvas and default order of the sequence rule (include/rwh.h) for given G_i: -> (rects [(mx, my, wt, ht)],
    (ox, oy), (fh, fw), order), or the rule's ValueError."""
    n = len(shapes)
    rects = []
    for i, (shape, G) in enumerate(zip(shapes, Gs)):
        h, w = int(shape[0]), int(shape[1])
        if h < 2 or w < 2:
            raise ValueError("sequence: image %d is %d x %d; sides of 2 at least" % (i, h, w))
        if i == anchor:
            rects.append((0, 0, w, h))
            continue
        with np.errstate(all="ignore"):
            p = np.asarray(G, dtype=np.float64) @ np.array([[0, w - 1, w - 1, 0], [0, 0, h - 1, h - 1], [1., 1, 1, 1]])
            p = p[:2] / p[2]
        if not (np.isfinite(G).all() and np.isfinite(p).all() and np.abs(p).max() < 2.0 ** 31):
            raise ValueError("sequence: image %d has a homography or a corner in the anchor's frame that is not finite" % i)
        mx, my, wt, ht = _bounds(h, w, G, 0)
        if wt <= 0 or ht <= 0:
            raise ValueError("sequence: image %d warps to an empty rectangle (%d x %d)" % (i, wt, ht))
        rects.append((mx, my, wt, ht))
    ox, oy = min(r[0] for r in rects), min(r[1] for r in rects)
    fw, fh = max(r[0] + r[2] for r in rects) - ox, max(r[1] + r[3] for r in rects) - oy
    if fw > 65535 or fh > 65535 or fw * fh * 3 > 2 ** 31 - 1:
        raise ValueError("sequence: a %d x %d canvas; sides of at most 65535 and at most 2^31 - 1 bytes (does a horizon cross an image?)"
                         % (fh, fw))
    order = sorted(range(n), key=lambda i: (abs(i - anchor), i))
    return rects, (ox, oy), (fh, fw), order


def _check_count(n, anchor):
    if not 1 <= n <= _lib.RWH_SEQ_MAX_IMAGES:
        raise ValueError("sequence: %d images; 1 .. %d are taken" % (n, _lib.RWH_SEQ_MAX_IMAGES))
    if not (isinstance(anchor, (int, np.integer)) and 0 <= anchor < n):
        raise ValueError("sequence: anchor %r outside 0 .. %d" % (anchor, n - 1))


PROJECTIONS = ("cylindrical", "spherical")


def _check_projection(who, projection, focal):
    """ValueError unless (projection, focal) is (None, None) or a known surface with a finite focal > 0."""
    if projection is None:
        if focal is not None:
            raise ValueError("%s: focal=%r without a projection" % (who, focal))
        return
    if not (isinstance(projection, str) and projection in PROJECTIONS):
        raise ValueError("%s: projection=%r; None, 'cylindrical' or 'spherical'" % (who, projection))
    if focal is None:
        raise ValueError("%s: projection=%r takes a focal length in pixels" % (who, projection))
    if isinstance(focal, (bool, str)) or not isinstance(focal, (int, float, np.integer, np.floating)) or not (np.isfinite(focal) and focal > 0):
        raise ValueError("%s: focal=%r; finite and > 0" % (who, focal))


def _camera(shape, focal):
    """K of the projection rule: the focal length and the centre of the anchor's image."""
    return np.array([[float(focal), 0.0, (int(shape[1]) - 1) / 2.0], [0.0, float(focal), (int(shape[0]) - 1) / 2.0], [0.0, 0.0, 1.0]])


def _surface(rays, projection, focal):
    """Surface points (u, s) of rays [3, n] by the projection rule."""
    theta = np.arctan2(rays[0], rays[2])
    hyp = np.hypot(rays[0], rays[2])
    t = rays[1] / hyp if projection == "cylindrical" else np.arctan2(rays[1], hyp)
    return focal * theta, focal * t


def _perimeter(h, w):
    """The perimeter pixels of an h x w image in order, [3, n] homogeneous; the loop closes from the last to the first."""
    xs, ys = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    x = np.concatenate([xs[:-1], np.full(h - 1, w - 1.0), xs[:0:-1], np.zeros(h - 1)])
    y = np.concatenate([np.zeros(w - 1), ys[:-1], np.full(w - 1, h - 1.0), ys[:0:-1]])
    return np.stack([x, y, np.ones_like(x)])


def _oriented(Gs):
    """G_i * sign(det G_i) of the projection rule; ValueError for a zero or non-finite determinant."""
    out = []
    for i, G in enumerate(Gs):
        G = np.asarray(G, dtype=np.float64)
        with np.errstate(all="ignore"):
            det = np.linalg.det(G) if np.isfinite(G).all() else np.nan
        if not np.isfinite(det) or det == 0.0:
            raise ValueError("sequence: image %d has a homography whose determinant is zero or not finite" % i)
        out.append(G if det > 0 else -G)
    return np.stack(out)


def _projected_canvas(shapes, Gs, anchor, projection, focal):
    """Rectangles (in surface pixels), canvas and default order of the projection rule (include/rwh.h) for oriented G_i: ->
    (rects, (ox, oy), (fh, fw), order), or the rule's ValueError."""
    n = len(shapes)
    kinv = np.linalg.inv(_camera(shapes[anchor], focal))
    rects = []
    for i, (shape, G) in enumerate(zip(shapes, Gs)):
        h, w = int(shape[0]), int(shape[1])
        if h < 2 or w < 2:
            raise ValueError("sequence: image %d is %d x %d; sides of 2 at least" % (i, h, w))
        with np.errstate(all="ignore"):
            rays = kinv @ (G @ _perimeter(h, w))
            u, v = _surface(rays, projection, float(focal))
            theta = u / float(focal)
        if not (np.isfinite(u).all() and np.isfinite(v).all() and max(np.abs(u).max(), np.abs(v).max()) < 2.0 ** 30):
            raise ValueError("sequence: image %d has a perimeter point on the %s surface that is not finite" % (i, projection))
        step = np.diff(np.append(theta, theta[0]))
        wrapped = (step + np.pi) % (2.0 * np.pi) - np.pi
        if int(np.rint(wrapped.sum() / (2.0 * np.pi))) != 0:
            raise ValueError("sequence: image %d contains a pole of the %s surface" % (i, projection))
        if (np.abs(step) >= np.pi).any():
            raise ValueError("sequence: image %d straddles the seam behind the anchor (360-degree wrap-around is not taken)" % i)
        mx, my = int(np.floor(u.min())) - 1, int(np.floor(v.min())) - 1
        rects.append((mx, my, int(np.ceil(u.max())) + 1 - mx + 1, int(np.ceil(v.max())) + 1 - my + 1))
    ox, oy = min(r[0] for r in rects), min(r[1] for r in rects)
    fw, fh = max(r[0] + r[2] for r in rects) - ox, max(r[1] + r[3] for r in rects) - oy
    if fw > 65535 or fh > 65535 or fw * fh * 3 > 2 ** 31 - 1:
        raise ValueError("sequence: a %d x %d canvas; sides of at most 65535 and at most 2^31 - 1 bytes" % (fh, fw))
    order = sorted(range(n), key=lambda i: (abs(i - anchor), i))
    return rects, (ox, oy), (fh, fw), order


RING_TILE, RING_MAX_PERIOD = 256, 65280


def sequence_period(focal):
    """The default period of the ring rule (include/rwh.h) for a focal length in pixels: P = 256 * max(1, rint(2 pi f / 256)), the
    multiple of 256 nearest the circumference of a cylinder of radius f.  ValueError: a focal that is not finite and > 0, a period
    above 65280."""
    _check_projection("sequence_period", PROJECTIONS[0], focal)
    period = RING_TILE * max(1, int(np.rint(2.0 * np.pi * float(focal) / RING_TILE)))
    if period > RING_MAX_PERIOD:
        raise ValueError("sequence_period: focal=%r gives a period of %d columns; at most %d" % (focal, period, RING_MAX_PERIOD))
    return period


def _check_wrap(who, wrap, projection, focal):
    """The period of a `wrap=` argument, None for wrap=False; ValueError for a wrap without a projection or one that is neither a bool
    nor a positive multiple of 256 up to 65280.  (projection, focal) have passed `_check_projection`."""
    if wrap is False:
        return None
    if wrap is not True and not (isinstance(wrap, (int, np.integer)) and not isinstance(wrap, (bool, np.bool_))
                                 and 0 < wrap <= RING_MAX_PERIOD and wrap % RING_TILE == 0):
        raise ValueError("%s: wrap=%r; False, True or a period in columns, a positive multiple of %d up to %d"
                         % (who, wrap, RING_TILE, RING_MAX_PERIOD))
    if projection is None:
        raise ValueError("%s: wrap=%r without a projection" % (who, wrap))
    return sequence_period(focal) if wrap is True else int(wrap)


def _ring_canvas(shapes, Gs, anchor, projection, focal, period):
    """Rectangles (in UNWRAPPED surface pixels: a rectangle may start left of -P / 2 or end right of P / 2), canvas and default order
    of the ring rule (include/rwh.h) for oriented G_i and the period P: -> (rects, (-P / 2, oy), (fh, P), order), or the rule's
    ValueError."""
    n = len(shapes)
    rho = period / (2.0 * np.pi)
    kinv = np.linalg.inv(_camera(shapes[anchor], focal))
    rects = []
    for i, (shape, G) in enumerate(zip(shapes, Gs)):
        h, w = int(shape[0]), int(shape[1])
        if h < 2 or w < 2:
            raise ValueError("sequence: image %d is %d x %d; sides of 2 at least" % (i, h, w))
        with np.errstate(all="ignore"):
            rays = kinv @ (G @ _perimeter(h, w))
            theta = np.arctan2(rays[0], rays[2])
            v = _surface(rays, projection, rho)[1]
        if not (np.isfinite(theta).all() and np.isfinite(v).all() and np.abs(v).max() < 2.0 ** 30):
            raise ValueError("sequence: image %d has a perimeter point on the %s surface that is not finite" % (i, projection))
        step = np.diff(np.append(theta, theta[0]))
        wrapped = (step + np.pi) % (2.0 * np.pi) - np.pi
        if int(np.rint(wrapped.sum() / (2.0 * np.pi))) != 0:
            raise ValueError("sequence: image %d contains a pole of the %s surface" % (i, projection))
        u = rho * np.cumsum(np.append(theta[0], wrapped[:-1]))
        lo, my = int(np.floor(u.min())) - 1, int(np.floor(v.min())) - 1
        rects.append((lo, my, min(int(np.ceil(u.max())) + 1 - lo + 1, period), int(np.ceil(v.max())) + 1 - my + 1))
    oy = min(r[1] for r in rects)
    fh = max(r[1] + r[3] for r in rects) - oy
    if fh > 65535 or period * fh * 3 > 2 ** 31 - 1:
        raise ValueError("sequence: a %d x %d canvas; sides of at most 65535 and at most 2^31 - 1 bytes" % (fh, period))
    order = sorted(range(n), key=lambda i: (abs(i - anchor), i))
    return rects, (-(period // 2), oy), (fh, period), order


def _curved_canvas(shapes, Gs, anchor, projection, focal, period):
    """`_projected_canvas`, or with a period `_ring_canvas`."""
    if period is None:
        return _projected_canvas(shapes, Gs, anchor, projection, focal)
    return _ring_canvas(shapes, Gs, anchor, projection, focal, period)


def sequence_ray_tables(projection, focal, origin, size):
    """The two ray tables of the projection rule (include/rwh.h) for a canvas of size (fh, fw) whose pixel (0, 0) is surface point
    origin = (ox, oy): -> (col float64 [fw, 2], row float64 [fh, 2]); col[cx] = (sin(u / f), cos(u / f)) with u = ox + cx,
    row[cy] = (s / f, 1.0) on the cylinder and (sin(s / f), cos(s / f)) on the sphere with s = oy + cy.  Pure numpy: the compositor,
    its host twin and a restatement all read these numbers, none of them calls a transcendental function."""
    _check_projection("sequence_ray_tables", projection, focal)
    if projection is None:
        raise ValueError("sequence_ray_tables: projection=None has no tables")
    f = float(focal)
    u = (int(origin[0]) + np.arange(int(size[1]), dtype=np.float64)) / f
    t = (int(origin[1]) + np.arange(int(size[0]), dtype=np.float64)) / f
    col = np.stack([np.sin(u), np.cos(u)], axis=1)
    row = np.stack([t, np.ones_like(t)], axis=1) if projection == "cylindrical" else np.stack([np.sin(t), np.cos(t)], axis=1)
    return np.ascontiguousarray(col), np.ascontiguousarray(row)


def sequence_focal(shapes, Hs, pairs=None):
    """A focal length in pixels from the pairwise homographies of a rotating camera, for `projection=`; pure numpy.

    shapes: N image shapes; Hs: N - 1 matrices as `sequence_plan`'s; or, with pairs = [(s, d), ...] (the edges of a pair graph,
    as `sequence_graph`'s), one matrix per pair, Hs[e] mapping image s into image d -- pairs=None is [(i + 1, i)].  With the principal points moved to the image centres,
    Hc = inv(C_i) @ H @ C_{i+1} (entries h0 .. h8) is K_i R inv(K_{i+1}) up to scale, and the orthonormality of R's rows and
    columns (Szeliski & Shum 1997; what OpenCV's stitcher uses) gives f0^2 as one of -h2 h5 / (h0 h3 + h1 h4) and
    (h5^2 - h2^2) / (h0^2 + h1^2 - h3^2 - h4^2), f1^2 as one of -(h0 h1 + h3 h4) / (h6 h7) and
    (h0^2 + h3^2 - h1^2 - h4^2) / (h7^2 - h6^2), in each case the candidate whose denominator is larger in magnitude.  A pair
    counts when both are finite and > 0 and gives sqrt(f0 f1) (the root of the product of the two focal lengths); the result is
    the median over the pairs.  ValueError: a wrong number of Hs, no pair that counts."""
    n = len(shapes)
    Hs = [np.asarray(H, dtype=np.float64) for H in Hs]
    if pairs is None:
        if n < 1 or len(Hs) != n - 1 or any(H.shape != (3, 3) for H in Hs):
            raise ValueError("sequence_focal: %d images take %d 3 x 3 homographies, got %d" % (n, n - 1, len(Hs)))
        pairs = [(i + 1, i) for i in range(n - 1)]
    else:
        pairs = _check_pairs("sequence_focal", n, pairs)
        if len(Hs) != len(pairs) or any(H.shape != (3, 3) for H in Hs):
            raise ValueError("sequence_focal: %d pairs take %d 3 x 3 homographies, got %d" % (len(pairs), len(pairs), len(Hs)))

    def centre(shape, sign):
        return np.array([[1.0, 0.0, sign * (int(shape[1]) - 1) / 2.0], [0.0, 1.0, sign * (int(shape[0]) - 1) / 2.0], [0.0, 0.0, 1.0]])

    def pick(cands):
        num, den = max(cands, key=lambda c: abs(c[1]))
        return num / den

    found = []
    for (src, dst), H in zip(pairs, Hs):
        with np.errstate(all="ignore"):
            h = (centre(shapes[dst], -1.0) @ H @ centre(shapes[src], 1.0)).reshape(9)
            f0 = pick([(-h[2] * h[5], h[0] * h[3] + h[1] * h[4]), (h[5] ** 2 - h[2] ** 2, h[0] ** 2 + h[1] ** 2 - h[3] ** 2 - h[4] ** 2)])
            f1 = pick([(-(h[0] * h[1] + h[3] * h[4]), h[6] * h[7]), (h[0] ** 2 + h[3] ** 2 - h[1] ** 2 - h[4] ** 2, h[7] ** 2 - h[6] ** 2)])
        if np.isfinite(f0) and np.isfinite(f1) and f0 > 0 and f1 > 0:
            found.append(float(np.sqrt(np.sqrt(f0) * np.sqrt(f1))))
    if not found:
        raise ValueError("sequence_focal: no pair of images gives a focal length (%d pairs)" % len(Hs))
    return float(np.median(found))


def sequence_plan(shapes, Hs, anchor=0, projection=None, focal=None, wrap=False):
    """The geometry of a sequence panorama from its pairwise homographies; pure numpy, no GPU.

    shapes: N image shapes (h, w[, c]); Hs: N - 1 matrices, Hs[i] maps image i+1 into image i -- what
    `stitching(trainImg=images[i+1], queryImg=images[i])` estimates.  C_0 = I, C_{i+1} = C_i @ Hs[i]; G_i = inv(C_a) @ C_i maps
    image i into the anchor's frame, G_a the identity exactly.  Returns (Gs float64 [N, 3, 3], rects [(mx, my, wt, ht)] in the
    anchor's frame, (ox, oy), (fh, fw), order): the rectangles, the canvas and the default paste order (the anchor first, then
    increasing |i - anchor|, the lower index on ties) of the sequence rule (include/rwh.h).  ValueError: N outside 1 .. 64, a wrong
    number of Hs, a non-finite G_i or corner, an empty rectangle, a canvas side above 65535 or a canvas above 2^31 - 1 bytes.

    projection: None -- the anchor's image plane, as above; "cylindrical" or "spherical" -- the canvas is that surface about the
    anchor's camera, with `focal` (pixels, finite and > 0) its radius (the projection rule of include/rwh.h).  The 5-tuple is the
    same, with Gs each multiplied by the sign of its determinant and rectangles and origin in SURFACE pixels.  ValueError in
    addition: an unknown projection, one without the other of projection and focal, a determinant that is zero or not finite, a
    perimeter point that is not finite, an image that straddles the seam behind the anchor or contains a pole.

    wrap: False -- as above; True or a period P in columns (a positive multiple of 256 up to 65280; True is `sequence_period(focal)`)
    -- the canvas closes the circle (the ring rule of include/rwh.h): the surface has the radius P / (2 pi) while the cameras keep
    `focal`, the rectangles are in UNWRAPPED surface pixels (one may pass -P / 2 or P / 2; no image is refused for lying across the
    seam), the origin is (-P / 2, oy) and the size (fh, P).  ValueError in addition: wrap without a projection, a wrap that is
    neither a bool nor such a period."""
    n = len(shapes)
    _check_count(n, anchor)
    _check_projection("sequence_plan", projection, focal)
    period = _check_wrap("sequence_plan", wrap, projection, focal)
    Hs = [np.asarray(H, dtype=np.float64) for H in Hs]
    if len(Hs) != n - 1 or any(H.shape != (3, 3) for H in Hs):
        raise ValueError("sequence: %d images take %d 3 x 3 homographies, got %d" % (n, n - 1, len(Hs)))
    with np.errstate(all="ignore"):
        C = [np.eye(3)]
        for H in Hs:
            C.append(C[-1] @ H)
        if not all(np.isfinite(c).all() for c in C):
            raise ValueError("sequence: a chained homography is not finite")
        inv_a = np.linalg.inv(C[anchor])
        Gs = np.stack([inv_a @ c for c in C])
    Gs[anchor] = np.eye(3)
    if projection is not None:
        Gs = _oriented(Gs)
        rects, origin, size, order = _curved_canvas(shapes, Gs, anchor, projection, focal, period)
        return Gs, rects, origin, size, order
    rects, origin, size, order = _sequence_canvas(shapes, Gs, anchor)
    return Gs, rects, origin, size, order


# ------------------------------------------------------ registration over a pair graph (the bundle rule) ----
# Conventions, not measured optima: the acceptance test of Brown & Lowe 2007, eq. 13 (an edge counts when its inliers exceed
# alpha + beta * matches); Levenberg-Marquardt starting at lambda = 1e-3, a factor of 10 down on an accepted step and up on a
# rejected one, given up above 1e12, ended by an accepted step that lowers the cost by less than 1e-12 of it.
GRAPH_ALPHA, GRAPH_BETA = 8.0, 0.3
ADJUST_LAMBDA0, ADJUST_LAMBDA_MAX, ADJUST_LAMBDA_FACTOR, ADJUST_REL_STOP = 1e-3, 1e12, 10.0, 1e-12


def _check_pairs(who, n, pairs):
    """[(s, d)] as ints, or ValueError: an end outside 0 .. n - 1, s == d, a pair that is not two integers, too many pairs."""
    out = []
    try:
        for pr in pairs:
            s, d = pr
            if isinstance(s, (bool, np.bool_)) or isinstance(d, (bool, np.bool_)) or int(s) != s or int(d) != d:
                raise TypeError
            out.append((int(s), int(d)))
    except (TypeError, ValueError):
        raise ValueError("%s: pairs=%r; a list of (s, d) image indices" % (who, pairs)) from None
    for s, d in out:
        if not (0 <= s < n and 0 <= d < n) or s == d:
            raise ValueError("%s: pair (%d, %d); two different images of 0 .. %d" % (who, s, d, n - 1))
    if len(out) > _lib.RWH_BUNDLE_MAX_EDGES:
        raise ValueError("%s: %d pairs; at most %d" % (who, len(out), _lib.RWH_BUNDLE_MAX_EDGES))
    return out


def sequence_graph(n, pairs, Hs, sizes, inliers, anchor=0):
    """The pair graph of a sequence and its initialisation along a spanning tree; pure numpy, no GPU.

    n: images; pairs: E edges (s, d); Hs[e]: 3 x 3, maps image s into image d (what `run_batch` estimates for the correspondences
    `match_batch` makes of (features of s, features of d)), or None; sizes[e], inliers[e]: matches and RANSAC inliers of the edge.
    An edge is ACCEPTED when inliers > 8 + 0.3 * sizes (Brown & Lowe 2007, eq. 13: alpha = 8 and beta = 0.3 are the paper's
    conventions, not measured here) and its H is finite.  The tree grows from the anchor: of the accepted edges that join an
    image of the tree to one outside it, the one with the most inliers is taken, on ties the lower (s, d); the new image's map is
    G_child = G_parent @ H when the child is s, G_parent @ inv(H) when it is d.  G_anchor is the identity exactly.

    Returns (Gs float64 [n, 3, 3], accepted bool [E], tree [(parent, child, e)] in the order taken).  With anchor 0 and
    pairs = [(i + 1, i)], all accepted, Gs is `sequence_plan`'s bit for bit.  ValueError: n or anchor as `sequence_plan`'s, a bad
    pair, lists of other lengths, an H of another shape, an image the accepted edges do not connect to the anchor (named)."""
    _check_count(n, anchor)
    pairs = _check_pairs("sequence_graph", n, pairs)
    E = len(pairs)
    if not (len(Hs) == len(sizes) == len(inliers) == E):
        raise ValueError("sequence_graph: %d pairs take %d homographies, sizes and inlier counts" % (E, E))
    mats, accepted = [], np.zeros(E, dtype=bool)
    for e, H in enumerate(Hs):
        H = None if H is None else np.asarray(H, dtype=np.float64)
        if H is not None and H.shape != (3, 3):
            raise ValueError("sequence_graph: pair %d has a homography of shape %s" % (e, H.shape))
        mats.append(H)
        accepted[e] = H is not None and bool(np.isfinite(H).all()) and float(inliers[e]) > GRAPH_ALPHA + GRAPH_BETA * float(sizes[e])
    Gs = np.zeros((n, 3, 3))
    Gs[anchor] = np.eye(3)
    inside, tree = {anchor}, []
    while len(inside) < n:
        best = None
        for e, (s, d) in enumerate(pairs):
            if accepted[e] and ((s in inside) != (d in inside)):
                key = (-int(inliers[e]), s, d, e)
                if best is None or key < best:
                    best = key
        if best is None:
            missing = [i for i in range(n) if i not in inside]
            raise ValueError("sequence_graph: image %d is not connected to the anchor (%d) by accepted pairs%s"
                             % (missing[0], anchor, "" if len(missing) == 1 else "; nor are %s" % missing[1:]))
        e = best[3]
        s, d = pairs[e]
        with np.errstate(all="ignore"):
            if d in inside:
                parent, child, G = d, s, Gs[d] @ mats[e]
            else:
                parent, child, G = s, d, Gs[s] @ np.linalg.inv(mats[e])
        if not np.isfinite(G).all():
            raise ValueError("sequence_graph: image %d gets a map that is not finite (pair %d)" % (child, e))
        Gs[child] = G
        inside.add(child)
        tree.append((parent, child, e))
    return Gs, accepted, tree


def _bundle_transfers(Gs, pairs):
    """T_e = inv(G_d) @ G_s, divided by its largest |entry| (the bundle rule): float64 [E, 3, 3]."""
    inv = np.linalg.inv(Gs)
    T = np.stack([inv[d] @ Gs[s] for s, d in pairs])
    return T / np.abs(T).reshape(len(pairs), 9).max(axis=1)[:, None, None]


def _delta_matrix(delta):
    """I + D(delta): delta_0 .. delta_7 in row-major order, D[2][2] = 0."""
    return np.eye(3) + np.append(delta, 0.0).reshape(3, 3)


def _adjust_problem(who, rule, pairs, matches, masks, on):
    """What `sequence_adjust` and `sequence_adjust_cameras` make of their matches and masks, once: sizes, offsets and mask words
    checked, and everything put where `on` says -> blocks(records): the (blocks, count, status) of every edge for the rule's
    per-edge records, from `kernels.<rule>_blocks` on the device or `kernels.host_<rule>_blocks` on the host.  rule: "bundle" or
    "camera"; the entry points are looked up in `kernels` at every call."""
    from .features import DeviceProblems
    E = len(pairs)
    on_dev = isinstance(matches, DeviceProblems)
    sizes = list(matches.sizes) if on_dev else [int(np.asarray(a).reshape(-1, 2).shape[0]) for a, _ in matches]
    if len(sizes) != E:
        raise ValueError("%s: %d pairs take %d sets of matches, got %d" % (who, E, E, len(sizes)))
    offsets = np.zeros(E + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(sizes)
    words = max((max(sizes) + 63) // 64, 1)
    tensor_masks = masks is not None and _is_tensor(masks)
    if masks is None:
        masks = np.full((E, words), -1, dtype=np.int64)
    elif not tensor_masks:
        masks = np.ascontiguousarray(masks)
        if masks.dtype not in (np.dtype(np.uint64), np.dtype(np.int64)) or masks.ndim != 2:
            raise ValueError("%s: masks takes [E, words] uint64 or int64 words" % who)
        masks = masks.view(np.int64)
    if tuple(masks.shape)[0] != E or len(masks.shape) != 2 or masks.shape[1] < 1:
        raise ValueError("%s: masks of shape %s for %d pairs" % (who, tuple(masks.shape), E))
    if on == "device":
        import torch
        dev = _lib.require_gpu()
        if on_dev:
            pa, pb = matches.pts_a, matches.pts_b
        else:
            pa = torch.from_numpy(np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1, 2) for a, _ in matches])).to(dev)
            pb = torch.from_numpy(np.concatenate([np.asarray(b, dtype=np.float32).reshape(-1, 2) for _, b in matches])).to(dev)
        off_dev = torch.from_numpy(offsets).to(dev)
        m_dev = (masks if tensor_masks else torch.from_numpy(masks)).to(dev).to(torch.int64).contiguous()

        def blocks(records):
            packed = getattr(kernels, rule + "_blocks")(pa, pb, off_dev, m_dev, records)
            return getattr(kernels, rule + "_split")(packed.cpu().numpy())
    else:
        if on_dev:
            pa, pb = matches.pts_a.cpu().numpy(), matches.pts_b.cpu().numpy()
        else:
            pa = np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1, 2) for a, _ in matches])
            pb = np.concatenate([np.asarray(b, dtype=np.float32).reshape(-1, 2) for _, b in matches])
        m_host = masks.cpu().numpy() if tensor_masks else masks

        def blocks(records):
            return getattr(kernels, "host_%s_blocks" % rule)(pa, pb, offsets, m_host, records)
    return blocks


def _levenberg(who, pairs, state, max_iters, info, evaluate, step, candidate, singular):
    """The Levenberg-Marquardt loop of both registration rules -> the state of the last accepted step (`state` itself if none).

    A rule supplies evaluate(state) -> (blocks, count, status) of every edge at a state, and the three things in which the loops
    differ:
      candidate(state, delta) -> the state the step leads to, or None for one that is refused without an evaluation;
      singular: what a step whose system is singular means after the first step tried (on the first it raises) -- "raise", or
        "reject" (a rejected step, lambda goes up);
      step(blocks, lam) -> (delta, status): its `kernels.host_<rule>_step` call.
    The rest is written once: the start's two refusals, lambda from ADJUST_LAMBDA0 by ADJUST_LAMBDA_FACTOR up to ADJUST_LAMBDA_MAX,
    a step accepted iff its candidate's cost is strictly lower and no edge reports RWH_BUNDLE_BEHIND, the end after `max_iters`
    accepted steps or on one that lowers the cost by less than ADJUST_REL_STOP of it, and `info`."""
    blocks, _, status = evaluate(state)
    if (status != _lib.RWH_BUNDLE_OK).any():
        e = int(np.nonzero(status != _lib.RWH_BUNDLE_OK)[0][0])
        raise ValueError("%s: pair %d (images %d and %d) has an inlier behind the camera at the start" % ((who, e) + pairs[e]))
    if not np.isfinite(blocks[:, -1]).all():
        e = int(np.nonzero(~np.isfinite(blocks[:, -1]))[0][0])
        raise ValueError("%s: pair %d (images %d and %d) has a cost that is not finite at the start (a correspondence that is not "
                         "finite?)" % ((who, e) + pairs[e]))
    cost = float(blocks[:, -1].sum())
    history, lam, iters, tried = [cost], ADJUST_LAMBDA0, 0, 0
    while iters < max_iters and lam <= ADJUST_LAMBDA_MAX:
        delta, st = step(blocks, lam)
        tried += 1
        if st != _lib.RWH_BUNDLE_OK:
            if tried == 1 or singular == "raise":
                raise ValueError("%s: the step's system is singular (an image that no edge with inliers touches?)" % who)
            lam *= ADJUST_LAMBDA_FACTOR
            continue
        cand = candidate(state, delta)
        accept = cand is not None
        if accept:
            cblocks, _, cstatus = evaluate(cand)
            ccost = float(cblocks[:, -1].sum())
            accept = bool((cstatus == _lib.RWH_BUNDLE_OK).all()) and ccost < cost
        if not accept:
            lam *= ADJUST_LAMBDA_FACTOR
            continue
        small = cost - ccost < ADJUST_REL_STOP * cost
        state, blocks, cost = cand, cblocks, ccost
        history.append(cost)
        iters += 1
        lam /= ADJUST_LAMBDA_FACTOR
        if small:
            break
    if info is not None:
        info["cost"], info["iters"], info["lambda"] = history, iters, lam
    return state


def sequence_adjust(Gs, pairs, matches, masks=None, anchor=0, max_iters=20, on="device", info=None):
    """Bundle adjustment of a sequence over its pair graph (the bundle rule of include/rwh.h): all G_i refined jointly, by
    Levenberg-Marquardt, over the inlier correspondences of every edge, so that the error of a chain no longer accumulates.

    Gs: N maps into the anchor's frame (`sequence_graph`'s or `sequence_plan`'s; Gs[anchor] the identity); pairs: E edges (s, d);
    matches: a `DeviceProblems` with one problem per edge (a in image s, b in image d), or a list of (ptsA [M, 2], ptsB [M, 2]);
    masks: the edges' inlier words, [E, words] (numpy uint64 / int64, or an int64 tensor on the GPU, e.g. `run_batch`'s
    info["mask_device"]; an all-zero row leaves an edge out), default: every correspondence is an inlier.
    on="device": the edge blocks come from `kernels.bundle_blocks` -- per evaluation one upload of E x 9 doubles, one launch, one
    download; on="host": from the host twin, no GPU needed.  Both give the same bits.

    An iteration: the blocks at the current Gs (those of the last accepted candidate), `rwh_host_bundle_step` at the current
    lambda, the candidate G_i @ (I + D(delta_i)), each divided by its largest |entry| (the anchor stays the identity), the
    candidate's blocks.  The step is accepted iff the candidate's cost (the sum of the edges' c) is strictly lower, no edge
    reports RWH_BUNDLE_BEHIND and every determinant is finite with the sign it had; then lambda <- lambda / 10, else lambda <-
    10 lambda.  Conventions, not measured optima: lambda starts at 1e-3; the loop ends after `max_iters` accepted steps, at
    lambda > 1e12, or on an accepted step that lowers the cost by less than 1e-12 of it.
    `info`: optional dict, receives "cost" (the start and every accepted step), "iters" (accepted steps) and "lambda".
    Returns Gs float64 [N, 3, 3], Gs[anchor] the identity.  ValueError: bad n, anchor, pairs, on or max_iters, matches or masks that
    do not fit the pairs, Gs that are not finite or invertible, a correspondence that is behind its camera at the start, a pair whose
    cost is not finite at the start (a NaN or infinite coordinate in its b, or residuals beyond float64; the pair is named), an
    image that no edge with inliers touches."""
    Gs = np.array([np.asarray(G, dtype=np.float64) for G in Gs])
    n = len(Gs)
    _check_count(n, anchor)
    pairs = _check_pairs("sequence_adjust", n, pairs)
    E = len(pairs)
    if on not in ("device", "host"):
        raise ValueError("sequence_adjust: on=%r; 'device' or 'host'" % (on,))
    if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or max_iters < 0:
        raise ValueError("sequence_adjust: max_iters=%r; an integer >= 0" % (max_iters,))
    if Gs.shape != (n, 3, 3) or not np.array_equal(Gs[anchor], np.eye(3)):
        raise ValueError("sequence_adjust: Gs takes %d 3 x 3 matrices with the identity at the anchor" % n)
    with np.errstate(all="ignore"):
        dets = np.linalg.det(Gs) if np.isfinite(Gs).all() else np.full(n, np.nan)
    if not (np.isfinite(dets) & (dets != 0.0)).all():
        raise ValueError("sequence_adjust: a map that is not finite or not invertible")
    if E < 1:
        raise ValueError("sequence_adjust: no pairs")
    blocks = _adjust_problem("sequence_adjust", "bundle", pairs, matches, masks, on)
    signs = np.sign(dets)

    def candidate(G, delta):
        # G_i (I + D(delta_i)), each over its largest |entry|; refused unless every determinant is finite with its starting sign
        with np.errstate(all="ignore"):
            cand = np.stack([G[i] if i == anchor else G[i] @ _delta_matrix(delta[i]) for i in range(n)])
            scale = np.abs(cand).reshape(n, 9).max(axis=1)
            scale[anchor] = 1.0
            cand = cand / scale[:, None, None]
            cdet = np.linalg.det(cand) if np.isfinite(cand).all() else np.full(n, np.nan)
        return cand if bool((np.isfinite(cdet) & (np.sign(cdet) == signs)).all()) else None

    return _levenberg("sequence_adjust", pairs, Gs, max_iters, info, evaluate=lambda G: blocks(_bundle_transfers(G, pairs)),
                      candidate=candidate, singular="raise",        # at every step
                      step=lambda blk, lam: kernels.host_bundle_step(n, anchor, pairs, blk, lam))


# ------------------------------------------- registration over rotations and focal lengths (the camera rule) ----
def _nearest_rotation(A):
    """U V^T of the SVD of A, the nearest rotation in the Frobenius norm (A has a positive determinant where this is called)."""
    U, _, Vt = np.linalg.svd(A)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R = U @ np.diag([1.0, 1.0, -1.0]) @ Vt
    return R


def _check_focal(who, focal):
    if isinstance(focal, (bool, str)) or not isinstance(focal, (int, float, np.integer, np.floating)) or not (np.isfinite(focal) and focal > 0):
        raise ValueError("%s: focal=%r; finite and > 0" % (who, focal))
    return float(focal)


def sequence_cameras(shapes, Gs, focal, anchor=0):
    """Rotations and focal lengths from the maps of a sequence (the geometry of the camera rule, include/rwh.h); pure numpy.

    shapes: N image shapes; Gs: N maps into the anchor's frame; focal: one focal length in pixels for every image.  With
    K_i = `_camera(shapes[i], focal)`, A = inv(K_a) @ (G_i * sign(det G_i)) @ K_i is scaled to determinant 1 and R_i is the
    rotation nearest to it (U V^T of its SVD); R_anchor is the identity exactly.  For maps that are K_a R_i inv(K_i) with this
    focal the R_i come back to rounding.  Returns (Rs float64 [N, 3, 3], fs float64 [N], every entry `focal`).  ValueError: N or
    anchor as `sequence_plan`'s, Gs of another shape, a determinant that is zero or not finite, a focal that is not finite and > 0."""
    n = len(shapes)
    _check_count(n, anchor)
    f = _check_focal("sequence_cameras", focal)
    mats = [np.asarray(G, dtype=np.float64) for G in Gs]
    if len(mats) != n or any(G.shape != (3, 3) for G in mats):
        raise ValueError("sequence_cameras: Gs takes %d 3 x 3 matrices" % n)
    Gs = _oriented(mats)
    kinv_a = np.linalg.inv(_camera(shapes[anchor], f))
    Rs = np.empty((n, 3, 3))
    for i in range(n):
        A = kinv_a @ Gs[i] @ _camera(shapes[i], f)
        with np.errstate(all="ignore"):
            det = np.linalg.det(A)
            A = A / np.cbrt(det)
        if not (np.isfinite(A).all() and det > 0):
            raise ValueError("sequence_cameras: image %d has a map without a rotation (focal %r)" % (i, f))
        Rs[i] = _nearest_rotation(A)
    Rs[anchor] = np.eye(3)
    return Rs, np.full(n, f)


def _check_cameras(who, shapes, Rs, fs, anchor):
    n = len(shapes)
    _check_count(n, anchor)
    Rs = np.array([np.asarray(R, dtype=np.float64) for R in Rs])
    fs = np.array(fs, dtype=np.float64).reshape(-1)
    if Rs.shape != (n, 3, 3) or not np.array_equal(Rs[anchor], np.eye(3)):
        raise ValueError("%s: Rs takes %d 3 x 3 rotations with the identity at the anchor" % (who, n))
    if not np.isfinite(Rs).all():
        raise ValueError("%s: a rotation that is not finite" % who)
    if fs.shape != (n,) or not (np.isfinite(fs) & (fs > 0)).all():
        raise ValueError("%s: fs takes %d focal lengths, finite and > 0" % (who, n))
    return Rs, fs


def sequence_camera_maps(shapes, Rs, fs, anchor=0):
    """G_i = K_a R_i inv(K_i) (the geometry of the camera rule): the maps `stitchSequence(Gs=...)` takes, from rotations and focal
    lengths; pure numpy.  Gs[anchor] is the identity exactly.  ValueError: N or anchor as `sequence_plan`'s, Rs that are not N
    finite 3 x 3 matrices with the identity at the anchor, fs that are not N finite focal lengths > 0."""
    Rs, fs = _check_cameras("sequence_camera_maps", shapes, Rs, fs, anchor)
    Ka = _camera(shapes[anchor], fs[anchor])
    Gs = np.stack([Ka @ R @ np.linalg.inv(_camera(shape, f)) for shape, R, f in zip(shapes, Rs, fs)])
    Gs[anchor] = np.eye(3)
    return Gs


def _camera_records(shapes, Rs, fs, pairs):
    """The edge records of the camera rule: R_d^T R_s row-major, then f_s, cx_s, cy_s, f_d, cx_d, cy_d: float64 [E, 15]."""
    centre = [((int(shape[1]) - 1) / 2.0, (int(shape[0]) - 1) / 2.0) for shape in shapes]
    return np.array([np.concatenate([(Rs[d].T @ Rs[s]).reshape(9), [fs[s], centre[s][0], centre[s][1], fs[d], centre[d][0], centre[d][1]]])
                     for s, d in pairs])


def _rodrigues(omega):
    """exp([omega]x) by Rodrigues' formula; below 1e-8 rad the series I + K + K K / 2, which is exact to rounding there."""
    theta = float(np.sqrt(omega @ omega))
    K = np.array([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]])
    if theta < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(theta) / theta) * K + ((1.0 - np.cos(theta)) / (theta * theta)) * (K @ K)


def sequence_adjust_cameras(shapes, Rs, fs, pairs, matches, masks=None, anchor=0, focals="shared", max_iters=20, on="device", info=None):
    """Bundle adjustment of a sequence over rotations and focal lengths (the camera rule of include/rwh.h): every R_i and the focal
    length -- one for all images, or one per image -- refined jointly, by Levenberg-Marquardt, over the inlier correspondences of every
    edge.  Four parameters per image where `sequence_adjust` has eight, and the maps stay those of a camera that turns about its
    centre: G_i = K_a R_i inv(K_i) (`sequence_camera_maps`).

    shapes: N image shapes; Rs, fs: N rotations (Rs[anchor] the identity) and N focal lengths, e.g. `sequence_cameras`'; pairs,
    matches, masks, on: as `sequence_adjust`'s.  focals="shared": one focal unknown, every fs equal at the start and at the end;
    focals="per-image": one per image, the anchor's included.  on="device": the edge blocks come from `kernels.camera_blocks` -- per
    evaluation one upload of E x 15 doubles, one launch, one download; on="host": from the host twin, no GPU needed.  Both give
    the same bits.

    The loop is `sequence_adjust`'s, with its constants: the blocks at the current cameras, `rwh_host_camera_step` at the current
    lambda, the candidate R_i exp([omega_i]x) (Rodrigues' formula, then U V^T of its SVD, so that it stays a rotation; the anchor
    stays the identity) and f_i (1 + phi_i), the candidate's blocks.  The step is accepted iff every candidate focal is finite and
    > 0, the candidate's cost (the sum of the edges' c) is strictly lower and no edge reports RWH_BUNDLE_BEHIND; then lambda <-
    lambda / 10, else lambda <- 10 lambda.  It ends after `max_iters` accepted steps, at lambda > 1e12, or on an accepted step that
    lowers the cost by less than 1e-12 of it.  A step whose system is singular raises on the first step tried (an image that no
    edge touches is singular at every lambda); later it counts as a rejected step -- where the data leave the focal length open
    (images that are translations of each other) the damping is all that keeps the system definite, and it shrinks with every
    accepted step.  `info`: optional dict, receives "cost" (the start and every accepted step), "iters"
    and "lambda".  Returns (Rs float64 [N, 3, 3], fs float64 [N]).  ValueError: bad n, anchor, pairs, on, focals or max_iters, Rs or
    fs that `sequence_camera_maps` refuses, focals="shared" with fs that differ, matches or masks that do not fit the pairs, a
    correspondence that is behind its camera at the start, a pair whose cost is not finite at the start (the pair is named), an
    image that no edge with inliers touches."""
    who = "sequence_adjust_cameras"
    Rs, fs = _check_cameras(who, shapes, Rs, fs, anchor)
    n = len(Rs)
    pairs = _check_pairs(who, n, pairs)
    E = len(pairs)
    if on not in ("device", "host"):
        raise ValueError("%s: on=%r; 'device' or 'host'" % (who, on))
    if not (isinstance(focals, str) and focals in kernels.CAMERA_FOCALS):
        raise ValueError("%s: focals=%r; 'shared' or 'per-image'" % (who, focals))
    if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or max_iters < 0:
        raise ValueError("%s: max_iters=%r; an integer >= 0" % (who, max_iters))
    if focals == "shared" and not (fs == fs[0]).all():
        raise ValueError("%s: focals='shared' takes equal focal lengths, got %r" % (who, fs.tolist()))
    for i, shape in enumerate(shapes):
        if len(shape) < 2:
            raise ValueError("%s: shape %r of image %d; (h, w[, c])" % (who, shape, i))
    if E < 1:
        raise ValueError("%s: no pairs" % who)
    blocks = _adjust_problem(who, "camera", pairs, matches, masks, on)

    def candidate(cameras, delta):
        # f_i (1 + phi_i), refused unless every one is finite and > 0 (and delta finite); then the rotations nearest to
        # R_i exp([omega_i]x), which are not computed for a refused candidate
        R, f = cameras
        with np.errstate(all="ignore"):
            cf = f * (1.0 + delta[:, 3])
            if not (bool((np.isfinite(cf) & (cf > 0)).all()) and bool(np.isfinite(delta).all())):
                return None
            return np.stack([R[i] if i == anchor else _nearest_rotation(R[i] @ _rodrigues(delta[i, :3])) for i in range(n)]), cf

    # A singular step raises on the first step tried only.  Later on it is the damping that has become too small for a direction the
    # data do not determine (the focal length of images that are translations of each other): a rejected step, lambda goes up again.
    return _levenberg(who, pairs, (Rs, fs), max_iters, info,
                      evaluate=lambda cameras: blocks(_camera_records(shapes, cameras[0], cameras[1], pairs)),
                      candidate=candidate, singular="reject",
                      step=lambda blk, lam: kernels.host_camera_step(n, anchor, pairs, blk, lam, focals))


def _sequence_inputs(who, images, Hs, Gs, anchor, projection=None, focal=None, wrap=False):
    """What stitchSequence and sequence_gains check of their images and geometry, before any GPU use: -> (rects, origin, size,
    default order, inv_g float64 [N, 3, 3], rays).  rays is None on the anchor's plane.  With a projection it is the two ray tables
    (numpy), the rectangles are in canvas coordinates and the matrices are the M_i = inv(G_i) @ K of the projection rule.  With
    wrap (the ring rule) the canvas is (fh, P), a rectangle's mx is taken modulo P (0 for a rectangle P wide) and the tables are made
    with the radius P / (2 pi).  The six-tuple is pinned: tests, probes and the registration driver unpack it."""
    n = len(images)
    _check_count(n, anchor)
    _check_projection(who, projection, focal)
    period = _check_wrap(who, wrap, projection, focal)
    if (Hs is None) == (Gs is None):
        raise ValueError("%s: exactly one of Hs and Gs" % who)
    for i, img in enumerate(images):
        if len(img.shape) != 3 or img.shape[2] != 3 or str(img.dtype).replace("torch.", "") != "uint8":
            raise NotImplementedError("%s: image %d is %s %s; uint8 [h, w, 3] images are taken" % (who, i, img.dtype, tuple(img.shape)))
    shapes = [tuple(int(v) for v in img.shape) for img in images]
    if Hs is not None:
        Gs, rects, origin, size, default = sequence_plan(shapes, Hs, anchor, projection, focal, wrap)
    else:
        Gs = np.array([np.asarray(G, dtype=np.float64) for G in Gs])
        if Gs.shape != (n, 3, 3) or not np.array_equal(Gs[anchor], np.eye(3)):
            raise ValueError("%s: Gs takes %d 3 x 3 matrices with the identity at the anchor" % (who, n))
        if projection is not None:
            Gs = _oriented(Gs)
            rects, origin, size, default = _curved_canvas(shapes, Gs, anchor, projection, focal, period)
        else:
            rects, origin, size, default = _sequence_canvas(shapes, Gs, anchor)
    if projection is not None:
        K = _camera(shapes[anchor], focal)
        with np.errstate(all="ignore"):
            m = np.stack([K if i == anchor else np.linalg.inv(Gs[i]) @ K for i in range(n)])
        if not np.isfinite(m).all():
            raise ValueError("%s: an inverse homography is not finite" % who)
        if period is not None:
            rects = [(0 if r[2] == period else (r[0] - origin[0]) % period, r[1] - origin[1], r[2], r[3]) for r in rects]
            return rects, origin, size, default, m, sequence_ray_tables(projection, period / (2.0 * np.pi), origin, size)
        rects = [(r[0] - origin[0], r[1] - origin[1], r[2], r[3]) for r in rects]
        return rects, origin, size, default, m, sequence_ray_tables(projection, focal, origin, size)
    inv_g = np.stack([np.eye(3) if i == anchor else np.linalg.inv(Gs[i]) for i in range(n)])
    return rects, origin, size, default, inv_g, None


def _sequence_geometry(who, images, Hs, Gs, anchor, projection=None, focal=None, wrap=False):
    """`_sequence_inputs` as the launchers take it -> (default order, kernels.SeqGeometry); the ray tables are still on the host."""
    rects, origin, size, default, mats, rays = _sequence_inputs(who, images, Hs, Gs, anchor, projection, focal, wrap)
    if rays is None:
        return default, kernels.SeqGeometry(mats, rects, size, anchor, origin)
    return default, kernels.SeqGeometry(mats, rects, size, rays=rays, ring=wrap is not False)


def _sequence_upload(images):
    dev = _lib.require_gpu()
    return [img.to(dev).contiguous() if _is_tensor(img) else _xfer.to_device(img, dev) for img in images]


def _check_gain_options(who, stride, sigma_n, sigma_g):
    if not (isinstance(stride, (int, np.integer)) and not isinstance(stride, bool) and 1 <= stride <= _lib.RWH_SEQ_MAX_STRIDE):
        raise ValueError("%s: stride %r; an integer of 1 .. %d" % (who, stride, _lib.RWH_SEQ_MAX_STRIDE))
    for name, v in (("sigma_n", sigma_n), ("sigma_g", sigma_g)):
        if not (isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v) and v > 0):
            raise ValueError("%s: %s = %r; finite and > 0" % (who, name, v))


def _gains_on_device(on_dev, geom, stride, sigma_n, sigma_g, info):
    """One statistics launch, one download of the two n x n tables, one call of rwh_host_sequence_gains -> float64 [N].
    geom: the call's kernels.SeqGeometry, its ray tables on the device."""
    n = len(on_dev)
    tabs = kernels.sequence_overlap_tables_on(on_dev, geom, int(stride)).cpu().numpy().view(np.uint64)
    gains = np.empty(n, dtype=np.float64)
    status = _lib.load().rwh_host_sequence_gains(tabs[0].ctypes.data, tabs[1].ctypes.data, n, float(sigma_n), float(sigma_g), gains.ctypes.data)
    if status == _lib.RWH_E_INVALID:
        raise ValueError("sequence_gains: the gain system has a non-positive pivot or a non-finite solution")
    _lib.check(status, "rwh_host_sequence_gains")
    if info is not None:
        info["count"], info["sum"] = tabs[0].copy(), tabs[1].copy()
    return gains


def sequence_gains(images, Hs=None, Gs=None, anchor=0, stride=4, sigma_n=10.0, sigma_g=0.1, info=None, projection=None, focal=None,
                   wrap=False):
    """One exposure gain per image of a sequence (the gain rule of include/rwh.h; Brown & Lowe 2007, section 6): the overlap
    statistics of the images, warped as `stitchSequence` warps them, are reduced on the GPU in one pass over every stride-th canvas
    pixel each way (`rwh_sequence_overlap_stats`), the two N x N integer tables come down in one copy, and the N x N system is
    solved on the host (`rwh_host_sequence_gains`).  -> float64 [N]; `stitchSequence(..., gains=...)` applies them.

    images, Hs, Gs, anchor: as `stitchSequence`'s, and refused as there.  sigma_n (10.0): the standard deviation of the intensity
    error, on the 0 .. 255 scale; sigma_g (0.1): that of the gain about 1.  stride=4 is a convention -- a sixteenth of the samples
    moves the gains of the test scenes in the third decimal -- not a measured optimum.  `info`: optional dict, receives "count" and
    "sum" (uint64 [N, N]), and with wrap "period" and "radius".  projection, focal, wrap: as `stitchSequence`'s -- the statistics
    are taken on that canvas.  ValueError: a stride outside 1 .. 255, a sigma that is not finite and > 0, before the GPU is touched."""
    _, geom = _sequence_geometry("sequence_gains", images, Hs, Gs, anchor, projection, focal, wrap)
    _check_gain_options("sequence_gains", stride, sigma_n, sigma_g)
    if geom.ring and info is not None:
        info["period"], info["radius"] = int(geom.size[1]), int(geom.size[1]) / (2.0 * np.pi)
    on_dev = _sequence_upload(images)
    return _gains_on_device(on_dev, geom.on_device(on_dev[0].device), stride, sigma_n, sigma_g, info)


class BlockGains(NamedTuple):
    """What `sequence_block_gains` returns and `stitchSequence(gains=...)` takes: maps, float64 numpy [N, gh, gw], the gain of each
    image in each `block` x `block` cell of the canvas; base, float64 [N], the one-gain-per-image part they were solved on top of
    (what the seam finder's survey is given)."""
    maps: object
    block: int
    base: object


def _check_block_options(who, block, stride, sigma_n, sigma_g, smooth):
    kernels.sequence_block_shift(who, block)
    _check_gain_options(who, stride, sigma_n, sigma_g)
    if not (isinstance(smooth, (int, np.integer)) and not isinstance(smooth, bool) and 0 <= smooth <= _lib.RWH_SEQ_MAX_SMOOTH):
        raise ValueError("%s: smooth %r; an integer of 0 .. %d" % (who, smooth, _lib.RWH_SEQ_MAX_SMOOTH))


def _no_wrap_blocks(who, wrap):
    if wrap is not False:
        raise NotImplementedError("%s: block gains on a wrap-around canvas are not provided (the block gain rule has no ring form)" % who)


def _block_gains_on_device(on_dev, geom, block, stride, sigma_n, sigma_g, smooth, base, info):
    """One cell-statistics launch, one download of the table, one call of rwh_host_sequence_block_gains -> BlockGains.
    base: "auto" (`sequence_gains`' defaults on the same upload), None (all ones) or N checked gains."""
    n = len(on_dev)
    if isinstance(base, str):
        base = _gains_on_device(on_dev, geom, 4, 10.0, 0.1, None)
    elif base is None:
        base = np.ones(n, dtype=np.float64)
    tabs = kernels.sequence_cell_tables_on(on_dev, geom, int(block), int(stride)).cpu().numpy().view(np.uint32)
    status, maps = kernels.host_sequence_block_gains(tabs, geom, n, int(block), base, sigma_n, sigma_g, int(smooth))
    if status == _lib.RWH_E_INVALID:
        raise ValueError("sequence_block_gains: a cell's gain system has a non-positive pivot, or a map entry is not finite and > 0")
    _lib.check(status, "rwh_host_sequence_block_gains")
    if info is not None:
        info["tables"], info["slots"] = tabs, int(tabs.shape[-1])
    return BlockGains(maps, int(block), base)


def sequence_block_gains(images, Hs=None, Gs=None, anchor=0, block=32, stride=1, sigma_n=10.0, sigma_g=0.1, smooth=2, base="auto", info=None,
                         projection=None, focal=None):
    """One exposure gain MAP per image of a sequence (the block gain rule of include/rwh.h; what OpenCV's stitcher does by default):
    the canvas is cut into `block` x `block` cells, the gain rule's overlap statistics are reduced per cell on the GPU in one launch
    (`rwh_sequence_cell_stats`, one workgroup per cell), the table comes down in one copy, and on the host every cell's small gain
    system is solved on top of `base`, the solutions are smoothed and become the maps (`rwh_host_sequence_block_gains`).  What
    varies inside an image -- vignetting, a sky brighter on one side -- is compensated, which one gain per image cannot do.
    -> BlockGains(maps float64 [N, gh, gw], block, base float64 [N]); `stitchSequence(..., gains=...)` applies it, interpolating
    the maps bilinearly between cell centres.

    images, Hs, Gs, anchor, projection, focal: as `stitchSequence`'s, and refused as there; the wrap-around canvas is not taken.
    block (32): 16, 32, 64 or 128 -- OpenCV's block size, a convention and not a measured optimum.  stride (1): every stride-th
    canvas pixel each way is a sample, 1 .. 255; 1 is a convention too (a cell of 32 x 32 has few samples to spare).  sigma_n, sigma_g:
    as `sequence_gains`'s.  smooth (2): iterations of the 1-2-1 filter over the cells, 0 .. 8; OpenCV's convention.
    base: "auto" -- `sequence_gains` with its defaults on the same upload; None -- all ones; or N gains, finite and > 0.
    `info`: optional dict, receives "tables" (uint32 [gh, gw, 2, K, K]) and "slots" (K, the most images that meet one cell).
    ValueError: another block, stride, sigma or smooth, a base of another length or string, before the GPU is touched."""
    who = "sequence_block_gains"
    _, geom = _sequence_geometry(who, images, Hs, Gs, anchor, projection, focal, False)
    _check_block_options(who, block, stride, sigma_n, sigma_g, smooth)
    if isinstance(base, str):
        if base != "auto":
            raise ValueError("%s: base=%r; 'auto', None or N gains" % (who, base))
    elif base is not None:
        base = kernels.sequence_gains_array(base, len(images), who)
    on_dev = _sequence_upload(images)
    return _block_gains_on_device(on_dev, geom.on_device(on_dev[0].device), block, stride, sigma_n, sigma_g, smooth, base, info)


def _check_block_gains(who, gains, n, size):
    """A BlockGains given to stitchSequence or sequence_seams, before the GPU is touched: ValueError for another block, maps that do
    not fit the canvas and block, an entry or a base gain that is not finite and > 0."""
    kernels.sequence_block_shift(who, gains.block)
    maps = np.ascontiguousarray(gains.maps, dtype=np.float64)
    want = (n,) + kernels.sequence_cell_grid(size, gains.block)
    if maps.shape != want:
        raise ValueError("%s: gain maps of shape %s; %s for a %d x %d canvas and block %d" % (who, maps.shape, want, size[0], size[1], gains.block))
    if not (np.isfinite(maps).all() and (maps > 0).all()):
        raise ValueError("%s: a gain map entry is not finite and > 0" % who)
    return BlockGains(maps, int(gains.block), kernels.sequence_gains_array(gains.base, n, who))


def _check_bands(who, bands):
    kernels.sequence_bands_check(who, bands)


def sequence_seams(images, Hs=None, Gs=None, anchor=0, gains=None, margin=8.0, tau=64, info=None, projection=None, focal=None):
    """Which image owns each canvas pixel of a sequence, decided by what the images show (the seam rule of include/rwh.h; a
    geodesic, watershed-style seam): every image grows outward from the pixels it owns beyond dispute -- those where every other
    covering image is within `margin` of its own border -- slowly (`tau` per pixel) where the covering images agree and fast where
    they disagree, and a pixel goes to the image that reaches it first.  An object that only one image shows is swept whole by one
    front instead of being cut along the overlap's midline.  -> labels, uint8 [fh, fw] on `stitchSequence`'s canvas: the owner's
    index, 255 where nothing covers; numpy arrays in -> a numpy plane, any tensor in -> a device tensor.
    `stitchSequence(..., seams=labels)` composites with them.

    images, Hs, Gs, anchor, projection, focal: as `stitchSequence`'s, and refused as there.  gains: None or N exposure gains (the
    disagreement is taken on the compensated bytes); a BlockGains gives its `base` -- the survey keeps one gain per image.  margin=8.0 and tau=64 (an integer of 1 .. 766) are conventions, not measured
    optima; margin=inf gives the feather winner of multi-band blending.  `info`: optional dict, receives "passes", the number of
    relaxation passes that changed a distance.  The relaxation runs until nothing changes and the host reads a flag between
    passes: the call synchronises torch's current stream.  The wrap-around canvas is not taken.
    ValueError: a margin that is negative or not a number, another tau, before the GPU is touched."""
    n = len(images)
    _, geom = _sequence_geometry("sequence_seams", images, Hs, Gs, anchor, projection, focal, False)
    kernels.sequence_seam_options("sequence_seams", margin, tau)
    if isinstance(gains, BlockGains):
        gains = _check_block_gains("sequence_seams", gains, n, geom.size).base
    elif gains is not None:
        gains = kernels.sequence_gains_array(gains, n, "sequence_seams")
    tens = any(_is_tensor(img) for img in images)
    on_dev = _sequence_upload(images)
    labels = kernels.sequence_seams_on(on_dev, geom.on_device(on_dev[0].device), gains=gains, margin=margin, tau=int(tau), info=info)
    return labels if tens else _xfer.to_host(labels)


def _check_seams(who, seams, blending, wrap):
    """`seams` of stitchSequence, before the GPU is touched -> None (no seams), ("find", margin, tau) or ("plane", labels)."""
    if seams is None or seams is False:
        return None
    if blending == "feather":
        raise ValueError("%s: seams with blending='feather': a feathered pixel has no single owner; blending=False or 'multiband'" % who)
    if wrap is not False:
        raise NotImplementedError("%s: seams on a wrap-around canvas are not provided (the seam rule has no ring form)" % who)
    if seams is True:
        return ("find", 8.0, 64)
    if isinstance(seams, dict):
        if set(seams) - {"margin", "tau"}:
            raise ValueError("%s: seams=%r; the keys are 'margin' and 'tau'" % (who, seams))
        margin, tau = seams.get("margin", 8.0), seams.get("tau", 64)
        kernels.sequence_seam_options(who, margin, tau)
        return ("find", margin, int(tau))
    if len(getattr(seams, "shape", ())) != 2 or str(seams.dtype).replace("torch.", "") != "uint8":
        raise ValueError("%s: seams=%r; None, True, a dict of 'margin' and 'tau', or a uint8 [fh, fw] label plane" % (who, type(seams)))
    return ("plane", seams)


def stitchSequence(images, Hs=None, Gs=None, anchor=0, blending=False, order=None, gains=None, info=None, projection=None, focal=None,
                   wrap=False, seams=None, bands=5):
    """N images into one panorama in ONE pass over the canvas (`rwh_stitch_sequence`): every image is warped once into the
    anchor's frame and every canvas pixel written once.  The reference has no counterpart -- its stitchPanorama takes two images,
    and folding it over a list resamples the growing canvas once per image; this is held to the sequence rule stated in
    include/rwh.h, the reference's paste compositor generalised.  With two images and blending=False the canvas is, byte for
    byte, stitchPanorama(images[0], images[1], H) with Hs = [H].

    images: N (1 .. 64) uint8 [h, w, 3] numpy arrays or tensors, sizes may differ; exactly one of Hs (N - 1 pairwise homographies,
    chained by `sequence_plan`) and Gs (N maps into the anchor's frame, used as given; Gs[anchor] must be the identity).
    blending: False -- the first image in `order` (default: the anchor, then the nearest) that covers a pixel gives it;
    "feather" -- every covering image, weighted by its distance to its own border (`order` is ignored); "multiband" -- multi-band
    blending (the multi-band rule of include/rwh.h; Burt & Adelson pyramids as Brown & Lowe 2007, section 7, use them): low
    frequencies are blended over a wide region, high frequencies come from the image with the greatest feather weight, so neither an
    exposure step nor ghosting remains (`order` is validated and otherwise ignored).  bands (5): the pyramid levels of "multiband",
    an integer of 1 .. 8, ignored by the other blends; 5 is OpenCV's convention, not a measured optimum, and it wants overlaps several
    times 2^(bands+2) pixels wide -- 170-pixel overlaps were visibly too narrow for 5.  gains: None -- the images
    as they are; N exposure gains (the gain rule of include/rwh.h: every sample value v of image i enters as min(v * g_i, 255.0));
    "auto" -- `sequence_gains` with its defaults on the same images and geometry, the images uploaded once; a BlockGains (the
    block gain rule: one gain MAP per image, `sequence_block_gains`) -- every sample value enters as min(v * g, 255.0) with g read
    from image i's map at the pixel, under every blend; "blocks" -- `sequence_block_gains` with its defaults on the same upload.
    Found seams survey the images with one gain each, the BlockGains' `base`.  Block gains are not provided with `wrap`
    (NotImplementedError, before the GPU is touched).  `info`: optional dict,
    receives "gains" (the gains used: float64 [N], the BlockGains, or None).  numpy arrays in -> a
    numpy canvas; any tensor in -> a device tensor and no host copy of pixels.  The caller's images are never written.
    projection: None -- the canvas is the anchor's image plane, which suits a narrow sweep (at 100 degrees off the anchor the plane
    is behind the camera); "cylindrical" or "spherical" -- the canvas is that surface about the anchor's camera with radius `focal`
    (pixels; `sequence_focal` estimates one from Hs), held to the projection rule of include/rwh.h: every image is warped, the
    anchor included, and all blends, gains and bands work on it as on the plane.  Without `wrap` an image that lies across the
    seam behind the anchor is refused.
    wrap: False; True or a period P in columns (a positive multiple of 256 up to 65280; True is `sequence_period(focal)`) -- a sweep
    that closes the circle, on a canvas exactly P columns wide that wraps around at the seam behind the anchor (the ring rule of
    include/rwh.h): the surface has the radius P / (2 pi), the cameras keep `focal`, an image may lie across the seam, and all
    blends, gains and bands work across it.  It takes a projection.  `info` then also receives "period" and "radius".  `bands` stays
    the last parameter: pass it, and `wrap`, by name.
    seams: None -- the owner of a pixel is decided by geometry alone, as above; True -- `sequence_seams` with its defaults (margin
    8.0, tau 64: conventions, not measured optima) on the same upload and with the gains in use; a dict with "margin" and / or
    "tau" -- the same with those; a uint8 [fh, fw] label plane (numpy or tensor) -- used as given, a label that names no covering
    image leaves the pixel to the geometric rule.  With blending=False the canvas is label paste (every pixel the bytes of its
    owner; `order` is validated and otherwise ignored), with "multiband" the labels replace the winner of the multi-band rule (the
    seam rule of include/rwh.h, "Using labels").  When seams are found `info` receives "passes" and "labels" (the plane used), and
    the call synchronises the stream.  ValueError: seams with "feather"; NotImplementedError, before the GPU is touched: seams
    with `wrap`.
    ValueError: what `sequence_plan` refuses, an `order` that is not a permutation, another `blending`, gains of another length,
    not finite or <= 0, or another string; NotImplementedError: images that are not uint8 [h, w, 3]."""
    n = len(images)
    _check_count(n, anchor)
    if blending is not False and blending != "feather" and blending != "multiband" and blending:
        raise ValueError("stitchSequence: blending=%r; False, 'feather' or 'multiband'" % (blending,))
    if blending == "multiband":
        _check_bands("stitchSequence", bands)
    seam = _check_seams("stitchSequence", seams, blending, wrap)
    if isinstance(gains, BlockGains) or (isinstance(gains, str) and gains == "blocks"):
        _no_wrap_blocks("stitchSequence", wrap)
    blend = _lib.RWH_SEQ_FEATHER if blending == "feather" else _lib.RWH_SEQ_PASTE
    default, geom = _sequence_geometry("stitchSequence", images, Hs, Gs, anchor, projection, focal, wrap)
    if seam is not None and seam[0] == "plane" and tuple(int(v) for v in seam[1].shape) != tuple(int(v) for v in geom.size):
        raise ValueError("stitchSequence: seams is a %s plane, the canvas is %s" % (tuple(seam[1].shape), tuple(geom.size)))
    order = default if order is None else [int(v) for v in order]
    if sorted(order) != list(range(n)):
        raise ValueError("stitchSequence: order %r is not a permutation of 0 .. %d" % (order, n - 1))
    if isinstance(gains, str):
        if gains not in ("auto", "blocks"):
            raise ValueError("stitchSequence: gains=%r; None, N gains, a BlockGains, 'auto' or 'blocks'" % (gains,))
    elif isinstance(gains, BlockGains):
        gains = _check_block_gains("stitchSequence", gains, n, geom.size)
    elif gains is not None:
        gains = kernels.sequence_gains_array(gains, n, "stitchSequence")
    tens = any(_is_tensor(img) for img in images)
    on_dev = _sequence_upload(images)
    geom = geom.on_device(on_dev[0].device)
    if isinstance(gains, str):
        gains = (_gains_on_device(on_dev, geom, 4, 10.0, 0.1, None) if gains == "auto" else
                 _block_gains_on_device(on_dev, geom, 32, 1, 10.0, 0.1, 2, "auto", None))
    if info is not None:
        info["gains"] = gains
        if geom.ring:
            info["period"], info["radius"] = int(geom.size[1]), int(geom.size[1]) / (2.0 * np.pi)
    survey = gains
    if isinstance(gains, BlockGains):                      # the compositors read the maps, the seam survey keeps one gain per image
        survey, gains = gains.base, kernels.SeqGainMaps(_xfer.to_device(gains.maps, on_dev[0].device), gains.block)
    labels = None
    if seam is not None and seam[0] == "find":
        found = {}
        labels = kernels.sequence_seams_on(on_dev, geom, gains=survey, margin=seam[1], tau=seam[2], info=found)
        if info is not None:
            info["passes"], info["labels"] = found["passes"], labels if tens else _xfer.to_host(labels)
    elif seam is not None:
        labels = seam[1]
    if blending == "multiband":
        out = kernels.stitch_sequence_multiband_on(on_dev, geom, int(bands), gains=gains, labels=labels)
    elif labels is not None:
        out = kernels.stitch_sequence_labels_on(on_dev, geom, labels, gains=gains)
    else:
        out = kernels.stitch_sequence_on(on_dev, geom, order, blend, gains=gains)
    return out if tens else _xfer.to_host(out)


# numpy element types the any-dtype compositor reads (bool as uint8); torch's are kernels.STITCH_DTYPE
_STITCH_NP = {np.dtype(t): np.dtype(v) for t, v in ((np.bool_, np.uint8), (np.uint8, np.uint8), (np.int8, np.int8), (np.uint16, np.uint16),
                                                    (np.int16, np.int16), (np.int32, np.int32), (np.uint32, np.uint32), (np.int64, np.int64),
                                                    (np.uint64, np.uint64), (np.float16, np.float16), (np.float32, np.float32),
                                                    (np.float64, np.float64))}


def _blank_channels(img, k):
    """Channels 0 .. k-1 of texel (0,0) of the caller's array or tensor set to 0, any dtype (a tensor through its bytes: torch
    has no fill for every dtype on the device)."""
    if _is_tensor(img) and img.stride(2) == 1:
        import torch
        try:
            img.view(torch.uint8)[0, 0, :k * img.element_size()] = 0
            return
        except RuntimeError:
            pass
    for c in range(k):
        img[0, 0, c] = 0


def _stitch_any(imgQ, imgT, H, blending, blendrate):
    """stitchPanorama on what the uint8 compositor does not take (homography.py:288-338): any numeric dtype, imgT with 3 or 4
    channels, imgQ with 1, 3 or 4.  The reference's sequence: addAlpha (a float32 copy; blend only), the bounds, the blanking of
    texel (0,0) by bilinear() (on the caller's imgT in paste: IndexError there with fewer than 3 channels), the warp (IndexError
    where it indexes past imgT), the canvas (ValueError where imgQ does not broadcast into it)."""
    import torch
    for img, what in ((imgT, "imgT"), (imgQ, "imgQ")):
        known = img.dtype in kernels.STITCH_DTYPE if _is_tensor(img) else np.asarray(img).dtype in _STITCH_NP
        if not known or img.shape[2] >= 5:
            raise NotImplementedError("stitchPanorama: %s (%s, %d channels) is not composited here: the compositor takes numeric images "
                                      "with 1 to 4 channels (homography.py:288-338)" % (what, img.dtype, img.shape[2]))
    ct, cq = int(imgT.shape[2]), int(imgQ.shape[2])
    paste = not blending
    if blending == 'Rate':
        print(blendrate + 1e-10)   # addAlpha prints the rate it stores (homography.py:257)
    elif blending == 'Gradient':
        print('not implement yet')  # homography.py:266
    h, w = int(imgT.shape[0]), int(imgT.shape[1])
    mx, my, wt, ht = _bounds(h, w, H, 0)
    if wt <= 0 or ht <= 0:
        raise ValueError("Number of samples, %d, must be non-negative." % min(wt, ht))
    hq, wq = int(imgQ.shape[0]), int(imgQ.shape[1])
    (tsx, tsy, tex, tey), (qsx, qsy, qex, qey), (fw, fh) = _stitch_geometry(wt, ht, wq, hq, mx, my)
    inv_h = np.linalg.inv(np.asarray(H, dtype=np.float64))
    cw = ct if paste else ct + 1                             # channels bilinear() sees (addAlpha appends one)
    if cw < 3:                                               # bilinear() blanks channels 0..2: IndexError at channel cw
        if paste:
            _blank_channels(imgT, cw)
        raise IndexError("index %d is out of bounds for axis 2 with size %d" % (cw, cw))
    if paste:
        _blank_channels(imgT, ct)                            # the caller's array, as bilinear() (the kernel blanks the device copy)
    dev = _lib.require_gpu()
    flag = kernels.warp_index_check((h, w), inv_h, kernels.Grid(mx, mx + wt - 1, wt, my, my + ht - 1, ht), (h, w), "bilinear", dev)
    # the canvas assignments after the warp: imgQ into the C_T-channel canvas (paste) or imgQ[:, :, :3] into channels 0..2 (blend)
    q_into = ct if paste else 3
    q_from = cq if paste else min(cq, 3)
    if (q_from != q_into and q_from != 1) or cw == 3 and not paste:
        bits = int(flag.item())
        if bits:
            kernels.raise_like_reference(bits, (h, w))
        if q_from != q_into and q_from != 1:
            raise ValueError("could not broadcast input array from shape (%d,%d,%d) into shape (%d,%d,%d)" % (hq, wq, q_from, hq, wq, q_into))
        raise IndexError("index 3 is out of bounds for axis 2 with size 3")      # a 2-channel imgT: the canvas has no alpha channel

    def on_device(img):
        if _is_tensor(img):
            t = img.to(dev)
            return (t.view(torch.uint8) if t.dtype == torch.bool else t).contiguous()
        a = np.ascontiguousarray(img)
        return _xfer.to_device(a.view(_STITCH_NP[a.dtype]), dev)
    t_dev, q_dev = on_device(imgT), on_device(imgQ)
    mode = 0 if paste else 1 if blending == 'Rate' else 2 if blending == 'Gradient' else 3
    out = kernels.stitch_panorama_ex(t_dev, q_dev, inv_h, (mx, my), (wt, ht), (tsx, tsy), (qsx, qsy), (fh, fw), mode, blendrate,
                                     zero_origin=True)
    if _is_tensor(imgQ) or _is_tensor(imgT):
        res = out
    else:
        res = _xfer.to_host(out)
    bits = int(flag.item())
    if bits:
        kernels.raise_like_reference(bits, (h, w))
    return res


def cylindericlMap(img, f=1600):
    """Import-compatibility stub: ransac.py:3 imports this name but no live code calls it
    (its only call sites are commented out, ransac.py:249-251).  Needs cv2.remap."""
    raise NotImplementedError("cylindrical warps are dead code in the reference and out of scope (SURVEY.md C11)")
