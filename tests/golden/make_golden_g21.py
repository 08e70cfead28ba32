#!/usr/bin/env python3
"""Generate tests/golden/g21_warp_dtypes.npz: the reference's warp entry points (homography.py:108-242) on images of every numeric
dtype with 1 to 5 channels -- wrapPerspective (nn / bilinear, boundary 0 / 1), wrapPerspectiveScan (`res` smaller and larger than
the image), transformImage (auto-bounds and `box`), transformImageH, and convertfunc['nn' / 'bilinear'] on precomputed
coordinates -- with special values (fractions, NaN, +-inf, -0.0, values past 2^24 / 2^31 / 2^53, negative integers) and
homographies that complete or raise (identity: IndexError; singular; NaN).

Imports the reference's unmodified homography.py the way make_golden.py does (an empty cv2 stub module) and writes data only.

Per case: the entry point and its arguments (an index into the image pool, H, convert, boundary, res, u / v, box, a z_t pool key);
the outcome (the exception's type name, or "ok"); the result's raw bytes (offset into `out_flat`), dtype and shape; the origin
(mx, my); the raw bytes of texel (0,0) of the caller's image after the call (`t00`; the generator asserts that nothing else of the
image changes); for convertfunc the caller's z_t after the call (`z_after`, offset into `z_flat`).

The legacy class -- uint8 / float32 images with 3 or 4 channels, which keep their kernels -- gets no non-finite value next to the
origin and no uint8-output case with values past int32: there the existing exact kernel returns 0 for a masked bilinear pixel and
casts to uint8 through a saturating int32 conversion, which this fixture does not cover.

Usage:  python tests/golden/make_golden_g21.py
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

REF = os.environ.get("RWH_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
sys.path.insert(0, REF)
import homography as ref_h  # noqa: E402  (the reference)

DTYPES = ("uint8", "int8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float16", "float32", "float64", "bool")
HWS = ((12, 16), (9, 11))
P = np.array([[1.0, 0.01, 0.0], [0.012, 0.99, 0.0], [2e-3, 1e-3, 1.0]])
SHIFTS = {"left_up": (-3.3, -2.6), "right_down": (4.7, 3.2), "inside": (1.4, 1.3), "left_down": (-4.2, 2.4), "right_up": (5.5, -2.3)}
ROT = np.array([[np.cos(0.3), -np.sin(0.3), 3.0], [np.sin(0.3), np.cos(0.3), -2.0], [1e-3, -2e-3, 1.0]])


def shifted(name):
    S = np.eye(3)
    S[0, 2], S[1, 2] = SHIFTS[name]
    return S @ P


SPECIAL = {
    "float64": [np.nan, np.inf, -np.inf, -0.0, 0.1, 2.9999999999, -0.5, 255.5, 2.0 ** 24 + 1, 2.0 ** 31 + 3, -2.0 ** 31 - 3, 2.0 ** 53 + 2,
                1e300, -1e300, 300.7, -1.5],
    "float32": [np.nan, np.inf, -np.inf, -0.0, 0.1, -0.5, 255.5, 2.0 ** 24 + 2, 2.0 ** 31 + 256, -2.0 ** 31 - 256, 3e38, 300.7, -1.5],
    "float16": [np.nan, np.inf, -np.inf, -0.0, 0.1, -0.5, 255.5, 65504.0, -65504.0, 300.7, -1.5, 2049.0],
    "int32": [2 ** 31 - 1, -2 ** 31, 2 ** 24 + 1, 16777217, -(2 ** 24) - 1, 255, 256, -1, -300],
    "int64": [2 ** 63 - 1, -2 ** 63, 2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53) - 1, 16777217, 2 ** 31 + 5, -2 ** 31 - 5, -1],
    "uint64": [2 ** 64 - 1, 2 ** 63 + 2 ** 39 + 1, 2 ** 53 + 1, 2 ** 32 + 7, 16777217, 255, 256],
    "uint32": [2 ** 32 - 1, 2 ** 31 + 1, 16777217, 2 ** 31 - 1, 256],
    "int16": [-2 ** 15, 2 ** 15 - 1, -1, 255, 256],
    "int8": [-128, 127, -1],
}


def legacy(dtype, c):
    return dtype in ("uint8", "float32") and c in (3, 4)


def plain(rng, dtype, hw, c):
    shape = hw + (c,)
    if dtype == "bool":
        return rng.integers(0, 2, shape).astype(bool)
    if dtype.startswith("float"):
        return rng.uniform(-60.0, 320.0, shape).astype(dtype)
    info = np.iinfo(dtype)
    v = rng.integers(max(int(info.min), -300), min(int(info.max), 600), shape, endpoint=True).astype(dtype)
    wide = rng.random(shape) < 0.15
    v[wide] = rng.integers(int(info.min), int(info.max), int(wide.sum()), endpoint=True, dtype=dtype)
    return v


def special(rng, dtype, hw, c):
    """Mostly special values; the texels around the origin (read by every masked pixel) special too, but finite in the legacy class."""
    v = plain(rng, dtype, hw, c)
    pool = np.array(SPECIAL[dtype], dtype=dtype)
    m = rng.random(v.shape) < 0.45
    m[:2, :2] = True
    v[m] = pool[rng.integers(0, pool.size, int(m.sum()))]
    if legacy(dtype, c):
        near = v[:2, :2]
        near[~np.isfinite(near)] = 7.25
    return v


def call(fn, img, case, z):
    """The reference's entry point -> (result array, mx, my)."""
    H, conv = case["H"], case["conv"]
    if fn == "wp":
        return ref_h.wrapPerspective(img, H, convert=conv, boundary=case["boundary"])
    if fn == "scan":
        return ref_h.wrapPerspectiveScan(img, H, case["res"], convert=conv)
    if fn == "tih":
        return ref_h.transformImageH(img, H, method=conv)
    if fn == "ti":
        return ref_h.transformImage(img, case["u"], case["v"], box=case["box"], method=conv), 0, 0
    if fn == "cf":
        mh, mw = case["res"]
        h, w = case["bound"]
        return ref_h.convertfunc[conv](z, img, h, w, mh, mw), 0, 0
    raise KeyError(fn)


def run(fn, img0, case, z0):
    img = img0.copy()
    z = None if z0 is None else z0.copy()
    try:
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
            r, mx, my = call(fn, img, case, z)
        outcome, out = "ok", np.asarray(r)
    except Exception as e:      # noqa: BLE001 -- the type is the datum
        outcome, out, mx, my = type(e).__name__, None, 0, 0
    rest = img.copy()
    rest[0, 0] = img0[0, 0]
    assert rest.tobytes() == img0.tobytes(), "more than texel (0,0) of the caller's image changed"
    return outcome, out, int(mx), int(my), img[0, 0].copy(), z


def corners(hw):
    h, w = hw
    return np.array([[0, w - 1, w - 1, 0], [0, 0, h - 1, h - 1], [1.0, 1, 1, 1]])


def main():
    rng = np.random.default_rng(21)
    pool, zpool = {}, {}

    def img(kind, dtype, hw, c):
        key = "%s_%s_%d_%dx%d" % (kind, dtype, c, hw[0], hw[1])
        if key not in pool:
            pool[key] = (special if kind == "sp" else plain)(rng, dtype, hw, c)
        return key

    def zkey(name, H, hw, res, edits=False):
        if name not in zpool:
            h, w = res
            x, y = np.linspace(-1.5, w + 0.5, w), np.linspace(-1.2, h + 0.7, h)
            xv, yv = np.meshgrid(x, y)
            z = np.dstack([xv, yv, np.ones((h, w))]).reshape([w * h, 3]).T
            z = np.linalg.inv(H) @ z
            z /= z[-1, :]
            if edits:                   # NaN coordinates (nn: masked) and coordinates on the last column / row
                z[0, 3] = np.nan
                z[1, 7] = np.nan
                z[0, 11], z[1, 11] = hw[1] - 1, 2.5
                z[0, 12], z[1, 12] = 2.5, hw[0] - 1
            zpool[name] = z
        return name

    base = dict(H=None, conv="nn", boundary=0, res=(0, 0), bound=(0, 0), u=None, v=None, box=None, z=None)
    cases = []      # (name, fn, image key, case dict)

    def add(name, fn, key, **kw):
        c = dict(base)
        c.update(kw)
        cases.append((name, fn, key, c))

    geo = list(SHIFTS)
    n = 0
    # 1. the dtype matrix on plain images: every entry point x every dtype x 3 / 4 / 5 channels
    for dt in DTYPES:
        for c in (3, 4, 5):
            hw = HWS[n % 2]
            k = img("pl", dt, hw, c)
            H = shifted(geo[n % len(geo)])
            h, w = hw
            u = corners(hw)
            v = u.copy()
            v[:2] += np.array([[1.2, 2.7, 3.1, 0.4], [0.6, 1.3, 2.2, 1.9]])
            add("mx_wp_nn_%s_c%d" % (dt, c), "wp", k, H=H, conv="nn")
            add("mx_wp_bil_%s_c%d" % (dt, c), "wp", k, H=H, conv="bilinear")
            add("mx_wp_bil_b1_%s_c%d" % (dt, c), "wp", k, H=shifted("left_up"), conv="bilinear", boundary=1)
            add("mx_wp_nn_b1_%s_c%d" % (dt, c), "wp", k, H=ROT, conv="nn", boundary=1)
            add("mx_scan_small_nn_%s_c%d" % (dt, c), "scan", k, H=H, conv="nn", res=(h - 3, w - 4))
            add("mx_scan_small_bil_%s_c%d" % (dt, c), "scan", k, H=ROT, conv="bilinear", res=(h - 2, w - 3))
            add("mx_scan_large_bil_%s_c%d" % (dt, c), "scan", k, H=H, conv="bilinear", res=(h + 3, w + 5))
            add("mx_scan_large_nn_%s_c%d" % (dt, c), "scan", k, H=H, conv="nn", res=(h + 2, w + 2))
            add("mx_tih_bil_%s_c%d" % (dt, c), "tih", k, H=H, conv="bilinear")
            add("mx_tih_nn_%s_c%d" % (dt, c), "tih", k, H=ROT, conv="nn")
            add("mx_ti_bil_%s_c%d" % (dt, c), "ti", k, u=u, v=v, conv="bilinear")
            add("mx_ti_box_nn_%s_c%d" % (dt, c), "ti", k, u=u, v=v, box=(h + 2, w + 3), conv="nn")
            add("mx_ti_box_bil_%s_c%d" % (dt, c), "ti", k, u=u, v=v, box=(h - 1, w - 2), conv="bilinear")
            n += 1
    # 2. special values: every dtype that has them x 3 / 4 / 5 channels
    for dt in SPECIAL:
        for c in (3, 4, 5):
            hw = HWS[n % 2]
            k = img("sp", dt, hw, c)
            H = shifted(geo[n % len(geo)])
            h, w = hw
            add("sp_wp_nn_%s_c%d" % (dt, c), "wp", k, H=H, conv="nn")
            add("sp_wp_bil_%s_c%d" % (dt, c), "wp", k, H=H, conv="bilinear")
            add("sp_scan_bil_%s_c%d" % (dt, c), "scan", k, H=ROT, conv="bilinear", res=(h + 1, w - 2))
            if not legacy(dt, c):       # uint8 outputs of values past int32: the any-dtype kernel only (see the docstring)
                add("sp_tih_bil_%s_c%d" % (dt, c), "tih", k, H=H, conv="bilinear")
                add("sp_tih_nn_%s_c%d" % (dt, c), "tih", k, H=ROT, conv="nn")
            n += 1
    # 3. 1 or 2 channels: the reference blanks channel 0 (and 1) of texel (0,0), then raises IndexError
    for i, dt in enumerate(DTYPES):
        for c in (1, 2):
            hw = HWS[i % 2]
            k = img("pl", dt, hw, c)
            fn = ("wp", "scan", "tih", "ti", "cf")[(i + c) % 5]
            conv = ("nn", "bilinear")[(i + c) % 2]
            h, w = hw
            u = corners(hw)
            add("c12_%s_%s_%s_c%d" % (fn, conv, dt, c), fn, k, H=shifted("inside"), conv=conv, res=(h, w), bound=(h, w), u=u, v=u + 1.0,
                z=zkey("z_inside_%dx%d" % hw, shifted("inside"), hw, (h, w)) if fn == "cf" else None)
    # 4. homographies that raise: identity (IndexError past the last column / row), singular (LinAlgError), NaN
    sing = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    nanH = np.array([[1.0, 0.0, np.nan], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    for i, dt in enumerate(("float64", "int64", "uint16", "float16", "bool", "int8", "uint64", "float32")):
        for c in (3, 5):
            hw = HWS[i % 2]
            h, w = hw
            k = img("pl", dt, hw, c)
            for conv in ("nn", "bilinear"):
                add("rz_ident_wp_%s_%s_c%d" % (conv, dt, c), "wp", k, H=np.eye(3), conv=conv)
                add("rz_sing_wp_%s_%s_c%d" % (conv, dt, c), "wp", k, H=sing, conv=conv)
                add("rz_nan_scan_%s_%s_c%d" % (conv, dt, c), "scan", k, H=nanH, conv=conv, res=(h, w))
            add("rz_ident_tih_%s_c%d" % (dt, c), "tih", k, H=np.eye(3), conv="bilinear")
    # 5. convertfunc on precomputed coordinates (bilinear zeroes the masked columns of the caller's z_t)
    for i, dt in enumerate(DTYPES):
        for c in (3, 4, 5):
            hw = HWS[i % 2]
            h, w = hw
            kind = "sp" if dt in SPECIAL and c != 4 else "pl"
            k = img(kind, dt, hw, c)
            zk = zkey("z_rot_%dx%d" % hw, ROT, hw, (h + 1, w - 1))
            add("cf_nn_%s_%s_c%d" % (kind, dt, c), "cf", k, conv="nn", res=(h + 1, w - 1), bound=(h, w), z=zk)
            add("cf_bil_%s_%s_c%d" % (kind, dt, c), "cf", k, conv="bilinear", res=(h + 1, w - 1), bound=(h, w), z=zk)
            ze = zkey("z_edits_%dx%d" % hw, shifted("inside"), hw, (h, w), edits=True)
            add("cf_edits_nn_%s_%s_c%d" % (kind, dt, c), "cf", k, conv="nn", res=(h, w), bound=(h, w), z=ze)
            add("cf_edits_bil_%s_%s_c%d" % (kind, dt, c), "cf", k, conv="bilinear", res=(h, w), bound=(h, w), z=ze)

    out = {"numpy_version": np.array(np.__version__)}
    for k, v in pool.items():
        out["img_" + k] = v
    for k, v in zpool.items():
        out["z_" + k] = v
    cols = {k: [] for k in ("names", "fn", "img", "H", "conv", "boundary", "res", "bound", "u", "v", "box", "zkey", "outcome", "out_dtype",
                            "out_shape", "out_off", "origin", "t00", "z_off")}
    flat, zflat, outcomes, off, zoff = [], [], {}, 0, 0
    for name, fn, key, c in cases:
        z0 = None if c["z"] is None else zpool[c["z"]]
        outcome, res, mx, my, t00, z = run(fn, pool[key], c, z0)
        row = np.zeros(64, np.uint8)                        # texel (0,0) of the caller's image after the call, its raw bytes
        row[:t00.nbytes] = np.frombuffer(t00.tobytes(), np.uint8)
        shape, dt = (0, 0, 0), ""
        if res is not None:
            shape, dt = res.shape, res.dtype.str
            assert res.ndim == 3, name
            b = np.frombuffer(np.ascontiguousarray(res).tobytes(), np.uint8)
            flat.append(b)
        zo = -1
        if z is not None:
            zo = zoff
            zflat.append(z.reshape(-1))
            zoff += z.size
        for k, v in (("names", name), ("fn", fn), ("img", key), ("H", c["H"] if c["H"] is not None else np.full((3, 3), np.nan)),
                     ("conv", c["conv"]), ("boundary", c["boundary"]), ("res", c["res"]), ("bound", c["bound"]),
                     ("u", c["u"] if c["u"] is not None else np.zeros((3, 4))), ("v", c["v"] if c["v"] is not None else np.zeros((3, 4))),
                     ("box", c["box"] if c["box"] is not None else (-1, -1)), ("zkey", c["z"] or ""), ("outcome", outcome),
                     ("out_dtype", dt), ("out_shape", shape), ("out_off", off), ("origin", (mx, my)), ("t00", row), ("z_off", zo)):
            cols[k].append(v)
        off += int(np.prod(shape)) * (np.dtype(dt).itemsize if dt else 0)
        outcomes[outcome] = outcomes.get(outcome, 0) + 1
    for k, v in cols.items():
        out[k] = np.array(v)
    out["out_flat"] = np.concatenate(flat)
    out["z_flat"] = np.concatenate(zflat)
    path = os.path.join(OUT, "g21_warp_dtypes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(cases), "cases", outcomes)


if __name__ == "__main__":
    main()
