#!/usr/bin/env python3
"""Generate tests/golden/g20_stitch_dtypes.npz: the reference's stitchPanorama (homography.py:288-338) on images that are not
uint8 RGB -- every numeric dtype on both images, 4-channel and 1-channel images, 1- / 2-channel imgT, every channel mismatch,
special values (NaN, +-inf, fractions, values beyond int32 / float32), the identity H (IndexError from the warp) crossed with
the mismatches.

Imports the reference's unmodified homography.py the way make_golden.py does (an empty cv2 stub module) and writes data only.

Per case: the inputs (an index into the image pool), H, `blending`, `blendrate`; the outcome (the exception's type name, or
"ok"), the canvas (uint8 in every case the reference completes: shape and offset into `out_flat`), the raw bytes of texel (0,0) of
the caller's imgT after the call (`t00`; the generator asserts that nothing else of either caller array changes).

Usage:  python tests/golden/make_golden_g20.py
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
T_HW, Q_HW = (12, 16), (10, 14)
P = np.array([[1.0, 0.01, 0.0], [0.012, 0.99, 0.0], [2e-3, 1e-3, 1.0]])
SHIFTS = {"left_up": (-3.3, -2.6), "right_down": (4.7, 3.2), "inside": (1.4, 1.3), "left_down": (-4.2, 2.4), "right_up": (5.5, -2.3)}
BLENDINGS = {"paste": False, "rate": "Rate", "grad": "Gradient", "true": True}


def shifted(name):
    S = np.eye(3)
    S[0, 2], S[1, 2] = SHIFTS[name]
    return S @ P


def plain(rng, dtype, hw, c):
    """Values across the dtype's range, mostly inside and around 0..255."""
    shape = hw + (c,)
    if dtype == "bool":
        return rng.integers(0, 2, shape).astype(bool)
    if dtype.startswith("float"):
        v = rng.uniform(-60.0, 320.0, shape)
        return v.astype(dtype)
    info = np.iinfo(dtype)
    v = rng.integers(max(int(info.min), -300), min(int(info.max), 600), shape, endpoint=True).astype(dtype)
    wide = rng.random(shape) < 0.15                         # some values from the whole range
    v[wide] = rng.integers(int(info.min), int(info.max), int(wide.sum()), endpoint=True, dtype=dtype)
    return v


SPECIAL = {
    "float64": [np.nan, np.inf, -np.inf, -0.5, 255.5, 256.0, 2.0 ** 31 + 3, 2.0 ** 31 - 2, -2.0 ** 31 - 3, -2.0 ** 31 + 2, 2.0 ** 31,
                -2.0 ** 31, 1e39, -1e39, 1e300, 300.7, -1.5, 70000.0, 2.0 ** 53 + 2, -0.0],
    "float32": [np.nan, np.inf, -np.inf, -0.5, 255.5, 256.0, 2.0 ** 31 + 256, 2.0 ** 31 - 128, -2.0 ** 31 - 256, -2.0 ** 31 + 128, 2.0 ** 31,
                -2.0 ** 31, 3e38, 300.7, -1.5, 70000.0, -0.0],
    "float16": [np.nan, np.inf, -np.inf, -0.5, 255.5, 256.0, 65504.0, -65504.0, 300.7, -1.5, -0.0],
    "int32": [2 ** 31 - 1, 2 ** 31 - 3, -2 ** 31, -2 ** 31 + 3, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24) - 1, 16777217 * 3, 255, 256, -1],
    "int64": [2 ** 63 - 1, -2 ** 63, 2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53) - 1, 2 ** 31 + 5, -2 ** 31 - 5, 2 ** 60 + 2 ** 36 + 1, 2 ** 24 + 1, -1],
    "uint64": [2 ** 64 - 1, 2 ** 63 + 2 ** 39 + 1, 2 ** 53 + 1, 2 ** 32 + 7, 2 ** 24 + 1, 255, 256],
    "uint32": [2 ** 32 - 1, 2 ** 31 + 1, 2 ** 24 + 1, 2 ** 31 - 1, 256],
}


def special(rng, dtype, hw, c):
    """Mostly special values, the rest plain; the texels around the origin (read by every masked pixel) always special."""
    v = plain(rng, dtype, hw, c)
    pool = np.array(SPECIAL[dtype], dtype=dtype)
    m = rng.random(v.shape) < 0.45
    m[:2, :2] = True
    v[m] = pool[rng.integers(0, pool.size, int(m.sum()))]
    return v


def run(Q, T, H, blending, rate):
    q, t = Q.copy(), T.copy()
    try:
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
            r = ref_h.stitchPanorama(q, t, H, blending=blending, blendrate=rate)
        outcome, canvas = "ok", np.asarray(r)
    except Exception as e:      # noqa: BLE001 -- the type is the datum
        outcome, canvas = type(e).__name__, None
    rest = t.copy()
    rest[0, 0] = T[0, 0]
    t_rest_same = rest.tobytes() == T.tobytes()
    q_same = q.tobytes() == Q.tobytes()
    return outcome, canvas, t[0, 0].copy(), t_rest_same, q_same


def main():
    rng = np.random.default_rng(20)
    pool = {}

    def img(kind, dtype, hw, c):
        key = "%s_%s_%d_%dx%d" % (kind, dtype, c, hw[0], hw[1])
        if key not in pool:
            pool[key] = (special if kind == "sp" else plain)(rng, dtype, hw, c)
        return key

    cases = []      # (name, q_key, t_key, H, blending name)

    # 1. the dtype matrix: every blending x the channel pairs the reference composites x every dtype on imgT (imgQ's dtype rotated)
    pairs = {"paste": [(3, 3), (3, 1), (4, 4), (4, 1)], "blend": [(3, 1), (3, 3), (3, 4), (4, 1), (4, 3), (4, 4)]}
    geo = list(SHIFTS)
    n = 0
    for bn in BLENDINGS:
        for ct, cq in pairs["paste" if bn == "paste" else "blend"]:
            for i, dt in enumerate(DTYPES):
                dq = DTYPES[(i + 1 + n) % len(DTYPES)]
                g = geo[n % len(geo)]
                cases.append(("mx_%s_t%d%s_q%d%s_%s" % (bn, ct, dt, cq, dq, g), img("pl", dq, Q_HW, cq), img("pl", dt, T_HW, ct), shifted(g), bn))
                n += 1
    # 2. special values on both images
    for bn in BLENDINGS:
        for ct in (3, 4):
            for dt in SPECIAL:
                for dq in (dt, "float64" if dt != "float64" else "int64"):
                    cq = 1 if (n % 3 == 0) else ct
                    g = geo[n % len(geo)]
                    cases.append(("sp_%s_t%d%s_q%d%s_%s" % (bn, ct, dt, cq, dq, g), img("sp", dq, Q_HW, cq), img("sp", dt, T_HW, ct), shifted(g), bn))
                    n += 1
    # 3. imgT with 1 or 2 channels (IndexError while blanking; in blend after the warp for 2 channels)
    for bn in BLENDINGS:
        for ct in (1, 2):
            for cq in (1, 2, 3):
                dt = DTYPES[n % len(DTYPES)]
                cases.append(("c12_%s_t%d%s_q%d" % (bn, ct, dt, cq), img("pl", "float32", Q_HW, cq), img("pl", dt, T_HW, ct), shifted("inside"), bn))
                n += 1
    # 4. every channel pair of 3- / 4-channel imgT with a 1..4-channel imgQ (mismatches raise ValueError after the warp), and the
    #    identity H on the same pairs (IndexError from the warp first)
    for hn in ("inside", "identity"):
        H = np.eye(3) if hn == "identity" else shifted(hn)
        for bn in BLENDINGS:
            for ct in (3, 4):
                for cq in (1, 2, 3, 4):
                    dt = ("float32", "int16", "float64", "uint16")[n % 4]
                    cases.append(("mm_%s_%s_t%d%s_q%d" % (hn, bn, ct, dt, cq), img("pl", "float64", Q_HW, cq), img("pl", dt, T_HW, ct), H, bn))
                    n += 1

    out = {"numpy_version": np.array(np.__version__)}
    for k, v in pool.items():
        out["img_" + k] = v
    # per case, one row of each table; the canvases (all uint8) flat, one after the other
    cols = {"names": [], "q": [], "t": [], "H": [], "blending": [], "rate": [], "outcome": [], "t00": [], "out_shape": [], "out_off": []}
    flat, outcomes, off = [], {}, 0
    for name, qk, tk, H, bn in cases:
        rate = float(np.round(rng.uniform(0.1, 0.6), 3))
        outcome, canvas, t00, t_rest_same, q_same = run(pool[qk], pool[tk], H, BLENDINGS[bn], rate)
        assert t_rest_same and q_same, name
        row = np.zeros(32, np.uint8)                        # texel (0,0) of the caller's imgT after the call, its raw bytes
        row[:t00.nbytes] = np.frombuffer(t00.tobytes(), np.uint8)
        shape = (0, 0, 0)
        if canvas is not None:
            assert canvas.dtype == np.uint8 and canvas.ndim == 3, name
            shape = canvas.shape
            flat.append(canvas.reshape(-1))
        for k, v in (("names", name), ("q", qk), ("t", tk), ("H", H), ("blending", bn), ("rate", rate), ("outcome", outcome),
                     ("t00", row), ("out_shape", shape), ("out_off", off)):
            cols[k].append(v)
        off += int(np.prod(shape))
        outcomes[outcome] = outcomes.get(outcome, 0) + 1
    for k, v in cols.items():
        out[k] = np.array(v)
    out["out_flat"] = np.concatenate(flat)
    names = cols["names"]
    path = os.path.join(OUT, "g20_stitch_dtypes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB,", len(names), "cases", outcomes)


if __name__ == "__main__":
    main()
