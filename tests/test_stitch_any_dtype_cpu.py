"""The any-dtype compositor without a GPU: the oracle against the reference's recorded stitchPanorama on non-uint8, RGBA and
1-channel images (g20), rwh_stitch_panorama_ex's exported symbol and argument validation, and the conversions of
csrc/rwh_cast.h (built with g++ through tests/cabi/stitch_cast_shim.cpp) against numpy's on about a million values."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from g20_cases import g20_cases, run_case
from oracle import rwh_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_reproduces_g20():
    cases = g20_cases()
    assert len(cases) > 400
    assert {c["outcome"] for c in cases} == {"ok", "IndexError", "ValueError"}
    bad = {}
    for c in cases:
        b = run_case(lambda q, t, H, bl, r: orc.stitch_panorama(q, t, H, blending=bl, blendrate=r), c)
        if b:
            bad[c["name"]] = b
    assert not bad, bad


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ransac_with_homography_amd import _lib
    return _lib.load()


def test_stitch_ex_exported_and_validates_abi5(lib):
    from ransac_with_homography_amd import _lib
    assert _lib.ABI_VERSION == 5 and lib.rwh_abi_version() == 5
    assert "rwh_stitch_panorama_ex" in _lib.EXPORTS
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert " rwh_stitch_panorama_ex" in nm
    ih = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(1)       # `one`: non-NULL, never dereferenced (validation comes first)

    def call(t=one, t_c=3, t_dt=_lib.RWH_F32, q=one, q_c=3, q_dt=_lib.RWH_U16, canvas=one, canvas_c=3, blend=0, rows=(0, 8), flags=0,
             h=ih, t_hw=(8, 8)):
        return lib.rwh_stitch_panorama_ex(t, t_hw[0], t_hw[1], t_c, t_dt, q, 8, 8, q_c, q_dt, h, 0, 0, 8, 8, 0, 0, 0, 0, 8, 8, canvas_c,
                                          blend, 0.2, canvas, rows[0], rows[1], flags, null)
    # RWH_E_INVALID: NULL pointers, unknown dtype codes, bad blend / flags / sizes / rows
    assert call(t=null) == -1 and call(q=null) == -1 and call(canvas=null) == -1
    assert call(h=ctypes.cast(null, ctypes.POINTER(ctypes.c_double))) == -1
    assert call(t_dt=11) == -1 and call(q_dt=-1) == -1 and call(t_dt=99) == -1
    assert call(blend=4) == -1 and call(blend=-1) == -1
    assert call(flags=_lib.RWH_STITCH_FAST) == -1 and call(flags=_lib.RWH_WARP_EXACT) == -1 and call(flags=1 << 7) == -1
    assert call(rows=(5, 4)) == -1 and call(rows=(0, 9)) == -1 and call(rows=(-1, 3)) == -1
    assert call(t_hw=(0, 8)) == -1
    # RWH_E_UNSUPPORTED: channel counts outside {3, 4} / {1, 3, 4}, a paste canvas that is not C_T wide, a paste imgQ that does not
    # broadcast, a blend canvas that is not 3 wide
    assert call(t_c=2) == -2 and call(t_c=5) == -2 and call(t_c=1) == -2
    assert call(q_c=2) == -2 and call(q_c=5) == -2
    assert call(t_c=4, q_c=4, canvas_c=3) == -2 and call(t_c=4, q_c=3, canvas_c=4) == -2 and call(t_c=3, q_c=4, canvas_c=3) == -2
    assert call(blend=1, t_c=4, q_c=4, canvas_c=4) == -2
    # valid arguments and an empty row range: nothing to launch (no GPU touched)
    for dt in range(11):
        assert call(t_dt=dt, q_dt=dt, rows=(3, 3)) == 0
    assert call(t_c=4, q_c=1, canvas_c=4, rows=(8, 8)) == 0 and call(blend=2, t_c=4, q_c=1, rows=(0, 0)) == 0
    # the uint8 entry points are unchanged
    assert lib.rwh_stitch_panorama(null, 8, 8, null, 8, 8, ih, 0, 0, 8, 8, 0, 0, 0, 0, 8, 8, 0, 0.2, null, 0, null) == -1


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cast_shim") / "stitch_cast_shim.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "ransac_with_homography_amd", "csrc"), os.path.join(ROOT, "tests", "cabi", "stitch_cast_shim.cpp"),
                    "-o", so], check=True)
    return ctypes.CDLL(so)


def _apply(shim, name, x, out_dtype):
    x = np.ascontiguousarray(x)
    y = np.empty(x.shape, out_dtype)
    getattr(shim, name)(ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(y.ctypes.data), ctypes.c_size_t(x.size))
    return y


def _edges64():
    """Every special value and the float64 / float32 neighbours of +-2^31, 0, 255, 256."""
    base = [0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 2.0 ** 32, 256.0, 255.0, -256.0, 0.5, -0.5, 255.5, 1.0,
            -1.0, 2.0 ** 63, -2.0 ** 63, 2.0 ** 64, 1e300, -1e300, 3.4028234663852886e38, 5e-324, 1e-45, 2.0 ** 24 + 1, 2.0 ** 53 + 1]
    v = []
    for b in base:
        v.append(b)
        for n in range(1, 4):
            for d in (np.inf, -np.inf):
                x64, x32 = b, np.float32(b)
                for _ in range(n):
                    x64 = np.nextafter(x64, d)
                    x32 = np.nextafter(x32, np.float32(d))
                v += [float(x64), float(x32)]
    return np.array(v, np.float64)


def test_cast_header_matches_numpy(shim):
    rng = np.random.default_rng(2020)
    n = 1 << 18
    with np.errstate(all="ignore"):
        f64 = np.concatenate([_edges64(), rng.uniform(-3e9, 3e9, n), rng.uniform(-600.0, 600.0, n), rng.normal(0, 1e6, n),
                              rng.standard_cauchy(n) * 1e10, (rng.integers(-2 ** 33, 2 ** 33, n)).astype(np.float64) + rng.choice([0.0, 0.5, -0.5], n),
                              rng.integers(0, 2 ** 64 - 1, n // 4, dtype=np.uint64).view(np.float64)])   # any bit pattern
        f32 = np.concatenate([f64.astype(np.float32), rng.integers(0, 2 ** 32 - 1, n, dtype=np.uint32).view(np.float32)])
        assert f64.size + f32.size > 10 ** 6
        i64 = np.concatenate([rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64, endpoint=True),
                              np.array([-2 ** 63, 2 ** 63 - 1, 2 ** 53 + 1, -(2 ** 53) - 1, 2 ** 24 + 1, -1, 0, 255, 256], np.int64),
                              (np.int64(2) ** rng.integers(0, 63, n)) + rng.integers(-3, 4, n)])
        u64 = np.concatenate([rng.integers(0, 2 ** 64 - 1, n, dtype=np.uint64, endpoint=True),
                              np.array([2 ** 64 - 1, 2 ** 63, 2 ** 63 + 2 ** 39 + 1, 2 ** 53 + 1, 0, 255], np.uint64)])
        # float -> uint8: astype and assignment into a uint8 array give the same bytes
        ref = f64.astype(np.uint8)
        assign = np.zeros(f64.size, np.uint8)
        assign[:] = f64
        assert np.array_equal(ref, assign)
        assert np.array_equal(_apply(shim, "shim_u8_of_f64", f64, np.uint8), ref)
        assert np.array_equal(_apply(shim, "shim_u8_of_f32", f32, np.uint8), f32.astype(np.uint8))
        assert np.array_equal(_apply(shim, "shim_u8_of_f32", f32.astype(np.float16).astype(np.float32), np.uint8),
                              f32.astype(np.float16).astype(np.uint8))
        assert np.array_equal(_apply(shim, "shim_u8_of_i64", i64, np.uint8), i64.astype(np.uint8))
        assert np.array_equal(_apply(shim, "shim_u8_of_u64", u64, np.uint8), u64.astype(np.uint8))
        assert np.array_equal(_apply(shim, "shim_u8_of_i64", i64.astype(np.int8).astype(np.int64), np.uint8), i64.astype(np.int8).astype(np.uint8))
        assert np.array_equal(_apply(shim, "shim_f32_of_i64", i64, np.float32), i64.astype(np.float32))
        assert np.array_equal(_apply(shim, "shim_f32_of_u64", u64, np.float32), u64.astype(np.float32))
        got = _apply(shim, "shim_f32_of_f64", f64, np.float32)
        want = f64.astype(np.float32)
        assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
        assert np.array_equal(np.isnan(got), np.isnan(want))
    # the spec's examples
    assert list(_apply(shim, "shim_u8_of_f64", np.array([300.7, -1.5, 70000, 2.0 ** 31 + 5, 1e10, np.nan]), np.uint8)) == [44, 255, 112, 0, 0, 0]


def test_still_refused_without_gpu():
    """5+ channels and non-numeric dtypes stay NotImplementedError, raised before any device work and before the caller's imgT is
    touched."""
    import torch
    import homography as hg
    H = np.array([[1.0, 0.01, 3.2], [0.01, 1.0, 2.1], [1e-4, 1e-4, 1.0]])
    q = np.full((6, 7, 3), 9.5, np.float32)
    for t in (np.full((6, 7, 5), 7.25, np.float32), np.full((6, 7, 6), 3, np.int16)):
        keep = t.copy()
        for blending in (False, "Rate"):
            with pytest.raises(NotImplementedError):
                hg.stitchPanorama(q, t, H, blending=blending)
            assert np.array_equal(t, keep)
    with pytest.raises(NotImplementedError):
        hg.stitchPanorama(np.full((6, 7, 5), 1.5), np.full((6, 7, 3), 1.5), H)
    with pytest.raises(NotImplementedError):
        hg.stitchPanorama(torch.full((6, 7, 3), 1.5, dtype=torch.bfloat16), torch.full((6, 7, 3), 2.5, dtype=torch.bfloat16), H)


def test_negative_int8_is_not_uint8_valued():
    """int8 survives a round trip through uint8 for every value, but -1 is no uint8 value: the reference's blend reads it as -1.0.
    Such images go to the any-dtype compositor; non-negative int8 keeps the uint8 path."""
    import torch
    from ransac_with_homography_amd import homography as impl
    neg = np.array([[[-1, 5, 7]]], np.int8)
    for img in (neg, torch.from_numpy(neg)):
        with pytest.raises(NotImplementedError):
            impl._as_uint8_image(img, "imgQ")
    assert impl._as_uint8_image(np.abs(neg), "imgQ").dtype == np.uint8
    assert impl._as_uint8_image(torch.from_numpy(np.abs(neg)), "imgQ").dtype == torch.uint8
