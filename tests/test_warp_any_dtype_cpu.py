"""The any-dtype exact warp without a GPU: the oracle against the reference's recorded warps on every numeric dtype and 1 to 5
channels (g21), rwh_warp_plan's dispatch of the widened source domain, and the refusals and IndexErrors the public functions raise
before any device work."""
import ctypes

import numpy as np
import pytest

from g21_cases import g21_cases, oracle_api, public_api, run_case


def test_oracle_reproduces_g21():
    cases = g21_cases()
    assert len(cases) > 800
    assert {c["outcome"] for c in cases} == {"ok", "IndexError", "LinAlgError"}
    assert {c["img"].dtype.name for c in cases} == {"uint8", "int8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float16",
                                                    "float32", "float64", "bool"}
    assert {c["img"].shape[2] for c in cases} == {1, 2, 3, 4, 5}
    api = oracle_api()
    bad = {}
    for c in cases:
        b = run_case(api, c)
        if b:
            bad[c["name"]] = b
    assert not bad, bad


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ransac_with_homography_amd import _lib
    return _lib.load()


INV = np.linalg.inv(np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]]))


def _plan(lib, c, src, interp, dst, flags, hw=(2160, 3840)):
    from ransac_with_homography_amd import kernels
    g = kernels.Grid(5, 3775, 3771, 7, 2034, 2028)
    buf = ctypes.create_string_buffer(128)
    st = lib.rwh_warp_plan(hw[0], hw[1], c, src, 1, INV.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1, g.x0, g.step_x, g.x_last,
                           g.y0, g.step_y, g.y_last, g.out_h, g.out_w, hw[0], hw[1], interp, dst, 0, g.out_h, flags, buf, 128)
    return st, buf.value.decode()


def test_plan_names_the_any_dtype_kernel(lib):
    from ransac_with_homography_amd import _lib as L
    ex = L.RWH_WARP_EXACT
    nn, bil = L.RWH_NEAREST, L.RWH_BILINEAR
    # bilinear: one instance per source type, float64 or uint8 out; nearest: raw elements of the source's size
    assert _plan(lib, 3, L.RWH_F64, bil, L.RWH_F64, ex) == (0, "rwh::warp_any<double, double, 1>")
    assert _plan(lib, 3, L.RWH_F64, nn, L.RWH_F64, ex) == (0, "rwh::warp_any<unsigned long, unsigned long, 0>")
    assert _plan(lib, 3, L.RWH_I64, bil, L.RWH_U8, ex) == (0, "rwh::warp_any<long, unsigned char, 1>")
    assert _plan(lib, 4, L.RWH_U16, bil, L.RWH_F64, ex) == (0, "rwh::warp_any<unsigned short, double, 1>")
    assert _plan(lib, 3, L.RWH_U16, nn, L.RWH_U16, ex) == (0, "rwh::warp_any<unsigned short, unsigned short, 0>")
    assert _plan(lib, 3, L.RWH_F16, bil, L.RWH_F64, ex) == (0, "rwh::warp_any<_Float16, double, 1>")
    assert _plan(lib, 3, L.RWH_F16, nn, L.RWH_F16, ex) == (0, "rwh::warp_any<unsigned short, unsigned short, 0>")
    assert _plan(lib, 3, L.RWH_I32, nn, L.RWH_I32, ex) == (0, "rwh::warp_any<unsigned int, unsigned int, 0>")
    assert _plan(lib, 3, L.RWH_I8, bil, L.RWH_F64, ex) == (0, "rwh::warp_any<signed char, double, 1>")
    # uint8 / float32 with other than 3 or 4 channels: the any-dtype kernel; with 3 or 4: their kernels, unchanged
    assert _plan(lib, 1, L.RWH_U8, bil, L.RWH_F64, ex) == (0, "rwh::warp_any<unsigned char, double, 1>")
    assert _plan(lib, 5, L.RWH_F32, nn, L.RWH_F32, ex) == (0, "rwh::warp_any<unsigned int, unsigned int, 0>")
    assert _plan(lib, 1, L.RWH_F64, bil, L.RWH_F64, ex) == (0, "rwh::warp_any<double, double, 1>")
    assert _plan(lib, 64, L.RWH_U64, bil, L.RWH_F64, ex) == (0, "rwh::warp_any<unsigned long, double, 1>")
    assert _plan(lib, 3, L.RWH_U8, bil, L.RWH_F64, ex) == (0, "rwh::warp_exact<unsigned char, 3, double, 1>")
    assert _plan(lib, 4, L.RWH_F32, nn, L.RWH_F32, ex) == (0, "rwh::warp_exact<float, 4, float, 0>")
    # batches and row tiles go through the same kernel
    assert _plan(lib, 5, L.RWH_I16, bil, L.RWH_F64, ex, hw=(100, 120))[1] == "rwh::warp_any<short, double, 1>"


def test_plan_refuses_outside_the_domain(lib):
    from ransac_with_homography_amd import _lib as L
    ex = L.RWH_WARP_EXACT
    nn, bil = L.RWH_NEAREST, L.RWH_BILINEAR
    # the new codes without the exact flag: the fast / generic dispatch does not take them
    for code in (L.RWH_F64, L.RWH_I64, L.RWH_U16, L.RWH_F16, L.RWH_I8, L.RWH_U64):
        assert _plan(lib, 3, code, bil, L.RWH_F32, 0)[0] == -2
        assert _plan(lib, 3, code, nn, code, 0)[0] == -2
    assert _plan(lib, 5, L.RWH_U8, bil, L.RWH_U8, 0)[0] == -2 and _plan(lib, 1, L.RWH_F32, nn, L.RWH_F32, 0)[0] == -2
    # unknown codes, channel counts outside 1..RWH_WARP_MAX_CHANNELS, destinations the kernel does not write
    for code in (11, 99, -1):
        assert _plan(lib, 3, code, bil, L.RWH_F64, ex)[0] == -2
    assert _plan(lib, L.RWH_WARP_MAX_CHANNELS + 1, L.RWH_F64, bil, L.RWH_F64, ex)[0] == -2
    assert _plan(lib, 0, L.RWH_F64, bil, L.RWH_F64, ex)[0] == -2
    assert _plan(lib, 3, L.RWH_I64, nn, L.RWH_U64, ex)[0] == -2           # nearest: dst == src
    assert _plan(lib, 3, L.RWH_I64, bil, L.RWH_F32, ex)[0] == -2          # bilinear: F64 or U8
    # rwh_sample_points: the same domain (validation before any device access)
    one, null = ctypes.c_void_p(1), ctypes.c_void_p(0)
    sp = lambda c, code, interp, dst: lib.rwh_sample_points(one, 8, 8, c, code, one, one, 0, 8, 8, interp, one, dst, 0, null)
    assert sp(5, L.RWH_F64, bil, L.RWH_F64) == 0 and sp(1, L.RWH_F16, nn, L.RWH_F16) == 0
    assert sp(65, L.RWH_F64, bil, L.RWH_F64) == -2 and sp(3, 11, bil, L.RWH_F64) == -2 and sp(0, L.RWH_U8, nn, L.RWH_U8) == -2


def test_plan_maps_torch_dtypes(lib):
    import torch
    from ransac_with_homography_amd import kernels
    g = kernels.Grid(0, 99, 100, 0, 79, 80)
    plan = lambda shape, dt, interp, out, exact=True: kernels.warp_plan(shape, dt, INV, g, (80, 100), interp, out, exact=exact)
    assert plan((80, 100, 3), torch.float64, "bilinear", torch.float64) == "rwh::warp_any<double, double, 1>"
    assert plan((80, 100, 5), torch.bool, "nn", torch.bool) == "rwh::warp_any<unsigned char, unsigned char, 0>"
    assert plan((80, 100, 3), torch.bool, "bilinear", torch.float64) == "rwh::warp_exact<unsigned char, 3, double, 1>"
    assert plan((80, 100, 3), torch.uint16, "bilinear", torch.uint8) == "rwh::warp_any<unsigned short, unsigned char, 1>"
    assert plan((4, 80, 100, 7), torch.int64, "nn", torch.int64) == "rwh::warp_any<unsigned long, unsigned long, 0>"
    from ransac_with_homography_amd._lib import RwhError
    with pytest.raises(RwhError):                                  # the fast / generic kernels: uint8 / float32 sources only
        plan((80, 100, 3), torch.float64, "bilinear", torch.float32, exact=False)
    with pytest.raises(KeyError):                                  # (no element code for them there)
        plan((80, 100, 3), torch.uint16, "nn", torch.uint16, exact=False)


NON_NUMERIC = (np.complex128, np.complex64, np.longdouble, object, "U2", "datetime64[s]")


@pytest.mark.parametrize("dtype", NON_NUMERIC, ids=lambda d: np.dtype(d).name)
def test_non_numeric_images_refused_untouched(dtype):
    """Refused before any device work: these pass without a GPU (and without the library)."""
    import homography as hg
    base = np.arange(9 * 11 * 3).reshape(9, 11, 3)
    img = base.astype(dtype) if np.dtype(dtype).kind != "M" else base.astype("datetime64[s]")
    keep = img.copy()
    H = np.array([[1.0, 0.01, 1.5], [0.01, 1.0, 1.2], [1e-3, 1e-3, 1.0]])
    u = np.array([[0, 10, 10, 0], [0, 0, 8, 8], [1.0, 1, 1, 1]])
    z = np.vstack([np.linspace(0, 9, 20), np.linspace(0, 7, 20), np.ones(20)])
    calls = [lambda: hg.wrapPerspective(img, H, "nn"), lambda: hg.wrapPerspective(img, H, "bilinear"),
             lambda: hg.wrapPerspectiveScan(img, H, (9, 11), "bilinear"), lambda: hg.transformImageH(img, H),
             lambda: hg.transformImage(img, u, u + 1.0), lambda: hg.transformImage(img, u, u + 1.0, box=(9, 11), method="nn"),
             lambda: hg.convertfunc["nn"](z, img, 9, 11, 4, 5), lambda: hg.convertfunc["bilinear"](z, img, 9, 11, 4, 5)]
    for fn in calls:
        with pytest.raises(NotImplementedError):
            fn()
        assert np.array_equal(img, keep) if img.dtype != object else (img == keep).all()


def test_one_and_two_channels_blank_then_raise():
    """The g21 cases with 1 or 2 channels: the reference blanks channel 0 (and 1) of the caller's texel (0,0) and raises IndexError;
    the public functions do the same before any device work."""
    cases = [c for c in g21_cases() if c["img"].shape[2] < 3]
    assert len(cases) == 24 and {c["fn"] for c in cases} == {"wp", "scan", "tih", "ti", "cf"}
    api = public_api()
    bad = {}
    for c in cases:
        b = run_case(api, c)
        if b:
            bad[c["name"]] = b
    assert not bad, bad
