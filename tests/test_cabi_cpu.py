"""CPU-only checks of the C ABI boundary: the library builds, loads, and exports every symbol
include/rwh.h declares; argument validation works without a GPU; the product refuses to compute
without one (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ransac_with_homography_amd import _lib
    return _lib.load()


def test_exports_match_header(lib):
    from ransac_with_homography_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rwh.h")).read()
    declared = set(re.findall(r"RWH_API\s+[\w\s\*]+?\b(rwh_\w+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS)
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.rwh_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define RWH_ABI_VERSION (\d+)", hdr).group(1))
    assert lib.rwh_strerror(-1) == b"invalid argument"


def test_argument_validation_without_gpu(lib):
    ih = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    null = ctypes.c_void_p(0)
    # NULL pointers -> RWH_E_INVALID before anything touches a device
    st = lib.rwh_warp_backward(null, 10, 10, 3, 0, 300, 1, ih, 1, 0., 1., 9., 0., 1., 9., 10, 10, 10, 10, 1,
                               null, 0, 300, 0, 10, 0, null)
    assert st == -1
    assert lib.rwh_dlt4_batched(null, null, 10, null, 4, null, null, null) == -1
    assert lib.rwh_score_count(null, null, null, 10, 4, 5.0, 0, 3, 0, null, null, null, null, null) == -1
    assert lib.rwh_project_points(null, null, 10, 0, null, null) == -1
    assert lib.rwh_ransac_search(null, null, 10, null, 4, 5.0, 0, 3, 0, null, null, null, null, null, 1, null) == -1
    assert lib.rwh_ransac_batched(null, null, null, 2, 10, 4, null, 0, 0, 5.0, 0, null, null, null, null, null, null, 0, null) == -1
    assert lib.rwh_stitch_panorama(null, 8, 8, null, 8, 8, ih, 0, 0, 8, 8, 0, 0, 0, 0, 8, 8, 0, 0.2, null, 0, null) == -1
    # n_h must be 1 or the batch size; bad row ranges; an empty row shard is a no-op even with NULL buffers
    one = ctypes.c_void_p(1)            # non-NULL, never dereferenced: validation comes first
    st = lib.rwh_warp_backward(one, 10, 10, 3, 0, 300, 3, ih, 2, 0., 1., 9., 0., 1., 9., 10, 10, 10, 10, 1, one, 0, 300, 0, 10, 0, null)
    assert st == -1
    st = lib.rwh_warp_backward(one, 10, 10, 3, 0, 300, 1, ih, 1, 0., 1., 9., 0., 1., 9., 10, 10, 10, 10, 1, one, 0, 300, 5, 4, 0, null)
    assert st == -1
    st = lib.rwh_warp_backward(null, 10, 10, 3, 0, 300, 1, ih, 1, 0., 1., 9., 0., 1., 9., 10, 10, 10, 10, 1, null, 0, 300, 4, 4, 0, null)
    assert st == 0
    # rwh_settle_decide (host only): NULL pointers, k < 0, slots that are not exactly 0 .. nset-1 -> RWH_E_INVALID before any callback
    from ransac_with_homography_amd import _lib
    calls = []
    iv = _lib.SETTLE_INTERVAL_FN(lambda *a: calls.append("iv") or 0)
    solve = _lib.SETTLE_SOLVE_FN(lambda *a: calls.append("solve") or 0)
    flags, pa, out = np.zeros(3, np.uint8), np.ones((3, 2), np.float32), np.zeros(5, np.int32)

    def decide(k=3, flags=flags.ctypes.data, counts=None, slot=None, pa=pa.ctypes.data, iv=iv, solve=solve, out=out.ctypes.data):
        cnt, sl = np.array([5, 9, 7], np.int32), np.array(slot if slot is not None else [-1, -1, -1], np.int32)
        return lib.rwh_settle_decide(k, flags, cnt.ctypes.data if counts is None else counts, sl.ctypes.data, pa, 3, 100, 0, 8,
                                     iv, solve, None, out)
    assert decide(k=-1) == -1 and decide(flags=None) == -1 and decide(counts=null) == -1 and decide(pa=None) == -1
    assert decide(iv=_lib.SETTLE_INTERVAL_FN()) == -1 and decide(solve=_lib.SETTLE_SOLVE_FN()) == -1 and decide(out=None) == -1   # (NULL callbacks)
    assert lib.rwh_settle_decide(3, flags.ctypes.data, out.ctypes.data, None, pa.ctypes.data, 3, 100, 0, 8, iv, solve, None,
                                 out.ctypes.data) == -1
    for bad in ([0, 0, -1], [1, -1, -1], [0, 2, -1], [-2, -1, -1], [3, -1, -1]):
        assert decide(slot=bad) == -1, bad
    assert calls == []
    # a valid call needs no GPU: the margin rule settles rows 1 and 2 in one round (the callback leaves their counts), row 1 wins
    assert decide(slot=[-1, -1, -1]) == 0 and out.tolist() == [1, 0, 9, 1, 0] and calls == ["solve"]


def test_round3_host_entry_points_without_gpu(lib):
    """rwh_ransac_run_layout (pure arithmetic), argument validation of rwh_ransac_run / rwh_host_dlt4_svd / rwh_lab_clock_probe,
    and the host solver itself -- rwh_host_dlt4_svd needs no GPU: it must reproduce the reference's H on golden samples."""
    from ransac_with_homography_amd import _lapack
    off = (ctypes.c_longlong * 27)()
    assert lib.rwh_ransac_run_layout(185, 1500, off, 27) == 27 and lib.rwh_ransac_run_layout(185, 1500, off, 22) == -1
    o = list(off)
    assert o[0] == 0 and all(b >= a for a, b in zip(o[:11], o[1:11])) and all(b >= a for a, b in zip(o[12:18], o[13:19]))
    assert o[5] == o[4] + 4 * 1500 and o[14] == o[13] + 4 * 1500            # counts and flags adjacent: one readback
    assert o[11] > 36 * 1500 * 3 and o[19] > 16 * 1500 + 36 * 1500
    assert o[10] < o[20] < o[11] and o[18] < o[21] < o[19]                  # the inverses of the settled rows: inside both workspaces
    assert o[20] < o[22] < o[23] < o[24] < o[11] and o[21] < o[25] < o[19] and o[26] == o[25] + 4 * 1500   # round 4: candidate rows, count intervals
    assert lib.rwh_ransac_run_layout(185, 1500, off, 21) == -1 and lib.rwh_ransac_run_layout(0, 10, off, 22) == -1
    null = ctypes.c_void_p(0)
    assert lib.rwh_ransac_run(null, null, 185, null, 10, 5.0, 0, 100, 8, null, null, 1, null, null, 0, null, null, null, null) == -1
    assert lib.rwh_score_interval(null, null, 4, null, null, null, 185, 5.0, 1000.0, 1e-6, 1e-5, null, null, null) == -1
    assert lib.rwh_host_dlt4_svd(null, null, 185, null, 4, null, 1, null) == -1
    assert lib.rwh_host_inv3(null, 4, null, null) == -1 and lib.rwh_score_count_inv(null, null, null, null, 4, 4, 1.0, 0, 1, 0, null, null, null, null, null) == -1
    assert lib.rwh_lab_clock_probe(null, 1.0, null) == -1
    addr = _lapack.dgesdd_address()
    if addr is None:
        pytest.skip("numpy's LAPACK symbol not found in this environment")
    g = np.load(os.path.join(ROOT, "tests", "golden", "g2_hyp_seed0.npz"))
    z = np.load(os.path.join(ROOT, "tests", "golden", "matchespoints.npz"))
    pa, pb = np.ascontiguousarray(z["ptsA"]), np.ascontiguousarray(z["ptsB"])
    idx = np.ascontiguousarray(g["idx"][:500], dtype=np.int32)
    out = np.empty((500, 9), np.float32)
    assert lib.rwh_host_dlt4_svd(pa.ctypes.data, pb.ctypes.data, 185, idx.ctypes.data, 500, ctypes.c_void_p(addr), 3, out.ctypes.data) == 0
    assert np.array_equal(out.view(np.uint32), g["H"][:500].view(np.uint32))
    bad = idx.copy(); bad[7, 2] = 185                                              # an index past the table: refused, nothing read
    assert lib.rwh_host_dlt4_svd(pa.ctypes.data, pb.ctypes.data, 185, bad.ctypes.data, 500, ctypes.c_void_p(addr), 3, out.ctypes.data) == -1
    # rwh_host_inv3 == numpy.linalg.inv on float32 3 x 3 matrices, bit for bit -- well-conditioned, pixel-scaled and nearly singular
    # ones (rank 2 plus 1e-9 .. 1e-3 of noise: where the kernels' own elimination and LAPACK's round apart)
    gesv = _lapack.dgesv_address()
    assert gesv is not None
    rng = np.random.default_rng(0)
    n = 5000
    well = (np.eye(3) + rng.normal(0, 0.3, (n, 3, 3))).astype(np.float32)
    u, v, w, x = (rng.normal(0, 1, sh) for sh in ((n, 3, 1), (n, 1, 3), (n, 3, 1), (n, 1, 3)))
    ill = (u @ v + w @ x + 10.0 ** rng.uniform(-9, -3, (n, 1, 1)) * rng.normal(0, 1, (n, 3, 3))).astype(np.float32)
    pix = well.copy(); pix[:, :2, 2] *= 300; pix[:, 2, :2] *= 1e-5
    for mats in (well, ill, pix, g["H"][:2000].reshape(-1, 3, 3).copy()):
        mats = np.ascontiguousarray(mats[np.isfinite(mats).all(axis=(1, 2))])
        got = np.empty_like(mats)
        assert lib.rwh_host_inv3(mats.ctypes.data, len(mats), ctypes.c_void_p(gesv), got.ctypes.data) == 0
        with np.errstate(all="ignore"):
            want = np.linalg.inv(mats)
        assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_new_entry_points_validate_and_plan(lib):
    """Round-2 entry points: NULL / bad arguments are refused before any device access, and rwh_warp_plan (the dispatch of
    rwh_warp_backward without the launch) names the kernel each configuration gets -- no GPU needed."""
    import torch
    from ransac_with_homography_amd import _lib, kernels
    null = ctypes.c_void_p(0)
    assert lib.rwh_sample_points(null, 8, 8, 3, 0, null, null, 4, 8, 8, 1, null, 2, 0, null) == -1
    assert lib.rwh_project_points_ex(null, null, 4, 2, null, null) == -1
    assert lib.rwh_lab_tune(_lib.RWH_TUNE_WARP_SHAPE, 9) == -1 and lib.rwh_lab_tune(_lib.RWH_TUNE_WARP_SHAPE, 0) == 0
    assert lib.rwh_lab_tune(_lib.RWH_TUNE_SCORE_HPW, 65) == -1 and lib.rwh_lab_tune(7, 0) == -1
    Hs = np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]])
    inv = np.linalg.inv(Hs)
    g = kernels.Grid(5, 3775, 3771, 7, 2034, 2028)
    plan = lambda shape, dt, *a, **k: kernels.warp_plan(shape, dt, inv, g, (2160, 3840), *a, **k)
    # a batch with one homography: the lab knob RWH_TUNE_WARP_FRAMES selects the multi-frame kernel (round 4; off by default)
    assert plan((32, 2160, 3840, 3), torch.uint8, "bilinear", torch.uint8) == "rwh::warp_rgb8_fast8<unsigned char, 6>"
    assert lib.rwh_lab_tune(_lib.RWH_TUNE_WARP_FRAMES, 65) == -1 and lib.rwh_lab_tune(_lib.RWH_TUNE_WARP_FRAMES, 4) == 0
    assert plan((32, 2160, 3840, 3), torch.uint8, "bilinear", torch.uint8) == "rwh::warp_rgb8_fast8m<6>"
    assert lib.rwh_lab_tune(_lib.RWH_TUNE_WARP_FRAMES, 0) == 0
    assert plan((2160, 3840, 3), torch.uint8, "bilinear", torch.uint8) == "rwh::warp_rgb8_fast8<unsigned char, 6>"
    assert plan((2160, 3840, 3), torch.uint8, "bilinear", torch.float32) == "rwh::warp_rgb8_fast8<float, 6>"
    assert plan((2160, 3840, 3), torch.uint8, "nn", torch.uint8) == "rwh::warp_rgb8_nn<6>"
    assert plan((2160, 3840, 3), torch.uint8, "bilinear", torch.float64, exact=True) == "rwh::warp_exact<unsigned char, 3, double, 1>"
    assert plan((2160, 3840, 4), torch.float32, "bilinear", torch.float32) == "rwh::warp_generic<float, 4, float, 1>"
    assert kernels.warp_plan((4, 2160, 3840, 3), torch.uint8, np.stack([inv] * 4), g, (2160, 3840), "bilinear",
                             torch.uint8) == "rwh::warp_rgb8_fast8_tab<unsigned char, 6>"
    # the shape is a function of the homography and the whole grid, never of the row shard
    assert plan((2160, 3840, 3), torch.uint8, "bilinear", torch.uint8, rows=(500, 700)) == "rwh::warp_rgb8_fast8<unsigned char, 6>"
    # a 30-degree rotation leaves the 64 x 8 window: 32 x 16 patches; an output narrower than 128 px: the 4 px kernel
    t = np.deg2rad(30)
    R = np.array([[np.cos(t), -np.sin(t), 100.0], [np.sin(t), np.cos(t), -50.0], [0, 0, 1.0]])
    assert kernels.warp_plan((2160, 3840, 3), torch.uint8, np.linalg.inv(R), g, (2160, 3840), "bilinear",
                             torch.uint8) == "rwh::warp_rgb8_fast8<unsigned char, 5>"
    assert kernels.warp_plan((100, 100, 3), torch.uint8, inv, kernels.Grid(0, 99, 100, 0, 99, 100), (100, 100), "bilinear",
                             torch.uint8) == "rwh::warp_rgb8_fast<unsigned char>"


def _plan_sweep_rows():
    """(key, thunk) per configuration of the plan sweep; thunk() -> the planned kernel name, or the status the library refuses with."""
    import torch
    from ransac_with_homography_amd import _lib, kernels
    SH, SW = 2160, 3840

    def zoom(s, deg=0.0):            # minification s (and a rotation) about the image centre
        t = np.deg2rad(deg)
        c, s_, cx, cy = np.cos(t) / s, np.sin(t) / s, (SW - 1) / 2, (SH - 1) / 2
        return np.array([[c, -s_, cx - c * cx + s_ * cy], [s_, c, cy - s_ * cx - c * cy], [0, 0, 1.0]])
    t30 = np.deg2rad(30)
    HOMS = {"HS": np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]]),      # bench.py's H_S
            "rot30": np.array([[np.cos(t30), -np.sin(t30), 100.0], [np.sin(t30), np.cos(t30), -50.0], [0, 0, 1.0]]),
            "rot90": zoom(1.0, 90.0), "min1.5": zoom(1.5), "min1.9": zoom(1.9), "min2": zoom(2.0), "min3": zoom(3.0),
            "scale1.5": np.diag([1 / 1.5, 1 / 1.5, 1.0]), "scale2": np.diag([0.5, 0.5, 1.0]), "scale3": np.diag([1 / 3.0, 1 / 3.0, 1.0])}
    INV = {k: np.linalg.inv(h) for k, h in HOMS.items()}
    MIXED = ["HS", "min1.5", "rot30", "min2", "min3", "rot90"]      # a per-image batch cycles through these: several shapes
    DT = {"u8": torch.uint8, "f32": torch.float32, "f64": torch.float64, "bool": torch.bool, "i8": torch.int8, "u16": torch.uint16,
          "i16": torch.int16, "i32": torch.int32, "u32": torch.uint32, "i64": torch.int64, "u64": torch.uint64, "f16": torch.float16}
    assert set(DT.values()) == set(kernels.STITCH_DTYPE)
    WIDTHS = (100, 127, 128, 255, 256, 257, 272, 273, 3771)

    def row(tag, src, c, interp, out, ow=3771, hom="HS", batch=1, per_image=None, rows=None, exact=False, tune=None):
        key = "|".join(str(v) for v in (tag, src, c, interp, out, ow, hom, batch, per_image or "-", "shard" if rows else "-",
                                        "exact" if exact else "-", "%s=%d" % tune if tune else "-"))

        def thunk():
            lib = _lib.load()
            inv = INV[hom] if not per_image else np.stack([INV[MIXED[i % len(MIXED)] if per_image == "mixed" else hom] for i in range(batch)])
            # ow columns of bench.py's 2028-row grid; ow None: the frame scaled by 1 / s on its own (SW / s) x (SH / s) grid
            s = float(hom[5:]) if ow is None else 0.0
            grid = kernels.Grid(5, 5 + ow - 1, ow, 7, 2034, 2028) if ow else kernels.Grid(0, int(SW / s) - 1, int(SW / s), 0, int(SH / s) - 1, int(SH / s))
            if tune: assert lib.rwh_lab_tune(getattr(_lib, "RWH_TUNE_WARP_" + tune[0]), tune[1]) == 0
            try:
                return kernels.warp_plan((batch, SH, SW, c), DT[src], inv, grid, (SH, SW), interp, DT[out], rows=rows, exact=exact)
            except _lib.RwhError as e:
                return int(re.search(r"\((-?\d+)\)$", str(e)).group(1))
            finally:
                if tune: assert lib.rwh_lab_tune(getattr(_lib, "RWH_TUNE_WARP_" + tune[0]), 0) == 0
        return key, thunk

    # A: the default mode on H_S -- every width for 3 and 4 channels; channel counts only the exact mode takes are refused
    for src in ("u8", "f32"):
        for interp in ("nn", "bilinear"):
            for out in ("u8", "f32", "f64"):
                for c in (3, 4):
                    for ow in (WIDTHS if out != "f64" else (3771,)): yield row("A", src, c, interp, out, ow)
                for c in (1, 5, 64): yield row("A", src, c, interp, out)
    # B: other homographies (rotations, minification: the patch shapes and the halves form)
    for hom in ("rot30", "rot90", "min1.5", "min1.9", "min2", "min3"):
        for c in (3, 4):
            for interp in ("nn", "bilinear"):
                for out in ("u8", "f32"):
                    for ow in (257, 3771): yield row("B", "u8", c, interp, out, ow, hom)
    for hom in ("scale1.5", "scale2", "scale3"):
        for c, interp, out, batch, per in ((3, "bilinear", "u8", 1, None), (3, "bilinear", "f32", 1, None), (3, "nn", "u8", 1, None),
                                           (4, "bilinear", "u8", 1, None), (3, "bilinear", "u8", 4, "same")):
            yield row("B", "u8", c, interp, out, None, hom, batch, per)
    # C: the exact mode, every element type and channel count (nn: the source's type out; bilinear: float64 or uint8)
    for src in DT:
        for c in (1, 3, 4, 5, 64):
            yield row("C", src, c, "nn", src, exact=True)
            yield row("C", src, c, "bilinear", "f64", exact=True)
            yield row("C", src, c, "bilinear", "u8", exact=True)
    for src, out in (("i16", "f64"), ("u8", "f32"), ("f32", "u8")): yield row("C", src, 3, "nn", out, exact=True)       # refused
    for ow in (100, 128): yield row("C", "u8", 3, "nn", "u8", ow, exact=True)
    yield row("C", "f32", 5, "bilinear", "f32", exact=True)                                                           # refused
    # D: batches with one homography, and with one per image (the same for all; mixed: different shapes in one call)
    for batch in (1, 4, 32):
        for per in (None, "same", "mixed"):
            for interp in ("nn", "bilinear"):
                for out in ("u8", "f32"):
                    for c, widths in ((3, (100, 257, 3771)), (4, (100, 3771))):
                        for ow in widths: yield row("D", "u8", c, interp, out, ow, "HS", batch, per)
            for hom in ("min1.5", "rot30"): yield row("D", "u8", 3, "bilinear", "u8", 3771, hom, batch, per)
            yield row("D", "f32", 3, "bilinear", "f32", 3771, "HS", batch, per)
            yield row("D", "i16", 5, "bilinear", "f64", 3771, "HS", batch, per, exact=True)
            yield row("D", "u8", 3, "bilinear", "f64", 3771, "HS", batch, per, exact=True)
    # E: a row shard plans what the whole grid plans
    for hom in ("HS", "rot30", "min1.5"):
        for interp, out in (("bilinear", "u8"), ("bilinear", "f32"), ("nn", "u8")):
            yield row("E", "u8", 3, interp, out, 3771, hom, rows=(500, 700))
            yield row("E", "u8", 3, interp, out, 3771, hom, 4, "mixed", rows=(500, 700))
    yield row("E", "u8", 4, "bilinear", "u8", 3771, "HS", rows=(500, 700))
    yield row("E", "f32", 3, "bilinear", "f32", 3771, "HS", rows=(500, 700))
    # F: the lab knobs the GPU tests set
    for shape in (0, 5, 6, 7, 13, 14):
        for hom in ("HS", "min1.5"):
            for c, interp, out, batch, per in ((3, "bilinear", "u8", 1, None), (3, "bilinear", "f32", 1, None), (3, "nn", "u8", 1, None),
                                               (4, "bilinear", "u8", 1, None), (3, "bilinear", "u8", 4, "same"), (3, "nn", "u8", 4, "same"),
                                               (3, "bilinear", "u8", 4, "mixed"), (3, "bilinear", "f32", 4, "same")):
                yield row("F", "u8", c, interp, out, 3771, hom, batch, per, tune=("SHAPE", shape))
        yield row("F", "u8", 3, "bilinear", "u8", 100, "HS", tune=("SHAPE", shape))
    for frames in (0, 1, 4, 104):
        for batch in (1, 4, 32):
            for hom in ("HS", "min1.5", "min3"):
                for c, interp, out, per in ((3, "bilinear", "u8", None), (3, "bilinear", "f32", None), (3, "nn", "u8", None),
                                            (4, "bilinear", "u8", None), (3, "bilinear", "u8", "same")):
                    yield row("F", "u8", c, interp, out, 3771, hom, batch, per, tune=("FRAMES", frames))
            yield row("F", "u8", 3, "bilinear", "u8", 272, "HS", batch, tune=("FRAMES", frames))
            yield row("F", "u8", 3, "bilinear", "u8", 100, "HS", batch, tune=("FRAMES", frames))


_PLAN_SWEEP = {      # planned kernel name (or refusal status) -> the rows of _plan_sweep_rows() that get it
    "rwh::warp_generic<unsigned char, 3, unsigned char, 0>": (
        "A|u8|3|nn|u8|100|HS|1|-|-|-|- A|u8|3|nn|u8|127|HS|1|-|-|-|- D|u8|3|nn|u8|100|HS|1|-|-|-|- D|u8|3|nn|u8|100|HS|1|same|-|-|- "
        "D|u8|3|nn|u8|100|HS|1|mixed|-|-|- D|u8|3|nn|u8|100|HS|4|-|-|-|- D|u8|3|nn|u8|100|HS|4|same|-|-|- "
        "D|u8|3|nn|u8|100|HS|4|mixed|-|-|- D|u8|3|nn|u8|100|HS|32|-|-|-|- D|u8|3|nn|u8|100|HS|32|same|-|-|- "
        "D|u8|3|nn|u8|100|HS|32|mixed|-|-|- "),
    "rwh::warp_rgb8_nn<6>": (
        "A|u8|3|nn|u8|128|HS|1|-|-|-|- A|u8|3|nn|u8|255|HS|1|-|-|-|- A|u8|3|nn|u8|256|HS|1|-|-|-|- A|u8|3|nn|u8|257|HS|1|-|-|-|- "
        "A|u8|3|nn|u8|272|HS|1|-|-|-|- A|u8|3|nn|u8|273|HS|1|-|-|-|- A|u8|3|nn|u8|3771|HS|1|-|-|-|- "
        "C|u8|3|nn|u8|3771|HS|1|-|-|exact|- C|bool|3|nn|bool|3771|HS|1|-|-|exact|- C|u8|3|nn|u8|128|HS|1|-|-|exact|- "
        "D|u8|3|nn|u8|257|HS|1|-|-|-|- D|u8|3|nn|u8|3771|HS|1|-|-|-|- D|u8|3|nn|u8|257|HS|1|same|-|-|- "
        "D|u8|3|nn|u8|3771|HS|1|same|-|-|- D|u8|3|nn|u8|257|HS|1|mixed|-|-|- D|u8|3|nn|u8|3771|HS|1|mixed|-|-|- "
        "D|u8|3|nn|u8|257|HS|4|-|-|-|- D|u8|3|nn|u8|3771|HS|4|-|-|-|- D|u8|3|nn|u8|257|HS|32|-|-|-|- D|u8|3|nn|u8|3771|HS|32|-|-|-|- "
        "E|u8|3|nn|u8|3771|HS|1|-|shard|-|- F|u8|3|nn|u8|3771|HS|1|-|-|-|SHAPE=0 F|u8|3|nn|u8|3771|HS|1|-|-|-|SHAPE=6 "
        "F|u8|3|nn|u8|3771|min1.5|1|-|-|-|SHAPE=6 F|u8|3|nn|u8|3771|HS|1|-|-|-|FRAMES=0 F|u8|3|nn|u8|3771|HS|4|-|-|-|FRAMES=0 "
        "F|u8|3|nn|u8|3771|HS|32|-|-|-|FRAMES=0 F|u8|3|nn|u8|3771|HS|1|-|-|-|FRAMES=1 F|u8|3|nn|u8|3771|HS|4|-|-|-|FRAMES=1 "
        "F|u8|3|nn|u8|3771|HS|32|-|-|-|FRAMES=1 F|u8|3|nn|u8|3771|HS|1|-|-|-|FRAMES=4 F|u8|3|nn|u8|3771|HS|4|-|-|-|FRAMES=4 "
        "F|u8|3|nn|u8|3771|HS|32|-|-|-|FRAMES=4 F|u8|3|nn|u8|3771|HS|1|-|-|-|FRAMES=104 F|u8|3|nn|u8|3771|HS|4|-|-|-|FRAMES=104 "
        "F|u8|3|nn|u8|3771|HS|32|-|-|-|FRAMES=104 "),
    "rwh::warp_generic<unsigned char, 4, unsigned char, 0>": (
        "A|u8|4|nn|u8|100|HS|1|-|-|-|- A|u8|4|nn|u8|127|HS|1|-|-|-|- A|u8|4|nn|u8|128|HS|1|-|-|-|- A|u8|4|nn|u8|255|HS|1|-|-|-|- "
        "A|u8|4|nn|u8|256|HS|1|-|-|-|- A|u8|4|nn|u8|257|HS|1|-|-|-|- A|u8|4|nn|u8|272|HS|1|-|-|-|- A|u8|4|nn|u8|273|HS|1|-|-|-|- "
        "A|u8|4|nn|u8|3771|HS|1|-|-|-|- B|u8|4|nn|u8|257|rot30|1|-|-|-|- B|u8|4|nn|u8|3771|rot30|1|-|-|-|- "
        "B|u8|4|nn|u8|257|rot90|1|-|-|-|- B|u8|4|nn|u8|3771|rot90|1|-|-|-|- B|u8|4|nn|u8|257|min1.5|1|-|-|-|- "
        "B|u8|4|nn|u8|3771|min1.5|1|-|-|-|- B|u8|4|nn|u8|257|min1.9|1|-|-|-|- B|u8|4|nn|u8|3771|min1.9|1|-|-|-|- "
        "B|u8|4|nn|u8|257|min2|1|-|-|-|- B|u8|4|nn|u8|3771|min2|1|-|-|-|- B|u8|4|nn|u8|257|min3|1|-|-|-|- "
        "B|u8|4|nn|u8|3771|min3|1|-|-|-|- D|u8|4|nn|u8|100|HS|1|-|-|-|- D|u8|4|nn|u8|3771|HS|1|-|-|-|- "
        "D|u8|4|nn|u8|100|HS|1|same|-|-|- D|u8|4|nn|u8|3771|HS|1|same|-|-|- D|u8|4|nn|u8|100|HS|1|mixed|-|-|- "
        "D|u8|4|nn|u8|3771|HS|1|mixed|-|-|- D|u8|4|nn|u8|100|HS|4|-|-|-|- D|u8|4|nn|u8|3771|HS|4|-|-|-|- "
        "D|u8|4|nn|u8|100|HS|4|same|-|-|- D|u8|4|nn|u8|3771|HS|4|same|-|-|- D|u8|4|nn|u8|100|HS|4|mixed|-|-|- "
        "D|u8|4|nn|u8|3771|HS|4|mixed|-|-|- D|u8|4|nn|u8|100|HS|32|-|-|-|- D|u8|4|nn|u8|3771|HS|32|-|-|-|- "
        "D|u8|4|nn|u8|100|HS|32|same|-|-|- D|u8|4|nn|u8|3771|HS|32|same|-|-|- D|u8|4|nn|u8|100|HS|32|mixed|-|-|- "
        "D|u8|4|nn|u8|3771|HS|32|mixed|-|-|- "),
    -2: (
        "A|u8|1|nn|u8|3771|HS|1|-|-|-|- A|u8|5|nn|u8|3771|HS|1|-|-|-|- A|u8|64|nn|u8|3771|HS|1|-|-|-|- A|u8|3|nn|f32|100|HS|1|-|-|-|- "
        "A|u8|3|nn|f32|127|HS|1|-|-|-|- A|u8|3|nn|f32|128|HS|1|-|-|-|- A|u8|3|nn|f32|255|HS|1|-|-|-|- A|u8|3|nn|f32|256|HS|1|-|-|-|- "
        "A|u8|3|nn|f32|257|HS|1|-|-|-|- A|u8|3|nn|f32|272|HS|1|-|-|-|- A|u8|3|nn|f32|273|HS|1|-|-|-|- A|u8|3|nn|f32|3771|HS|1|-|-|-|- "
        "A|u8|4|nn|f32|100|HS|1|-|-|-|- A|u8|4|nn|f32|127|HS|1|-|-|-|- A|u8|4|nn|f32|128|HS|1|-|-|-|- A|u8|4|nn|f32|255|HS|1|-|-|-|- "
        "A|u8|4|nn|f32|256|HS|1|-|-|-|- A|u8|4|nn|f32|257|HS|1|-|-|-|- A|u8|4|nn|f32|272|HS|1|-|-|-|- A|u8|4|nn|f32|273|HS|1|-|-|-|- "
        "A|u8|4|nn|f32|3771|HS|1|-|-|-|- A|u8|1|nn|f32|3771|HS|1|-|-|-|- A|u8|5|nn|f32|3771|HS|1|-|-|-|- "
        "A|u8|64|nn|f32|3771|HS|1|-|-|-|- A|u8|3|nn|f64|3771|HS|1|-|-|-|- A|u8|4|nn|f64|3771|HS|1|-|-|-|- "
        "A|u8|1|nn|f64|3771|HS|1|-|-|-|- A|u8|5|nn|f64|3771|HS|1|-|-|-|- A|u8|64|nn|f64|3771|HS|1|-|-|-|- "
        "A|u8|1|bilinear|u8|3771|HS|1|-|-|-|- A|u8|5|bilinear|u8|3771|HS|1|-|-|-|- A|u8|64|bilinear|u8|3771|HS|1|-|-|-|- "
        "A|u8|1|bilinear|f32|3771|HS|1|-|-|-|- A|u8|5|bilinear|f32|3771|HS|1|-|-|-|- A|u8|64|bilinear|f32|3771|HS|1|-|-|-|- "
        "A|u8|3|bilinear|f64|3771|HS|1|-|-|-|- A|u8|4|bilinear|f64|3771|HS|1|-|-|-|- A|u8|1|bilinear|f64|3771|HS|1|-|-|-|- "
        "A|u8|5|bilinear|f64|3771|HS|1|-|-|-|- A|u8|64|bilinear|f64|3771|HS|1|-|-|-|- A|f32|3|nn|u8|100|HS|1|-|-|-|- "
        "A|f32|3|nn|u8|127|HS|1|-|-|-|- A|f32|3|nn|u8|128|HS|1|-|-|-|- A|f32|3|nn|u8|255|HS|1|-|-|-|- A|f32|3|nn|u8|256|HS|1|-|-|-|- "
        "A|f32|3|nn|u8|257|HS|1|-|-|-|- A|f32|3|nn|u8|272|HS|1|-|-|-|- A|f32|3|nn|u8|273|HS|1|-|-|-|- A|f32|3|nn|u8|3771|HS|1|-|-|-|- "
        "A|f32|4|nn|u8|100|HS|1|-|-|-|- A|f32|4|nn|u8|127|HS|1|-|-|-|- A|f32|4|nn|u8|128|HS|1|-|-|-|- A|f32|4|nn|u8|255|HS|1|-|-|-|- "
        "A|f32|4|nn|u8|256|HS|1|-|-|-|- A|f32|4|nn|u8|257|HS|1|-|-|-|- A|f32|4|nn|u8|272|HS|1|-|-|-|- A|f32|4|nn|u8|273|HS|1|-|-|-|- "
        "A|f32|4|nn|u8|3771|HS|1|-|-|-|- A|f32|1|nn|u8|3771|HS|1|-|-|-|- A|f32|5|nn|u8|3771|HS|1|-|-|-|- "
        "A|f32|64|nn|u8|3771|HS|1|-|-|-|- A|f32|1|nn|f32|3771|HS|1|-|-|-|- A|f32|5|nn|f32|3771|HS|1|-|-|-|- "
        "A|f32|64|nn|f32|3771|HS|1|-|-|-|- A|f32|3|nn|f64|3771|HS|1|-|-|-|- A|f32|4|nn|f64|3771|HS|1|-|-|-|- "
        "A|f32|1|nn|f64|3771|HS|1|-|-|-|- A|f32|5|nn|f64|3771|HS|1|-|-|-|- A|f32|64|nn|f64|3771|HS|1|-|-|-|- "
        "A|f32|1|bilinear|u8|3771|HS|1|-|-|-|- A|f32|5|bilinear|u8|3771|HS|1|-|-|-|- A|f32|64|bilinear|u8|3771|HS|1|-|-|-|- "
        "A|f32|1|bilinear|f32|3771|HS|1|-|-|-|- A|f32|5|bilinear|f32|3771|HS|1|-|-|-|- A|f32|64|bilinear|f32|3771|HS|1|-|-|-|- "
        "A|f32|3|bilinear|f64|3771|HS|1|-|-|-|- A|f32|4|bilinear|f64|3771|HS|1|-|-|-|- A|f32|1|bilinear|f64|3771|HS|1|-|-|-|- "
        "A|f32|5|bilinear|f64|3771|HS|1|-|-|-|- A|f32|64|bilinear|f64|3771|HS|1|-|-|-|- B|u8|3|nn|f32|257|rot30|1|-|-|-|- "
        "B|u8|3|nn|f32|3771|rot30|1|-|-|-|- B|u8|4|nn|f32|257|rot30|1|-|-|-|- B|u8|4|nn|f32|3771|rot30|1|-|-|-|- "
        "B|u8|3|nn|f32|257|rot90|1|-|-|-|- B|u8|3|nn|f32|3771|rot90|1|-|-|-|- B|u8|4|nn|f32|257|rot90|1|-|-|-|- "
        "B|u8|4|nn|f32|3771|rot90|1|-|-|-|- B|u8|3|nn|f32|257|min1.5|1|-|-|-|- B|u8|3|nn|f32|3771|min1.5|1|-|-|-|- "
        "B|u8|4|nn|f32|257|min1.5|1|-|-|-|- B|u8|4|nn|f32|3771|min1.5|1|-|-|-|- B|u8|3|nn|f32|257|min1.9|1|-|-|-|- "
        "B|u8|3|nn|f32|3771|min1.9|1|-|-|-|- B|u8|4|nn|f32|257|min1.9|1|-|-|-|- B|u8|4|nn|f32|3771|min1.9|1|-|-|-|- "
        "B|u8|3|nn|f32|257|min2|1|-|-|-|- B|u8|3|nn|f32|3771|min2|1|-|-|-|- B|u8|4|nn|f32|257|min2|1|-|-|-|- "
        "B|u8|4|nn|f32|3771|min2|1|-|-|-|- B|u8|3|nn|f32|257|min3|1|-|-|-|- B|u8|3|nn|f32|3771|min3|1|-|-|-|- "
        "B|u8|4|nn|f32|257|min3|1|-|-|-|- B|u8|4|nn|f32|3771|min3|1|-|-|-|- C|i16|3|nn|f64|3771|HS|1|-|-|exact|- "
        "C|u8|3|nn|f32|3771|HS|1|-|-|exact|- C|f32|3|nn|u8|3771|HS|1|-|-|exact|- C|f32|5|bilinear|f32|3771|HS|1|-|-|exact|- "
        "D|u8|3|nn|f32|100|HS|1|-|-|-|- D|u8|3|nn|f32|257|HS|1|-|-|-|- D|u8|3|nn|f32|3771|HS|1|-|-|-|- D|u8|4|nn|f32|100|HS|1|-|-|-|- "
        "D|u8|4|nn|f32|3771|HS|1|-|-|-|- D|u8|3|nn|f32|100|HS|1|same|-|-|- D|u8|3|nn|f32|257|HS|1|same|-|-|- "
        "D|u8|3|nn|f32|3771|HS|1|same|-|-|- D|u8|4|nn|f32|100|HS|1|same|-|-|- D|u8|4|nn|f32|3771|HS|1|same|-|-|- "
        "D|u8|3|nn|f32|100|HS|1|mixed|-|-|- D|u8|3|nn|f32|257|HS|1|mixed|-|-|- D|u8|3|nn|f32|3771|HS|1|mixed|-|-|- "
        "D|u8|4|nn|f32|100|HS|1|mixed|-|-|- D|u8|4|nn|f32|3771|HS|1|mixed|-|-|- D|u8|3|nn|f32|100|HS|4|-|-|-|- "
        "D|u8|3|nn|f32|257|HS|4|-|-|-|- D|u8|3|nn|f32|3771|HS|4|-|-|-|- D|u8|4|nn|f32|100|HS|4|-|-|-|- "
        "D|u8|4|nn|f32|3771|HS|4|-|-|-|- D|u8|3|nn|f32|100|HS|4|same|-|-|- D|u8|3|nn|f32|257|HS|4|same|-|-|- "
        "D|u8|3|nn|f32|3771|HS|4|same|-|-|- D|u8|4|nn|f32|100|HS|4|same|-|-|- D|u8|4|nn|f32|3771|HS|4|same|-|-|- "
        "D|u8|3|nn|f32|100|HS|4|mixed|-|-|- D|u8|3|nn|f32|257|HS|4|mixed|-|-|- D|u8|3|nn|f32|3771|HS|4|mixed|-|-|- "
        "D|u8|4|nn|f32|100|HS|4|mixed|-|-|- D|u8|4|nn|f32|3771|HS|4|mixed|-|-|- D|u8|3|nn|f32|100|HS|32|-|-|-|- "
        "D|u8|3|nn|f32|257|HS|32|-|-|-|- D|u8|3|nn|f32|3771|HS|32|-|-|-|- D|u8|4|nn|f32|100|HS|32|-|-|-|- "
        "D|u8|4|nn|f32|3771|HS|32|-|-|-|- D|u8|3|nn|f32|100|HS|32|same|-|-|- D|u8|3|nn|f32|257|HS|32|same|-|-|- "
        "D|u8|3|nn|f32|3771|HS|32|same|-|-|- D|u8|4|nn|f32|100|HS|32|same|-|-|- D|u8|4|nn|f32|3771|HS|32|same|-|-|- "
        "D|u8|3|nn|f32|100|HS|32|mixed|-|-|- D|u8|3|nn|f32|257|HS|32|mixed|-|-|- D|u8|3|nn|f32|3771|HS|32|mixed|-|-|- "
        "D|u8|4|nn|f32|100|HS|32|mixed|-|-|- D|u8|4|nn|f32|3771|HS|32|mixed|-|-|- "),
    "rwh::warp_rgb8_fast<unsigned char>": (
        "A|u8|3|bilinear|u8|100|HS|1|-|-|-|- A|u8|3|bilinear|u8|127|HS|1|-|-|-|- D|u8|3|bilinear|u8|100|HS|1|-|-|-|- "
        "D|u8|3|bilinear|u8|100|HS|1|same|-|-|- D|u8|3|bilinear|u8|100|HS|1|mixed|-|-|- D|u8|3|bilinear|u8|100|HS|4|-|-|-|- "
        "D|u8|3|bilinear|u8|100|HS|4|same|-|-|- D|u8|3|bilinear|u8|100|HS|4|mixed|-|-|- D|u8|3|bilinear|u8|100|HS|32|-|-|-|- "
        "D|u8|3|bilinear|u8|100|HS|32|same|-|-|- D|u8|3|bilinear|u8|100|HS|32|mixed|-|-|- F|u8|3|bilinear|u8|100|HS|1|-|-|-|SHAPE=0 "
        "F|u8|3|bilinear|u8|100|HS|1|-|-|-|SHAPE=5 F|u8|3|bilinear|u8|100|HS|1|-|-|-|SHAPE=6 "
        "F|u8|3|bilinear|u8|100|HS|1|-|-|-|SHAPE=7 F|u8|3|bilinear|u8|100|HS|1|-|-|-|SHAPE=13 "
        "F|u8|3|bilinear|u8|100|HS|1|-|-|-|SHAPE=14 F|u8|3|bilinear|u8|100|HS|1|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|100|HS|4|-|-|-|FRAMES=0 F|u8|3|bilinear|u8|100|HS|32|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|100|HS|1|-|-|-|FRAMES=1 F|u8|3|bilinear|u8|100|HS|4|-|-|-|FRAMES=1 "
        "F|u8|3|bilinear|u8|100|HS|32|-|-|-|FRAMES=1 F|u8|3|bilinear|u8|100|HS|1|-|-|-|FRAMES=4 "
        "F|u8|3|bilinear|u8|100|HS|4|-|-|-|FRAMES=4 F|u8|3|bilinear|u8|100|HS|32|-|-|-|FRAMES=4 "
        "F|u8|3|bilinear|u8|100|HS|1|-|-|-|FRAMES=104 F|u8|3|bilinear|u8|100|HS|4|-|-|-|FRAMES=104 "
        "F|u8|3|bilinear|u8|100|HS|32|-|-|-|FRAMES=104 "),
    "rwh::warp_rgb8_fast8<unsigned char, 6>": (
        "A|u8|3|bilinear|u8|128|HS|1|-|-|-|- A|u8|3|bilinear|u8|255|HS|1|-|-|-|- A|u8|3|bilinear|u8|256|HS|1|-|-|-|- "
        "A|u8|3|bilinear|u8|257|HS|1|-|-|-|- A|u8|3|bilinear|u8|272|HS|1|-|-|-|- A|u8|3|bilinear|u8|273|HS|1|-|-|-|- "
        "A|u8|3|bilinear|u8|3771|HS|1|-|-|-|- D|u8|3|bilinear|u8|257|HS|1|-|-|-|- D|u8|3|bilinear|u8|3771|HS|1|-|-|-|- "
        "D|u8|3|bilinear|u8|257|HS|1|same|-|-|- D|u8|3|bilinear|u8|3771|HS|1|same|-|-|- D|u8|3|bilinear|u8|257|HS|1|mixed|-|-|- "
        "D|u8|3|bilinear|u8|3771|HS|1|mixed|-|-|- D|u8|3|bilinear|u8|3771|min1.5|1|mixed|-|-|- "
        "D|u8|3|bilinear|u8|3771|rot30|1|mixed|-|-|- D|u8|3|bilinear|u8|257|HS|4|-|-|-|- D|u8|3|bilinear|u8|3771|HS|4|-|-|-|- "
        "D|u8|3|bilinear|u8|257|HS|32|-|-|-|- D|u8|3|bilinear|u8|3771|HS|32|-|-|-|- E|u8|3|bilinear|u8|3771|HS|1|-|shard|-|- "
        "F|u8|3|bilinear|u8|3771|HS|1|-|-|-|SHAPE=0 F|u8|3|bilinear|u8|3771|HS|1|-|-|-|SHAPE=6 "
        "F|u8|3|bilinear|u8|3771|min1.5|1|-|-|-|SHAPE=6 F|u8|3|bilinear|u8|3771|HS|1|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|3771|HS|1|same|-|-|FRAMES=0 F|u8|3|bilinear|u8|272|HS|1|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|3771|HS|4|-|-|-|FRAMES=0 F|u8|3|bilinear|u8|272|HS|4|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|3771|HS|32|-|-|-|FRAMES=0 F|u8|3|bilinear|u8|272|HS|32|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|3771|HS|1|-|-|-|FRAMES=1 F|u8|3|bilinear|u8|3771|HS|1|same|-|-|FRAMES=1 "
        "F|u8|3|bilinear|u8|272|HS|1|-|-|-|FRAMES=1 F|u8|3|bilinear|u8|3771|HS|4|-|-|-|FRAMES=1 "
        "F|u8|3|bilinear|u8|272|HS|4|-|-|-|FRAMES=1 F|u8|3|bilinear|u8|3771|HS|32|-|-|-|FRAMES=1 "
        "F|u8|3|bilinear|u8|272|HS|32|-|-|-|FRAMES=1 F|u8|3|bilinear|u8|3771|HS|1|-|-|-|FRAMES=4 "
        "F|u8|3|bilinear|u8|3771|HS|1|same|-|-|FRAMES=4 F|u8|3|bilinear|u8|272|HS|1|-|-|-|FRAMES=4 "
        "F|u8|3|bilinear|u8|3771|HS|1|-|-|-|FRAMES=104 F|u8|3|bilinear|u8|3771|HS|1|same|-|-|FRAMES=104 "
        "F|u8|3|bilinear|u8|272|HS|1|-|-|-|FRAMES=104 "),
    "rwh::warp_generic<unsigned char, 4, unsigned char, 1>": (
        "A|u8|4|bilinear|u8|100|HS|1|-|-|-|- A|u8|4|bilinear|u8|127|HS|1|-|-|-|- D|u8|4|bilinear|u8|100|HS|1|-|-|-|- "
        "D|u8|4|bilinear|u8|100|HS|1|same|-|-|- D|u8|4|bilinear|u8|100|HS|1|mixed|-|-|- D|u8|4|bilinear|u8|100|HS|4|-|-|-|- "
        "D|u8|4|bilinear|u8|100|HS|4|same|-|-|- D|u8|4|bilinear|u8|100|HS|4|mixed|-|-|- D|u8|4|bilinear|u8|100|HS|32|-|-|-|- "
        "D|u8|4|bilinear|u8|100|HS|32|same|-|-|- D|u8|4|bilinear|u8|100|HS|32|mixed|-|-|- "),
    "rwh::warp_rgba8_fast8<6>": (
        "A|u8|4|bilinear|u8|128|HS|1|-|-|-|- A|u8|4|bilinear|u8|255|HS|1|-|-|-|- A|u8|4|bilinear|u8|256|HS|1|-|-|-|- "
        "A|u8|4|bilinear|u8|257|HS|1|-|-|-|- A|u8|4|bilinear|u8|272|HS|1|-|-|-|- A|u8|4|bilinear|u8|273|HS|1|-|-|-|- "
        "A|u8|4|bilinear|u8|3771|HS|1|-|-|-|- D|u8|4|bilinear|u8|3771|HS|1|-|-|-|- D|u8|4|bilinear|u8|3771|HS|1|same|-|-|- "
        "D|u8|4|bilinear|u8|3771|HS|1|mixed|-|-|- D|u8|4|bilinear|u8|3771|HS|4|-|-|-|- D|u8|4|bilinear|u8|3771|HS|4|same|-|-|- "
        "D|u8|4|bilinear|u8|3771|HS|4|mixed|-|-|- D|u8|4|bilinear|u8|3771|HS|32|-|-|-|- D|u8|4|bilinear|u8|3771|HS|32|same|-|-|- "
        "D|u8|4|bilinear|u8|3771|HS|32|mixed|-|-|- E|u8|4|bilinear|u8|3771|HS|1|-|shard|-|- "
        "F|u8|4|bilinear|u8|3771|HS|1|-|-|-|SHAPE=0 F|u8|4|bilinear|u8|3771|HS|1|-|-|-|SHAPE=6 "
        "F|u8|4|bilinear|u8|3771|min1.5|1|-|-|-|SHAPE=6 F|u8|4|bilinear|u8|3771|HS|1|-|-|-|FRAMES=0 "
        "F|u8|4|bilinear|u8|3771|HS|4|-|-|-|FRAMES=0 F|u8|4|bilinear|u8|3771|HS|32|-|-|-|FRAMES=0 "
        "F|u8|4|bilinear|u8|3771|HS|1|-|-|-|FRAMES=1 F|u8|4|bilinear|u8|3771|HS|4|-|-|-|FRAMES=1 "
        "F|u8|4|bilinear|u8|3771|HS|32|-|-|-|FRAMES=1 F|u8|4|bilinear|u8|3771|HS|1|-|-|-|FRAMES=4 "
        "F|u8|4|bilinear|u8|3771|HS|4|-|-|-|FRAMES=4 F|u8|4|bilinear|u8|3771|HS|32|-|-|-|FRAMES=4 "
        "F|u8|4|bilinear|u8|3771|HS|1|-|-|-|FRAMES=104 F|u8|4|bilinear|u8|3771|HS|4|-|-|-|FRAMES=104 "
        "F|u8|4|bilinear|u8|3771|HS|32|-|-|-|FRAMES=104 "),
    "rwh::warp_rgb8_fast<float>": (
        "A|u8|3|bilinear|f32|100|HS|1|-|-|-|- A|u8|3|bilinear|f32|127|HS|1|-|-|-|- D|u8|3|bilinear|f32|100|HS|1|-|-|-|- "
        "D|u8|3|bilinear|f32|100|HS|1|same|-|-|- D|u8|3|bilinear|f32|100|HS|1|mixed|-|-|- D|u8|3|bilinear|f32|100|HS|4|-|-|-|- "
        "D|u8|3|bilinear|f32|100|HS|4|same|-|-|- D|u8|3|bilinear|f32|100|HS|4|mixed|-|-|- D|u8|3|bilinear|f32|100|HS|32|-|-|-|- "
        "D|u8|3|bilinear|f32|100|HS|32|same|-|-|- D|u8|3|bilinear|f32|100|HS|32|mixed|-|-|- "),
    "rwh::warp_rgb8_fast8<float, 6>": (
        "A|u8|3|bilinear|f32|128|HS|1|-|-|-|- A|u8|3|bilinear|f32|255|HS|1|-|-|-|- A|u8|3|bilinear|f32|256|HS|1|-|-|-|- "
        "A|u8|3|bilinear|f32|257|HS|1|-|-|-|- A|u8|3|bilinear|f32|272|HS|1|-|-|-|- A|u8|3|bilinear|f32|273|HS|1|-|-|-|- "
        "A|u8|3|bilinear|f32|3771|HS|1|-|-|-|- D|u8|3|bilinear|f32|257|HS|1|-|-|-|- D|u8|3|bilinear|f32|3771|HS|1|-|-|-|- "
        "D|u8|3|bilinear|f32|257|HS|1|same|-|-|- D|u8|3|bilinear|f32|3771|HS|1|same|-|-|- D|u8|3|bilinear|f32|257|HS|1|mixed|-|-|- "
        "D|u8|3|bilinear|f32|3771|HS|1|mixed|-|-|- D|u8|3|bilinear|f32|257|HS|4|-|-|-|- D|u8|3|bilinear|f32|3771|HS|4|-|-|-|- "
        "D|u8|3|bilinear|f32|257|HS|32|-|-|-|- D|u8|3|bilinear|f32|3771|HS|32|-|-|-|- E|u8|3|bilinear|f32|3771|HS|1|-|shard|-|- "
        "F|u8|3|bilinear|f32|3771|HS|1|-|-|-|SHAPE=0 F|u8|3|bilinear|f32|3771|HS|1|-|-|-|SHAPE=6 "
        "F|u8|3|bilinear|f32|3771|min1.5|1|-|-|-|SHAPE=6 F|u8|3|bilinear|f32|3771|HS|1|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|f32|3771|HS|4|-|-|-|FRAMES=0 F|u8|3|bilinear|f32|3771|HS|32|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|f32|3771|HS|1|-|-|-|FRAMES=1 F|u8|3|bilinear|f32|3771|HS|4|-|-|-|FRAMES=1 "
        "F|u8|3|bilinear|f32|3771|HS|32|-|-|-|FRAMES=1 F|u8|3|bilinear|f32|3771|HS|1|-|-|-|FRAMES=4 "
        "F|u8|3|bilinear|f32|3771|HS|4|-|-|-|FRAMES=4 F|u8|3|bilinear|f32|3771|HS|32|-|-|-|FRAMES=4 "
        "F|u8|3|bilinear|f32|3771|HS|1|-|-|-|FRAMES=104 F|u8|3|bilinear|f32|3771|HS|4|-|-|-|FRAMES=104 "
        "F|u8|3|bilinear|f32|3771|HS|32|-|-|-|FRAMES=104 "),
    "rwh::warp_generic<unsigned char, 4, float, 1>": (
        "A|u8|4|bilinear|f32|100|HS|1|-|-|-|- A|u8|4|bilinear|f32|127|HS|1|-|-|-|- A|u8|4|bilinear|f32|128|HS|1|-|-|-|- "
        "A|u8|4|bilinear|f32|255|HS|1|-|-|-|- A|u8|4|bilinear|f32|256|HS|1|-|-|-|- A|u8|4|bilinear|f32|257|HS|1|-|-|-|- "
        "A|u8|4|bilinear|f32|272|HS|1|-|-|-|- A|u8|4|bilinear|f32|273|HS|1|-|-|-|- A|u8|4|bilinear|f32|3771|HS|1|-|-|-|- "
        "B|u8|4|bilinear|f32|257|rot30|1|-|-|-|- B|u8|4|bilinear|f32|3771|rot30|1|-|-|-|- B|u8|4|bilinear|f32|257|rot90|1|-|-|-|- "
        "B|u8|4|bilinear|f32|3771|rot90|1|-|-|-|- B|u8|4|bilinear|f32|257|min1.5|1|-|-|-|- B|u8|4|bilinear|f32|3771|min1.5|1|-|-|-|- "
        "B|u8|4|bilinear|f32|257|min1.9|1|-|-|-|- B|u8|4|bilinear|f32|3771|min1.9|1|-|-|-|- B|u8|4|bilinear|f32|257|min2|1|-|-|-|- "
        "B|u8|4|bilinear|f32|3771|min2|1|-|-|-|- B|u8|4|bilinear|f32|257|min3|1|-|-|-|- B|u8|4|bilinear|f32|3771|min3|1|-|-|-|- "
        "D|u8|4|bilinear|f32|100|HS|1|-|-|-|- D|u8|4|bilinear|f32|3771|HS|1|-|-|-|- D|u8|4|bilinear|f32|100|HS|1|same|-|-|- "
        "D|u8|4|bilinear|f32|3771|HS|1|same|-|-|- D|u8|4|bilinear|f32|100|HS|1|mixed|-|-|- D|u8|4|bilinear|f32|3771|HS|1|mixed|-|-|- "
        "D|u8|4|bilinear|f32|100|HS|4|-|-|-|- D|u8|4|bilinear|f32|3771|HS|4|-|-|-|- D|u8|4|bilinear|f32|100|HS|4|same|-|-|- "
        "D|u8|4|bilinear|f32|3771|HS|4|same|-|-|- D|u8|4|bilinear|f32|100|HS|4|mixed|-|-|- D|u8|4|bilinear|f32|3771|HS|4|mixed|-|-|- "
        "D|u8|4|bilinear|f32|100|HS|32|-|-|-|- D|u8|4|bilinear|f32|3771|HS|32|-|-|-|- D|u8|4|bilinear|f32|100|HS|32|same|-|-|- "
        "D|u8|4|bilinear|f32|3771|HS|32|same|-|-|- D|u8|4|bilinear|f32|100|HS|32|mixed|-|-|- "
        "D|u8|4|bilinear|f32|3771|HS|32|mixed|-|-|- "),
    "rwh::warp_generic<float, 3, float, 0>": (
        "A|f32|3|nn|f32|100|HS|1|-|-|-|- A|f32|3|nn|f32|127|HS|1|-|-|-|- A|f32|3|nn|f32|128|HS|1|-|-|-|- "
        "A|f32|3|nn|f32|255|HS|1|-|-|-|- A|f32|3|nn|f32|256|HS|1|-|-|-|- A|f32|3|nn|f32|257|HS|1|-|-|-|- "
        "A|f32|3|nn|f32|272|HS|1|-|-|-|- A|f32|3|nn|f32|273|HS|1|-|-|-|- A|f32|3|nn|f32|3771|HS|1|-|-|-|- "),
    "rwh::warp_generic<float, 4, float, 0>": (
        "A|f32|4|nn|f32|100|HS|1|-|-|-|- A|f32|4|nn|f32|127|HS|1|-|-|-|- A|f32|4|nn|f32|128|HS|1|-|-|-|- "
        "A|f32|4|nn|f32|255|HS|1|-|-|-|- A|f32|4|nn|f32|256|HS|1|-|-|-|- A|f32|4|nn|f32|257|HS|1|-|-|-|- "
        "A|f32|4|nn|f32|272|HS|1|-|-|-|- A|f32|4|nn|f32|273|HS|1|-|-|-|- A|f32|4|nn|f32|3771|HS|1|-|-|-|- "),
    "rwh::warp_generic<float, 3, unsigned char, 1>": (
        "A|f32|3|bilinear|u8|100|HS|1|-|-|-|- A|f32|3|bilinear|u8|127|HS|1|-|-|-|- A|f32|3|bilinear|u8|128|HS|1|-|-|-|- "
        "A|f32|3|bilinear|u8|255|HS|1|-|-|-|- A|f32|3|bilinear|u8|256|HS|1|-|-|-|- A|f32|3|bilinear|u8|257|HS|1|-|-|-|- "
        "A|f32|3|bilinear|u8|272|HS|1|-|-|-|- A|f32|3|bilinear|u8|273|HS|1|-|-|-|- A|f32|3|bilinear|u8|3771|HS|1|-|-|-|- "),
    "rwh::warp_generic<float, 4, unsigned char, 1>": (
        "A|f32|4|bilinear|u8|100|HS|1|-|-|-|- A|f32|4|bilinear|u8|127|HS|1|-|-|-|- A|f32|4|bilinear|u8|128|HS|1|-|-|-|- "
        "A|f32|4|bilinear|u8|255|HS|1|-|-|-|- A|f32|4|bilinear|u8|256|HS|1|-|-|-|- A|f32|4|bilinear|u8|257|HS|1|-|-|-|- "
        "A|f32|4|bilinear|u8|272|HS|1|-|-|-|- A|f32|4|bilinear|u8|273|HS|1|-|-|-|- A|f32|4|bilinear|u8|3771|HS|1|-|-|-|- "),
    "rwh::warp_generic<float, 3, float, 1>": (
        "A|f32|3|bilinear|f32|100|HS|1|-|-|-|- A|f32|3|bilinear|f32|127|HS|1|-|-|-|- A|f32|3|bilinear|f32|128|HS|1|-|-|-|- "
        "A|f32|3|bilinear|f32|255|HS|1|-|-|-|- A|f32|3|bilinear|f32|256|HS|1|-|-|-|- A|f32|3|bilinear|f32|257|HS|1|-|-|-|- "
        "A|f32|3|bilinear|f32|272|HS|1|-|-|-|- A|f32|3|bilinear|f32|273|HS|1|-|-|-|- A|f32|3|bilinear|f32|3771|HS|1|-|-|-|- "
        "D|f32|3|bilinear|f32|3771|HS|1|-|-|-|- D|f32|3|bilinear|f32|3771|HS|1|same|-|-|- D|f32|3|bilinear|f32|3771|HS|1|mixed|-|-|- "
        "D|f32|3|bilinear|f32|3771|HS|4|-|-|-|- D|f32|3|bilinear|f32|3771|HS|4|same|-|-|- D|f32|3|bilinear|f32|3771|HS|4|mixed|-|-|- "
        "D|f32|3|bilinear|f32|3771|HS|32|-|-|-|- D|f32|3|bilinear|f32|3771|HS|32|same|-|-|- "
        "D|f32|3|bilinear|f32|3771|HS|32|mixed|-|-|- E|f32|3|bilinear|f32|3771|HS|1|-|shard|-|- "),
    "rwh::warp_generic<float, 4, float, 1>": (
        "A|f32|4|bilinear|f32|100|HS|1|-|-|-|- A|f32|4|bilinear|f32|127|HS|1|-|-|-|- A|f32|4|bilinear|f32|128|HS|1|-|-|-|- "
        "A|f32|4|bilinear|f32|255|HS|1|-|-|-|- A|f32|4|bilinear|f32|256|HS|1|-|-|-|- A|f32|4|bilinear|f32|257|HS|1|-|-|-|- "
        "A|f32|4|bilinear|f32|272|HS|1|-|-|-|- A|f32|4|bilinear|f32|273|HS|1|-|-|-|- A|f32|4|bilinear|f32|3771|HS|1|-|-|-|- "),
    "rwh::warp_rgb8_nn<5>": (
        "B|u8|3|nn|u8|257|rot30|1|-|-|-|- B|u8|3|nn|u8|3771|rot30|1|-|-|-|- B|u8|3|nn|u8|257|rot90|1|-|-|-|- "
        "B|u8|3|nn|u8|3771|rot90|1|-|-|-|- E|u8|3|nn|u8|3771|rot30|1|-|shard|-|- F|u8|3|nn|u8|3771|HS|1|-|-|-|SHAPE=5 "
        "F|u8|3|nn|u8|3771|min1.5|1|-|-|-|SHAPE=5 "),
    "rwh::warp_rgb8_fast8<unsigned char, 5>": (
        "B|u8|3|bilinear|u8|257|rot30|1|-|-|-|- B|u8|3|bilinear|u8|3771|rot30|1|-|-|-|- B|u8|3|bilinear|u8|257|rot90|1|-|-|-|- "
        "B|u8|3|bilinear|u8|3771|rot90|1|-|-|-|- D|u8|3|bilinear|u8|3771|rot30|1|-|-|-|- D|u8|3|bilinear|u8|3771|rot30|1|same|-|-|- "
        "D|u8|3|bilinear|u8|3771|rot30|4|-|-|-|- D|u8|3|bilinear|u8|3771|rot30|32|-|-|-|- E|u8|3|bilinear|u8|3771|rot30|1|-|shard|-|- "
        "F|u8|3|bilinear|u8|3771|HS|1|-|-|-|SHAPE=5 F|u8|3|bilinear|u8|3771|min1.5|1|-|-|-|SHAPE=5 "),
    "rwh::warp_rgb8_fast8<float, 5>": (
        "B|u8|3|bilinear|f32|257|rot30|1|-|-|-|- B|u8|3|bilinear|f32|3771|rot30|1|-|-|-|- B|u8|3|bilinear|f32|257|rot90|1|-|-|-|- "
        "B|u8|3|bilinear|f32|3771|rot90|1|-|-|-|- E|u8|3|bilinear|f32|3771|rot30|1|-|shard|-|- "
        "F|u8|3|bilinear|f32|3771|HS|1|-|-|-|SHAPE=5 F|u8|3|bilinear|f32|3771|min1.5|1|-|-|-|SHAPE=5 "),
    "rwh::warp_rgba8_fast8<5>": (
        "B|u8|4|bilinear|u8|257|rot30|1|-|-|-|- B|u8|4|bilinear|u8|3771|rot30|1|-|-|-|- B|u8|4|bilinear|u8|257|rot90|1|-|-|-|- "
        "B|u8|4|bilinear|u8|3771|rot90|1|-|-|-|- F|u8|4|bilinear|u8|3771|HS|1|-|-|-|SHAPE=5 "
        "F|u8|4|bilinear|u8|3771|min1.5|1|-|-|-|SHAPE=5 "),
    "rwh::warp_rgb8_nn<7>": (
        "B|u8|3|nn|u8|257|min1.5|1|-|-|-|- B|u8|3|nn|u8|3771|min1.5|1|-|-|-|- B|u8|3|nn|u8|257|min1.9|1|-|-|-|- "
        "B|u8|3|nn|u8|3771|min1.9|1|-|-|-|- B|u8|3|nn|u8|257|min2|1|-|-|-|- B|u8|3|nn|u8|3771|min2|1|-|-|-|- "
        "B|u8|3|nn|u8|257|min3|1|-|-|-|- B|u8|3|nn|u8|3771|min3|1|-|-|-|- B|u8|3|nn|u8|None|scale1.5|1|-|-|-|- "
        "B|u8|3|nn|u8|None|scale2|1|-|-|-|- B|u8|3|nn|u8|None|scale3|1|-|-|-|- E|u8|3|nn|u8|3771|min1.5|1|-|shard|-|- "
        "F|u8|3|nn|u8|3771|min1.5|1|-|-|-|SHAPE=0 F|u8|3|nn|u8|3771|HS|1|-|-|-|SHAPE=7 F|u8|3|nn|u8|3771|min1.5|1|-|-|-|SHAPE=7 "
        "F|u8|3|nn|u8|3771|HS|1|-|-|-|SHAPE=13 F|u8|3|nn|u8|3771|min1.5|1|-|-|-|SHAPE=13 F|u8|3|nn|u8|3771|HS|1|-|-|-|SHAPE=14 "
        "F|u8|3|nn|u8|3771|min1.5|1|-|-|-|SHAPE=14 F|u8|3|nn|u8|3771|min1.5|1|-|-|-|FRAMES=0 F|u8|3|nn|u8|3771|min3|1|-|-|-|FRAMES=0 "
        "F|u8|3|nn|u8|3771|min1.5|4|-|-|-|FRAMES=0 F|u8|3|nn|u8|3771|min3|4|-|-|-|FRAMES=0 F|u8|3|nn|u8|3771|min1.5|32|-|-|-|FRAMES=0 "
        "F|u8|3|nn|u8|3771|min3|32|-|-|-|FRAMES=0 F|u8|3|nn|u8|3771|min1.5|1|-|-|-|FRAMES=1 F|u8|3|nn|u8|3771|min3|1|-|-|-|FRAMES=1 "
        "F|u8|3|nn|u8|3771|min1.5|4|-|-|-|FRAMES=1 F|u8|3|nn|u8|3771|min3|4|-|-|-|FRAMES=1 F|u8|3|nn|u8|3771|min1.5|32|-|-|-|FRAMES=1 "
        "F|u8|3|nn|u8|3771|min3|32|-|-|-|FRAMES=1 F|u8|3|nn|u8|3771|min1.5|1|-|-|-|FRAMES=4 F|u8|3|nn|u8|3771|min3|1|-|-|-|FRAMES=4 "
        "F|u8|3|nn|u8|3771|min1.5|4|-|-|-|FRAMES=4 F|u8|3|nn|u8|3771|min3|4|-|-|-|FRAMES=4 F|u8|3|nn|u8|3771|min1.5|32|-|-|-|FRAMES=4 "
        "F|u8|3|nn|u8|3771|min3|32|-|-|-|FRAMES=4 F|u8|3|nn|u8|3771|min1.5|1|-|-|-|FRAMES=104 "
        "F|u8|3|nn|u8|3771|min3|1|-|-|-|FRAMES=104 F|u8|3|nn|u8|3771|min1.5|4|-|-|-|FRAMES=104 "
        "F|u8|3|nn|u8|3771|min3|4|-|-|-|FRAMES=104 F|u8|3|nn|u8|3771|min1.5|32|-|-|-|FRAMES=104 "
        "F|u8|3|nn|u8|3771|min3|32|-|-|-|FRAMES=104 "),
    "rwh::warp_rgb8_fast8h<6>": (
        "B|u8|3|bilinear|u8|257|min1.5|1|-|-|-|- B|u8|3|bilinear|u8|3771|min1.5|1|-|-|-|- B|u8|3|bilinear|u8|None|scale1.5|1|-|-|-|- "
        "D|u8|3|bilinear|u8|3771|min1.5|1|-|-|-|- D|u8|3|bilinear|u8|3771|min1.5|1|same|-|-|- "
        "D|u8|3|bilinear|u8|3771|min1.5|4|-|-|-|- D|u8|3|bilinear|u8|3771|min1.5|32|-|-|-|- "
        "E|u8|3|bilinear|u8|3771|min1.5|1|-|shard|-|- F|u8|3|bilinear|u8|3771|min1.5|1|-|-|-|SHAPE=0 "
        "F|u8|3|bilinear|u8|3771|HS|1|-|-|-|SHAPE=14 F|u8|3|bilinear|u8|3771|min1.5|1|-|-|-|SHAPE=14 "
        "F|u8|3|bilinear|u8|3771|min1.5|1|-|-|-|FRAMES=0 F|u8|3|bilinear|u8|3771|min1.5|1|same|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|3771|min1.5|4|-|-|-|FRAMES=0 F|u8|3|bilinear|u8|3771|min1.5|32|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|3771|min1.5|1|-|-|-|FRAMES=1 F|u8|3|bilinear|u8|3771|min1.5|1|same|-|-|FRAMES=1 "
        "F|u8|3|bilinear|u8|3771|min1.5|4|-|-|-|FRAMES=1 F|u8|3|bilinear|u8|3771|min1.5|32|-|-|-|FRAMES=1 "
        "F|u8|3|bilinear|u8|3771|min1.5|1|-|-|-|FRAMES=4 F|u8|3|bilinear|u8|3771|min1.5|1|same|-|-|FRAMES=4 "
        "F|u8|3|bilinear|u8|3771|min1.5|4|-|-|-|FRAMES=4 F|u8|3|bilinear|u8|3771|min1.5|32|-|-|-|FRAMES=4 "
        "F|u8|3|bilinear|u8|3771|min1.5|1|-|-|-|FRAMES=104 F|u8|3|bilinear|u8|3771|min1.5|1|same|-|-|FRAMES=104 "
        "F|u8|3|bilinear|u8|3771|min1.5|4|-|-|-|FRAMES=104 F|u8|3|bilinear|u8|3771|min1.5|32|-|-|-|FRAMES=104 "),
    "rwh::warp_rgb8_fast8<float, 7>": (
        "B|u8|3|bilinear|f32|257|min1.5|1|-|-|-|- B|u8|3|bilinear|f32|3771|min1.5|1|-|-|-|- B|u8|3|bilinear|f32|257|min1.9|1|-|-|-|- "
        "B|u8|3|bilinear|f32|3771|min1.9|1|-|-|-|- B|u8|3|bilinear|f32|257|min2|1|-|-|-|- B|u8|3|bilinear|f32|3771|min2|1|-|-|-|- "
        "B|u8|3|bilinear|f32|257|min3|1|-|-|-|- B|u8|3|bilinear|f32|3771|min3|1|-|-|-|- B|u8|3|bilinear|f32|None|scale1.5|1|-|-|-|- "
        "B|u8|3|bilinear|f32|None|scale2|1|-|-|-|- B|u8|3|bilinear|f32|None|scale3|1|-|-|-|- "
        "E|u8|3|bilinear|f32|3771|min1.5|1|-|shard|-|- F|u8|3|bilinear|f32|3771|min1.5|1|-|-|-|SHAPE=0 "
        "F|u8|3|bilinear|f32|3771|HS|1|-|-|-|SHAPE=7 F|u8|3|bilinear|f32|3771|min1.5|1|-|-|-|SHAPE=7 "
        "F|u8|3|bilinear|f32|3771|HS|1|-|-|-|SHAPE=13 F|u8|3|bilinear|f32|3771|min1.5|1|-|-|-|SHAPE=13 "
        "F|u8|3|bilinear|f32|3771|HS|1|-|-|-|SHAPE=14 F|u8|3|bilinear|f32|3771|min1.5|1|-|-|-|SHAPE=14 "
        "F|u8|3|bilinear|f32|3771|min1.5|1|-|-|-|FRAMES=0 F|u8|3|bilinear|f32|3771|min3|1|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|f32|3771|min1.5|4|-|-|-|FRAMES=0 F|u8|3|bilinear|f32|3771|min3|4|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|f32|3771|min1.5|32|-|-|-|FRAMES=0 F|u8|3|bilinear|f32|3771|min3|32|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|f32|3771|min1.5|1|-|-|-|FRAMES=1 F|u8|3|bilinear|f32|3771|min3|1|-|-|-|FRAMES=1 "
        "F|u8|3|bilinear|f32|3771|min1.5|4|-|-|-|FRAMES=1 F|u8|3|bilinear|f32|3771|min3|4|-|-|-|FRAMES=1 "
        "F|u8|3|bilinear|f32|3771|min1.5|32|-|-|-|FRAMES=1 F|u8|3|bilinear|f32|3771|min3|32|-|-|-|FRAMES=1 "
        "F|u8|3|bilinear|f32|3771|min1.5|1|-|-|-|FRAMES=4 F|u8|3|bilinear|f32|3771|min3|1|-|-|-|FRAMES=4 "
        "F|u8|3|bilinear|f32|3771|min1.5|4|-|-|-|FRAMES=4 F|u8|3|bilinear|f32|3771|min3|4|-|-|-|FRAMES=4 "
        "F|u8|3|bilinear|f32|3771|min1.5|32|-|-|-|FRAMES=4 F|u8|3|bilinear|f32|3771|min3|32|-|-|-|FRAMES=4 "
        "F|u8|3|bilinear|f32|3771|min1.5|1|-|-|-|FRAMES=104 F|u8|3|bilinear|f32|3771|min3|1|-|-|-|FRAMES=104 "
        "F|u8|3|bilinear|f32|3771|min1.5|4|-|-|-|FRAMES=104 F|u8|3|bilinear|f32|3771|min3|4|-|-|-|FRAMES=104 "
        "F|u8|3|bilinear|f32|3771|min1.5|32|-|-|-|FRAMES=104 F|u8|3|bilinear|f32|3771|min3|32|-|-|-|FRAMES=104 "),
    "rwh::warp_rgba8_fast8<7>": (
        "B|u8|4|bilinear|u8|257|min1.5|1|-|-|-|- B|u8|4|bilinear|u8|3771|min1.5|1|-|-|-|- B|u8|4|bilinear|u8|257|min1.9|1|-|-|-|- "
        "B|u8|4|bilinear|u8|3771|min1.9|1|-|-|-|- B|u8|4|bilinear|u8|257|min2|1|-|-|-|- B|u8|4|bilinear|u8|3771|min2|1|-|-|-|- "
        "B|u8|4|bilinear|u8|257|min3|1|-|-|-|- B|u8|4|bilinear|u8|3771|min3|1|-|-|-|- B|u8|4|bilinear|u8|None|scale1.5|1|-|-|-|- "
        "B|u8|4|bilinear|u8|None|scale2|1|-|-|-|- B|u8|4|bilinear|u8|None|scale3|1|-|-|-|- "
        "F|u8|4|bilinear|u8|3771|min1.5|1|-|-|-|SHAPE=0 F|u8|4|bilinear|u8|3771|HS|1|-|-|-|SHAPE=7 "
        "F|u8|4|bilinear|u8|3771|min1.5|1|-|-|-|SHAPE=7 F|u8|4|bilinear|u8|3771|HS|1|-|-|-|SHAPE=13 "
        "F|u8|4|bilinear|u8|3771|min1.5|1|-|-|-|SHAPE=13 F|u8|4|bilinear|u8|3771|HS|1|-|-|-|SHAPE=14 "
        "F|u8|4|bilinear|u8|3771|min1.5|1|-|-|-|SHAPE=14 F|u8|4|bilinear|u8|3771|min1.5|1|-|-|-|FRAMES=0 "
        "F|u8|4|bilinear|u8|3771|min3|1|-|-|-|FRAMES=0 F|u8|4|bilinear|u8|3771|min1.5|4|-|-|-|FRAMES=0 "
        "F|u8|4|bilinear|u8|3771|min3|4|-|-|-|FRAMES=0 F|u8|4|bilinear|u8|3771|min1.5|32|-|-|-|FRAMES=0 "
        "F|u8|4|bilinear|u8|3771|min3|32|-|-|-|FRAMES=0 F|u8|4|bilinear|u8|3771|min1.5|1|-|-|-|FRAMES=1 "
        "F|u8|4|bilinear|u8|3771|min3|1|-|-|-|FRAMES=1 F|u8|4|bilinear|u8|3771|min1.5|4|-|-|-|FRAMES=1 "
        "F|u8|4|bilinear|u8|3771|min3|4|-|-|-|FRAMES=1 F|u8|4|bilinear|u8|3771|min1.5|32|-|-|-|FRAMES=1 "
        "F|u8|4|bilinear|u8|3771|min3|32|-|-|-|FRAMES=1 F|u8|4|bilinear|u8|3771|min1.5|1|-|-|-|FRAMES=4 "
        "F|u8|4|bilinear|u8|3771|min3|1|-|-|-|FRAMES=4 F|u8|4|bilinear|u8|3771|min1.5|4|-|-|-|FRAMES=4 "
        "F|u8|4|bilinear|u8|3771|min3|4|-|-|-|FRAMES=4 F|u8|4|bilinear|u8|3771|min1.5|32|-|-|-|FRAMES=4 "
        "F|u8|4|bilinear|u8|3771|min3|32|-|-|-|FRAMES=4 F|u8|4|bilinear|u8|3771|min1.5|1|-|-|-|FRAMES=104 "
        "F|u8|4|bilinear|u8|3771|min3|1|-|-|-|FRAMES=104 F|u8|4|bilinear|u8|3771|min1.5|4|-|-|-|FRAMES=104 "
        "F|u8|4|bilinear|u8|3771|min3|4|-|-|-|FRAMES=104 F|u8|4|bilinear|u8|3771|min1.5|32|-|-|-|FRAMES=104 "
        "F|u8|4|bilinear|u8|3771|min3|32|-|-|-|FRAMES=104 "),
    "rwh::warp_rgb8_fast8h<5>": (
        "B|u8|3|bilinear|u8|257|min1.9|1|-|-|-|- B|u8|3|bilinear|u8|3771|min1.9|1|-|-|-|- B|u8|3|bilinear|u8|257|min2|1|-|-|-|- "
        "B|u8|3|bilinear|u8|None|scale2|1|-|-|-|- F|u8|3|bilinear|u8|3771|HS|1|-|-|-|SHAPE=13 "
        "F|u8|3|bilinear|u8|3771|min1.5|1|-|-|-|SHAPE=13 "),
    "rwh::warp_rgb8_fast8<unsigned char, 7>": (
        "B|u8|3|bilinear|u8|3771|min2|1|-|-|-|- B|u8|3|bilinear|u8|257|min3|1|-|-|-|- B|u8|3|bilinear|u8|3771|min3|1|-|-|-|- "
        "B|u8|3|bilinear|u8|None|scale3|1|-|-|-|- F|u8|3|bilinear|u8|3771|HS|1|-|-|-|SHAPE=7 "
        "F|u8|3|bilinear|u8|3771|min1.5|1|-|-|-|SHAPE=7 F|u8|3|bilinear|u8|3771|min3|1|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|3771|min3|1|same|-|-|FRAMES=0 F|u8|3|bilinear|u8|3771|min3|4|-|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|3771|min3|32|-|-|-|FRAMES=0 F|u8|3|bilinear|u8|3771|min3|1|-|-|-|FRAMES=1 "
        "F|u8|3|bilinear|u8|3771|min3|1|same|-|-|FRAMES=1 F|u8|3|bilinear|u8|3771|min3|4|-|-|-|FRAMES=1 "
        "F|u8|3|bilinear|u8|3771|min3|32|-|-|-|FRAMES=1 F|u8|3|bilinear|u8|3771|min3|1|-|-|-|FRAMES=4 "
        "F|u8|3|bilinear|u8|3771|min3|1|same|-|-|FRAMES=4 F|u8|3|bilinear|u8|3771|min3|1|-|-|-|FRAMES=104 "
        "F|u8|3|bilinear|u8|3771|min3|1|same|-|-|FRAMES=104 "),
    "rwh::warp_rgb8_fast8h_tab<6>": (
        "B|u8|3|bilinear|u8|None|scale1.5|4|same|-|-|- D|u8|3|bilinear|u8|3771|min1.5|4|same|-|-|- "
        "D|u8|3|bilinear|u8|257|HS|4|mixed|-|-|- D|u8|3|bilinear|u8|3771|HS|4|mixed|-|-|- "
        "D|u8|3|bilinear|u8|3771|min1.5|4|mixed|-|-|- D|u8|3|bilinear|u8|3771|rot30|4|mixed|-|-|- "
        "D|u8|3|bilinear|u8|3771|min1.5|32|same|-|-|- D|u8|3|bilinear|u8|257|HS|32|mixed|-|-|- "
        "D|u8|3|bilinear|u8|3771|HS|32|mixed|-|-|- D|u8|3|bilinear|u8|3771|min1.5|32|mixed|-|-|- "
        "D|u8|3|bilinear|u8|3771|rot30|32|mixed|-|-|- E|u8|3|bilinear|u8|3771|HS|4|mixed|shard|-|- "
        "E|u8|3|bilinear|u8|3771|rot30|4|mixed|shard|-|- E|u8|3|bilinear|u8|3771|min1.5|4|mixed|shard|-|- "
        "F|u8|3|bilinear|u8|3771|HS|4|mixed|-|-|SHAPE=0 F|u8|3|bilinear|u8|3771|min1.5|4|same|-|-|SHAPE=0 "
        "F|u8|3|bilinear|u8|3771|min1.5|4|mixed|-|-|SHAPE=0 F|u8|3|bilinear|u8|3771|HS|4|same|-|-|SHAPE=14 "
        "F|u8|3|bilinear|u8|3771|HS|4|mixed|-|-|SHAPE=14 F|u8|3|bilinear|u8|3771|min1.5|4|same|-|-|SHAPE=14 "
        "F|u8|3|bilinear|u8|3771|min1.5|4|mixed|-|-|SHAPE=14 F|u8|3|bilinear|u8|3771|min1.5|4|same|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|3771|min1.5|32|same|-|-|FRAMES=0 F|u8|3|bilinear|u8|3771|min1.5|4|same|-|-|FRAMES=1 "
        "F|u8|3|bilinear|u8|3771|min1.5|32|same|-|-|FRAMES=1 F|u8|3|bilinear|u8|3771|min1.5|4|same|-|-|FRAMES=4 "
        "F|u8|3|bilinear|u8|3771|min1.5|32|same|-|-|FRAMES=4 F|u8|3|bilinear|u8|3771|min1.5|4|same|-|-|FRAMES=104 "
        "F|u8|3|bilinear|u8|3771|min1.5|32|same|-|-|FRAMES=104 "),
    "rwh::warp_rgb8_fast8h_tab<5>": (
        "B|u8|3|bilinear|u8|None|scale2|4|same|-|-|- F|u8|3|bilinear|u8|3771|HS|4|same|-|-|SHAPE=13 "
        "F|u8|3|bilinear|u8|3771|HS|4|mixed|-|-|SHAPE=13 F|u8|3|bilinear|u8|3771|min1.5|4|same|-|-|SHAPE=13 "
        "F|u8|3|bilinear|u8|3771|min1.5|4|mixed|-|-|SHAPE=13 "),
    "rwh::warp_rgb8_fast8_tab<unsigned char, 7>": (
        "B|u8|3|bilinear|u8|None|scale3|4|same|-|-|- F|u8|3|bilinear|u8|3771|HS|4|same|-|-|SHAPE=7 "
        "F|u8|3|bilinear|u8|3771|HS|4|mixed|-|-|SHAPE=7 F|u8|3|bilinear|u8|3771|min1.5|4|same|-|-|SHAPE=7 "
        "F|u8|3|bilinear|u8|3771|min1.5|4|mixed|-|-|SHAPE=7 F|u8|3|bilinear|u8|3771|min3|4|same|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|3771|min3|32|same|-|-|FRAMES=0 F|u8|3|bilinear|u8|3771|min3|4|same|-|-|FRAMES=1 "
        "F|u8|3|bilinear|u8|3771|min3|32|same|-|-|FRAMES=1 F|u8|3|bilinear|u8|3771|min3|4|same|-|-|FRAMES=4 "
        "F|u8|3|bilinear|u8|3771|min3|32|same|-|-|FRAMES=4 F|u8|3|bilinear|u8|3771|min3|4|same|-|-|FRAMES=104 "
        "F|u8|3|bilinear|u8|3771|min3|32|same|-|-|FRAMES=104 "),
    "rwh::warp_any<unsigned char, unsigned char, 0>": (
        "C|u8|1|nn|u8|3771|HS|1|-|-|exact|- C|u8|5|nn|u8|3771|HS|1|-|-|exact|- C|u8|64|nn|u8|3771|HS|1|-|-|exact|- "
        "C|bool|1|nn|bool|3771|HS|1|-|-|exact|- C|bool|5|nn|bool|3771|HS|1|-|-|exact|- C|bool|64|nn|bool|3771|HS|1|-|-|exact|- "
        "C|i8|1|nn|i8|3771|HS|1|-|-|exact|- C|i8|3|nn|i8|3771|HS|1|-|-|exact|- C|i8|4|nn|i8|3771|HS|1|-|-|exact|- "
        "C|i8|5|nn|i8|3771|HS|1|-|-|exact|- C|i8|64|nn|i8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<unsigned char, double, 1>": (
        "C|u8|1|bilinear|f64|3771|HS|1|-|-|exact|- C|u8|5|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|u8|64|bilinear|f64|3771|HS|1|-|-|exact|- C|bool|1|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|bool|5|bilinear|f64|3771|HS|1|-|-|exact|- C|bool|64|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<unsigned char, unsigned char, 1>": (
        "C|u8|1|bilinear|u8|3771|HS|1|-|-|exact|- C|u8|5|bilinear|u8|3771|HS|1|-|-|exact|- C|u8|64|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|bool|1|bilinear|u8|3771|HS|1|-|-|exact|- C|bool|5|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|bool|64|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_exact<unsigned char, 3, double, 1>": (
        "C|u8|3|bilinear|f64|3771|HS|1|-|-|exact|- C|bool|3|bilinear|f64|3771|HS|1|-|-|exact|- "
        "D|u8|3|bilinear|f64|3771|HS|1|-|-|exact|- D|u8|3|bilinear|f64|3771|HS|1|same|-|exact|- "
        "D|u8|3|bilinear|f64|3771|HS|1|mixed|-|exact|- D|u8|3|bilinear|f64|3771|HS|4|-|-|exact|- "
        "D|u8|3|bilinear|f64|3771|HS|4|same|-|exact|- D|u8|3|bilinear|f64|3771|HS|4|mixed|-|exact|- "
        "D|u8|3|bilinear|f64|3771|HS|32|-|-|exact|- D|u8|3|bilinear|f64|3771|HS|32|same|-|exact|- "
        "D|u8|3|bilinear|f64|3771|HS|32|mixed|-|exact|- "),
    "rwh::warp_exact<unsigned char, 3, unsigned char, 1>": (
        "C|u8|3|bilinear|u8|3771|HS|1|-|-|exact|- C|bool|3|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_exact<unsigned char, 4, unsigned char, 0>": (
        "C|u8|4|nn|u8|3771|HS|1|-|-|exact|- C|bool|4|nn|bool|3771|HS|1|-|-|exact|- "),
    "rwh::warp_exact<unsigned char, 4, double, 1>": (
        "C|u8|4|bilinear|f64|3771|HS|1|-|-|exact|- C|bool|4|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_exact<unsigned char, 4, unsigned char, 1>": (
        "C|u8|4|bilinear|u8|3771|HS|1|-|-|exact|- C|bool|4|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<unsigned int, unsigned int, 0>": (
        "C|f32|1|nn|f32|3771|HS|1|-|-|exact|- C|f32|5|nn|f32|3771|HS|1|-|-|exact|- C|f32|64|nn|f32|3771|HS|1|-|-|exact|- "
        "C|i32|1|nn|i32|3771|HS|1|-|-|exact|- C|i32|3|nn|i32|3771|HS|1|-|-|exact|- C|i32|4|nn|i32|3771|HS|1|-|-|exact|- "
        "C|i32|5|nn|i32|3771|HS|1|-|-|exact|- C|i32|64|nn|i32|3771|HS|1|-|-|exact|- C|u32|1|nn|u32|3771|HS|1|-|-|exact|- "
        "C|u32|3|nn|u32|3771|HS|1|-|-|exact|- C|u32|4|nn|u32|3771|HS|1|-|-|exact|- C|u32|5|nn|u32|3771|HS|1|-|-|exact|- "
        "C|u32|64|nn|u32|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<float, double, 1>": (
        "C|f32|1|bilinear|f64|3771|HS|1|-|-|exact|- C|f32|5|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|f32|64|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<float, unsigned char, 1>": (
        "C|f32|1|bilinear|u8|3771|HS|1|-|-|exact|- C|f32|5|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|f32|64|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_exact<float, 3, float, 0>": (
        "C|f32|3|nn|f32|3771|HS|1|-|-|exact|- "),
    "rwh::warp_exact<float, 3, double, 1>": (
        "C|f32|3|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_exact<float, 3, unsigned char, 1>": (
        "C|f32|3|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_exact<float, 4, float, 0>": (
        "C|f32|4|nn|f32|3771|HS|1|-|-|exact|- "),
    "rwh::warp_exact<float, 4, double, 1>": (
        "C|f32|4|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_exact<float, 4, unsigned char, 1>": (
        "C|f32|4|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<unsigned long, unsigned long, 0>": (
        "C|f64|1|nn|f64|3771|HS|1|-|-|exact|- C|f64|3|nn|f64|3771|HS|1|-|-|exact|- C|f64|4|nn|f64|3771|HS|1|-|-|exact|- "
        "C|f64|5|nn|f64|3771|HS|1|-|-|exact|- C|f64|64|nn|f64|3771|HS|1|-|-|exact|- C|i64|1|nn|i64|3771|HS|1|-|-|exact|- "
        "C|i64|3|nn|i64|3771|HS|1|-|-|exact|- C|i64|4|nn|i64|3771|HS|1|-|-|exact|- C|i64|5|nn|i64|3771|HS|1|-|-|exact|- "
        "C|i64|64|nn|i64|3771|HS|1|-|-|exact|- C|u64|1|nn|u64|3771|HS|1|-|-|exact|- C|u64|3|nn|u64|3771|HS|1|-|-|exact|- "
        "C|u64|4|nn|u64|3771|HS|1|-|-|exact|- C|u64|5|nn|u64|3771|HS|1|-|-|exact|- C|u64|64|nn|u64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<double, double, 1>": (
        "C|f64|1|bilinear|f64|3771|HS|1|-|-|exact|- C|f64|3|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|f64|4|bilinear|f64|3771|HS|1|-|-|exact|- C|f64|5|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|f64|64|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<double, unsigned char, 1>": (
        "C|f64|1|bilinear|u8|3771|HS|1|-|-|exact|- C|f64|3|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|f64|4|bilinear|u8|3771|HS|1|-|-|exact|- C|f64|5|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|f64|64|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<signed char, double, 1>": (
        "C|i8|1|bilinear|f64|3771|HS|1|-|-|exact|- C|i8|3|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|i8|4|bilinear|f64|3771|HS|1|-|-|exact|- C|i8|5|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|i8|64|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<signed char, unsigned char, 1>": (
        "C|i8|1|bilinear|u8|3771|HS|1|-|-|exact|- C|i8|3|bilinear|u8|3771|HS|1|-|-|exact|- C|i8|4|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|i8|5|bilinear|u8|3771|HS|1|-|-|exact|- C|i8|64|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<unsigned short, unsigned short, 0>": (
        "C|u16|1|nn|u16|3771|HS|1|-|-|exact|- C|u16|3|nn|u16|3771|HS|1|-|-|exact|- C|u16|4|nn|u16|3771|HS|1|-|-|exact|- "
        "C|u16|5|nn|u16|3771|HS|1|-|-|exact|- C|u16|64|nn|u16|3771|HS|1|-|-|exact|- C|i16|1|nn|i16|3771|HS|1|-|-|exact|- "
        "C|i16|3|nn|i16|3771|HS|1|-|-|exact|- C|i16|4|nn|i16|3771|HS|1|-|-|exact|- C|i16|5|nn|i16|3771|HS|1|-|-|exact|- "
        "C|i16|64|nn|i16|3771|HS|1|-|-|exact|- C|f16|1|nn|f16|3771|HS|1|-|-|exact|- C|f16|3|nn|f16|3771|HS|1|-|-|exact|- "
        "C|f16|4|nn|f16|3771|HS|1|-|-|exact|- C|f16|5|nn|f16|3771|HS|1|-|-|exact|- C|f16|64|nn|f16|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<unsigned short, double, 1>": (
        "C|u16|1|bilinear|f64|3771|HS|1|-|-|exact|- C|u16|3|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|u16|4|bilinear|f64|3771|HS|1|-|-|exact|- C|u16|5|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|u16|64|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<unsigned short, unsigned char, 1>": (
        "C|u16|1|bilinear|u8|3771|HS|1|-|-|exact|- C|u16|3|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|u16|4|bilinear|u8|3771|HS|1|-|-|exact|- C|u16|5|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|u16|64|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<short, double, 1>": (
        "C|i16|1|bilinear|f64|3771|HS|1|-|-|exact|- C|i16|3|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|i16|4|bilinear|f64|3771|HS|1|-|-|exact|- C|i16|5|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|i16|64|bilinear|f64|3771|HS|1|-|-|exact|- D|i16|5|bilinear|f64|3771|HS|1|-|-|exact|- "
        "D|i16|5|bilinear|f64|3771|HS|1|same|-|exact|- D|i16|5|bilinear|f64|3771|HS|1|mixed|-|exact|- "
        "D|i16|5|bilinear|f64|3771|HS|4|-|-|exact|- D|i16|5|bilinear|f64|3771|HS|4|same|-|exact|- "
        "D|i16|5|bilinear|f64|3771|HS|4|mixed|-|exact|- D|i16|5|bilinear|f64|3771|HS|32|-|-|exact|- "
        "D|i16|5|bilinear|f64|3771|HS|32|same|-|exact|- D|i16|5|bilinear|f64|3771|HS|32|mixed|-|exact|- "),
    "rwh::warp_any<short, unsigned char, 1>": (
        "C|i16|1|bilinear|u8|3771|HS|1|-|-|exact|- C|i16|3|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|i16|4|bilinear|u8|3771|HS|1|-|-|exact|- C|i16|5|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|i16|64|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<int, double, 1>": (
        "C|i32|1|bilinear|f64|3771|HS|1|-|-|exact|- C|i32|3|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|i32|4|bilinear|f64|3771|HS|1|-|-|exact|- C|i32|5|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|i32|64|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<int, unsigned char, 1>": (
        "C|i32|1|bilinear|u8|3771|HS|1|-|-|exact|- C|i32|3|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|i32|4|bilinear|u8|3771|HS|1|-|-|exact|- C|i32|5|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|i32|64|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<unsigned int, double, 1>": (
        "C|u32|1|bilinear|f64|3771|HS|1|-|-|exact|- C|u32|3|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|u32|4|bilinear|f64|3771|HS|1|-|-|exact|- C|u32|5|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|u32|64|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<unsigned int, unsigned char, 1>": (
        "C|u32|1|bilinear|u8|3771|HS|1|-|-|exact|- C|u32|3|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|u32|4|bilinear|u8|3771|HS|1|-|-|exact|- C|u32|5|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|u32|64|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<long, double, 1>": (
        "C|i64|1|bilinear|f64|3771|HS|1|-|-|exact|- C|i64|3|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|i64|4|bilinear|f64|3771|HS|1|-|-|exact|- C|i64|5|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|i64|64|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<long, unsigned char, 1>": (
        "C|i64|1|bilinear|u8|3771|HS|1|-|-|exact|- C|i64|3|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|i64|4|bilinear|u8|3771|HS|1|-|-|exact|- C|i64|5|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|i64|64|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<unsigned long, double, 1>": (
        "C|u64|1|bilinear|f64|3771|HS|1|-|-|exact|- C|u64|3|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|u64|4|bilinear|f64|3771|HS|1|-|-|exact|- C|u64|5|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|u64|64|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<unsigned long, unsigned char, 1>": (
        "C|u64|1|bilinear|u8|3771|HS|1|-|-|exact|- C|u64|3|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|u64|4|bilinear|u8|3771|HS|1|-|-|exact|- C|u64|5|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|u64|64|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<_Float16, double, 1>": (
        "C|f16|1|bilinear|f64|3771|HS|1|-|-|exact|- C|f16|3|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|f16|4|bilinear|f64|3771|HS|1|-|-|exact|- C|f16|5|bilinear|f64|3771|HS|1|-|-|exact|- "
        "C|f16|64|bilinear|f64|3771|HS|1|-|-|exact|- "),
    "rwh::warp_any<_Float16, unsigned char, 1>": (
        "C|f16|1|bilinear|u8|3771|HS|1|-|-|exact|- C|f16|3|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|f16|4|bilinear|u8|3771|HS|1|-|-|exact|- C|f16|5|bilinear|u8|3771|HS|1|-|-|exact|- "
        "C|f16|64|bilinear|u8|3771|HS|1|-|-|exact|- "),
    "rwh::warp_exact<unsigned char, 3, unsigned char, 0>": (
        "C|u8|3|nn|u8|100|HS|1|-|-|exact|- "),
    "rwh::warp_rgb8_nn_tab<6>": (
        "D|u8|3|nn|u8|257|HS|4|same|-|-|- D|u8|3|nn|u8|3771|HS|4|same|-|-|- D|u8|3|nn|u8|257|HS|32|same|-|-|- "
        "D|u8|3|nn|u8|3771|HS|32|same|-|-|- F|u8|3|nn|u8|3771|HS|4|same|-|-|SHAPE=0 F|u8|3|nn|u8|3771|HS|4|same|-|-|SHAPE=6 "
        "F|u8|3|nn|u8|3771|min1.5|4|same|-|-|SHAPE=6 "),
    "rwh::warp_rgb8_fast8_tab<unsigned char, 6>": (
        "D|u8|3|bilinear|u8|257|HS|4|same|-|-|- D|u8|3|bilinear|u8|3771|HS|4|same|-|-|- D|u8|3|bilinear|u8|257|HS|32|same|-|-|- "
        "D|u8|3|bilinear|u8|3771|HS|32|same|-|-|- F|u8|3|bilinear|u8|3771|HS|4|same|-|-|SHAPE=0 "
        "F|u8|3|bilinear|u8|3771|HS|4|same|-|-|SHAPE=6 F|u8|3|bilinear|u8|3771|HS|4|mixed|-|-|SHAPE=6 "
        "F|u8|3|bilinear|u8|3771|min1.5|4|same|-|-|SHAPE=6 F|u8|3|bilinear|u8|3771|min1.5|4|mixed|-|-|SHAPE=6 "
        "F|u8|3|bilinear|u8|3771|HS|4|same|-|-|FRAMES=0 F|u8|3|bilinear|u8|3771|HS|32|same|-|-|FRAMES=0 "
        "F|u8|3|bilinear|u8|3771|HS|4|same|-|-|FRAMES=1 F|u8|3|bilinear|u8|3771|HS|32|same|-|-|FRAMES=1 "
        "F|u8|3|bilinear|u8|3771|HS|4|same|-|-|FRAMES=4 F|u8|3|bilinear|u8|3771|HS|32|same|-|-|FRAMES=4 "
        "F|u8|3|bilinear|u8|3771|HS|4|same|-|-|FRAMES=104 F|u8|3|bilinear|u8|3771|HS|32|same|-|-|FRAMES=104 "),
    "rwh::warp_rgb8_fast8_tab<float, 6>": (
        "D|u8|3|bilinear|f32|257|HS|4|same|-|-|- D|u8|3|bilinear|f32|3771|HS|4|same|-|-|- D|u8|3|bilinear|f32|257|HS|32|same|-|-|- "
        "D|u8|3|bilinear|f32|3771|HS|32|same|-|-|- F|u8|3|bilinear|f32|3771|HS|4|same|-|-|SHAPE=0 "
        "F|u8|3|bilinear|f32|3771|HS|4|same|-|-|SHAPE=6 F|u8|3|bilinear|f32|3771|min1.5|4|same|-|-|SHAPE=6 "),
    "rwh::warp_rgb8_fast8_tab<unsigned char, 5>": (
        "D|u8|3|bilinear|u8|3771|rot30|4|same|-|-|- D|u8|3|bilinear|u8|3771|rot30|32|same|-|-|- "
        "F|u8|3|bilinear|u8|3771|HS|4|same|-|-|SHAPE=5 F|u8|3|bilinear|u8|3771|HS|4|mixed|-|-|SHAPE=5 "
        "F|u8|3|bilinear|u8|3771|min1.5|4|same|-|-|SHAPE=5 F|u8|3|bilinear|u8|3771|min1.5|4|mixed|-|-|SHAPE=5 "),
    "rwh::warp_rgb8_nn_tab<7>": (
        "D|u8|3|nn|u8|257|HS|4|mixed|-|-|- D|u8|3|nn|u8|3771|HS|4|mixed|-|-|- D|u8|3|nn|u8|257|HS|32|mixed|-|-|- "
        "D|u8|3|nn|u8|3771|HS|32|mixed|-|-|- E|u8|3|nn|u8|3771|HS|4|mixed|shard|-|- E|u8|3|nn|u8|3771|rot30|4|mixed|shard|-|- "
        "E|u8|3|nn|u8|3771|min1.5|4|mixed|shard|-|- F|u8|3|nn|u8|3771|min1.5|4|same|-|-|SHAPE=0 "
        "F|u8|3|nn|u8|3771|HS|4|same|-|-|SHAPE=7 F|u8|3|nn|u8|3771|min1.5|4|same|-|-|SHAPE=7 F|u8|3|nn|u8|3771|HS|4|same|-|-|SHAPE=13 "
        "F|u8|3|nn|u8|3771|min1.5|4|same|-|-|SHAPE=13 F|u8|3|nn|u8|3771|HS|4|same|-|-|SHAPE=14 "
        "F|u8|3|nn|u8|3771|min1.5|4|same|-|-|SHAPE=14 "),
    "rwh::warp_rgb8_fast8_tab<float, 7>": (
        "D|u8|3|bilinear|f32|257|HS|4|mixed|-|-|- D|u8|3|bilinear|f32|3771|HS|4|mixed|-|-|- D|u8|3|bilinear|f32|257|HS|32|mixed|-|-|- "
        "D|u8|3|bilinear|f32|3771|HS|32|mixed|-|-|- E|u8|3|bilinear|f32|3771|HS|4|mixed|shard|-|- "
        "E|u8|3|bilinear|f32|3771|rot30|4|mixed|shard|-|- E|u8|3|bilinear|f32|3771|min1.5|4|mixed|shard|-|- "
        "F|u8|3|bilinear|f32|3771|min1.5|4|same|-|-|SHAPE=0 F|u8|3|bilinear|f32|3771|HS|4|same|-|-|SHAPE=7 "
        "F|u8|3|bilinear|f32|3771|min1.5|4|same|-|-|SHAPE=7 F|u8|3|bilinear|f32|3771|HS|4|same|-|-|SHAPE=13 "
        "F|u8|3|bilinear|f32|3771|min1.5|4|same|-|-|SHAPE=13 F|u8|3|bilinear|f32|3771|HS|4|same|-|-|SHAPE=14 "
        "F|u8|3|bilinear|f32|3771|min1.5|4|same|-|-|SHAPE=14 "),
    "rwh::warp_rgb8_nn_tab<5>": (
        "F|u8|3|nn|u8|3771|HS|4|same|-|-|SHAPE=5 F|u8|3|nn|u8|3771|min1.5|4|same|-|-|SHAPE=5 "),
    "rwh::warp_rgb8_fast8_tab<float, 5>": (
        "F|u8|3|bilinear|f32|3771|HS|4|same|-|-|SHAPE=5 F|u8|3|bilinear|f32|3771|min1.5|4|same|-|-|SHAPE=5 "),
    "rwh::warp_rgb8_fast8m<6>": (
        "F|u8|3|bilinear|u8|3771|HS|4|-|-|-|FRAMES=4 F|u8|3|bilinear|u8|272|HS|4|-|-|-|FRAMES=4 "
        "F|u8|3|bilinear|u8|3771|HS|32|-|-|-|FRAMES=4 F|u8|3|bilinear|u8|272|HS|32|-|-|-|FRAMES=4 "),
    "rwh::warp_rgb8_fast8m<7>": (
        "F|u8|3|bilinear|u8|3771|min3|4|-|-|-|FRAMES=4 F|u8|3|bilinear|u8|3771|min3|32|-|-|-|FRAMES=4 "),
    "rwh::warp_rgb8_fast8mb<6>": (
        "F|u8|3|bilinear|u8|3771|HS|4|-|-|-|FRAMES=104 F|u8|3|bilinear|u8|272|HS|4|-|-|-|FRAMES=104 "
        "F|u8|3|bilinear|u8|3771|HS|32|-|-|-|FRAMES=104 F|u8|3|bilinear|u8|272|HS|32|-|-|-|FRAMES=104 "),
    "rwh::warp_rgb8_fast8mb<7>": (
        "F|u8|3|bilinear|u8|3771|min3|4|-|-|-|FRAMES=104 F|u8|3|bilinear|u8|3771|min3|32|-|-|-|FRAMES=104 "),
}

def test_warp_plan_sweep_matches_parent(lib):
    """Every kernel name rwh_warp_plan reports over a fixed matrix of configurations equals what the library reported BEFORE the
    warp dispatch was refactored to choose each kernel once: _PLAN_SWEEP was generated from the library of the parent commit
    6f87344 (not from this tree), so a change of selection -- or of a single byte of a name -- fails here, without a GPU.
    The matrix: uint8 / float32 sources and, in exact mode, every STITCH_DTYPE type; 1, 3, 4, 5 and 64 channels; nn and bilinear;
    uint8 / float32 / float64 outputs, legal or refused (a refusal is a row: its status code); output widths around the 128 px tiles
    and the ragged-edge strip; batches of 1, 4 and 32 with one homography and with one per image (the same, and mixed ones that choose
    different shapes); bench.py's H_S, rotations by 30 and 90 degrees, minifications about the image centre and plain scales by
    1 / 1.5, 1 / 2, 1 / 3 on their own grids; a row shard; RWH_TUNE_WARP_SHAPE in 0, 5, 6, 7, 13, 14 and RWH_TUNE_WARP_FRAMES in 0, 1, 4, 104.
    Known limit: rwh_warp_plan records only the FIRST launch of a call, so the ragged-edge strip launch (warp_rgb8_strip*: out_w >= 256
    and out_w % 128 in 1..16) and the second and later shape groups of a per-image batch do not show in it; those are covered by the
    GPU tests test_warp_vs_oracle_1080p_and_ragged, test_warp_one_homography_per_image and test_warp_minification_halves_per_image."""
    from ransac_with_homography_amd import _lib
    want = {key: result for result, keys in _PLAN_SWEEP.items() for key in keys.split()}
    assert len(want) == sum(len(keys.split()) for keys in _PLAN_SWEEP.values()) > 900
    got = {}
    try:
        for key, thunk in _plan_sweep_rows():
            assert key not in got, key
            got[key] = thunk()
    finally:
        assert lib.rwh_lab_tune(_lib.RWH_TUNE_WARP_SHAPE, 0) == 0 and lib.rwh_lab_tune(_lib.RWH_TUNE_WARP_FRAMES, 0) == 0
    assert set(got) == set(want)
    wrong = {key: (got[key], want[key]) for key in got if got[key] != want[key]}
    assert not wrong, wrong
    # the matrix reaches the kernels it is meant to reach (the host's own choices on the parent, not forced ones)
    for key, name in (("B|u8|3|bilinear|u8|None|scale1.5|1|-|-|-|-", "rwh::warp_rgb8_fast8h<6>"),
                      ("B|u8|3|bilinear|u8|None|scale2|1|-|-|-|-", "rwh::warp_rgb8_fast8h<5>"),
                      ("B|u8|3|bilinear|u8|None|scale3|1|-|-|-|-", "rwh::warp_rgb8_fast8<unsigned char, 7>"),
                      ("F|u8|3|bilinear|u8|3771|HS|32|-|-|-|FRAMES=4", "rwh::warp_rgb8_fast8m<6>"),
                      ("F|u8|3|bilinear|u8|3771|HS|32|-|-|-|FRAMES=104", "rwh::warp_rgb8_fast8mb<6>"),
                      ("F|u8|3|bilinear|u8|3771|HS|1|-|-|-|SHAPE=13", "rwh::warp_rgb8_fast8h<5>"),
                      ("F|u8|3|bilinear|u8|3771|HS|1|-|-|-|SHAPE=14", "rwh::warp_rgb8_fast8h<6>"),
                      ("C|i16|5|bilinear|f64|3771|HS|1|-|-|exact|-", "rwh::warp_any<short, double, 1>"),
                      ("C|i16|5|nn|i16|3771|HS|1|-|-|exact|-", "rwh::warp_any<unsigned short, unsigned short, 0>"),
                      ("A|u8|3|bilinear|u8|100|HS|1|-|-|-|-", "rwh::warp_rgb8_fast<unsigned char>"),
                      ("A|u8|3|bilinear|u8|127|HS|1|-|-|-|-", "rwh::warp_rgb8_fast<unsigned char>"),
                      ("A|u8|3|bilinear|u8|128|HS|1|-|-|-|-", "rwh::warp_rgb8_fast8<unsigned char, 6>"),
                      ("A|u8|3|bilinear|u8|3771|HS|1|-|-|-|-", "rwh::warp_rgb8_fast8<unsigned char, 6>"),
                      ("A|u8|1|bilinear|u8|3771|HS|1|-|-|-|-", -2)):
        assert want[key] == name, key


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import homography as hg
    import ransac as rs
    from ransac_with_homography_amd import RwhUnavailable
    with pytest.raises(RwhUnavailable):
        hg.wrapPerspective(np.zeros((8, 8, 3), np.uint8), np.eye(3), "bilinear")
    with pytest.raises(RwhUnavailable):
        rs.RANSAC(rs.HomoModel(), k=10).run([np.zeros((2, 8), np.float32), np.zeros((2, 8), np.float32)], "fwd")


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing shipped may reference it."""
    shipped = [os.path.join(ROOT, "homography.py"), os.path.join(ROOT, "ransac.py")]
    pkg = os.path.join(ROOT, "ransac_with_homography_amd")
    for d, _, files in os.walk(pkg):
        shipped += [os.path.join(d, f) for f in files if f.endswith((".py", ".hip", ".h"))]
    for path in shipped:
        text = open(path).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), path


def test_host_solvers_match_goldens():
    """Host-side O(1) solvers of the product against the reference's G1 outputs."""
    import homography as hg
    from conftest import load_golden
    z = load_golden("g1_fourpoint")
    u, v = z["u"].T[:, :2], z["v"].T[:, :2]
    A, b = hg.calc_correspLinear(u, v)
    assert np.array_equal(A, z["A"]) and np.array_equal(b, z["b"])
    assert np.array_equal(hg.calc_corresp(u, v), z["mat"])
    assert np.array_equal(hg.calcHomographyLinear(u, v), z["H_linear"])
    assert np.array_equal(hg.calcHomography(u, v), z["H_dlt"])          # float64 inputs: host SVD path
    assert hg.calcH is hg.calcHomographyLinear and hg.perspectiveTransform is hg.wrapPerspective


def test_plain_c_consumer(lib, tmp_path):
    """include/rwh.h compiles as C and a gcc-built program links the library and gets the documented status codes."""
    import subprocess
    from ransac_with_homography_amd import _lib
    exe = str(tmp_path / "cabi_smoke")
    libdir = os.path.dirname(_lib.LIB_PATH)
    torch_lib = os.path.join(os.path.dirname(__import__("torch").__file__), "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cabi", "cabi_smoke.c"), "-o", exe, "-L", libdir, "-lrwh_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath," + torch_lib,
                    "-Wl,--allow-shlib-undefined"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "cabi ok" in out
