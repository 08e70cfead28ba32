"""The warp entry points on images of every numeric dtype and channel count (the any-dtype exact kernel, warp_any) on the MI355X:
the reference's recorded outcomes, results and side effects (g21) through the public functions, a seeded soak against the oracle,
row tiles and per-image homographies against the whole warp, one 4K float64 frame (the pipelined host path) against oracle-computed
windows, and convertfunc on precomputed coordinates."""
import contextlib
import io

import numpy as np
import pytest

from g21_cases import g21_cases, public_api, run_case, same_result
from oracle import rwh_oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = ("uint8", "int8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float16", "float32", "float64", "bool")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch


def test_g21_public_api(gpu):
    api = public_api()
    bad = {}
    for c in g21_cases():
        b = run_case(api, c)
        if b:
            bad[c["name"]] = b
    assert not bad, bad


SPECIAL_F = (np.nan, np.inf, -np.inf, -0.0, 0.1, 2.9999999999, -0.5, 255.5, 2.0 ** 24 + 1, 2.0 ** 31 + 3, -2.0 ** 31 - 3, 2.0 ** 53 + 2)


def _random_image(rng, dt, h, w, c, special):
    shape = (h, w, c)
    if dt == "bool":
        return rng.integers(0, 2, shape).astype(bool)
    if dt.startswith("float"):
        v = rng.uniform(-60.0, 320.0, shape)
        if special:
            m = rng.random(shape) < 0.3
            v[m] = np.array(SPECIAL_F)[rng.integers(0, len(SPECIAL_F), int(m.sum()))]
        with np.errstate(over="ignore"):
            return v.astype(dt)
    info = np.iinfo(dt)
    v = rng.integers(max(int(info.min), -300), min(int(info.max), 600), shape, endpoint=True).astype(dt)
    if special:
        m = rng.random(shape) < 0.3
        v[m] = rng.integers(int(info.min), int(info.max), int(m.sum()), endpoint=True, dtype=dt)
    return v


def _case(api_fn, img, ref_img, expect, bits):
    """(outcome, result, origin) of api_fn on img -> what differs from `expect` (the oracle's on ref_img)."""
    try:
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
            r = api_fn(img)
        got = ("ok", np.asarray(r[0]), tuple(int(v) for v in r[1:]))
    except (IndexError, ValueError) as e:
        got = (type(e).__name__, None, None)
    bad = []
    if got[0] != expect[0]:
        bad.append("outcome %s, oracle %s" % (got[0], expect[0]))
    elif got[1] is not None:
        if got[1].dtype != expect[1].dtype or got[1].shape != expect[1].shape:
            bad.append("result %s %s, oracle %s %s" % (got[1].dtype, got[1].shape, expect[1].dtype, expect[1].shape))
        elif not same_result(got[1], expect[1], bits):
            bad.append("result differs")
        if got[2] != expect[2]:
            bad.append("origin %s, oracle %s" % (got[2], expect[2]))
    if img.tobytes() != ref_img.tobytes():
        bad.append("caller's image differs")
    return bad


def _expect(fn, img):
    try:
        with np.errstate(all="ignore"):
            r = fn(img)
        return ("ok", np.asarray(r[0]), tuple(int(v) for v in r[1:]))
    except (IndexError, ValueError) as e:
        return (type(e).__name__, None, None)


def test_soak_against_oracle(gpu):
    import homography as hg
    rng = np.random.default_rng(2121)
    modes = {"nn": (lambda H: lambda a: hg.wrapPerspective(a, H, "nn"), lambda H: lambda a: orc.wrap_perspective(a, H, "nn")),
             "bilinear": (lambda H: lambda a: hg.wrapPerspective(a, H, "bilinear"), lambda H: lambda a: orc.wrap_perspective(a, H, "bilinear")),
             "tih": (lambda H: lambda a: hg.transformImageH(a, H), lambda H: lambda a: orc.transform_image_h(a, H))}
    bad, outcomes, n = {}, {}, 0
    for dt in DTYPES:
        for c in (3, 4, 5, 7):
            for mode, (ours, ref) in modes.items():
                h, w = int(rng.integers(8, 70)), int(rng.integers(8, 90))
                legacy = dt in ("uint8", "float32") and c in (3, 4)     # (their kernels: the cases test_gpu_parity covers)
                img = _random_image(rng, dt, h, w, c, special=not legacy and n % 2 == 0)
                H = np.array([[1 + rng.normal(0, 0.08), rng.normal(0, 0.08), rng.uniform(-0.3, 0.3) * w],
                              [rng.normal(0, 0.08), 1 + rng.normal(0, 0.08), rng.uniform(-0.3, 0.3) * h],
                              [rng.normal(0, 1e-3), rng.normal(0, 1e-3), 1.0]])
                ref_img = img.copy()
                expect = _expect(ref(H), ref_img)
                outcomes[expect[0]] = outcomes.get(expect[0], 0) + 1
                b = _case(ours(H), img, ref_img, expect, bits=mode == "nn")
                if b:
                    bad["%s %s c%d %dx%d" % (mode, dt, c, h, w)] = b
                n += 1
    assert n == 144 and outcomes.get("ok", 0) > 90, outcomes
    assert not bad, bad


def test_row_tiles_and_batches_equal_whole_warp(gpu):
    torch = gpu
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(9)
    Hs = [np.array([[0.98, 0.03, 4.5], [-0.02, 1.01, -2.25], [1e-4, -5e-5, 1.0]]),
          np.array([[1.05, -0.02, -3.5], [0.01, 0.97, 5.0], [-2e-4, 1e-4, 1.0]]),
          np.array([[0.9, 0.1, 8.0], [-0.1, 0.9, 6.0], [0.0, 0.0, 1.0]])]
    ih = np.stack([np.linalg.inv(H) for H in Hs])
    h, w = 150, 210
    grid = kernels.Grid(-7, 219, 227, -5, 152, 158)
    for dt, c in (("float64", 3), ("int64", 5), ("uint16", 1), ("float16", 7), ("bool", 5), ("int8", 2), ("uint32", 4), ("float32", 6)):
        src = torch.from_numpy(np.stack([_random_image(rng, dt, h, w, c, special=True) for _ in Hs])).cuda()
        for interp, out_dtype in (("nn", src.dtype), ("bilinear", torch.float64), ("bilinear", torch.uint8)):
            whole = kernels.warp_backward(src.clone(), ih, grid, (h, w), interp, out_dtype, zero_origin=True, exact=True)
            s2 = src.clone()
            bounds = [0, 1, 5, 64, 65, grid.out_h // 2, grid.out_h - 3, grid.out_h]
            tiles = [kernels.warp_backward(s2, ih, grid, (h, w), interp, out_dtype, zero_origin=(i == 0), rows=(bounds[i], bounds[i + 1]),
                                           exact=True) for i in range(len(bounds) - 1)]
            tiled = torch.cat([t.view(torch.uint8) for t in tiles], dim=1)     # (bytes: not every op takes every dtype)
            assert tiled.view(torch.uint8).equal(whole.view(torch.uint8)), (dt, c, interp, out_dtype)
            for b in range(len(Hs)):            # image b of the batch = a single warp of image b by its own homography
                one = kernels.warp_backward(src[b].clone(), ih[b], grid, (h, w), interp, out_dtype, zero_origin=True, exact=True)
                assert one.view(torch.uint8).equal(whole[b].view(torch.uint8)), (dt, c, interp, out_dtype, b)
            # the blanking: channels 0..2 of texel (0,0), and 3 only with exactly 4 channels
            k = 4 if c == 4 else min(c, 3)
            t0 = s2[:, 0, 0].view(torch.uint8).reshape(len(Hs), c, -1)
            assert not t0[:, :k].any() and t0[:, k:].equal(src[:, 0, 0].view(torch.uint8).reshape(len(Hs), c, -1)[:, k:])
            assert s2.view(torch.uint8).reshape(len(Hs), -1)[:, c * src.element_size():].equal(
                src.view(torch.uint8).reshape(len(Hs), -1)[:, c * src.element_size():])


def test_4k_float64_against_oracle_windows(gpu, monkeypatch):
    import homography as hg
    from ransac_with_homography_amd import homography as impl
    calls = []
    real = impl._warp_pipelined

    def spy(*a, **k):
        calls.append(a[0].dtype)
        return real(*a, **k)
    monkeypatch.setattr(impl, "_warp_pipelined", spy)
    rng = np.random.default_rng(45)
    base = rng.uniform(-10.0, 270.0, (270, 480, 3))
    T = np.ascontiguousarray(np.repeat(np.repeat(base, 8, axis=0), 8, axis=1) + rng.uniform(-0.5, 0.5, (2160, 3840, 3)))
    T[5, 7] = (np.nan, np.inf, -0.0)
    H = np.array([[0.97, 0.02, 40.5], [-0.015, 1.01, 30.25], [-3e-6, 2e-6, 1.0]])
    h, w, _ = T.shape
    mx, my, wt, ht = orc.output_bounds(h, w, H, 0)
    n = 256
    for conv in ("bilinear", "nn"):
        img = T.copy()
        out, ox, oy = hg.wrapPerspective(img, H, conv)
        assert (ox, oy) == (mx, my) and out.shape == (ht, wt, 3) and out.dtype == np.float64
        assert img[0, 0].tobytes() == bytes(24) and img[0, 1:].tobytes() == T[0, 1:].tobytes()
        for x0, y0 in ((0, 0), (wt - n, ht - n), (wt // 2, ht // 2), (100, ht - n), (wt - n - 3, 17)):
            z_t = orc._source_coords(H, mx + x0, mx + x0 + n - 1, n, my + y0, my + y0 + n - 1, n)
            ref = orc.INTERPOLATORS[conv](z_t, T.copy(), h, w, n, n)
            assert same_result(out[y0:y0 + n, x0:x0 + n], ref, bits=conv == "nn"), (conv, x0, y0)
    assert calls == [np.dtype(np.float64)] * 2, calls        # both went through the pipelined host path


def test_convertfunc_new_dtypes(gpu):
    import homography as hg
    rng = np.random.default_rng(17)
    bad = {}
    for dt in DTYPES:
        for c in (3, 5, 7):
            h, w = int(rng.integers(6, 40)), int(rng.integers(6, 40))
            legacy = dt in ("uint8", "float32") and c in (3, 4)     # (their kernel returns 0 for a masked pixel: finite values only)
            img = _random_image(rng, dt, h, w, c, special=not legacy)
            mh, mw = int(rng.integers(2, 30)), int(rng.integers(2, 30))
            z = np.vstack([rng.uniform(-3, w + 1, mh * mw), rng.uniform(-3, h + 1, mh * mw), np.ones(mh * mw)])
            if c == 5:                  # NaN coordinates: masked in nn, IndexError in bilinear (after z_t's masked columns are zeroed)
                z[:, rng.random(mh * mw) < 0.1] = np.nan
            # (coordinates in [w-1, w) or [h-1, h) index past the image in the reference: IndexError from both)
            for conv in ("nn", "bilinear"):
                ref_img, ref_z, my_img, my_z = img.copy(), z.copy(), img.copy(), z.copy()
                try:
                    with np.errstate(all="ignore"):
                        ref = ("ok", orc.INTERPOLATORS[conv](ref_z, ref_img, h, w, mh, mw))
                except IndexError:
                    ref = ("IndexError", None)
                try:
                    got = ("ok", hg.convertfunc[conv](my_z, my_img, h, w, mh, mw))
                except IndexError:
                    got = ("IndexError", None)
                key = "%s %s c%d" % (conv, dt, c)
                if got[0] != ref[0]:
                    bad[key] = "outcome %s, oracle %s" % (got[0], ref[0])
                elif got[1] is not None and not same_result(got[1], ref[1], bits=conv == "nn"):
                    bad[key] = "result differs"
                if my_img.tobytes() != ref_img.tobytes():
                    bad[key + " img"] = "caller's image differs"
                if my_z.tobytes() != ref_z.tobytes():
                    bad[key + " z"] = "caller's z_t differs"
    assert not bad, bad
