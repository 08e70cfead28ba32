"""stitchPanorama on images that are not uint8 RGB (the any-dtype compositor, rwh_stitch_panorama_ex) on the MI355X: the
reference's recorded outcomes, canvases and side effects (g20) through numpy arrays and device tensors, a seeded soak against the
oracle, row tiles against the whole canvas, and two 4K float32 frames against oracle-computed canvas windows."""
import contextlib
import io

import numpy as np
import pytest

from g20_cases import g20_cases, run_case
from oracle import rwh_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch


def _stitch(q, t, H, blending, rate):
    import homography as hg
    return hg.stitchPanorama(q, t, H, blending=blending, blendrate=rate)


def _u8_route(Q, T):
    """True when stitchPanorama takes these images down its uint8 path (3 / 3 channels, uint8 values): not this feature's."""
    from ransac_with_homography_amd import homography as impl
    if Q.shape[2] != 3 or T.shape[2] != 3:
        return False
    try:
        impl._as_uint8_image(Q, "imgQ"), impl._as_uint8_image(T, "imgT")
        return True
    except NotImplementedError:
        return False


def test_g20_numpy(gpu):
    bad = {}
    for c in g20_cases():
        b = run_case(_stitch, c)
        if b:
            bad[c["name"]] = b
    assert not bad, bad


def test_g20_device_tensors(gpu):
    torch = gpu
    bad, n = {}, 0
    for c in g20_cases():
        if _u8_route(c["Q"], c["T"]):
            continue            # the uint8 path's fast kernel (within 1 LSB): covered by test_gpu_parity
        n += 1
        b = run_case(_stitch, c, to_input=lambda a: torch.from_numpy(a.copy()).cuda(), to_numpy=lambda x: x.cpu().numpy())
        if b:
            bad[c["name"]] = b
    assert n > 350 and not bad, bad


DTYPES = ("uint8", "int8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float16", "float32", "float64", "bool")


def _random_image(rng, dtype, h, w, c):
    shape = (h, w, c)
    if dtype == "bool":
        return rng.integers(0, 2, shape).astype(bool)
    if dtype.startswith("float"):
        v = rng.uniform(-40.0, 300.0, shape)
        sp = rng.random(shape) < 0.01
        v[sp] = rng.choice([np.nan, np.inf, -np.inf, 255.5, -0.5, 2.0 ** 31 + 3, 1e39], int(sp.sum()))
        with np.errstate(all="ignore"):
            return v.astype(dtype)
    info = np.iinfo(dtype)
    v = rng.integers(max(int(info.min), -100), min(int(info.max), 400), shape, endpoint=True).astype(dtype)
    wide = rng.random(shape) < 0.05
    v[wide] = rng.integers(int(info.min), int(info.max), int(wide.sum()), endpoint=True, dtype=dtype)
    return v


def test_soak_against_oracle(gpu):
    torch = gpu
    rng = np.random.default_rng(4242)
    blendings = (False, "Rate", "Gradient", True)
    bad, outcomes = {}, {}
    for i in range(400):
        blending = blendings[i % 4]
        ct = int(rng.choice([3, 4]))
        cq = int(rng.choice([ct, 1])) if not blending else int(rng.choice([1, 3, 4]))
        dt, dq = rng.choice(DTYPES), rng.choice(DTYPES)
        h, w = int(rng.integers(8, 301)), int(rng.integers(8, 401))
        hq, wq = int(rng.integers(8, 301)), int(rng.integers(8, 401))
        T, Q = _random_image(rng, dt, h, w, ct), _random_image(rng, dq, hq, wq, cq)
        H = np.array([[1 + rng.normal(0, 0.05), rng.normal(0, 0.05), rng.uniform(-0.6, 0.6) * w],
                      [rng.normal(0, 0.05), 1 + rng.normal(0, 0.05), rng.uniform(-0.6, 0.6) * h],
                      [rng.normal(0, 2e-4), rng.normal(0, 2e-4), 1.0]])
        rate = float(rng.uniform(0.05, 0.7))
        q_ref, t_ref = Q.copy(), T.copy()
        try:
            with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                canvas = orc.stitch_panorama(q_ref, t_ref, H, blending=blending, blendrate=rate)
            outcome = "ok"
        except (IndexError, ValueError) as e:
            outcome, canvas = type(e).__name__, None
        outcomes[outcome] = outcomes.get(outcome, 0) + 1
        case = dict(Q=Q, T=T, H=H, blending=blending, rate=rate, outcome=outcome, canvas=canvas, t_after=t_ref)
        if i % 2 and not _u8_route(Q, T):
            b = run_case(_stitch, case, to_input=lambda a: torch.from_numpy(a.copy()).cuda(), to_numpy=lambda x: x.cpu().numpy())
        else:
            b = run_case(_stitch, case)
        if b:
            bad["%d %s %s %s %d/%d" % (i, blending, dt, dq, ct, cq)] = b
    assert outcomes.get("ok", 0) > 300, outcomes
    assert not bad, bad


def test_row_tiles_equal_whole_canvas(gpu):
    torch = gpu
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(7)
    H = np.array([[0.98, 0.03, 40.5], [-0.02, 1.01, -25.25], [1e-4, -5e-5, 1.0]])
    for k, (dt, ct, cq, blend) in enumerate(((torch.float32, 3, 3, 0), (torch.float64, 4, 1, 0), (torch.uint16, 4, 4, 1),
                                             (torch.int32, 3, 1, 2), (torch.float16, 4, 3, 3))):
        T = torch.from_numpy(rng.uniform(-20, 280, (150, 210, ct))).to(dt).cuda()
        Q = torch.from_numpy(rng.uniform(-20, 280, (140, 190, cq))).to(torch.float32).cuda()
        mx, my, wt, ht = orc.output_bounds(150, 210, H, 0)
        (tsx, tsy, _, _), (qsx, qsy, _, _), (fw, fh) = orc.stitch_geometry(wt, ht, 190, 140, mx, my)
        ih = np.linalg.inv(H)
        args = (ih, (mx, my), (wt, ht), (tsx, tsy), (qsx, qsy), (fh, fw), blend, 0.3)
        whole = kernels.stitch_panorama_ex(T.clone(), Q, *args, zero_origin=True)
        T2 = T.clone()
        tiled = torch.full_like(whole, 77)
        bounds = [0, 1, 7, 64, 65, fh // 2, fh - 3, fh]
        for i in range(len(bounds) - 1):
            # paste: the flag writes imgT, first tile only; blend: it blanks in registers, every tile
            kernels.stitch_panorama_ex(T2, Q, *args, zero_origin=(i == 0 or blend > 0), rows=(bounds[i], bounds[i + 1]), out=tiled)
        torch.cuda.synchronize()
        assert torch.equal(whole, tiled), k
        if blend:
            assert torch.equal(T2, T), k               # blend never writes imgT
        else:
            assert not T2[0, 0].any() and torch.equal(T2.view(-1)[ct:], T.view(-1)[ct:]), k


def _window_ref(Q, T, H, blending, rate, x0, y0, n=256):
    """The reference's canvas on columns x0 .. x0 + n - 1, rows y0 .. y0 + n - 1 (homography.py:288-338 on those coordinates only)."""
    h, w, _ = T.shape
    mx, my, wt, ht = orc.output_bounds(h, w, H, 0)
    (tsx, tsy, tex, tey), (qsx, qsy, qex, qey), _ = orc.stitch_geometry(wt, ht, Q.shape[1], Q.shape[0], mx, my)
    xs, ys = np.arange(x0, x0 + n), np.arange(y0, y0 + n)
    in_t = ((xs >= tsx) & (xs <= tex))[None, :] & ((ys >= tsy) & (ys <= tey))[:, None]
    in_q = ((xs >= qsx) & (xs <= qex))[None, :] & ((ys >= qsy) & (ys <= qey))[:, None]
    src = orc.add_alpha_rate(T, rate) if blending else T.copy()
    z_t = orc._source_coords(H, x0 - tsx + mx, x0 + n - 1 - tsx + mx, n, y0 - tsy + my, y0 + n - 1 - tsy + my, n)
    warped = orc.bilinear(z_t, src, h, w, n, n)
    yy, xx = np.nonzero(in_q)
    qwin = np.zeros((n, n, Q.shape[2]), Q.dtype)
    qwin[yy, xx] = Q[ys[yy] - qsy, xs[xx] - qsx]
    with np.errstate(all="ignore"):
        if not blending:
            ref = np.zeros((n, n, 3), np.uint8)
            ref[in_t] = warped.astype(np.uint8)[in_t]
            ref[in_q] = qwin[in_q]
            return ref
        can = np.zeros((n, n, 4), np.float32)
        can[:, :, :3][in_q] = qwin[in_q].astype(np.float32)
        can[:, :, 3] += 1e-10
        can[:, :, 3][in_q] = 1 + 1e-10 - rate
        base = can[:, :, 3:4] + warped[:, :, 3:4]
        mixed = (can[:, :, 3:4] / base) * can[:, :, :3] + (warped[:, :, 3:4] / base) * warped[:, :, :3]
        can[:, :, :3][in_t] = mixed[in_t]
        return can[:, :, :3].astype(np.uint8)


def test_4k_float32_against_oracle_windows(gpu):
    import homography as hg
    rng = np.random.default_rng(44)
    base = rng.uniform(-10.0, 270.0, (270, 480, 3))
    T = np.ascontiguousarray(np.repeat(np.repeat(base, 8, axis=0), 8, axis=1) + rng.uniform(-0.5, 0.5, (2160, 3840, 3))).astype(np.float32)
    Q = np.ascontiguousarray(T[::-1, ::-1] * np.float32(0.9) + np.float32(3.25))
    H = np.array([[0.97, 0.02, 2400.5], [-0.015, 1.01, 130.25], [-3e-6, 2e-6, 1.0]])
    h, w, _ = T.shape
    mx, my, wt, ht = orc.output_bounds(h, w, H, 0)
    (tsx, tsy, tex, tey), (qsx, qsy, qex, qey), (fw, fh) = orc.stitch_geometry(wt, ht, Q.shape[1], Q.shape[0], mx, my)
    for blending in (False, "Rate"):
        with contextlib.redirect_stdout(io.StringIO()):
            out = hg.stitchPanorama(Q, T.copy(), H, blending=blending, blendrate=0.3)
        assert out.shape == (fh, fw, 3) and out.dtype == np.uint8
        for cx, cy in ((qex - 128, (qsy + qey) // 2), ((tsx + tex) // 2, max(tsy - 100, 0)), (tex - 1500, (tsy + tey) // 2), (0, 0),
                       (fw - 256, fh - 256)):
            x0, y0 = max(cx, 0), max(cy, 0)
            ref = _window_ref(Q, T, H, blending, 0.3, x0, y0)
            assert np.array_equal(out[y0:y0 + 256, x0:x0 + 256], ref), (blending, cx, cy)
