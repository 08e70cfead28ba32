"""GPU parity tests (run with `-m gpu` on an MI355X): the HIP path, called through the C ABI
(librwh_hip.so via ransac_with_homography_amd), against
  * the committed golden fixtures the REFERENCE produced (tests/golden), and
  * the CPU oracle on the same seeded inputs.

Tolerances, stated once:
  WARP_RTOL  bilinear pixels: |gpu - ref| <= 1e-4 * |ref| + 1e-5   (north_star: 1e-4 relative fp32;
             the 1e-5 absolute floor is 4e-8 of full scale and only matters for |ref| < 0.1)
  nearest-neighbour pixels, inlier counts / indices / masks, per-pair losses: bit-exact
  uint8 bilinear results: +-1 LSB where the reference's float64 value sits within ~4e-5 of an integer
             (float32 vs float64 blend followed by TRUNCATION): rare on noise (< 2 %),
             common in flat regions of photographs, where four equal taps p give p or p-1ulp in
             float64 (measured 7.4 % on notebook.jpg); never more than 1 LSB
  per-hypothesis H: bit-identical to LAPACK's on >= 97.5 % of non-degenerate samples (the rest is
             LAPACK round-off on ill-conditioned systems, SURVEY A.2: the exact null vector itself
             rounds to a different float32 there)
"""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(autouse=True)
def fast_kernels_by_default():
    """The numpy-facing API defaults to the exact float64 kernel; the tolerance tests below are about the FAST
    kernels, so they force them.  Tests of the exact / default behaviour override this with `exact_mode` / `auto_mode`."""
    import ransac_with_homography_amd.homography as impl
    old = impl.EXACT
    impl.EXACT = False
    yield
    impl.EXACT = old


@pytest.fixture(scope="module")
def gpu():
    from ransac_with_homography_amd import _lib
    return _lib.require_gpu()  # raises (test error, not skip) when the HIP path is unavailable


def _force_shape(shape):
    """Pin (or release, None) the fast bilinear kernel's patch shape through the lab hook of the C ABI."""
    from ransac_with_homography_amd import _lib
    assert _lib.load().rwh_lab_tune(_lib.RWH_TUNE_WARP_SHAPE, int(shape) if shape else 0) == 0


def _force_frames(n):
    """Frames per block of the multi-frame lab kernel (warp_rgb8_fast8m; 0 = the product's one-frame kernel)."""
    from ransac_with_homography_amd import _lib
    assert _lib.load().rwh_lab_tune(_lib.RWH_TUNE_WARP_FRAMES, int(n)) == 0


@pytest.fixture(autouse=True)
def release_lab_overrides():
    yield
    _force_shape(None)
    _force_frames(0)
    from ransac_with_homography_amd import _lib
    assert _lib.load().rwh_lab_tune(_lib.RWH_TUNE_SCORE_HPW, 0) == 0 and _lib.load().rwh_lab_tune(_lib.RWH_TUNE_SCORE_EXACT, 0) == 0


def close(gpu_img, ref):
    ref = ref.astype(np.float64)
    return np.abs(gpu_img.astype(np.float64) - ref) <= 1e-4 * np.abs(ref) + 1e-5


# ------------------------------------------------------------------------------------------------
# K3 against the reference's own outputs (G6)
# ------------------------------------------------------------------------------------------------
def test_warp_small_goldens(gpu):
    import homography as hg
    z = load_golden("g6_small_warps")
    worst = 0.0
    for iname in ("noise", "ramp"):
        img = z["img_" + iname]
        for hn in [str(h) for h in z["H_names"]]:
            H = z["H_" + hn]
            k = "wp_%s_%s_bilinear" % (iname, hn)
            src = img.copy()
            o, mx, my = hg.wrapPerspective(src, H, convert="bilinear")
            assert o.dtype == np.float64 and o.shape == z[k].shape and (mx, my) == tuple(z[k + "_org"])
            assert not src[0, 0].any()                      # caller's texel (0,0) zeroed like the reference
            ok = close(o, z[k])
            assert ok.all(), (k, np.abs(o - z[k]).max())
            worst = max(worst, np.abs(o - z[k]).max())
            k = "wp_%s_%s_nn" % (iname, hn)
            o, mx, my = hg.wrapPerspective(img.copy(), H, convert="nn")
            assert o.dtype == np.uint8 and np.array_equal(o, z[k]), k
            # fused uint8 truncation (transformImageH): +-1 LSB at most, and rarely
            o, _, _ = hg.transformImageH(img.copy(), H)
            ref = z["tih_%s_%s" % (iname, hn)]
            d = np.abs(o.astype(np.int16) - ref.astype(np.int16))
            assert d.max() <= 1 and (d != 0).mean() < 0.02, (iname, hn, d.max(), (d != 0).mean())
        o, mx, my = hg.wrapPerspective(img.copy(), z["H_rot"], convert="bilinear", boundary=1)
        assert (mx, my) == tuple(z["wpb_%s_rot_bilinear_org" % iname]) and close(o, z["wpb_%s_rot_bilinear" % iname]).all()
        hs, ws, _ = img.shape
        for hn in ("bench", "rot"):
            o, _, _ = hg.wrapPerspectiveScan(img.copy(), z["H_" + hn], (hs - 8, ws - 16), convert="bilinear")
            assert close(o, z["scan_%s_%s_bilinear" % (iname, hn)]).all()
            o, _, _ = hg.wrapPerspectiveScan(img.copy(), z["H_" + hn], (hs - 8, ws - 16), convert="nn")
            assert np.array_equal(o, z["scan_%s_%s_nn" % (iname, hn)])
        rgba = z["rgba_" + iname]
        o, _, _ = hg.wrapPerspective(rgba.copy(), z["H_notebook"], convert="bilinear")
        assert o.dtype == np.float64 and close(o, z["wp4_%s_notebook_bilinear" % iname]).all()
        o, _, _ = hg.wrapPerspective(rgba.copy(), z["H_notebook"], convert="nn")
        assert o.dtype == np.float32 and np.array_equal(o, z["wp4_%s_notebook_nn" % iname])
    print("max |gpu-ref| over G6 bilinear:", worst)


def check_pick(z, prefix, img, exact):
    assert tuple(z[prefix + "_shape"]) == img.shape
    got = img.reshape(-1)[z[prefix + "_pick"]]
    ref = z[prefix + "_vals"]
    if exact:
        assert np.array_equal(got, ref)
    elif ref.dtype == np.uint8:
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        assert d.max() <= 1 and (d != 0).mean() < 0.12, (prefix, d.max(), (d != 0).mean())
    else:
        assert close(got, ref).all(), prefix


def test_warp_notebook_and_stitch_goldens(gpu):
    """G7 (config 1: 4-point solve + warp of notebook.jpg, scanner A4 mode) and G8 (config 4 geometry)."""
    import homography as hg
    z = load_golden("g7_notebook")
    img = load_golden("img_notebook")["img"]
    o, mx, my = hg.wrapPerspective(img.copy(), z["H"], convert="bilinear")
    assert (mx, my) == (-65, -168)
    check_pick(z, "wp_bilinear", o, exact=False)
    o, _, _ = hg.wrapPerspective(img.copy(), z["H"], convert="nn")
    check_pick(z, "wp_nn", o, exact=True)
    check_pick(z, "ti", hg.transformImage(img.copy(), z["u"], z["v"]), exact=False)
    check_pick(z, "ti_nn", hg.transformImage(img.copy(), z["u"], z["v"], method="nn"), exact=True)
    check_pick(z, "scan_a4", hg.transformImage(img.copy(), z["u"], z["v_a4"], box=[1188, 840]), exact=False)
    check_pick(z, "scan_a4_nn", hg.transformImage(img.copy(), z["u"], z["v_a4"], box=[1188, 840], method="nn"), exact=True)

    z = load_golden("g8_stitch")
    f = load_golden("img_foto1")
    A, B = f["A"], f["B"]
    o, mx, my = hg.transformImageH(A.copy(), z["H_notebook"])
    assert (mx, my) == (434, -90)
    check_pick(z, "tih", o, exact=False)
    check_pick(z, "stitch_paste", hg.stitchPanorama(B.copy(), A.copy(), z["H_notebook"]), exact=False)
    check_pick(z, "stitch_rate", hg.stitchPanorama(B.copy(), A.copy(), z["H_notebook"], blending="Rate", blendrate=0.2), exact=False)


# ------------------------------------------------------------------------------------------------
# K3 against the oracle on seeded inputs, edge cases, sharding, full-size properties
# ------------------------------------------------------------------------------------------------
H_BENCH = np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]])


def test_warp_vs_oracle_1080p_and_ragged(gpu):
    import homography as hg
    from oracle import rwh_oracle as orc
    rng = np.random.default_rng(1234)
    for (h, w) in ((1080, 1920), (37, 53), (5, 7), (130, 259)):   # ragged widths: not multiples of 4 / 256
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref, rmx, rmy = orc.wrap_perspective(img.copy(), H_BENCH, convert="bilinear")
        o, mx, my = hg.wrapPerspective(img.copy(), H_BENCH, convert="bilinear")
        assert (mx, my) == (rmx, rmy) and o.shape == ref.shape
        assert close(o, ref).all(), ((h, w), np.abs(o - ref).max())
        ref, _, _ = orc.wrap_perspective(img.copy(), H_BENCH, convert="nn")
        o, _, _ = hg.wrapPerspective(img.copy(), H_BENCH, convert="nn")
        assert np.array_equal(o, ref), (h, w)


def test_warp_row_shards_and_batch_match_full(gpu):
    """Output-row tiles (the multi-GPU unit) and batched images reproduce the full single launch bit for bit."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(5)
    src = torch.from_numpy(rng.integers(0, 256, (3, 300, 517, 3), dtype=np.uint8)).to(gpu)
    inv = np.linalg.inv(H_BENCH)
    grid = kernels.Grid(-3, 530, 534, -2, 310, 313)
    full = kernels.warp_backward(src, inv, grid, (300, 517), "bilinear", torch.uint8)
    assert full.shape == (3, 313, 534, 3)
    parts = [kernels.warp_backward(src, inv, grid, (300, 517), "bilinear", torch.uint8, rows=r)
             for r in ((0, 101), (101, 102), (102, 102), (102, 313))]
    assert torch.equal(torch.cat(parts, dim=1), full)
    for b in range(3):
        one = kernels.warp_backward(src[b].contiguous(), inv, grid, (300, 517), "bilinear", torch.uint8)
        assert torch.equal(one, full[b])
    # fused u8 conversion == truncating the float result, except values within 3e-5 below an integer
    # (the u8 path computes floor(v + 2^-15), see rwh_warp_rgb8.h)
    f32 = kernels.warp_backward(src, inv, grid, (300, 517), "bilinear", torch.float32)
    d = (f32.to(torch.uint8).to(torch.int16) - full.to(torch.int16))
    assert int(d.abs().max()) <= 1 and float((d != 0).float().mean()) < 2e-4
    frac = f32 - torch.floor(f32)
    assert bool(((d == 0) | (frac > 1 - 1e-4)).all())


def test_warp_4k_translation_and_linearity(gpu):
    """Size-independent properties at the BASELINE size (3840x2160 RGB u8):
    an integer translation must reproduce the source exactly; the warp is linear in the image."""
    from ransac_with_homography_amd import kernels
    g = torch.Generator(device="cpu").manual_seed(1234)
    src = torch.randint(0, 256, (2160, 3840, 3), dtype=torch.uint8, generator=g).to(gpu)
    T = np.array([[1.0, 0, 17.0], [0, 1.0, -9.0], [0, 0, 1.0]])
    grid = kernels.Grid(0, 3839, 3840, 0, 2159, 2160)
    out = kernels.warp_backward(src.clone(), np.linalg.inv(T), grid, (2160, 3840), "bilinear", torch.uint8)
    # output (x,y) samples source (x-17, y+9); valid where that is inside [0,w-1]x[0,h-1]
    srcz = src.clone()
    srcz[0, 0] = 0                                   # the warp blanks source texel (0,0) first
    exp = torch.zeros_like(src)
    exp[0:2160 - 9, 17:3840] = srcz[9:2160, 0:3840 - 17]
    assert torch.equal(out, exp)
    # linearity (float32 output): warp(a) + warp(b) == warp(a+b) within float32 rounding
    a = (src // 2).contiguous(); b = (src - a).contiguous()
    inv = np.linalg.inv(H_BENCH)
    wa = kernels.warp_backward(a, inv, grid, (2160, 3840), "bilinear", torch.float32)
    wb = kernels.warp_backward(b, inv, grid, (2160, 3840), "bilinear", torch.float32)
    ws = kernels.warp_backward(src.clone(), inv, grid, (2160, 3840), "bilinear", torch.float32)
    assert torch.allclose(wa + wb, ws, rtol=1e-5, atol=1e-4)


def test_warp_one_homography_per_image(gpu):
    """n_h == batch: 19 images (more than two coefficient tables of 8, with a remainder), each with its own rotation /
    perspective: every image of the batched call equals its own single-image call, for the staged bilinear (u8 and
    float32 out) and nearest kernels, the exact kernel and a narrow output (the per-image launch fallback)."""
    from ransac_with_homography_amd import kernels
    g = torch.Generator(device="cpu").manual_seed(19)
    src = torch.randint(0, 256, (19, 240, 352, 3), dtype=torch.uint8, generator=g).to(gpu)
    rng = np.random.default_rng(19)
    invs = []
    for i in range(19):
        t = rng.uniform(-0.8, 0.8)
        H = np.array([[np.cos(t), -np.sin(t), rng.uniform(0, 60)], [np.sin(t), np.cos(t), rng.uniform(-30, 30)],
                      [rng.uniform(-2e-4, 2e-4), rng.uniform(-2e-4, 2e-4), 1.0]])
        invs.append(np.linalg.inv(H))
    invs = np.stack(invs)
    for (ow, oh) in ((400, 260), (100, 90)):
        grid = kernels.Grid(-10, -10 + ow - 1, ow, -6, -6 + oh - 1, oh)
        for interp, dt, exact in (("bilinear", torch.uint8, False), ("bilinear", torch.float32, False), ("nn", torch.uint8, False),
                                  ("bilinear", torch.uint8, True)):
            per = kernels.warp_backward(src, invs, grid, (240, 352), interp, dt, exact=exact)
            for i in (0, 7, 8, 15, 16, 18):
                one = kernels.warp_backward(src[i].contiguous(), invs[i], grid, (240, 352), interp, dt, exact=exact)
                assert torch.equal(per[i], one), (ow, interp, dt, exact, i)


def test_warp_8k_properties(gpu):
    """The north_star's 8K frame (7680x4320 RGB u8) through the fast kernels: an integer translation reproduces the
    source exactly (bilinear u8, bilinear float32 and nearest neighbour), a half-pixel shift is the exact average of two
    neighbours, and row shards equal the full launch."""
    from ransac_with_homography_amd import kernels
    g = torch.Generator(device="cpu").manual_seed(4321)
    src = torch.randint(0, 256, (4320, 7680, 3), dtype=torch.uint8, generator=g).to(gpu)
    src[0, 0] = 0
    grid = kernels.Grid(0, 7679, 7680, 0, 4319, 4320)
    T = np.array([[1.0, 0, -33.0], [0, 1.0, 21.0], [0, 0, 1.0]])
    exp = torch.zeros_like(src)
    exp[21:4320, 0:7680 - 33] = src[0:4320 - 21, 33:7680]
    for interp, dt in (("bilinear", torch.uint8), ("bilinear", torch.float32), ("nn", torch.uint8)):
        out = kernels.warp_backward(src, np.linalg.inv(T), grid, (4320, 7680), interp, dt, zero_origin=False)
        want = exp
        if interp == "nn":       # homography.py:110: (s + 0.5) truncates TOWARDS ZERO, so s = -1 lands on row 0, not outside
            want = exp.clone()
            want[20, 0:7680 - 33] = src[0, 33:7680]
        assert torch.equal(out.to(torch.uint8), want) and (dt != torch.float32 or torch.equal(out, want.to(torch.float32))), (interp, dt)
    Th = np.array([[1.0, 0, 0.5], [0, 1.0, 0.0], [0, 0, 1.0]])          # output x samples source x - 0.5
    half = kernels.warp_backward(src, np.linalg.inv(Th), grid, (4320, 7680), "bilinear", torch.float32, zero_origin=False)
    avg = (src[:, :-1].to(torch.float32) + src[:, 1:].to(torch.float32)) * 0.5
    assert torch.equal(half[:, 1:], avg)
    inv = np.linalg.inv(H_BENCH)
    full = kernels.warp_backward(src, inv, grid, (4320, 7680), "bilinear", torch.uint8, zero_origin=False)
    part = kernels.warp_backward(src, inv, grid, (4320, 7680), "bilinear", torch.uint8, zero_origin=False, rows=(1000, 3001))
    assert torch.equal(part, full[1000:3001])


def test_warp_error_behaviour(gpu):
    import homography as hg
    img = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(KeyError):
        hg.wrapPerspective(img, np.eye(3) * 2, convert="cubic")
    with pytest.raises(np.linalg.LinAlgError):
        hg.wrapPerspective(img, np.array([[1., 2, 3], [2, 4, 6], [0, 0, 1]]), convert="nn")   # singular -> inv raises
    with pytest.raises(ValueError):
        hg.wrapPerspective(img, np.zeros((3, 3)), convert="nn")                                # NaN bounds -> int() raises


# ------------------------------------------------------------------------------------------------
# K1 / K2 against the reference's per-hypothesis outputs (G2, G3)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g2_hyp_seed0", "g3_hyp_seed7"])
def test_dlt_and_scorer_per_hypothesis(gpu, name, matches):
    from ransac_with_homography_amd import kernels
    z = load_golden(name)
    ptsA, ptsB = matches
    pa, pb = torch.from_numpy(ptsA).to(gpu), torch.from_numpy(ptsB).to(gpu)
    idx = torch.from_numpy(z["idx"]).to(gpu)
    H, flags = kernels.dlt4_batched(pa, pb, idx)
    Hg, fl = H.cpu().numpy(), flags.cpu().numpy()
    deg = z["degenerate"]
    assert np.array_equal((fl & 1).astype(bool), deg)                 # repeated-index flag
    same = np.all(Hg.view(np.uint32) == z["H"].view(np.uint32), axis=1)
    rate = same[~deg].mean()
    print(name, "H bit-identical on", same[~deg].sum(), "/", (~deg).sum())
    assert rate >= 0.975
    assert np.all(Hg[:, 8][~deg] == 1.0)

    # K2 given the REFERENCE's H: counts, masks and losses are bit-exact for every hypothesis
    Href = torch.from_numpy(z["H"]).to(gpu)
    for method in ("fwd", "backward", "reproj"):
        best = kernels.new_best(gpu)
        counts, masks, err = kernels.score_count(Href, pa, pb, 5.0, method, kernels.need_count(185, 70, 4), best,
                                                 want_err=(method == "fwd"))
        c = counts.cpu().numpy()
        ref = z["counts_" + method].astype(np.int32)
        finite = np.isfinite(z["H"]).all(axis=1)
        assert np.array_equal(c[finite], ref[finite]), (method, int((c != ref).sum()))
        if method == "fwd":
            w, cnt, early = kernels.decode_best(best.cpu().numpy(), 10000)
            assert (w, cnt, early) == (int(z["winner"]), int(z["winner_count"]), False)
            bits = np.unpackbits(masks[w].cpu().numpy().view(np.uint8), bitorder="little")[:185]
            assert np.array_equal(np.nonzero(bits)[0], z["winner_inliers"])
            assert np.array_equal(err[w].cpu().numpy().view(np.uint32), z["winner_err"].view(np.uint32))

    # K1 -> K2 end to end: the winner is the reference's winner, with the reference's inlier set
    best = kernels.new_best(gpu)
    counts, masks, _ = kernels.score_count(H, pa, pb, 5.0, "fwd", kernels.need_count(185, 70, 4), best)
    w, cnt, early = kernels.decode_best(best.cpu().numpy(), 10000)
    assert (w, cnt, early) == (int(z["winner"]), int(z["winner_count"]), False)
    c = counts.cpu().numpy()
    nd = ~deg
    print(name, "count mismatches vs reference (non-degenerate):", int((c[nd] != z["counts_fwd"][nd]).sum()))
    assert (c[nd] != z["counts_fwd"][nd]).mean() < 0.002
    assert np.array_equal(c[same], z["counts_fwd"][same])            # identical H -> identical count


def test_ransac_run_matches_reference_runs(gpu, matches):
    """G4 (ransac.example0 parameters, 3 seeds x 3 losses), G5 (app.py parameters) and early-exit cases."""
    import ransac as rs
    z = load_golden("g4_ransac_runs")
    ptsA, ptsB = matches
    for key in [str(k) for k in z["cases"]]:
        _, s, th, d, k, method = key.split("_")
        np.random.seed(int(s[1:]))
        model = rs.HomoModel(th=int(th[2:]), d=int(d[1:]), n=4)
        H, inl, cnt = rs.RANSAC(model, k=int(k[1:])).run([ptsA.T, ptsB.T], method=method)
        assert int(cnt) == int(z[key + "_count"]), key
        assert np.array_equal(inl[0], z[key + "_inliers"]), key
        assert H.dtype == np.float64 and H.shape == (3, 3) and model.val is H
        np.testing.assert_allclose(H, z[key + "_H"], rtol=1e-3, atol=1e-6, err_msg=key)
        # generator left where the reference leaves it: replay and compare the next draw
        nxt = np.random.randint(0, 1 << 30)
        np.random.seed(int(s[1:]))
        from oracle import rwh_oracle as orc
        orc.ransac_run(ptsA.T, ptsB.T, th=int(th[2:]), d=int(d[1:]), n=4, k=int(k[1:]), method=method)
        assert nxt == np.random.randint(0, 1 << 30), key


def test_ransac_run_low_inlier_reference_winner(gpu, matches):
    """G9: contaminated problems on which the REFERENCE's winner is a sample with a repeated index (np.random.randint
    draws with replacement, LAPACK still returns a null vector, that H wins: ransac.py:177,199-202, homography.py:81-87).
    RANSAC.run must return the reference's iteration, count and inlier list -- including the case where the repeated
    sample triggers the early `break` -- and run_batch(idx=) the same."""
    import ransac as rs
    from ransac_with_homography_amd import ransac as rmod
    z = load_golden("g9_low_inlier")
    ptsA, _ = matches
    for key in [str(k) for k in z["cases"]]:
        tag, s, th, d, k, method = key.split("_")
        B = z["ptsB_" + tag]
        np.random.seed(int(s[1:]))
        model = rs.HomoModel(th=int(th[2:]), d=int(d[1:]), n=4)
        r = rs.RANSAC(model, k=int(k[1:]))
        H, inl, cnt = r.run([ptsA.T, B.T], method=method)
        w = r.last_run["winner"]
        assert w == int(z[key + "_winner"]) and len(set(z[key + "_idx"][w].tolist())) < 4, key
        assert int(cnt) == int(z[key + "_count"]) and np.array_equal(inl[0], z[key + "_inliers"]), key
        assert r.last_run["early_exit"] == bool(z[key + "_early"])
        np.testing.assert_allclose(H, z[key + "_H"], rtol=1e-3, atol=1e-6, err_msg=key)
        assert np.array_equal(r.last_run["settled"][w].view(np.uint32), z[key + "_hyp_H"][w].view(np.uint32))
        print(key, "host-settled hypotheses:", r.last_run["host_settled"], "in", r.last_run["host_rounds"], "rounds")
        assert 30 <= r.last_run["host_settled"] <= 250, r.last_run["host_settled"]   # ~3.7 % repeated + the near-best
        # generator left where the reference's loop leaves it
        nxt = np.random.randint(0, 1 << 30)
        np.random.seed(int(s[1:]))
        np.random.randint(0, 185, ((w + 1) if bool(z[key + "_early"]) else int(k[1:]), 4))
        assert nxt == np.random.randint(0, 1 << 30), key
        got = rmod.run_batch([[ptsA.T, B.T]], th=int(th[2:]), d=int(d[1:]), k=int(k[1:]), method=method, idx=[z[key + "_idx"]])
        assert int(got[0][2]) == int(cnt) and np.array_equal(got[0][1][0], inl[0]) and np.array_equal(got[0][0], H), key


def test_config5_search_100k_hypotheses(gpu, matches):
    """BASELINE config 5's search (G10: the reference's loop body over 100 000 samples, seed 0): the single search and a
    2-shard split of the hypothesis range (sharded.gpu_score_slice with hyp_base, keys merged by MAX as the all-reduce
    does) both return the reference's winner, count and inlier list; K1 + K2's raw counts differ from the reference's
    only on flagged samples and, by at most 2, on a handful of ill-conditioned ones (what RESCORE_MARGIN covers)."""
    import ransac as rs
    from ransac_with_homography_amd import kernels, sharded
    from ransac_with_homography_amd import ransac as rmod
    z = load_golden("g10_config5_search")
    ptsA, ptsB = matches
    K = int(z["K"])
    np.random.seed(0)
    r = rs.RANSAC(rs.HomoModel(th=5, d=70, n=4), k=K)
    H, inl, cnt = r.run([ptsA.T, ptsB.T], method="fwd")
    assert (r.last_run["winner"], int(cnt)) == (int(z["winner"]), int(z["winner_count"])) == (99206, 122)
    assert np.array_equal(inl[0], z["winner_inliers"]) and np.array_equal(r.last_run["idx"][99206], z["winner_sample"])
    fl = r.last_run["flags"].cpu().numpy()
    flagged = fl != 0
    from ransac_with_homography_amd import _lib
    assert int(((fl & _lib.RWH_HYP_REPEATED) != 0).sum()) == int(z["degenerate"])
    assert int((fl == _lib.RWH_HYP_ILLCOND).sum()) < 0.03 * K              # the conditioning flag alone: ~2 % of natural samples
    raw = r.last_run["raw_counts"].astype(np.int64)
    ref = z["counts"].astype(np.int64)
    diff = np.abs(raw - ref)[~flagged]
    print("config 5: raw count mismatches on unflagged samples:", int((diff != 0).sum()), "max", int(diff.max()),
          "host-settled:", r.last_run["host_settled"])
    assert diff.max() <= 3 < rmod.RESCORE_MARGIN and (diff != 0).mean() < 1e-3
    # 2 shards
    pa, pb = torch.from_numpy(ptsA).to(gpu), torch.from_numpy(ptsB).to(gpu)
    idx = r.last_run["idx"]
    keys = [sharded.gpu_score_slice(pa, pb, idx[b:e], 5.0, "fwd", kernels.need_count(185, 70, 4), b)
            for b, e in (sharded.shard_range(K, 0, 2), sharded.shard_range(K, 1, 2))]
    merged = torch.maximum(keys[0], keys[1]).cpu().numpy()
    assert kernels.decode_best(merged, K) == (99206, 122, False)
    inl2, c2 = sharded.winner_inliers(pa, pb, idx[99206], 5.0, "fwd")
    assert c2 == 122 and np.array_equal(inl2, z["winner_inliers"])


def test_batched_short_tables_exact_size_buffers(gpu, matches):
    """rwh_ransac_batched with k < 64 and P*k not a multiple of 64 (P = 3, k = 10) on buffers of EXACTLY the required
    size (hipMalloc through ctypes, no allocator slack): lanes past the last hypothesis must not index the offsets table
    or the points (they used to read offsets[t / k] for t >= P*k)."""
    import ctypes
    from ransac_with_homography_amd import _lib, kernels
    lib = _lib.load()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ptsA, ptsB = matches
    sizes, P, K = [185, 40, 7], 3, 10
    A = np.concatenate([ptsA[:m] for m in sizes]).astype(np.float32)
    B = np.concatenate([ptsB[:m] for m in sizes]).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rng = np.random.default_rng(5)
    idx = np.stack([rng.integers(0, m, (K, 4)) for m in sizes]).astype(np.int32)
    needs = np.array([kernels.need_count(m, 70, 4) for m in sizes], np.int32)
    words = 3
    bufs = {}

    def dev(name, nbytes, host=None):
        ptr = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(ptr), nbytes) == 0
        if host is not None:
            assert hip.hipMemcpy(ptr, host.ctypes.data_as(ctypes.c_void_p), nbytes, 1) == 0
        bufs[name] = (ptr, nbytes)
        return ptr

    try:
        d_a, d_b = dev("a", A.nbytes, A), dev("b", B.nbytes, B)
        d_off, d_idx, d_need = dev("off", offs.nbytes, offs), dev("idx", idx.nbytes, idx), dev("need", needs.nbytes, needs)
        d_h, d_fl, d_cnt = dev("h", P * K * 36), dev("fl", P * K), dev("cnt", P * K * 4)
        d_mask, d_best = dev("mask", P * K * words * 8), dev("best", P * 16)
        torch.cuda.synchronize()
        st = lib.rwh_ransac_batched(d_a, d_b, d_off, P, 185, K, d_idx, 0, 0, 5.0, 0, d_need, d_h, d_fl, d_cnt, d_mask, d_best, 0, None)
        assert st == 0
        torch.cuda.synchronize()
        Hout = np.empty((P, K, 9), np.float32); cnt = np.empty((P, K), np.int32)
        assert hip.hipMemcpy(Hout.ctypes.data_as(ctypes.c_void_p), d_h, Hout.nbytes, 2) == 0
        assert hip.hipMemcpy(cnt.ctypes.data_as(ctypes.c_void_p), d_cnt, cnt.nbytes, 2) == 0
    finally:
        for ptr, _ in bufs.values():
            hip.hipFree(ptr)
    for p, m in enumerate(sizes):     # every problem equals its own single search on torch buffers
        pa, pb = torch.from_numpy(A[offs[p]:offs[p] + m]).to(gpu), torch.from_numpy(B[offs[p]:offs[p] + m]).to(gpu)
        ws = kernels.SearchWorkspace(K, m, gpu)
        kernels.ransac_search(pa, pb, torch.from_numpy(idx[p]).to(gpu), 5.0, "fwd", int(needs[p]), ws)
        assert np.array_equal(ws.H.cpu().numpy().view(np.uint32), Hout[p].view(np.uint32)), p
        assert np.array_equal(ws.counts.cpu().numpy(), cnt[p]), p


def _batch_problems(matches):
    """Five problems of different sizes cut from the 185 real correspondences (3 mask words down to 1; one with
    exactly 4 points)."""
    ptsA, ptsB = matches
    rng = np.random.default_rng(11)
    sets = [np.arange(185), np.sort(rng.choice(185, 130, replace=False)), np.sort(rng.choice(185, 64, replace=False)),
            np.sort(rng.choice(185, 33, replace=False)), np.array([3, 50, 90, 140])]
    return [[ptsA[i].T.copy(), ptsB[i].T.copy()] for i in sets]


@pytest.mark.parametrize("method", ["fwd", "reproj"])
def test_batched_search_equals_single_searches(gpu, matches, method):
    """rwh_ransac_batched with the caller's index tables == one rwh_ransac_search per problem, bit for bit
    (hypotheses, flags, counts, masks, packed keys), and run_batch(idx=) == RANSAC.run on the same numpy stream."""
    import ransac as rs
    from ransac_with_homography_amd import kernels
    from ransac_with_homography_amd import ransac as rmod
    probs = _batch_problems(matches)
    K, th, d = 700, 5, 40
    tables = []
    for p, (X, _) in enumerate(probs):
        np.random.seed(100 + p)
        tables.append(np.random.randint(0, X.shape[1], (K, 4)))
    sizes = [X.shape[1] for X, _ in probs]
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=gpu)
    pa = torch.from_numpy(np.concatenate([np.ascontiguousarray(X.T[:, :2], np.float32) for X, _ in probs])).to(gpu)
    pb = torch.from_numpy(np.concatenate([np.ascontiguousarray(Y.T[:, :2], np.float32) for _, Y in probs])).to(gpu)
    needs = torch.tensor([kernels.need_count(m, d, 4) for m in sizes], dtype=torch.int32, device=gpu)
    ws = kernels.BatchWorkspace(len(probs), K, max(sizes), gpu)
    idx = torch.from_numpy(np.stack(tables).astype(np.int32)).to(gpu)
    kernels.ransac_batched(pa, pb, offsets, needs, float(th), method, ws, idx=idx)
    for p, m in enumerate(sizes):
        o = int(offsets[p])
        single = kernels.SearchWorkspace(K, m, gpu)
        kernels.ransac_search(pa[o:o + m].contiguous(), pb[o:o + m].contiguous(), idx[p].contiguous(), float(th), method,
                              kernels.need_count(m, d, 4), single)
        assert torch.equal(ws.H[p].view(torch.int32), single.H.view(torch.int32)), p
        assert torch.equal(ws.flags[p], single.flags) and torch.equal(ws.counts[p], single.counts), p
        w = (m + 63) // 64
        assert torch.equal(ws.masks[p][:, :w], single.masks) and not ws.masks[p][:, w:].any(), p
        assert torch.equal(ws.best[p], single.best), p
    got = rmod.run_batch(probs, th=th, d=d, k=K, method=method, idx=tables)
    for p, (X, Y) in enumerate(probs):
        np.random.seed(100 + p)
        H, inl, cnt = rs.RANSAC(rs.HomoModel(th=th, d=d, n=4), k=K).run([X, Y], method=method)
        assert int(got[p][2]) == int(cnt) and np.array_equal(got[p][1][0], inl[0]), p
        assert np.array_equal(got[p][0], H), p
    # the caller's tables follow numpy's indexing rules (ransac.py:178 `data[:, idx]`): negative indices wrap, others raise
    wrapped = [np.where(np.arange(t.size).reshape(t.shape) % 7 == 0, t - sizes[p], t) for p, t in enumerate(tables)]
    again = rmod.run_batch(probs, th=th, d=d, k=K, method=method, idx=wrapped)
    for p in range(len(probs)):
        assert int(again[p][2]) == int(got[p][2]) and np.array_equal(again[p][0], got[p][0]), p
    bad = [t.copy() for t in tables]
    bad[1][5, 2] = sizes[1]
    with pytest.raises(IndexError):
        rmod.run_batch(probs, th=th, d=d, k=K, method=method, idx=bad)
    bad[1][5, 2] = -sizes[1] - 1
    with pytest.raises(IndexError):
        rmod.run_batch(probs, th=th, d=d, k=K, method=method, idx=bad)
    with pytest.raises(ValueError):
        rmod.run_batch(probs, th=th, d=d, k=K, method=method, idx=tables[:-1])


def test_batched_device_sampling(gpu, matches):
    """Device Philox sampling: the index table is the documented function of (seed, problem, hypothesis), the scores on
    it are the oracle's, the result does not depend on what else is in the batch, and the early exit works per problem."""
    from oracle import rwh_oracle as orc
    from philox_ref import sample4
    from ransac_with_homography_amd import kernels
    from ransac_with_homography_amd import ransac as rmod
    probs = _batch_problems(matches)
    sizes = [X.shape[1] for X, _ in probs]
    K, seed = 512, 0x1234567890ABCDEF
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=gpu)
    pa = torch.from_numpy(np.concatenate([np.ascontiguousarray(X.T[:, :2], np.float32) for X, _ in probs])).to(gpu)
    pb = torch.from_numpy(np.concatenate([np.ascontiguousarray(Y.T[:, :2], np.float32) for _, Y in probs])).to(gpu)
    needs = torch.tensor([kernels.need_count(m, 70, 4) for m in sizes], dtype=torch.int32, device=gpu)
    ws = kernels.BatchWorkspace(len(probs), K, max(sizes), gpu)
    kernels.ransac_batched(pa, pb, offsets, needs, 5.0, "fwd", ws, seed=seed)
    idx = ws.idx.cpu().numpy()
    for p, m in enumerate(sizes):
        assert np.array_equal(idx[p], sample4(seed, p, K, m)), p
    # problem 0 (all 185 correspondences): the oracle's scores on the device-drawn samples
    X, Y = probs[0]
    Hs_ref, counts_ref = orc.ransac_table(X, Y, idx[0].astype(np.int64), th=5, method="fwd")
    c = ws.counts[0].cpu().numpy()
    same = np.all(ws.H[0].cpu().numpy().view(np.uint32) == Hs_ref.view(np.uint32), axis=1)
    assert same.mean() > 0.97 and np.array_equal(c[same], counts_ref[same])
    assert not (ws.flags[0].cpu().numpy() & 1).any()                  # distinct indices: never "repeated"
    # the 4-point problem: every hypothesis is a permutation of its 4 points
    assert (np.sort(idx[4], axis=1) == np.arange(4)).all()
    # same seed, same problem index -> same result whatever follows it in the batch
    ws2 = kernels.BatchWorkspace(2, K, max(sizes[:2]), gpu)
    kernels.ransac_batched(pa[:sizes[0] + sizes[1]], pb[:sizes[0] + sizes[1]], offsets[:3].contiguous(), needs[:2].contiguous(),
                           5.0, "fwd", ws2, seed=seed)
    assert torch.equal(ws2.best, ws.best[:2]) and torch.equal(ws2.counts, ws.counts[:2])
    # a problem list split over two calls draws the tables of the unsplit call (problem_base = global index)
    o2 = (offsets[2:] - offsets[2]).contiguous()
    ws3 = kernels.BatchWorkspace(3, K, max(sizes[2:]), gpu)
    kernels.ransac_batched(pa[int(offsets[2]):].contiguous(), pb[int(offsets[2]):].contiguous(), o2, needs[2:].contiguous(),
                           5.0, "fwd", ws3, seed=seed, problem_base=2)
    assert torch.equal(ws3.idx, ws.idx[2:]) and torch.equal(ws3.best, ws.best[2:]) and torch.equal(ws3.counts, ws.counts[2:])
    # host wrapper: finds the panorama homography's inlier set size class on the full problem, early exit at d=40
    res = rmod.run_batch(probs[:3], th=5, d=70, k=2000, method="fwd", seed=7)
    assert 110 <= int(res[0][2]) <= 125 and res[0][0].shape == (3, 3) and res[0][0].dtype == np.float64
    tail = rmod.run_batch(probs[1:3], th=5, d=70, k=2000, method="fwd", seed=7, problem_base=1)
    for a, b in zip(res[1:3], tail):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][0], b[1][0]) and int(a[2]) == int(b[2])
    res40 = rmod.run_batch(probs[:3], th=5, d=40, k=2000, method="fwd", seed=7)
    for (X, _), r in zip(probs[:3], res40):
        assert int(r[2]) >= X.shape[1] * 40 / 100 + 4


def test_batched_early_stop_and_device_handoff(gpu, matches):
    """f-3: (i) RWH_BATCH_EARLY_STOP -- the `break` of ransac.py:186-190 as saved work: with d = 40 every problem exits early,
    far fewer hypotheses are scored, and winner / count / mask / keys are exactly those of the run that scores everything;
    with d = 70 (no exit) nothing is skipped; (ii) DeviceProblems: correspondences that already live on the GPU give the
    same results as the list-of-arrays form, and with refit=False nothing but the winners' masks comes back."""
    from ransac_with_homography_amd import kernels
    from ransac_with_homography_amd import ransac as rmod
    probs = _batch_problems(matches)[:4]
    sizes = [X.shape[1] for X, _ in probs]
    K, seed = 4096, 77
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=gpu)
    pa = torch.from_numpy(np.concatenate([np.ascontiguousarray(X.T[:, :2], np.float32) for X, _ in probs])).to(gpu)
    pb = torch.from_numpy(np.concatenate([np.ascontiguousarray(Y.T[:, :2], np.float32) for _, Y in probs])).to(gpu)
    for d, expect_exit in ((40, True), (70, False)):
        needs = torch.tensor([kernels.need_count(m, d, 4) for m in sizes], dtype=torch.int32, device=gpu)
        full = kernels.BatchWorkspace(len(probs), K, max(sizes), gpu)
        kernels.ransac_batched(pa, pb, offsets, needs, 5.0, "fwd", full, seed=seed)
        stop = kernels.BatchWorkspace(len(probs), K, max(sizes), gpu)
        kernels.ransac_batched(pa, pb, offsets, needs, 5.0, "fwd", stop, seed=seed, early_stop=True)
        # word 1 (the exit) is the same; word 0 (max count so far) is the same unless an exit cut the problem short -- the
        # reference never looks at hypotheses past its `break` either
        assert torch.equal(stop.best[:, 1], full.best[:, 1]) and torch.equal(stop.idx, full.idx)
        assert expect_exit or torch.equal(stop.best, full.best)
        for p in range(len(probs)):
            assert kernels.decode_best(stop.best[p].cpu().numpy(), K) == kernels.decode_best(full.best[p].cpu().numpy(), K)
        scored = (stop.counts >= 0)
        assert torch.equal(stop.counts[scored], full.counts[scored]) and torch.equal(stop.masks[scored], full.masks[scored])
        assert not stop.masks[~scored].any()
        if expect_exit:
            # problems with more than 4 096 correspondences (mask rows longer than one wavefront: the general scorer) into
            # a buffer full of ones: every word of a skipped hypothesis must come back zero
            big = [np.concatenate([X] * 40, axis=1) for X, _ in probs[:2]], [np.concatenate([Y] * 40, axis=1) for _, Y in probs[:2]]
            bs = [x.shape[1] for x in big[0]]
            assert min(bs) > 4096
            boffs = torch.tensor(np.concatenate([[0], np.cumsum(bs)]), dtype=torch.int32, device=gpu)
            bpa = torch.from_numpy(np.concatenate([np.ascontiguousarray(x.T[:, :2], np.float32) for x in big[0]])).to(gpu)
            bpb = torch.from_numpy(np.concatenate([np.ascontiguousarray(y.T[:, :2], np.float32) for y in big[1]])).to(gpu)
            bneeds = torch.tensor([kernels.need_count(m, d, 4) for m in bs], dtype=torch.int32, device=gpu)
            bws = kernels.BatchWorkspace(2, 16384, max(bs), gpu)      # enough hypotheses that late waves start after the first exit
            bws.masks.fill_(-1)
            kernels.ransac_batched(bpa, bpb, boffs, bneeds, 5.0, "fwd", bws, seed=seed, early_stop=True)
            skipped = bws.counts < 0
            assert bws.masks.shape[2] > 64 and bool(skipped.any()) and not bws.masks[skipped].any()
        best = full.best.cpu().numpy()
        for p in range(len(probs)):
            w, _, early = kernels.decode_best(best[p], K)
            assert early == expect_exit, (d, p)
            n_scored = int(scored[p].sum())
            if early:
                assert bool(scored[p, : w + 1].all())            # everything up to the exit was scored
                print("d=%d problem %d: exit at %d, scored %d of %d" % (d, p, w, n_scored, K))
            else:
                assert n_scored == K
        if expect_exit:
            # (all 16 384 waves of this small batch are resident almost at once -- 8 192 fit the chip -- so about a third
            #  still start before the first exit is on record; the saving grows with the batch)
            assert int(scored.sum()) < 0.6 * scored.numel()
    # host wrapper: DeviceProblems == list of arrays, and the info dict reports the saved work
    dp = rmod.DeviceProblems(pa, pb, sizes)
    info = {}
    a = rmod.run_batch(probs, th=5, d=40, k=K, method="fwd", seed=seed)
    b = rmod.run_batch(dp, th=5, d=40, k=K, method="fwd", seed=seed, info=info)
    c = rmod.run_batch(dp, th=5, d=40, k=K, method="fwd", seed=seed, refit=False)
    for ra, rb, rc in zip(a, b, c):
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1][0], rb[1][0]) and int(ra[2]) == int(rb[2])
        assert rc[0] is None and np.array_equal(rc[1][0], ra[1][0]) and int(rc[2]) == int(ra[2])
    assert all(info["early"]) and int(info["scored"].sum()) < 0.6 * K * len(probs)


def test_scorer_threshold_edges(gpu):
    """`err < th` is decided on the squared error against a host-computed limit (no square root per pair): the decision
    must equal the oracle's `sqrt(...) < th` for thresholds sitting exactly on, one ulp below and one ulp above
    attainable error values, as float32 and as float64 thresholds, and for degenerate thresholds."""
    from oracle import rwh_oracle as orc
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(3)
    M = 150
    X = rng.uniform(0, 2000, (2, M)).astype(np.float32)
    d = np.array([[3, 4], [1, 1], [0, 0], [5, 12], [0.5, 0.25], [1e-3, 2e-3], [300, 400]], dtype=np.float32)
    Y = (X + d[rng.integers(0, len(d), M)].T).astype(np.float32)
    Hs = np.stack([np.eye(3, dtype=np.float32).reshape(9),
                   np.array([1.001, 2e-4, 0.5, -3e-4, 0.999, -0.25, 1e-7, -2e-7, 1], dtype=np.float32)])
    pa = torch.from_numpy(np.ascontiguousarray(X.T)).to(gpu)
    pb = torch.from_numpy(np.ascontiguousarray(Y.T)).to(gpu)
    Hd = torch.from_numpy(Hs).to(gpu)
    for method in ("fwd", "backward"):
        errs = [orc.compute_loss(h.reshape(3, 3), X, Y, method) for h in Hs]
        ths = [0.0, -1.0, float("inf"), float("nan"), 1e-30, 5, 5.0, np.float32(5.0), np.float64(np.nextafter(np.float32(5), np.float32(6))),
               np.nextafter(5.0, 6.0), np.nextafter(5.0, 4.0)]
        for e in np.unique(np.concatenate(errs))[::7]:
            ths += [np.float64(e), np.nextafter(np.float64(e), np.inf), np.nextafter(np.float64(e), -np.inf)]
        for th in ths:
            best = kernels.new_best(gpu)
            counts, masks, _ = kernels.score_count(Hd, pa, pb, float(th), method, 1 << 30, best)
            for i, e in enumerate(errs):
                want = e.astype(np.float64) < float(th)
                bits = np.unpackbits(masks[i].cpu().numpy().view(np.uint8), bitorder="little")[:M].astype(bool)
                assert np.array_equal(bits, want) and int(counts[i]) == int(want.sum()), (method, th, i)


def test_scorer_filter_never_changes_a_decision(gpu):
    """K2 decides most pairs from a * rcp(den) and a proven error band, and re-does a hypothesis with the two IEEE
    divisions when any pair is inside the band (score_filter_kernel).  Counts and masks must equal the all-exact
    kernel's (rwh_lab_tune RWH_TUNE_SCORE_EXACT) and the oracle's on inputs built to stress the band: pairs exactly on,
    and one ulp around, the threshold; coordinates up to 1e5; hypotheses with a horizon crossing the points (den ~ 0),
    huge, tiny, infinite and NaN entries; thresholds from 1e-3 to 1e4."""
    from oracle import rwh_oracle as orc
    from ransac_with_homography_amd import kernels, _lib
    lib = _lib.load()
    rng = np.random.default_rng(77)
    for M, scale in ((185, 1200.0), (256, 1e5), (70, 30.0)):
        X = rng.uniform(0, scale, (2, M)).astype(np.float32)
        base = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [1e-6, -2e-6, 1.0]])
        P = base @ np.vstack([X.astype(np.float64), np.ones(M)])
        Y = (P[:2] / P[2]).astype(np.float32)
        kind = rng.integers(0, 4, M)
        Y[:, kind == 1] += rng.normal(0, 3.0, (2, int((kind == 1).sum()))).astype(np.float32)        # around a 5 px threshold
        Y[:, kind == 2] = rng.uniform(0, scale, (2, int((kind == 2).sum()))).astype(np.float32)      # outliers
        Y[0, kind == 3] += np.float32(5.0)                                                           # (nearly) on the threshold
        hs = [base.astype(np.float32).reshape(9)]
        for _ in range(120):
            hs.append((base + rng.normal(0, 1, (3, 3)) * np.array([[1e-3, 1e-3, 1.0], [1e-3, 1e-3, 1.0], [1e-7, 1e-7, 1e-3]])).astype(np.float32).reshape(9))
        for sc in (1e-30, 1e-20, 1e20, 1e30):                                                        # H is homogeneous: same answers, other magnitudes
            hs.append((base * sc).astype(np.float32).reshape(9))
        for j in range(12):                                                                          # the horizon through point j: den ~ 0 there
            h = base.copy(); h[2] = [1.0 / max(X[0, j], 1.0), 0.0, -1.0 if X[0, j] >= 1.0 else -X[0, j]]
            hs.append(h.astype(np.float32).reshape(9))
        for bad in (np.nan, np.inf, -np.inf, 0.0):
            for pos in (0, 4, 8):
                h = base.astype(np.float32).reshape(9).copy(); h[pos] = bad
                hs.append(h)
        hs.append(np.zeros(9, np.float32))
        Hs = np.stack(hs)
        pa = torch.from_numpy(np.ascontiguousarray(X.T)).to(gpu)
        pb = torch.from_numpy(np.ascontiguousarray(Y.T)).to(gpu)
        Hd = torch.from_numpy(Hs).to(gpu)
        for method in ("fwd", "backward", "reproj"):
            with np.errstate(all="ignore"):
                errs = []
                for h in Hs:
                    try:
                        errs.append(orc.compute_loss(h.reshape(3, 3), X, Y, method))
                    except np.linalg.LinAlgError:                    # singular H in 'backward' / 'reproj': the reference raises
                        errs.append(None)
            fin = np.concatenate([e[np.isfinite(e)] for e in errs if e is not None])
            ths = [1e-3, 0.5, 5.0, 40.0, 1e4] + [float(v) for v in np.sort(fin[(fin > 1e-2) & (fin < 1e3)])[::97][:6]]
            for th in ths:
                got = {}
                for exact in (1, 0):
                    assert lib.rwh_lab_tune(_lib.RWH_TUNE_SCORE_EXACT, exact) == 0
                    try:
                        counts, masks, _ = kernels.score_count(Hd, pa, pb, th, method, 1 << 30, kernels.new_best(gpu))
                    finally:
                        lib.rwh_lab_tune(_lib.RWH_TUNE_SCORE_EXACT, 0)
                    got[exact] = (counts.cpu().numpy(), masks.cpu().numpy())
                assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), (M, method, th)
                # against the oracle: every hypothesis for 'fwd'; the well-conditioned ones for the losses that invert H
                # (the device inverts with its own float64 LU: equal to LAPACK's after the float32 rounding on ordinary
                # matrices, not promised on singular / overflowing ones, where the reference raises or returns inf)
                for i, e in enumerate(errs[:len(errs) if method == "fwd" else 121]):
                    if e is None:
                        continue
                    want = e.astype(np.float64) < th
                    bits = np.unpackbits(got[0][1][i].view(np.uint8), bitorder="little")[:M].astype(bool)
                    assert np.array_equal(bits, want), (M, method, th, i)


def test_scorer_filter_random_problems(gpu):
    """A short run of tools/soak_ransac.py inside the suite: filter kernels (registers / chunked) against the all-exact scorer
    on random problems -- sizes 5 ... 3000, coordinate scales 50 ... 1e5, thresholds 0.05 ... 40, all losses, single and
    batched entry points: counts, masks and packed keys identical."""
    from ransac_with_homography_amd import kernels, _lib
    lib = _lib.load()
    rng = np.random.default_rng(31)
    for case in range(24):
        M = int(rng.choice([5, 64, 65, 185, 256, 257, 700, 3000]))
        scale = float(rng.choice([50.0, 1200.0, 8000.0, 1e5]))
        Hs = np.array([[rng.uniform(0.7, 1.3), rng.uniform(-0.2, 0.2), rng.uniform(-50, 50)], [rng.uniform(-0.2, 0.2), rng.uniform(0.7, 1.3), rng.uniform(-50, 50)],
                       [rng.uniform(-1e-5, 1e-5), rng.uniform(-1e-5, 1e-5), 1.0]])
        A = rng.uniform(0, scale, (M, 2))
        P = np.c_[A, np.ones(M)] @ Hs.T
        B = P[:, :2] / P[:, 2:] + rng.normal(0, rng.uniform(0.1, 3.0), (M, 2))
        out = rng.random(M) < rng.uniform(0.1, 0.7)
        B[out] = rng.uniform(0, scale, (int(out.sum()), 2))
        pa, pb = torch.from_numpy(A.astype(np.float32)).to(gpu), torch.from_numpy(B.astype(np.float32)).to(gpu)
        K = int(rng.choice([7, 500, 3000]))
        idx = torch.from_numpy(rng.integers(0, M, (K, 4)).astype(np.int32)).to(gpu)
        th = float(rng.choice([0.05, 1.0, 3.0, 5.0, 40.0]))
        need = kernels.need_count(M, int(rng.integers(30, 95)), 4)
        for method in ("fwd", "backward", "reproj"):
            res = {}
            for exact in (1, 0):
                assert lib.rwh_lab_tune(_lib.RWH_TUNE_SCORE_EXACT, exact) == 0
                try:
                    ws = kernels.SearchWorkspace(K, M, gpu)
                    kernels.ransac_search(pa, pb, idx, th, method, need, ws)
                    bws = kernels.BatchWorkspace(2, K, M, gpu)
                    kernels.ransac_batched(torch.cat([pa, pa]), torch.cat([pb, pb]), torch.tensor([0, M, 2 * M], dtype=torch.int32, device=gpu),
                                           torch.tensor([need, need], dtype=torch.int32, device=gpu), th, method, bws, idx=torch.stack([idx, idx]))
                finally:
                    lib.rwh_lab_tune(_lib.RWH_TUNE_SCORE_EXACT, 0)
                res[exact] = [ws.counts.clone(), ws.masks.clone(), ws.best.clone(), bws.counts.clone(), bws.masks.clone(), bws.best.clone()]
            assert all(torch.equal(a, b) for a, b in zip(res[0], res[1])), (case, M, K, th, scale, method)
            assert torch.equal(res[0][3][0], res[0][0]) and torch.equal(res[0][3][1], res[0][0]), (case, method)


@pytest.mark.parametrize("M", [64, 65, 256, 257, 1000, 1024, 16384])
def test_scorer_any_number_of_correspondences(gpu, M):
    """SURVEY 8d scaling set: synthetic correspondences (Hs-projected uniform points + 1 px noise + 40 % outliers).
    M <= 256 keeps the points in registers (1..4 mask words), larger M streams them: K1 + K2 + accept rules against
    the oracle hypothesis by hypothesis, all three losses, single search and the batched entry point."""
    from oracle import rwh_oracle as orc
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(42 + M)
    Hs = np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]])
    A = rng.uniform(0, 4000, (M, 2))
    P = np.c_[A, np.ones(M)] @ Hs.T
    B = P[:, :2] / P[:, 2:] + rng.normal(0, 1.0, (M, 2))
    out = rng.random(M) < 0.4
    B[out] = rng.uniform(0, 4000, (int(out.sum()), 2))
    A, B = A.astype(np.float32), B.astype(np.float32)
    X, Y = A.T.copy(), B.T.copy()
    K = 200 if M <= 1024 else 48          # (the oracle loops over hypotheses in Python)
    idx = rng.integers(0, M, (K, 4))
    pa, pb = torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu)
    idx_d = torch.from_numpy(idx.astype(np.int32)).to(gpu)
    need = kernels.need_count(M, 50, 4)
    for method in ("fwd", "backward", "reproj"):
        Href, cref = orc.ransac_table(X, Y, idx, th=3, method=method)
        ws = kernels.SearchWorkspace(K, M, gpu)
        kernels.ransac_search(pa, pb, idx_d, 3.0, method, need, ws)
        same = np.all(ws.H.cpu().numpy().view(np.uint32) == Href.view(np.uint32), axis=1)
        c = ws.counts.cpu().numpy()
        nd = np.array([len(set(r)) == 4 for r in idx.tolist()])   # repeated samples are singular: NaN here, arbitrary in LAPACK
        assert np.array_equal((ws.flags.cpu().numpy() & 1).astype(bool), ~nd)
        assert same[nd].mean() > 0.95 and np.array_equal(c[same], cref[same]), (M, method, float(same[nd].mean()))
        assert np.abs(c - cref)[nd].max() <= 3                 # a 1-ulp H moves at most a few borderline pairs
        # masks agree with the counts; bits past M are clear
        bits = np.unpackbits(ws.masks.cpu().numpy().view(np.uint8), axis=1, bitorder="little")
        assert np.array_equal(bits.sum(axis=1), c) and not bits[:, M:].any()
        # accept rules on the GPU's own counts
        w, _, early = kernels.decode_best(ws.best.cpu().numpy(), K)
        assert (w, early) == orc.select_winner(c, need)
        # the batched entry point with this single problem gives the same bits
        bws = kernels.BatchWorkspace(1, K, M, gpu)
        kernels.ransac_batched(pa, pb, torch.tensor([0, M], dtype=torch.int32, device=gpu),
                               torch.tensor([need], dtype=torch.int32, device=gpu), 3.0, method, bws, idx=idx_d.view(1, K, 4))
        assert torch.equal(bws.counts[0], ws.counts) and torch.equal(bws.masks[0], ws.masks) and torch.equal(bws.best[0], ws.best)


def test_model_helpers_match_oracle(gpu, matches):
    import ransac as rs
    from oracle import rwh_oracle as orc
    z = load_golden("g2_hyp_seed0")
    ptsA, ptsB = matches
    X, Y = ptsA.T, ptsB.T
    model = rs.HomoModel(th=5, d=70, n=4)
    model.val = z["H"][int(z["winner"])].reshape(3, 3).copy()
    assert np.array_equal(model.fwd(X).view(np.uint32), orc.project_fwd(model.val, X).view(np.uint32))
    assert np.array_equal(model.reproj(Y).view(np.uint32), orc.project_back(model.val, Y).view(np.uint32))
    for m in ("fwd", "backward", "reproj"):
        assert np.array_equal(model.computeLoss(X, Y, m).view(np.uint32), orc.compute_loss(model.val, X, Y, m).view(np.uint32)), m
    idx = z["idx"][1]
    got = model.fit(X[:, idx], Y[:, idx])
    assert got.dtype == np.float32 and got.shape == (3, 3)
    assert np.array_equal(got.reshape(9).view(np.uint32), z["H"][1].view(np.uint32))     # the reference's solver itself (host SVD)
    # ... on every one of the 10 000 G2 samples, the 373 with a repeated index included (homography.py:71-88, ransac.py:52)
    import homography as hg
    for i in range(len(z["idx"])):
        H = hg.calcHomography(ptsA[z["idx"][i]], ptsB[z["idx"][i]])
        assert np.array_equal(H.reshape(9).view(np.uint32), z["H"][i].view(np.uint32)), i


def test_model_helpers_float64_and_three_row_inputs(gpu, matches):
    """After RANSAC.run model.val is the float64 refit: fwd / reproj / computeLoss then run in float64 in the reference
    (numpy promotes val @ x), and a 3 x M input keeps its own third row (ransac.py:58-62).  Bit-identical to the oracle."""
    import ransac as rs
    from oracle import rwh_oracle as orc
    z = load_golden("g4_ransac_runs")
    ptsA, ptsB = matches
    X, Y = ptsA.T, ptsB.T
    model = rs.HomoModel(th=5, d=70, n=4)
    model.val = z["g4_s0_th5_d70_k1000_fwd_H"].copy()                   # float64 3 x 3
    for P in (X, Y):
        got = model.fwd(P)
        ref = orc.project_fwd(model.val, P)
        assert got.dtype == ref.dtype == np.float64 and np.array_equal(got.view(np.uint64), ref.view(np.uint64))
        got = model.reproj(P)
        ref = orc.project_back(model.val, P)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))
    for m in ("fwd", "backward", "reproj"):
        got, ref = model.computeLoss(X, Y, m), orc.compute_loss(model.val, X, Y, m)
        assert got.dtype == ref.dtype and np.array_equal(got.view(np.uint64), ref.view(np.uint64)), m
    rng = np.random.default_rng(4)
    X3 = np.vstack([X.astype(np.float64), rng.uniform(0.5, 2.0, (1, X.shape[1]))])          # float64, third row != 1
    X3f = X3.astype(np.float32)
    g2 = load_golden("g2_hyp_seed0")
    val32 = g2["H"][int(g2["winner"])].reshape(3, 3).copy()
    for val in (model.val, val32):
        for P in (X3, X3f):
            model.val = val
            for fn, ofn in ((model.fwd, orc.project_fwd), (model.reproj, orc.project_back)):
                got, ref = fn(P), ofn(val, P)
                assert got.dtype == ref.dtype, (val.dtype, P.dtype)
                assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (val.dtype, P.dtype, fn.__name__)


@pytest.mark.parametrize("chn", [3, 4])
def test_convertfunc_on_precomputed_coordinates(gpu, chn):
    """homography.convertfunc['nn' | 'bilinear'](z_t, img, h, w, mh, mw) (homography.py:108-140) on coordinates the caller
    computed -- including out-of-range ones, exact integers, .5 ties and the image's last row / column -- equals the
    oracle's interpolators bit for bit, blanks texel (0,0) of the caller's image and (bilinear) zeroes the masked columns of
    the caller's z_t like the reference's in-place view does."""
    import homography as hg
    from oracle import rwh_oracle as orc
    rng = np.random.default_rng(5)
    h, w, mh, mw = 37, 53, 30, 40
    img8 = rng.integers(1, 256, (h, w, chn), dtype=np.uint8)
    imgf = (rng.random((h, w, chn)) * 255).astype(np.float32)
    n = mh * mw
    z = np.ones((3, n))
    z[0] = rng.uniform(-3, w + 2, n); z[1] = rng.uniform(-3, h + 2, n)
    z[0][(z[0] > w - 2) & (z[0] <= w - 1)] -= 1.0; z[1][(z[1] > h - 2) & (z[1] <= h - 1)] -= 1.0   # nn ties to the last index are fine, bilinear +1 taps are not
    z[0, :40] = np.arange(40) * 1.0; z[1, :40] = (np.arange(40) % (h - 1)) * 1.0      # exact integers (not the last row: IndexError in the reference)
    z[0, 40:80] = np.arange(40) + 0.5; z[1, 40:80] = (np.arange(40) % (h - 1)) + 0.5  # nearest-neighbour ties
    z[0, 80:90] = w - 1 - 1e-9; z[1, 90:100] = h - 1 - 1e-9                            # just inside the last column / row
    z[0, 100:105] = -1e-12; z[1, 105:110] = h - 1 + 1e-12                             # just outside
    # non-finite coordinates with the other one in range: numpy's astype(int32) makes INT_MIN of them -> masked (nn), and the
    # float comparisons of bilinear's mask are False for NaN ... which the reference then indexes with: keep those for nn only
    z_nn = z.copy()
    z_nn[0, 110:114] = np.nan; z_nn[1, 110:114] = 5.0
    z_nn[1, 114:118] = np.nan; z_nn[0, 114:118] = 7.0
    z_nn[0, 118:120] = np.inf; z_nn[1, 118:120] = 3.0; z_nn[0, 120:122] = -np.inf; z_nn[1, 120:122] = 3.0
    for img in (img8, imgf):
        with np.errstate(all="ignore"):
            zr, zg, ir, ig = z_nn.copy(), z_nn.copy(), img.copy(), img.copy()
            ref = orc.nearest_neighbor(zr, ir, h, w, mh, mw)
            got = hg.convertfunc["nn"](zg, ig, h, w, mh, mw)
        assert np.array_equal(got, ref) and not got.reshape(-1, chn)[110:122].any()        # every one of them is masked
    for img in (img8, imgf):
        for conv, ofn in (("nn", orc.nearest_neighbor), ("bilinear", orc.bilinear)):
            zr, zg, ir, ig = z.copy(), z.copy(), img.copy(), img.copy()
            ref = ofn(zr, ir, h, w, mh, mw)
            got = hg.convertfunc[conv](zg, ig, h, w, mh, mw)
            assert got.dtype == ref.dtype and got.shape == ref.shape == (mh, mw, chn)
            assert np.array_equal(got, ref), (img.dtype, conv, float(np.abs(got.astype(np.float64) - ref).max()))
            assert np.array_equal(ig, ir) and not ig[0, 0].any()        # caller's image: texel (0,0) blanked, nothing else touched
            assert np.array_equal(zg, zr)                               # caller's z_t mutated exactly like the reference's
    assert hg.bilinear is hg.convertfunc["bilinear"] and hg.nearestNeighbor is hg.convertfunc["nn"]


def test_stitching_with_injected_matches(gpu, matches):
    """Config 4 driver at native size: RANSAC (app.py parameters) + warp + 'Rate' blend == reference canvas."""
    import ransac as rs
    z = load_golden("g8_stitch")
    f = load_golden("img_foto1")
    np.random.seed(0)
    out = rs.stitching(f["A"].copy(), f["B"].copy(), blending="Rate", th=4, blendrate=0.2, d=95, k=1500, override=0,
                       matches=matches)
    check_pick(z, "stitch_g5_rate", out, exact=False)


@pytest.mark.parametrize("blending", [False, "Rate"])
def test_fast_compositor_vs_reference_and_exact(gpu, blending):
    """stitchPanorama on tensors = the staged warp kernel with the compositor epilogue (rwh::warp_rgb8_comp): the canvas is
    within 1 LSB of the reference's (G8 picks, native size, both homographies) and of the exact float64 kernel's on the x8
    canvas (13 181 x 6 313), where it must also reproduce imgQ's pixels and the empty corners exactly."""
    import homography as hg
    import ransac_with_homography_amd.homography as impl
    z = load_golden("g8_stitch")
    f = load_golden("img_foto1")
    A, B = torch.from_numpy(f["A"].copy()).to(gpu), torch.from_numpy(f["B"].copy()).to(gpu)
    key = "stitch_rate" if blending else "stitch_paste"
    out = hg.stitchPanorama(B, A.clone(), z["H_notebook"], blending=blending, blendrate=0.2).cpu().numpy()
    check_pick(z, key, out, exact=False)
    if blending:
        check_pick(z, "stitch_g5_rate", hg.stitchPanorama(B, A.clone(), z["H_g5"], blending="Rate", blendrate=0.2).cpu().numpy(), exact=False)
    # x8: fast (tensors) against exact (same tensors, EXACT forced)
    A8 = torch.from_numpy(np.ascontiguousarray(np.repeat(np.repeat(f["A"], 8, axis=0), 8, axis=1))).to(gpu)
    B8 = torch.from_numpy(np.ascontiguousarray(np.repeat(np.repeat(f["B"], 8, axis=0), 8, axis=1))).to(gpu)
    S = np.diag([8.0, 8.0, 1.0])
    H8 = S @ z["H_g5"] @ np.linalg.inv(S)
    fast = hg.stitchPanorama(B8, A8.clone(), H8, blending=blending, blendrate=0.2)
    old = impl.EXACT
    impl.EXACT = True
    try:
        exact = hg.stitchPanorama(B8, A8.clone(), H8, blending=blending, blendrate=0.2)
    finally:
        impl.EXACT = old
    assert fast.shape == exact.shape and fast.dtype == torch.uint8
    d = (fast.to(torch.int16) - exact.to(torch.int16)).abs()
    nbad = int((d > 1).sum())
    assert nbad <= 24, nbad                                      # (the pixels around imgT's blanked alpha texel (0,0))
    assert float((d != 0).float().mean()) < 0.12
    from oracle import rwh_oracle as orc
    mx, my, wt, ht = orc.output_bounds(A8.shape[0], A8.shape[1], H8, 0)
    (tsx, tsy, tex, tey), (qsx, qsy, qex, qey), (fw, fh) = orc.stitch_geometry(wt, ht, B8.shape[1], B8.shape[0], mx, my)
    assert tuple(fast.shape[:2]) == (fh, fw)
    if not blending:                                             # paste: imgQ's rectangle is imgQ, bit for bit
        assert torch.equal(fast[qsy:qey + 1, qsx:qex + 1], B8)
    outside = torch.ones((fh, fw), dtype=torch.bool, device=gpu)  # the corners neither rectangle covers stay 0
    outside[tsy:tey + 1, tsx:tex + 1] = False
    outside[qsy:qey + 1, qsx:qex + 1] = False
    assert int(outside.sum()) > 0 and not fast[outside].any()
    left = fast[qsy:qey + 1, qsx:min(tsx, qex + 1)]              # imgQ's part outside T: untouched by the blend too
    assert torch.equal(left, B8[:, : left.shape[1]])


def test_config4_panorama_8k_end_to_end(gpu, matches, auto_mode):
    """BASELINE config 4: foto1A/foto1B upsampled x8 (8192x5464), RANSAC (app.py parameters, threshold
    scaled with the image) + warp + paste, end to end on one GPU.  Scaling by a power of two is exact
    in floating point, so the x8 problem must pick the same hypothesis with the same inlier set as the
    native one, and the canvas geometry must be the native geometry scaled."""
    import homography as hg
    import ransac as rs
    f = load_golden("img_foto1")
    A8 = np.ascontiguousarray(np.repeat(np.repeat(f["A"], 8, axis=0), 8, axis=1))
    B8 = np.ascontiguousarray(np.repeat(np.repeat(f["B"], 8, axis=0), 8, axis=1))
    ptsA, ptsB = matches
    np.random.seed(0)
    m1 = rs.HomoModel(th=4, d=95, n=4)
    H1, inl1, c1 = rs.RANSAC(m1, k=1500).run([ptsA.T, ptsB.T], method="fwd")
    np.random.seed(0)
    m8 = rs.HomoModel(th=32, d=95, n=4)
    r8 = rs.RANSAC(m8, k=1500)
    H8, inl8, c8 = r8.run([(ptsA * 8).T, (ptsB * 8).T], method="fwd")
    z = load_golden("g4_ransac_runs")
    assert int(c1) == int(z["g5_s0_th4_d95_k1500_fwd_count"]) == 114
    g13 = load_golden("g13_config4_x8")                                  # the reference's own run on the scaled points
    assert int(c8) == int(g13["count"]) == 114 and r8.last_run["winner"] == int(g13["winner"]) == 40
    assert np.array_equal(inl8[0], g13["inliers"])
    np.testing.assert_allclose(H8, g13["H"], rtol=1e-3, atol=1e-3)       # float32 normal equations (refit)
    out = hg.stitchPanorama(B8, A8, H8)
    native = hg.stitchPanorama(f["B"].copy(), f["A"].copy(), H1)
    assert abs(out.shape[0] - 8 * native.shape[0]) <= 16 and abs(out.shape[1] - 8 * native.shape[1]) <= 16
    assert out.dtype == np.uint8 and out.shape[2] == 3
    # the query image is pasted unchanged; the warped part is non-trivial
    assert out[:, : B8.shape[1]].any() and out[:, B8.shape[1]:].any()
    # pixels: oracle-computed 256 x 256 canvas windows (the reference's float64 arithmetic on exactly those output
    # coordinates, homography.py:166-179 + 335-338 / 322-334), bit for bit: one straddling the seam at the right edge of
    # the pasted query image, one straddling the top edge of the warped image, one deep inside the warped part
    from oracle import rwh_oracle as orc
    h8, w8, _ = A8.shape
    mx, my, wt, ht = orc.output_bounds(h8, w8, H8, 0)
    (tsx, tsy, tex, tey), (qsx, qsy, qex, qey), (fw, fh) = orc.stitch_geometry(wt, ht, B8.shape[1], B8.shape[0], mx, my)
    assert out.shape == (fh, fw, 3)
    inv8 = np.linalg.inv(H8)
    blended = hg.stitchPanorama(B8, A8, H8, blending="Rate", blendrate=0.2)
    for (cx, cy) in ((qex - 128, (qsy + qey) // 2), ((tsx + tex) // 2, max(tsy, qsy) - 100 if max(tsy, qsy) > 100 else tsy),
                     (tex - 1500, (tsy + tey) // 2)):
        x0, y0 = max(cx, 0), max(cy, 0)
        xs, ys = np.arange(x0, x0 + 256), np.arange(y0, y0 + 256)
        in_t = ((xs >= tsx) & (xs <= tex))[None, :] & ((ys >= tsy) & (ys <= tey))[:, None]
        in_q = ((xs >= qsx) & (xs <= qex))[None, :] & ((ys >= qsy) & (ys <= qey))[:, None]
        warped = _oracle_warp_on_grid(A8, inv8, (xs - tsx + mx).astype(np.float64), (ys - tsy + my).astype(np.float64), (h8, w8))
        qwin = np.zeros((256, 256, 3), np.uint8)
        yy, xx = np.nonzero(in_q)
        qwin[yy, xx] = B8[ys[yy] - qsy, xs[xx] - qsx]
        # paste (homography.py:335-338)
        ref = np.zeros((256, 256, 3), np.uint8)
        ref[in_t] = warped.astype(np.uint8)[in_t]
        ref[in_q] = qwin[in_q]
        assert np.array_equal(out[y0:y0 + 256, x0:x0 + 256], ref), (cx, cy)
        # 'Rate' blend (homography.py:322-334): float32 canvas RGBA, alpha-weighted average on the warped rectangle
        rate = np.float32(0.2 + 1e-10)
        can = np.zeros((256, 256, 4), np.float32)
        can[:, :, :3][in_q] = qwin[in_q].astype(np.float32)
        can[:, :, 3] += 1e-10
        can[:, :, 3][in_q] = 1 + 1e-10 - 0.2
        rgba = np.concatenate([A8, np.zeros((h8, w8, 1), np.uint8)], axis=2).astype(np.float32)
        rgba[:, :, 3] = rate
        wt4 = _oracle_warp_on_grid(rgba, inv8, (xs - tsx + mx).astype(np.float64), (ys - tsy + my).astype(np.float64), (h8, w8))
        base = can[:, :, 3:4] + wt4[:, :, 3:4]
        mixed = (can[:, :, 3:4] / base) * can[:, :, :3] + (wt4[:, :, 3:4] / base) * wt4[:, :, :3]
        refb = can[:, :, :3].copy()
        refb[in_t] = mixed[in_t]
        assert np.array_equal(blended[y0:y0 + 256, x0:x0 + 256], refb.astype(np.uint8)), ("rate", cx, cy)
        del rgba


def test_config5_batch_1080p(gpu):
    """BASELINE config 5 (per-GPU share, 64 of the 512 frames): the batch in ONE launch equals frame-by-frame launches."""
    from ransac_with_homography_amd import kernels
    g = torch.Generator(device="cpu").manual_seed(7)
    src = torch.randint(0, 256, (64, 1080, 1920, 3), dtype=torch.uint8, generator=g).to(gpu)   # one GPU's 64 of the 512
    inv = np.linalg.inv(H_BENCH)
    grid = kernels.Grid(0, 1919, 1920, 0, 1079, 1080)
    full = kernels.warp_backward(src, inv, grid, (1080, 1920), "bilinear", torch.uint8)
    for b in (0, 3, 31, 63):
        assert torch.equal(kernels.warp_backward(src[b].contiguous(), inv, grid, (1080, 1920), "bilinear", torch.uint8), full[b])
    # nearest-neighbour batch path too
    nn = kernels.warp_backward(src, inv, grid, (1080, 1920), "nn", torch.uint8)
    assert torch.equal(kernels.warp_backward(src[5].contiguous(), inv, grid, (1080, 1920), "nn", torch.uint8), nn[5])
    # one homography per image (n_h == batch): every image equals its own single-image warp
    rng = np.random.default_rng(8)
    invs = np.stack([np.linalg.inv(np.array([[np.cos(t), -np.sin(t), 30 * t], [np.sin(t), np.cos(t), 5.0], [1e-5 * i, 0, 1.0]]))
                     for i, t in enumerate(rng.uniform(-0.3, 0.3, src.shape[0]))])
    for interp, dt in (("bilinear", torch.uint8), ("nn", torch.uint8), ("bilinear", torch.float32)):
        per = kernels.warp_backward(src, invs, grid, (1080, 1920), interp, dt)
        for i in (0, 3, src.shape[0] - 1):
            assert torch.equal(per[i], kernels.warp_backward(src[i].contiguous(), invs[i], grid, (1080, 1920), interp, dt)), (interp, i)


def test_config5_whole_batch_512_frames(gpu):
    """BASELINE config 5 at its full size on ONE GPU: 512 distinct 1080p frames (3.19 GB) in one launch -- every sampled
    frame equals its own single-frame launch (bilinear uint8 / float32 and nearest), also with one homography per frame."""
    from ransac_with_homography_amd import kernels
    g = torch.Generator(device=gpu).manual_seed(1234)
    src = torch.randint(0, 256, (512, 1080, 1920, 3), dtype=torch.uint8, generator=g, device=gpu)
    inv = np.linalg.inv(H_BENCH)
    grid = kernels.Grid(0, 1919, 1920, 0, 1079, 1080)
    picks = (0, 1, 255, 256, 511)
    for interp, dt in (("bilinear", torch.uint8), ("nn", torch.uint8), ("bilinear", torch.float32)):
        full = kernels.warp_backward(src, inv, grid, (1080, 1920), interp, dt)
        assert full.shape == (512, 1080, 1920, 3)
        for b in picks:
            assert torch.equal(kernels.warp_backward(src[b].contiguous(), inv, grid, (1080, 1920), interp, dt), full[b]), (interp, b)
        del full
    rng = np.random.default_rng(5)
    invs = np.stack([np.linalg.inv(np.array([[np.cos(t), -np.sin(t), 30 * t], [np.sin(t), np.cos(t), 5.0], [0, 0, 1.0]]))
                     for t in rng.uniform(-0.2, 0.2, 512)])
    per = kernels.warp_backward(src, invs, grid, (1080, 1920), "bilinear", torch.uint8)
    for b in picks:
        assert torch.equal(kernels.warp_backward(src[b].contiguous(), invs[b], grid, (1080, 1920), "bilinear", torch.uint8), per[b]), b


def _oracle_warp_on_grid(img, inv_h, xs, ys, bound_hw, snap=0.0):
    """numpy float64 restatement of homography.py:166-179 for an arbitrary output grid (the oracle's own
    interpolator on coordinates computed exactly like the reference computes them).  snap > 0: coordinates within `snap` of a
    mask edge are moved onto it first (what a kernel that rounds coordinates onto a grid of that pitch sees)."""
    from oracle import rwh_oracle as orc
    xv, yv = np.meshgrid(xs, ys)
    z = np.dstack([xv, yv, np.ones(xv.shape)]).reshape([xv.size, 3]).T
    z_t = inv_h @ z
    z_t /= z_t[-1, :]
    if snap:
        for row, lim in ((0, bound_hw[1] - 1.0), (1, bound_hw[0] - 1.0)):
            v = z_t[row]
            v[np.abs(v) <= snap] = 0.0
            v[np.abs(v - lim) <= snap] = lim
    return orc.bilinear(z_t, img.copy(), bound_hw[0], bound_hw[1], len(ys), len(xs))


@pytest.mark.parametrize("case", ["rot30", "zoom_out", "zoom_in", "horizon", "shear"])
def test_warp_fallback_paths_vs_oracle(gpu, case):
    """Geometries that leave the LDS-staged fast path: large rotation / zoom-out (footprint does not fit the
    slab), zoom-in, and a homography whose W changes sign inside the output (per-pixel reciprocal path)."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(99)
    img = rng.integers(0, 256, (300, 420, 3), dtype=np.uint8)
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    H = {"rot30": np.array([[c, -s, 150.0], [s, c, -40.0], [0, 0, 1.0]]),
         "zoom_out": np.array([[0.37, 0.0, 3.3], [0.0, 0.41, 2.2], [0, 0, 1.0]]),
         "zoom_in": np.array([[3.1, 0.0, -20.5], [0.02, 2.7, -11.25], [0, 0, 1.0]]),
         "horizon": np.array([[1.0, 0.05, 3.0], [0.02, 1.0, 2.0], [2.13e-3, 1.07e-3, 1.0]]),
         "shear": np.array([[1.0, 0.35, 0.0], [0.21, 1.0, 0.0], [1e-4, 0, 1.0]])}[case]
    inv = np.linalg.inv(H)
    if case == "horizon":   # inverse map denominator crosses zero inside this grid (no exactly-zero W: offsets are odd)
        inv = np.array([[1.0, 0.02, 3.0], [0.01, 1.0, 2.0], [-3.1e-3, -2.3e-3, 1.0]])
    xs = np.linspace(-13, 506, 520)
    ys = np.linspace(-7, 352, 360)
    ref = _oracle_warp_on_grid(img, inv, xs, ys, (300, 420))
    src = torch.from_numpy(img).to(gpu)
    grid = kernels.Grid(-13, 506, 520, -7, 352, 360)
    got = kernels.warp_backward(src, inv, grid, (300, 420), "bilinear", torch.float32).cpu().numpy()
    ok = close(got, ref)
    # discontinuity pixels: coordinates within 1e-9 of the mask edge may fall on either side
    assert (~ok).sum() <= 3, (case, int((~ok).sum()), float(np.abs(got - ref).max()))
    u8 = kernels.warp_backward(src, inv, grid, (300, 420), "bilinear", torch.uint8).cpu().numpy()
    d = np.abs(u8.astype(np.int16) - ref.astype(np.uint8).astype(np.int16))
    assert (d > 1).sum() <= 9 and (d != 0).mean() < 0.02, (case, int((d > 1).sum()), float((d != 0).mean()))


@pytest.mark.parametrize("case", ["mirror_x", "rot90", "rot180", "shift_eps"])
def test_warp_image_edge_band_vs_oracle(gpu, case):
    """Axis-aligned maps put whole output rows / columns ON the mask edge, and inv(H) round-off (rot180: sin(pi) = 1.2e-16)
    or a 1e-11 px shift puts them a hair off it.  Contract (include/rwh.h): the EXACT kernel takes the reference's decision
    bit for bit everywhere; the fast kernels agree with the reference on every pixel whose float64 coordinate is farther
    than 2^-32 px from a mask edge, and inside that band return either the reference's value or the edge texel's blend.
    (The bounds are 2 texels inside the image so that the reference's own +1 taps never raise IndexError.)"""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(77)
    img = rng.integers(1, 256, (200, 300, 3), dtype=np.uint8)           # no zeros: a masked pixel is unmistakable
    h, w = 198, 298                                                      # the `h, w` of the interpolator call (bounds)
    if case == "mirror_x":
        H = np.array([[-1.0, 0.0, w - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    elif case == "rot90":
        H = np.array([[0.0, -1.0, h - 1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    elif case == "rot180":
        t = np.pi
        H = np.array([[np.cos(t), -np.sin(t), w - 1.0], [np.sin(t), np.cos(t), h - 1.0], [0.0, 0.0, 1.0]])
    else:
        H = np.array([[1.0, 0.0, 1e-11], [0.0, 1.0, -1e-11], [0.0, 0.0, 1.0]])
    inv = np.linalg.inv(H)
    xs = np.arange(-3.0, 305.0); ys = np.arange(-2.0, 204.0)
    ref = _oracle_warp_on_grid(img, inv, xs, ys, (h, w))
    xv, yv = np.meshgrid(xs, ys)
    z = inv @ np.dstack([xv, yv, np.ones(xv.shape)]).reshape([xv.size, 3]).T
    z /= z[-1]
    sx, sy = z[0].reshape(xv.shape), z[1].reshape(xv.shape)
    eps = 2.0 ** -32
    band = (np.abs(sx) <= eps) | (np.abs(sx - (w - 1)) <= eps) | (np.abs(sy) <= eps) | (np.abs(sy - (h - 1)) <= eps)
    assert band.sum() >= 200                                            # whole border rows / columns sit in the band
    src = torch.from_numpy(img.copy()).to(gpu)
    grid = kernels.Grid(xs[0], xs[-1], len(xs), ys[0], ys[-1], len(ys))
    exact = kernels.warp_backward(src, inv, grid, (h, w), "bilinear", torch.float64, zero_origin=True, exact=True).cpu().numpy()
    assert np.array_equal(exact, ref), case
    got = kernels.warp_backward(src, inv, grid, (h, w), "bilinear", torch.float32, zero_origin=True).cpu().numpy()
    ok = close(got, ref).all(axis=2)
    assert ok[~band].all(), (case, int((~ok[~band]).sum()))
    # inside the band: the reference's value (0 when it masks) or the blend the unmasked coordinate gives
    clipped = _oracle_warp_on_grid(img, inv, xs, ys, (h, w), snap=eps)
    assert (ok | close(got, clipped).all(axis=2))[band].all(), case


@pytest.mark.parametrize("shape", ["7", "6", "5", None])
@pytest.mark.parametrize("case", ["mild", "rot4", "rot12", "rot45", "rot89", "persp"])
def test_warp_patch_shapes_vs_oracle(gpu, case, shape, monkeypatch):
    """The 8 px kernel's three patch shapes (128x4 / 64x8 / 32x16, rwh_lab_tune forces one, None = the host's
    choice) against the oracle on rotations that fit some shapes' slabs and not others, on a grid wider than one
    tile with a ragged right edge and bottom (tile shift / row clamp)."""
    from ransac_with_homography_amd import kernels
    _force_shape(shape)
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (333, 517, 3), dtype=np.uint8)

    def rot(deg, sc=1.0):
        t = np.deg2rad(deg)
        c, s, cx, cy = sc * np.cos(t), sc * np.sin(t), 258.0, 166.0
        return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0, 0, 1.0]])
    H = {"mild": np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]]),
         "rot4": rot(4), "rot12": rot(12, 1.07), "rot45": rot(45, 0.93), "rot89": rot(89.3),   # (exactly 90: integer coordinates on the last row make the reference itself index out of bounds)
         "persp": np.array([[0.9, 0.2, 11.0], [-0.15, 1.1, 30.0], [3e-4, -2e-4, 1.0]])}[case]
    inv = np.linalg.inv(H)
    xs = np.linspace(-9, 540, 550)      # 550 columns: 4 full tiles + a 38-column ragged one
    ys = np.linspace(-5, 345, 351)      # 351 rows: 21 full tile rows + 15
    ref = _oracle_warp_on_grid(img, inv, xs, ys, (333, 517))
    src = torch.from_numpy(img).to(gpu)
    grid = kernels.Grid(-9, 540, 550, -5, 345, 351)
    got = kernels.warp_backward(src, inv, grid, (333, 517), "bilinear", torch.float32).cpu().numpy()
    ok = close(got, ref)
    assert (~ok).sum() <= 3, (case, shape, int((~ok).sum()), float(np.abs(got - ref).max()))
    u8 = kernels.warp_backward(src, inv, grid, (333, 517), "bilinear", torch.uint8).cpu().numpy()
    d = np.abs(u8.astype(np.int16) - ref.astype(np.uint8).astype(np.int16))
    assert (d > 1).sum() <= 9 and (d != 0).mean() < 0.02, (case, shape, int((d > 1).sum()), float((d != 0).mean()))
    # row shards of the same launch reproduce it bit for bit (tile rows restart at the shard's first row)
    part = kernels.warp_backward(src, inv, grid, (333, 517), "bilinear", torch.uint8, rows=(100, 229)).cpu().numpy()
    assert np.array_equal(part, u8[100:229])


@pytest.mark.parametrize("shape", ["7", "6", "5"])
@pytest.mark.parametrize("case", ["mild", "rot4", "persp"])
def test_warp_multi_frame_equals_single(gpu, case, shape):
    """The multi-frame lab kernel (rwh_lab_tune RWH_TUNE_WARP_FRAMES, warp_rgb8_fast8m: a block walks its tile through n
    consecutive frames of a one-homography batch, the patch's coordinate / weight arithmetic done once) against the product's
    one-frame kernel: BIT-IDENTICAL, every patch shape, frames per block that do and do not divide the batch, on a grid with
    ragged right / bottom tiles, border patches and patches wholly outside the source, whole launches and row shards."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(21)
    imgs = rng.integers(0, 256, (7, 333, 517, 3), dtype=np.uint8)

    def rot(deg, sc=1.0):
        t = np.deg2rad(deg)
        c, s, cx, cy = sc * np.cos(t), sc * np.sin(t), 258.0, 166.0
        return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0, 0, 1.0]])
    H = {"mild": np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]]), "rot4": rot(4),
         "persp": np.array([[0.9, 0.2, 11.0], [-0.15, 1.1, 30.0], [3e-4, -2e-4, 1.0]])}[case]
    inv = np.linalg.inv(H)
    grid = kernels.Grid(-40, 609, 650, -25, 385, 411)      # overhangs the source on every side; 650 = 5 tiles + 10 columns
    src = torch.from_numpy(imgs).to(gpu)
    _force_shape(shape)
    _force_frames(0)
    ref = kernels.warp_backward(src, inv, grid, (333, 517), "bilinear", torch.uint8)
    assert "fast8<" in kernels.warp_plan(tuple(src.shape), torch.uint8, inv, grid, (333, 517), "bilinear", torch.uint8)
    for n in (2, 3, 4, 7, 16, 102, 103, 104, 107, 116):      # 100 + n: the variant with ONE staging window per block (warp_rgb8_fast8mb)
        _force_frames(n)
        assert ("fast8mb" if n > 100 else "fast8m<") in kernels.warp_plan(tuple(src.shape), torch.uint8, inv, grid, (333, 517), "bilinear", torch.uint8)
        got = kernels.warp_backward(src, inv, grid, (333, 517), "bilinear", torch.uint8)
        assert torch.equal(got, ref), (case, shape, n, int((got != ref).sum()))
        part = kernels.warp_backward(src, inv, grid, (333, 517), "bilinear", torch.uint8, rows=(100, 229))
        assert torch.equal(part, ref[:, 100:229]), (case, shape, n)
    # and the one-frame kernel's own check against the oracle holds for what both produce
    xs, ys = np.linspace(-40, 609, 650), np.linspace(-25, 385, 411)
    o = _oracle_warp_on_grid(imgs[3], inv, xs, ys, (333, 517))
    d = np.abs(ref[3].cpu().numpy().astype(np.int16) - o.astype(np.uint8).astype(np.int16))
    assert (d > 1).sum() <= 9, (case, shape, int((d > 1).sum()))


def test_warp_multi_frame_random_cases(gpu):
    """Round 4 regression: 160 random launches (the generator of tools/soak_mf.py, seed 81) of both multi-frame lab kernels against the
    one-frame kernel, bit for bit.  Before the fix a border wave that fell back to the one-frame body indexed the block's slab array with
    THAT body's per-wave stride (5 040 B) inside the multi-frame kernel's 5 168 B slots and overwrote the end of its interior neighbour's
    window: a few pixels on patch edges wrong in 3 % of such launches (cases 12, 47, 60, 80, 85, 99, 107, 128 of this stream), differently
    every time -- the fixed-geometry test above never saw it."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(81)
    for case in range(160):
        sh, sw = int(rng.integers(40, 900)), int(rng.integers(140, 1500))
        nb = int(rng.integers(2, 12))
        img = torch.randint(0, 256, (nb, sh, sw, 3), dtype=torch.uint8, device=gpu)
        t = rng.uniform(-np.pi, np.pi) if case % 4 == 0 else rng.uniform(-0.08, 0.08)
        sx, sy = rng.uniform(0.6, 1.6, 2) if case % 5 == 0 else rng.uniform(0.9, 1.15, 2)
        A = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]) @ np.array([[sx, rng.uniform(-0.1, 0.1)], [0, sy]])
        H = np.eye(3); H[:2, :2] = A
        H[:2, 2] = rng.uniform(-60, 60, 2) + np.array([sw / 2, sh / 2]) - A @ np.array([sw / 2, sh / 2])
        H[2, :2] = rng.uniform(-2e-4, 2e-4, 2) if case % 7 else rng.uniform(-2e-3, 2e-3, 2)
        inv = np.linalg.inv(H)
        ow, oh = int(rng.integers(128, 1900)), int(rng.integers(5, 1100))
        x0, y0 = rng.uniform(-120, 60, 2)
        stepx, stepy = rng.uniform(0.85, 1.2, 2)
        grid = kernels.Grid(x0, x0 + stepx * (ow - 1), ow, y0, y0 + stepy * (oh - 1), oh)
        bound = (sh, sw) if case % 4 else (int(rng.integers(sh // 2, sh + 1)), int(rng.integers(sw // 2, sw + 1)))
        shape = int(rng.choice([0, 0, 5, 6, 7]))
        rows = None if case % 3 else tuple(sorted(int(v) for v in rng.integers(0, oh + 1, 2)))
        if rows is not None and rows[0] == rows[1]:
            rows = None
        ns = (int(rng.integers(2, 6)), 100 + int(rng.integers(2, 6)))
        _force_shape(shape)
        _force_frames(1)
        ref = kernels.warp_backward(img, inv, grid, bound, "bilinear", torch.uint8, zero_origin=False, rows=rows)
        for n in ns:
            _force_frames(n)
            for _ in range(2):          # (the race showed differently from launch to launch)
                got = kernels.warp_backward(img, inv, grid, bound, "bilinear", torch.uint8, zero_origin=False, rows=rows)
                assert torch.equal(got, ref), (case, shape, n, int((got != ref).sum()))


@pytest.mark.parametrize("case", ["zoom1p4", "zoom1p6", "zoom2", "zoom2_rot3", "persp_zoom", "zoom3"])
def test_warp_minification_halves(gpu, case, monkeypatch):
    """Minification: when no whole patch fits its staging window the host picks the kernel that stages a patch by halves
    (rwh_warp_rgb8.h, HALVES).  Its arithmetic is the whole-patch kernel's, so the output must be BIT-IDENTICAL to the same
    patch shape run with gathers (shapes 13 / 14 vs 5 / 6), whatever fits; and both are checked against the oracle."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(11)
    sh, sw = 700, 1100
    img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)

    def zoom(s, deg=0.0):          # minification s about the image centre: output pixel spacing = s source texels
        t = np.deg2rad(deg)
        c, s_, cx, cy = np.cos(t) / s, np.sin(t) / s, sw / 2, sh / 2
        return np.array([[c, -s_, cx - c * cx + s_ * cy], [s_, c, cy - s_ * cx - c * cy], [0, 0, 1.0]])
    H = {"zoom1p4": zoom(1.4), "zoom1p6": zoom(1.6), "zoom2": zoom(2.0), "zoom2_rot3": zoom(1.9, 3.0), "zoom3": zoom(3.1),      # (exactly 3: a coordinate lands on the last column and the reference itself indexes out of bounds)
         "persp_zoom": zoom(1.5) @ np.array([[1, 0.02, 0], [0.01, 1, 0], [2e-4, 1e-4, 1.0]])}[case]
    inv = np.linalg.inv(H)
    # the grid overhangs the warped image on every side (border patches, patches wholly outside) and is ragged
    ow, oh = int(sw / 1.3) + 37, int(sh / 1.3) + 11
    x0, y0 = sw / 2 - ow / 2 - 3.5, sh / 2 - oh / 2 + 2.25
    xs, ys = np.linspace(x0, x0 + ow - 1, ow), np.linspace(y0, y0 + oh - 1, oh)
    grid = kernels.Grid(xs[0], xs[-1], ow, ys[0], ys[-1], oh)
    src = torch.from_numpy(img).to(gpu)
    ref = _oracle_warp_on_grid(img, inv, xs, ys, (sh, sw))
    outs = {}
    for shape in (None, "5", "13", "6", "14"):
        _force_shape(shape)
        outs[shape] = kernels.warp_backward(src, inv, grid, (sh, sw), "bilinear", torch.uint8)
        plan = kernels.warp_plan((sh, sw, 3), torch.uint8, inv, grid, (sh, sw), "bilinear", torch.uint8)
        if shape in ("13", "14"): assert "fast8h" in plan, plan
        # the host's own choice: halves while staging pays (a window of <= 4 texels per output pixel), gathers beyond
        if shape is None and case in ("zoom1p4", "zoom1p6"): assert "fast8h" in plan, plan
        if shape is None and case in ("zoom2", "zoom3"): assert "fast8h" not in plan, plan
    _force_shape(None)
    assert torch.equal(outs["13"], outs["5"]) and torch.equal(outs["14"], outs["6"])
    for shape, o in outs.items():
        d = np.abs(o.cpu().numpy().astype(np.int16) - ref.astype(np.uint8).astype(np.int16))
        # (an axis-aligned zoom by 1.4 / 1.6 / 2 puts the fractions on a lattice where many float64 blends are exact integers:
        #  the float32 blend then lands a hair under some of them and truncates to one less -- 1 LSB, up to ~3 % of the bytes)
        assert (d > 1).sum() <= 9 and (d != 0).mean() < 0.05, (case, shape, int((d > 1).sum()), float((d != 0).mean()))
    # row shards agree bit for bit with the whole launch (the shape is a function of the whole grid)
    part = kernels.warp_backward(src, inv, grid, (sh, sw), "bilinear", torch.uint8, rows=(64, 203))
    assert torch.equal(part, outs[None][64:203])


def test_warp_minification_halves_per_image(gpu, monkeypatch):
    """Batches with one homography per image: images whose homography minifies go to `warp_rgb8_fast8h_tab`, the others to
    the whole-patch table kernel; every image equals its single-image launch bit for bit.  (uint8 RGBA keeps its gathers at
    every minification -- they are faster there -- so its plan never names a halves kernel.)"""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(77)
    sh, sw = 420, 900

    def zoom(s, deg=0.0, px=0.0):
        t = np.deg2rad(deg)
        c, s_, cx, cy = np.cos(t) / s, np.sin(t) / s, sw / 2, sh / 2
        return np.array([[c, -s_, cx - c * cx + s_ * cy], [s_, c, cy - s_ * cx - c * cy], [px, 0, 1.0]])
    ow, oh = 701, 333
    grid = kernels.Grid(90.5, 90.5 + ow - 1, ow, 40.25, 40.25 + oh - 1, oh)
    assert "fast8h" not in kernels.warp_plan((sh, sw, 4), torch.uint8, np.linalg.inv(zoom(1.45, 1.0)), grid, (sh, sw), "bilinear", torch.uint8)
    # one homography per image: minifying and non-minifying images in one call
    n = 11
    imgs = torch.from_numpy(rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)).to(gpu)
    Hs = [zoom(1.5), zoom(1.0, 2.0), zoom(1.4, 8.0), zoom(1.7), zoom(2.6), zoom(1.0), zoom(1.55, 0.0, 1e-4), zoom(0.8), zoom(1.35, -3.0),
          zoom(1.5), zoom(1.2, 30.0)]
    invs = np.stack([np.linalg.inv(h) for h in Hs])
    per = kernels.warp_backward(imgs, invs, grid, (sh, sw), "bilinear", torch.uint8)
    plans = set()
    for i in range(n):
        one = kernels.warp_backward(imgs[i].contiguous(), invs[i], grid, (sh, sw), "bilinear", torch.uint8)
        assert torch.equal(per[i], one), i
        plans.add(kernels.warp_plan((sh, sw, 3), torch.uint8, invs[i], grid, (sh, sw), "bilinear", torch.uint8))
    assert any("fast8h" in p for p in plans) and any("fast8<" in p for p in plans), plans


@pytest.mark.parametrize("c0", [127.002, 127.001, 127.0008])
def test_warp_patch_next_to_the_horizon(gpu, c0, monkeypatch):
    """A 128-pixel patch whose denominator stays positive but reaches 0.002 at its last column: the source x coordinate runs
    from +3 (valid) to -2.3e6.  Below -1.5 * 2^20 the magic-number sum s + MAGIC turns negative and its high dword no longer
    encodes floor(s); for s in (-3 * 2^20, -1.5 * 2^20) a 32-bit subtraction used to wrap the footprint's minimum around to a
    large POSITIVE texel index (round 3: clamped before the subtraction).  Every fast kernel, every patch shape, against the
    exact float64 kernel; and whole patches far outside the source (the early exit of round 3) come out as zeros."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(3)
    img = rng.integers(1, 256, (64, 64, 3), dtype=np.uint8)
    src = torch.from_numpy(img).to(gpu)
    ih = np.array([[-40.0, 0, 400.0], [-5.0, 0, 5 * c0], [-1.0, 0, c0]])      # x = (400 - 40 c) / (c0 - c), y = 5, W = c0 - c
    grid = kernels.Grid(0, 255, 256, 0, 15, 16)
    for shape in ("7", "6", "5", None):
        _force_shape(shape)
        ex = kernels.warp_backward(src, ih, grid, (64, 64), "bilinear", torch.float64, zero_origin=False, exact=True)
        assert int((ex != 0).any(dim=2).sum()) == 176            # columns 0..10 of 16 rows
        f = kernels.warp_backward(src, ih, grid, (64, 64), "bilinear", torch.float32, zero_origin=False)
        u = kernels.warp_backward(src, ih, grid, (64, 64), "bilinear", torch.uint8, zero_origin=False)
        assert float((f.double() - ex).abs().max()) < 1e-4 * 255, shape
        assert int((u.to(torch.int16) - ex.to(torch.uint8).to(torch.int16)).abs().max()) <= 1, shape
        nn_e = kernels.warp_backward(src, ih, grid, (64, 64), "nn", torch.uint8, zero_origin=False, exact=True)
        nn_f = kernels.warp_backward(src, ih, grid, (64, 64), "nn", torch.uint8, zero_origin=False)
        assert torch.equal(nn_e, nn_f), shape
    _force_shape(None)
    # far outside on each side: zeros (uint8, float32, RGBA)
    img4 = torch.from_numpy(rng.integers(1, 256, (64, 64, 4), dtype=np.uint8)).to(gpu)
    for tx, ty in ((-3.0e6, 0.0), (3.0e6, 0.0), (0.0, -2.0e5), (0.0, 7.0e4), (-2.0e6, 3.0e6)):
        ih2 = np.array([[1.0, 0.001, tx], [0.002, 1.0, ty], [1e-6, 0, 1.0]])
        for s_, dt in ((src, torch.uint8), (src, torch.float32), (img4, torch.uint8)):
            out = kernels.warp_backward(s_, ih2, grid, (64, 64), "bilinear", dt, zero_origin=False)
            assert int(torch.count_nonzero(out)) == 0, (tx, ty, dt)


def _oracle_nn_on_grid(img, inv_h, xs, ys, bound_hw):
    """homography.py:166-179 with the nearest-neighbour interpolator on an arbitrary output grid."""
    from oracle import rwh_oracle as orc
    xv, yv = np.meshgrid(xs, ys)
    z = np.dstack([xv, yv, np.ones(xv.shape)]).reshape([xv.size, 3]).T
    z_t = inv_h @ z
    z_t /= z_t[-1, :]
    return orc.nearest_neighbor(z_t, img.copy(), bound_hw[0], bound_hw[1], len(ys), len(xs))


@pytest.mark.parametrize("block", range(6))
def test_warp_fuzz_vs_oracle(gpu, block, monkeypatch):
    """Random homographies (rotation, anisotropic scale 0.6-1.8, shear, perspective, translation), random source and
    output sizes (narrower and wider than one 128-pixel tile), random patch shape: fast kernels vs the oracle.  Blocks 4-5:
    larger sources whose grids overhang them on every side (border patches: clamped windows, masked taps) and bounds smaller
    than the source (wrapPerspectiveScan's `res`)."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(1000 + block)
    big = block >= 4
    for case in range(10 if not big else 6):
        sh, sw = (int(rng.integers(24, 260)), int(rng.integers(24, 420))) if not big else (int(rng.integers(300, 520)), int(rng.integers(400, 900)))
        img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        t = rng.uniform(-np.pi, np.pi) if case % 2 else rng.uniform(-0.1, 0.1)
        sx, sy = rng.uniform(0.6, 1.8, 2)
        A = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]) @ np.array([[sx, rng.uniform(-0.2, 0.2)], [0, sy]])
        H = np.eye(3)
        H[:2, :2] = A
        H[:2, 2] = rng.uniform(-40, 40, 2) + np.array([sw / 2, sh / 2]) - A @ np.array([sw / 2, sh / 2])
        H[2, :2] = rng.uniform(-4e-4, 4e-4, 2)
        inv = np.linalg.inv(H)
        ow, oh = (int(rng.integers(8, 520)), int(rng.integers(5, 300))) if not big else (int(rng.integers(500, 1100)), int(rng.integers(300, 620)))
        x0, y0 = rng.uniform(-30, 30, 2) if not big else rng.uniform(-90, -20, 2)
        stepx, stepy = rng.uniform(0.7, 1.3, 2)
        xs, ys = x0 + stepx * np.arange(ow), y0 + stepy * np.arange(oh)
        grid = kernels.Grid(xs[0], xs[-1], ow, ys[0], ys[-1], oh)
        xs, ys = np.linspace(xs[0], xs[-1], ow), np.linspace(ys[0], ys[-1], oh)
        shape = [None, "5", "6", "7"][int(rng.integers(0, 4))]
        _force_shape(shape)
        bound = (sh, sw) if not (big and case % 2) else (int(rng.integers(sh // 2, sh)), int(rng.integers(sw // 2, sw)))
        ref = _oracle_warp_on_grid(img, inv, xs, ys, bound)
        src = torch.from_numpy(img).to(gpu)
        got = kernels.warp_backward(src, inv, grid, bound, "bilinear", torch.float32).cpu().numpy()
        ok = close(got, ref)
        assert (~ok).sum() <= 3, (block, case, shape, (sh, sw), (oh, ow), int((~ok).sum()), float(np.abs(got - ref).max()))
        u8 = kernels.warp_backward(src, inv, grid, bound, "bilinear", torch.uint8).cpu().numpy()
        d = np.abs(u8.astype(np.int16) - ref.astype(np.uint8).astype(np.int16))
        assert (d > 1).sum() <= 9 and (d != 0).mean() < 0.02, (block, case, shape, int((d > 1).sum()), float((d != 0).mean()))
        # nearest neighbour: every pixel equal (index work is bit-exact)
        nn_ref = _oracle_nn_on_grid(img, inv, xs, ys, bound)
        nn = kernels.warp_backward(src, inv, grid, bound, "nn", torch.uint8).cpu().numpy()
        assert np.array_equal(nn, nn_ref), (block, case, shape, int((nn != nn_ref).any(axis=2).sum()))


@pytest.mark.parametrize("shape", [None, "5", "6", "7"])
def test_warp_rgba_u8_staged_vs_oracle(gpu, shape, monkeypatch):
    """uint8 RGBA images (4-byte texels: staged without the RGB -> RGBX expansion, `warp_rgba8_fast8`): bilinear uint8 output
    against the oracle on mild, rotated, bordered and ragged geometries, per patch shape; the alpha channel is a channel
    like the others (homography.py:123-138 with chn == 4)."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(404)
    _force_shape(shape)
    for case in range(6):
        sh, sw = int(rng.integers(150, 420)), int(rng.integers(200, 640))
        img = rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8)
        t = [0.01, -0.04, 0.6, 2.4, 0.02, -0.01][case]
        A = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]) * rng.uniform(0.9, 1.15)
        H = np.eye(3); H[:2, :2] = A
        H[:2, 2] = rng.uniform(-30, 30, 2) + np.array([sw / 2, sh / 2]) - A @ np.array([sw / 2, sh / 2])
        H[2, :2] = rng.uniform(-1e-4, 1e-4, 2)
        inv = np.linalg.inv(H)
        ow, oh = int(rng.integers(128, 700)), int(rng.integers(40, 400))
        x0, y0 = rng.uniform(-40, 10, 2)
        xs, ys = x0 + np.arange(ow) * 1.0, y0 + np.arange(oh) * 1.0
        grid = kernels.Grid(xs[0], xs[-1], ow, ys[0], ys[-1], oh)
        xs, ys = np.linspace(xs[0], xs[-1], ow), np.linspace(ys[0], ys[-1], oh)
        bound = (sh, sw) if case % 2 == 0 else (sh - 7, sw - 11)
        src = torch.from_numpy(img).to(gpu)
        assert kernels.warp_plan((sh, sw, 4), torch.uint8, inv, grid, bound, "bilinear", torch.uint8).startswith("rwh::warp_rgba8_fast8<")
        ref = _oracle_warp_on_grid(img, inv, xs, ys, bound)
        u8 = kernels.warp_backward(src, inv, grid, bound, "bilinear", torch.uint8).cpu().numpy()
        assert u8.shape == (oh, ow, 4)
        d = np.abs(u8.astype(np.int16) - ref.astype(np.uint8).astype(np.int16))
        assert (d > 1).sum() <= 9 and (d != 0).mean() < 0.02, (case, shape, int((d > 1).sum()), float((d != 0).mean()))
        # batch of two and a row shard agree with the single launch bit for bit
        both = kernels.warp_backward(torch.stack([src, src]), inv, grid, bound, "bilinear", torch.uint8)
        assert torch.equal(both[0].cpu(), torch.from_numpy(u8)) and torch.equal(both[1].cpu(), torch.from_numpy(u8))
        r0, r1 = oh // 3, oh - 5
        part = kernels.warp_backward(src, inv, grid, bound, "bilinear", torch.uint8, rows=(r0, r1))
        assert np.array_equal(part.cpu().numpy(), u8[r0:r1])
    # a grid that overhangs the source by 150 px on every side: whole patches outside it (the kernel's whole-run store is an
    # assembly dwordx4 -- a missing wait state after it once left the first two pixels of such runs to the next instruction:
    # found by tools/soak_warp.py CH=4) -- against the exact float64 kernel
    rng = np.random.default_rng(405)
    for t in (0.02, -0.9, 2.03):
        img = torch.from_numpy(rng.integers(0, 256, (500, 700, 4), dtype=np.uint8)).to(gpu)
        A = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
        H = np.eye(3); H[:2, :2] = A; H[:2, 2] = np.array([350.0, 250.0]) - A @ np.array([350.0, 250.0]); H[2, :2] = (3e-5, -2e-5)
        inv = np.linalg.inv(H)
        grid = kernels.Grid(-150.0, 849.0, 1000, -150.0, 649.0, 800)
        ex = kernels.warp_backward(img, inv, grid, (500, 700), "bilinear", torch.float64, exact=True)
        u8 = kernels.warp_backward(img, inv, grid, (500, 700), "bilinear", torch.uint8)
        d = (u8.to(torch.int16) - ex.to(torch.uint8).to(torch.int16)).abs()
        assert int((d > 1).sum()) == 0 and float((d != 0).float().mean()) < 0.02, (shape, t, int((d > 1).sum()))


@pytest.mark.parametrize("chn", [3, 4])
def test_warp_fast_kernels_vs_exact_kernel_random_geometries(gpu, chn, monkeypatch):
    """A short run of tools/soak_warp.py inside the suite: the fast kernels (staged RGB / RGBA bilinear uint8 and float32,
    nearest neighbour) against the exact float64 kernel -- itself pinned bit for bit to the reference by the goldens -- on
    random source sizes up to 1400 x 2000, rotations, zooms 0.5-2.2, horizons inside the grid, overhanging grids, scan-mode
    bounds and every patch shape.  (The soak found what the targeted tests had missed: a missing wait state after an
    assembly store that garbled two pixels of some runs.)"""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(9000 + chn)
    for case in range(14):
        sh, sw = int(rng.integers(40, 1400)), int(rng.integers(40, 2000))
        img = torch.from_numpy(rng.integers(0, 256, (sh, sw, chn), dtype=np.uint8)).to(gpu)
        t = rng.uniform(-np.pi, np.pi) if case % 3 == 0 else rng.uniform(-0.08, 0.08)
        sx, sy = rng.uniform(0.5, 2.2, 2) if case % 5 == 0 else rng.uniform(0.85, 1.2, 2)
        A = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]) @ np.array([[sx, rng.uniform(-0.15, 0.15)], [0, sy]])
        H = np.eye(3); H[:2, :2] = A
        H[:2, 2] = rng.uniform(-60, 60, 2) + np.array([sw / 2, sh / 2]) - A @ np.array([sw / 2, sh / 2])
        H[2, :2] = rng.uniform(-2e-4, 2e-4, 2) if case % 7 else rng.uniform(-2e-3, 2e-3, 2)
        inv = np.linalg.inv(H)
        ow, oh = int(rng.integers(8, 2300)), int(rng.integers(5, 1500))
        x0, y0 = rng.uniform(-120, 60, 2)
        stepx, stepy = rng.uniform(0.8, 1.25, 2)
        grid = kernels.Grid(x0, x0 + stepx * (ow - 1), ow, y0, y0 + stepy * (oh - 1), oh)
        bound = (sh, sw) if case % 4 else (int(rng.integers(sh // 2, sh + 1)), int(rng.integers(sw // 2, sw + 1)))
        _force_shape([None, None, "5", "6", "7"][int(rng.integers(0, 5))])
        ex = kernels.warp_backward(img, inv, grid, bound, "bilinear", torch.float64, zero_origin=False, exact=True)
        f32 = kernels.warp_backward(img, inv, grid, bound, "bilinear", torch.float32, zero_origin=False)
        u8 = kernels.warp_backward(img, inv, grid, bound, "bilinear", torch.uint8, zero_origin=False)
        rel = (f32.double() - ex).abs() / ex.abs().clamp(min=1.0)
        d = (u8.to(torch.int16) - ex.to(torch.uint8).to(torch.int16)).abs()
        assert int((rel > 1e-4).sum()) <= 6 and int((d > 1).sum()) <= 6, (chn, case, int((rel > 1e-4).sum()), int((d > 1).sum()))
        nn_e = kernels.warp_backward(img, inv, grid, bound, "nn", torch.uint8, zero_origin=False, exact=True)
        nn_f = kernels.warp_backward(img, inv, grid, bound, "nn", torch.uint8, zero_origin=False)
        assert torch.equal(nn_e, nn_f), (chn, case)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("case", ["mild", "integer_ties", "rot12", "rot45", "persp", "zoom_out", "horizon"])
def test_nearest_fast_kernel_bit_exact(gpu, case, exact, monkeypatch):
    """The LDS-staged nearest-neighbour kernel (outputs >= 128 px wide, RGB u8) against the oracle, every pixel equal:
    half-integer ties (an integer translation puts EVERY coordinate on x.5 after the +0.5), rotations that change the
    patch shape, perspective, waves that gather (zoom-out), a horizon inside the output, ragged tiles, all shapes."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(77)
    img = rng.integers(0, 256, (301, 433, 3), dtype=np.uint8)

    def rot(deg, sc=1.0):
        t = np.deg2rad(deg)
        c, s, cx, cy = sc * np.cos(t), sc * np.sin(t), 216.0, 150.0
        return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0, 0, 1.0]])
    H = {"mild": np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]]),
         "integer_ties": np.array([[1.0, 0, 7.5], [0, 1.0, -3.5], [0, 0, 1.0]]),   # coordinates k + 0.5: trunc(s + 0.5) ties
         "rot12": rot(12, 1.05), "rot45": rot(45, 0.9),
         "persp": np.array([[0.9, 0.2, 11.0], [-0.15, 1.1, 30.0], [3e-4, -2e-4, 1.0]]),
         "zoom_out": np.array([[0.4, 0, 20.0], [0, 0.45, 10.0], [0, 0, 1.0]]),
         "horizon": np.linalg.inv(np.array([[1.0, 0.02, 3.0], [0.01, 1.0, 2.0], [-3.1e-3, -2.3e-3, 1.0]]))}[case]
    inv = np.linalg.inv(H)
    xs, ys = np.linspace(-9, 470, 480), np.linspace(-5, 325, 331)
    grid = kernels.Grid(-9, 470, 480, -5, 325, 331)
    ref = _oracle_nn_on_grid(img, inv, xs, ys, (301, 433))
    src = torch.from_numpy(img).to(gpu)
    for shape in ("5", "6", "7", None):
        _force_shape(shape)
        got = kernels.warp_backward(src, inv, grid, (301, 433), "nn", torch.uint8, exact=exact).cpu().numpy()
        bad = int((got != ref).any(axis=2).sum())
        assert bad == 0, (case, shape, exact, bad)
    part = kernels.warp_backward(src, inv, grid, (301, 433), "nn", torch.uint8, rows=(37, 200), exact=exact).cpu().numpy()
    assert np.array_equal(part, ref[37:200])


# ------------------------------------------------------------------------------------------------
# Exact mode (RWH_WARP_EXACT): bit-identical float64 / uint8 results
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def exact_mode():
    import ransac_with_homography_amd.homography as impl
    old = impl.EXACT
    impl.EXACT = True
    yield impl
    impl.EXACT = old


@pytest.fixture
def auto_mode():
    import ransac_with_homography_amd.homography as impl
    old = impl.EXACT
    impl.EXACT = None
    yield impl
    impl.EXACT = old


def test_default_mode_numpy_exact_tensor_fast(gpu, auto_mode):
    """Default policy: numpy in -> bit-identical to the reference; torch tensor in -> fast kernels (float32 out)."""
    import homography as hg
    z = load_golden("g6_small_warps")
    img, H = z["img_noise"], z["H_bench"]
    o, _, _ = hg.wrapPerspective(img.copy(), H, convert="bilinear")
    assert np.array_equal(o, z["wp_noise_bench_bilinear"])
    t, _, _ = hg.wrapPerspective(torch.from_numpy(img.copy()).to(gpu), H, convert="bilinear")
    assert t.is_cuda and t.dtype == torch.float32 and close(t.cpu().numpy(), z["wp_noise_bench_bilinear"]).all()


def _sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_exact_mode_small_goldens_bit_identical(gpu, exact_mode):
    """Every G6 output of the reference -- float64 bilinear, uint8 transformImageH, scan mode, boundary=1, RGBA
    float32 -- reproduced bit for bit (np.array_equal on float64)."""
    import homography as hg
    z = load_golden("g6_small_warps")
    for iname in ("noise", "ramp"):
        img = z["img_" + iname]
        for hn in [str(h) for h in z["H_names"]]:
            H = z["H_" + hn]
            o, mx, my = hg.wrapPerspective(img.copy(), H, convert="bilinear")
            k = "wp_%s_%s_bilinear" % (iname, hn)
            assert o.dtype == np.float64 and np.array_equal(o, z[k]), k
            o, _, _ = hg.wrapPerspective(img.copy(), H, convert="nn")
            assert np.array_equal(o, z["wp_%s_%s_nn" % (iname, hn)])
            o, _, _ = hg.transformImageH(img.copy(), H)
            assert o.dtype == np.uint8 and np.array_equal(o, z["tih_%s_%s" % (iname, hn)])
        o, _, _ = hg.wrapPerspective(img.copy(), z["H_rot"], convert="bilinear", boundary=1)
        assert np.array_equal(o, z["wpb_%s_rot_bilinear" % iname])
        hs, ws, _ = img.shape
        for hn in ("bench", "rot"):
            o, _, _ = hg.wrapPerspectiveScan(img.copy(), z["H_" + hn], (hs - 8, ws - 16), convert="bilinear")
            assert np.array_equal(o, z["scan_%s_%s_bilinear" % (iname, hn)])
        rgba = z["rgba_" + iname]
        o, _, _ = hg.wrapPerspective(rgba.copy(), z["H_notebook"], convert="bilinear")
        assert o.dtype == np.float64 and np.array_equal(o, z["wp4_%s_notebook_bilinear" % iname])


def test_exact_mode_photo_goldens_sha256(gpu, exact_mode):
    """G7 / G8: the SHA-256 of the full float64 warp of notebook.jpg (1607 x 1251 x 3), of the uint8 scanner / crop
    outputs and of the stitched canvases equals the reference's."""
    import homography as hg
    z = load_golden("g7_notebook")
    img = load_golden("img_notebook")["img"]
    o, mx, my = hg.wrapPerspective(img.copy(), z["H"], convert="bilinear")
    assert _sha(o) == str(z["wp_bilinear_sha256"])
    assert _sha(hg.transformImage(img.copy(), z["u"], z["v"])) == str(z["ti_sha256"])
    assert _sha(hg.transformImage(img.copy(), z["u"], z["v_a4"], box=[1188, 840])) == str(z["scan_a4_sha256"])
    z = load_golden("g8_stitch")
    f = load_golden("img_foto1")
    o, _, _ = hg.transformImageH(f["A"].copy(), z["H_notebook"])
    assert _sha(o) == str(z["tih_sha256"])
    assert _sha(hg.stitchPanorama(f["B"].copy(), f["A"].copy(), z["H_notebook"])) == str(z["stitch_paste_sha256"])
    assert _sha(hg.stitchPanorama(f["B"].copy(), f["A"].copy(), z["H_notebook"], blending="Rate", blendrate=0.2)) == str(z["stitch_rate_sha256"])
    assert _sha(hg.stitchPanorama(f["B"].copy(), f["A"].copy(), z["H_g5"], blending="Rate", blendrate=0.2)) == str(z["stitch_g5_rate_sha256"])
    # 'Gradient' (homography.py:259-266): the alpha ramp is synthesised per tap in the fused kernel, for numpy and tensor callers
    zg = load_golden("g11_stitch_gradient")
    assert _sha(hg.stitchPanorama(f["B"].copy(), f["A"].copy(), z["H_notebook"], blending="Gradient")) == str(zg["stitch_gradient_sha256"])
    assert _sha(hg.stitchPanorama(f["B"].copy(), f["A"].copy(), z["H_g5"], blending="Gradient")) == str(zg["stitch_g5_gradient_sha256"])
    At, Bt = torch.from_numpy(f["A"]).to(gpu), torch.from_numpy(f["B"]).to(gpu)
    assert _sha(hg.stitchPanorama(Bt, At, z["H_g5"], blending="Gradient").cpu().numpy()) == str(zg["stitch_g5_gradient_sha256"])
    assert int(At[0, 0].sum()) == int(f["A"][0, 0].sum())     # addAlpha copies: the caller's texel (0,0) survives


def test_entry_points_are_graph_capturable(gpu):
    """The C entry points enqueue on the caller's stream and neither allocate nor synchronise: a hipGraph captured
    around them (torch.cuda.CUDAGraph) replays to the eager result."""
    from ransac_with_homography_amd import kernels
    g = torch.Generator(device="cpu").manual_seed(3)
    src = torch.randint(0, 256, (2, 240, 320, 3), dtype=torch.uint8, generator=g).to(gpu)
    inv = np.linalg.inv(H_BENCH)
    grid = kernels.Grid(0, 319, 320, 0, 239, 240)
    eager = kernels.warp_backward(src, inv, grid, (240, 320), "bilinear", torch.uint8)
    out = torch.zeros_like(eager)
    z = load_golden("matchespoints")
    pa, pb = torch.from_numpy(z["ptsA"]).to(gpu), torch.from_numpy(z["ptsB"]).to(gpu)
    np.random.seed(0)
    idx = torch.from_numpy(np.random.randint(0, 185, (2000, 4)).astype(np.int32)).to(gpu)
    ws = kernels.SearchWorkspace(2000, 185, gpu)
    kernels.ransac_search(pa, pb, idx, 5.0, "fwd", 134, ws)
    ref_best = ws.best.clone(); ref_counts = ws.counts.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):       # warm-up on the side stream, as graph capture requires
        kernels.warp_backward(src, inv, grid, (240, 320), "bilinear", torch.uint8, out=out)
        kernels.ransac_search(pa, pb, idx, 5.0, "fwd", 134, ws)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        kernels.warp_backward(src, inv, grid, (240, 320), "bilinear", torch.uint8, out=out)
        kernels.ransac_search(pa, pb, idx, 5.0, "fwd", 134, ws)
    out.zero_(); ws.best.zero_(); ws.counts.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(ws.best, ref_best) and torch.equal(ws.counts, ref_counts)


def test_ransac_run_illcond_samples_vs_reference(gpu):
    """g12 (written by the unmodified reference): lattice / cluster problems whose samples are ill-conditioned WITHOUT a
    repeated index -- three collinear source points, equal coordinates at different indices.  K1's elimination returns a
    finite H there that has nothing to do with LAPACK's (inlier counts apart by up to ~500), so K1 flags them
    (RWH_HYP_ILLCOND) and RANSAC.run settles them with the reference's solver: winner, count, inlier list and the position of
    numpy's generator equal the reference's on every case (early exits, a running best over 1 500 hypotheses, ties at the
    top).  Per hypothesis: the K1 count of every UNFLAGGED sample is within the rescore margin of the reference's."""
    import ransac as rs
    from ransac_with_homography_amd import _lib
    from ransac_with_homography_amd import ransac as rmod
    z = load_golden("g12_illcond")
    for key in [str(c) for c in z["cases"]]:
        tag, s, th, d, k, m = key.split("_")
        A, B = z["ptsA_" + tag], z["ptsB_" + tag]
        np.random.seed(int(s[1:]))
        model = rs.HomoModel(th=int(th[2:]), d=int(d[1:]), n=4)
        r = rs.RANSAC(model, k=int(k[1:]))
        with np.errstate(all="ignore"):
            H, inl, cnt = r.run([A.T, B.T], method=m)
        nxt = np.random.randint(0, 1 << 30)
        assert int(cnt) == int(z[key + "_count"]) and r.last_run["winner"] == int(z[key + "_winner"]), (key, int(cnt), r.last_run["winner"])
        assert r.last_run["early_exit"] == bool(z[key + "_early"])
        assert np.array_equal(inl[0], z[key + "_inliers"]), key
        np.testing.assert_allclose(H, z[key + "_H"], rtol=2e-2, atol=2e-2)      # float32 normal equations on 600-2400 inliers
        np.random.seed(int(s[1:]))
        np.random.randint(0, A.shape[0], (r.last_run["winner"] + 1 if r.last_run["early_exit"] else int(k[1:]), 4))
        assert np.random.randint(0, 1 << 30) == nxt, key                         # the generator is where the reference leaves it
        flags = r.last_run["flags"].cpu().numpy()
        raw = r.last_run["raw_counts"]
        ref = z[key + "_hyp_counts"].astype(np.int64)
        end = r.last_run["winner"] + 1 if r.last_run["early_exit"] else len(ref)
        unfl = flags[:end] == 0
        dif = np.abs(raw[:end].astype(np.int64) - ref[:end])
        assert dif[unfl].max() <= rmod.RESCORE_MARGIN, (key, int(dif[unfl].max()))
        ill = (flags[:end] & _lib.RWH_HYP_ILLCOND) != 0
        print(key, "flagged ill-conditioned: %d of %d, largest |K1 count - reference| among them %d, among unflagged %d; host-settled %d in %d rounds"
              % (int(ill.sum()), end, int(dif[ill].max()) if ill.any() else 0, int(dif[unfl].max()), r.last_run["host_settled"], r.last_run["host_rounds"]))
        assert r.last_run["host_rounds"] <= 3


def test_score_interval_kernel_and_dense_cloud_share(gpu):
    """K2i (rwh_score_interval, round 4): (1) the kernel against its numpy emulation (tests/interval_emulation.py) -- lo / hi
    equal up to pairs exactly on the boundary, budgets by flag; (2) CONTAINMENT, the property the 'fwd' settle rule stands on, against the
    reference's solver: for every sample that is not repeated / non-finite / degenerate, the count of LAPACK's H (svd_hypotheses
    + K2) lies inside [lo, hi] of K1's H -- on dense clouds (Gaussian around (500, 500), sigma 3-40 px, 30 % outliers: the
    verdict's recipe), two clusters, a lattice and matchespoints; (3) RANSAC.run on those problems equals the oracle's loop and
    hands LESS THAN 10 % of the hypotheses to the host beyond the repeated-index samples (rounds 2-3: 27-90 % on dense clouds)."""
    import interval_emulation as ive
    import ransac as rs
    from oracle import rwh_oracle as orc
    from ransac_with_homography_amd import _lib, kernels
    from ransac_with_homography_amd import ransac as rmod
    rng = np.random.default_rng(17)
    HS = np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]])

    def problem(kind, M, sigma):
        if kind == "cloud": G = rng.normal(500, sigma, (M, 2))
        elif kind == "two": G = np.array([[400., 450.], [620., 560.]])[rng.integers(0, 2, M)] + rng.normal(0, sigma, (M, 2))
        else: G = np.stack([rng.integers(0, 12, M) * 37.0, rng.integers(0, 9, M) * 53.0], 1)
        P = np.c_[G, np.ones(M)] @ HS.T
        B = P[:, :2] / P[:, 2:3] + rng.normal(0, 1.0, (M, 2))
        out = rng.random(M) < 0.3
        B[out] = rng.uniform(B.min(), B.max(), (int(out.sum()), 2))
        return G.astype(np.float32), B.astype(np.float32)
    always_bits = _lib.RWH_HYP_REPEATED | _lib.RWH_HYP_SINGULAR | _lib.RWH_HYP_DEGENERATE
    for kind, M, sigma in (("cloud", 1400, 3), ("cloud", 2000, 10), ("cloud", 2900, 40), ("two", 2000, 5), ("lattice", 600, 0)):
        A, B = problem(kind, M, sigma)
        K = 6000
        idx = rng.integers(0, M, (K, 4)).astype(np.int32)
        pa, pb = torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu)
        ws = kernels.SearchWorkspace(K, M, gpu)
        kernels.ransac_search(pa, pb, torch.from_numpy(idx).to(gpu), 5.0, "fwd", 1 << 30, ws)
        flags = ws.flags.cpu().numpy()
        rows = np.flatnonzero((flags & always_bits) == 0)
        C = max(1.0, float(np.abs(A).max()))
        lo, hi = kernels.score_interval(ws.H, rows, ws.flags, pa, pb, 5.0, C, rmod.IV_DELTA0, rmod.IV_DELTA1)
        Hk = ws.H.cpu().numpy()
        pick = rows[:: max(1, len(rows) // 300)]
        elo, ehi = ive.score_interval(Hk, pick, flags, A, B, 5.0, C, rmod.IV_DELTA0, rmod.IV_DELTA1)
        sel = np.searchsorted(rows, pick)
        # (a pair exactly on e + margin == th may fall either way: the emulation's fmaf is a float64 sum rounded once)
        assert np.abs(lo[sel] - elo).max() <= 1 and np.abs(hi[sel] - ehi).max() <= 1 and (lo[sel] == elo).mean() > 0.97, (kind, sigma)
        kc = ws.counts.cpu().numpy()[rows]
        assert ((lo <= kc) & (kc <= hi)).all()                                   # K2's own count is inside its interval
        Hl = rmod.svd_hypotheses(A, B, idx[rows])
        cl, _, _ = kernels.score_count(torch.from_numpy(Hl).to(gpu), pa, pb, 5.0, "fwd", 1 << 30, kernels.new_best(gpu), want_masks=False)
        cl = cl.cpu().numpy()
        fin = np.isfinite(Hl).all(axis=1)
        bad = fin & ((cl < lo) | (cl > hi))
        assert not bad.any(), (kind, sigma, int(bad.sum()), int(np.abs(cl - kc)[bad].max()))
        # RANSAC.run against the oracle's sequential loop, and what it costs the host
        for seed in (1, 2):
            np.random.seed(seed)
            with np.errstate(all="ignore"):
                Ho, inlo, cnto, ito = orc.ransac_run(A.T, B.T, th=5, d=95, n=4, k=400, method="fwd")
            nxt_o = np.random.randint(0, 1 << 30)
            np.random.seed(seed)
            r = rs.RANSAC(rs.HomoModel(th=5, d=95, n=4), k=400)
            with np.errstate(all="ignore"):
                Hg, inlg, cntg = r.run([A.T, B.T], method="fwd")
            assert int(cntg) == int(cnto) and r.last_run["winner"] == ito and np.array_equal(inlg[0], inlo[0]) and np.random.randint(0, 1 << 30) == nxt_o
        np.random.seed(5)
        r = rs.RANSAC(rs.HomoModel(th=5, d=95, n=4), k=10000)
        with np.errstate(all="ignore"):
            r.run([A.T, B.T], method="fwd")
        if not r.last_run["early_exit"]:
            rep = int(rmod.repeated_rows(r.last_run["idx"]).sum())
            share = (r.last_run["host_settled"] - rep) / 10000.0
            print("%s M %d sigma %g: flagged by K1 %d, host-solved beyond the %d repeated-index samples: %d of 10000 (%.2f %%), intervals for %d"
                  % (kind, M, sigma, r.last_run["flagged"], rep, r.last_run["host_settled"] - rep, 100 * share, r.last_run["intervals"]))
            assert share < 0.10, (kind, sigma, share)


def test_ransac_run_n6_vs_reference(gpu, matches):
    """HomoModel(n = 6): six indices per iteration from numpy's stream, the model fitted on the first four, early exit at
    d + 6 (ransac.py:177-190, homography.py:4-14); n < 4 fails like the reference's u[3,0] does.  g13 (reference run)."""
    import ransac as rs
    ptsA, ptsB = matches
    g = load_golden("g13_config4_x8")
    for seed, d in ((0, 70), (3, 50)):
        key = "n6_s%d_d%d" % (seed, d)
        np.random.seed(seed)
        H, inl, cnt = rs.RANSAC(rs.HomoModel(th=5, d=d, n=6), k=1000).run([ptsA.T, ptsB.T], method="fwd")
        assert int(cnt) == int(g[key + "_count"]) and np.array_equal(inl[0], g[key + "_inliers"])
        np.testing.assert_allclose(H, g[key + "_H"], rtol=1e-3, atol=1e-3)
        assert np.random.randint(0, 1 << 30) == int(g[key + "_next_draw"])
    with pytest.raises(IndexError):
        rs.RANSAC(rs.HomoModel(th=5, d=70, n=3), k=10).run([ptsA.T, ptsB.T], method="fwd")
    np.random.seed(5)
    idx = [np.random.randint(0, 185, (300, 6)) for _ in range(2)]
    res = rs.run_batch([[ptsA.T, ptsB.T]] * 2, th=5, d=70, n=6, k=300, method="fwd", idx=idx)
    for p in range(2):
        from oracle import rwh_oracle as orc
        Hs, counts = orc.ransac_table(ptsA.T, ptsB.T, idx[p][:, :4], th=5, method="fwd")
        assert int(res[p][2]) == int(counts.max())


def test_host_transfer_pipeline_round_trip(gpu):
    """_xfer: the chunked, page-locked, multi-threaded upload / download used by the numpy-facing API moves every byte
    (sizes around the chunk boundaries, uint8 and float32, back-to-back calls re-using the staging ring)."""
    from ransac_with_homography_amd import _xfer
    rng = np.random.default_rng(3)
    for shape, dt in (((1000, 1371, 3), np.uint8), ((2 * _xfer.CHUNK + 5,), np.uint8), ((7 * _xfer.CHUNK,), np.uint8),
                      ((701, 1203, 4), np.float32), ((13 * _xfer.CHUNK // 4 + 3,), np.float32), ((100, 100, 3), np.uint8)):
        a = rng.integers(0, 255, shape).astype(dt)
        t = _xfer.to_device(a, gpu)
        assert tuple(t.shape) == shape and torch.equal(t.cpu(), torch.from_numpy(a))
        b = _xfer.to_host(t + 1 if dt == np.float32 else t)
        assert b.dtype == dt and b.shape == shape and np.array_equal(b, a + 1 if dt == np.float32 else a)
        c = _xfer._to_host_staged(t.contiguous()) if a.nbytes >= _xfer.MIN_BYTES else b      # the pageable fallback of to_host
        assert c.dtype == dt and c.shape == shape and (c is b or np.array_equal(c, a)) and b.flags.writeable
    # a kernel's result read back right after the launch: the download waits for the producer stream
    src = torch.randint(0, 256, (2160, 3840, 3), dtype=torch.uint8, device=gpu)
    for _ in range(3):
        out = src.flip(0).contiguous()
        assert np.array_equal(_xfer.to_host(out), src.cpu().numpy()[::-1])


def test_ransac_run_random_problem_families_vs_oracle(gpu):
    """A short version of tests/soak_settle.py inside the suite: RANSAC.run against the oracle's sequential loop (same numpy
    seed) on random lattice / cluster / contaminated / tiny / large-coordinate problems with random th, d, k, n and loss:
    winner iteration, count, inlier list, the generator's position -- or the same failure (a winner with fewer inliers than
    the refit accepts, ransac.py:38)."""
    import contextlib
    import io
    import ransac as rs
    from oracle import rwh_oracle as orc
    rng = np.random.default_rng(2025)
    Hs = np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]])

    def project(G, noise):
        P = np.concatenate([G, np.ones((len(G), 1))], 1) @ Hs.T
        return P[:, :2] / P[:, 2:3] + rng.normal(0, noise, (len(G), 2))

    for case in range(40):
        kind = case % 4
        if kind == 0:
            M = int(rng.integers(30, 500)); G = np.stack([rng.integers(0, 12, M) * 37.0, rng.integers(0, 7, M) * 53.0], 1)
        elif kind == 1:
            M = int(rng.integers(30, 300)); c = rng.uniform(0, 2000, (5, 2)); G = c[rng.integers(0, 5, M)] + rng.normal(0, 0.01, (M, 2))
        elif kind == 2:
            M = int(rng.integers(5, 13)); G = rng.uniform(0, 500, (M, 2))
        else:
            M = int(rng.integers(50, 800)); G = rng.uniform(0, 1e4, (M, 2))
        B = project(G, 0.7)
        out = rng.random(M) < rng.choice([0.0, 0.3, 0.7])
        B[out] = rng.uniform(0, float(np.abs(B).max()) + 1.0, (int(out.sum()), 2))
        A, B = G.astype(np.float32), B.astype(np.float32)
        th = float(rng.choice([1, 3, 5])); d = int(rng.choice([20, 50, 95])); k = int(rng.integers(40, 200)); n = int(rng.choice([4, 4, 6]))
        m = str(rng.choice(["fwd", "backward", "reproj"])); seed = int(rng.integers(0, 1 << 30))
        res = []
        for runner in ("oracle", "gpu"):
            np.random.seed(seed)
            with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                try:
                    if runner == "oracle":
                        H, inl, cnt, it = orc.ransac_run(A.T, B.T, th=th, d=d, n=n, k=k, method=m)
                    else:
                        r = rs.RANSAC(rs.HomoModel(th=th, d=d, n=n), k=k)
                        H, inl, cnt = r.run([A.T, B.T], method=m)
                        it = r.last_run["winner"]
                    res.append((int(cnt), it, inl[0].tolist(), int(np.random.randint(0, 1 << 30))))
                except (AssertionError, ValueError, TypeError, np.linalg.LinAlgError) as e:
                    res.append(type(e).__name__)
        if isinstance(res[0], str) or isinstance(res[1], str):
            assert isinstance(res[0], str) and isinstance(res[1], str), (case, res)
        else:
            assert res[0] == res[1], (case, kind, M, th, d, k, n, m, seed, res[0][:2], res[1][:2])


def test_warp_entry_points_edge_cases_vs_reference(gpu, auto_mode):
    """g15 (written by the unmodified reference): the warp entry points at the corners of their input space, numpy arrays in (the
    reference's own callers) -- the same array bit for bit, dtype and origin, or the same exception TYPE: bilinear on a coordinate
    exactly ON the last column / row (identity, integer shifts, pure scales, rot90, mirrors) indexes one past the image in the
    reference (IndexError: `rwh_warp_index_check` finds those), a scan `res` beyond the image, a singular H (LinAlgError), a NaN
    entry (ValueError), 2 x 2 and 3 x 3 images, transformImage with and without a box."""
    import homography as hg
    from test_oracle_golden import _g15_call
    g = load_golden("g15_warp_edge_cases")
    fns = {"wrapPerspective": hg.wrapPerspective, "wrapPerspectiveScan": hg.wrapPerspectiveScan,
           "transformImage": hg.transformImage, "transformImageH": hg.transformImageH}
    for name in [str(n) for n in g["names"]]:
        want = str(g[name + "_outcome"])
        try:
            with np.errstate(all="ignore"):
                r = _g15_call(fns, g, name)
            got = "ok"
        except Exception as e:      # noqa: BLE001 -- the type is what is compared
            got = type(e).__name__
        assert got == want, (name, got, want)
        if want == "ok":
            arr = r[0] if isinstance(r, tuple) else r
            assert arr.dtype == g[name + "_out"].dtype and np.array_equal(arr, g[name + "_out"]), name
            if isinstance(r, tuple):
                assert [int(r[1]), int(r[2])] == g[name + "_origin"].tolist(), name


def test_stitch_geometry_and_blending_vs_reference(gpu, auto_mode):
    """g16 (written by the unmodified reference): stitchPanorama on small images for every branch of its canvas geometry, every
    `blending` value its code distinguishes (False, 'Rate', 'Gradient', another truthy value -- an all-zero alpha plane) and the
    identity homography (IndexError from the bilinear warp of imgT): numpy arrays in, the same canvas bit for bit or the same
    exception type."""
    import contextlib
    import io
    import homography as hg
    from test_oracle_golden import _g16_cases
    g = load_golden("g16_stitch_geometry")
    for name, Q, T, H, blending, want in _g16_cases(g):
        try:
            with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                r = hg.stitchPanorama(Q, T, H, blending=blending, blendrate=0.35)
            got = "ok"
        except Exception as e:      # noqa: BLE001 -- the type is what is compared
            got = type(e).__name__
        assert got == want, (name, got, want)
        if want == "ok":
            assert r.dtype == g[name + "_out"].dtype and np.array_equal(r, g[name + "_out"]), (name, r.shape, g[name + "_out"].shape)


def test_model_helpers_edge_cases_vs_reference(gpu):
    """g17 (written by the unmodified reference): HomoModel.fwd / reproj / dist / computeLoss / fit at the corners of their input
    space -- float32 and float64 `val`, a zero bottom row, a singular and a NaN `val`; 2- and 3-row inputs whose third row is kept,
    float64 and integer inputs, no point, one point, wrong row counts (AssertionError); every `method` and an unknown one
    (SystemExit); fits on 2- / 3-row samples, collective refits, wrong sizes, a repeated point: the same array -- values bit for
    bit AND dtype -- or the same exception type."""
    import contextlib
    import io
    import ransac as rs
    from test_oracle_golden import _g17_cases, _same_array
    g = load_golden("g17_model_helpers")
    wrong = []
    for name, op, val, args, want in _g17_cases(g):
        m = rs.HomoModel(th=5, d=50, n=4)
        if val is not None:
            m.val = val
        try:
            with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                r = getattr(m, op)(*args)
            got = "ok"
        except BaseException as e:      # noqa: BLE001 -- SystemExit included
            got = type(e).__name__
        if got != want:
            wrong.append((name, got, want))
        elif want == "ok" and not _same_array(r, g[name + "_out"]):
            ra = np.asarray(r)
            wrong.append((name, str(ra.dtype), str(g[name + "_out"].dtype), ra.shape,
                          int((ra != g[name + "_out"]).sum()) if ra.shape == g[name + "_out"].shape else -1))
    assert not wrong, wrong


def test_host_helpers_and_interpolators_vs_reference(gpu, auto_mode):
    """g18 (written by the unmodified reference): the module's builders / solvers, addAlpha and the two interpolators on
    caller-computed coordinates at the corners of their input space -- float32 / float64 / integer points, huge coordinates,
    equal and collinear points (LinAlgError), too few points (IndexError), a NaN point; every addAlpha method, direction
    (TOP: UnboundLocalError) and channel count; coordinates inside, outside, exactly on the last column / row (bilinear:
    IndexError), on .5, NaN (bilinear: IndexError) and Inf, bounds smaller and larger than the image (IndexError): the same
    arrays bit for bit and in dtype, the same side effects on the arguments, or the same exception type."""
    import contextlib
    import io
    import homography as hg
    from test_oracle_golden import _g18_cases, _g18_check
    g = load_golden("g18_host_helpers")
    wrong = []
    for name, fn, args, kw, want, outs, after in _g18_cases(g):
        try:
            with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                r = getattr(hg, fn)(*args, **kw)
            got = "ok"
        except Exception as e:      # noqa: BLE001 -- the type is what is compared
            got = type(e).__name__
        if got != want:
            wrong.append((name, got, want))
        elif want == "ok":
            _g18_check(name, r, args, outs, after, wrong)
    assert not wrong, wrong


def test_ransac_run_near_singular_inverse_vs_reference(gpu):
    """g19 (written by the unmodified reference): cluster problems under 'backward' / 'reproj'.  A sample drawn from two or three
    tight clusters gives a nearly singular H; the reference inverts every hypothesis with numpy.linalg.inv (ransac.py:74) and the
    loss then depends on how THAT routine rounds -- the kernels' own float64 elimination rounds apart from it there (case 0:
    same winner and count, another inlier list; found by tests/soak_settle.py).  The settle step scores its hypotheses with
    numpy's own inverses (rwh_host_inv3 / rwh_score_count_inv): winner, count, inlier list, refit and generator position of
    every run, through the native driver and through its Python twin."""
    import contextlib
    import io
    import ransac as rs
    from ransac_with_homography_amd import ransac as rmod
    from test_oracle_golden import _g19_cases
    g = load_golden("g19_near_singular_inverse")
    for force in (False, True):
        rmod.FORCE_PYTHON_DRIVER = force
        try:
            for key, A, B, th, d, k, n, seed, m in _g19_cases(g):
                np.random.seed(seed)
                with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                    r = rs.RANSAC(rs.HomoModel(th=th, d=d, n=n), k=k)
                    H, inl, cnt = r.run([A.T, B.T], method=m)
                assert int(cnt) == int(g[key + "_count"]) and np.array_equal(inl[0], g[key + "_inliers"]), (key, force, int(cnt), int(g[key + "_count"]))
                assert int(np.random.randint(0, 1 << 30)) == int(g[key + "_next_draw"]), (key, force)
                assert np.allclose(H, g[key + "_H"], rtol=1e-3, atol=1e-6), (key, force)
        finally:
            rmod.FORCE_PYTHON_DRIVER = False
    # the batched form with the caller's index tables settles the same way
    for key, A, B, th, d, k, n, seed, m in list(_g19_cases(g))[:6]:
        np.random.seed(seed)
        table = np.random.randint(0, len(A), (k, n))
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
            (Hb, inlb, cntb), = rmod.run_batch([[A.T, B.T]], th=th, d=d, n=n, k=k, method=m, idx=[table])
        assert int(cntb) == int(g[key + "_count"]) and np.array_equal(inlb[0], g[key + "_inliers"]), (key, "run_batch")
    # the single-call helpers take numpy's inverse too: a nearly singular val, bit for bit against the reference's expressions
    key, A, B, th, d, k, n, seed, m = next(_g19_cases(g))
    rng = np.random.default_rng(5)
    for t in range(40):
        idx = rng.integers(0, len(A), 4)
        with np.errstate(all="ignore"):
            val = np.asarray(rs.HomoModel().fit(A[idx].T, B[idx].T))
            if not np.isfinite(val).all():
                continue
            mod = rs.HomoModel(); mod.val = val
            x = np.ones((3, len(A)), np.float32); x[:2] = B.T
            want = np.linalg.inv(val) @ x
            want = want / (want[-1, :] + 1e-10)
            assert np.array_equal(mod.reproj(B.T), want, equal_nan=True), t
            e = mod.computeLoss(A.T, B.T, "backward")
            dlt = want[:2] - A.T
            assert np.array_equal(e, np.sqrt(np.sum(dlt * dlt, axis=0)), equal_nan=True), t


def test_stitch_pipelined_equals_plain(gpu, auto_mode):
    """stitchPanorama from host arrays: the pipelined form (uploads interleaved in the order the row tiles need them, tiles
    composed by rwh_stitch_panorama_rows as their rows arrive, finished tiles sent down between the upload chunks) returns
    the plain form's canvas bit for bit -- every canvas-geometry branch, every blending mode, a strong perspective whose tiles
    need rows of imgT far from their own, the horizon inside the canvas -- and leaves the caller's arrays the same way."""
    import contextlib
    import io
    import homography as hg
    impl = auto_mode
    rng = np.random.default_rng(21)
    Q = rng.integers(1, 256, (700, 900, 3), dtype=np.uint8)
    T = rng.integers(1, 256, (640, 1000, 3), dtype=np.uint8)
    P = np.array([[1.0, 0.02, 0], [0.015, 0.98, 0], [1e-5, 2e-5, 1.0]])

    def shift(tx, ty, M=P):
        S = np.eye(3); S[0, 2] = tx; S[1, 2] = ty
        return S @ M
    strong = np.array([[0.8, 0.3, 0], [-0.25, 0.9, 0], [4e-4, -2e-4, 1.0]])
    Hm = [shift(-300.3, -200.6), shift(-250.2, 310.4), shift(420.5, -150.3), shift(380.7, 290.2), shift(40.4, 30.3), shift(1500.2, 40.1),
          shift(30.3, -900.7), shift(200.1, 100.2, strong), shift(-100.1, 50.2, strong)]
    old, old_f = impl.PIPELINE_MIN_BYTES, impl.PIPELINE_WARP_FACTOR
    impl.PIPELINE_WARP_FACTOR = 1.0
    try:
        for hi, H in enumerate(Hm):
            for blending in (False, "Rate", "Gradient"):
                outs, afters = [], []
                for pipe in (None, 1 << 16):
                    impl.PIPELINE_MIN_BYTES = pipe
                    t_in, q_in = T.copy(), Q.copy()
                    with contextlib.redirect_stdout(io.StringIO()):
                        outs.append(hg.stitchPanorama(q_in, t_in, H, blending=blending, blendrate=0.3))
                    afters.append((t_in, q_in))
                assert outs[0].shape == outs[1].shape and np.array_equal(outs[0], outs[1]), (hi, blending)
                assert np.array_equal(afters[0][0], afters[1][0]) and np.array_equal(afters[0][1], afters[1][1]), (hi, blending)
        # the single warps take the same pipeline (output-row tiles of rwh_warp_backward): every entry point, both interpolators,
        # uint8 RGB and float32 RGBA images, the exact and the fast kernels, a strong perspective, a horizon inside the grid
        T4 = rng.uniform(0, 255, (640, 1000, 4)).astype(np.float32)
        horizon = np.linalg.inv(np.array([[1.0, 0.02, 3.0], [0.01, 1.0, 2.0], [-3.1e-3, -2.3e-3, 1.0]]))
        for exact_mode in (None, False):
            impl.EXACT = exact_mode
            for hi, H in enumerate([shift(40.4, 30.3), shift(-300.3, 200.6, strong), np.array([[0.6, 0.05, 10.0], [0.02, 0.7, 5.0], [1e-5, 0, 1.0]]), horizon]):
                for conv in ("nn", "bilinear"):
                    for img in (T, T4):
                        for fn, args in ((hg.wrapPerspective, (H,)), (hg.wrapPerspectiveScan, (H, (500, 700))), (hg.transformImageH, (H,))):
                            kw = {"method": conv} if fn is hg.transformImageH else {"convert": conv}
                            outs, afters = [], []
                            for pipe in (None, 1 << 16):
                                impl.PIPELINE_MIN_BYTES = pipe
                                a_in = img.copy()
                                try:
                                    with np.errstate(all="ignore"):
                                        r = fn(a_in, *args, **kw)
                                    outs.append(r)
                                except Exception as e:      # noqa: BLE001
                                    outs.append(type(e).__name__)
                                afters.append(a_in)
                            if isinstance(outs[0], str) or isinstance(outs[1], str):
                                assert outs[0] == outs[1], (exact_mode, hi, conv, img.dtype, fn.__name__, outs)
                            else:
                                assert outs[0][0].dtype == outs[1][0].dtype and np.array_equal(outs[0][0], outs[1][0], equal_nan=True) and \
                                    outs[0][1:] == outs[1][1:], (exact_mode, hi, conv, img.dtype, fn.__name__)
                            assert np.array_equal(afters[0], afters[1]), (exact_mode, hi, conv, fn.__name__)
    finally:
        impl.PIPELINE_MIN_BYTES, impl.PIPELINE_WARP_FACTOR = old, old_f
        impl.EXACT = None


def test_ransac_run_edge_cases_vs_reference(gpu):
    """g14 (written by the unmodified reference): the corners of RANSAC.run's input space -- one to four correspondences, none,
    k = 0 / 1, thresholds of 0, below 0 and huge, d of 0 and beyond the number of points, n < 4 and n > M, all points equal,
    collinear points, NaN / Inf coordinates, observation counts that differ.  Same count, inlier list, refit and generator
    position, or the same exception TYPE raised with the generator where the reference leaves it."""
    import contextlib
    import io
    import ransac as rs
    g = load_golden("g14_edge_cases")
    same_numpy = str(g["numpy_version"]).split(".")[:2] == np.__version__.split(".")[:2]
    for name in [str(n) for n in g["names"]]:
        A, B = g[name + "_A"], g[name + "_B"]
        th, d, n, k = g[name + "_par"]
        for m in ("fwd", "reproj"):
            key = "%s_%s" % (name, m)
            want = str(g[key + "_outcome"])
            if want == "ValueError" and not same_numpy and A.shape[0] > 0:
                continue                      # np.where(None): an empty index up to numpy 2.0, an error from 2.1 on
            np.random.seed(4242)
            with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                try:
                    r = rs.RANSAC(rs.HomoModel(th=th, d=d, n=int(n)), k=int(k))
                    H, inl, cnt = r.run([A.T, B.T], method=m)
                    got = "ok"
                except Exception as e:      # noqa: BLE001 -- the type is what is compared
                    got = type(e).__name__
            assert got == want, (key, got, want)
            assert int(np.random.randint(0, 1 << 30)) == int(g[key + "_next_draw"]), key
            if want == "ok":
                assert int(cnt) == int(g[key + "_count"]) and np.array_equal(inl[0], g[key + "_inliers"]), key
                assert np.allclose(H, g[key + "_H"], rtol=1e-3, atol=1e-6, equal_nan=True), key


@pytest.mark.parametrize("block", range(3))
def test_warp_exact_kernels_vs_oracle_next_to_the_horizon(gpu, block):
    """The exact kernels are what tools/soak_horizon.py trusts: here they are held against the oracle itself, bit for bit, on
    its kind of map -- a denominator that reaches ~0 within 1e-5 .. 0.5 px of a patch-lattice corner (coordinates up to 1e9,
    both signs of W in the grid), scaled homographies, an infinite entry."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(500 + block)
    compared = 0
    for case in range(10):
        sh, sw = int(rng.integers(40, 200)), int(rng.integers(40, 300))
        img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        img[0, 0] = 0                                        # (the reference blanks texel (0,0) before it samples)
        ow, oh = int(rng.integers(128, 330)), int(rng.integers(16, 120))
        pw = int(rng.choice([32, 64, 128])); ph = 512 // pw
        cc = float(rng.integers(0, ow // pw + 1) * pw - rng.integers(0, 2)); rr = float(rng.integers(0, oh // ph + 1) * ph - rng.integers(0, 2))
        delta = 10.0 ** rng.uniform(-5, -0.3) * rng.choice([-1, 1])
        t = rng.uniform(0, 2 * np.pi)
        nrm = np.array([np.cos(t), np.sin(t)])
        g = 10.0 ** rng.uniform(-4, 0)
        p0 = np.array([cc, rr]) + delta * nrm
        w_row = np.array([g * nrm[0], g * nrm[1], -g * (nrm @ p0)]) * rng.choice([-1, 1])
        A = rng.uniform(-1.5, 1.5, (2, 3)); A[:, 2] = rng.uniform(-50, 50, 2) + np.array([sw / 2, sh / 2]) * abs(w_row[2])
        if case % 3 == 0: A[1] = w_row * rng.uniform(0, sh - 1)
        if case % 3 == 1: A[0] = w_row * rng.uniform(0, sw - 1)
        ih = np.vstack([A, w_row])
        if case % 5 == 4: ih = ih * 10.0 ** rng.uniform(-280, 280)
        if case == 7: ih[2, int(rng.integers(0, 3))] = np.inf
        xs, ys = np.arange(ow, dtype=np.float64), np.arange(oh, dtype=np.float64)
        grid = kernels.Grid(0, ow - 1, ow, 0, oh - 1, oh)
        src = torch.from_numpy(img).to(gpu)
        try:
            with np.errstate(all="ignore"):
                ref = _oracle_warp_on_grid(img, ih, xs, ys, (sh, sw))
                ref_nn = _oracle_nn_on_grid(img, ih, xs, ys, (sh, sw))
        except IndexError:          # a NaN coordinate (0 / 0, Inf / Inf) escapes the reference's mask and indexes with INT_MIN:
            continue                # the reference raises where the kernels return 0 (rwh.h)
        compared += 1
        ex = kernels.warp_backward(src, ih, grid, (sh, sw), "bilinear", torch.float64, zero_origin=False, exact=True).cpu().numpy()
        assert np.array_equal(ex, ref), (block, case, int((ex != ref).any(axis=2).sum()))
        nn = kernels.warp_backward(src, ih, grid, (sh, sw), "nn", torch.uint8, zero_origin=False, exact=True).cpu().numpy()
        assert np.array_equal(nn, ref_nn), (block, case, int((nn != ref_nn).any(axis=2).sum()))
        nn_fast = kernels.warp_backward(src, ih, grid, (sh, sw), "nn", torch.uint8, zero_origin=False).cpu().numpy()
        assert np.array_equal(nn_fast, ref_nn), (block, case)
    assert compared >= 6, compared


def test_warp_output_beyond_4GB(gpu):
    """A single image whose output passes 2^32 bytes (36 000 x 40 000 RGB u8 = 4.32 GB; MI355X has 288 GB): the staged kernels
    address their output with 32-bit lane offsets and hand such a launch to the generic kernel (64-bit offsets); row shards of
    the same warp are small enough for the staged kernel again.  Shards from the top, the 2^32-byte line and the bottom agree
    with the whole launch within 1 LSB, and a float32 sample of the same rows agrees with the exact kernel."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(8)
    sh, sw, oh, ow = 300, 400, 36000, 40000
    src = torch.from_numpy(rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)).to(gpu)
    # (every coordinate strictly inside the source: no mask-edge band, where fast and exact kernels may differ -- rwh.h)
    inv = np.array([[sw / ow * 0.98, 1e-4, 1.5], [2e-5, sh / oh * 0.97, 2.25], [1e-8, 2e-8, 1.0]])
    grid = kernels.Grid(0, ow - 1, ow, 0, oh - 1, oh)
    assert kernels.warp_plan((sh, sw, 3), torch.uint8, inv, grid, (sh, sw), "bilinear", torch.uint8).startswith("rwh::warp_generic")
    assert kernels.warp_plan((sh, sw, 3), torch.uint8, inv, grid, (sh, sw), "bilinear", torch.uint8, rows=(0, 512)).startswith("rwh::warp_rgb8_fast8")
    whole = kernels.warp_backward(src, inv, grid, (sh, sw), "bilinear", torch.uint8, zero_origin=False)
    assert whole.shape == (oh, ow, 3) and whole.numel() > (1 << 32)
    line = (1 << 32) // (3 * ow)          # the row that holds byte 2^32
    for r0, r1 in ((0, 256), (line - 128, line + 128), (oh - 300, oh)):
        part = kernels.warp_backward(src, inv, grid, (sh, sw), "bilinear", torch.uint8, zero_origin=False, rows=(r0, r1))
        d = (whole[r0:r1].to(torch.int16) - part.to(torch.int16)).abs()
        assert int(d.max()) <= 1 and float((d != 0).float().mean()) < 0.02, (r0, r1, int(d.max()))
        ex = kernels.warp_backward(src, inv, grid, (sh, sw), "bilinear", torch.float64, zero_origin=False, exact=True, rows=(r0, r0 + 16))
        d2 = (whole[r0:r0 + 16].to(torch.int16) - ex.to(torch.uint8).to(torch.int16)).abs()
        assert int(d2.max()) <= 1, (r0, int(d2.max()))
    assert int(torch.count_nonzero(whole[oh - 4:])) > 0            # the last rows were written
    del whole
    nn = kernels.warp_backward(src, inv, grid, (sh, sw), "nn", torch.uint8, zero_origin=False)
    for r0, r1 in ((line - 64, line + 64), (oh - 100, oh)):
        part = kernels.warp_backward(src, inv, grid, (sh, sw), "nn", torch.uint8, zero_origin=False, rows=(r0, r1))
        assert torch.equal(nn[r0:r1], part), (r0, r1)


def test_ransac_run_from_several_threads(gpu, matches):
    """rwh_ransac_run is called with the GIL released: four Python threads running searches of the SAME size at once (a server
    handling requests) must each get the result of their own sequential run -- the page-locked host workspace is cached per
    thread, the library's host pool serialises the LAPACK batches."""
    import threading
    from ransac_with_homography_amd import _lapack, kernels
    from ransac_with_homography_amd import ransac as rmod
    ptsA, ptsB = matches
    addr = _lapack.dgesdd_address()
    if addr is None:
        pytest.skip("numpy's LAPACK symbol not found: RANSAC.run uses the Python driver")
    pa, pb = np.ascontiguousarray(ptsA, np.float32), np.ascontiguousarray(ptsB, np.float32)
    m, k = pa.shape[0], 1500
    need = kernels.need_count(m, 70, 4)
    tables = [np.ascontiguousarray(np.random.default_rng(s).integers(0, m, (k, 4)), dtype=np.int32) for s in range(4)]

    def one(t):
        ws = kernels.RunWorkspace(m, k, gpu)
        r = kernels.ransac_run(pa, pb, tables[t], 5.0, "fwd", need, rmod.RESCORE_MARGIN, ws, addr, 4)
        return r[:6] + (r[6].tolist(), ws.host_counts(settled=True).tolist())
    want = [one(t) for t in range(4)]
    for rep in range(5):
        got, errs = [None] * 4, []

        def work(t):
            try:
                for _ in range(6): got[t] = one(t)
            except Exception as e:      # noqa: BLE001 -- reported below
                errs.append(e)
        ths = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for th_ in ths: th_.start()
        for th_ in ths: th_.join()
        assert not errs, errs
        assert got == want, rep


def test_native_and_python_run_drivers_agree(gpu, matches):
    """rwh_ransac_run (the native driver RANSAC.run uses) against its Python twin (`RANSAC._run_python_driver`: the same upload /
    search / presettle / settle sequence step by step): identical winner, early flag, count, inlier list, settle statistics and
    generator position on reference fixtures of every kind -- ordinary runs, low-inlier runs won by a repeated-index sample,
    lattice / cluster problems, early exits, n = 6, k = 0."""
    import contextlib
    import io
    import ransac as rs
    from ransac_with_homography_amd import ransac as rmod
    ptsA, ptsB = matches
    g9, g12 = load_golden("g9_low_inlier"), load_golden("g12_illcond")
    cases = [(ptsA, ptsB, 0, 5, 70, 4, 1000, "fwd"), (ptsA, ptsB, 1, 5, 50, 4, 1000, "reproj"), (ptsA, ptsB, 3, 5, 50, 6, 1000, "fwd"),
             (ptsA, g9["ptsB_a"], 2, 5, 20, 4, 1000, "fwd"), (ptsA, g9["ptsB_b"], 2, 5, 70, 4, 1000, "backward"),
             (g12["ptsA_lat2024"], g12["ptsB_lat2024"], 41, 3, 95, 4, 1500, "fwd"), (g12["ptsA_clus1"], g12["ptsB_clus1"], 3, 1, 101, 4, 1000, "fwd"),
             (g12["ptsA_lat5"], g12["ptsB_lat5"], 3, 3, 70, 4, 1000, "reproj"), (ptsA, ptsB, 5, 5, 70, 4, 0, "fwd")]
    for A, B, seed, th, d, n, k, m in cases:
        res = []
        for force in (False, True):
            rmod.FORCE_PYTHON_DRIVER = force
            try:
                np.random.seed(seed)
                r = rs.RANSAC(rs.HomoModel(th=th, d=d, n=n), k=k)
                with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                    try:
                        H, inl, cnt = r.run([A.T, B.T], method=m)
                        res.append((r.last_run["winner"], r.last_run["early_exit"], int(cnt), inl[0].tolist(), r.last_run["host_settled"],
                                    r.last_run["host_rounds"], r.last_run["flagged"], r.last_run["raw_counts"].tolist(),
                                    r.last_run["flags"].cpu().numpy().tolist(), int(np.random.randint(0, 1 << 30)), np.asarray(H).tolist()))
                    except UnboundLocalError:
                        res.append("UnboundLocalError")     # k = 0: like the reference (ransac.py:203)
            finally:
                rmod.FORCE_PYTHON_DRIVER = False
        assert res[0] == res[1], (seed, th, d, n, k, m, res[0][:7] if not isinstance(res[0], str) else res[0], res[1][:7] if not isinstance(res[1], str) else res[1])


# ---- K2i soundness: [lo, hi] against the reference's float32 arithmetic at sampled points of the perturbation box --------------
from k1_cases import k2i_box as _k2i_box      # the box has one statement: tests/k1_cases.py


def _box_points(h, D, rng, n_interior=200):
    """float32 points of the box around h (float32 [9]): the 3^6 combinations of {-1, 0, +1} in the affine entries h0..h5, each with
    the two extreme points of the projective entries h6, h7, h8 (all low, all high), and n_interior random interior points; every
    point rounded to float32 and kept inside the box (one step back toward h where rounding left it)."""
    import itertools
    aff = np.array(list(itertools.product((-1.0, 0.0, 1.0), repeat=6)))
    S = np.concatenate([np.c_[np.repeat(aff, 2, axis=0), np.tile([[-1.0] * 3, [1.0] * 3], (len(aff), 1))],
                        rng.uniform(-1, 1, (n_interior, 9))])
    h32 = np.asarray(h, np.float32)
    P = (h32.astype(np.float64) + S * D).astype(np.float32)
    out = np.abs(P.astype(np.float64) - h32) > D
    P = np.where(out, np.nextafter(P, np.broadcast_to(h32, P.shape)), P)
    assert (np.abs(P.astype(np.float64) - h32) <= D).all()
    return P


def _inliers_over_box(h, D, X, Y, th, rng):
    """[n_points, M] bool: the reference's inlier test (oracle.compute_loss 'fwd' < th, float32 as the reference computes it) at
    every sampled point of the box."""
    from oracle import rwh_oracle as orc
    with np.errstate(all="ignore"):
        return np.stack([orc.compute_loss(p.reshape(3, 3), X, Y, "fwd") < th for p in _box_points(h, D, rng)])


def _k2i_edge_problems(rng, th):
    """Problems built round one H each, with adversarial pairs: targets placed at th +- 1e-5 .. 3e-4 px from the float64 projection of
    a source point (then rounded to float32), at the places the margin formula could be too tight.  -> [(name, A, B, H, adversarial
    pair indices)]."""
    eps = np.array([1e-5, 3e-5, 1e-4, 3e-4])
    eps = np.concatenate([-eps, eps])
    out = []
    for name in ("cancel_1e4", "cancel_1e5", "horizon", "below2"):
        if name.startswith("cancel"):       # h0 x + h1 y + h2 ~ 0 with terms of 1e4 / 1e5: cancellation in the numerators
            c0 = 5e4 if name == "cancel_1e4" else 5e5
            x0, y0 = c0 * 0.3, c0 * 0.2
            H = np.array([[1.0, 0.5, -(x0 + 0.5 * y0)], [0.3, 1.0, -(0.3 * x0 + y0)], [1e-8, 2e-8, 1.0]])
            A = np.c_[rng.uniform(x0 - c0 * 0.2, x0 + c0 * 0.2, 160), rng.uniform(y0 - c0 * 0.2, y0 + c0 * 0.2, 160)]
            src = np.c_[x0 + rng.uniform(-50, 50, 12), y0 + rng.uniform(-50, 50, 12)]
        elif name == "horizon":             # 1 + h6 x near 0: the denominator close to the horizon line x = 1052.6
            H = np.array([[1.0, 0.02, 3.0], [0.01, 1.0, -2.0], [-9.5e-4, 0.0, 1.0]])
            A = np.c_[rng.uniform(0, 1000, 160), rng.uniform(0, 1000, 160)]
            src = np.c_[rng.uniform(1040, 1051, 12), rng.uniform(0, 1000, 12)]
        else:                               # every coordinate below 2: coord_scale is clamped to 1
            H = np.array([[0.9, 0.05, 0.1], [-0.03, 1.1, 0.05], [0.02, -0.01, 1.0]])
            A = rng.uniform(0, 1.99, (160, 2))
            src = rng.uniform(0, 1.99, (12, 2))
        H32 = H.astype(np.float32).reshape(9)
        Hq = H32.astype(np.float64).reshape(3, 3)

        def proj(P):
            q = np.c_[P, np.ones(len(P))] @ Hq.T
            return q[:, :2] / q[:, 2:3]
        B = proj(A) + rng.normal(0, 0.6 * th, (len(A), 2))
        phi = rng.uniform(0, 2 * np.pi, (len(src), len(eps)))
        tgt = proj(src)[:, None, :] + (th + eps)[None, :, None] * np.stack([np.cos(phi), np.sin(phi)], -1)
        A = np.concatenate([A, np.repeat(src, len(eps), axis=0)]).astype(np.float32)
        B = np.concatenate([B, tgt.reshape(-1, 2)]).astype(np.float32)
        out.append((name, A, B, H32, np.arange(160, len(A))))
    return out


def test_score_interval_sound_over_the_box(gpu, matches):
    """K2i's claim as stated (include/rwh.h, rwh_score_interval): lo counts the pairs that are inliers for EVERY H within the
    perturbation box, hi those that are inliers for SOME.  Checked against the reference's own float32 arithmetic (the oracle's
    compute_loss) at sampled points of the box -- the 729 affine corners x 2 projective extremes and 200 interior points, in float32,
    inside the box -- for unflagged (delta0) and RWH_HYP_ILLCOND (delta1) rows.
      * count level, one launch per problem: lo <= count(H') <= hi on dense-cloud, two-cluster, lattice and matchespoints problems
        (K1's hypotheses nearest the top, the ill-conditioned ones, a few at random) and on the adversarial problems;
      * pair level, one launch with m = 1 per adversarial pair (the full problem's coord_scale): a pair counted in lo is an inlier
        at every sampled H', a pair excluded by hi an outlier at every one.  Adversarial pairs sit at th +- 1e-5 .. 3e-4 px where
        h0 x + h1 y + h2 cancels at coordinates of 1e4 / 1e5, next to the horizon, and with every coordinate below 2."""
    from ransac_with_homography_amd import _lib, kernels
    from ransac_with_homography_amd import ransac as rmod
    rng = np.random.default_rng(31)
    d0, d1, th = rmod.IV_DELTA0, rmod.IV_DELTA1, 5.0
    ILL = _lib.RWH_HYP_ILLCOND
    always_bits = _lib.RWH_HYP_REPEATED | _lib.RWH_HYP_SINGULAR | _lib.RWH_HYP_DEGENERATE
    HS = np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]])

    def real_problem(kind):
        if kind == "matches":
            return matches
        M = {"cloud": 1400, "two": 2000, "lattice": 600}[kind]
        if kind == "cloud": G = rng.normal(500, 3, (M, 2))
        elif kind == "two": G = np.array([[400., 450.], [620., 560.]])[rng.integers(0, 2, M)] + rng.normal(0, 5, (M, 2))
        else: G = np.stack([rng.integers(0, 12, M) * 37.0, rng.integers(0, 9, M) * 53.0], 1)
        P = np.c_[G, np.ones(M)] @ HS.T
        B = P[:, :2] / P[:, 2:3] + rng.normal(0, 1.0, (M, 2))
        o = rng.random(M) < 0.3
        B[o] = rng.uniform(B.min(), B.max(), (int(o.sum()), 2))
        return G.astype(np.float32), B.astype(np.float32)

    checked = {"count": 0, "pair_lo": 0, "pair_hi": 0, "ill": 0}
    for kind in ("cloud", "two", "lattice", "matches"):
        A, B = real_problem(kind)
        X, Y = A.T, B.T
        K = 2000
        idx = rng.integers(0, A.shape[0], (K, 4)).astype(np.int32)
        pa, pb = torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu)
        ws = kernels.SearchWorkspace(K, A.shape[0], gpu)
        kernels.ransac_search(pa, pb, torch.from_numpy(idx).to(gpu), th, "fwd", 1 << 30, ws)
        flags, counts, Hk = ws.flags.cpu().numpy(), ws.counts.cpu().numpy(), ws.H.cpu().numpy()
        free = np.flatnonzero((flags & always_bits) == 0)
        top = free[np.argsort(-counts[free], kind="stable")[:14]]
        ill = free[(flags[free] & ILL) != 0][:10]
        rows = np.unique(np.concatenate([top, ill, rng.choice(free, 4, replace=False)]))
        C = max(1.0, float(np.abs(A).max()))
        lo, hi = kernels.score_interval(ws.H, rows, ws.flags, pa, pb, th, C, d0, d1)
        for j, r in enumerate(rows):
            D = _k2i_box(Hk[r], flags[r] & ILL, C, d0, d1)
            c = _inliers_over_box(Hk[r], D, X, Y, th, rng).sum(axis=1)
            assert lo[j] <= c.min() and c.max() <= hi[j], (kind, int(r), int(flags[r]), int(lo[j]), int(hi[j]), int(c.min()), int(c.max()))
            checked["count"] += 1
            checked["ill"] += bool(flags[r] & ILL)

    for name, A, B, H32, adv in _k2i_edge_problems(rng, th):
        X, Y = A.T, B.T
        C = max(1.0, float(np.abs(A).max()))
        Hs = np.stack([H32, H32, np.nextafter(H32, np.float32(np.inf)), np.nextafter(H32, np.float32(-np.inf))])
        fl = np.array([0, ILL, 0, ILL], np.uint8)
        H_dev, fl_dev = torch.from_numpy(Hs).to(gpu), torch.from_numpy(fl).to(gpu)
        rows = np.arange(len(Hs))
        pa, pb = torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu)
        lo, hi = kernels.score_interval(H_dev, rows, fl_dev, pa, pb, th, C, d0, d1)
        box = [_inliers_over_box(Hs[r], _k2i_box(Hs[r], fl[r], C, d0, d1), X, Y, th, rng) for r in rows]
        for r in rows:
            c = box[r].sum(axis=1)
            assert lo[r] <= c.min() and c.max() <= hi[r], (name, int(r), int(lo[r]), int(hi[r]), int(c.min()), int(c.max()))
            checked["count"] += 1
        for p in adv:
            plo, phi = kernels.score_interval(H_dev, rows, fl_dev, pa[p:p + 1], pb[p:p + 1], th, C, d0, d1)
            for r in rows:
                if plo[r]:
                    assert box[r][:, p].all(), (name, int(r), int(p), "counted in lo, an outlier at some H' of the box")
                    checked["pair_lo"] += 1
                if not phi[r]:
                    assert not box[r][:, p].any(), (name, int(r), int(p), "excluded by hi, an inlier at some H' of the box")
                    checked["pair_hi"] += 1
    print("K2i soundness:", checked)
    assert checked["ill"] > 0 and checked["pair_lo"] > 0 and checked["pair_hi"] > 0, checked


def test_ransac_run_nan_coordinate_vs_oracle(gpu):
    """A NaN source coordinate: the settle step takes the margin rule under 'fwd' (the interval kernel's coordinate scale cannot be
    formed; both drivers test for the NaN explicitly).  RANSAC.run against the oracle's loop on a dense cloud with one NaN
    coordinate: the same winner, count, inlier list and generator position -- or, where a sample holding the NaN point comes before
    any early exit, the same LinAlgError."""
    import ransac as rs
    from oracle import rwh_oracle as orc
    from ransac_with_homography_amd import ransac as rmod
    rng = np.random.default_rng(43)
    HS = np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]])
    M = 1400
    G = rng.normal(500, 3, (M, 2))
    P = np.c_[G, np.ones(M)] @ HS.T
    B = P[:, :2] / P[:, 2:3] + rng.normal(0, 1.0, (M, 2))
    o = rng.random(M) < 0.3
    B[o] = rng.uniform(B.min(), B.max(), (int(o.sum()), 2))
    A, B = G.astype(np.float32), B.astype(np.float32)
    A[777, 0] = np.nan
    completed = 0
    for d, k in ((95, 300), (5000, 60)):
        for seed in (1, 2, 3):
            for force in (False, True):
                np.random.seed(seed)
                try:
                    with np.errstate(all="ignore"):
                        Ho, inlo, cnto, ito = orc.ransac_run(A.T, B.T, th=5, d=d, n=4, k=k, method="fwd")
                    ref = (int(cnto), int(ito), inlo[0].tolist())
                except np.linalg.LinAlgError:
                    ref = "LinAlgError"
                nxt_o = np.random.randint(0, 1 << 30)
                np.random.seed(seed)
                rmod.FORCE_PYTHON_DRIVER = force
                try:
                    r = rs.RANSAC(rs.HomoModel(th=5, d=d, n=4), k=k)
                    with np.errstate(all="ignore"):
                        Hg, inlg, cntg = r.run([A.T, B.T], method="fwd")
                    got = (int(cntg), int(r.last_run["winner"]), inlg[0].tolist())
                except np.linalg.LinAlgError:
                    got = "LinAlgError"
                finally:
                    rmod.FORCE_PYTHON_DRIVER = False
                assert got == ref and np.random.randint(0, 1 << 30) == nxt_o, (d, k, seed, force, str(got)[:80], str(ref)[:80])
                if ref != "LinAlgError":
                    completed += 1
                    assert r.last_run["intervals"] == 0, r.last_run      # the margin rule: no interval was asked for
    assert completed >= 4, completed
