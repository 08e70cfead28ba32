"""The cases of tests/golden/g21_warp_dtypes.npz (written by make_golden_g21.py from the reference's warp entry points) and the one
check every driver of them applies: same outcome, the same result (same_result), dtype, shape and origin, the same caller image (texel
(0,0) blanked as the reference blanks it, nothing else touched) and, for convertfunc, the same caller z_t after the call."""
import contextlib
import io

import numpy as np

from conftest import load_golden


def same_result(got, ref, bits):
    """Same dtype, shape and values: every element bit for bit (-0.0 included), or with bits=False (float results of arithmetic)
    NaN wherever the reference has NaN -- NaN's sign and payload are the arithmetic unit's (x86's default NaN is negative, the
    GPU's positive), not numpy's -- and every other element bit for bit."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    if bits or ref.dtype.kind != "f":
        return got.tobytes() == ref.tobytes()
    n_got, n_ref = np.isnan(got), np.isnan(ref)
    return bool(np.array_equal(n_got, n_ref)) and got[~n_got].tobytes() == ref[~n_ref].tobytes()


def g21_cases():
    z = load_golden("g21_warp_dtypes")
    flat, zflat = z["out_flat"], z["z_flat"]
    out = []
    for i, name in enumerate(z["names"]):
        img = z["img_" + str(z["img"][i])]
        after = img.copy()
        after[0, 0] = np.frombuffer(z["t00"][i][:img.itemsize * img.shape[2]].tobytes(), img.dtype)
        res = None
        if str(z["outcome"][i]) == "ok":
            dt = np.dtype(str(z["out_dtype"][i]))
            shape = tuple(int(v) for v in z["out_shape"][i])
            off = int(z["out_off"][i])
            res = np.frombuffer(flat[off:off + int(np.prod(shape)) * dt.itemsize].tobytes(), dt).reshape(shape)
        zk = str(z["zkey"][i])
        z_in = z["z_" + zk] if zk else None
        z_after = None
        if zk:
            zo = int(z["z_off"][i])
            z_after = zflat[zo:zo + z_in.size].reshape(z_in.shape)
        box = tuple(int(v) for v in z["box"][i])
        out.append(dict(name=str(name), fn=str(z["fn"][i]), img=img, H=z["H"][i], conv=str(z["conv"][i]), boundary=int(z["boundary"][i]),
                        res=tuple(int(v) for v in z["res"][i]), bound=tuple(int(v) for v in z["bound"][i]), u=z["u"][i], v=z["v"][i],
                        box=None if box[0] < 0 else box, z=z_in, outcome=str(z["outcome"][i]), result=res,
                        origin=tuple(int(v) for v in z["origin"][i]), img_after=after, z_after=z_after))
    return out


class RefAPI:
    """The reference's names over a module with its call surface (homography.py here, or the oracle's spelling)."""

    def __init__(self, wrap, scan, ti, tih, cf):
        self.wrap, self.scan, self.ti, self.tih, self.cf = wrap, scan, ti, tih, cf


def public_api():
    import homography as hg
    return RefAPI(lambda img, H, conv, b: hg.wrapPerspective(img, H, convert=conv, boundary=b),
                  lambda img, H, res, conv: hg.wrapPerspectiveScan(img, H, res, convert=conv),
                  lambda img, u, v, box, conv: hg.transformImage(img, u, v, box=box, method=conv),
                  lambda img, H, conv: hg.transformImageH(img, H, method=conv),
                  hg.convertfunc)


def oracle_api():
    from oracle import rwh_oracle as orc
    return RefAPI(lambda img, H, conv, b: orc.wrap_perspective(img, H, convert=conv, boundary=b),
                  lambda img, H, res, conv: orc.wrap_perspective_scan(img, H, res, convert=conv),
                  lambda img, u, v, box, conv: orc.transform_image(img, u, v, box=box, method=conv),
                  lambda img, H, conv: orc.transform_image_h(img, H, method=conv),
                  orc.INTERPOLATORS)


def call(api, case, img, z):
    fn, conv = case["fn"], case["conv"]
    if fn == "wp":
        return api.wrap(img, case["H"], conv, case["boundary"])
    if fn == "scan":
        return api.scan(img, case["H"], case["res"], conv)
    if fn == "tih":
        return api.tih(img, case["H"], conv)
    if fn == "ti":
        return api.ti(img, case["u"], case["v"], case["box"], conv), 0, 0
    mh, mw = case["res"]
    h, w = case["bound"]
    return api.cf[conv](z, img, h, w, mh, mw), 0, 0


def run_case(api, case):
    """The case through `api` on fresh copies of its image (and z_t) -> list of what differs from the reference."""
    img = case["img"].copy()
    z = None if case["z"] is None else case["z"].copy()
    try:
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
            r, mx, my = call(api, case, img, z)
        outcome = "ok"
    except Exception as e:      # noqa: BLE001 -- the type is compared with the reference's
        outcome, r, mx, my = type(e).__name__, None, 0, 0
    bad = []
    if outcome != case["outcome"]:
        bad.append("outcome %s, reference %s" % (outcome, case["outcome"]))
    elif r is not None:
        r = np.asarray(r)
        ref = case["result"]
        if r.dtype != ref.dtype or r.shape != ref.shape:
            bad.append("result %s %s, reference %s %s" % (r.dtype, r.shape, ref.dtype, ref.shape))
        elif not same_result(r, ref, bits=case["conv"] == "nn"):        # (nearest copies texels: NaN payloads included)
            bad.append("result differs in %d of %d bytes" % (int((np.ascontiguousarray(r).view(np.uint8) != ref.view(np.uint8)).sum()),
                                                             r.nbytes))
        if (int(mx), int(my)) != case["origin"]:
            bad.append("origin %s, reference %s" % ((mx, my), case["origin"]))
    if img.tobytes() != case["img_after"].tobytes():
        bad.append("caller's image after the call differs")
    if z is not None and z.tobytes() != case["z_after"].tobytes():
        bad.append("caller's z_t after the call differs")
    return bad
