"""The cases of tests/golden/g20_stitch_dtypes.npz (written by make_golden_g20.py from the reference's stitchPanorama) and the
one check every driver of them applies: same outcome, the same canvas bytes, the same caller arrays after the call."""
import contextlib
import io

import numpy as np

from conftest import load_golden

BLENDINGS = {"paste": False, "rate": "Rate", "grad": "Gradient", "true": True}


def g20_cases():
    z = load_golden("g20_stitch_dtypes")
    flat = z["out_flat"]
    out = []
    for i, name in enumerate(z["names"]):
        name = str(name)
        Q, T = z["img_" + str(z["q"][i])], z["img_" + str(z["t"][i])]
        t_after = T.copy()
        c = T.shape[2]
        t_after[0, 0] = np.frombuffer(z["t00"][i][:T.itemsize * c].tobytes(), T.dtype)
        shape = tuple(int(v) for v in z["out_shape"][i])
        off = int(z["out_off"][i])
        canvas = flat[off:off + int(np.prod(shape))].reshape(shape) if str(z["outcome"][i]) == "ok" else None
        out.append(dict(name=name, Q=Q, T=T, H=z["H"][i], blending=BLENDINGS[str(z["blending"][i])], rate=float(z["rate"][i]),
                        outcome=str(z["outcome"][i]), canvas=canvas, t_after=t_after))
    return out


def run_case(fn, case, to_input=lambda a: a.copy(), to_numpy=np.asarray):
    """fn(imgQ, imgT, H, blending, blendrate) on fresh copies of the case's images -> list of what differs from the reference."""
    q, t = to_input(case["Q"]), to_input(case["T"])
    try:
        with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
            r = fn(q, t, case["H"], case["blending"], case["rate"])
        outcome = "ok"
    except (IndexError, ValueError) as e:
        outcome, r = type(e).__name__, None
    bad = []
    if outcome != case["outcome"]:
        bad.append("outcome %s, reference %s" % (outcome, case["outcome"]))
    elif r is not None:
        r = to_numpy(r)
        if r.dtype != case["canvas"].dtype or r.shape != case["canvas"].shape:
            bad.append("canvas %s %s, reference %s %s" % (r.dtype, r.shape, case["canvas"].dtype, case["canvas"].shape))
        elif not np.array_equal(r, case["canvas"]):
            bad.append("canvas differs in %d of %d bytes" % (int((r != case["canvas"]).sum()), r.size))
    if to_numpy(t).tobytes() != case["t_after"].tobytes():
        bad.append("caller's imgT after the call differs")
    if to_numpy(q).tobytes() != case["Q"].tobytes():
        bad.append("caller's imgQ after the call differs")
    return bad
