"""MI355X-backed mirror of the reference's `ransac.py` call surface.

`HomoModel`, `RANSAC` and `stitching` keep the reference's names, constructor
arguments, defaults, return values and data layout (features x observations,
ransac.py:159-166).  The k-iteration Python loop of `RANSAC.run`
(ransac.py:176-202) is replaced by ONE library call, `rwh_ransac_search`, which enqueues

    K1  rwh_dlt4_batched   all k four-point DLT hypotheses        (ransac.py:178-180)
    K2  rwh_score_count    k x M reprojection errors, `err < th`,  (ransac.py:182-184)
                           wavefront ballot + popcount, and the
                           order-independent form of the accept
                           rules (packed argmax keys)             (ransac.py:186-202)

followed by the reference's own final N-point refit on the host
(ransac.py:206-211 -> calcHomographyLinear, O(1)).

Sampling parity: the k x 4 index table is drawn from numpy's global legacy
generator exactly as k successive `np.random.randint(0, M, 4)` calls would
(ransac.py:177), and the generator is left where the reference would leave it
(an early exit at iteration e consumes only e+1 draws).

Solver parity (ransac.py:177 draws WITH replacement; homography.py:81-87): a sample with a repeated
index gives a rank-deficient 8 x 9 system, for which the reference still takes whatever null vector
LAPACK's SVD returns and lets it compete for the running best; an ill-conditioned sample (three collinear
source points, equal coordinates at different indices) gives K1 and LAPACK unrelated H; and on ~2 % of
ordinary samples the two round to neighbouring float32 H.  K1 flags the first two kinds
(RWH_HYP_REPEATED / _SINGULAR / _ILLCOND), and the settle step re-derives, with the reference's own arithmetic
(float32 DLT matrix -> LAPACK dgesdd, the routine numpy.linalg.svd calls -> /h[8]: `svd_hypotheses`), every
hypothesis that can decide the run (the rule: csrc/rwh_settle.h), re-scores those rows with K2 (bit-exact given H)
and only then applies the accept rules.  The repeated-index samples are known before anything is launched: they are
solved on the host while the GPU searches; the whole driver is one native call (`rwh_ransac_run`).  k = 1500 at
M = 185: ~90 host solves, 0.36-0.42 ms per run end to end.

Error behaviour (fixture g14, written by the unmodified reference): k = 0 raises UnboundLocalError (ransac.py:203 reads a
variable only the loop assigns), a run in which no hypothesis has an inlier indexes with np.where(None) (an error from numpy
2.1 on), n < 4 raises IndexError after the first draw, a sample holding a NaN coordinate raises LinAlgError at ITS iteration
unless an earlier one took the early exit, a winner with fewer inliers than the refit accepts fails the refit's assertion --
each with numpy's generator left where the reference leaves it.

`run_batch` is the same search for MANY pairs in one submission; `stitching` and `stitch_sequence` are the pipelines around it.
The stage in front of the search -- the feature extractor and the Hamming matchers (`extract_batch`, `match_batch` with cross-check,
`match_graph` with the ratio test over a pair graph, their tables, the hand-off type `DeviceProblems`) -- lives in `features.py`; its public names are imported here: this module stays the call surface.

There is no CPU implementation of the loop here: without librwh_hip.so and a GPU
`RANSAC.run` raises `RwhUnavailable`.
"""
import ctypes
import os

import numpy as np

from . import _lapack, _lib, kernels
from .features import (DeviceProblems, _host_rows, default_pattern, detect_and_describe, extract_batch, match_batch,  # noqa: F401
                       match_descriptors, match_descriptors_ratio, match_graph, match_ratio, orb_bin_table, orb_layout,
                       orb_level_quotas, orb_scales, rotate_pattern)
from .homography import (_check_bands, _check_focal, _check_pairs, _check_projection, _check_wrap, _oriented, _pair_rows,  # noqa: F401
                         _sequence_inputs, calcHomography, calcHomographyLinear, cylindericlMap, sequence_adjust,
                         sequence_adjust_cameras, sequence_camera_maps, sequence_cameras, sequence_focal, sequence_gains,
                         sequence_block_gains, BlockGains, sequence_graph, sequence_period, sequence_plan, sequence_seams,
                         stitchPanorama, stitchSequence)

# Which hypotheses need the reference's own solver (`_settle_on_host`, natively `rwh_ransac_run`): the rule and its reasons are
# in csrc/rwh_settle.h.  RESCORE_MARGIN caps the margin of the 'backward' / 'reproj' rule: an unflagged K1 count moves by <= 2
# on all ~130 000 golden hypotheses and by <= 8 on the stress sets of tests/golden/g12_illcond.npz (tools/README).
RESCORE_MARGIN = 8


LVL = 0


def DEBUG(*args):
    if LVL >= 1:
        print("[DEBUG]", *args)


def _weak_threshold(th):
    """`err_total < self.th` (ransac.py:183) compares float32 errors with `th`:
    Python scalars are weak (compared as float32), numpy float64 scalars promote
    the comparison to float64.  Return the double the kernel must compare with."""
    if type(th) in (int, float, bool) or isinstance(th, (np.float32, np.float16, np.integer)):
        return float(np.float32(th))
    return float(th)


def _points_rows(P):
    """features x observations (2 x M or 3 x M) -> contiguous M x 2 float32.

    The search kernels take float32 correspondences -- what the reference's own pipeline hands to RANSAC.run (ransac.py:263-267:
    np.float32 keypoints; matchespoints.npy is float32).  On float64 or integer arrays the reference forms the DLT products in THAT
    dtype (homography.py:6-13) and -- even when every value is a float32 value -- the distances in float64 (ransac.py:78-82:
    float32 projection minus a float64 / integer target), so a borderline pair can fall the other way than in a float32 search.
    Round 3 cast such arrays with a warning; they are now refused: pass `X.astype(np.float32)` to get the float32 search."""
    P = np.asarray(P)
    if P.dtype != np.float32:
        raise TypeError("RANSAC: %s correspondences: the MI355X search computes in float32 like the reference's own pipeline "
                        "(ransac.py:263-267); on this input the reference forms its DLT products in %s and its distances in float64, "
                        "which this path does not reproduce -- pass float32 arrays (X.astype(np.float32))" % (P.dtype, P.dtype))
    return np.ascontiguousarray(P.T[:, :2])


def legacy_randint_table(m, k, n, want64=True):
    """np.random.randint(0, m, (k, n)) from numpy's GLOBAL legacy generator -- the stream ransac.py:177 consumes, one draw
    of n per iteration -- with the generator left exactly where that call leaves it.  -> (int64 [k, n] or None, int32 [k, n]).

    Native form (`rwh_host_legacy_randint`, host code of librwh_hip.so): MT19937 + numpy's masked rejection in a tight loop on
    the state `np.random.get_state()` hands out, written back with `set_state()`: 0.4 ms for 400 000 draws where numpy's own
    call takes 2.1 ms (39 % of a k = 100 000 run).  Identical output and generator position (tests/test_settle_cpu.py);
    any other bit generator, a missing library or an unexpected state layout take numpy's own call."""
    m, k, n = int(m), int(k), int(n)
    if k * n >= 4096 and 1 <= m < 2 ** 31 and os.path.exists(_lib.LIB_PATH):
        try:
            st = np.random.get_state()
            if st[0] == "MT19937" and len(st[1]) == 624 and 0 <= int(st[2]) <= 624:
                key = np.ascontiguousarray(st[1], dtype=np.uint32).copy()
                pos = ctypes.c_int32(int(st[2]))
                out32 = np.empty((k, n), dtype=np.int32)
                out64 = np.empty((k, n), dtype=np.int64) if want64 else None
                rc = _lib.load().rwh_host_legacy_randint(key.ctypes.data, ctypes.byref(pos), m, k * n, out32.ctypes.data,
                                                         out64.ctypes.data if want64 else None)
                if rc == 0:
                    np.random.set_state((st[0], key, int(pos.value), st[3], st[4]))
                    return out64, out32
        except (_lib.RwhUnavailable, OSError, ValueError, TypeError):
            pass
    t = np.random.randint(0, m, (k, n))
    return t, np.ascontiguousarray(t, dtype=np.int32)


def _host_thread_share():
    """Host threads of the settle step's LAPACK loop: this process's share of the cores it may run on -- one rank per GPU under
    torchrun (LOCAL_WORLD_SIZE), so 8 ranks on a 256-thread host take 32 each -- capped at 32 (k = 100 000 on matchespoints: 3 257
    repeated-index SVDs take 1.0 ms on 16 threads, 0.55 ms on 32, 0.44 ms on 64: tools/run_phases.py)."""
    try:
        cpus = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        cpus = os.cpu_count() or 1
    try:
        ranks = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))
    except ValueError:
        ranks = 1
    return max(1, min(32, cpus // ranks))


HOST_THREADS = _host_thread_share()
FORCE_PYTHON_DRIVER = False        # tests: RANSAC.run through `_run_python_driver`, the step-by-step form of rwh_ransac_run


def svd_hypotheses(pts_a, pts_b, idx_rows, threads=None):
    """The reference's 4-point solve (homography.py:4-14, 71-88) for n samples at once on the host:
    float32 DLT matrices -> LAPACK dgesdd (float64 inside, cast back to float32) -> last right-singular vector / its
    9th element.  -> float32 [n, 9].

    Native form: `rwh_host_dlt4_svd` runs the loop in librwh_hip.so's host code on `threads` cores, calling -- by address
    -- the very dgesdd numpy.linalg.svd calls (`_lapack.dgesdd_address`): the same numbers bit for bit
    (tests/test_settle_cpu.py), ~6 us per sample per core instead of ~11 us under the interpreter lock.  If that symbol
    cannot be found (another numpy build) or the library is missing, the stacked numpy call below does the same work."""
    idx_rows = np.ascontiguousarray(np.asarray(idx_rows).reshape(-1, 4), dtype=np.int32)
    n = idx_rows.shape[0]
    addr = _lapack.dgesdd_address()
    if addr is not None and n and os.path.exists(_lib.LIB_PATH):
        pa = np.ascontiguousarray(pts_a, dtype=np.float32)
        pb = np.ascontiguousarray(pts_b, dtype=np.float32)
        out = np.empty((n, 9), dtype=np.float32)
        st = _lib.load().rwh_host_dlt4_svd(pa.ctypes.data, pb.ctypes.data, pa.shape[0], idx_rows.ctypes.data, n,
                                           ctypes.c_void_p(addr), int(threads or HOST_THREADS), out.ctypes.data)
        if st == 0:
            return out
    flat = idx_rows.reshape(-1)
    mats = _pair_rows(pts_a[flat], pts_b[flat], -1).reshape(-1, 8, 9)
    with np.errstate(all="ignore"):          # h[8] == 0 divides like the reference does (inf / nan rows score 0)
        _, _, vt = np.linalg.svd(mats)
        h = vt[:, -1, :]
        return np.ascontiguousarray(h / h[:, 8:9])


def repeated_rows(idx):
    """Samples of a K x >=4 index table whose first four indices are not distinct (what K1 flags RWH_HYP_REPEATED):
    known to the host before anything is launched."""
    a, b, c, d = (np.asarray(idx)[:, i] for i in range(4))
    return (a == b) | (a == c) | (a == d) | (b == c) | (b == d) | (c == d)


class _Settled(object):
    """Hypotheses re-derived with the reference's solver so far: index -> (H row, count, where its mask lives)."""

    def __init__(self):
        self.batches = []          # (indices, H float32 [n, 9], mask tensor [n, words] on the device)
        self.where = {}

    def add(self, cand, H, masks):
        b = len(self.batches)
        self.batches.append((cand, H, masks))
        for j, i in enumerate(cand.tolist()):
            self.where[i] = (b, j)

    def mask_words(self, i):
        if i not in self.where:
            return None
        b, j = self.where[i]
        return self.batches[b][2][j].cpu().numpy()

    def rows(self):
        return {i: self.batches[b][1][j] for i, (b, j) in self.where.items()}


def _score_settled(H, pa_dev, pb_dev, th, method):
    """K2 on hypotheses the host solved (H: [n, 9] float32 host array) -> (counts, masks) device tensors.  'backward' and
    'reproj' project through numpy.linalg.inv(H) (ransac.py:74): these rows get numpy's own inverse, not the kernel's
    elimination, which rounds apart from LAPACK's on nearly singular H (rwh.h, rwh_score_count_inv)."""
    import torch
    dev = pa_dev.device
    hd = torch.from_numpy(H).to(dev)
    hinv = None if method == "fwd" else torch.from_numpy(kernels.host_inverses(H)).to(dev)
    cnt, msk, _ = kernels.score_count(hd, pa_dev, pb_dev, th, method, 1 << 30, kernels.scratch_best(dev), hinv=hinv)
    return cnt, msk


def presettle(pa_dev, pb_dev, pa, pb, idx_host, rows, th, method):
    """First part of the settle step, for samples the HOST can name before the GPU has said anything (repeated indices):
    their reference H by `svd_hypotheses` -- host time that overlaps the search already enqueued on the GPU -- then K2 on
    those rows, enqueued behind the search.  Returns (rows, H, counts tensor, masks tensor) for `_settle_on_host(pre=...)`."""
    import torch
    rows = np.asarray(rows, dtype=np.int64)
    if rows.size == 0:
        return None
    H = svd_hypotheses(pa, pb, idx_host[rows][:, :4])
    cnt, msk = _score_settled(H, pa_dev, pb_dev, th, method)
    return rows, H, cnt, msk


IV_DELTA0, IV_DELTA1 = 2.0 ** -20, 2.0 ** -18     # interval budgets (natural scale of an entry): unflagged / RWH_HYP_ILLCOND rows


def _settle_on_host(pa_dev, pb_dev, pa, pb, idx_host, counts, flags, need, th, method, margin, stats=None, pre=None, H_dev=None,
                    flags_dev=None):
    """Accept rules of ransac.py:186-202 over K1/K2's results, exact with respect to the reference's solver.

    counts / flags: host copies of K2's counts and K1's flags for the k hypotheses of `idx_host`; `pre`: what `presettle`
    returned (its counts are read here).  Which hypotheses are "settled" (H from the host SVD, count + mask from K2 on that H),
    in which rounds, and the accept rules are rwh_ransac_run's rule (csrc/rwh_settle.h), called through `rwh_settle_decide`:
    the interval rule for 'fwd' with K1's H at hand (`H_dev`), else the margin rule capped at `margin`.  This function does the
    work it asks for (`svd_hypotheses` + `_score_settled`, `kernels.score_interval`); an exception raised there propagates.
    Returns (winner | None, early, count, mask_words | None, H_rows, counts): mask_words is the winner's uint64 mask if the
    winner was settled here (None: take K2's own mask for it), H_rows maps settled index -> float32[9], counts is the int64
    count table with the settled entries replaced."""
    import torch
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    k = flags.shape[0]
    cnt, slot, st = np.array(counts, dtype=np.int32), np.full(k, -1, dtype=np.int32), _Settled()
    if pre is not None:
        rows, H, c, msk = pre
        cnt[rows], slot[rows] = c.cpu().numpy(), np.arange(len(rows))
        st.add(rows, H, msk)
    failed = []

    def callback(fn_type, body):        # an exception inside a ctypes callback would be printed and dropped: kept, raised below
        def call(rows, n, *args):
            try:
                body(np.ctypeslib.as_array(rows, (n,)).astype(np.int64), *args[:-1])
                return 0
            except BaseException as e:
                failed.append(e)
                return 1
        return fn_type(call)

    def solve(rows, cnt_p):
        H = svd_hypotheses(pa, pb, idx_host[rows][:, :4])
        c, msk = _score_settled(H, pa_dev, pb_dev, th, method)
        np.ctypeslib.as_array(cnt_p, (k,))[rows] = c.cpu().numpy()
        st.add(rows, H, msk)

    def interval(rows, coord_scale, lo_p, hi_p):
        f_dev = flags_dev if flags_dev is not None else torch.from_numpy(flags).to(H_dev.device)
        lo, hi = kernels.score_interval(H_dev, rows, f_dev, pa_dev, pb_dev, th, coord_scale, IV_DELTA0, IV_DELTA1)
        np.ctypeslib.as_array(lo_p, (k,))[rows], np.ctypeslib.as_array(hi_p, (k,))[rows] = lo, hi

    pa32 = np.ascontiguousarray(pa, dtype=np.float32)
    out = np.zeros(5, dtype=np.int32)
    fns = callback(_lib.SETTLE_INTERVAL_FN, interval), callback(_lib.SETTLE_SOLVE_FN, solve)     # alive until the call returns
    rc = _lib.load().rwh_settle_decide(k, flags.ctypes.data, cnt.ctypes.data, slot.ctypes.data, pa32.ctypes.data, pa32.size // 2,
                                       int(need), int(method == "fwd" and H_dev is not None), int(margin), *fns, None, out.ctypes.data)
    if failed:
        raise failed[0]
    _lib.check(rc, "rwh_settle_decide")
    w, early, count, rounds, n_iv = out.tolist()
    if stats is not None:
        stats.update(host_settled=int((slot >= 0).sum()), host_rounds=rounds, flagged=int((flags != 0).sum()), intervals=n_iv)
    if w < 0:
        return None, False, 0, None, st.rows(), cnt.astype(np.int64)
    return w, bool(early), count, st.mask_words(w), st.rows(), cnt.astype(np.int64)


class Model(object):
    __slots__ = ('val', 'th', 'd', 'n')

    def fit(self, X, Y):
        raise NotImplementedError

    def fwd(self, X):
        raise NotImplementedError

    def dist(self, predY, trueY):
        raise NotImplementedError


class HomoModel(Model):
    """ransac.py:22-98."""

    def __init__(self, th=5, d=50, n=4):
        self.th = th
        self.d = d
        self.n = n
        self.val = np.empty((3, 3), dtype=np.float32)

    def fit(self, X, Y, collective=False):
        """ransac.py:30-53.  X, Y: 2 x n or 3 x n (n == self.n, or more with collective=True)."""
        nx, mx = X.shape
        ny, my = Y.shape
        assert ((mx == my) and (mx == self.n)) or ((mx == my) and (mx > self.n) and collective), \
            "invalid data size should be %d" % self.n
        assert (nx == ny) and nx in [2, 3], "invalid input dimension for row numbers"
        if collective:
            self.val = calcHomographyLinear(X.T[:, :2], Y.T[:, :2], True)
        else:
            self.val = calcHomography(X.T[:, :2], Y.T[:, :2], False)
        return self.val

    # -- projection helpers: one launch of the projection kernel each -------------------------
    def _project(self, P, inverse):
        """ransac.py:55-76 with numpy's dtype rules: a 2-row input becomes a float32 3 x M with ones (ransac.py:59-60), a
        3-row input is used as it is (third row included); `val @ x` is float32 only if both operands are, float64
        otherwise; reproj goes through numpy.linalg.inv(val) in val's dtype (host, 3 x 3)."""
        import torch
        P = np.asarray(P)
        nrow, m = P.shape
        assert nrow in [2, 3], "invalid input dimension for row numbers"
        dev = _lib.require_gpu()
        val = np.asarray(self.val)
        if nrow == 2:
            x = np.ones((3, m), dtype=np.float32)
            x[:2, :] = P
        else:
            x = P
        if m < 2:
            # no point: numpy's empty product.  ONE point: numpy hands a 3 x 3 by 3 x 1 product to BLAS's matrix-VECTOR routine,
            # whose sums round differently from the matrix-matrix routine every other width takes (and the kernels reproduce):
            # the reference's own expression on the host (ransac.py:63-64 / 74-76), nine multiply-adds
            h = np.linalg.inv(val) if inverse else val
            y = h @ x
            return y / (y[-1, :] + 1e-10)
        if val.dtype == np.float32 and x.dtype == np.float32 and nrow == 2:
            # the RANSAC loop's own case: float32 H, w == 1, inverse by the kernel's float64 LU (bit-identical to numpy's)
            if inverse:
                val = np.linalg.inv(val)                  # ransac.py:74: numpy's own float32 inverse (LinAlgError on a singular val);
            h9 = torch.from_numpy(np.ascontiguousarray(val).reshape(9)).to(dev)      # the kernel then projects forward through it
            pts = torch.from_numpy(np.ascontiguousarray(x[:2].T)).to(dev)
            return kernels.project_points(h9, pts, False).cpu().numpy()
        if inverse:
            val = np.linalg.inv(val)                      # ransac.py:74: float64 inside, result in val's dtype
        dt = np.result_type(val.dtype, x.dtype)
        if dt not in (np.float32, np.float64):
            dt = np.dtype(np.float64)
        h9 = torch.from_numpy(np.ascontiguousarray(val, dtype=dt).reshape(9)).to(dev)
        pts3 = torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
        return kernels.project_points_ex(h9, pts3).cpu().numpy()

    def fwd(self, X):
        """val @ [X;1] / (row2 + 1e-10), 3 x M in numpy's result dtype (ransac.py:55-64)."""
        return self._project(X, False)

    def reproj(self, Y):
        """inv(val) @ [Y;1] / (row2 + 1e-10) (ransac.py:66-76)."""
        return self._project(Y, True)

    def dist(self, predY, trueY):
        """Column-wise L2 distance (ransac.py:78-82); two arrays in, one out: host numpy."""
        delta = (predY - trueY)
        delta = np.sum(delta * delta, axis=0)
        return np.sqrt(delta)

    def computeLoss(self, X, Y, method="reproj"):
        """Per-correspondence loss, float32 [M] (ransac.py:84-98), from the scorer kernel."""
        import torch
        if method not in _lib.RWH_LOSS:
            exit("Invalid method!")  # ransac.py:97
        if method != "fwd":
            np.linalg.inv(self.val)                       # ransac.py:74 raises LinAlgError on a singular val
        if np.asarray(self.val).dtype != np.float32 or np.asarray(X).dtype != np.float32 or np.asarray(Y).dtype != np.float32 \
                or X.shape[0] != 2 or Y.shape[0] != 2 or X.shape[1] < 2:
            # not the RANSAC loop's float32 case (e.g. model.val is the float64 refit after run()): numpy computes these in
            # float64 -- the reference's own composition of fwd / reproj / dist (ransac.py:84-96), projections on the GPU
            err = None
            if method in ("fwd", "reproj"):
                err = self.dist(self.fwd(X)[:2, :], Y)
            if method in ("backward", "reproj"):
                back = self.dist(self.reproj(Y)[:2, :], X)
                err = back if err is None else err + back
            return err
        dev = _lib.require_gpu()
        h9 = torch.from_numpy(np.ascontiguousarray(self.val, dtype=np.float32).reshape(1, 9)).to(dev)
        pa = torch.from_numpy(_points_rows(X)).to(dev)
        pb = torch.from_numpy(_points_rows(Y)).to(dev)
        best = kernels.new_best(dev)
        hinv = None if method == "fwd" else torch.from_numpy(kernels.host_inverses(np.asarray(self.val, dtype=np.float32).reshape(1, 9))).to(dev)
        _, _, err = kernels.score_count(h9, pa, pb, 0.0, method, 1 << 30, best, want_masks=False, want_err=True, hinv=hinv)
        return err[0].cpu().numpy()


class RANSAC(object):
    """ransac.py:137-213."""

    __slots__ = ('model', 'th', 'd', 'n', 'k', 'last_run', 'rescore_margin')

    def __init__(self, model, k=1000):
        self.model = model
        self.th = model.th
        self.d = model.d
        self.n = model.n
        self.k = k
        self.last_run = None
        self.rescore_margin = RESCORE_MARGIN

    def computeLoss(self, X, Y, method="reproj"):
        return self.model.computeLoss(X, Y, method)

    def run(self, data, method="reproj"):
        """Returns (finalModel float64 3x3, (inlier_indices,), count) like ransac.py:159-213 and
        sets `model.val`.  `self.last_run` keeps diagnostics (winner index, early-exit flag,
        per-hypothesis flags/counts tensors) that the reference does not expose."""
        import torch
        X, Y = data
        nx, mx = X.shape
        ny, my = Y.shape
        assert mx == my, "data observation not consistent!"
        if method not in _lib.RWH_LOSS:
            exit("Invalid method!")
        k = int(self.k)
        if k <= 0:      # the loop body never runs and ransac.py:203 reads the count it would have assigned
            raise UnboundLocalError("local variable 'lenalsoIninears' referenced before assignment")
        if self.n < 4:
            # the first iteration draws its sample (ransac.py:177), then ransac.py:180 -> homography.py:9: calc_corresp reads u[3]
            np.random.randint(0, mx, self.n)
            raise IndexError("index 3 is out of bounds for axis 0 with size %d" % self.n)
        dev = _lib.require_gpu()
        need = mx * self.d / 100 + self.n

        # sampling: identical stream to k successive randint(0, mx, n) calls (ransac.py:177); the model is fitted on the
        # first four of the n sampled correspondences (ransac.py:180 -> homography.py:4-14)
        rng_state = np.random.get_state()
        idx_host, idx_n32 = legacy_randint_table(mx, k, self.n, want64=False)
        if idx_host is None:
            idx_host = idx_n32        # (int32: the same values; numpy's own call would have returned int64)

        pa_host, pb_host = _points_rows(X), _points_rows(Y)
        # A sample that holds a NaN coordinate makes the reference's SVD raise LinAlgError at ITS iteration (homography.py:81:
        # LAPACK's dgesdd rejects a matrix with a NaN) -- unless an earlier iteration has taken the early exit.  Such samples are
        # known from the index table: search the iterations before the first of them, and raise where the reference would.
        # (+-Inf coordinates pass LAPACK's check: those samples are solved like any other flagged sample.)
        first_bad = None
        with np.errstate(invalid="ignore"):
            maybe_nan = bool(np.isnan(pa_host.sum() + pb_host.sum()))      # one reduction per run (also NaN for Inf - Inf: sorted out below)
        if maybe_nan:
            nonfinite = np.isnan(pa_host).any(axis=1) | np.isnan(pb_host).any(axis=1)
            bad_rows = nonfinite[idx_host[:, :4]].any(axis=1)
            if bad_rows.any():
                first_bad = int(np.argmax(bad_rows))
                if first_bad == 0:
                    np.random.set_state(rng_state)
                    np.random.randint(0, mx, (1, self.n))
                    raise np.linalg.LinAlgError("SVD did not converge")
                k = first_bad
                idx_host = idx_host[:k]
        idx32 = np.ascontiguousarray(idx_n32[:k, :4])
        need_i = kernels.need_count(mx, self.d, self.n)
        th = _weak_threshold(self.th)
        addr = _lapack.dgesdd_address()
        gesv = None if method == "fwd" else _lapack.dgesv_address()
        if addr is not None and not FORCE_PYTHON_DRIVER and (method == "fwd" or gesv is not None):
            # the whole driver in ONE native call (rwh_ransac_run, csrc/rwh_run.hip): upload, K1 + K2 + argmax, the settle step
            # (repeated-index samples solved on host threads while the GPU searches), the accept rules
            ws = kernels.RunWorkspace(mx, k, dev)
            try:
                winner, early, totalfit, n_set, n_rounds, n_flagged, mask_words, _keys, n_iv = kernels.ransac_run(
                    pa_host, pb_host, idx32, th, method, need_i, self.rescore_margin, ws, addr, HOST_THREADS,
                    dgesv=gesv, want_keys=True)
            except _lib.RwhError:
                # LAPACK refused a sample (info != 0: e.g. an Inf coordinate times 0 is a NaN in the DLT matrix): the step-by-step
                # driver reaches numpy.linalg.svd, which raises the reference's LinAlgError for it
                ws = None
        else:
            ws = None
        if ws is not None:
            counts_host = ws.host_counts(settled=True)
            stats = {"raw_counts": ws.host_counts(), "host_settled": n_set, "host_rounds": n_rounds, "flagged": n_flagged, "intervals": n_iv}
            Hs, flags, counts, masks = ws.H, ws.flags, ws.counts, ws.masks
            settled_rows = _SettledRows(pa_host, pb_host, idx32)
        else:
            winner, early, totalfit, mask_words, settled_rows, counts_host, stats, (Hs, flags, counts, masks) = self._run_python_driver(
                pa_host, pb_host, idx_host, idx32, k, mx, need_i, th, method, dev)

        if early:  # leave the generator where the reference's `break` would
            np.random.set_state(rng_state)
            np.random.randint(0, mx, (winner + 1, self.n))
        elif first_bad is not None:  # no early exit before the sample whose SVD fails
            np.random.set_state(rng_state)
            np.random.randint(0, mx, (first_bad + 1, self.n))
            raise np.linalg.LinAlgError("SVD did not converge")
        elif k and counts_host[k - 1] < need:  # ransac.py:203-204 tests the LAST iteration's count
            print("Warning:: fitting model does not exceed required threshold %d vs %d" % (totalfit, need))

        if winner is None:
            # ransac.py:206 with inliers_pos_final = None: whatever the installed numpy makes of np.where(None) -- an empty index
            # (then the refit asserts, ransac.py:38) up to numpy 2.0, ValueError from 2.1 on
            inliers = np.where(None)
            totalfit = 0
        else:
            words = mask_words
            bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:mx]
            inliers = (np.nonzero(bits)[0].astype(np.int64),)
            totalfit = np.int64(totalfit)
        self.last_run = {"winner": winner, "early_exit": early, "counts": counts, "flags": flags,
                         "hypotheses": Hs, "idx": idx_host, "settled": settled_rows, **stats}
        inliers_x = X[:, inliers[0]]
        inliers_y = Y[:, inliers[0]]
        DEBUG("Fitting final model using all inliers")
        finalModel = self.model.fit(inliers_x, inliers_y, collective=True)
        self.model.val = finalModel
        return finalModel, inliers, totalfit


    def _run_python_driver(self, pa_host, pb_host, idx_host, idx32, k, mx, need_i, th, method, dev):
        """The same driver step by step from Python (rounds 2-3; used when numpy's LAPACK cannot be taken by address, and by
        tests that compare the two drivers): one upload, rwh_ransac_search, `presettle` while the GPU searches, one readback,
        `_settle_on_host`."""
        import torch
        if k == 0:      # no iteration: the reference keeps no model and its refit fails (ransac.py:206-208)
            e = torch.empty(0, dtype=torch.int32, device=dev)
            return None, False, 0, None, {}, np.zeros(0, np.int32), {"raw_counts": np.zeros(0, np.int32), "host_settled": 0, "host_rounds": 0,
                                                                     "flagged": 0}, (e, e.to(torch.uint8), e, e)
        blob = torch.from_numpy(np.concatenate([pa_host.reshape(-1).view(np.uint8), pb_host.reshape(-1).view(np.uint8),
                                                idx32.reshape(-1).view(np.uint8)])).to(dev)
        nb = 8 * mx
        pa = blob[:nb].view(torch.float32).reshape(mx, 2)
        pb = blob[nb:2 * nb].view(torch.float32).reshape(mx, 2)
        idx = blob[2 * nb:].view(torch.int32).reshape(k, 4)
        ws = kernels.SearchWorkspace(k, mx, dev)
        kernels.ransac_search(pa, pb, idx, th, method, need_i, ws)             # enqueued; the host goes on
        pre = presettle(pa, pb, pa_host, pb_host, idx_host, np.flatnonzero(repeated_rows(idx_host)), th, method)
        counts_host, flags_host = ws.counts_flags()                           # one readback for counts + flags
        stats = {"raw_counts": counts_host.copy()}           # K2 on K1's own H, before the settle step
        winner, early, totalfit, mask_words, settled_rows, counts_host = _settle_on_host(
            pa, pb, pa_host, pb_host, idx_host, counts_host, flags_host, need_i, th, method, self.rescore_margin, stats, pre=pre,
            H_dev=ws.H, flags_dev=ws.flags)
        if winner is not None and mask_words is None:
            mask_words = ws.masks[winner].cpu().numpy()
        return winner, early, totalfit, mask_words, settled_rows, counts_host, stats, (ws.H, ws.flags, ws.counts, ws.masks)


class _SettledRows(object):
    """`RANSAC.last_run["settled"]` of the native driver: index -> the H the settle step gives that hypothesis, i.e. the
    reference's own (host SVD), computed on demand."""

    def __init__(self, pa, pb, idx32):
        self._pa, self._pb, self._idx = pa, pb, idx32

    def __getitem__(self, i):
        return svd_hypotheses(self._pa, self._pb, self._idx[int(i):int(i) + 1])[0]


def run_batch(datas, th=5, d=50, n=4, k=1000, method="reproj", seed=0, idx=None, problem_base=0, refit=True, info=None):
    """RANSAC over MANY image pairs in one GPU submission (the reference has no
    counterpart: its RANSAC.run handles one pair per call, ransac.py:159-213).

    datas: list of [X, Y] (each 2 x M_p or 3 x M_p, the `RANSAC.run` layout), or a `DeviceProblems` (correspondences
    already on the GPU: nothing but the winners' inlier masks -- and, with refit=True, the points for the host refit --
    comes back).  Returns a list of `(finalModel float64 3x3, (inlier_indices,), count)` -- per problem exactly what
    `RANSAC.run` returns for the same samples, including the final N-point refit on the host (ransac.py:206-211);
    `finalModel` is None for a problem whose winner has too few inliers to refit (where `RANSAC.run` raises
    AssertionError) and with refit=False (no correspondence then visits the host at all).

    refit="device": the N-point refit runs on the GPU for all problems in one launch (kernels.refit_batched); when `idx` is
    None no correspondence visits the host (with `idx=` the host settle step still downloads them).  A documented NON-PARITY mode: it solves the same least-squares problem as the reference in
    float64 and is not the reference's float32 bits (it is closer to the exact least-squares solution).  `finalModel` is None
    where the refit reports anything but RWH_REFIT_OK or the winner has fewer than `n` inliers; inliers and counts are as with
    refit=True.  `info` then also receives "H_device" ([P,3,3] float64, NaN where the status is not OK) and "refit_status"
    ([P] int32), the device tensors, for a consumer on the GPU, and with them "mask_device" ([P, words] int64: the winners' inlier
    mask rows, the layout `kernels.refit_batched` takes) and "offsets_device" ([P + 1] int32) -- what `sequence_adjust` reads
    without a visit to the host.  Any other value of `refit` raises ValueError.

    Sampling: by default on the device (Philox4x32-10 keyed by `seed`, four distinct correspondences per hypothesis):
    a documented NON-PARITY mode -- the reference draws with replacement from numpy's global legacy generator
    (ransac.py:177).  Pass `idx` (list of [k,4] integer arrays, one per problem) to supply the samples yourself; each
    problem's result then equals `RANSAC.run` on that table bit for bit.  The early-exit rule (ransac.py:186-190)
    holds per problem either way: the first hypothesis whose count reaches M*d/100 + n wins -- and in the device-sampling
    mode it also stops the work: scorer waves of later hypotheses of that problem skip (RWH_BATCH_EARLY_STOP; with the
    caller's tables every hypothesis is scored, because the host settle step may move the exit).  `problem_base`: global
    index of datas[0] when a longer problem list is split over several calls (sharded.run_batch_sharded), so that the
    device sampler draws the tables of the unsplit run.  `info`: optional dict, receives "scored" (hypotheses actually
    scored per problem) and "early" (per problem: did it exit early)."""
    import torch
    if method not in _lib.RWH_LOSS:
        exit("Invalid method!")
    if n < 4:
        raise IndexError("index 3 is out of bounds for axis 0 with size %d" % n)   # as RANSAC.run (homography.py:9)
    if not isinstance(refit, (bool, np.bool_, int, np.integer)) and refit != "device":   # truthy / falsy flags as before
        raise ValueError("refit: True (host refit, the reference's bits), False (none) or 'device', got %r" % (refit,))
    device_refit = isinstance(refit, str)
    dev = _lib.require_gpu()
    P = len(datas)
    if P == 0:
        return []
    on_device = isinstance(datas, DeviceProblems)
    if on_device:
        sizes = datas.sizes
        pa, pb = datas.pts_a, datas.pts_b
    else:
        sizes = []
        for X, Y in datas:
            assert X.shape[1] == Y.shape[1], "data observation not consistent!"
            sizes.append(X.shape[1])
        pa = torch.from_numpy(np.concatenate([_points_rows(X) for X, _ in datas])).to(dev)
        pb = torch.from_numpy(np.concatenate([_points_rows(Y) for _, Y in datas])).to(dev)
    offsets = np.zeros(P + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(sizes)
    needs_host = [kernels.need_count(m, d, n) for m in sizes]
    needs = torch.tensor(needs_host, dtype=torch.int32, device=dev)
    offsets_dev = torch.from_numpy(offsets).to(dev)
    ws = kernels.BatchWorkspace(P, int(k), max(max(sizes), 1), dev)
    if idx is not None:
        if len(idx) != P:
            raise ValueError("idx: one [k, n] table per problem (%d tables for %d problems)" % (len(idx), P))
        tables = []
        for p_, t in enumerate(idx):        # numpy's own indexing rules (ransac.py:178 `data[:, idx]`): negative indices wrap, others raise
            t = np.asarray(t)
            if t.ndim != 2 or t.shape[0] != int(k) or t.shape[1] < 4:
                raise ValueError("idx[%d]: expected a [%d, >= 4] integer array, got shape %s" % (p_, int(k), t.shape))
            m_ = sizes[p_]
            if t.size and (int(t.min()) < -m_ or int(t.max()) >= m_):
                bad = int(t.max()) if int(t.max()) >= m_ else int(t.min())
                raise IndexError("index %d is out of bounds for axis 1 with size %d" % (bad, m_))
            tables.append(np.where(t < 0, t + m_, t))
        idx = tables
        table = torch.from_numpy(np.stack([t[:, :4].astype(np.int32) for t in idx])).to(dev)   # fit on the first four
        kernels.ransac_batched(pa, pb, offsets_dev, needs, _weak_threshold(th), method, ws, idx=table)
    else:
        kernels.ransac_batched(pa, pb, offsets_dev, needs, _weak_threshold(th), method, ws, seed=seed,
                               problem_base=problem_base, early_stop=True)
    pa_host = pb_host = None
    if idx is not None or (refit and on_device and not device_refit):
        pa_host, pb_host = pa.cpu().numpy(), pb.cpu().numpy()
    if idx is not None:
        # the caller's tables may hold repeated indices (numpy's sampler draws with replacement): settle every problem
        # with the reference's solver, exactly as RANSAC.run does
        counts_host = ws.counts.cpu().numpy()
        flags_host = ws.flags.cpu().numpy()
        winners, win_counts, host_masks = [], [], []
        for p in range(P):
            o0, o1 = int(offsets[p]), int(offsets[p + 1])
            w, early, cnt, words, _, _ = _settle_on_host(pa[o0:o1], pb[o0:o1], pa_host[o0:o1], pb_host[o0:o1], np.asarray(idx[p])[:, :4],
                                                     counts_host[p], flags_host[p], needs_host[p], _weak_threshold(th),
                                                     method, RESCORE_MARGIN, H_dev=ws.H[p], flags_dev=ws.flags[p])
            winners.append((w, None, early)); win_counts.append(cnt); host_masks.append(words)
    else:
        best = ws.best.cpu().numpy()
        winners = [kernels.decode_best(best[p], int(k)) for p in range(P)]
        host_masks = [None] * P
    rows = torch.tensor([[p, w[0] if w[0] is not None else 0] for p, w in enumerate(winners)], device=dev)
    win_dev = ws.masks[rows[:, 0], rows[:, 1]]
    win_masks = win_dev.cpu().numpy()                                   # one gather, one copy for all problems
    if idx is None:
        win_counts = ws.counts[rows[:, 0], rows[:, 1]].cpu().numpy()
    if info is not None:
        info["scored"] = (ws.counts >= 0).sum(dim=1).cpu().numpy()
        info["early"] = [bool(w[2]) for w in winners]
    if device_refit:
        # the winners' mask rows are on the device already; rows the host settle step replaced (and winners that do not exist)
        # are overwritten by one upload
        patch = {p: host_masks[p] for p in range(P) if host_masks[p] is not None or winners[p][0] is None}
        if patch:
            words = np.zeros((len(patch), ws.words), dtype=np.int64)
            for j, w in enumerate(patch.values()):
                if w is not None:
                    w = np.ascontiguousarray(w).view(np.int64).ravel()
                    words[j, :w.size] = w
            win_dev[torch.tensor(list(patch), device=dev)] = torch.from_numpy(words).to(dev)
        H_dev, status_dev = kernels.refit_batched(pa, pb, offsets_dev, win_dev)
        both = torch.cat([H_dev.reshape(P, 9), status_dev.to(torch.float64)[:, None]], dim=1).cpu().numpy()   # one copy
        if info is not None:
            info["H_device"], info["refit_status"] = H_dev, status_dev
            info["mask_device"], info["offsets_device"] = win_dev, offsets_dev
    out = []
    for p, (winner, _, early) in enumerate(winners):
        model = HomoModel(th=th, d=d, n=n)
        if winner is None or int(win_counts[p]) == 0:
            inliers, total = (np.array([], dtype=np.int64),), 0
        else:
            words = host_masks[p] if host_masks[p] is not None else win_masks[p]
            bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:sizes[p]]
            inliers, total = (np.nonzero(bits)[0].astype(np.int64),), np.int64(win_counts[p])
        H = None
        if device_refit:
            if both[p, 9] == _lib.RWH_REFIT_OK and int(total) >= n:     # fewer inliers than n: None, as the host refit
                H = both[p, :9].reshape(3, 3).copy()
        elif refit:
            if on_device:
                o0 = int(offsets[p])
                X, Y = pa_host[o0:o0 + sizes[p]].T, pb_host[o0:o0 + sizes[p]].T
            else:
                X, Y = datas[p]
            try:
                H = model.fit(X[:, inliers[0]], Y[:, inliers[0]], collective=True)
            except AssertionError:      # fewer inliers than a refit needs: RANSAC.run would raise here (ransac.py:38)
                H = None
        out.append((H, inliers, total))
    return out


def _match_features(trainImg, queryImg):
    """ORB + brute-force Hamming matcher of ransac.py:252-267.  This is OpenCV C++ and outside the
    GPU path; it runs only when cv2 is installed."""
    try:
        import cv2
    except ImportError as e:
        raise ImportError("stitching() needs OpenCV for ORB/BFMatcher, or pass matches=(ptsA, ptsB) "
                          "(float32 [N,2] each, the matchespoints.npy layout)") from e
    trainImg_gray = cv2.cvtColor(trainImg, cv2.COLOR_RGB2GRAY)
    queryImg_gray = cv2.cvtColor(queryImg, cv2.COLOR_RGB2GRAY)
    descriptor = cv2.ORB_create()
    kpsA, featuresA = descriptor.detectAndCompute(trainImg_gray, None)
    kpsB, featuresB = descriptor.detectAndCompute(queryImg_gray, None)
    bf = cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=True)
    found = sorted(bf.match(featuresA, featuresB), key=lambda m: m.distance)
    kpsA = np.float32([kp.pt for kp in kpsA])
    kpsB = np.float32([kp.pt for kp in kpsB])
    return np.float32([kpsA[m.queryIdx] for m in found]), np.float32([kpsB[m.trainIdx] for m in found])


def stitching(trainImg, queryImg, ransacMet="fwd", th=5, d=70, n=4, k=1000, blending=False, blendrate=0.2,
              mode=None, override=0, cylinderT=1, matches=None, features=None):
    """Panorama pipeline of ransac.py:235-283: matches -> RANSAC homography -> warp + composite.
    `matches=(ptsA, ptsB)` injects precomputed correspondences so the
    GPU path works without OpenCV; `features=(kpsA, descA, kpsB, descB)` (keypoints float32 [N, 2], binary descriptors uint8
    [N, nbytes], A = trainImg's) injects the extractor's output and matches it on the GPU (`match_descriptors`);
    `features="extract"` extracts both images on the GPU first (`extract_batch` with its defaults: the rule stated there, on one
    scale, which is not OpenCV's ORB); a dict does the same with its entries as `extract_batch`'s keyword arguments, e.g.
    `features={"n_levels": 8}` for a pair whose images differ in zoom.  `matches` wins over `features`; with neither, the OpenCV path runs.  Everything else keeps the reference's
    signature."""
    if override != 0:
        import cv2
        status, imgn = cv2.Stitcher_create().stitch([trainImg, queryImg])
        return imgn
    if matches is not None:
        ptsA, ptsB = matches
    elif features is not None:
        if isinstance(features, (str, dict)):
            if isinstance(features, str) and features != "extract":
                raise ValueError("stitching: features=%r; 'extract', a dict of extract_batch's arguments or (kpsA, descA, kpsB, descB)" % features)
            (kpsA, descA), (kpsB, descB) = extract_batch([trainImg, queryImg], **(features if isinstance(features, dict) else {}))
        else:
            kpsA, descA, kpsB, descB = features
        qi, ti, _ = match_descriptors(descA, descB)
        ptsA, ptsB = _host_rows(kpsA)[qi], _host_rows(kpsB)[ti]
    else:
        ptsA, ptsB = _match_features(trainImg, queryImg)
    ptsA = np.asarray(ptsA, dtype=np.float32)
    ptsB = np.asarray(ptsB, dtype=np.float32)
    if mode is None:
        model = HomoModel(th=th, d=d, n=4)
        H, inliers, _len = RANSAC(model, k=k).run([ptsA.T, ptsB.T], method=ransacMet)
    else:
        import cv2
        H, status = cv2.findHomography(ptsA, ptsB, cv2.RANSAC, 4)
    return stitchPanorama(queryImg, trainImg, H=H, blending=blending, blendrate=blendrate)


def stitch_sequence(images, anchor=0, th=5, d=70, k=1000, ransacMet="fwd", seed=0, blending=False, features=None, info=None, gains=None,
                    projection=None, focal=None, pairs="adjacent", adjust=False, bands=5):
    """Pixels -> panorama for a SEQUENCE of N overlapping images (images[i+1] overlaps images[i]), every stage batched: one
    `extract_batch` over the N images, one `match_batch` over the N - 1 adjacent pairs, one `run_batch(refit="device")`, one download
    of the [N - 1, 3, 3] homographies -- the only geometry that visits the host, because the canvas must be allocated -- and one
    pass of the sequence compositor (`stitchSequence`, which chains the homographies into the anchor's frame).  The reference
    stitches two images per call (ransac.py:235-283); this goes beyond it, under the rules stated for each stage in include/rwh.h.

    th, d, k, ransacMet, seed: as `run_batch`'s (device sampling, the float64 device refit: a NON-PARITY mode);
    features: a dict of `extract_batch`'s keyword arguments; anchor, blending, bands, gains: as `stitchSequence`'s
    (blending="multiband": multi-band blending with `bands` pyramid levels, checked before any GPU work; blending="seams" and
    "multiband+seams": `stitchSequence(blending=False | "multiband", seams=True)`, seam finding by the seam rule of include/rwh.h
    with its defaults, then label paste or labelled multi-band -- not on a canvas that wraps; gains="auto": exposure
    gains from the overlaps, `sequence_gains` with its defaults; gains="blocks": one gain map per image, `sequence_block_gains`
    with its defaults, which `stitch_ring` refuses).  numpy arrays in -> a numpy canvas, tensors in -> a device
    tensor.  `info`: optional dict, receives "Hs" (float64 [N - 1, 3, 3], Hs[i] maps image i+1 into image i), "Gs", "origin"
    ((ox, oy) of the canvas in the anchor's frame), "sizes" (matches per pair), "inliers" (per pair) and "gains" (the gains used,
    float64 [N], or None).  projection, focal: as `stitchSequence`'s (a cylindrical or spherical canvas, for sweeps too wide for the
    anchor's plane; "origin" is then in surface pixels); focal="auto" calls `sequence_focal` on the estimated homographies, and
    `info` receives "focal" (the focal used, or None).  ValueError: a pair without a homography (too few matches or inliers, a singular refit), naming the pair and its
    match count; whatever `stitchSequence` refuses.

    pairs, adjust: registration over a pair graph (the bundle rule of include/rwh.h).  pairs="adjacent" (default): the N - 1 pairs
    (i + 1, i), chained.  pairs="all" or a list of (s, d): those pairs are matched and searched in one `match_batch` and one
    `run_batch(refit="device")` (features of s against features of d, H maps s into d), `sequence_graph` accepts the verified
    ones and initialises every G_i along a maximum spanning tree from the anchor, so the images need not come in order.
    adjust=True: `sequence_adjust` then refines all G_i jointly over the inliers of the accepted pairs, correspondences and masks
    staying on the device.  The canvas comes from `stitchSequence(images, Gs=...)`.  `info` then receives "pairs", "accepted"
    (bool per pair), "tree" and "adjust" (`sequence_adjust`'s info, or None); "Hs" is set only with pairs="adjacent".  The
    defaults make the calls and give the results they always did.  `bands` stays the last parameter: pass it, and everything
    behind `focal`, by name.  ValueError, before the GPU is asked for: another `pairs` or `adjust`.

    adjust="cameras" or "cameras-per-image": the adjustment runs over rotations and focal lengths instead (the camera rule of
    include/rwh.h), four parameters per image in place of eight, with one focal length for all images or one per image.  After
    `sequence_graph` the starting focal is the numeric `focal=` where one was given (here also without a projection), else
    `sequence_focal` over the accepted pairs -- or, where no pair gives one (images that are translations of each other), the mean
    of h + w, the stand-in OpenCV's stitcher uses; then `sequence_cameras`, `sequence_adjust_cameras` with the matches and masks on
    the device, and `sequence_camera_maps`, whose G_i = K_a R_i inv(K_i) go to `stitchSequence`.  With a projection and
    focal="auto" the canvas takes the adjusted focal of the anchor.  info["adjust"] also receives "Rs" and "focals"; info["focal"]
    stays the focal of the canvas (None without a projection).

    The matcher.  A key "ratio" in the `features` dict (features={"ratio": 0.7, "n_levels": 4}) is taken out before the rest goes to
    `extract_batch`: the pairs -- adjacent or of the graph -- are then matched by `match_graph(feats, pairs, ratio)`, Lowe's ratio
    test with every image's descriptors held once, in place of `match_batch`'s cross-check.  With pairs="all" that is the matcher to
    use: cross-check's unsupported matches raise the bar of `sequence_graph`'s acceptance rule and can cost a true overlap.
    Without the key every call and result is what it was.  ValueError, before any GPU work: a ratio `match_ratio` refuses.

    A full circle.  pairs="ring": the adjacent pairs plus (0, N - 1), the pair that closes the circle, for N >= 3; it goes down the
    graph path.  Without `adjust` only the spanning tree places the images, so the drift of the chain shows at the closing overlap,
    as a step where the last image meets the first; adjust="cameras" is the mode to use, since it spreads the closing error over all
    rotations and fits the focal length that makes the circle close.  ValueError, before any GPU work: pairs="ring" with fewer than
    3 images.  The canvas of this call does not wrap around, so a sweep that closes the circle still has an image across the seam
    behind the anchor and is refused: `stitch_ring` is this call on a canvas that wraps (`wrap=`).  The parameter list of this
    function is fixed."""
    return _stitch_sequence(images, anchor, th, d, k, ransacMet, seed, blending, features, info, gains, projection, focal, pairs, adjust, bands, False)


def stitch_ring(images, anchor=0, th=5, d=70, k=1000, ransacMet="fwd", seed=0, blending=False, features=None, info=None, gains=None,
                projection="cylindrical", focal="auto", pairs="ring", adjust="cameras", bands=5, wrap=True):
    """Pixels -> a FULL-CIRCLE panorama: `stitch_sequence` on a canvas that wraps around behind the anchor (the ring rule of
    include/rwh.h).  Every parameter is `stitch_sequence`'s, with defaults that suit a sweep that closes the circle -- a cylinder,
    focal="auto", pairs="ring" (the chain plus the pair that closes it) and adjust="cameras" (the mode that spreads the closing error
    over all rotations and fits the focal length that makes the circle close; without `adjust` only the spanning tree places the
    images and the drift of the chain shows where the last image meets the first) -- and one more: wrap, as `stitchSequence`'s:
    True -- the period is `sequence_period` of the focal the canvas ends up with; a period in columns (a positive multiple of 256 up
    to 65280); False -- `stitch_sequence` itself.  `info` also receives "period" and "radius".  With fewer than 3 images pass
    pairs="adjacent".  ValueError, before any GPU work: what `stitch_sequence` refuses, wrap without a projection, a wrap that is
    neither a bool nor such a period."""
    return _stitch_sequence(images, anchor, th, d, k, ransacMet, seed, blending, features, info, gains, projection, focal, pairs, adjust, bands, wrap)


def _stitch_sequence(images, anchor, th, d, k, ransacMet, seed, blending, features, info, gains, projection, focal, pairs, adjust, bands, wrap):
    """`stitch_sequence` and `stitch_ring`: the checks that come before any GPU work, then the chain or the graph path."""
    n = len(images)
    seams = None
    if isinstance(blending, str) and blending in ("seams", "multiband+seams"):      # (the parameter lists are fixed: seams ride on `blending`)
        blending, seams = (False if blending == "seams" else "multiband"), True
        if wrap is not False:
            raise NotImplementedError("stitch_sequence: seams on a wrap-around canvas are not provided (the seam rule has no ring form)")
    ratio = None
    if isinstance(features, dict) and "ratio" in features:
        features = dict(features)
        ratio = match_ratio(features.pop("ratio"), "stitch_sequence")
    if not 1 <= n <= _lib.RWH_SEQ_MAX_IMAGES:
        raise ValueError("stitch_sequence: %d images; 1 .. %d are taken" % (n, _lib.RWH_SEQ_MAX_IMAGES))
    cameras = isinstance(adjust, str) and adjust in ("cameras", "cameras-per-image")
    if not isinstance(adjust, (bool, np.bool_)) and not cameras:
        raise ValueError("stitch_sequence: adjust=%r; True or False, 'cameras' or 'cameras-per-image'" % (adjust,))
    if isinstance(pairs, str):
        if pairs not in ("adjacent", "all", "ring"):
            raise ValueError("stitch_sequence: pairs=%r; 'adjacent', 'all', 'ring' or a list of (s, d)" % (pairs,))
        if pairs == "ring" and n < 3:
            raise ValueError("stitch_sequence: pairs='ring' takes 3 images at least, got %d" % n)
    else:
        pairs = _check_pairs("stitch_sequence", n, pairs)
        if len(set(pairs)) != len(pairs):
            raise ValueError("stitch_sequence: pairs=%r names a pair twice" % (pairs,))
    graph = adjust or pairs != "adjacent"
    if isinstance(gains, str):
        if gains not in ("auto", "blocks"):
            raise ValueError("stitch_sequence: gains=%r; None, N gains, 'auto' or 'blocks'" % (gains,))
        if gains == "blocks" and wrap is not False:
            raise NotImplementedError("stitch_ring: gains='blocks'; the block gain rule (include/rwh.h) has no ring form")
    elif gains is not None and not isinstance(gains, BlockGains):          # (a BlockGains is checked against the canvas by stitchSequence)
        gains = kernels.sequence_gains_array(gains, n, "stitch_sequence")
    if blending == "multiband":
        _check_bands("stitch_sequence", bands)
    auto_focal = isinstance(focal, str) and focal == "auto" and projection is not None
    if cameras and projection is None:      # the camera model takes a starting focal of its own, with or without a surface
        if focal is not None and not (isinstance(focal, str) and focal == "auto"):
            _check_focal("stitch_sequence", focal)
    else:
        _check_projection("stitch_sequence", projection, 1.0 if auto_focal else focal)
    _check_wrap("stitch_sequence", wrap, projection, 1.0 if auto_focal else focal)
    if graph:
        return _stitch_sequence_graph(images, anchor, dict(th=th, d=d, n=4, k=k, method=ransacMet, seed=seed), blending, features, info, gains,
                                      projection, focal, auto_focal, bands, pairs, adjust, ratio, wrap, seams)
    Hs, sizes, inliers = np.zeros((0, 3, 3)), [], []
    if n > 1:
        feats = extract_batch(images, **(features or {}))
        if ratio is None:
            pairs = match_batch([(feats[i + 1][0], feats[i + 1][1], feats[i][0], feats[i][1]) for i in range(n - 1)])
        else:
            pairs = match_graph(feats, [(i + 1, i) for i in range(n - 1)], ratio)
        sizes = [int(m) for m in pairs.sizes]
        # (run_batch brings the [N - 1, 3, 3] homographies and their refit status down in ONE copy; a pair without one gives None)
        res = run_batch(pairs, th=th, d=d, n=4, k=k, method=ransacMet, seed=seed, refit="device")
        inliers = [int(r[2]) for r in res]
        for p in range(n - 1):
            if res[p][0] is None:
                raise ValueError("stitch_sequence: pair %d (images %d and %d) has no homography: %d matches, %d inliers"
                                 % (p, p, p + 1, sizes[p], inliers[p]))
        Hs = np.stack([r[0] for r in res])
    shapes = [tuple(int(v) for v in img.shape) for img in images]
    if auto_focal:
        focal = sequence_focal(shapes, Hs)
    Gs, _, origin, _, _ = sequence_plan(shapes, Hs, anchor, projection, focal, wrap)
    if info is not None:
        info["Hs"], info["Gs"], info["origin"], info["sizes"], info["inliers"] = Hs, Gs, origin, sizes, inliers
        info["focal"] = focal
    used = {}
    out = stitchSequence(images, Hs=Hs, anchor=anchor, blending=blending, gains=gains, info=used, bands=bands, projection=projection,
                         focal=focal, wrap=wrap, seams=seams)
    if info is not None:
        info["gains"] = used["gains"]
        if "passes" in used:
            info["passes"], info["labels"] = used["passes"], used["labels"]
        if wrap is not False:
            info["period"], info["radius"] = used["period"], used["radius"]
    return out


def _stitch_sequence_graph(images, anchor, search, blending, features, info, gains, projection, focal, auto_focal, bands, pairs, adjust,
                           ratio=None, wrap=False, seams=None):
    """`stitch_sequence` over a pair graph: one extract, one match (`match_batch`, or `match_graph` with a ratio) and one search over
    the listed pairs, `sequence_graph`, with adjust=True `sequence_adjust` on the device -- with adjust="cameras" or
    "cameras-per-image" `sequence_cameras`, `sequence_adjust_cameras` on the device and `sequence_camera_maps` --, then
    `stitchSequence(Gs=...)`."""
    n = len(images)
    adjacent = isinstance(pairs, str) and pairs == "adjacent"
    if isinstance(pairs, str):
        if pairs == "all":
            pairs = [(s, d) for d in range(n) for s in range(d + 1, n)]
        else:       # the chain, and with "ring" the pair that closes the circle
            pairs = [(i + 1, i) for i in range(n - 1)] + ([] if adjacent else [(0, n - 1)])
    Hs, sizes, inliers, masks, problems = [], [], [], None, None
    if pairs:
        feats = extract_batch(images, **(features or {}))
        if ratio is None:
            problems = match_batch([(feats[s][0], feats[s][1], feats[d][0], feats[d][1]) for s, d in pairs])
        else:
            problems = match_graph(feats, pairs, ratio)
        sizes = [int(m) for m in problems.sizes]
        found = {}
        res = run_batch(problems, refit="device", info=found, **search)
        Hs, inliers, masks = [r[0] for r in res], [int(r[2]) for r in res], found["mask_device"]
    Gs, accepted, tree = sequence_graph(n, pairs, Hs, sizes, inliers, anchor)
    adjusted = None
    shapes = [tuple(int(v) for v in img.shape) for img in images]
    cameras = isinstance(adjust, str)

    def estimate():
        return sequence_focal(shapes, [H for H, ok in zip(Hs, accepted) if ok], pairs=[pr for pr, ok in zip(pairs, accepted) if ok])

    if cameras and pairs:
        import torch
        adjusted = {}
        masks = masks.clone()
        masks[torch.from_numpy(~accepted).to(masks.device)] = 0
        if focal is None or isinstance(focal, str):
            try:
                start = estimate()
            except ValueError:
                # no pair gives a focal length (images that are translations of each other): the stand-in of OpenCV's stitcher
                start = float(np.mean([shape[0] + shape[1] for shape in shapes]))
        else:
            start = float(focal)
        Rs, fs = sequence_cameras(shapes, Gs, start, anchor)
        Rs, fs = sequence_adjust_cameras(shapes, Rs, fs, pairs, problems, masks=masks, anchor=anchor, on="device", info=adjusted,
                                         focals="shared" if adjust == "cameras" else "per-image")
        adjusted["Rs"], adjusted["focals"] = Rs, fs
        Gs = sequence_camera_maps(shapes, Rs, fs, anchor)
        if projection is None:
            focal = None
        elif auto_focal:
            focal = float(fs[anchor])
    elif cameras:
        focal = None if projection is None else focal
    elif adjust and pairs:
        import torch
        adjusted = {}
        masks = masks.clone()
        masks[torch.from_numpy(~accepted).to(masks.device)] = 0      # an edge that is not accepted has no inliers: a zero block
        Gs = sequence_adjust(Gs, pairs, problems, masks=masks, anchor=anchor, on="device", info=adjusted)
    if auto_focal and isinstance(focal, str):
        focal = estimate()
    if info is not None:
        _, origin, _, _, _, _ = _sequence_inputs("stitch_sequence", images, None, Gs, anchor, projection, focal, wrap)
        info["Gs"], info["origin"] = (Gs if projection is None else _oriented(Gs)), origin
        info["sizes"], info["inliers"], info["focal"] = sizes, inliers, focal
        info["pairs"], info["accepted"], info["tree"], info["adjust"] = pairs, accepted, tree, adjusted
        if adjacent:        # every pair of a chain is accepted, or sequence_graph has raised
            info["Hs"] = np.stack(Hs) if Hs else np.zeros((0, 3, 3))
    used = {}
    out = stitchSequence(images, Gs=Gs, anchor=anchor, blending=blending, gains=gains, info=used, bands=bands, projection=projection,
                         focal=focal, wrap=wrap, seams=seams)
    if info is not None:
        info["gains"] = used["gains"]
        if "passes" in used:
            info["passes"], info["labels"] = used["passes"], used["labels"]
        if wrap is not False:
            info["period"], info["radius"] = used["period"], used["radius"]
    return out
