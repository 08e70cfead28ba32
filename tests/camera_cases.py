"""The camera rule (include/rwh.h: the normal-equation blocks of a bundle adjustment over rotations and focal lengths) restated in
numpy -- a plain loop over the rows in the stated order, vectorised over the 45 entries of a block --, the exact-rational model of
one correspondence with the forward rounding bound of the stated operation sequence, the generators (random edges over turning
cameras, the GRID scene of bundle_cases as cameras), the ctypes drivers of the host twin and the step, and the whole problem stated
independently: the cost from the geometry and its minimum by a plain numpy optimiser over GLOBAL rotation vectors and focal
lengths with finite-difference Jacobians.  Shared by tests/test_sequence_cameras_cpu.py and tests/test_sequence_cameras_gpu.py;
nothing here calls the library's Python layer except `device_blocks`."""
from fractions import Fraction

import numpy as np

import bundle_cases as bc
import projection_cases as pc

BLOCK, PARAMS, N_S, RECORD = 45, 8, 36, 15
OK, BEHIND, SINGULAR = bc.OK, bc.BEHIND, bc.SINGULAR
SHARED, PER_IMAGE = 0, 1
fma = bc.fma


# ---- the rule ----
def entries():
    """The (i0, j0, i1, j1) of every block entry, as index arrays into a row's 18 values [J0 (8), J1 (8), r0, r1]."""
    quad = [(a, b, 8 + a, 8 + b) for a in range(8) for b in range(a, 8)]
    quad += [(k, 16, 8 + k, 17) for k in range(8)] + [(16, 16, 17, 17)]
    return tuple(np.array(col) for col in zip(*quad))


def row_values(rec, a, b):
    """The 18 values of one correspondence, or None where it is not valid.  Written from the rule's general formula: a dv of three
    components for each of the seven columns that have one, zeros included as operands."""
    rec = np.asarray(rec, dtype=np.float64)
    R, (fs, cxs, cys, fd, cxd, cyd) = rec[:9].reshape(3, 3), rec[9:]
    f64 = np.float64
    with np.errstate(all="ignore"):
        u = [f64(a[0]) - cxs, f64(a[1]) - cys, fs]
        v = [f64(fma(R[i, 2], u[2], fma(R[i, 1], u[1], R[i, 0] * u[0]))) for i in range(3)]
        m = [v[0] / v[2], v[1] / v[2]]
        q = [f64(fma(fd, m[0], cxd)), f64(fma(fd, m[1], cyd))]
        if not (np.isfinite(v[2]) and v[2] > 0 and np.isfinite(q[0]) and np.isfinite(q[1])):
            return None
        dv = [[f64(fma(R[i, 2], u[1], R[i, 1] * -u[2])) for i in range(3)],
              [f64(fma(R[i, 2], -u[0], R[i, 0] * u[2])) for i in range(3)],
              [f64(fma(R[i, 1], u[0], R[i, 0] * -u[1])) for i in range(3)],
              [R[i, 2] * u[2] for i in range(3)],
              [f64(0.0), v[2], -v[1]], [-v[2], f64(0.0), v[0]], [v[1], -v[0], f64(0.0)]]
        row = np.empty(18)
        for k in range(7):
            for c in range(2):
                row[8 * c + k] = (fd * (dv[k][c] - m[c] * dv[k][2])) / v[2]
        row[7], row[15] = fd * m[0], fd * m[1]
        row[16], row[17] = q[0] - f64(b[0]), q[1] - f64(b[1])
    return row


def restate(pts_a, pts_b, offsets, masks, records, cache=None):
    """-> (blocks float64 [E, 45], count, status) of the rule.  cache: a dict that keeps the rows between calls over the same
    points and records (the masks may differ)."""
    i0, j0, i1, j1 = entries()
    E = len(offsets) - 1
    blocks, count, status = np.zeros((E, BLOCK)), np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32)
    masks = np.asarray(masks).view(np.uint64)
    cache = {} if cache is None else cache
    for e in range(E):
        part = np.zeros((4, BLOCK))
        for i in range(int(offsets[e + 1]) - int(offsets[e])):
            if not bc.mask_bit(masks[e], i):
                continue
            if (e, i) not in cache:
                cache[(e, i)] = row_values(records[e], pts_a[offsets[e] + i], pts_b[offsets[e] + i])
            row = cache[(e, i)]
            if row is None:
                status[e] = BEHIND
                continue
            count[e] += 1
            part[i % 4] = part[i % 4] + (row[i0] * row[j0] + row[i1] * row[j1])
        blocks[e] = (part[0] + part[1]) + (part[2] + part[3])
    return blocks, count, status


def unpack(block):
    """-> (S symmetric [8, 8], g [8], c) of one block."""
    S = np.zeros((8, 8))
    S[np.triu_indices(8)] = block[:N_S]
    S = S + np.triu(S, 1).T
    return S, block[N_S:N_S + 8].copy(), float(block[44])


# ---- the geometry, independently of the library ----
def centre(shape):
    return (shape[1] - 1) / 2.0, (shape[0] - 1) / 2.0


def records(shapes, Rs, fs, pairs):
    """The edge records: R_d^T R_s row-major, then f_s, cx_s, cy_s, f_d, cx_d, cy_d."""
    out = np.empty((len(pairs), RECORD))
    for e, (s, d) in enumerate(pairs):
        out[e, :9] = (np.asarray(Rs[d]).T @ np.asarray(Rs[s])).reshape(9)
        out[e, 9:] = [fs[s], *centre(shapes[s]), fs[d], *centre(shapes[d])]
    return out


def maps(shapes, Rs, fs, anchor=0):
    """G_i = K_a R_i inv(K_i), the anchor's the identity exactly."""
    Ka = pc.camera(shapes[anchor], fs[anchor])
    Gs = np.stack([Ka @ R @ np.linalg.inv(pc.camera(shape, f)) for shape, R, f in zip(shapes, Rs, fs)])
    Gs[anchor] = np.eye(3)
    return Gs


def rodrigues(w):
    t = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if t < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / (t * t) * (K @ K)


def rotation_vector(R):
    """The w with rodrigues(w) = R, for angles below pi."""
    t = np.arccos(np.clip((np.trace(R) - 1) / 2, -1.0, 1.0))
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return axis / 2 if t < 1e-9 else axis * t / (2 * np.sin(t))


# ---- one correspondence in exact rationals, and the forward bound of the stated operations ----
def _cross_matrix(w):
    return [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]


def exact_residual(rec, a, b, delta_s, delta_d):
    """r of the rule in exact rationals under the stated local update to first order in omega: R_s (I + [omega_s]x),
    R_d (I + [omega_d]x), f (1 + phi); delta = (omega_0, omega_1, omega_2, phi).  The exponential differs from I + [omega]x from the
    second order on, which a derivative at 0 does not see."""
    F = Fraction
    R = [[F(float(rec[3 * i + j])) for j in range(3)] for i in range(3)]
    fs, cxs, cys, fd, cxd, cyd = [F(float(v)) for v in rec[9:]]

    def upd(w):
        X = _cross_matrix(w)
        return [[F(int(i == j)) + X[i][j] for j in range(3)] for i in range(3)]

    def mul(A, B):
        return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]

    Ud = upd(delta_d[:3])
    UdT = [[Ud[j][i] for j in range(3)] for i in range(3)]
    M = mul(mul(UdT, R), upd(delta_s[:3]))
    u = [F(float(a[0])) - cxs, F(float(a[1])) - cys, fs * (1 + delta_s[3])]
    v = [sum(M[i][k] * u[k] for k in range(3)) for i in range(3)]
    f = fd * (1 + delta_d[3])
    return f * v[0] / v[2] + cxd - F(float(b[0])), f * v[1] / v[2] + cyd - F(float(b[1]))


def exact_jacobian(rec, a, b, h=Fraction(1, 10 ** 30)):
    """J [2][8] in exact rationals by a central difference of `exact_residual` with step h."""
    J = [[None] * 8 for _ in range(2)]
    zero = [Fraction(0)] * 4
    for k in range(8):
        step = [h if j == k % 4 else Fraction(0) for j in range(4)]
        back = [-v for v in step]
        hi = exact_residual(rec, a, b, step, zero) if k < 4 else exact_residual(rec, a, b, zero, step)
        lo = exact_residual(rec, a, b, back, zero) if k < 4 else exact_residual(rec, a, b, zero, back)
        for c in range(2):
            J[c][k] = (hi[c] - lo[c]) / (2 * h)
    return J


def jacobian_bound(rec, a):
    """-> (J exact [2][8] by the rule's formulas in rationals, bound [2][8]): the forward rounding bound of every J entry of the
    stated operation sequence, propagated operation by operation from the operands (bundle_cases._Run: every rounded operation adds
    u times the magnitude of what it rounds, inherited errors go through the operation's own algebra).  The operations on a zero
    component of dv are counted like any other, which only makes the bound larger."""
    Rn = bc._Run
    R = [[Rn(Fraction(float(rec[3 * i + j]))) for j in range(3)] for i in range(3)]
    fs, cxs, cys, fd = [Rn(Fraction(float(v))) for v in rec[9:13]]
    u = [Rn(Fraction(float(a[0]))).sub(cxs), Rn(Fraction(float(a[1]))).sub(cys), fs]
    v = [R[i][2].fma(u[2], R[i][1].fma(u[1], R[i][0].mul(u[0]))) for i in range(3)]
    m = [v[0].div(v[2]), v[1].div(v[2])]
    zero = Rn(0)
    dv = [[R[i][2].fma(u[1], R[i][1].mul(u[2].neg())) for i in range(3)],
          [R[i][2].fma(u[0].neg(), R[i][0].mul(u[2])) for i in range(3)],
          [R[i][1].fma(u[0], R[i][0].mul(u[1].neg())) for i in range(3)],
          [R[i][2].mul(u[2]) for i in range(3)],
          [zero, v[2], v[1].neg()], [v[2].neg(), zero, v[0]], [v[1], v[0].neg(), zero]]
    J = [[fd.mul(dv[k][c].sub(m[c].mul(dv[k][2]))).div(v[2]) for k in range(7)] + [fd.mul(m[c])] for c in range(2)]
    return [[x.v for x in r] for r in J], [[x.e for x in r] for r in J]


# ---- generators ----
SHAPE = (120, 160)


def random_cameras(n, seed, yaw=0.12):
    """n cameras that turn by `yaw` per image with a little pitch and roll, focal lengths within 5 % of 150 -> (shapes, Rs, fs)."""
    rng = np.random.default_rng(seed)
    Rs = [np.eye(3)] + [pc.rotation(yaw * i + rng.uniform(-0.02, 0.02), rng.uniform(-0.05, 0.05), rng.uniform(-0.03, 0.03)) for i in range(1, n)]
    return [SHAPE] * n, np.stack(Rs), 150.0 * (1 + rng.uniform(-0.05, 0.05, n))


def transfer(shapes, Rs, fs, s, d):
    return pc.camera(shapes[d], fs[d]) @ Rs[d].T @ Rs[s] @ np.linalg.inv(pc.camera(shapes[s], fs[s]))


def size_list_case(seed=11, n=5, sizes=bc.SIZES, yaw=0.12):
    """len(sizes) edges over n turning cameras, edge e with sizes[e] correspondences in [0, 160) x [0, 120), b = the true transfer
    of a plus 0.5 px noise, float32 -> dict(pairs, rec, pa, pb, offsets, sizes, shapes, Rs, fs)."""
    rng = np.random.default_rng(seed)
    shapes, Rs, fs = random_cameras(n, seed, yaw)
    every = [(s, d) for d in range(n) for s in range(d + 1, n)]
    pairs = [every[e] if e < len(every) else every[e - len(every)][::-1] for e in range(len(sizes))]
    pa = (rng.uniform(0, 1, (sum(sizes), 2)) * [160.0, 120.0]).astype(np.float32)
    offsets = np.zeros(len(sizes) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(sizes)
    pb = np.empty_like(pa)
    for e, (s, d) in enumerate(pairs):
        o0, o1 = offsets[e], offsets[e + 1]
        pb[o0:o1] = (bc.project(transfer(shapes, Rs, fs, s, d), pa[o0:o1]) + rng.normal(0, 0.5, (o1 - o0, 2))).astype(np.float32)
    return dict(pairs=pairs, rec=records(shapes, Rs, fs, pairs), pa=pa, pb=pb, offsets=offsets, sizes=list(sizes), shapes=shapes, Rs=Rs, fs=fs)


def behind_case():
    """Edge 1 of three gets a record that turns by 0.5 rad about y: v2 = -sin(0.5) u0 + cos(0.5) 150 is positive for every x in
    [0, 160) and negative at x = 500 (u0 = 420.5), where row 70 is put."""
    c = size_list_case(seed=21, sizes=[65, 129, 5])
    pa, rec = c["pa"].copy(), c["rec"].copy()
    pa[c["offsets"][1] + 70] = [500.0, 10.0]
    rec[1, :9] = pc.rotation(0.5).reshape(9)
    rec[1, 9], rec[1, 12] = 150.0, 150.0
    masks = bc.mask_sets(c["sizes"])["ones"]
    cleared = masks.copy()
    cleared[1, 1] &= ~np.int64(1 << (70 - 64))
    return c, pa, rec, masks, cleared


def launch_case():
    """The largest launch with one row each: 2016 edges (every pair of 64 cameras 0.01 rad apart) -> the case."""
    return size_list_case(seed=5, n=64, sizes=[1] * 2016, yaw=0.01)


def single_edge(c, masks, e):
    o0, o1 = int(c["offsets"][e]), int(c["offsets"][e + 1])
    return (np.ascontiguousarray(c["pa"][o0:o1]), np.ascontiguousarray(c["pb"][o0:o1]), np.array([0, o1 - o0], dtype=np.int32),
            np.ascontiguousarray(masks[e:e + 1]), c["rec"][e:e + 1])


def grid_cameras():
    """The GRID scene of bundle_cases as cameras: -> (scene, shapes, true Rs relative to image 0, true focal)."""
    g = bc.GRID
    Rs = [pc.rotation(g["yaw"] * c, g["pitch"] * r) for r in range(g["rows"]) for c in range(g["cols"])]
    return bc.grid_scene(), [(g["h"], g["w"])] * len(Rs), np.stack([Rs[0].T @ R for R in Rs]), g["f"]


# ---- the host twins ----
def host_blocks(lib, pa, pb, offsets, masks, rec):
    """rwh_host_camera_blocks through bundle_cases.rule_host_blocks: the outputs between canaries."""
    return bc.rule_host_blocks(lib, "rwh_host_camera_blocks", BLOCK, RECORD, pa, pb, offsets, masks, rec)


def device_blocks(pa, pb, offsets, masks, rec):
    """kernels.camera_blocks through bundle_cases.rule_device_blocks: the outputs between guard words."""
    return bc.rule_device_blocks("camera", BLOCK, pa, pb, offsets, masks, rec)


def host_step(lib, n, anchor, focals, pairs, blocks, lam):
    """rwh_host_camera_step -> (status of the call, delta [n, 4], step status), delta between canaries."""
    edges = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    blocks = np.ascontiguousarray(blocks, dtype=np.float64)
    buf, status = np.full(4 * max(n, 0) + 16, -7.0), np.full(1, -1, dtype=np.int32)
    st = lib.rwh_host_camera_step(n, anchor, focals, edges.ctypes.data, len(edges), blocks.ctypes.data, float(lam), buf[8:].ctypes.data,
                                  status.ctypes.data)
    assert (buf[:8] == -7.0).all() and (buf[-8:] == -7.0).all()
    return st, buf[8:-8].reshape(max(n, 0), 4).copy(), int(status[0])


def assemble(n, anchor, focals, pairs, blocks, lam):
    """The step's system in numpy: -> (A with lambda * diag added, g, slot): over 4 n parameters (omega, phi per image) first, then
    reduced by the matrix P that drops the anchor's omega and, with one focal for all, sums every phi into one unknown; slot[j] is
    the list of the 4 n parameters that unknown j stands for."""
    A, g = np.zeros((4 * n, 4 * n)), np.zeros(4 * n)
    for (s, d), blk in zip(pairs, blocks):
        S, ge, _ = unpack(blk)
        at = np.concatenate([np.arange(4 * s, 4 * s + 4), np.arange(4 * d, 4 * d + 4)])
        A[np.ix_(at, at)] += S
        g[at] += ge
    slot = [[4 * i + k] for i in range(n) if i != anchor for k in range(3)]
    slot += [[4 * i + 3] for i in range(n)] if focals == PER_IMAGE else [[4 * i + 3 for i in range(n)]]
    P = np.zeros((4 * n, len(slot)))
    for j, members in enumerate(slot):
        P[members, j] = 1.0
    A, g = P.T @ A @ P, P.T @ g
    A[np.diag_indices_from(A)] += lam * np.diag(A)
    return A, g, slot


# ---- the whole problem stated independently: the cost from the geometry, its minimum by a plain optimiser ----
def reference_cost(shapes, Rs, fs, pairs, matches, anchor=0, masks=None):
    """The cost at (Rs, fs) from the geometry alone: bundle_cases.reference_cost at the maps K_a R_i inv(K_i)."""
    return bc.reference_cost(maps(shapes, Rs, fs, anchor), pairs, matches, masks)


def reference_optimum(shapes, Rs0, fs0, pairs, matches, anchor, focals):
    """The minimum of `reference_cost` by Levenberg-Marquardt in plain numpy -> dict(Rs, fs, cost, se, steps).  Another
    parameterisation than the library's: GLOBAL rotation vectors w_i (R_i = exp([w_i]x)) of every image but the anchor and the focal
    length(s) themselves, not local updates; the Jacobian by forward differences of the residual vector (step 1e-7 for a rotation
    vector's component, 1e-7 of a focal).  se: the standard error of every focal unknown from its own normal matrix,
    sqrt(sigma^2 inv(J^T J)_ff) with sigma^2 = cost / (rows - unknowns).  The optimiser only has to FIND the minimum; what it
    returns is judged by `reference_cost`."""
    rows = bc._inlier_rows(matches, None)
    n = len(shapes)
    free = [i for i in range(n) if i != anchor]
    n_f = n if focals == PER_IMAGE else 1

    def unpack_x(x):
        Rs = [np.eye(3)] * n
        for j, i in enumerate(free):
            Rs[i] = rodrigues(x[3 * j:3 * j + 3])
        fs = x[3 * len(free):] if focals == PER_IMAGE else np.full(n, x[-1])
        return np.stack(Rs), np.asarray(fs, dtype=np.float64)

    def res(x):
        Rs, fs = unpack_x(x)
        return bc._residuals(maps(shapes, Rs, fs, anchor), pairs, rows)

    x = np.concatenate([rotation_vector(np.asarray(Rs0[i])) for i in free] + [np.asarray(fs0, dtype=np.float64)[:n_f]])
    r = res(x)
    cost, lam, steps, J = float(r @ r), 1e-3, 0, None
    for _ in range(100):
        J = np.empty((len(r), len(x)))
        for k in range(len(x)):
            xh = x.copy()
            xh[k] += 1e-7 * (1.0 if k < 3 * len(free) else abs(x[k]))
            J[:, k] = (res(xh) - r) / (xh[k] - x[k])
        A, g = J.T @ J, J.T @ r
        took = None
        while lam <= 1e15 and took is None:
            step = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
            with np.errstate(all="ignore"):
                r2 = res(x + step)
            c2 = float(r2 @ r2)
            if np.isfinite(c2) and c2 < cost and (x + step)[3 * len(free):].min() > 0:
                took = (x + step, r2, c2)
            else:
                lam *= 10.0
        if took is None:
            break
        gain = cost - took[2]
        x, r, cost = took
        steps += 1
        lam = max(lam / 10.0, 1e-9)
        if gain <= 1e-15 * cost:
            break
    Rs, fs = unpack_x(x)
    sigma2 = cost / (len(r) - len(x))
    se = np.sqrt(sigma2 * np.diag(np.linalg.inv(J.T @ J))[3 * len(free):])
    return dict(Rs=Rs, fs=fs, cost=reference_cost(shapes, Rs, fs, pairs, matches, anchor), se=se if focals == PER_IMAGE else np.full(n, se[0]),
                steps=steps)
