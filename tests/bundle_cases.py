"""The bundle rule (include/rwh.h: the normal-equation blocks of a bundle adjustment over a pair graph) restated in numpy -- a plain
loop over the rows in the stated order, vectorised over the 153 entries of a block --, the exact-rational model of one
correspondence with the forward rounding bound of the stated operation sequence, the generators (random edges, the GRID scene)
and the ctypes drivers of the host twin and the solver that tests/test_sequence_bundle_cpu.py and tests/test_sequence_bundle_gpu.py
share; for tests/test_bundle_loop_cpu.py and tests/test_bundle_loop_gpu.py the whole problem stated independently (the cost from the
geometry, its minimum by a plain numpy optimiser in another parameterisation), the far starts, the validity cases, the largest
launch and three warped views of one scene."""
from fractions import Fraction

import numpy as np

import projection_cases as pc

U = 2.0 ** -53
BLOCK, PARAMS, N_S = 153, 16, 136
OK, BEHIND, SINGULAR = 0, 1, 2
# the edge sizes of the parity tests: they cross the mask word (64), the staged chunk (128) and the four partials
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257, 600]


# ---- the rule ----
def fma(a, b, c):
    """a * b + c rounded once, through exact rationals.  With an operand that is not finite it is the plain float expression (the
    result is NaN or an infinity either way, no rounding is involved); where the exact result lies beyond the largest float64 it
    is the infinity of its sign, as IEEE 754 rounds it."""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        # the sign of a zero result: a zero product and a zero c of one sign keep it, everything else (an exact cancellation
        # included) is +0 in round-to-nearest; a rational has no -0, so this is stated here
        negative = (a == 0.0 or b == 0.0) and np.signbit(a) != np.signbit(b) and np.signbit(c)
        return -0.0 if negative else 0.0
    try:
        return float(exact)
    except OverflowError:
        return float("inf") if exact > 0 else float("-inf")


def entries():
    """The (i0, j0, i1, j1) of every block entry, as index arrays into a row's 34 values [J0 (16), J1 (16), r0, r1]."""
    quad = [(a, b, 16 + a, 16 + b) for a in range(16) for b in range(a, 16)]
    quad += [(k, 32, 16 + k, 33) for k in range(16)] + [(32, 32, 33, 33)]
    return tuple(np.array(col) for col in zip(*quad))


def row_values(T, a, b):
    """The 34 values of one correspondence, or None where it is not valid.  Written from the rule's general formula, a dp of three
    components for each of the 16 columns, zeros included."""
    T = np.asarray(T, dtype=np.float64).reshape(3, 3)
    at = np.array([np.float64(a[0]), np.float64(a[1]), 1.0])
    with np.errstate(all="ignore"):
        p = np.array([np.float64(fma(T[i, 1], at[1], T[i, 0] * at[0])) + T[i, 2] for i in range(3)])
        q = p[:2] / p[2]
    if not (np.isfinite(p[2]) and p[2] > 0 and np.isfinite(q).all()):
        return None
    dp = np.zeros((3, 16))
    for rho in range(3):
        for c in range(3):
            k = 3 * rho + c
            if k < 8:
                dp[:, k] = at[c] * T[:, rho]
                dp[rho, 8 + k] = -p[c]
    row = np.empty(34)
    row[:16] = (dp[0] - q[0] * dp[2]) / p[2]
    row[16:32] = (dp[1] - q[1] * dp[2]) / p[2]
    row[32], row[33] = q[0] - np.float64(b[0]), q[1] - np.float64(b[1])
    return row


def row_p2(T, a):
    """p2 of one correspondence as the rule computes it (the third component of `row_values`' p)."""
    T = np.asarray(T, dtype=np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        return np.float64(fma(T[2, 1], np.float64(a[1]), T[2, 0] * np.float64(a[0]))) + T[2, 2]


def mask_bit(words, i):
    return i < 64 * len(words) and bool((int(words[i >> 6]) >> (i & 63)) & 1)


def restate(pts_a, pts_b, offsets, masks, T):
    """-> (blocks float64 [E, 153], count, status) of the rule."""
    i0, j0, i1, j1 = entries()
    E = len(offsets) - 1
    blocks, count, status = np.zeros((E, BLOCK)), np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32)
    masks = np.asarray(masks).view(np.uint64)
    for e in range(E):
        part = np.zeros((4, BLOCK))
        for i in range(int(offsets[e + 1]) - int(offsets[e])):
            if not mask_bit(masks[e], i):
                continue
            row = row_values(T[e], pts_a[offsets[e] + i], pts_b[offsets[e] + i])
            if row is None:
                status[e] = BEHIND
                continue
            count[e] += 1
            part[i % 4] = part[i % 4] + (row[i0] * row[j0] + row[i1] * row[j1])
        blocks[e] = (part[0] + part[1]) + (part[2] + part[3])
    return blocks, count, status


def unpack(block):
    """-> (S symmetric [16, 16], g [16], c) of one block."""
    S = np.zeros((16, 16))
    S[np.triu_indices(16)] = block[:N_S]
    S = S + np.triu(S, 1).T
    return S, block[N_S:N_S + 16].copy(), float(block[152])


def transfers(Gs, pairs):
    """T_e = inv(G_d) @ G_s over its largest |entry|, as the Python layer makes it."""
    inv = np.linalg.inv(np.asarray(Gs, dtype=np.float64))
    T = np.stack([inv[d] @ np.asarray(Gs[s], dtype=np.float64) for s, d in pairs])
    return T / np.abs(T).reshape(len(pairs), 9).max(axis=1)[:, None, None]


# ---- one correspondence in exact rationals, and the forward bound of the stated operations ----
def exact_residual(T, a, b, delta_s, delta_d):
    """r of the rule in exact rationals for the updated maps: (I + D(delta_d))^-1 T (I + D(delta_s)) a~, dehomogenised, minus b."""
    F = Fraction

    def upd(delta):
        m = [[F(int(i == j)) for j in range(3)] for i in range(3)]
        for k in range(8):
            m[k // 3][k % 3] += delta[k]
        return m

    def mul(A, B):
        return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]

    def inverse(A):
        cof = [[A[(i + 1) % 3][(j + 1) % 3] * A[(i + 2) % 3][(j + 2) % 3] - A[(i + 1) % 3][(j + 2) % 3] * A[(i + 2) % 3][(j + 1) % 3]
                for j in range(3)] for i in range(3)]
        det = sum(A[0][j] * cof[0][j] for j in range(3))
        return [[cof[j][i] / det for j in range(3)] for i in range(3)]

    Tf = [[F(float(T[i][j])) for j in range(3)] for i in range(3)]
    M = mul(mul(inverse(upd(delta_d)), Tf), upd(delta_s))
    at = [F(float(a[0])), F(float(a[1])), F(1)]
    p = [sum(M[i][k] * at[k] for k in range(3)) for i in range(3)]
    return p[0] / p[2] - F(float(b[0])), p[1] / p[2] - F(float(b[1]))


def exact_jacobian(T, a, b, h=Fraction(1, 10 ** 30)):
    """J [2][16] in exact rationals by a central difference of `exact_residual` with step h."""
    J = [[None] * 16 for _ in range(2)]
    zero = [Fraction(0)] * 8
    for k in range(16):
        step = [h if j == k % 8 else Fraction(0) for j in range(8)]
        back = [-v for v in step]
        hi = exact_residual(T, a, b, step, zero) if k < 8 else exact_residual(T, a, b, zero, step)
        lo = exact_residual(T, a, b, back, zero) if k < 8 else exact_residual(T, a, b, zero, back)
        for c in range(2):
            J[c][k] = (hi[c] - lo[c]) / (2 * h)
    return J


class _Run(object):
    """A value of the stated operation sequence with its running forward error: `v` is what exact arithmetic gives, and the
    float64 the sequence computes lies within `e` of it.  Standard model: every rounded operation adds u times the magnitude of
    what it rounds; inherited errors propagate by the operation's own algebra (no first-order truncation)."""
    u = Fraction(1, 2 ** 53)

    def __init__(self, v, e=Fraction(0)):
        self.v, self.e = Fraction(v), Fraction(e)

    def _rounded(self, w, e_in):
        return _Run(w, e_in + self.u * (abs(w) + e_in))

    def mul(self, o):
        return self._rounded(self.v * o.v, abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e)

    def fma(self, o, c):
        return self._rounded(self.v * o.v + c.v, abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e + c.e)

    def add(self, o):
        return self._rounded(self.v + o.v, self.e + o.e)

    def sub(self, o):
        return self._rounded(self.v - o.v, self.e + o.e)

    def div(self, o):
        assert abs(o.v) > o.e
        w = self.v / o.v
        return self._rounded(w, (self.e + abs(w) * o.e) / (abs(o.v) - o.e))

    def neg(self):
        return _Run(-self.v, self.e)


def jacobian_bound(T, a):
    """-> (J exact [2][16] by the rule's formulas in rationals, bound [2][16]): the forward rounding bound of every J entry of the
    stated operation sequence, computed from the operands.  Where p has no cancellation it is at most gamma_k (|dp| + |q| |dp2|) /
    |p2| with k <= 15 rounded operations on the path (p0 and p2 three each, p2 twice more in q's and J's quotients, q, dp, the
    product, the difference, the quotient); with cancellation in p the same propagation gives the larger, still valid, figure."""
    R = _Run
    Tf = [[R(Fraction(float(T[i][j]))) for j in range(3)] for i in range(3)]
    at = [R(Fraction(float(a[0]))), R(Fraction(float(a[1]))), R(1)]
    p = [Tf[i][1].fma(at[1], Tf[i][0].mul(at[0])).add(Tf[i][2]) for i in range(3)]
    q = [p[0].div(p[2]), p[1].div(p[2])]
    zero = R(0)
    J = [[None] * 16 for _ in range(2)]
    for rho in range(3):
        for c in range(3):
            k = 3 * rho + c
            if k >= 8:
                continue
            dp = [Tf[i][rho] if c == 2 else at[c].mul(Tf[i][rho]) for i in range(3)]
            dd = [p[c].neg() if i == rho else zero for i in range(3)]
            for row in range(2):
                J[row][k] = dp[row].sub(q[row].mul(dp[2])).div(p[2])
                # the zero operands of delta_d: x - q * 0 and 0 - q * 0 are exact, so those operations add no rounding
                if rho == 2:
                    J[row][8 + k] = R(-(q[row].v * dd[2].v), q[row].mul(dd[2]).e).div(p[2])
                else:
                    J[row][8 + k] = dd[row].div(p[2]) if row == rho else zero
    return [[x.v for x in r] for r in J], [[x.e for x in r] for r in J]


# ---- generators ----
def random_maps(n, seed):
    """n maps into image 0's frame: shifts of a few dozen pixels with a small affine and perspective part."""
    rng = np.random.default_rng(seed)
    Gs = [np.eye(3)]
    for i in range(1, n):
        G = np.eye(3) + np.array([[0.04, 0.04, 0.0], [0.04, 0.04, 0.0], [2e-4, 2e-4, 0.0]]) * rng.uniform(-1, 1, (3, 3))
        G[0, 2], G[1, 2] = 35.0 * i + rng.uniform(-5, 5), rng.uniform(-12, 12)
        Gs.append(G)
    return np.stack(Gs)


def project(T, pts):
    z = np.asarray(T) @ np.vstack([pts.T.astype(np.float64), np.ones(len(pts))])
    return (z[:2] / z[2]).T


def size_list_case(seed=11, n=5, sizes=SIZES):
    """len(sizes) edges over n images, edge e with sizes[e] correspondences in [0, 160) x [0, 120), b = T a plus 0.5 px noise,
    float32 -> dict(pairs, T, pa, pb, offsets, sizes)."""
    rng = np.random.default_rng(seed)
    Gs = random_maps(n, seed)
    every = [(s, d) for d in range(n) for s in range(d + 1, n)]
    pairs = [every[e] if e < len(every) else every[e - len(every)][::-1] for e in range(len(sizes))]
    T = transfers(Gs, pairs)
    pa = (rng.uniform(0, 1, (sum(sizes), 2)) * [160.0, 120.0]).astype(np.float32)
    offsets = np.zeros(len(sizes) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(sizes)
    pb = np.empty_like(pa)
    for e in range(len(sizes)):
        o0, o1 = offsets[e], offsets[e + 1]
        pb[o0:o1] = (project(T[e], pa[o0:o1]) + rng.normal(0, 0.5, (o1 - o0, 2))).astype(np.float32)
    return dict(pairs=pairs, T=T, pa=pa, pb=pb, offsets=offsets, sizes=list(sizes), Gs=Gs)


def mask_sets(sizes, seed=3):
    """-> {"ones", "random", "short"}: int64 [E, words] mask rows.  "short" has one word fewer than the largest edge needs, so
    that edge's last rows are no inliers and nothing is read past the row."""
    words = max((max(sizes) + 63) // 64, 1)
    rng = np.random.default_rng(seed)
    random = rng.integers(0, 2 ** 63, (len(sizes), words), dtype=np.int64) ^ (rng.integers(0, 2, (len(sizes), words), dtype=np.int64) << 63)
    return {"ones": np.full((len(sizes), words), -1, dtype=np.int64), "random": random,
            "short": np.ascontiguousarray(random[:, :max(words - 1, 1)])}


def behind_case():
    """Edge 1 of three gets a transfer whose third row sends exactly one inlier (row 70: x = 500) to p2 <= 0."""
    c = size_list_case(seed=21, sizes=[65, 129, 5])
    pa, T = c["pa"].copy(), c["T"].copy()
    pa[c["offsets"][1] + 70] = [500.0, 10.0]
    T[1] = np.array([[1.0, 0.0, 3.0], [0.0, 1.0, -2.0], [-1.0 / 256.0, 0.0, 1.0]])
    T[1] /= np.abs(T[1]).max()
    masks = mask_sets(c["sizes"])["ones"]
    cleared = masks.copy()
    cleared[1, 1] &= ~np.int64(1 << (70 - 64))
    return c, pa, T, masks, cleared


GRID = dict(rows=2, cols=4, h=120, w=160, f=150.0, yaw=0.30, pitch=0.25, points=400, keep=30, sigma=0.5, seed=2007)
SNAKE = [(1, 0), (2, 1), (3, 2), (7, 3), (7, 6), (6, 5), (5, 4)]      # the chain 0-1-2-3-7-6-5-4 as stored pairs (s > d)


def grid_scene():
    """The 2 x 4 grid of views of a rotating camera: ground truth G_i = K R_0^T R_i K^-1, for every pair (s > d) up to 400 uniform
    points of image s kept where they land inside image d (pairs with >= 30 kept), float32, 0.5 px Gaussian noise on b, fixed
    seed -> dict(n, Gs, pairs, matches [(a, b)], sizes)."""
    g = GRID
    rng = np.random.default_rng(g["seed"])
    K = pc.camera((g["h"], g["w"]), g["f"])
    Rs = [pc.rotation(g["yaw"] * c, g["pitch"] * r) for r in range(g["rows"]) for c in range(g["cols"])]
    Gs = np.stack([K @ Rs[0].T @ R @ np.linalg.inv(K) for R in Rs])
    n = len(Rs)
    pairs, matches = [], []
    for d in range(n):
        for s in range(d + 1, n):
            a = rng.uniform(0, 1, (g["points"], 2)) * [g["w"] - 1.0, g["h"] - 1.0]
            z = np.linalg.inv(Gs[d]) @ Gs[s] @ np.vstack([a.T, np.ones(len(a))])
            b = (z[:2] / z[2]).T
            keep = (z[2] > 0) & (b[:, 0] >= 0) & (b[:, 0] <= g["w"] - 1) & (b[:, 1] >= 0) & (b[:, 1] <= g["h"] - 1)
            noise = rng.normal(0, g["sigma"], b.shape)
            if keep.sum() >= g["keep"]:
                pairs.append((s, d))
                matches.append((a[keep].astype(np.float32), (b + noise)[keep].astype(np.float32)))
    return dict(n=n, Gs=Gs, pairs=pairs, matches=matches, sizes=[len(a) for a, _ in matches])


def snake_start(lib, scene):
    """The chain's maps from pairwise least-squares homographies (rwh_host_refit over every match of each chain pair), walked by
    `sequence_graph` over the seven chain pairs -> Gs float64 [8, 3, 3]."""
    import homography as hg
    Hs = []
    for pr in SNAKE:
        a, b = scene["matches"][scene["pairs"].index(pr)]
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        words = np.full((len(a) + 63) // 64, -1, dtype=np.int64)
        H, st = np.empty(9), np.zeros(1, dtype=np.int32)
        assert lib.rwh_host_refit(a.ctypes.data, b.ctypes.data, len(a), words.ctypes.data, H.ctypes.data, st.ctypes.data) == 0 and st[0] == 0
        Hs.append(H.reshape(3, 3))
    sizes = [len(scene["matches"][scene["pairs"].index(pr)][0]) for pr in SNAKE]
    Gs, accepted, tree = hg.sequence_graph(scene["n"], SNAKE, Hs, sizes, sizes, anchor=0)
    assert accepted.all() and len(tree) == 7
    return Gs


def concatenated(matches):
    pa = np.ascontiguousarray(np.concatenate([a for a, _ in matches]), dtype=np.float32)
    pb = np.ascontiguousarray(np.concatenate([b for _, b in matches]), dtype=np.float32)
    offsets = np.zeros(len(matches) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(a) for a, _ in matches])
    return pa, pb, offsets


# ---- the host twins ----
def rule_host_blocks(lib, entry, block, record, pa, pb, offsets, masks, rec):
    """The host twin `entry` of a rule with blocks of `block` values and records of `record` -> (status of the call, blocks, count,
    status); the three outputs sit between 64-byte canaries that are checked here."""
    E = len(offsets) - 1
    pa, pb = np.ascontiguousarray(pa, dtype=np.float32), np.ascontiguousarray(pb, dtype=np.float32)
    offsets, masks = np.ascontiguousarray(offsets, dtype=np.int32), np.ascontiguousarray(masks).view(np.uint64)
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(E, record)
    sizes = [E * block * 8, E * 4, E * 4]
    bufs = [np.full(sz + 128, 0xA5, dtype=np.uint8) for sz in sizes]
    st = getattr(lib, entry)(pa.ctypes.data, pb.ctypes.data, offsets.ctypes.data, E, masks.ctypes.data, masks.shape[1], rec.ctypes.data,
                             bufs[0][64:].ctypes.data, bufs[1][64:].ctypes.data, bufs[2][64:].ctypes.data)
    for buf in bufs:
        assert (buf[:64] == 0xA5).all() and (buf[-64:] == 0xA5).all(), "a byte outside an output was written"
    return (st, bufs[0][64:-64].view(np.float64).reshape(E, block).copy(), bufs[1][64:-64].view(np.int32).copy(),
            bufs[2][64:-64].view(np.int32).copy())


def host_blocks(lib, pa, pb, offsets, masks, T):
    """rwh_host_bundle_blocks through `rule_host_blocks`."""
    return rule_host_blocks(lib, "rwh_host_bundle_blocks", BLOCK, 9, pa, pb, offsets, masks, T)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def rule_device_blocks(rule, block, pa, pb, offsets, masks, rec):
    """kernels.<rule>_blocks into outputs that sit between guard words -> (blocks, count, status) in numpy; the guards are checked
    and the packed result, taken apart by kernels.<rule>_split, is checked against the three outputs."""
    import torch
    from ransac_with_homography_amd import kernels
    E = len(offsets) - 1
    blocks_buf = torch.full((E * block + 16,), -7.0, dtype=torch.float64, device="cuda")
    tail_buf = torch.full((2, E + 32), -7, dtype=torch.int32, device="cuda")
    out = (blocks_buf[8:-8].view(E, block), tail_buf[0, 16:-16], tail_buf[1, 16:-16])
    packed = getattr(kernels, rule + "_blocks")(torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda(), torch.from_numpy(offsets).cuda(),
                                                torch.from_numpy(np.ascontiguousarray(masks).view(np.int64)).cuda(), rec, out=out)
    flat, tail = blocks_buf.cpu().numpy(), tail_buf.cpu().numpy()
    assert (flat[:8] == -7.0).all() and (flat[-8:] == -7.0).all(), "a value outside the blocks was written"
    assert (tail[:, :16] == -7).all() and (tail[:, -16:] == -7).all(), "a word outside count or status was written"
    blocks, count, status = getattr(kernels, rule + "_split")(packed.cpu().numpy())
    assert _same_bits(blocks, flat[8:-8].reshape(E, block)) and np.array_equal(count, tail[0, 16:-16]) and np.array_equal(status, tail[1, 16:-16])
    return blocks, count, status


def device_blocks(pa, pb, offsets, masks, T):
    """kernels.bundle_blocks through `rule_device_blocks`."""
    return rule_device_blocks("bundle", BLOCK, pa, pb, offsets, masks, T)


def host_step(lib, n, anchor, pairs, blocks, lam):
    """rwh_host_bundle_step -> (status of the call, delta [n, 8], step status), delta between canaries."""
    edges = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    blocks = np.ascontiguousarray(blocks, dtype=np.float64)
    buf, status = np.full(8 * n + 16, -7.0), np.full(1, -1, dtype=np.int32)
    st = lib.rwh_host_bundle_step(n, anchor, edges.ctypes.data, len(edges), blocks.ctypes.data, float(lam), buf[8:].ctypes.data,
                                  status.ctypes.data)
    assert (buf[:8] == -7.0).all() and (buf[-8:] == -7.0).all()
    return st, buf[8:-8].reshape(n, 8).copy(), int(status[0])


def assemble(n, anchor, pairs, blocks, lam):
    """The step's system in numpy: -> (A with lambda * diag added, g, keep) over the parameters that are not the anchor's."""
    A, g = np.zeros((8 * n, 8 * n)), np.zeros(8 * n)
    for (s, d), blk in zip(pairs, blocks):
        S, ge, _ = unpack(blk)
        at = np.concatenate([np.arange(8 * s, 8 * s + 8), np.arange(8 * d, 8 * d + 8)])
        A[np.ix_(at, at)] += S
        g[at] += ge
    keep = np.array([i for i in range(8 * n) if i // 8 != anchor])
    A, g = A[np.ix_(keep, keep)], g[keep]
    A[np.diag_indices_from(A)] += lam * np.diag(A)
    return A, g, keep


def solve_bound(A, x):
    """The backward-error bound of a Cholesky solve, as tests/gain_cases.residual_bound: 4 n^2 u |A|_inf |x|_inf."""
    n = len(x)
    return 4 * n * n * U * np.abs(A).sum(axis=1).max() * np.abs(x).max()


# ---- the whole problem stated independently: the cost from the geometry, its minimum by a plain optimiser ----
def _inlier_rows(matches, masks):
    """[(a, b)] in float64, each edge's rows cut down to those whose mask bit is set (masks None: every row)."""
    out = []
    words = None if masks is None else np.ascontiguousarray(masks).view(np.uint64)
    for e, (a, b) in enumerate(matches):
        a, b = np.asarray(a, dtype=np.float64).reshape(-1, 2), np.asarray(b, dtype=np.float64).reshape(-1, 2)
        if words is not None:
            keep = np.array([mask_bit(words[e], i) for i in range(len(a))], dtype=bool)
            a, b = a[keep], b[keep]
        out.append((a, b))
    return out


def _residuals(Gs, pairs, rows):
    """Every r = dehomogenised(inv(G_d) G_s a~) - b of the kept rows, one flat vector."""
    inv = np.linalg.inv(Gs)
    return np.concatenate([(project(inv[d] @ Gs[s], a) - b).ravel() for (s, d), (a, b) in zip(pairs, rows)])


def reference_cost(Gs, pairs, matches, masks=None):
    """The bundle cost at Gs from the geometry alone, float64 numpy: T = inv(G_d) @ G_s, a projected, b subtracted, the squares
    summed over the rows whose mask bit is set.  No J, no blocks, no scaling of T (the projection does not see it)."""
    r = _residuals(np.asarray(Gs, dtype=np.float64), pairs, _inlier_rows(matches, masks))
    return float(np.sum(r * r))


def reference_optimum(Gs0, pairs, matches, anchor, masks=None):
    """The minimum of `reference_cost` by Levenberg-Marquardt in plain numpy -> (Gs, cost).  Another parameterisation than the
    library's: the 8 entries of every G_i / G_i[2][2] but the anchor's, global, not the local I + D(delta); the Jacobian by
    forward differences of the residual vector (step 1e-7 of the entry's size, floored at 1e-7, 1e-11 on the perspective row).
    The optimiser only has to FIND the minimum; what it returns is judged by `reference_cost`."""
    rows = _inlier_rows(matches, masks)
    Gs0 = np.asarray(Gs0, dtype=np.float64)
    n = len(Gs0)
    free = [i for i in range(n) if i != anchor]
    floor = np.tile([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1e-4, 1e-4], len(free))

    def unpack_x(x):
        Gs = np.empty((n, 3, 3))
        Gs[anchor] = np.eye(3)
        for j, i in enumerate(free):
            Gs[i] = np.append(x[8 * j:8 * j + 8], 1.0).reshape(3, 3)
        return Gs

    def res(x):
        return _residuals(unpack_x(x), pairs, rows)

    x = np.concatenate([(Gs0[i] / Gs0[i, 2, 2]).reshape(9)[:8] for i in free])
    r = res(x)
    cost, lam = float(r @ r), 1e-3
    for _ in range(100):
        J = np.empty((len(r), len(x)))
        for k in range(len(x)):
            h = 1e-7 * max(abs(x[k]), floor[k])
            xh = x.copy()
            xh[k] += h
            J[:, k] = (res(xh) - r) / (xh[k] - x[k])
        A, g = J.T @ J, J.T @ r
        took = None
        while lam <= 1e15 and took is None:
            try:
                step = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
            except np.linalg.LinAlgError:
                step = None
            if step is not None:
                with np.errstate(all="ignore"):
                    r2 = res(x + step)
                c2 = float(r2 @ r2)
                if np.isfinite(c2) and c2 < cost:
                    took = (x + step, r2, c2)
            if took is None:
                lam *= 10.0
        if took is None:
            break
        gain = cost - took[2]
        x, r, cost = took
        lam = max(lam / 10.0, 1e-9)
        if gain <= 1e-15 * cost:
            break
    Gs = unpack_x(x)
    return Gs, reference_cost(Gs, pairs, matches, masks)


# The far starts of the loop tests: (seed, persp) of `far_start`, with what the host loop does from each of them on GRID from the
# chain start (steps tried, steps accepted), counted where this was written; tests/test_bundle_loop_cpu.py asserts the counts.
FAR_ONE_REJECT = dict(seed=3, persp=0.003, tried=8, accepted=7)
FAR_MANY_REJECTS = dict(seed=35, persp=0.0025, tried=27, accepted=6)


def far_start(start, seed, persp):
    """`start` with every map but the first multiplied from the right by I + [[.1, .1, 20], [.1, .1, 20], [persp, persp, 0]] *
    uniform(-1, 1): far enough that Levenberg-Marquardt rejects steps on the way back."""
    rng = np.random.default_rng(seed)
    spread = np.array([[0.1, 0.1, 20.0], [0.1, 0.1, 20.0], [persp, persp, 0.0]])
    out = [np.array(start[0], dtype=np.float64)]
    for G in start[1:]:
        out.append(np.asarray(G, dtype=np.float64) @ (np.eye(3) + spread * rng.uniform(-1, 1, (3, 3))))
    return np.stack(out)


def reframed(Gs, anchor):
    """The same maps expressed in image `anchor`'s frame: inv(G_anchor) @ G_i, the anchor's the identity exactly."""
    Gs = np.asarray(Gs, dtype=np.float64)
    out = np.stack([np.linalg.inv(Gs[anchor]) @ G for G in Gs])
    out[anchor] = np.eye(3)
    return out


# ---- the validity test from every side ----
VALIDITY_ROW = 130          # of edge 1 (200 rows): past the first staged chunk, row 2 of the second, so wave 2's partial


def validity_cases():
    """Three edges of 70, 200 and 9 rows, every row an inlier; row 130 of edge 1 made invalid in eight ways -> (c, masks, cleared,
    [(name, pa, T)]): c the undisturbed case, `cleared` the masks without that row's bit.  Coordinate cases keep c's transfers:
    T[1][2][0] < 0 (asserted), so the float32-huge x gives a large negative p2.  Transfer cases give edge 1 the transfer
    [[1, 0, 1/2], [0, 1, -1/4], [1/512, 1/16, t]]: p2 = x / 512 + y / 16 + t is positive on every other row (x, y >= 0, not both
    0: asserted), and at the row's (x, y) = (-512, 16) both products are exact and cancel, so p2 = t exactly."""
    c = size_list_case(seed=21, sizes=[70, 200, 9])
    at = int(c["offsets"][1]) + VALIDITY_ROW
    masks = mask_sets(c["sizes"])["ones"]
    cleared = masks.copy()
    cleared[1, VALIDITY_ROW >> 6] &= ~np.int64(1 << (VALIDITY_ROW & 63))
    assert c["T"][1][2, 0] < 0
    others = np.delete(c["pa"][c["offsets"][1]:c["offsets"][2]], VALIDITY_ROW, axis=0)
    assert (others >= 0).all() and (others.sum(axis=1) > 0).all()

    def transfer(t):
        return np.array([[1.0, 0.0, 0.5], [0.0, 1.0, -0.25], [1.0 / 512.0, 1.0 / 16.0, t]])

    listed = [("x nan", (np.nan, None), None), ("x +inf", (np.inf, None), None), ("y -inf", (None, -np.inf), None),
              ("x 3e38", (np.float32(3e38), None), None),
              ("p2 +0", (-512.0, 16.0), transfer(0.0)),                    # (+1) + (-1) = +0, + 0 = +0
              ("p2 -0", (-0.0, -0.0), transfer(-0.0)),                     # (-0) + (-0) = -0 twice: every term is a negative zero
              ("p2 negative", (-512.0, 8.0), transfer(0.0)),               # -1 + 1/2
              ("p2 denormal", (-512.0, 16.0), transfer(2.0 ** -1070))]     # p2 = 2^-1070 > 0 and p0 = -511.5: q0 overflows
    cases = []
    for name, (x, y), T1 in listed:
        pa, T = c["pa"].copy(), c["T"].copy()
        if x is not None:
            pa[at, 0] = x
        if y is not None:
            pa[at, 1] = y
        if T1 is not None:
            T[1] = T1
        cases.append((name, pa, T))
    return c, masks, cleared, cases


# ---- the launch's two ends ----
LAUNCH_SIZES = [(0, 1, 2, 3, 4, 5, 7, 64, 65)[e % 9] for e in range(2016)]


def launch_case():
    """The largest launch: 2016 edges (every pair of 64 images), 33 824 rows, the "random" masks -> (c, masks)."""
    c = size_list_case(seed=5, n=64, sizes=LAUNCH_SIZES)
    return c, mask_sets(c["sizes"])["random"]


def single_edge(c, masks, e):
    """Edge e of a case as a launch of its own: its rows, offsets from 0, its mask row, its transfer."""
    o0, o1 = int(c["offsets"][e]), int(c["offsets"][e + 1])
    return (np.ascontiguousarray(c["pa"][o0:o1]), np.ascontiguousarray(c["pb"][o0:o1]), np.array([0, o1 - o0], dtype=np.int32),
            np.ascontiguousarray(masks[e:e + 1]), c["T"][e:e + 1])


# ---- three views with real residuals ----
VIEW_SHAPE, VIEW_SHIFTS = (180, 290), [(3.3, 9.6), (48.7, 7.3), (139.2, 11.8)]


def warped_views(seed=12):
    """Three views of sequence_cases.scene() that are no integer shifts of it: view i shows the scene under M_i =
    sc.homography(rng, tx, ty, affine=0.01, persp=2e-5) (view pixel -> scene pixel; views 45.4 and 90.5 px apart, so that the outer
    pair still shares half a view: with 90 px twice it has too few matches to be accepted), sampled bilinearly in float64 and
    rounded to uint8; every view lies inside the scene (asserted) -> (views, Gs): Gs[i] = inv(M_0) @ M_i, the ground truth maps
    into view 0's frame.  On the host twins of the extractor and the matcher the pairs (1, 0), (2, 0), (2, 1) have 109, 100 and 104
    matches, 87, 59 and 77 of them within 5 px of the truth; acceptance needs more than 40.7, 38.0 and 39.2."""
    import sequence_cases as sc
    scene = sc.scene().astype(np.float64)
    rng = np.random.default_rng(seed)
    h, w = VIEW_SHAPE
    yy, xx = np.mgrid[0:h, 0:w]
    views, Ms = [], []
    for tx, ty in VIEW_SHIFTS:
        M = sc.homography(rng, tx, ty, affine=0.01, persp=2e-5)
        z = M @ np.stack([xx.ravel(), yy.ravel(), np.ones(h * w)]).astype(np.float64)
        x, y = z[0] / z[2], z[1] / z[2]
        assert x.min() >= 0 and y.min() >= 0 and x.max() <= scene.shape[1] - 1 and y.max() <= scene.shape[0] - 1
        x0, y0 = np.minimum(np.floor(x).astype(int), scene.shape[1] - 2), np.minimum(np.floor(y).astype(int), scene.shape[0] - 2)
        fx, fy = (x - x0)[:, None], (y - y0)[:, None]
        img = ((scene[y0, x0] * (1 - fx) + scene[y0, x0 + 1] * fx) * (1 - fy) + (scene[y0 + 1, x0] * (1 - fx) + scene[y0 + 1, x0 + 1] * fx) * fy)
        views.append(np.ascontiguousarray(np.rint(img).astype(np.uint8).reshape(h, w, 3)))
        Ms.append(M)
    Gs = np.stack([np.linalg.inv(Ms[0]) @ M for M in Ms])
    Gs[0] = np.eye(3)
    return views, Gs
