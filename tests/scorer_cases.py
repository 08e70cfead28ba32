"""Shared by tests/test_scorer_walk_cpu.py and tests/test_scorer_walk_gpu.py: the inputs of the scorer-walk tests (K2 with several
hypotheses per wavefront, rwh_lab_tune RWH_TUNE_SCORE_HPW) and the oracle's answers for them.  Not a test module.

The yardstick everywhere is oracle/rwh_oracle.py: compute_loss(H.reshape(3, 3), X, Y, method) per hypothesis, its float32 errors
widened to float64 and compared with `< float(th)`; select_winner for the accept rules.

Two families of inputs:

  stress   points under one mild homography, 1 px noise, 40 % outliers, hypotheses from the oracle's own 4-point fits of random
           samples: many pairs lie near the threshold, and a dozen pairs outside every sample are moved onto it (`plant`), so
           the exact branch of the filter kernel runs at every position of a block of 7 hypotheses.  Used where the kernel's
           arithmetic is the oracle's by construction: 'fwd', and 'backward' / 'reproj' with numpy's inverses handed in (hinv=).

  cleared  for the kernel's own inverse and for K1's own H, which may sit an ulp from LAPACK's: no decision may hinge on one.
           The points fall into G groups, each under its own homography with translations >= 250 px apart; inside a group some
           pairs carry no noise, some 0 .. 1.2 px, some 4.5 .. 6 px.  Hypothesis i is group (i mod G)'s homography (translation
           moved by <= 0.3 px, or, batched, K1's fit of four noise-free pairs of that group), so every error stays far from
           th = 3 ('reproj': 6), seven consecutive hypotheses have seven different inlier sets, and i and i + G tie in count.
           CLEARANCE is what the CPU test holds every (hypothesis, pair) error to; an ulp of a float32 entry of H or inv(H)
           moves a projected point by about 1e-3 px at these coordinates.
"""
import numpy as np

from oracle import rwh_oracle as orc

METHODS = ("fwd", "backward", "reproj")
TH = 3.0
CLEARANCE = 0.25                       # px: the smallest |error - threshold| a cleared case may have
SINGLE_SIZES = (5, 64, 65, 185, 256, 257, 700)        # filter W = 1..4; 257 and 700: the chunked form
HPW_SINGLE = (1, 2, 6, 7, 8, 14, 15, 64)              # below / at / past a block of 7; bench.py's 14; past it; the knob's maximum
HPW_BATCHED = (1, 2, 7, 14, 15, 64)
K_SINGLE = 100                                        # a short last wave for every hpw > 1 above but 2 (that one: K = 3)
REGISTER_BATCH = (5, 64, 65, 185, 256)                # m_max = 256: the filter kernel, W = 4, shorter problems ride along
STREAMED_BATCH = (700, 30, 257)                       # m_max = 700: the general kernel with offsets, mask stride 11
K_PER = 23
K_PER_BENCH = (2100, 2102)                            # more than one argmax block per problem; 2102 % 14 != 0
WEIGHTS = (3, 2, 4, 6, 2, 8, 3, 4)                    # group sizes: group 3 larger than 0..2, group 5 the largest


def threshold(method):
    return 2.0 * TH if method == "reproj" else TH


def oracle_errors(H, X, Y, method):
    """[K, M] float32: compute_loss of every row of H ([K, 9] float32)."""
    with np.errstate(all="ignore"):
        return np.stack([orc.compute_loss(np.ascontiguousarray(h).reshape(3, 3), X, Y, method) for h in H])


def decisions(err, th):
    """(inlier bits [K, M] bool, counts [K] int64): the reference's `err < th` on float32 errors."""
    bits = err.astype(np.float64) < float(th)
    return bits, bits.sum(axis=1).astype(np.int64)


def unpack(words, m_bits):
    """uint64 / int64 mask words [K, W] -> bool [K, 64 * W]; bit i of word i // 64 is pair i."""
    w = np.ascontiguousarray(words).view(np.uint8).reshape(words.shape[0], -1)
    return np.unpackbits(w, axis=1, bitorder="little").astype(bool)


def clearance(err, th):
    """Smallest distance of a finite error from the threshold."""
    e = err.astype(np.float64)
    return float(np.abs(e[np.isfinite(e)] - float(th)).min())


# ---------------------------------------------------------------------------------------------------------------------------
# family A
# ---------------------------------------------------------------------------------------------------------------------------
def stress(M, K=K_SINGLE, seed=7):
    """-> dict(X, Y [2, M] float32, A, B [M, 2] float32, idx [K, 4], H [K, 9] float32: the oracle's 4-point fits)."""
    rng = np.random.default_rng([seed, M])
    Hs = np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]])
    A = rng.uniform(0, 2000, (M, 2))
    P = np.c_[A, np.ones(M)] @ Hs.T
    B = P[:, :2] / P[:, 2:] + rng.normal(0, 1.0, (M, 2))
    out = rng.random(M) < 0.4
    out[:4] = False                                    # (M = 5: keep a consensus)
    B[out] = rng.uniform(0, 2000, (int(out.sum()), 2))
    A, B = A.astype(np.float32), B.astype(np.float32)
    n_plant = min(12, max(0, M - 8))                   # the last pairs: in no sample, moved onto the threshold below
    idx = np.stack([rng.choice(M - n_plant, 4, replace=False) for _ in range(K)])
    X, Y = A.T.copy(), B.T.copy()
    H, _ = orc.ransac_table(X, Y, idx, th=TH, method="fwd")
    planted = []
    for t in range(n_plant):                           # hypotheses 0, 8, 16, ...: every position inside a block of 7
        p, method = M - n_plant + t, METHODS[t % 3]
        for hyp in range(8 * t % K, K, 7):             # (a wild H cannot hold a pair on the threshold: the next one 7 on)
            if plant(H[hyp].reshape(3, 3), X, Y, p, method):
                planted.append((hyp, p, method))
                break
    return dict(M=M, X=X, Y=Y, A=np.ascontiguousarray(X.T), B=np.ascontiguousarray(Y.T), idx=idx, H=H, planted=planted)


def plant(val, X, Y, p, method):
    """Move pair p so that its loss under `val` sits on the threshold: float32 bisection of one coordinate between a value whose
    loss is below the threshold and one 10 px away, until the two are neighbours -- inside the filter's band, whatever its width.
    In place; False (pair untouched) when `val` is too wild: the two ends do not straddle the threshold, or a float32 step
    of the coordinate moves the loss by 2^-10 px or more."""
    th = threshold(method)
    with np.errstate(all="ignore"):
        if method == "backward":
            T, base = X, orc.project_back(val, Y[:, p:p + 1])[:2, 0]
        else:
            T, base = Y, orc.project_fwd(val, X[:, p:p + 1])[:2, 0]
        if not np.isfinite(base).all() or np.abs(base).max() > 1e4:
            return False
        keep = T[:, p].copy()
        T[:, p] = base.astype(np.float32)

        def loss(v):
            T[0, p] = v
            return float(orc.compute_loss(val, X[:, p:p + 1], Y[:, p:p + 1], method)[0])
        lo, hi = np.float32(T[0, p]), np.float32(T[0, p] + np.float32(10.0))
        if not (loss(lo) < th <= loss(hi)):
            T[:, p] = keep
            return False
        while np.nextafter(lo, hi) != hi:
            mid = np.float32(0.5 * (np.float64(lo) + np.float64(hi)))
            if loss(mid) < th:
                lo = mid
            else:
                hi = mid
        if not (abs(loss(lo) - th) < 2.0 ** -10 and abs(loss(hi) - th) < 2.0 ** -10):
            T[:, p] = keep
            return False
        T[0, p] = lo if p % 2 else hi                  # odd pairs end just inside, even ones just outside
    return True


# ---------------------------------------------------------------------------------------------------------------------------
# family B
# ---------------------------------------------------------------------------------------------------------------------------
def n_groups(M):
    return 8 if M >= 64 else 4 if M >= 28 else 1


SEED = 11


def cleared(M, seed=SEED):
    """-> dict(X, Y, A, B, G, group [M], cls [M] (0 no noise, 1 <= 1.2 px, 2 4.5 .. 6 px), Hg [G, 3, 3] float64,
    corners [G][4] lists of noise-free pairs near the four corners of the field)."""
    assert M >= 5
    rng = np.random.default_rng([seed, M])
    G = n_groups(M)
    w = np.array(WEIGHTS[:G], dtype=np.float64)
    size = np.maximum(4, np.floor(M * w / w.sum()).astype(int))
    size[int(np.argmax(w))] += M - size.sum()
    assert size.sum() == M and size.min() >= 4
    Hg = np.empty((G, 3, 3))
    for g in range(G):
        Hg[g] = [[1 + rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), 250.0 * (g % 4)],
                 [rng.uniform(-0.01, 0.01), 1 + rng.uniform(-0.01, 0.01), 300.0 * (g // 4)],
                 [rng.uniform(-2e-6, 2e-6), rng.uniform(-2e-6, 2e-6), 1.0]]
    A, B, group, cls, corners = [], [], [], [], []
    box = [(0.0, 0.0), (900.0, 0.0), (900.0, 900.0), (0.0, 900.0)]          # 300 px boxes in the corners of a 1200 px field
    at = 0
    for g in range(G):
        n = int(size[g])
        rest = n - 4
        n_far = int(round(0.25 * rest))
        n_near = int(round(0.35 * rest))
        c = np.array([0] * (n - n_far - n_near) + [1] * n_near + [2] * n_far)
        src = rng.uniform(0, 1200, (n, 2))
        corners.append([[], [], [], []])
        for j in np.nonzero(c == 0)[0]:                 # noise-free pairs go round the corner boxes: samples stay well spread
            src[j] = np.array(box[j % 4]) + rng.uniform(0, 300, 2)
            corners[g][j % 4].append(at + int(j))
        p = np.c_[src, np.ones(n)] @ Hg[g].T
        dst = p[:, :2] / p[:, 2:]
        ang = rng.uniform(0, 2 * np.pi, n)
        mag = np.where(c == 0, 0.0, np.where(c == 1, rng.uniform(0, 1.2, n), rng.uniform(4.5, 6.0, n)))
        dst = dst + (mag * np.stack([np.cos(ang), np.sin(ang)])).T
        A.append(src); B.append(dst); group += [g] * n; cls += c.tolist()
        at += n
    A, B = np.concatenate(A).astype(np.float32), np.concatenate(B).astype(np.float32)
    return dict(M=M, seed=seed, G=G, A=A, B=B, X=A.T.copy(), Y=B.T.copy(), group=np.array(group), cls=np.array(cls), Hg=Hg, corners=corners)


def cleared_hypotheses(case, K, seed=13):
    """[K, 9] float32: hypothesis i = the homography of group i mod G with its translation moved by at most 0.3 px."""
    rng = np.random.default_rng([seed, case["M"], K])
    H = np.empty((K, 9), dtype=np.float32)
    for i in range(K):
        h = case["Hg"][i % case["G"]].copy()
        r, a = rng.uniform(0, 0.3), rng.uniform(0, 2 * np.pi)
        h[0, 2] += r * np.cos(a); h[1, 2] += r * np.sin(a)
        H[i] = h.reshape(9)
    return H


def cleared_samples(case, K):
    """[K, 4] int32 sample rows for K1: row i names one noise-free pair from each corner box of group i mod G (another choice
    every G rows where the group has more than four)."""
    idx = np.empty((K, 4), dtype=np.int32)
    for i in range(K):
        boxes = case["corners"][i % case["G"]]
        idx[i] = [b[(i // case["G"] + 3 * c) % len(b)] for c, b in enumerate(boxes)]
    return idx


def fitted(case, idx):
    """The oracle's H of every sample row (fit_minimal: float32 DLT matrix, LAPACK SVD)."""
    return np.stack([orc.fit_minimal(case["X"][:, r], case["Y"][:, r]).reshape(9) for r in idx]).astype(np.float32)


def group_need(case, counts, g=3):
    """A `need` that group g's hypotheses reach and no earlier hypothesis does (G = 1: the only group's)."""
    return int(counts[min(g, case["G"] - 1)])


def check_cleared(case, H, method, label):
    """The conditions a cleared case has to meet before a GPU result may be held to the oracle's decision with no tolerance;
    -> (measured clearance, bits, counts)."""
    th = threshold(method)
    err = oracle_errors(H, case["X"], case["Y"], method)
    assert np.isfinite(err).all(), label
    cl = clearance(err, th)
    assert cl >= CLEARANCE, (label, cl)
    bits, counts = decisions(err, th)
    G, K = case["G"], len(H)
    if case["M"] >= 64:
        for i in range(K - 6):                          # any 7 consecutive hypotheses: 7 different inlier sets
            assert len({bits[j].tobytes() for j in range(i, i + 7)}) == 7, (label, i)
    if G >= 4 and K >= G:
        assert len(set(counts.tolist())) >= 4, (label, sorted(set(counts.tolist())))
        assert counts[3] > counts[:3].max(), label      # `need` of group 3 is first met at hypothesis 3
        assert int(np.argmax(counts)) == int(np.argmax(WEIGHTS[:G])), label
    assert all(counts[i] == counts[i + G] for i in range(K - G)), label                  # the tie the accept rule has to break
    return cl, bits, counts


def concat(cases):
    """(pa, pb [total, 2] float32, offsets [P + 1] int32) of a batch of problems."""
    off = np.zeros(len(cases) + 1, dtype=np.int32)
    off[1:] = np.cumsum([c["M"] for c in cases])
    return np.concatenate([c["A"] for c in cases]), np.concatenate([c["B"] for c in cases]), off
