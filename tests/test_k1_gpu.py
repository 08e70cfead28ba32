"""K1 (`dlt4_kernel`) itself on the MI355X against the exact null vector and the flag rules (tests/k1_cases.py; the numbers it is
measured against are fixed on the CPU by tests/test_k1_cpu.py):

  accuracy      per family, every row the settle rule keeps on the device (no REPEATED / SINGULAR / DEGENERATE) has an exact H, that
                H lies inside the row's box (IV_DELTA0 unflagged, IV_DELTA1 for ILLCOND), the bit-identical share is the
                emulation's minus at most one percentage point (recip and the order of operations move only the last bits of a
                float64, which decides a float32 rounding only on a boundary), and entry 8 is exactly 1;
  flags         REPEATED is the integer rule on every row; away from the borderline rows the whole byte is the emulation's, without
                and with the determinant test of the searches that invert; the edge table;
  launch edges  K = 1 .. 1000 into caller-owned buffers one wave longer than needed: rows as in the K = 1024 launch, nothing written
                past 9 K floats / K flags;
  batched mode  the index bound is the problem's own m (the existing batched tests never pass an index that is valid for a larger
                problem of the batch only)."""
import ctypes

import numpy as np
import pytest

import k1_cases as kc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    from ransac_with_homography_amd import _lib
    return _lib.require_gpu()  # raises (test error, not skip) when the HIP path is unavailable


def _k1(gpu, A, B, idx, near_singular=False):
    """One launch of K1 -> (H float32 [K, 9], flags uint8 [K]) on the host: rwh_dlt4_batched, or -- near_singular -- the K1 launch
    of rwh_ransac_search under 'reproj', which raises ILLCOND | DEGENERATE on nearly singular H too."""
    from ransac_with_homography_amd import kernels
    pa, pb = torch.from_numpy(np.array(A, np.float32)).to(gpu), torch.from_numpy(np.array(B, np.float32)).to(gpu)
    d_idx = torch.from_numpy(np.array(idx, np.int32)).to(gpu)
    if not near_singular:
        H, flags = kernels.dlt4_batched(pa, pb, d_idx)
        return H.cpu().numpy(), flags.cpu().numpy()
    ws = kernels.SearchWorkspace(len(idx), A.shape[0], gpu)
    kernels.ransac_search(pa, pb, d_idx, 5.0, "reproj", 1 << 30, ws)
    return ws.H.cpu().numpy(), ws.flags.cpu().numpy()


@pytest.mark.parametrize("name", kc.FAMILIES)
def test_kernel_against_exact_null_vector(gpu, name):
    from ransac_with_homography_amd.ransac import IV_DELTA0, IV_DELTA1
    A, B, idx = kc.family(name)
    ex = kc.family_exact(name)
    H, flags = _k1(gpu, A, B, idx)
    C = kc.coord_scale(A)
    rows = np.flatnonzero((flags & kc.HOST_BITS) == 0)
    assert len(rows) >= 200
    assert all(ex[r] is not None for r in rows), [int(r) for r in rows if ex[r] is None]
    frac = np.array([kc.box_fraction(ex[r], H[r], flags[r], C, IV_DELTA0, IV_DELTA1) for r in rows])
    equal = sum(np.array_equal(ex[r].view(np.uint32), H[r].view(np.uint32)) for r in rows)
    emu_equal, emu_rows = kc.EMULATION_BIT_EQUAL[name]
    bl = kc.borderline(kc.family_emulation(name, True)[2], True)
    print("k1_exact %-14s bit-identical %d / %d = %.4f (emulation %d / %d = %.4f)  worst distance %.3g of the box (row %d, flags %d)"
          "  borderline %d / %d" % (name, equal, len(rows), equal / len(rows), emu_equal, emu_rows, emu_equal / emu_rows, frac.max(),
                                    rows[frac.argmax()], flags[rows[frac.argmax()]], int(bl.sum()), len(bl)))
    assert (frac <= 1.0).all(), (name, rows[frac > 1.0].tolist(), frac.max())
    assert equal / len(rows) >= emu_equal / emu_rows - 0.01, (name, equal, len(rows))
    finite = np.isfinite(H).all(axis=1)
    assert finite[rows].all() and np.all(H[finite, 8] == 1.0)


@pytest.mark.parametrize("near_singular", [False, True])
@pytest.mark.parametrize("name", kc.FAMILIES)
def test_kernel_flags(gpu, name, near_singular):
    A, B, idx = kc.family(name)
    H, flags = _k1(gpu, A, B, idx, near_singular)
    He, fe, inter = kc.family_emulation(name, near_singular)
    assert np.array_equal((flags & kc.REPEATED) != 0, kc.repeated_rule(idx, A.shape[0]))
    firm = ~kc.borderline(inter, near_singular)
    assert firm.mean() >= 0.98
    bad = np.flatnonzero(firm & (flags != fe))
    assert bad.size == 0, (name, near_singular, [(int(r), int(flags[r]), int(fe[r]), inter["ratios"][r].tolist(), float(inter["det_ratio"][r]))
                                                 for r in bad[:5]])
    # SINGULAR is what it says: set exactly on the rows with a non-finite entry
    assert np.array_equal((flags & kc.SINGULAR) != 0, ~np.isfinite(H).all(axis=1))


def test_edge_table(gpu):
    pa, pb, rows = kc.edge_table()
    idx, twins = kc.edge_launch(rows)
    H, flags = _k1(gpu, pa, pb, idx)
    print("edge table flags:", {r[0]: int(f) for r, f in zip(rows, flags)})
    kc.check_edge_rows(rows, twins, H, flags)
    assert np.array_equal((flags & kc.REPEATED) != 0, kc.repeated_rule(idx, len(pa)))


def test_launch_edges_write_nothing_past_the_end(gpu):
    """rwh_dlt4_batched directly: a partial last wave computes its dead lanes on point 0 and stages the wave's store through LDS, cut
    at 9 x (live lanes): the live rows are those of the full launch and every byte behind them keeps the caller's pattern."""
    from ransac_with_homography_amd import _lib
    lib = _lib.load()
    A, B, idx = kc.launch_edge_table()
    pa, pb, d_idx = torch.from_numpy(A.copy()).to(gpu), torch.from_numpy(B.copy()).to(gpu), torch.from_numpy(idx.copy()).to(gpu)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def launch(K):
        h = torch.full((9 * K + 64 * 9,), -7.25, dtype=torch.float32, device=gpu)
        f = torch.full((K + 64,), 0xA5, dtype=torch.uint8, device=gpu)
        assert lib.rwh_dlt4_batched(ptr(pa), ptr(pb), A.shape[0], ptr(d_idx), K, ptr(h), ptr(f), _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        return h.cpu().numpy(), f.cpu().numpy()

    Hfull, ffull = launch(1024)
    assert (Hfull[:9 * 1024] != np.float32(-7.25)).all() and (ffull[:1024] != 0xA5).all()
    for K in (1, 63, 64, 65, 127, 129, 1000):
        h, f = launch(K)
        assert np.array_equal(h[:9 * K].view(np.uint32), Hfull[:9 * K].view(np.uint32)), K
        assert np.array_equal(f[:K], ffull[:K]), K
        assert (h[9 * K:] == np.float32(-7.25)).all() and (f[K:] == 0xA5).all(), K


def test_batched_index_bound_is_the_problems_own(gpu):
    """rwh_ransac_batched(idx=): three problems of 7, 64 and 200 correspondences; one hypothesis of each carries an index that is
    valid for the largest problem (m_max) only.  Every problem equals the single launch on its slice, and the out-of-range rows are
    REPEATED there."""
    from ransac_with_homography_amd import kernels
    U, V, _ = kc.family("uniform")
    sizes, K = [7, 64, 200], 70
    A, B = (np.concatenate([P[:7], P[10:74], P[50:250]]) for P in (U, V))
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rng = np.random.default_rng(977)
    idx = np.stack([rng.integers(0, m, (K, 4)) for m in sizes]).astype(np.int32)
    idx[0, 5] = (1, 2, 100, 3)          # >= 7, valid for the problem of 200
    idx[0, 66] = (7, 1, 2, 3)           # == m of its own problem
    idx[1, 64] = (0, 1, 2, 199)         # >= 64
    idx[2, 69] = (200, 5, 6, 7)         # == m_max
    assert A.shape == (offs[-1], 2)
    pa, pb = torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu)
    ws = kernels.BatchWorkspace(3, K, max(sizes), gpu)
    needs = torch.tensor([1 << 30] * 3, dtype=torch.int32, device=gpu)
    kernels.ransac_batched(pa, pb, torch.from_numpy(offs).to(gpu), needs, 5.0, "fwd", ws, idx=torch.from_numpy(idx).to(gpu))
    Hb, fb = ws.H.cpu().numpy(), ws.flags.cpu().numpy()
    for p, m in enumerate(sizes):
        o = int(offs[p])
        H, flags = _k1(gpu, A[o:o + m], B[o:o + m], idx[p])
        assert np.array_equal(Hb[p].view(np.uint32), H.view(np.uint32)) and np.array_equal(fb[p], flags), p
        assert np.array_equal((flags & kc.REPEATED) != 0, kc.repeated_rule(idx[p], m)), p
        Hc, fc = _k1(gpu, A[o:o + m], B[o:o + m], kc.clamp_idx(idx[p], m))
        assert np.array_equal(Hc.view(np.uint32), H.view(np.uint32)) and np.array_equal(fc | (flags & kc.REPEATED), flags), p
    assert fb[0, 5] & fb[0, 66] & fb[1, 64] & fb[2, 69] & kc.REPEATED
