"""Edge blocks of the batch form of the uint8 bilinear warp (warp_rgb8_fast8<unsigned char, S, true>, body fast8mb_body): blocks with
patches on the border of the source, or wholly outside it, walk their tile through the frames of the group with ONE clamped block
window, per-pixel zero weights and clamped tap addresses instead of running the one-frame body frame by frame.  Only blocks with a
horizon wave, or whose window does not fit or reaches the last two source rows, still do that.

The yardstick is the one-frame kernel, which rwh_lab_tune(RWH_TUNE_WARP_FRAMES, 1) forces (and which the rest of the suite ties to
the oracle): the host's choice (knob 0) must equal it BIT FOR BIT.  Every case uses 24-26 frames, checks that the reference is not
all zeros, releases the knobs whatever happens and launches the batch form twice (a race shows differently from launch to launch)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H_S = np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]])
SRC_H, SRC_W, FRAMES = 333, 517, 26


@pytest.fixture(scope="module")
def gpu():
    from ransac_with_homography_amd import _lib
    return _lib.require_gpu()  # raises (test error, not skip) when the HIP path is unavailable


@pytest.fixture(scope="module")
def frames(gpu):
    rng = np.random.default_rng(36)
    return torch.from_numpy(rng.integers(0, 256, (FRAMES, SRC_H, SRC_W, 3), dtype=np.uint8)).to(gpu)


def _tune(knob, value):
    from ransac_with_homography_amd import _lib
    assert _lib.load().rwh_lab_tune(knob, int(value)) == 0


def _both(src, inv, grid, bound, rows=None, shape=0, launches=2):
    """(forced one-frame kernel, the host's choice x launches) of one warp call; the knobs are released whatever happens."""
    from ransac_with_homography_amd import _lib, kernels
    try:
        _tune(_lib.RWH_TUNE_WARP_SHAPE, shape)
        _tune(_lib.RWH_TUNE_WARP_FRAMES, 1)
        ref = kernels.warp_backward(src, inv, grid, bound, "bilinear", torch.uint8, zero_origin=False, rows=rows)
        _tune(_lib.RWH_TUNE_WARP_FRAMES, 0)
        got = [kernels.warp_backward(src, inv, grid, bound, "bilinear", torch.uint8, zero_origin=False, rows=rows) for _ in range(launches)]
    finally:
        _tune(_lib.RWH_TUNE_WARP_FRAMES, 0)
        _tune(_lib.RWH_TUNE_WARP_SHAPE, 0)
    return ref, got


def _check(ref, got, what):
    assert ref.any(), what                                   # (a reference of zeros would compare equal to anything unwritten)
    assert len(got) == 2, what
    for g in got:
        assert torch.equal(g, ref), (what, int((g != ref).sum()))


def _source_coords(inv, grid_x, grid_y):
    """Source coordinates (sx, sy, W) of the output grid points (grid_x[j], grid_y[i]), float64."""
    x, y = np.meshgrid(np.asarray(grid_x, dtype=np.float64), np.asarray(grid_y, dtype=np.float64))
    X = inv[0, 0] * x + inv[0, 1] * y + inv[0, 2]
    Y = inv[1, 0] * x + inv[1, 1] * y + inv[1, 2]
    W = inv[2, 0] * x + inv[2, 1] * y + inv[2, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return X / W, Y / W, W


def _edge_grid():
    """Overhangs the 333 x 517 source by more than one 128 x 16 tile on every side: all four edges, four corners, and blocks that map
    wholly outside."""
    from ransac_with_homography_amd import kernels
    return kernels.Grid(-300, 799, 1100, -60, 419, 480)


@pytest.mark.parametrize("shape", [6, 7, 0])
def test_all_edges_corners_and_outside_blocks(gpu, frames, shape):
    inv = np.linalg.inv(H_S)
    sx, sy, _ = _source_coords(inv, [-300 + 128, 799 - 128], [-60 + 16, 419 - 16])      # one tile in from each grid corner
    assert sx[0, 0] < 0 and sy[0, 0] < 0 and sx[-1, -1] > SRC_W - 1 and sy[-1, -1] > SRC_H - 1
    ref, got = _both(frames[:25], inv, _edge_grid(), (SRC_H, SRC_W), shape=shape)
    _check(ref, got, shape)


@pytest.mark.parametrize("shape", [6, 7, 0])
def test_bound_smaller_than_the_source(gpu, frames, shape):
    """Scan mode: the valid region ends inside the image, so the clamp must use `bound`, not the source size."""
    ref, got = _both(frames[:25], np.linalg.inv(H_S), _edge_grid(), (200, 400), shape=shape)
    _check(ref, got, shape)
    full, _ = _both(frames[:25], np.linalg.inv(H_S), _edge_grid(), (SRC_H, SRC_W), shape=shape, launches=2)
    assert not torch.equal(full, ref)                        # (the bound really cuts pixels away)


def test_exact_integers_on_the_last_row_and_column(gpu):
    """Identity, output grid = the pixel grid of a 64 x 256 source: s == bound - 1 exactly on the last column and row, whose far taps lie
    outside with weight 0.  The result is the source itself."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(37)
    src = torch.from_numpy(rng.integers(0, 256, (24, 64, 256, 3), dtype=np.uint8)).to(gpu)
    ref, got = _both(src, np.eye(3), kernels.Grid(0, 255, 256, 0, 63, 64), (64, 256))
    _check(ref, got, "identity")
    assert torch.equal(ref, src)


def test_last_two_source_rows_at_the_end_of_the_allocation(gpu):
    """The bottom tiles reach source rows src_h - 2 and src_h - 1: a staging chunk may read 9 bytes past its last texel, so these
    blocks must stay on the one-frame body.  The source is the last bytes of its allocation."""
    from ransac_with_homography_amd import kernels
    n = 24 * SRC_H * SRC_W * 3
    flat = torch.empty(14 << 20, dtype=torch.uint8, device=gpu)     # a multiple of the allocator's 2 MiB granule: nothing behind it
    assert n <= flat.numel()
    src = flat[flat.numel() - n:].view(24, SRC_H, SRC_W, 3)
    src.copy_(torch.from_numpy(np.random.default_rng(38).integers(0, 256, (24, SRC_H, SRC_W, 3), dtype=np.uint8)))
    inv = np.linalg.inv(H_S)
    _, sy, _ = _source_coords(inv, [0, 516], [385])
    assert sy.min() > SRC_H - 1                              # the grid's last row maps below the source: rows src_h - 2, src_h - 1 are inside it
    for shape in (6, 7):
        ref, got = _both(src, inv, kernels.Grid(-40, 609, 650, -25, 385, 411), (SRC_H, SRC_W), shape=shape)
        _check(ref, got, shape)


@pytest.mark.parametrize("hw", [(12, 150), (40, 140)])
def test_tiny_sources(gpu, hw):
    """The clamped window is smaller than one staging pass."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(39)
    src = torch.from_numpy(rng.integers(0, 256, (24,) + hw + (3,), dtype=np.uint8)).to(gpu)
    ref, got = _both(src, np.linalg.inv(H_S), kernels.Grid(-60, 239, 300, -80, 119, 200), hw)
    _check(ref, got, hw)


@pytest.mark.parametrize("shape", [0, 6])
@pytest.mark.parametrize("out_w", [273, 300])
def test_moved_last_tile_with_a_left_overhang(gpu, frames, out_w, shape):
    """A last tile moved left that owns 17 / 44 columns (its left waves own none and only stage), on a grid that overhangs the source
    on the left, top and bottom: own-nothing waves, the ragged-row store shift and border blocks together."""
    from ransac_with_homography_amd import kernels
    grid = kernels.Grid(-40, -40 + out_w - 1, out_w, -25, 385, 411)
    ref, got = _both(frames[:25], np.linalg.inv(H_S), grid, (SRC_H, SRC_W), shape=shape)
    _check(ref, got, (out_w, shape))


@pytest.mark.parametrize("rows", [(60, 396), (65, 390)])
def test_row_shards_inside_the_edge_blocks(gpu, frames, rows):
    """Source row 0 maps to output rows 62-79 of this grid and the last source row to rows 387-400, depending on the column: the
    shard's first tile row (16 output rows) straddles the top edge of the source, its last one the bottom edge."""
    inv = np.linalg.inv(H_S)
    last0 = rows[0] + (rows[1] - 1 - rows[0]) // 16 * 16                                  # first output row of the shard's last tile row
    _, top, _ = _source_coords(inv, np.arange(-300, 800), -60 + np.arange(rows[0], rows[0] + 16))
    _, bot, _ = _source_coords(inv, np.arange(-300, 800), -60 + np.arange(last0, rows[1]))
    assert top.min() < 0 < top.max() and bot.min() < SRC_H - 1 < bot.max()
    ref, got = _both(frames[:26], inv, _edge_grid(), (SRC_H, SRC_W), rows=rows)
    assert ref.shape[1] == rows[1] - rows[0]
    _check(ref, got, rows)


def test_horizon_inside_the_grid(gpu, frames):
    """W crosses zero inside the grid: the blocks it crosses stay on the one-frame body and must still agree."""
    H = H_S.copy()
    H[2, :2] = (2e-3, 1.5e-3)
    inv = np.linalg.inv(H)
    _, _, W = _source_coords(inv, [-300, 799], [-60, 419])
    assert W.min() < 0 < W.max()
    ref, got = _both(frames[:24], inv, _edge_grid(), (SRC_H, SRC_W))
    _check(ref, got, "horizon")


def test_random_launches_overhanging_the_source(gpu):
    """40 random launches drawn the way test_warp_batch_walk_gpu.py::test_random_launches draws them, but with the grid origin drawn
    until the grid overhangs the source on at least two sides; each batch-form launch twice."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(2036)
    for case in range(40):
        sh, sw = int(rng.integers(40, 900)), int(rng.integers(140, 1500))
        nb = int(rng.integers(24, 27))
        gen = torch.Generator(device=gpu).manual_seed(2036 + case)                              # (a failing case can be rerun alone)
        img = torch.randint(0, 256, (nb, sh, sw, 3), dtype=torch.uint8, device=gpu, generator=gen)
        t = rng.uniform(-np.pi, np.pi) if case % 4 == 0 else rng.uniform(-0.08, 0.08)
        sx, sy = rng.uniform(0.6, 1.6, 2) if case % 5 == 0 else rng.uniform(0.9, 1.15, 2)
        A = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]) @ np.array([[sx, rng.uniform(-0.1, 0.1)], [0, sy]])
        H = np.eye(3); H[:2, :2] = A
        H[:2, 2] = rng.uniform(-60, 60, 2) + np.array([sw / 2, sh / 2]) - A @ np.array([sw / 2, sh / 2])
        H[2, :2] = rng.uniform(-2e-4, 2e-4, 2) if case % 7 else rng.uniform(-2e-3, 2e-3, 2)      # sometimes a horizon inside the grid
        inv = np.linalg.inv(H)
        ow, oh = int(rng.integers(128, 1900)), int(rng.integers(5, 1100))
        stepx, stepy = rng.uniform(0.85, 1.2, 2)
        bound = (sh, sw) if case % 4 else (int(rng.integers(sh // 2, sh + 1)), int(rng.integers(sw // 2, sw + 1)))
        shape = int(rng.choice([0, 0, 5, 6, 7]))
        rows = None if case % 3 else tuple(sorted(int(v) for v in rng.integers(0, oh + 1, 2)))
        if rows is not None and rows[0] == rows[1]:
            rows = None
        r0, r1 = rows if rows is not None else (0, oh)
        for _ in range(500):
            x0, y0 = rng.uniform(-400, 60, 2)
            gx, gy = x0 + stepx * np.arange(ow), y0 + stepy * np.arange(oh)
            px, py, pw = (np.concatenate([c[0], c[-1], c[:, 0], c[:, -1]]) for c in _source_coords(inv, gx, gy))   # the grid's border
            ok = pw > 0
            sides = int((px[ok] < 0).any()) + int((px[ok] > sw - 1).any()) + int((py[ok] < 0).any()) + int((py[ok] > sh - 1).any())
            qx, qy, qw = _source_coords(inv, gx[::4], gy[r0:r1:4])                       # ... and a sample of the rows the launch writes
            hit = (qw > 0) & (qx > 1) & (qx < bound[1] - 2) & (qy > 1) & (qy < bound[0] - 2)
            if sides >= 2 and hit.any():
                break
        else:
            raise AssertionError(("no overhanging origin drawn", case))
        grid = kernels.Grid(x0, x0 + stepx * (ow - 1), ow, y0, y0 + stepy * (oh - 1), oh)
        ref, got = _both(img, inv, grid, bound, rows=rows, shape=shape, launches=2)
        assert ref.any(), case
        for g in got:
            assert torch.equal(g, ref), (case, shape, nb, rows, int((g != ref).sum()))
