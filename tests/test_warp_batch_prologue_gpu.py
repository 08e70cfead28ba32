"""The batch form of the uint8 bilinear warp (warp_rgb8_fast8<unsigned char, S, true>, body fast8mb_body) requests its first frame's
window in front of the per-pixel geometry, and its block window is 21 rows x 36 chunks (three staging slots per thread).  The moved
loads must be in flight in exactly the blocks that walk with a window and in no other, so every case here is a launch in which the
block classes coexist, and says so on the CPU (tests/warp_window_rule.py restates the block rule) before it launches anything:
interior blocks beside masked edge blocks, blocks with a wave that does not blend (wholly outside the source, or owning no column of
a moved last tile), blocks that map wholly outside (zeros, no loads) and blocks that fall back to the one-frame body (the last two
source rows; a 10 degree turn with 64 x 8 patches forced, whose interior windows are taller than the block window).

The yardstick is the one-frame kernel, which rwh_lab_tune(RWH_TUNE_WARP_FRAMES, 1) forces (and which the rest of the suite ties to
the oracle): the host's choice (knob 0) must equal it BIT FOR BIT.  Every case uses 24-26 frames of 333 x 517 (last groups of 3, 1
and 2 frames: a one-frame group requests nothing after its first window), checks that the reference is not all zeros, releases the
knobs whatever happens and launches the batch form twice."""
import numpy as np
import pytest

import warp_window_rule as rule

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
    rng = np.random.default_rng(47)
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


def _grid(t):
    from ransac_with_homography_amd import kernels
    return kernels.Grid(*t)


# grids as (x0, x_last, out_w, y0, y_last, out_h)
EDGE = (-300, 799, 1100, -60, 419, 480)                      # overhangs the source by more than one tile on every side


def _bottom(out_w=640):
    """411 rows from y = -25, out_w columns from x = -40: the top rows map above the source, the last tile rows onto its last two rows."""
    return (-40, -40 + out_w - 1, out_w, -25, 385, 411)


def _turned(deg=10.0):
    """inv(H) of a rotation about the centre of the source, with H_S's perspective row."""
    t = np.deg2rad(deg)
    c = np.array([(SRC_W - 1) / 2, (SRC_H - 1) / 2])
    H = np.eye(3)
    H[:2, :2] = [[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]
    H[:2, 2] = c - H[:2, :2] @ c
    H[2, :2] = H_S[2, :2]
    return np.linalg.inv(H)


def _classes(inv, grid, bound=(SRC_H, SRC_W), shape=6, rows=None):
    """Tiles per block class of the launch, by the restated rule."""
    win = rule.tile_windows(inv, grid, (SRC_H, SRC_W), bound, shape=shape, rows=rows)
    walk, back = rule.walks(win), rule.falls_back(win)
    return {"interior": int((walk & (win.masked == 0) & (win.blending == 4)).sum()),
            "masked": int((walk & (win.masked != 0)).sum()),
            "idle_outside": int((walk & (win.blending < win.owning)).sum()),      # a wave that owns pixels and maps wholly outside
            "idle_own_nothing": int((walk & (win.owning < 4)).sum()),             # a wave of a moved last tile that owns no column
            "outside": int((win.kind == 1).sum()),
            "fallback": int(back.sum()),
            "too_tall": int((back & (win.nrows > rule.BROWS)).sum())}


# ---- the block classes side by side ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [6, 7])
def test_every_window_class_and_the_bottom_fallback(gpu, frames, shape):
    """Interior, masked, wave-outside and all-outside blocks, and the bottom tiles that reach the last two source rows; 24 frames."""
    inv = np.linalg.inv(H_S)
    n = _classes(inv, EDGE, shape=shape)
    assert min(n["interior"], n["masked"], n["idle_outside"], n["outside"], n["fallback"]) > 0, n
    ref, got = _both(frames[:24], inv, _grid(EDGE), (SRC_H, SRC_W), shape=shape)
    _check(ref, got, shape)


@pytest.mark.parametrize("batch", [24, 25, 26])
def test_turned_windows_too_tall_beside_clamped_ones(gpu, frames, batch):
    """10 degrees with 64 x 8 patches: the interior tiles' windows are taller than the block window (fallback), the border tiles are
    clamped into the source and walk, the grid's corners map wholly outside.  Last groups of 3, 1 and 2 frames."""
    inv = _turned()
    n = _classes(inv, EDGE)
    assert min(n["too_tall"], n["masked"], n["idle_outside"], n["outside"]) > 0, n
    ref, got = _both(frames[:batch], inv, _grid(EDGE), (SRC_H, SRC_W), shape=6)
    assert ref.shape[0] == batch and ref[batch - 1].any()
    _check(ref, got, batch)


@pytest.mark.parametrize("batch", [24, 25, 26])
def test_bottom_fallback_with_last_groups_of_three_one_and_two(gpu, frames, batch):
    inv = np.linalg.inv(H_S)
    n = _classes(inv, _bottom())
    assert min(n["interior"], n["masked"], n["fallback"]) > 0, n
    ref, got = _both(frames[:batch], inv, _grid(_bottom()), (SRC_H, SRC_W))
    assert ref.shape[0] == batch and ref[batch - 1].any()
    _check(ref, got, batch)


@pytest.mark.parametrize("shape", [6, 7])
@pytest.mark.parametrize("out_w", [129, 641, 571])
def test_moved_last_tile_whose_first_waves_own_nothing(gpu, frames, out_w, shape):
    """out_w % 128 = 1 (129: the last tile is moved left and owns ONE column; 641: the strip kernel takes the column and the tiled launch
    has pitch_w != out_w) and 59 (the last tile's first wave column owns nothing): such waves stage their slots, keep the barriers and
    store nothing.  One-frame last group."""
    assert out_w % 128 in (1, 59)
    inv = np.linalg.inv(H_S)
    n = _classes(inv, _bottom(out_w), shape=shape)
    assert n["fallback"] > 0 and n["masked"] > 0, n
    assert (n["idle_own_nothing"] > 0) == (out_w != 641 and shape == 6), n       # (128 x 4 patches: every wave spans the tile's width)
    ref, got = _both(frames[:25], inv, _grid(_bottom(out_w)), (SRC_H, SRC_W), shape=shape)
    assert ref.shape[2] == out_w
    _check(ref, got, (out_w, shape))


@pytest.mark.parametrize("base", ["edge", "turned"])
@pytest.mark.parametrize("rows", [(37, 411), (21, 406)])
def test_row_shard_with_a_ragged_last_tile_row(gpu, frames, rows, base):
    """row_begin != 0 and rows % 16 != 0 (374 = 23 x 16 + 6, 385 = 24 x 16 + 1)."""
    assert rows[0] != 0 and (rows[1] - rows[0]) % 16 != 0
    inv = np.linalg.inv(H_S) if base == "edge" else _turned()
    n = _classes(inv, EDGE, rows=rows)
    assert min(n["masked"], n["outside"], n["fallback"]) > 0, n
    ref, got = _both(frames[:26], inv, _grid(EDGE), (SRC_H, SRC_W), rows=rows, shape=6)
    assert ref.shape[1] == rows[1] - rows[0]
    _check(ref, got, (rows, base))


# ---- the window's row count: the tallest window that still walks, and one row more ---------------------------------------------------

@pytest.mark.parametrize("shape", [6, 7])
def test_windows_of_exactly_the_largest_row_count_and_one_row_taller(gpu, frames, shape):
    """A homography that minifies in y: a tile's 16 output rows span 15 s source rows, and its window has floor(y_max) - floor(y_min) + 2
    rows.  With 15 s = BROWS - 1.5 that is BROWS or BROWS + 1, depending on where the tile row starts (s = 1.3 for 21 rows; the tile rows
    start 16 s = 20.8 source rows apart, so the phase moves through both).  Both counts occur, strictly inside the source."""
    s = (rule.BROWS - 1.5) / 15
    assert 1.25 <= s <= 1.35
    inv = np.array([[1.0, 0.0, 0.0], [0.002, s, 0.0], [0.0, 0.0, 1.0]])
    grid = (20, 403, 384, 8, 231, 224)                       # 3 x 14 tiles; source rows 10 .. 302, columns 20 .. 403
    win = rule.tile_windows(inv, grid, (SRC_H, SRC_W), (SRC_H, SRC_W), shape=shape)
    assert (win.kind == 0).all() and (win.masked == 0).all() and (win.chunks <= rule.BCH).all()
    at, over = int((win.nrows == rule.BROWS).sum()), int((win.nrows == rule.BROWS + 1).sum())
    assert at >= 3 and over >= 3 and at + over == win.nrows.size, (at, over, np.unique(win.nrows))
    assert int(rule.walks(win).sum()) == at and int(rule.falls_back(win).sum()) == over
    ref, got = _both(frames[:25], inv, _grid(grid), (SRC_H, SRC_W), shape=shape)
    _check(ref, got, (shape, at, over))
