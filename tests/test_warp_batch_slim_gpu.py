"""The batch form of the uint8 bilinear warp (warp_rgb8_fast8<unsigned char, S, true>, body fast8mb_body) without spill code: the blocks
that still run the one-frame body frame by frame (a window that reaches the last two source rows, a window over 22 rows x 36 chunks, a
horizon wave) read FastArgs again from the kernarg segment instead of keeping the kernel's copy live across the window path.  Every
case here is a launch in which such fallback blocks and window blocks coexist, and each varies one group of the argument fields the
fallback reads by that route: source size and strides, bounds, row shard, grid steps, out_w / pitch_w, tile counts, frames per group.

The yardstick is the one-frame kernel, which rwh_lab_tune(RWH_TUNE_WARP_FRAMES, 1) forces (and which the rest of the suite ties to
the oracle): the host's choice (knob 0) must equal it BIT FOR BIT.  Every case uses 24-26 frames of 333 x 517, checks that the reference
is not all zeros, releases the knobs whatever happens and launches the batch form twice.

Two bases put fallback blocks next to window blocks:
  * BOTTOM: the grid's last tile rows map onto and below the last two source rows (those blocks fall back, the rows above them walk);
  * TURNED: a 10 degree rotation with 64 x 8 patches forced: an interior tile's footprint is 128 sin 10 + 16 cos 10 + 2 = 40 rows,
    taller than the 22-row block window (fallback), while tiles on the border are clamped into the source and fit (window), and the
    grid's corners map wholly outside (zeros)."""
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
    rng = np.random.default_rng(41)
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


def _bottom_grid(out_w=640, x_step=1.0, y_step=1.0):
    """411 rows from y = -25, out_w columns from x = -40: the top rows map above the source, the last tile rows onto and below its last
    two rows."""
    from ransac_with_homography_amd import kernels
    grid = kernels.Grid(-40, -40 + x_step * (out_w - 1), out_w, -25, -25 + y_step * 410, 411)
    _, sy, _ = _source_coords(np.linalg.inv(H_S), [-40, -40 + x_step * (out_w - 1)], [-25 + y_step * 410])
    assert sy.min() > SRC_H - 1                              # below the source: rows src_h - 2 and src_h - 1 lie inside the grid
    return grid


def _edge_grid():
    """Overhangs the 333 x 517 source by more than one 128 x 16 tile on every side."""
    from ransac_with_homography_amd import kernels
    return kernels.Grid(-300, 799, 1100, -60, 419, 480)


def _turned(deg=10.0):
    """inv(H) of a rotation about the centre of the source, with H_S's perspective row."""
    t = np.deg2rad(deg)
    c = np.array([(SRC_W - 1) / 2, (SRC_H - 1) / 2])
    H = np.eye(3)
    H[:2, :2] = [[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]
    H[:2, 2] = c - H[:2, :2] @ c
    H[2, :2] = H_S[2, :2]
    return np.linalg.inv(H)


# ---- (a) the fallback's arguments, one group of fields per case ---------------------------------------------------------------------

@pytest.mark.parametrize("shape", [6, 7, 0])
def test_bottom_tiles_reach_the_last_two_source_rows(gpu, frames, shape):
    ref, got = _both(frames[:25], np.linalg.inv(H_S), _bottom_grid(), (SRC_H, SRC_W), shape=shape)
    _check(ref, got, shape)


def test_horizon_inside_the_grid(gpu, frames):
    H = H_S.copy()
    H[2, :2] = (2e-3, 1.5e-3)
    inv = np.linalg.inv(H)
    _, _, W = _source_coords(inv, [-300, 799], [-60, 419])
    assert W.min() < 0 < W.max()
    ref, got = _both(frames[:24], inv, _edge_grid(), (SRC_H, SRC_W))
    _check(ref, got, "horizon")


def test_turned_by_ten_degrees_window_taller_than_22_rows(gpu, frames):
    inv = _turned()
    _, sy, _ = _source_coords(inv, [200, 327], [150, 165])   # one 128 x 16 tile in the middle of the source
    assert sy.max() - sy.min() + 2 > 22 and sy.min() > 0 and sy.max() < SRC_H - 1
    ref, got = _both(frames[:25], inv, _edge_grid(), (SRC_H, SRC_W), shape=6)
    _check(ref, got, "turned")


@pytest.mark.parametrize("base", ["bottom", "turned"])
def test_bound_smaller_than_the_source(gpu, frames, base):
    if base == "bottom":                                     # (the bound keeps the last two source rows, so the bottom tiles still fall back)
        args, bound, shape = (np.linalg.inv(H_S), _bottom_grid()), (SRC_H, 400), 0
    else:
        args, bound, shape = (_turned(), _edge_grid()), (200, 400), 6
    ref, got = _both(frames[:25], *args, bound, shape=shape)
    _check(ref, got, base)
    full, _ = _both(frames[:25], *args, (SRC_H, SRC_W), shape=shape)
    assert not torch.equal(full, ref)                        # (the bound really cuts pixels away)


@pytest.mark.parametrize("rows", [(37, 411), (21, 406)])
def test_row_shard_with_a_ragged_last_tile_row(gpu, frames, rows):
    """row_begin != 0 and rows % 16 != 0 (374 = 23 x 16 + 6, 385 = 24 x 16 + 1); the shard ends in the fallback's rows."""
    assert rows[0] != 0 and (rows[1] - rows[0]) % 16 != 0
    ref, got = _both(frames[:25], np.linalg.inv(H_S), _bottom_grid(), (SRC_H, SRC_W), rows=rows)
    assert ref.shape[1] == rows[1] - rows[0]
    _check(ref, got, rows)


def test_linspace_grid_with_non_unit_steps(gpu, frames):
    grid = _bottom_grid(x_step=1.013, y_step=1.0079)
    ref, got = _both(frames[:25], np.linalg.inv(H_S), grid, (SRC_H, SRC_W))
    _check(ref, got, "linspace")
    unit, _ = _both(frames[:25], np.linalg.inv(H_S), _bottom_grid(), (SRC_H, SRC_W))
    assert not torch.equal(unit, ref)


@pytest.mark.parametrize("out_w", [513, 650, 656, 571])
def test_ragged_rows(gpu, frames, out_w):
    """out_w % 128 = 1, 10, 16: the strip kernel takes the ragged edge and the tiled launch has pitch_w != out_w.  out_w % 128 = 59: the
    last tile is moved left and its first wave(s) own no column."""
    assert out_w % 128 in (1, 10, 16, 59)
    ref, got = _both(frames[:25], np.linalg.inv(H_S), _bottom_grid(out_w=out_w), (SRC_H, SRC_W))
    assert ref.shape[2] == out_w
    _check(ref, got, out_w)


@pytest.mark.parametrize("shape", [6, 7])
def test_moved_last_tile_in_the_turned_launch(gpu, frames, shape):
    """out_w % 128 = 59 where the fallback blocks are the interior ones: their waves that own no column return at once."""
    from ransac_with_homography_amd import kernels
    grid = kernels.Grid(-100, -100 + 698, 699, -60, 419, 480)
    assert 699 % 128 == 59
    ref, got = _both(frames[:25], _turned(), grid, (SRC_H, SRC_W), shape=shape)
    _check(ref, got, shape)


@pytest.mark.parametrize("base", ["bottom", "turned"])
@pytest.mark.parametrize("batch", [25, 26])
def test_last_group_of_one_and_two_frames(gpu, frames, batch, base):
    args, shape = ((np.linalg.inv(H_S), _bottom_grid()), 0) if base == "bottom" else ((_turned(), _edge_grid()), 6)
    ref, got = _both(frames[:batch], *args, (SRC_H, SRC_W), shape=shape)
    assert ref.shape[0] == batch and ref[batch - 1].any()
    _check(ref, got, (batch, base))


# ---- (b) the tap weights at the ends of the fraction's range, interior and edge blocks -----------------------------------------------

@pytest.mark.parametrize("shape", [6, 7, 0])
@pytest.mark.parametrize("where", ["interior", "edge"])
@pytest.mark.parametrize("shift", [0.0, 0.5, 1.0 - 2.0 ** -20])
def test_fractions_zero_half_and_next_to_one(gpu, frames, shift, where, shape):
    """Identity homography, unit steps, the grid shifted by `shift`: every pixel's fractions are 0, 1/2 or 1 - 2^-20."""
    from ransac_with_homography_amd import kernels
    if where == "interior":                                  # 384 x 288 output pixels strictly inside the source: 3 x 18 whole tiles
        grid = kernels.Grid(20 + shift, 20 + shift + 383, 384, 10 + shift, 10 + shift + 287, 288)
    else:
        grid = kernels.Grid(-300 + shift, -300 + shift + 1099, 1100, -60 + shift, -60 + shift + 479, 480)
    ref, got = _both(frames[:25], np.eye(3), grid, (SRC_H, SRC_W), shape=shape)
    _check(ref, got, (shift, where, shape))
    if shift == 0.0 and where == "interior":
        assert torch.equal(ref, frames[:25, 10:298, 20:404])
