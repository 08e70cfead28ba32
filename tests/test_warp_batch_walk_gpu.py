"""The batch form of the uint8 bilinear warp kernel (warp_rgb8_fast8<unsigned char, S, true>: for 24 or more frames of at most 4K
with one homography a block walks its 128 x 16 tile through consecutive frames and stages one window per block) against the
one-frame kernel, which rwh_lab_tune(RWH_TUNE_WARP_FRAMES, 1) forces: the two must agree BIT FOR BIT.  Both report the same plan
string (the kernel family), so every case compares the host's own choice (knob 0) with the forced one-frame launch.

Source: 333 x 517 RGB uint8 noise (interior, border and wholly-outside patches on the grids below; 517 * 3 is odd, so source rows
are not 16-byte aligned) and a 512-wide one whose rows are."""
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
    rng = np.random.default_rng(24)
    return torch.from_numpy(rng.integers(0, 256, (FRAMES, SRC_H, SRC_W, 3), dtype=np.uint8)).to(gpu)


def _tune(knob, value):
    from ransac_with_homography_amd import _lib
    assert _lib.load().rwh_lab_tune(knob, int(value)) == 0


def _both(src, inv, grid, bound, rows=None, shape=0, launches=1):
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


def _auto_grid(h, w, H):
    from ransac_with_homography_amd import kernels
    from ransac_with_homography_amd import homography as hg
    mx, my, ow, oh = hg._bounds(h, w, H, 0)
    return kernels.Grid(mx, mx + ow - 1, ow, my, my + oh - 1, oh)


def _rot(deg):
    t = np.deg2rad(deg)
    c, s, cx, cy = np.cos(t), np.sin(t), 258.0, 166.0
    return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0, 0, 1.0]])


def _check(ref, got, what):
    assert ref.any(), what                                   # (a reference of zeros would compare equal to anything unwritten)
    for g in got:
        assert torch.equal(g, ref), (what, int((g != ref).sum()))


@pytest.mark.parametrize("batch", [23, 24, 25, 26])
def test_batch_sizes_on_auto_bounds_grid(gpu, frames, batch):
    """Groups of 3 frames with a remainder of 0, 1 and 2 frames (24, 25, 26); 23 frames stay on the one-frame path and agree too."""
    ref, got = _both(frames[:batch], np.linalg.inv(H_S), _auto_grid(SRC_H, SRC_W, H_S), (SRC_H, SRC_W))
    assert ref.shape[0] == batch
    _check(ref, got, batch)


@pytest.mark.parametrize("out_w", [256, 272, 273, 300])
def test_ragged_right_edges(gpu, frames, out_w):
    """256: whole tiles; 272: two tiles and the strip launch; 273, 300: a last tile moved left that owns 17 / 44 columns."""
    from ransac_with_homography_amd import kernels
    grid = kernels.Grid(-40, -40 + out_w - 1, out_w, -25, 385, 411)      # overhangs the source on the left, top and bottom
    ref, got = _both(frames[:25], np.linalg.inv(H_S), grid, (SRC_H, SRC_W))
    _check(ref, got, out_w)


def test_rotation_by_10_degrees(gpu, frames):
    """Another patch shape (32 x 16) is the host's choice here."""
    from ransac_with_homography_amd import kernels
    grid = kernels.Grid(-40, 609, 650, -25, 385, 411)
    ref, got = _both(frames[:24], np.linalg.inv(_rot(10)), grid, (SRC_H, SRC_W))
    _check(ref, got, "rot10")


@pytest.mark.parametrize("rows", [(5, 37), (100, 229), (200, 211)])
def test_row_shards(gpu, frames, rows):
    """Row shards restart the tile rows at their first row; a shard of fewer than 16 rows takes the one-frame path."""
    from ransac_with_homography_amd import kernels
    grid = kernels.Grid(-40, 609, 650, -25, 385, 411)
    ref, got = _both(frames[:25], np.linalg.inv(H_S), grid, (SRC_H, SRC_W), rows=rows)
    assert ref.shape[1] == rows[1] - rows[0]
    _check(ref, got, rows)


def test_source_rows_16_byte_aligned(gpu):
    """A 512-wide source: every source row starts on a 16-byte boundary (the 517-wide one's rows do not)."""
    rng = np.random.default_rng(25)
    src = torch.from_numpy(rng.integers(0, 256, (24, SRC_H, 512, 3), dtype=np.uint8)).to(gpu)
    ref, got = _both(src, np.linalg.inv(H_S), _auto_grid(SRC_H, 512, H_S), (SRC_H, 512))
    _check(ref, got, "aligned rows")


def test_random_launches(gpu):
    """40 random launches drawn the way tools/soak_mf.py draws them (homography, grid, bound, patch shape, row shard), all with 24 or
    more frames; each batch-form launch twice (a race shows differently from launch to launch)."""
    from ransac_with_homography_amd import kernels
    rng = np.random.default_rng(2024)
    for case in range(40):
        sh, sw = int(rng.integers(40, 900)), int(rng.integers(140, 1500))
        nb = int(rng.integers(24, 34))
        img = torch.randint(0, 256, (nb, sh, sw, 3), dtype=torch.uint8, device=gpu)
        t = rng.uniform(-np.pi, np.pi) if case % 4 == 0 else rng.uniform(-0.08, 0.08)
        sx, sy = rng.uniform(0.6, 1.6, 2) if case % 5 == 0 else rng.uniform(0.9, 1.15, 2)
        A = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]) @ np.array([[sx, rng.uniform(-0.1, 0.1)], [0, sy]])
        H = np.eye(3); H[:2, :2] = A
        H[:2, 2] = rng.uniform(-60, 60, 2) + np.array([sw / 2, sh / 2]) - A @ np.array([sw / 2, sh / 2])
        H[2, :2] = rng.uniform(-2e-4, 2e-4, 2) if case % 7 else rng.uniform(-2e-3, 2e-3, 2)      # sometimes a horizon inside the grid
        inv = np.linalg.inv(H)
        ow, oh = int(rng.integers(128, 1900)), int(rng.integers(5, 1100))
        x0, y0 = rng.uniform(-120, 60, 2)
        stepx, stepy = rng.uniform(0.85, 1.2, 2)
        grid = kernels.Grid(x0, x0 + stepx * (ow - 1), ow, y0, y0 + stepy * (oh - 1), oh)
        bound = (sh, sw) if case % 4 else (int(rng.integers(sh // 2, sh + 1)), int(rng.integers(sw // 2, sw + 1)))
        shape = int(rng.choice([0, 0, 5, 6, 7]))
        rows = None if case % 3 else tuple(sorted(int(v) for v in rng.integers(0, oh + 1, 2)))
        if rows is not None and rows[0] == rows[1]:
            rows = None
        ref, got = _both(img, inv, grid, bound, rows=rows, shape=shape, launches=2)
        for g in got:
            assert torch.equal(g, ref), (case, shape, nb, rows, int((g != ref).sum()))
