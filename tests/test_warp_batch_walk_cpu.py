"""rwh_warp_plan names the kernel FAMILY: the bench configuration (32 x 4K RGB uint8, bilinear, uint8 out, H_S) reports
rwh::warp_rgb8_fast8<unsigned char, 6> whether the host picks the family's batch form (knob 0) or the one-frame kernel is forced
(rwh_lab_tune(RWH_TUNE_WARP_FRAMES, 1)).  No GPU needed: nothing is launched."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


def test_bench_configuration_plan_is_the_family_name():
    from ransac_with_homography_amd import _lib, kernels
    lib = _lib.load()
    H_S = np.array([[1.02, 0.01, 5.0], [0.015, 0.98, 7.0], [1e-5, 2e-5, 1.0]])
    inv = np.linalg.inv(H_S)
    grid = kernels.Grid(5, 3775, 3771, 7, 2034, 2028)
    try:
        for knob in (0, 1):
            assert lib.rwh_lab_tune(_lib.RWH_TUNE_WARP_FRAMES, knob) == 0
            plan = kernels.warp_plan((32, 2160, 3840, 3), torch.uint8, inv, grid, (2160, 3840), "bilinear", torch.uint8)
            assert plan == "rwh::warp_rgb8_fast8<unsigned char, 6>", (knob, plan)
    finally:
        assert lib.rwh_lab_tune(_lib.RWH_TUNE_WARP_FRAMES, 0) == 0
