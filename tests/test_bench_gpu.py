"""bench.py on the GPU: a plain run prints the headline line only, and --dump-outputs writes what its timed warp computed --
the same values a second process computes from the same seeded frames, and the reference's transformImageH within 1 LSB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_step(tmp_path):
    import torch
    import bench
    from oracle import rwh_oracle as orc
    out_dir = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "2",
                        "--src", "640x480", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "Mpix/s" and line["config"]["full"] is False
    assert "ransac" not in line and "cpu_baseline" not in line and "warp_8k" not in line
    got = np.load(out_dir / "warp_out.npy")

    backend = bench.GpuBackend(0)
    step, out_h, out_w, _, _, (src, dst, _, _) = backend.make_warp(2, 640, 480, 1234)      # rank 0's frames: seed 1234
    step()
    torch.cuda.synchronize()
    assert got.dtype == np.float32 and got.shape == (2, out_h, out_w, 3)
    assert np.array_equal(got, dst.cpu().numpy().astype(np.float32))
    for f in range(2):
        ref, _, _ = orc.transform_image_h(src[f].cpu().numpy(), bench.H_S)
        assert ref.shape == (out_h, out_w, 3)
        d = np.abs(got[f].astype(np.int16) - ref.astype(np.int16))
        assert d.max() <= 1 and (d != 0).mean() < 0.02, (f, d.max(), (d != 0).mean())
