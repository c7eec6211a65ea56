"""examples/gpe_rotation_fit.py (PDEModel.optimize_rotation recovering omega and e from a final density) runs end to end
on the GPU at a small size (64 x 64, 20 substeps: the CPU reference gradient converges on it as well)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpe_rotation_fit_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "gpe_rotation_fit.py"), "--points", "64", "--substeps", "20"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-2000:]
