"""examples/smoothed_boundary_fit.py (PDEModel.train on a Cahn-Hilliard particle inside a disc, ramped contact angle) runs
end to end on the GPU at a reduced size."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_smoothed_boundary_fit_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "smoothed_boundary_fit.py"), "--quick"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
