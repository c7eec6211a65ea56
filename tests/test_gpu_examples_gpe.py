"""examples/gpe_control_gradient.py (PDEModel.optimize over a laser spot's position with the adjoint of the Strang step)
runs end to end on the GPU and prints a decreasing objective."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpe_control_gradient_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "gpe_control_gradient.py"), "--quick"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    J = [float(v) for v in re.findall(r"^step \d+: J = (\S+)$", r.stdout, flags=re.M)]
    assert len(J) >= 3, r.stdout[-2000:]
    assert all(b < a for a, b in zip(J, J[1:])), J
    assert J[-1] < 1e-2 * J[0], J
