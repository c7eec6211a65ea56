"""examples/cahn_hilliard_energy.py (PDEModel.free_energy_trace on a spinodal decomposition and one VectorPDEEnv episode
rewarded by the free energy) runs end to end on the GPU."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cahn_hilliard_energy_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cahn_hilliard_energy.py"), "--quick"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-2000:]
