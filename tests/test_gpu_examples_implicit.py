"""examples/implicit_euler.py (ImplicitEuler next to SemiImplicitFourierSpectral on Cahn-Hilliard, then Allen-Cahn with the
logarithmic potential) runs end to end on the GPU at its reduced size."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_implicit_euler_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "implicit_euler.py"), "--quick"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok", r.stdout[-2000:]
    assert any(ln.startswith("stats:") and "krylov_iterations" in ln for ln in lines)
    assert sum(1 for ln in lines if "rms difference" in ln) == 1
