"""examples/cahn_hilliard_coarsening.py (PDEModel.structure_factor_trace on a spinodal decomposition) runs end to end on
the GPU at its reduced size, and the coarsening length it prints grows from save point to save point."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cahn_hilliard_coarsening_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cahn_hilliard_coarsening.py"), "--quick"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok", r.stdout[-2000:]
    rows = [ln.split() for ln in lines[1:7]]  # the table: t, length, <k>, sqrt<k^2>, variance at the 6 save points
    lengths = [float(row[1]) for row in rows]
    assert len(lengths) == 6 and all(b > a for a, b in zip(lengths, lengths[1:])), lengths
