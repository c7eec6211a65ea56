"""examples/gpe_stirring_fit.py (PDEModel.optimize_stirring recovering a beam's speed and the spin-up rate from a final
state) runs end to end on the GPU at its small size (64 x 64, 20 substeps) and its history falls."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpe_stirring_fit_example_runs_and_its_history_falls():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "gpe_stirring_fit.py"), "--points", "64", "--substeps", "20"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-2000:]
    hist = [float(v) for v in re.findall(r"iteration +\d+: J = (\S+)", r.stdout)]
    assert len(hist) >= 2 and all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < hist[0], hist
