"""examples/kappa_fit.py (PDEModel.train with kappa as a TrainableScalar next to mu, IMEX) runs end to end on the GPU and
brings kappa closer to the truth than it started."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kappa_fit_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "kappa_fit.py"), "--quick"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"^KAPPA_FIT (\S+)$", r.stdout, flags=re.M)
    assert m, r.stdout[-2000:]
    assert abs(float(m.group(1)) - 0.002) < abs(0.003 - 0.002), r.stdout[-2000:]  # truth 0.002, start 0.003
    assert len(re.findall(r"^iteration \d+: kappa = ", r.stdout, flags=re.M)) >= 2  # kappa is printed per iteration
