"""examples/mobility_and_mu_fit.py --quick runs on the MI355X, its loss decreases and D moves"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mobility_and_mu_fit_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "mobility_and_mu_fit.py"), "--quick"], env=env,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "native" in r.stdout and "D coefficients [0. 0.] ->" in r.stdout
    m = re.search(r"loss ([0-9.e+-]+) -> ([0-9.e+-]+)", r.stdout)
    assert m and float(m.group(2)) < float(m.group(1))
