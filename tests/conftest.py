import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")


def pytest_sessionstart(session):
    """A fresh checkout has no libpdeopt_hip.so (built artefacts are git-ignored): build it once -- hipcc
    cross-compiles for gfx950 without a GPU; nothing happens when the library is up to date.  The C oracle
    (test infrastructure) builds itself on first use."""
    lib = os.path.join(ROOT, "pde_opt_amd", "libpdeopt_hip.so")
    if not os.path.exists(lib):
        from pde_opt_amd.csrc import build as B

        B.build(verbose=False)


class _GoldenParts:
    """a golden stored as <stem>.part0.npz, <stem>.part1.npz, ... (each under the 1 MiB limit for a committed file;
    oracle/gen_golden.py splits it), read as the one npz it was: ``.files`` and ``[key]``"""

    def __init__(self, paths):
        import numpy as np

        self._parts = [np.load(p) for p in paths]
        self.files = [k for z in self._parts for k in z.files]

    def __getitem__(self, key):
        for z in self._parts:
            if key in z.files:
                return z[key]
        raise KeyError(key)


@pytest.fixture(scope="session")
def golden():
    import glob

    import numpy as np

    def load(name):
        path = os.path.join(GOLDEN, name)
        parts = glob.glob(path[: -len(".npz")] + ".part*.npz")
        if os.path.exists(path) or not parts:
            return np.load(path)
        return _GoldenParts(sorted(parts, key=lambda p: int(p[: -len(".npz")].rsplit(".part", 1)[1])))

    return load
