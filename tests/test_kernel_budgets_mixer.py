"""The mixer kernels (csrc/mixer.hip) use no scratch and at most 64 KB of LDS per workgroup, from the compiler's own
report (the one tests/test_kernel_budgets.py reads), and the C header, the library and the ctypes table agree on the
``pdeopt_mixer_*`` calls.  No GPU needed: hipcc cross-compiles for gfx950."""
import os
import re

import pytest

from pde_opt_amd import _lib as L
from pde_opt_amd.csrc import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["create", "set_params", "forward", "vjp", "grad_read", "destroy"]


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return {k: v for k, v in B.kernel_resources().items() if k.startswith("mixer_")}


def test_every_instantiation_is_reported(res):
    # the product: 2 dtypes x (no activation + 4 activations); everything else: 2 dtypes each
    assert sum(k.startswith("mixer_gemm_kernel<") for k in res) == 10
    for k in ("mixer_wgrad_kernel", "mixer_stats_kernel", "mixer_ln_bwd_sums_kernel", "mixer_ln_bwd_apply_kernel", "mixer_sum_kernel"):
        assert f"{k}<float>" in res and f"{k}<double>" in res
    assert len(res) == 20


def test_mixer_kernels_use_no_scratch_and_little_lds(res):
    assert res
    for name, v in res.items():
        assert v["scratch"] == 0, name
        assert v["lds_static"] <= 64 * 1024, name


def test_abi_symbols_and_ctypes_table_agree():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdeopt_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(pdeopt_mixer_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(f"pdeopt_mixer_{c}" for c in CALLS)
    assert sorted(k for k in L._SIGNATURES if k.startswith("pdeopt_mixer_")) == declared
    lib = L.load_library()
    for name in declared:
        assert hasattr(lib, name), name
