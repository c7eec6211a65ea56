"""The field-mu kernels (csrc/fieldmu.hip) use no scratch, from the compiler's own report (the one
tests/test_kernel_budgets.py reads).  No GPU needed: hipcc cross-compiles for gfx950."""
import pytest

from pde_opt_amd.csrc import build as B


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return B.kernel_resources()


@pytest.mark.parametrize("kernel", ["fieldmu_rhs_kernel", "fieldmu_adjoint_kernel"])
@pytest.mark.parametrize("dtype", ["float", "double"])
def test_fieldmu_kernels_use_no_scratch(res, kernel, dtype):
    v = res[f"{kernel}<{dtype}>"]
    assert v["scratch"] == 0 and v["agpr"] == 0
    # five tiles of the adjoint kernel in fp64 are 27 KB: at least two workgroups per CU whatever the registers
    assert v["lds_static"] <= 32 * 1024
