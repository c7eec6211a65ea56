"""The adjoint kernel that also sums the mobility's coefficient gradient (csrc/fieldmu.hip) uses no scratch and stays
within the LDS of two workgroups per CU, from the compiler's own report; the kernel it was copied from is still there.
No GPU needed: hipcc cross-compiles for gfx950."""
import pytest

from pde_opt_amd.csrc import build as B


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return B.kernel_resources()


@pytest.mark.parametrize("dtype", ["float", "double"])
def test_coefficient_gradient_kernel_budgets(res, dtype):
    v = res[f"fieldmu_adjoint_coef_kernel<{dtype}>"]
    assert v["scratch"] == 0 and v["agpr"] == 0
    # fp64: the five tiles (27 KB), one fp64 weight per owned cell (4 KB), 16 x 4 partial sums
    assert v["lds_static"] <= 32 * 1024


@pytest.mark.parametrize("dtype", ["float", "double"])
def test_the_plain_adjoint_kernel_is_still_there(res, dtype):
    assert f"fieldmu_adjoint_kernel<{dtype}>" in res
