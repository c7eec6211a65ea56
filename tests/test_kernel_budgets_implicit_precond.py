"""The kernels of ImplicitEuler's spectral preconditioner (csrc/implicit.hip, names precond_*) use no scratch and stay
within the register and LDS budgets below, from the compiler's own report, like tests/test_kernel_budgets_implicit.py for
the kernels of the unpreconditioned solver.  No GPU needed: hipcc cross-compiles for gfx950.

The preconditioned operators are the unpreconditioned ones with another source for the stored basis vector: the same
limits.  The rest sit at the 8-waves-per-SIMD step (64 VGPRs) and declare a reduction row (coefficients) or the column of
the small system (the combination V y_k) at most."""
import pytest

from pde_opt_amd.csrc import build as B

R2, R1 = 20 * 36, 18 * 34
# kernel: (VGPR limit, static LDS limit in bytes)
BUDGETS = {
    "precond_op_ch_kernel<float>": (64, (2 * R2 + 4 * R1) * 4),
    "precond_op_ch_kernel<double>": (128, (2 * R2 + 4 * R1) * 8),
    "precond_op_ac_kernel<float>": (64, 2 * R1 * 4),
    "precond_op_ac_kernel<double>": (128, 2 * R1 * 8),
    "precond_coef_kernel<float>": (64, 4 * 8),
    "precond_coef_kernel<double>": (64, 4 * 8),
    "precond_coef_finish_kernel": (64, 0),
    "precond_mul_kernel<float>": (64, 0),
    "precond_mul_kernel<double>": (64, 0),
    "precond_combine_kernel<float>": (64, 64 * 8),
    "precond_combine_kernel<double>": (64, 64 * 8),
    "precond_add_kernel<float>": (64, 0),
    "precond_add_kernel<double>": (64, 0),
}


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return B.kernel_resources()


def test_the_list_names_every_preconditioner_kernel(res):
    assert sorted(k for k in res if k.startswith("precond_")) == sorted(BUDGETS)


@pytest.mark.parametrize("kernel", sorted(BUDGETS))
def test_preconditioner_kernels_use_no_scratch(res, kernel):
    assert res[kernel]["scratch"] == 0


@pytest.mark.parametrize("kernel", sorted(BUDGETS))
def test_registers_and_lds_within_budget(res, kernel):
    vgpr, lds = BUDGETS[kernel]
    assert res[kernel]["vgpr"] + res[kernel]["agpr"] <= vgpr
    assert res[kernel]["lds_static"] <= lds
