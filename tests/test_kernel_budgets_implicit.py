"""The kernels of the implicit Euler step (csrc/implicit.hip) use no scratch, and stay within the register and LDS
budgets below, from the compiler's own report (the one tests/test_kernel_budgets.py reads).  No GPU needed: hipcc
cross-compiles for gfx950.

The limits are the compiler's figures at the time of writing, rounded up to the next occupancy step of a 256-thread
workgroup (128 VGPRs: 4 waves per SIMD; 64: 8), and for LDS the arrays the kernels declare: the Cahn-Hilliard operator
holds u and v on the 20 x 36 ring-2 tile and four face quantities on the 18 x 34 ring-1 tile, the Allen-Cahn operator u
and v on the ring-1 tile, the vector kernels their reduction rows and the column of the small system."""
import pytest

from pde_opt_amd.csrc import build as B

R2, R1 = 20 * 36, 18 * 34
# kernel: (VGPR limit, static LDS limit in bytes)
BUDGETS = {
    "imp_op_ch_kernel<float>": (64, (2 * R2 + 4 * R1) * 4),
    "imp_op_ch_kernel<double>": (128, (2 * R2 + 4 * R1) * 8),
    "imp_op_ac_kernel<float>": (64, 2 * R1 * 4),
    "imp_op_ac_kernel<double>": (128, 2 * R1 * 8),
    "imp_residual_kernel<float>": (64, 4 * 8),
    "imp_residual_kernel<double>": (64, 4 * 8),
    "imp_dots_kernel<float>": (64, 4 * 8 * 8),
    "imp_dots_kernel<double>": (64, 4 * 8 * 8),
    "imp_update_kernel<float>": (64, (64 + 4) * 8),
    "imp_update_kernel<double>": (64, (64 + 4) * 8),
    "imp_solution_kernel<float>": (64, 64 * 8),
    "imp_solution_kernel<double>": (64, 64 * 8),
    "imp_restart_kernel<float>": (64, 4 * 8),
    "imp_restart_kernel<double>": (64, 4 * 8),
    "imp_newton_small_kernel": (64, 0),
    "imp_gmres_small_kernel": (64, 65 * 8),
    "imp_restart_small_kernel": (64, 0),
}


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return B.kernel_resources()


def test_the_list_names_every_kernel_of_the_file(res):
    assert sorted(k for k in res if k.startswith("imp_")) == sorted(BUDGETS)


@pytest.mark.parametrize("kernel", sorted(BUDGETS))
def test_implicit_kernels_use_no_scratch(res, kernel):
    assert res[kernel]["scratch"] == 0


@pytest.mark.parametrize("kernel", sorted(BUDGETS))
def test_registers_and_lds_within_budget(res, kernel):
    vgpr, lds = BUDGETS[kernel]
    assert res[kernel]["vgpr"] + res[kernel]["agpr"] <= vgpr
    assert res[kernel]["lds_static"] <= lds
