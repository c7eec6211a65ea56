"""The kernels of the stirred rotating-frame split step's adjoint (csrc/gpe_rot_adjoint.hip) use no scratch and no
AGPRs, from the compiler's own report (the one tests/test_kernel_budgets.py reads).  No GPU needed: hipcc cross-compiles
for gfx950."""
import pytest

from pde_opt_amd.csrc import build as B

KERNELS = ["rsadj_mul_kernel<{}, 0>", "rsadj_mul_kernel<{}, 1>", "rsadj_conj_mul_kernel<{}, 0, false>",
           "rsadj_conj_mul_kernel<{}, 1, false>", "rsadj_conj_mul_kernel<{}, 1, true>", "rsadj_recompute_kernel<{}>",
           "rsadj_pointwise_kernel<{}>", "rsadj_finish_kernel<{}>"]


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return B.kernel_resources()


def test_the_list_names_every_kernel_of_the_file(res):
    assert sorted(k for k in res if k.startswith("rsadj_")) == sorted(k.format(d) for k in KERNELS for d in ("float", "double"))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype", ["float", "double"])
def test_rot_stir_adjoint_kernels_use_no_scratch_and_no_agprs(res, kernel, dtype):
    v = res[kernel.format(dtype)]
    assert v["scratch"] == 0 and v["agpr"] == 0
