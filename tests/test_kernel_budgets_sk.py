"""The kernels of the structure factor (csrc/structure_factor.hip) use no scratch and no static LDS beyond the finish
kernel's reduction, from the compiler's own report (the one tests/test_kernel_budgets.py reads).  No GPU needed: hipcc
cross-compiles for gfx950."""
import pytest

from pde_opt_amd.csrc import build as B

KERNELS = ["sk_bin_kernel<float>", "sk_bin_kernel<double>", "sk_finish_kernel"]


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return B.kernel_resources()


def test_the_list_names_every_kernel_of_the_file(res):
    assert sorted(k for k in res if k.startswith("sk_")) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_structure_factor_kernels_use_no_scratch(res, kernel):
    assert res[kernel]["scratch"] == 0


def test_static_lds_is_the_reduction_only(res):
    """the four waves' shell arrays of sk_bin_kernel are its dynamic allocation (4 n_bins doubles, sized per call); the
    only static LDS is the finish kernel's four partial sums per shell of its 64-shell tile"""
    assert res["sk_bin_kernel<float>"]["lds_static"] == 0 and res["sk_bin_kernel<double>"]["lds_static"] == 0
    assert res["sk_finish_kernel"]["lds_static"] == 4 * 64 * 8


def test_the_library_is_not_built_with_a_flag_that_weakens_the_fp64_root():
    """host and device must agree on floor(sqrt(q) + 0.5) bit for bit: the root has to be the correctly rounded one"""
    weak = ("-ffast-math", "-Ofast", "-funsafe-math-optimizations", "-ffp-model=fast", "-ffp-model=aggressive", "-fapprox-func",
            "-freciprocal-math", "-fgpu-approx-transcendentals")
    assert not [f for f in B.CXXFLAGS if f in weak]
