"""The kernels of the GPE observables (csrc/gpe_obs.hip) use no scratch, from the compiler's own report (the one
tests/test_kernel_budgets.py reads).  No GPU needed: hipcc cross-compiles for gfx950."""
import pytest

from pde_opt_amd.csrc import build as B

SIZES = (64, 128, 256, 512, 1024)


def cols(dtype, n):
    """columns per workgroup of the column pass (gobs_cols in gpe_obs.hip)"""
    c, cap = (16, 512) if dtype == "float" else (8, 256)
    tt = n // (16 if n > 512 else 8)
    return cap // tt if c * tt > cap else c


def kernels():
    out = ["gobs_finish_kernel"]
    for d in ("float", "double"):
        out += [f"gobs_row_kernel<{d}, {n}>" for n in SIZES]
        out += [f"gobs_col_kernel<{d}, {n}, {cols(d, n)}>" for n in SIZES]
        out += [f"gobs_point_kernel<{d}>", f"gobs_spec_kernel<{d}>"]
    return out


KERNELS = kernels()


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return B.kernel_resources()


def test_the_list_names_every_kernel_of_the_file(res):
    assert sorted(k for k in res if k.startswith("gobs_")) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_observable_kernels_use_no_scratch(res, kernel):
    assert res[kernel]["scratch"] == 0
