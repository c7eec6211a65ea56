"""The kernels of the stirred, ramped rotating-frame split step (csrc/gpe_rot.hip) use no scratch, from the
compiler's own report (the one tests/test_kernel_budgets.py reads).  No GPU needed: hipcc cross-compiles for gfx950."""
import pytest

from pde_opt_amd.csrc import build as B

SIZES = (64, 128, 256, 512, 1024)


def cols(dtype, n):
    """columns per workgroup of the column pass (rot_cols in gpe_rot_step.hpp)"""
    c, cap, tt = (16, 512, n // (16 if n > 512 else 8)) if dtype == "float" else (8, 256, n // (16 if n > 512 else 8))
    return cap // tt if c * tt > cap else c


def kernels():
    out = []
    for d in ("float", "double"):
        out += [f"rstir_row_kernel<{d}, {n}>" for n in SIZES]
        for n in SIZES:
            # FIRST, LAST, JOIN; fp64 at 1024 runs JOIN as LAST + FIRST (rot_join_fits)
            forms = ["false, true", "true, false"] + ([] if (d, n) == ("double", 1024) else ["true, true"])
            out += [f"rstir_col_kernel<{d}, {n}, {cols(d, n)}, {f}>" for f in forms]
        out += [f"rstir_mul_kernel<{d}, 0, false>", f"rstir_mul_kernel<{d}, 0, true>", f"rstir_mul_kernel<{d}, 1, false>",
                f"rstir_b_kernel<{d}>"]
    return out


KERNELS = kernels()


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return B.kernel_resources()


def test_the_list_names_every_kernel_of_the_file(res):
    assert sorted(k for k in res if k.startswith("rstir_")) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_stirred_step_kernels_use_no_scratch(res, kernel):
    assert res[kernel]["scratch"] == 0
