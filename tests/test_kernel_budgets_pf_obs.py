"""The kernels of the phase-field observables (csrc/pf_obs.hip) use no scratch, from the compiler's own report (the one
tests/test_kernel_budgets.py reads).  No GPU needed: hipcc cross-compiles for gfx950."""
import pytest

from pde_opt_amd.csrc import build as B

CH, AC = 0, 1                      # PDEOPT_EQ_CAHN_HILLIARD, PDEOPT_EQ_ALLEN_CAHN
GENERIC, POLY, LOGIT = 0, 1, 2     # closure classes CL_GENERIC, CL_POLY, CL_LOGIT (common.hpp)


def kernels():
    out = ["pfobs_finish_kernel"]
    for d in ("float", "double"):
        for cl in (GENERIC, POLY, LOGIT):
            out += [f"pfobs_tile_kernel<{d}, {eq}, {cl}>" for eq in (CH, AC)]
            out += [f"pfobs_mu3_kernel<{d}, {cl}>", f"pfobs_sum3_kernel<{d}, {cl}>"]
    return out


KERNELS = kernels()


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return B.kernel_resources()


def test_the_list_names_every_kernel_of_the_file(res):
    assert sorted(k for k in res if k.startswith("pfobs_")) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_observable_kernels_use_no_scratch(res, kernel):
    assert res[kernel]["scratch"] == 0


def test_the_tile_kernels_keep_their_lds(res):
    """u on the tile + ring in the state's type, and for Cahn-Hilliard mu and D on the tile + forward ring in fp64
    (DESIGN.md section 4.19): the arrays + the 256 bytes of the workgroup reduction (+ alignment padding between them)"""
    for d, size in (("float", 4), ("double", 8)):
        for cl in (GENERIC, POLY, LOGIT):
            for eq, arrays in ((CH, size * 20 * 68 + 8 * 2 * 17 * 65), (AC, size * 18 * 66)):
                assert 0 <= res[f"pfobs_tile_kernel<{d}, {eq}, {cl}>"]["lds_static"] - (arrays + 256) <= 64
