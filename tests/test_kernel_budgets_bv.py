"""The Butler-Volmer kernels (csrc/butler_volmer.hip) use no scratch and leave room for two workgroups per compute unit,
from the compiler's own report (the one tests/test_kernel_budgets.py reads).  No GPU needed: hipcc cross-compiles for
gfx950.

A workgroup is 256 threads = one wave on each of the CU's four SIMDs, so two resident workgroups are two waves per
SIMD: 512 registers per lane / 2 = 256 VGPRs + AGPRs per wave, and half of the CU's 160 KiB of LDS each."""
import pytest

from pde_opt_amd.csrc import build as B

VGPR_BUDGET = 256
LDS_BUDGET = 80 * 1024


def kernels():
    out = ["bv_finish_kernel"]
    for d in ("float", "double"):
        out += [f"bv_mu_sums_kernel<{d}, {s}>" for s in ("false", "true")]
        out += [f"bv_rate_kernel<{d}, {s}>" for s in (0, 1, 2)]
    return out


KERNELS = kernels()


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return B.kernel_resources()


def test_the_list_names_every_kernel_of_the_file(res):
    assert sorted(k for k in res if k.startswith("bv_")) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_bv_kernels_use_no_scratch(res, kernel):
    assert res[kernel]["scratch"] == 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_two_workgroups_fit_a_compute_unit(res, kernel):
    r = res[kernel]
    assert r["vgpr"] + r["agpr"] <= VGPR_BUDGET, r
    assert r["lds_static"] <= LDS_BUDGET, r
    assert r["occupancy"] >= 2, r
