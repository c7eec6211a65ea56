"""The kappa instantiations of the tangent kernels (csrc/sens.hip, template parameter KAPPA) and the IMEX multiply with the
operator's derivative (csrc/spectral.hip, sens_imex_mul_kappa_kernel) use no scratch and stay under the register and LDS
figures recorded here, and the KAPPA = false instantiations -- what every fit without kappa launches -- report the figures
of the kernels before the template parameter existed.  From the compiler's own report; no GPU needed: hipcc
cross-compiles for gfx950."""
import pytest

from pde_opt_amd.csrc import build as B

# kernel -> (VGPRs, static LDS bytes) of the KAPPA = false instantiation: the figures of the untemplated kernels, which
# these must keep exactly (their instruction streams were compared once)
PARENT = {
    "sens_tangent_rhs_kernel<float, false>": (33, 22896),
    "sens_tangent_rhs_kernel<double, false>": (83, 45792),
    "sens_ac_tangent_rhs_kernel<float, false>": (44, 5760),
    "sens_ac_tangent_rhs_kernel<double, false>": (74, 10368),
    "sens3d_dmu_kernel<float, false>": (41, 0),
    "sens3d_dmu_kernel<double, false>": (42, 0),
}
# ceilings of the new code: (VGPRs, static LDS bytes).  The 2-D Cahn-Hilliard kernel recomputes lap(u) from the resident
# tile (no LDS growth), Allen-Cahn keeps two more registers, the 3-D kernel one; the multiply holds a handful of complex
# values.  The VGPR ceilings leave the occupancy of the false instantiations unchanged (512 / VGPRs waves per SIMD).
CEILINGS = {
    "sens_tangent_rhs_kernel<float, true>": (40, 22896),
    "sens_tangent_rhs_kernel<double, true>": (84, 45792),
    "sens_ac_tangent_rhs_kernel<float, true>": (48, 5760),
    "sens_ac_tangent_rhs_kernel<double, true>": (80, 10368),
    "sens3d_dmu_kernel<float, true>": (48, 0),
    "sens3d_dmu_kernel<double, true>": (48, 0),
    "sens_imex_mul_kappa_kernel<float>": (32, 0),
    "sens_imex_mul_kappa_kernel<double>": (40, 0),
}


@pytest.fixture(scope="module")
def res():
    B.build(verbose=False)
    return B.kernel_resources()


def test_the_lists_name_every_instantiation(res):
    names = [k for k in res if k.startswith(("sens_tangent_rhs_kernel", "sens_ac_tangent_rhs_kernel", "sens3d_dmu_kernel",
                                             "sens_imex_mul_kappa_kernel"))]
    assert sorted(names) == sorted(list(PARENT) + list(CEILINGS))


@pytest.mark.parametrize("kernel", list(CEILINGS))
def test_kappa_kernels_use_no_scratch_and_keep_their_ceilings(res, kernel):
    r = res[kernel]
    vgpr, lds = CEILINGS[kernel]
    assert r["scratch"] == 0, r
    assert r["vgpr"] + r["agpr"] <= vgpr and r["lds_static"] <= lds, r


@pytest.mark.parametrize("kernel", list(PARENT))
def test_instantiations_without_kappa_report_the_figures_they_had(res, kernel):
    r = res[kernel]
    assert (r["vgpr"], r["lds_static"]) == PARENT[kernel] and r["scratch"] == 0 and r["agpr"] == 0, r
