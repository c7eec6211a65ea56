"""The spectral steps (csrc/strang_fused.hip with fft_lds.hpp / fft_reg.hpp / fft_reg32.hpp, csrc/spectral.hip) on inputs
that fill every bin and distinguish every bin: white-noise states and multiplier tables with one independent complex value
per frequency (tests/spectral_ref.py).  A wrong twiddle, digit reversal, multiplier slot (col_mult_index), mirror index of
the IMEX symmetrisation or a transposed table moves the result by O(1) here (tests/test_spectral_ref_cpu.py holds the
margins), where a smooth Gaussian under an even table hides all of them.

Gates.  fp64: the project's relative L2 of 1e-10 on Strang states (tests/test_gpu_fuzz.py) and 1e-9 on IMEX increments
(tests/test_gpu_fft.py).  fp32: 8 x the distance of the single-precision reference from the complex128 one on the same
case (the margin of tests/test_gpu_gpe_adjoint.py: the device rounds in another order), under the project's ceilings 2e-5
and 5e-4.  The single-precision reference's distance, measured on the CPU over these cases: Strang 4.6e-7 .. 1.4e-6, IMEX
increments 9.7e-7 .. 2.1e-6.  The device's distances are recorded beside the assertions below."""
import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L

import spectral_ref as S

pytestmark = pytest.mark.gpu

STRANG_KERNEL = {"fused": "strang_fused_lds_fft", "rocfft": "strang_rocfft_c2c", "generic": "strang_rocfft_c2c"}


def strang_engine(case, dtype, path, table=None, group=2):
    """a configured engine holding the case: per-environment k, groups of 2 (a window boundary inside the batch of 3)"""
    eng = P.HipEngine()
    eng.set_group_envs(group)
    if path == "generic":
        eng.set_kernel_path(L.PATH_GENERIC)
    eng.configure(dtype=np.dtype(dtype), batch=len(case.y0), **case.eq._engine_problem())
    case.eq._engine_upload(eng, 0.0)
    case.solver(P, table).configure_engine(eng, case.eq)
    eng.set_env_gpe_k(0, case.ks)
    eng.set_state(case.y0.astype(dtype))
    return eng


def imex_engine(case, dtype, path, table=None):
    eng = P.HipEngine()
    if path == "generic":
        eng.set_kernel_path(L.PATH_GENERIC)
    eng.configure(dtype=np.dtype(dtype), batch=len(case.y0), **case.eq._engine_problem())
    case.eq._engine_upload(eng, 0.0)
    case.solver(P, table).configure_engine(eng, case.eq)
    if path == "per_env":
        eng.set_env_params(0, kappa=S.KAPPA * case.scales)
        eng.set_env_imex_scale(0, case.scales)
    eng.set_state(case.y0.astype(dtype))
    return eng


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("time_scale", S.TIME_SCALES)
@pytest.mark.parametrize("shape,path", S.STRANG_CASES)
def test_strang_white_noise_asymmetric_table(shape, path, time_scale, dtype):
    case = S.StrangCase(P, shape, time_scale)
    eng = strang_engine(case, dtype, path)
    try:
        eng.advance(L.INT_STRANG, case.dt, case.steps, 0.0)
        got = eng.get_state()
        assert eng.last_kernel == STRANG_KERNEL[path], eng.last_kernel
    finally:
        eng.close()
    y0 = case.y0.astype(dtype)
    want = case.reference(y0)
    d = S.states_distance(got, want)
    if dtype is np.float64:
        print(f"strang fp64 {shape} {path} ts={time_scale}: {d:.3e}")
        # measured on the MI355X over these 33 cases: 1.4e-15 .. 2.2e-15
        assert d < S.STRANG_GATE64
    else:
        d_ref = S.states_distance(case.reference_single(y0), want)
        print(f"strang fp32 {shape} {path} ts={time_scale}: {d:.3e} (complex64 reference {d_ref:.3e})")
        # measured on the MI355X over these 33 cases: 4.3e-7 .. 1.3e-6 against 4.8e-7 .. 1.4e-6 of the complex64 reference
        # (0.86 .. 2.2 x the reference's on the same case; the gate came to 3.8e-6 .. 1.1e-5, under the 2e-5 ceiling)
        assert d <= S.gate32(d_ref, S.STRANG_CEIL32)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,batch,path", S.IMEX_CASES)
def test_imex_white_noise_asymmetric_symbol(shape, batch, path, dtype):
    """the fused passes with an even and an odd batch (the last complex field half empty), one environment per field
    with unequal scales, rocFFT's real transforms in 2-D, the two 1-D layouts and 3-D, rocFFT forced"""
    case = S.imex_case(P, shape, batch, path)
    eng = imex_engine(case, dtype, path)
    try:
        eng.advance(L.INT_IMEX, case.dt, case.steps)
        got = eng.get_state()
        fused = path in ("fused", "per_env")
        assert ("imex_fused_lds_fft" in eng.last_kernel) == fused and ("imex_rocfft_r2c" in eng.last_kernel) == (not fused), eng.last_kernel
    finally:
        eng.close()
    y0 = case.y0.astype(dtype)
    want = case.reference(y0)
    assert np.isfinite(got).all()
    d = S.increments_distance(got, want, y0)
    if dtype is np.float64:
        print(f"imex fp64 {shape} batch {batch} {path}: {d:.3e}")
        # measured on the MI355X over these 18 cases: 1.5e-15 .. 2.5e-15
        assert d < S.IMEX_GATE64
    else:
        d_ref = S.increments_distance(case.reference_single(y0), want, y0)
        print(f"imex fp32 {shape} batch {batch} {path}: {d:.3e} (complex64 reference {d_ref:.3e})")
        # measured on the MI355X over these 18 cases: 9.8e-7 .. 2.0e-6 against 9.7e-7 .. 2.1e-6 of the complex64 reference
        # (0.96 .. 1.11 x the reference's on the same case; the gate came to 7.7e-6 .. 1.7e-5, under the 5e-4 ceiling)
        assert d <= S.gate32(d_ref, S.IMEX_CEIL32)


# ---- a table uploaded over another one with the same dt and time_scale / A ----------------------------------------------


@pytest.mark.parametrize("shape,path", [((64, 128), "fused"), ((48, 40), "rocfft")])
def test_strang_second_table_is_not_served_from_the_first(shape, path):
    """the multiplier exp(A tau / 2) is cached on (dt, time_scale): a new A_term under the same key must rebuild it"""
    case = S.StrangCase(P, shape, -1j)
    table_b = S.strang_table(case.A_even, case.dt, case.time_scale, 99)
    eng = strang_engine(case, np.float64, path)
    fresh = strang_engine(case, np.float64, path, table_b)
    try:
        eng.advance(L.INT_STRANG, case.dt, case.steps, 0.0)
        first = eng.get_state()
        case.solver(P, table_b).configure_engine(eng, case.eq)
        eng.set_state(case.y0)
        eng.advance(L.INT_STRANG, case.dt, case.steps, 0.0)
        second = eng.get_state()
        fresh.advance(L.INT_STRANG, case.dt, case.steps, 0.0)
        want = fresh.get_state()
        assert eng.last_kernel == fresh.last_kernel == STRANG_KERNEL[path]
    finally:
        eng.close()
        fresh.close()
    assert S.states_distance(first, want) > 0.1  # the two tables give different answers
    np.testing.assert_array_equal(second, want)


@pytest.mark.parametrize("shape,path", [((64, 256), "fused"), ((48, 40), "rocfft")])
def test_imex_second_symbol_is_not_served_from_the_first(shape, path):
    """the implicit multiplier is cached on (dt, A): a new fourier_symbol under the same key must rebuild it"""
    case = S.imex_case(P, shape, 3, path)
    table_b = S.imex_table(case.s0, 99)
    eng = imex_engine(case, np.float64, path)
    fresh = imex_engine(case, np.float64, path, table_b)
    try:
        eng.advance(L.INT_IMEX, case.dt, case.steps)
        first = eng.get_state()
        case.solver(P, table_b).configure_engine(eng, case.eq)
        eng.set_state(case.y0)
        eng.advance(L.INT_IMEX, case.dt, case.steps)
        second = eng.get_state()
        fresh.advance(L.INT_IMEX, case.dt, case.steps)
        want = fresh.get_state()
        assert ("imex_fused_lds_fft" in eng.last_kernel) == (path == "fused")
    finally:
        eng.close()
        fresh.close()
    assert S.increments_distance(first, want, case.y0) > 0.01
    np.testing.assert_array_equal(second, want)
