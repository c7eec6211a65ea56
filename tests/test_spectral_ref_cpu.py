"""CPU checks of what tests/test_gpu_spectral_broadband.py leans on (tests/spectral_ref.py): the symmetrisation identity
the IMEX kernels use, the single-precision restatement of the two steps against the numpy oracle, and that every input of
the GPU tests discriminates -- a mirrored, a transposed or the even table moves the complex128 reference by far more than
the gates the device is held to."""
import numpy as np
import pytest

import pde_opt_amd as P

import spectral_ref as S


# ---- Re ifftn(M fftn f) == ifftn(M_h fftn f) -------------------------------------------------------------------------


@pytest.mark.parametrize("shape", [(256, 1), (1, 96), (48, 40), (64, 256), (7, 10), (8, 6, 10), (16, 12, 20)])
def test_symmetrisation_identity(shape):
    """M_h(k) = (M(k) + conj M(-k)) / 2 of csrc/spectral.hip (half_spectrum) and csrc/strang_fused.hip (imex_prepare_t)
    for the asymmetric complex symbol, in 1, 2 and 3 dimensions; the k = 0 and Nyquist bins mirror onto themselves"""
    rng = np.random.default_rng(5)
    k = np.meshgrid(*[np.fft.fftfreq(n, 0.01) for n in shape], indexing="ij")
    symbol = S.imex_table(S.KAPPA * (sum((2.0 * np.pi * q) ** 2 for q in k)) ** 2, 6)  # kappa |2 pi k|^4 as s0
    assert np.abs(symbol.imag).max() > 0 and np.abs(symbol - S.mirrored(symbol)).max() > 0.1 * np.abs(symbol).max()
    M = 1.0 / (1.0 + S.IMEX_A * S.IMEX_DT * symbol)
    Mh = S.symmetrised(M)
    # the self-mirrored bins (0 and, on an even axis, n / 2) hold Re M
    for idx in np.ndindex(*[2] * len(shape)):
        cell = tuple((n // 2) * i for n, i in zip(shape, idx))
        if all(c == (-c) % n for c, n in zip(cell, shape)):
            assert Mh[cell].imag == 0.0 and Mh[cell].real == M[cell].real
    f = rng.standard_normal(shape)
    full = np.fft.ifftn(M * np.fft.fftn(f))
    half = np.fft.ifftn(Mh * np.fft.fftn(f))
    scale = np.abs(full.real).max()
    assert np.abs(half.real - full.real).max() <= 1e-13 * scale
    assert np.abs(half.imag).max() <= 1e-13 * scale
    assert np.abs(full.imag).max() > 1e-3 * scale  # the table is not hermitian: `.real` does discard something
    # two real fields in one complex transform, as the fused IMEX passes carry them
    g = rng.standard_normal(shape)
    pair = np.fft.ifftn(Mh * np.fft.fftn(f + 1j * g))
    assert np.abs(pair.real - full.real).max() <= 1e-13 * scale
    assert np.abs(pair.imag - np.fft.ifftn(M * np.fft.fftn(g)).real).max() <= 1e-13 * scale


def test_per_environment_scale_does_not_commute_with_the_symmetrisation():
    """why the one-environment-per-field mode keeps the unsymmetrised table: scaling the symbol by sigma and
    symmetrising is not symmetrising and rescaling 1 / (1 + sigma (1 / M_h - 1)) unless the symbol is even"""
    case = S.ImexCase(P, (64, 128), 1)
    adt, sigma = S.IMEX_A * S.IMEX_DT, 1.5
    want = S.symmetrised(1.0 / (1.0 + adt * sigma * case.symbol))
    rescaled = 1.0 / (1.0 + sigma * (1.0 / S.symmetrised(1.0 / (1.0 + adt * case.symbol)) - 1.0))
    assert np.abs(rescaled - want).max() > 1e-3
    even = 1.0 / (1.0 + sigma * (1.0 / S.symmetrised(1.0 / (1.0 + adt * case.s0)) - 1.0))
    assert np.abs(even - 1.0 / (1.0 + adt * sigma * case.s0)).max() < 1e-12


# ---- the single-precision steps -------------------------------------------------------------------------------------


@pytest.mark.parametrize("time_scale", S.TIME_SCALES)
def test_strang_restatement_equals_the_oracle_in_double(time_scale):
    case = S.StrangCase(P, (48, 40), time_scale)
    got, want = case.reference_single(case.y0, double=True), case.reference(case.y0)
    assert S.states_distance(got, want) < 1e-13


@pytest.mark.parametrize("shape,batch,path", [((48, 40), 2, "rocfft"), ((128, 256), 3, "per_env"), ((8, 6, 10), 2, "rocfft")])
def test_imex_restatement_equals_the_oracle_in_double(shape, batch, path):
    case = S.imex_case(P, shape, batch, path)
    got, want = case.reference_single(case.y0, double=True), case.reference(case.y0)
    assert S.increments_distance(got, want, case.y0) < 1e-12


# ---- every input of the GPU tests discriminates -------------------------------------------------------------------------


def test_every_transform_size_runs_on_both_axes():
    """each line length of the hand-written transforms is an nx and an ny of a non-square Strang case (both precisions
    run on every case), and the 1024-point lines, where fft_reg32.hpp runs in fp32 only, also of an IMEX case"""
    oblong = [s for s in S.STRANG_FUSED_SHAPES if s[0] != s[1]]
    assert {s[0] for s in oblong} == set(S.FFT_SIZES) and {s[1] for s in oblong} == set(S.FFT_SIZES)
    assert any(s[0] == s[1] for s in S.STRANG_FUSED_SHAPES)  # the transposed table needs a square case
    imex = S.IMEX_FUSED_SHAPES + (S.IMEX_PER_ENV_SHAPE,)
    assert {s[0] for s in imex} == set(S.FFT_SIZES) and 1024 in {s[1] for s in imex}


def _margins(d, gate64, gate32):
    return d >= 1000.0 * gate64 and d >= 100.0 * gate32


@pytest.mark.parametrize("time_scale", S.TIME_SCALES)
@pytest.mark.parametrize("shape,path", S.STRANG_CASES)
def test_strang_inputs_discriminate(shape, path, time_scale):
    case = S.StrangCase(P, shape, time_scale)
    assert np.abs(case.A - S.mirrored(case.A)).max() > 0
    y32 = case.y0.astype(np.float32)
    want = case.reference(y32)
    assert np.isfinite(want).all()
    d32 = S.states_distance(case.reference_single(y32), want)
    gate32 = S.gate32(d32, S.STRANG_CEIL32)
    others = {"mirrored": S.mirrored(case.A), "even": case.A_even}
    if shape[0] == shape[1]:
        others["transposed"] = case.A.T
    dist = {name: min(S.rel_l2(g, w) for g, w in zip(case.reference(y32, t), want)) for name, t in others.items()}
    print(f"strang {shape} ts={time_scale}: complex64 reference {d32:.3e} (fp32 gate {gate32:.3e}), "
          + ", ".join(f"{k} {v:.3e}" for k, v in dist.items()))
    assert 1e-8 < d32 < S.STRANG_CEIL32 / S.F32_MARGIN  # single precision really, and the ceiling is not what decides
    for name, d in dist.items():
        assert _margins(d, S.STRANG_GATE64, gate32), (name, d)


@pytest.mark.parametrize("shape,batch,path", S.IMEX_CASES)
def test_imex_inputs_discriminate(shape, batch, path):
    case = S.imex_case(P, shape, batch, path)
    assert case.symbol.real.min() >= 0.0
    adt = case.A * case.dt * np.abs(case.symbol).max()
    y32 = case.y0.astype(np.float32)
    want = case.reference(y32)
    assert np.isfinite(want).all() and want.min() > 0.0 and want.max() < 1.0
    d32 = S.increments_distance(case.reference_single(y32), want, y32)
    gate32 = S.gate32(d32, S.IMEX_CEIL32)
    y64 = y32.astype(np.float64)
    others = {"mirrored": S.mirrored(case.symbol), "even": case.s0}
    dist = {name: min(S.rel_l2(g - y, w - y) for g, w, y in zip(case.reference(y32, t), want, y64)) for name, t in others.items()}
    print(f"imex {shape} batch {batch} {path}: max A dt |symbol| {adt:.1f}, complex64 reference {d32:.3e} "
          f"(fp32 gate {gate32:.3e}), " + ", ".join(f"{k} {v:.3e}" for k, v in dist.items()))
    assert d32 > 1e-8
    for name, d in dist.items():
        assert _margins(d, S.IMEX_GATE64, gate32), (name, d)
