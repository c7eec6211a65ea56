"""CPU checks of what tests/test_gpu_gpe_rot_broadband.py leans on (tests/gpe_rot_broadband_ref.py): the references agree
with each other, the domain damps no bin away, the smooth states of the older tests are blind to the faults this file is
about, and every white-noise case of the GPU tests discriminates: each applicable mutant of the complex128 reference moves
the result by 10 x the case's fp32 gate or more, after one step and after three."""
import numpy as np
import pytest

import gpe_rot_broadband_ref as B
import gpe_rot_ref as R
import gpe_rot_stir_ref as S

ALL_CASES = [(s, p, False) for s, p in B.FROZEN_CASES] + [(s, p, True) for s, p in B.STIR_CASES]


# ---- the shapes ---------------------------------------------------------------------------------------------------------


def test_every_line_length_runs_on_both_axes():
    """each line length of the fused passes is an nx and an ny of an oblong frozen case (both precisions run on every
    case); 256 and 1024 also of a stirred one, with 512 as a stirred nx and the library path in both variants"""
    oblong = [s for s in B.FUSED_SHAPES if s[0] != s[1]]
    assert {s[0] for s in oblong} == set(B.ROT_SIZES) and {s[1] for s in oblong} == set(B.ROT_SIZES)
    assert any(s[0] == s[1] for s in B.FUSED_SHAPES)
    stirred = [s for s, p in B.STIR_CASES if p == "fused"]
    assert {256, 512, 1024} <= {s[0] for s in stirred} and {256, 1024} <= {s[1] for s in stirred}
    assert any(p == "rocfft" for _, p in B.STIR_CASES) and any(p == "rocfft" for _, p in B.FROZEN_CASES)
    assert (B.GENERIC_SHAPE, "generic") in B.FROZEN_CASES and all(n in B.ROT_SIZES for n in B.GENERIC_SHAPE)
    for shape, _ in B.BITWISE_CASES:
        assert (shape, "fused") in B.FROZEN_CASES and (shape, "fused") in B.STIR_CASES


@pytest.mark.parametrize("shape", sorted({s for s, _, _ in ALL_CASES}))
def test_the_domain_has_one_cell_size_and_the_state_is_normalised(shape):
    dom = B.domain(shape)
    assert dom.dx == (B.H, B.H)
    psi = B.white_noise(shape)
    assert psi.shape == (B.BATCH,) + tuple(shape) and not psi.flags.writeable
    assert np.array_equal(psi, psi.astype(np.complex64))  # both precisions of the device start from these numbers
    assert np.allclose(np.sum(np.abs(psi) ** 2, axis=(1, 2)) * B.H**2, 1.0, rtol=1e-6)
    # white: the upper half of every line's spectrum holds its share of the weight
    for axis, n in ((1, shape[0]), (2, shape[1])):
        spec = np.abs(np.fft.fft(psi, axis=axis)) ** 2
        upper = np.take(spec, range(n // 4, 3 * n // 4), axis=axis).sum() / spec.sum()
        assert 0.4 < upper < 0.6, (axis, upper)


@pytest.mark.parametrize("shape,path,stirred", ALL_CASES)
def test_damping_bound(shape, path, stirred):
    """max |Re (tau / 2) A| over every bin, line, environment, time scale and step: no bin is damped away or blown up in
    imaginary time (0.28 at 128 points and 1.27 at 1024 for the frozen Omega, 1.71 at 1024 with the ramp)"""
    d = B.damping(shape, stirred)
    print(f"damping {shape} stirred={stirred}: {d:.3f}")
    assert d <= B.DAMPING_BOUND


# ---- the references agree -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("time_scale", B.TIME_SCALES)
def test_stir_case_without_spots_and_ramp_is_rot_case(time_scale):
    """``StirCase`` with rate 0 and no lights is ``RotCase``, at every Omega of the batch (Omega = 0 among them), from
    any start time"""
    shape = (64, 128)
    dom = B.domain(shape)
    for b, psi in enumerate(B.white_noise(shape)):
        rot = R.RotCase(dom, B.KS[b], B.E, B.OMEGAS[b], time_scale).advance(psi, B.DT, B.STEPS)
        stir = S.StirCase(dom, B.KS[b], B.E, B.OMEGAS[b], time_scale).advance(psi, B.DT, B.STEPS, B.T0)
        assert np.array_equal(rot, stir), b


@pytest.mark.parametrize("stirred", [False, True])
@pytest.mark.parametrize("time_scale", B.TIME_SCALES)
def test_torch_transforms_in_double_are_the_numpy_reference(time_scale, stirred):
    shape = (48, 40) if stirred else (96, 80)
    for got, want in zip(B.reference(shape, time_scale, stirred, "torch_double"), B.reference(shape, time_scale, stirred)):
        assert B.dist(got, want) <= 1e-13


# ---- what the smooth states cannot see ----------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", [(256, 64), (1024, 64), (512, 256)])
def test_smooth_states_are_blind_to_the_upper_bins(shape):
    """on ``gpe_rot_ref.smooth_state`` the Nyquist sign and the exchanged upper bins of the x lines stay below the fp64
    gate of the older tests (the Gaussians are narrow against the long axis of these boxes, as against a line of that
    many points in the older tests); on white noise the same mutants are 10 x the fp32 gate away (below)"""
    dom = B.domain(shape)
    psi = R.smooth_state(dom, 5)[0]
    p = B.params_of(0, False)
    want = R.RotCase(dom, p["k"], p["e"], p["omega"], 1.0).advance(psi, B.DT, B.STEPS)
    for mutant in ("nyquist_x", "exchange_x"):
        case = B.make_case(shape, 0, 1.0, False, mutant=mutant)
        d = B.dist(case.advance(psi, B.DT, B.STEPS), want)
        print(f"smooth state {shape} {mutant}: {d:.3e}")
        assert d < B.GATE64


# ---- every input of the GPU tests discriminates -------------------------------------------------------------------------



@pytest.mark.parametrize("shape,path,stirred", ALL_CASES)
@pytest.mark.parametrize("time_scale", B.TIME_SCALES)
def test_white_noise_discriminates(shape, path, stirred, time_scale):
    """after 1 step and after 3: the torch complex64 reference is the complex128 one to 1e-5 and is single precision
    really; every applicable mutant is 10 x the gate made of it away or more"""
    want = B.reference(shape, time_scale, stirred)
    assert all(np.isfinite(w).all() for w in want)
    gates = B.gates32(shape, time_scale, stirred)
    for d32, gate in gates:
        assert 1e-8 < d32 <= 1e-5 and gate == min(B.F32_MARGIN * d32, B.CEIL32)
    names = [m for m in B.MUTANTS if B.applicable(m, shape, time_scale)]
    # left out at most: bit reversal on the rocFFT sizes or the other axis's coordinate on a square grid, the conjugate
    assert len(names) >= len(B.MUTANTS) - 3
    # the mutants on the environments that rotate: the distance over those is a lower bound of the batch's, and at
    # Omega = 0 most of the mutants are the reference
    envs = [b for b in range(B.BATCH) if B.OMEGAS[b] != 0.0]
    below = lambda g, w: float(np.max(np.abs(g - w[envs])) / np.max(np.abs(w)))
    moved = {m: [below(g, w) for g, w in zip(B.mutant_reference(shape, time_scale, stirred, m, envs=envs), want)]
             for m in names}
    print(f"{shape} stirred={stirred} ts={time_scale}: complex64 reference {gates[0][0]:.3e} / {gates[1][0]:.3e}, "
          + ", ".join(f"{m} {a:.2e}/{b:.2e}" for m, (a, b) in moved.items()))
    for m, ds in moved.items():
        for d, (_, gate) in zip(ds, gates):
            assert d >= B.MUTANT_MARGIN * gate and d >= 1000.0 * B.GATE64, (m, d, gate)
