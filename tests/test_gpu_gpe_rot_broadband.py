"""The rotating-frame split step (csrc/gpe_rot.hip with gpe_rot_line.hpp, fft_reg.hpp and fft_lds.hpp; DESIGN.md sections
4.10 and 4.13) on white noise: every line length of the fused passes as nx and as ny, the library path, frozen and stirred,
both precisions, one interaction strength and one Omega per environment (tests/gpe_rot_broadband_ref.py).  A wrong
frequency slot, digit reversal, late-stage twiddle or Nyquist sign in a line operator moves these results by 10 x the fp32
gate or more (tests/test_gpe_rot_broadband_cpu.py holds that for every case below), where the smooth states of
tests/test_gpu_gpe_rot.py and tests/test_gpu_gpe_rot_stir.py leave the upper bins at rounding level.

Gates.  fp64: 1e-10, max-abs relative to max-abs (tests/test_gpu_gpe_rot.py).  fp32: 8 x the distance of the
single-precision reference (transforms at complex64 through torch.fft on the CPU) from the complex128 one on the same case,
under the project's Strang ceiling 2e-5.  Neither comes from the device; the device's distances are recorded beside the
assertions below.

Launches per advance of n steps, from strang_rot_t (csrc/gpe_rot.hip): the fused step runs window by window, a window
being ``set_group_envs`` environments, and a window takes FIRST, then per step the row pass and a column pass (JOIN, the
last one LAST): 2 n + 1.  In fp64 at nx = 1024 JOIN runs as LAST + FIRST (rot_join_fits), which makes every step but
the last three launches: 1 + 3 (n - 1) + 2 = 3 n.  The library path counts 6 per step for the whole batch
(rot_library_step), whatever the group setting."""
import functools

import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd.engine import HipEngine

import gpe_rot_broadband_ref as B
import gpe_rot_ref as R

pytestmark = pytest.mark.gpu

GROUP = 2  # a window boundary inside the batch of 3


def kernel_name(path, stirred):
    stir = "_stir" if stirred else ""
    return f"strang_rot{stir}_fused_lds_fft" if path == "fused" else f"strang_rot{stir}_rocfft_1d"


def launches(shape, path, dtype, batch, group, n):
    """stage launches of one advance of n steps (derived in the module docstring)"""
    if path != "fused":
        return 6 * n
    windows = -(-batch // min(group, batch))
    per_window = 3 * n if (np.dtype(dtype) == np.float64 and shape[0] == 1024) else 2 * n + 1
    return windows * per_window


def engine_for(shape, path, time_scale, dtype, stirred, envs=tuple(range(B.BATCH)), group=GROUP):
    """a configured engine holding the environments `envs` of the case, and the solver's integrator"""
    dom = B.domain(shape)
    eqs = [P.GPE2DTSRot(dom, **B.params_of(b, stirred)) for b in envs]
    solver = P.RotatingStrangSplitting(eqs[0].dx, time_scale)
    y0 = R.to_pairs(B.white_noise(tuple(shape))[list(envs)]).astype(dtype)
    t0 = B.T0 if stirred else 0.0
    eng = HipEngine(0)
    eng.set_group_envs(group)
    if path == "generic":
        eng.set_kernel_path(L.PATH_GENERIC)
    eng.configure(dtype=y0.dtype, batch=len(envs), **eqs[0]._engine_problem())
    if len(envs) == 1:
        eqs[0]._engine_upload(eng, t0, t0 + 1.0)
    else:
        P.GPE2DTSRot._engine_upload_batch(eng, eqs, t0, t0 + 1.0)
    solver.configure_engine(eng, eqs[0])
    eng.set_state(y0)
    return eng, solver.integrator, y0, t0


def advance(eng, integ, y0, t0, calls):
    """the state after the advance calls in `calls` (numbers of steps) from y0, each call starting at the local time the
    one before it ended at, and the stage launches of every call"""
    eng.set_state(y0)
    done, counts = 0, []
    for n in calls:
        before = eng.stage_launches()
        eng.advance(integ, B.DT, n, t0 + done * B.DT)
        counts.append(eng.stage_launches() - before)
        done += n
    return R.from_pairs(eng.get_state().astype(np.float64)), counts


def check_against_the_reference(shape, path, time_scale, dtype, stirred):
    eng, integ, y0, t0 = engine_for(shape, path, time_scale, dtype, stirred)
    try:
        three, (count3,) = advance(eng, integ, y0, t0, (B.STEPS,))
        kernel = eng.last_kernel
        one, (count1,) = advance(eng, integ, y0, t0, (1,))
        assert eng.last_kernel == kernel == kernel_name(path, stirred), (eng.last_kernel, kernel)
        if path == "fused":
            assert eng.last_groups() == 2
    finally:
        eng.close()
    assert count3 == launches(shape, path, dtype, B.BATCH, GROUP, B.STEPS), count3
    assert count1 == launches(shape, path, dtype, B.BATCH, GROUP, 1), count1
    want = B.reference(tuple(shape), time_scale, stirred)
    assert np.isfinite(one).all() and np.isfinite(three).all()
    d1, d3 = B.dist(one, want[0]), B.dist(three, want[1])
    tag = f"{'stirred' if stirred else 'frozen'} {np.dtype(dtype).name} {shape} {path} ts={time_scale}"
    if np.dtype(dtype) == np.float64:
        print(f"{tag}: 1 step {d1:.3e}, {B.STEPS} steps {d3:.3e}")
        return (d1, d3), (B.GATE64, B.GATE64)
    (own1, gate1), (own3, gate3) = B.gates32(tuple(shape), time_scale, stirred)
    print(f"{tag}: 1 step {d1:.3e} (complex64 reference {own1:.3e}, ratio {d1 / own1:.2f}), "
          f"{B.STEPS} steps {d3:.3e} (complex64 reference {own3:.3e}, ratio {d3 / own3:.2f})")
    return (d1, d3), (gate1, gate3)


# the precision varies fastest: the two precisions of a case share its references (gpe_rot_broadband_ref.reference)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("time_scale", B.TIME_SCALES)
@pytest.mark.parametrize("shape,path", B.FROZEN_CASES)
def test_frozen_white_noise(shape, path, time_scale, dtype):
    """rot_col FIRST / JOIN / LAST and rot_row at every line length, rot_mul and rot_b on rocFFT's plans"""
    (d1, d3), (gate1, gate3) = check_against_the_reference(shape, path, time_scale, dtype, False)
    # measured on the MI355X over these 36 cases, 1 step / 3 steps.  fp64: 7.8e-16 .. 2.7e-15 / 1.9e-15 .. 7.5e-15.
    # fp32: 3.0e-7 .. 1.6e-6 / 6.3e-7 .. 4.5e-6 against 2.8e-7 .. 9.4e-7 / 5.5e-7 .. 2.6e-6 of the complex64 reference:
    # 0.87 .. 4.2 / 0.93 .. 6.0 x the reference's on the same case (the gate is 8 x).  The largest ratios are the
    # 1024-point lines away from real time, (64, 1024) at -1j first: there the device's distance grows in step with the
    # number of steps (1.5e-6, 4.5e-6) and the reference's with its root (3.8e-7, 7.6e-7).  Lines of up to 256 points,
    # frozen and stirred: under 3.9 x.
    assert d1 <= gate1 and d3 <= gate3


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("time_scale", B.TIME_SCALES)
@pytest.mark.parametrize("shape,path", B.STIR_CASES)
def test_stirred_white_noise(shape, path, time_scale, dtype):
    """the rstir_ kernels: Omega(t) per environment in the line operators (the JOIN's two halves at their own local
    times), two moving spots and an anisotropy per environment in b, from the local time T0"""
    (d1, d3), (gate1, gate3) = check_against_the_reference(shape, path, time_scale, dtype, True)
    # measured on the MI355X over these 18 cases, 1 step / 3 steps.  fp64: 7.7e-16 .. 2.8e-15 / 1.9e-15 .. 7.9e-15.
    # fp32: 3.2e-7 .. 1.6e-6 / 5.7e-7 .. 4.6e-6 against 3.0e-7 .. 1.1e-6 / 5.4e-7 .. 2.7e-6 of the complex64 reference:
    # 1.06 .. 4.0 / 0.94 .. 6.95 x the reference's on the same case (the gate is 8 x); the largest is (64, 1024) at -1j
    # after 3 steps, 4.48e-6 against 6.45e-7, then (64, 1024) at 0.3 - 1j (5.95 x) and (1024, 64) at -1j (5.84 x).
    assert d1 <= gate1 and d3 <= gate3


# ---- bitwise properties on white noise -----------------------------------------------------------------------------

BITWISE = [(s, d, st) for s, d in B.BITWISE_CASES for st in (False, True)]
BITWISE_TS = 0.3 - 1j


@functools.lru_cache(maxsize=None)
def whole_batch(shape, dtype, stirred):
    """advance(STEPS) of the whole batch in windows of GROUP, computed once and shared by the three tests below"""
    eng, integ, y0, t0 = engine_for(shape, "fused", BITWISE_TS, dtype, stirred)
    try:
        out, _ = advance(eng, integ, y0, t0, (B.STEPS,))
        assert eng.last_kernel == kernel_name("fused", stirred)
    finally:
        eng.close()
    out.flags.writeable = False
    return out


@pytest.mark.parametrize("shape,dtype,stirred", BITWISE)
def test_advance_n_is_n_single_advances_bitwise(shape, dtype, stirred):
    """FIRST, JOIN, JOIN, LAST against three times FIRST, LAST"""
    eng, integ, y0, t0 = engine_for(shape, "fused", BITWISE_TS, dtype, stirred)
    try:
        singles, counts = advance(eng, integ, y0, t0, (1,) * B.STEPS)
    finally:
        eng.close()
    assert counts == [launches(shape, "fused", dtype, B.BATCH, GROUP, 1)] * B.STEPS
    assert np.array_equal(singles, whole_batch(shape, dtype, stirred))


@pytest.mark.parametrize("shape,dtype,stirred", BITWISE)
def test_a_repeat_is_identical(shape, dtype, stirred):
    eng, integ, y0, t0 = engine_for(shape, "fused", BITWISE_TS, dtype, stirred)
    try:
        first, _ = advance(eng, integ, y0, t0, (B.STEPS,))
        again, _ = advance(eng, integ, y0, t0, (B.STEPS,))
    finally:
        eng.close()
    assert np.array_equal(first, again)
    assert np.array_equal(first, whole_batch(shape, dtype, stirred))  # another engine, the same bits


@pytest.mark.parametrize("shape,dtype,stirred", BITWISE)
def test_the_batch_is_its_single_environment_runs_bitwise(shape, dtype, stirred):
    """per-environment k, Omega (and rate, spots, potential) are indexed by the environment, windows or not"""
    batch = whole_batch(shape, dtype, stirred)
    for b in range(B.BATCH):
        eng, integ, y0, t0 = engine_for(shape, "fused", BITWISE_TS, dtype, stirred, envs=(b,))
        try:
            one, (count,) = advance(eng, integ, y0, t0, (B.STEPS,))
        finally:
            eng.close()
        assert count == launches(shape, "fused", dtype, 1, GROUP, B.STEPS)
        assert np.array_equal(one[0], batch[b]), b
    assert not np.array_equal(batch[0], batch[1])
