"""The adjoint of the stirred, ramped rotating-frame split step on the MI355X (csrc/gpe_rot_adjoint.hip,
gpe_control.RotStirControlSolver, PDEModel.stirring_gradient / optimize_stirring) against the
torch autograd reference on the CPU (tests/gpe_rot_stir_adjoint_ref.py): one backward substep with per-environment k, e,
omega, rate and spots, the gradient of a whole solve with chunked recomputation, its bitwise properties, the frozen case
against the older entry, the library's refusals, and an optimisation end to end.  States and cotangents are white noise."""
import functools

import numpy as np
import pytest
import torch

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd import fit
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.gpe_control import CHUNK_BYTES_ENV, STIR_NAMES
from pde_opt_amd.numerics.functions.lights import SPOT_NUMBERS, GaussianSpot, GaussianSpots
from pde_opt_amd.utils import prepare_solver_params

import gpe_rot_stir_adjoint_ref as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

BOX = ((-2.0, 2.0), (-1.5, 1.5))  # hx != hy
K, E, OMEGA, RATE, DT, T0 = 50.0, 0.1, 0.5, 0.9, 0.02, 0.3  # those of test_gpu_gpe_rot_stir.py
SPOT_COLUMNS = SPOT_NUMBERS[:6] + ("inv_two_w2",)  # the library's block


def domain(points):
    return P.Domain(tuple(points), BOX, "dimensionless")


def spots_of(b, n=2):
    """n moving spots of environment b: off-centre, placed and moving differently in x and y"""
    four = [GaussianSpot(3.0 + b, 0.5, -0.6 + 0.1 * b, 0.8, 0.3 - 0.07 * b, -0.4, 0.35),
            GaussianSpot(-2.0, 1.0 + b, 0.7, -0.5 - 0.2 * b, -0.45, 0.6 + 0.1 * b, 0.25 + 0.05 * b),
            GaussianSpot(1.5, -0.7, -1.1, 0.3, -0.8, 0.9, 0.45), GaussianSpot(-2.5, 0.4, 1.2, -0.6, 0.7, -0.2, 0.3)]
    return GaussianSpots(four[:n])


def params_of(b, variant="both", n=2):
    """(k, e, omega, lights, omega_rate) of environment b: all of them differ between the environments of a batch"""
    lights = spots_of(b, n) if variant in ("both", "spots") else None
    rate = (RATE - 0.7 * b) if variant in ("both", "ramp") else 0.0
    return dict(k=K + 7.0 * b, e=E + 0.05 * b, omega=OMEGA - 0.3 * b, lights=lights, omega_rate=rate)


def reference_inputs(B, variant, n=2):
    """(p (B, 4), spots (B, S, 7) in the library's order or None)"""
    ps = [params_of(b, variant, n) for b in range(B)]
    p = np.array([[q["k"], q["e"], q["omega"], q["omega_rate"]] for q in ps])
    spots = np.stack([q["lights"].table(n) for q in ps]) if ps[0]["lights"] is not None else None
    return p, spots


def solver_of(eq, time_scale):
    return P.RotatingStrangSplitting(**prepare_solver_params(P.RotatingStrangSplitting, {"time_scale": time_scale}, eq))


def fields(points, B, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B,) + tuple(points) + (2,)), rng.standard_normal((B,) + tuple(points) + (2,))


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def quantities(lam, grad, spot_grad):
    """every gated quantity by name: lam0, the four scalars' columns over the batch, the spots' seven columns"""
    out = {"lam0": lam}
    out.update({n: grad[:, j] for j, n in enumerate(STIR_NAMES)})
    if spot_grad is not None:
        out.update({"spot " + n: spot_grad[..., j] for j, n in enumerate(SPOT_COLUMNS)})
    return out


# ---- one backward substep ------------------------------------------------------------------------------------------------

# (64, 64): the grid of the forward step's register / LDS passes; (48, 40): ragged, no power of two; (64, 128): nx != ny
GRIDS = [((64, 64), 1), ((64, 64), 3), ((48, 40), 1), ((48, 40), 3), ((64, 128), 2)]
TIME_SCALES = [1.0, -1j, 0.3 - 1j]
VARIANTS = ["both", "spots", "ramp", "none"]
STEP_CASES = [(p, b, ts, v, 2) for p, b in GRIDS for ts in TIME_SCALES for v in VARIANTS]
STEP_CASES.append(((48, 40), 1, 0.3 - 1j, "both", 4))  # PDEOPT_MAX_SPOTS spots: the full accumulator loop
SEED = 1  # of the cases that are not gated against the complex64 reference
FP32_FLOOR = 2.0 ** -23  # fp32's epsilon


@functools.lru_cache(maxsize=None)
def seed_of(points, B, time_scale, variant, n):
    """The seed of a case's white noise, chosen from the CPU reference alone, on the machine that runs the test.  The
    fp32 gate is a multiple of the complex64 reference's own distance from complex128, and with one environment that
    distance is the error of ONE sum: over 61 cases x 12 quantities some land far below fp32's resolution by accident
    (measured: 5e-9 for e at 64 x 64 x 1 in imaginary time), a gate no fp32 code can meet and no statement about the
    code; which cases do depends on the CPU's transforms, so a list of seeds fixed on one machine does not carry to
    another (the same case and seed: 2.5e-7 on one CPU, 5.0e-9 on another).  So a case takes the smallest seed for which
    every quantity's complex64 distance is at least fp32's epsilon 2^-23 -- one rounding of the result alone can be half
    of that -- and no entry of the complex128 gradient blocks is below 1e-3 of its block's largest (no quantity is a
    cancellation of its own terms).  The code under test plays no part in the choice."""
    for seed in range(1, 200):
        ref, ref32 = step_reference(points, B, time_scale, variant, n, seed, True), step_reference(points, B, time_scale, variant, n, seed, False)
        blocks = [np.stack([ref[k] for k in STIR_NAMES], -1)]
        if "spot amp0" in ref:
            blocks.append(np.stack([ref["spot " + k] for k in SPOT_COLUMNS], -1))
        if (all(rel(ref32[k], ref[k]) >= FP32_FLOOR for k in ref) and
                all(np.min(np.abs(blk)) >= 1e-3 * np.max(np.abs(blk)) for blk in blocks)):
            return seed
    raise AssertionError("no seed below 200 gives a complex64 reference free of cancellation artefacts")



@functools.lru_cache(maxsize=None)
def step_reference(points, B, time_scale, variant, n, seed, double):
    y0, lam1 = fields(points, B, seed)
    p, spots = reference_inputs(B, variant, n)
    g, gs, lam0 = A.step_vjp(A.Case(domain(points), time_scale, double), y0, p, spots, DT, T0, lam1)
    return quantities(lam0, g, gs)


def configured_engine(points, B, time_scale, dtype, variant, n=2):
    eqs = [P.GPE2DTSRot(domain(points), **params_of(b, variant, n)) for b in range(B)]
    eng = HipEngine(0)
    eng.configure(dtype=np.dtype(dtype), batch=B, **eqs[0]._engine_problem())
    P.GPE2DTSRot._engine_upload_batch(eng, eqs, T0, T0 + 1.0)
    solver_of(eqs[0], time_scale).configure_engine(eng, eqs[0])
    return eng, eqs


def device_step(points, B, time_scale, variant, n, seed, dtype, host_blocks=False):
    y0, lam1 = fields(points, B, seed)
    eng, _ = configured_engine(points, B, time_scale, dtype, variant, n)
    eng.set_state(y0.astype(dtype))
    lam = torch.as_tensor(lam1.astype(dtype)).to(DEV)
    has_spots = variant in ("both", "spots")
    if host_blocks:
        grad, sg = np.zeros((B, 4)), (np.zeros((B, n, 7)) if has_spots else None)
        ptrs = grad.ctypes.data, (sg.ctypes.data if has_spots else 0)
    else:
        grad = torch.zeros((B, 4), dtype=torch.float64, device=DEV)
        sg = torch.zeros((B, n, 7), dtype=torch.float64, device=DEV) if has_spots else None
        ptrs = grad.data_ptr(), (sg.data_ptr() if has_spots else 0)
    torch.cuda.synchronize()
    eng.gpe_rot_stir_adjoint_step(T0, DT, eng.state_device_ptr()[0], lam.data_ptr(), *ptrs)
    eng.sync()
    assert eng.last_kernel == "strang_rot_stir_adjoint_rocfft_1d"
    if not host_blocks:
        grad, sg = grad.cpu().numpy(), (sg.cpu().numpy() if has_spots else None)
    return quantities(lam.double().cpu().numpy(), grad, sg)


@pytest.mark.parametrize("points,B,time_scale,variant,n", STEP_CASES)
def test_backward_substep_fp64(points, B, time_scale, variant, n):
    seed = seed_of(points, B, time_scale, variant, n)
    ref = step_reference(points, B, time_scale, variant, n, seed, True)
    got = device_step(points, B, time_scale, variant, n, seed, np.float64)
    assert got.keys() == ref.keys()
    errs = {name: rel(got[name], ref[name]) for name in ref}
    print(f"fp64 substep {points} B={B} ts={time_scale} {variant} S={n}: " + " ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    # rounding of a few dozen transforms, relative to the largest component of each quantity over the batch: the gate
    # of test_gpu_gpe_rot_adjoint.py
    for name, e in errs.items():
        assert e <= 1e-10, name


# Measured on the MI355X over STEP_CASES, largest ratio of the device's distance to the complex64 reference's: lam0 2.0,
# k 4.1, e 7.4, omega 2.9, omega_rate 2.8, spot amp0 3.3, amp_rate 3.0, x0 6.2, x_rate 5.0, inv_two_w2 5.0 -- and spot y0
# 10.9, y_rate 9.5, both at 48 x 40 x 1 in imaginary time, spots only (device 2.6e-6, reference 2.4e-7 / 2.7e-7).  Read
# from the code: spots_value and spot_partials take exp through the fast __expf (common.hpp t_exp_neg<float>), whose
# argument is scaled by log2(e) in fp32 first -- a relative error of about |r^2 c| 2^-24 with one sign over a spot, which
# a sum over the spot does not average away, and the forward step's own potential carries it too; the complex64
# reference rounds exp correctly.  These two quantities alone are gated at twice their measured ratio.
FP32_WIDER = {"spot y0": 2 * 10.85, "spot y_rate": 2 * 9.45}


@pytest.mark.parametrize("points,B,time_scale,variant,n", STEP_CASES)
def test_backward_substep_fp32(points, B, time_scale, variant, n):
    seed = seed_of(points, B, time_scale, variant, n)
    ref = step_reference(points, B, time_scale, variant, n, seed, True)
    ref32 = step_reference(points, B, time_scale, variant, n, seed, False)
    got = device_step(points, B, time_scale, variant, n, seed, np.float32)
    gates = {name: rel(ref32[name], ref[name]) for name in ref}
    errs = {name: rel(got[name], ref[name]) for name in ref}
    print(f"fp32 substep {points} B={B} ts={time_scale} {variant} S={n} seed {seed}: " +
          " ".join(f"{k} {errs[k]:.3e} (complex64 reference {gates[k]:.3e}, ratio {errs[k] / gates[k]:.2f})" for k in ref))
    # each quantity within 8 x the distance of the reference at complex64 from itself at complex128 on this case; the two
    # quantities of FP32_WIDER alone at twice their measured ratio
    for name in ref:
        assert errs[name] <= FP32_WIDER.get(name, 8.0) * gates[name], name


def test_host_blocks_equal_the_device_ones():
    case = ((48, 40), 3, 1.0, "both", 2, SEED)
    dev = device_step(*case, np.float64)
    host = device_step(*case, np.float64, host_blocks=True)
    for name in dev:
        np.testing.assert_array_equal(dev[name], host[name], err_msg=name)


def test_frozen_case_agrees_with_the_older_entry():
    """no spots, rate 0: lam0 and (k, e, omega) are pdeopt_gpe_rot_adjoint_step's to 1e-12 of each quantity's magnitude (the
    line coefficient is formed in another order, Omega0 (w coord) against (w Omega) coord: rounding, no more), and the
    rate entry is t0 x the omega entry, formed from the one sum"""
    points, B = (48, 40), 3
    new = device_step(points, B, 0.3 - 1j, "none", 2, SEED, np.float64)
    y0, lam1 = fields(points, B, SEED)
    eng, _ = configured_engine(points, B, 0.3 - 1j, np.float64, "none")
    eng.set_state(y0)
    lam = torch.as_tensor(lam1).to(DEV)
    grad = torch.zeros((B, 3), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    eng.gpe_rot_adjoint_step(DT, eng.state_device_ptr()[0], lam.data_ptr(), grad.data_ptr())
    eng.sync()
    old = grad.cpu().numpy()
    assert rel(new["lam0"], lam.cpu().numpy()) <= 1e-12
    for j, name in enumerate(("k", "e", "omega")):
        assert rel(new[name], old[:, j]) <= 1e-12, name
    np.testing.assert_array_equal(new["omega_rate"], T0 * new["omega"])


# ---- the whole gradient -----------------------------------------------------------------------------------------------

POINTS, DT0 = (48, 40), 0.02
TS = 0.3 + DT0 * np.array([0.0, 3.0, 4.4, 6.5])  # a step edge, a save inside a step, a clipped 7th substep
TIME_SCALE = 0.3 - 1j


def shared():
    return params_of(0, "both")


def weights():
    rng = np.random.default_rng(11)
    return torch.as_tensor(rng.standard_normal((len(TS), 2) + POINTS + (2,)))


def objective(ys):
    return (ys * weights()).sum() + 0.5 * (ys[-1] ** 2).sum()


class Recording:
    """objective as a value_and_grad object that keeps the solution it was given"""

    def __init__(self):
        self.inner = fit.torch_objective(objective)

    def value_and_grad(self, ys):
        self.ys = np.array(ys)
        return self.inner.value_and_grad(ys)


@functools.lru_cache(maxsize=None)
def solve_reference(double):
    """per environment: grad (2, 4), the spots' block (2, 2, 7) in USER units (last column d/d width), lam0"""
    y0, _ = fields(POINTS, 2, SEED)
    p, spots = reference_inputs(1, "both")
    p, spots = np.repeat(p, 2, axis=0), np.repeat(spots, 2, axis=0)
    J, ys, g, gs, lam0 = A.solve_grad(A.Case(domain(POINTS), TIME_SCALE, double), y0, p, spots, TS, DT0, objective)
    w = np.array([s.width for s in shared()["lights"].spots])
    gs = gs.copy()
    gs[..., 6] *= -1.0 / w**3  # inv_two_w2 = 1 / (2 w^2)
    return J, ys, g, gs, lam0


def model():
    return P.PDEModel(P.GPE2DTSRot, domain(POINTS), P.RotatingStrangSplitting)


def device_gradient(dtype, cap=None, monkeypatch=None, per_environment=False):
    m = model()
    y0 = fields(POINTS, 2, SEED)[0].astype(dtype)
    if cap is not None:
        monkeypatch.setenv(CHUNK_BYTES_ENV, str(cap))
    obj = Recording()
    J, grad, lam0 = m.stirring_gradient(obj, y0, TS, shared(), {"time_scale": TIME_SCALE}, dt0=DT0, per_environment=per_environment)
    assert list(grad) == list(STIR_NAMES) + ["lights"]
    return m, y0, obj.ys, J, np.stack([grad[n] for n in STIR_NAMES], axis=-1), grad["lights"], lam0


def whole_errors(grad, lights, lam0, ref):
    _, _, g_ref, gs_ref, l_ref = ref
    tot, stot = g_ref[0] + g_ref[1], gs_ref[0] + gs_ref[1]
    errs = {"lam0": rel(lam0, l_ref)}
    errs.update({n: abs(grad[j] - tot[j]) / abs(tot[j]) for j, n in enumerate(STIR_NAMES)})
    errs.update({"spot " + n: rel(lights[:, j], stot[:, j]) for j, n in enumerate(SPOT_NUMBERS)})
    return errs


def test_whole_gradient_fp64_and_its_bitwise_properties(monkeypatch):
    ref = solve_reference(True)
    m, y0, ys, J, grad, lights, lam0 = device_gradient(np.float64)
    assert m.rot_stir_control_solver().last_chunks == 1
    errs = whole_errors(grad, lights, lam0, ref)
    print(f"fp64 whole gradient: J {abs(J - ref[0]) / abs(ref[0]):.3e} " + " ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    assert grad.shape == (4,) and lights.shape == (2, 7) and lam0.shape == y0.shape
    for name, e in errs.items():
        assert e <= 1e-10, name
    # the objective saw the array solve returns
    np.testing.assert_array_equal(ys, m.solve(shared(), y0, TS, {"time_scale": TIME_SCALE}, dt0=DT0))
    # a repeat gives the same bits
    _, _, _, J2, grad2, lights2, lam02 = device_gradient(np.float64)
    assert J2 == J
    np.testing.assert_array_equal(grad2, grad)
    np.testing.assert_array_equal(lights2, lights)
    np.testing.assert_array_equal(lam02, lam0)
    # three chunks (3 + 3 + 1 substeps) give the same bits as one
    m3, _, _, J3, grad3, lights3, lam03 = device_gradient(np.float64, cap=3 * y0.nbytes, monkeypatch=monkeypatch)
    assert m3.rot_stir_control_solver().last_chunks == 3
    assert J3 == J
    np.testing.assert_array_equal(grad3, grad)
    np.testing.assert_array_equal(lights3, lights)
    np.testing.assert_array_equal(lam03, lam0)


def test_whole_gradient_per_environment_sums_to_the_shared_one():
    _, _, g_ref, gs_ref, _ = solve_reference(True)
    _, _, _, _, per, per_lights, _ = device_gradient(np.float64, per_environment=True)
    _, _, _, _, tot, tot_lights, _ = device_gradient(np.float64)
    assert per.shape == (2, 4) and per_lights.shape == (2, 2, 7)
    np.testing.assert_array_equal(per[0] + per[1], tot)
    np.testing.assert_array_equal(per_lights[0] + per_lights[1], tot_lights)
    for j in range(4):
        assert rel(per[:, j], g_ref[:, j]) <= 1e-10
    for j in range(7):
        assert rel(per_lights[..., j], gs_ref[..., j]) <= 1e-10


def test_whole_gradient_fp32():
    ref, ref32 = solve_reference(True), solve_reference(False)
    _, _, _, _, grad, lights, lam0 = device_gradient(np.float32)
    errs = whole_errors(grad, lights, lam0, ref)
    tot32, stot32 = ref32[2][0] + ref32[2][1], ref32[3][0] + ref32[3][1]
    gates = whole_errors(tot32, stot32, ref32[4], ref)
    print("fp32 whole gradient: " +
          " ".join(f"{k} {errs[k]:.3e} (complex64 reference {gates[k]:.3e}, ratio {errs[k] / gates[k]:.2f})" for k in errs))
    # 8 x the complex64 reference's own distance from complex128 on this case
    for name in errs:
        assert errs[name] <= 8 * gates[name], name


# ---- the library's refusals ---------------------------------------------------------------------------------------------


def refused(eng, lam, grad, sg, psi0=None, dt=DT, match=None):
    """the engine turns PDEOPT_EINVAL into ValueError and every other status into PdeoptError"""
    with pytest.raises((ValueError, L.PdeoptError), match=match) as e:
        eng.gpe_rot_stir_adjoint_step(T0, dt, psi0 if psi0 is not None else eng.state_device_ptr()[0], lam.data_ptr(),
                                      grad if isinstance(grad, int) else grad.data_ptr(),
                                      sg if isinstance(sg, int) else sg.data_ptr())
    return L.EINVAL if isinstance(e.value, ValueError) else e.value.code


def test_library_refusals():
    points, B = (48, 40), 2
    eqs = [P.GPE2DTSRot(domain(points), **params_of(b, "both")) for b in range(B)]
    solver = solver_of(eqs[0], 1.0)
    lam1 = torch.as_tensor(fields(points, B, SEED)[1]).to(DEV)
    lam = lam1.clone()
    grad = torch.zeros((B, 4), dtype=torch.float64, device=DEV)
    sg = torch.zeros((B, 2, 7), dtype=torch.float64, device=DEV)
    host_grad, host_sg = np.zeros((B, 4)), np.zeros((B, 2, 7))
    torch.cuda.synchronize()
    # another equation
    eng = HipEngine(0)
    ch = P.CahnHilliard2DPeriodic(domain(points), 0.01, lambda c: c**3 - c, lambda c: 1.0)
    eng.configure(dtype=np.dtype(np.float64), batch=B, **ch._engine_problem())
    assert refused(eng, lam, grad, sg, match="needs the GPE") == L.EINVAL
    # the rotation not set
    eng = HipEngine(0)
    eng.configure(dtype=np.dtype(np.float64), batch=B, **eqs[0]._engine_problem())
    eng.set_aux(L.AUX_GPE_POTENTIAL, eqs[0].trap_potential())
    solver.configure_engine(eng, eqs[0])
    eng.set_state(np.ones((B,) + points + (2,)))
    assert refused(eng, lam, grad, 0, match="pdeopt_set_gpe_rotation") == L.ESTATE
    P.GPE2DTSRot._engine_upload_batch(eng, eqs, T0, T0 + 1.0)
    psi0 = eng.state_device_ptr()[0]
    # the spots' block missing while spots are set, and given while none are
    assert refused(eng, lam, grad, 0, match="not NULL") == L.EINVAL
    eng.set_gpe_spots(None)
    assert refused(eng, lam, grad, sg, match="must be NULL") == L.EINVAL
    P.GPE2DTSRot._engine_upload_batch(eng, eqs, T0, T0 + 1.0)
    # a non-positive dt
    assert refused(eng, lam, grad, sg, dt=0.0, match="dt = 0") == L.EINVAL
    assert refused(eng, lam, grad, sg, dt=-DT, match="dt = -0.02") == L.EINVAL
    # one block on the device, one on the host
    assert refused(eng, lam, grad, host_sg.ctypes.data, match="both device memory or both host memory") == L.EINVAL
    assert refused(eng, lam, host_grad.ctypes.data, sg, match="both device memory or both host memory") == L.EINVAL
    # misaligned and overlapping pointers
    assert refused(eng, lam, grad.data_ptr() + 4, sg, match="aligned") == L.EINVAL
    assert refused(eng, lam, grad, sg.data_ptr() + 4, match="aligned") == L.EINVAL
    assert refused(eng, lam, grad, sg, psi0=lam.data_ptr(), match="overlap") == L.EINVAL
    assert refused(eng, lam, lam.data_ptr(), sg, match="overlap") == L.EINVAL
    assert refused(eng, lam, grad, lam.data_ptr(), match="overlap") == L.EINVAL
    assert refused(eng, lam, sg.data_ptr(), sg, match="overlap") == L.EINVAL
    # a potential from a host callable
    eng.set_aux_time_fn(L.AUX_GPE_POTENTIAL, lambda t: eqs[0].trap_potential())
    assert refused(eng, lam, grad, sg, match="host callable") == L.EINVAL
    # every refusal left lam untouched and both blocks zero
    eng.sync()
    assert torch.equal(lam, lam1) and not grad.any() and not sg.any() and not host_grad.any() and not host_sg.any()
    # and the supported call on the same engine still runs
    P.GPE2DTSRot._engine_upload_batch(eng, eqs, T0, T0 + 1.0)
    eng.gpe_rot_stir_adjoint_step(T0, DT, psi0, lam.data_ptr(), grad.data_ptr(), sg.data_ptr())
    eng.sync()
    assert np.all(np.isfinite(grad.cpu().numpy())) and np.all(np.isfinite(sg.cpu().numpy())) and not torch.equal(lam, lam1)
    # the older entry keeps refusing spots and a ramp
    g3 = torch.zeros((B, 3), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="no light spots"):
        eng.gpe_rot_adjoint_step(DT, psi0, lam.data_ptr(), g3.data_ptr())
    eng.set_gpe_spots(None)
    with pytest.raises(ValueError, match="constant Omega"):
        eng.gpe_rot_adjoint_step(DT, psi0, lam.data_ptr(), g3.data_ptr())


# ---- an optimisation ----------------------------------------------------------------------------------------------------

import gpe_rot_stir_fit_problem as C  # noqa: E402  (the case; the CPU reference run that meets the same bounds is recorded there)


def test_optimisation_recovers_the_ramp_and_the_beam_speed():
    m = P.PDEModel(P.GPE2DTSRot, C.domain(), P.RotatingStrangSplitting)
    fitted = m.optimize_stirring(C.objective, C.y0(), C.TS, {"omega_rate": C.RATE_START, "lights": C.lights(C.XRATE_START)},
                                 C.fixed(), max_steps=C.MAX_STEPS, dt0=C.DT0)
    hist = m.last_optimize_history
    spot = fitted["lights"].spots[0]
    print("J per accepted step:", " ".join(f"{v:.6e}" for v in hist), "omega_rate", fitted["omega_rate"], "x_rate", spot.x_rate)
    assert hist[-1] <= 1e-6 * hist[0]
    assert abs(fitted["omega_rate"] - C.RATE_TRUE) <= 1e-3
    assert abs(spot.x_rate - C.XRATE_TRUE) <= 1e-3
    # the fixed parameters and the beam's fixed numbers come back unchanged
    assert all(fitted[n] == v for n, v in C.fixed().items())
    start = C.lights(C.XRATE_START).spots[0]
    assert all(getattr(spot, n) == getattr(start, n) for n in SPOT_NUMBERS if n != "x_rate")
