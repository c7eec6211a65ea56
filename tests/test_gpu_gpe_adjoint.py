"""The adjoint of the GPE's Strang step on the MI355X (csrc/gpe_adjoint.hip, pde_opt_amd.gpe_control) against the torch
autograd reference on the CPU (tests/gpe_adjoint_ref.py): one backward substep, the gradient of a whole solve with
chunked recomputation, its bitwise properties, the library's refusals, and an optimisation end to end."""
import functools

import numpy as np
import pytest
import torch

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd import fit
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.gpe_control import CHUNK_BYTES_ENV, SpotMap
from pde_opt_amd.numerics.functions.lights import GaussianSpot, GaussianSpots
from pde_opt_amd.utils import prepare_solver_params

import gpe_adjoint_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

K_GPE, E_GPE, TRAP = 1.3, 0.2, 0.7
BOX = ((-2.0, 2.0), (-1.5, 1.5))
ALL_SPOTS = np.array([[1.5, -0.8, 0.4, 0.9, -0.3, 0.5, 0.6], [-0.7, 0.4, -0.8, -0.6, 0.5, 0.3, 0.9],
                      [0.9, 0.5, -0.2, 0.3, -0.6, -0.4, 0.5], [-1.1, -0.3, 0.7, -0.5, 0.2, 0.6, 0.8]])


def spots_of(p, free=None):
    return GaussianSpots([GaussianSpot(*(float(v) for v in row)) for row in np.asarray(p).reshape(-1, 7)], free=free)


def parameters(p, **kw):
    return dict(k=K_GPE, e=E_GPE, lights=spots_of(p), trap_factor=TRAP, kinetic=True, **kw)


def build(points, p, time_scale):
    eq = P.GPE2DTSControl(P.Domain(tuple(points), BOX, "dimensionless"), **parameters(p))
    solver = P.StrangSplitting(**prepare_solver_params(P.StrangSplitting, {"time_scale": time_scale}, eq))
    return eq, solver


def fields(points, B, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B,) + tuple(points) + (2,)), rng.standard_normal((B,) + tuple(points) + (2,))


# ---- one backward substep ------------------------------------------------------------------------------------------------

T0, DT = 0.3, 0.02
STEP_CASES = [((64, 64), 1, 1, 1.0), ((64, 64), 3, 4, -1j), ((48, 40), 1, 2, -1j), ((48, 40), 3, 4, 1.0), ((48, 40), 3, 1, 0.3 - 1j),
              # the other line lengths of the LDS transforms, nx != ny
              ((128, 256), 2, 2, 0.3 - 1j), ((256, 64), 1, 1, 1.0)]


@functools.lru_cache(maxsize=None)
def step_reference(points, B, S, time_scale, double):
    eq, solver = build(points, ALL_SPOTS[:S], time_scale)
    y0, lam1 = fields(points, B, 7)
    _, per, lam0 = R.step_vjp(R.Case.of(eq, solver, double), y0, ALL_SPOTS[:S], T0, DT, lam1)
    return per, lam0


def device_step(points, B, S, time_scale, dtype, host_grad=False):
    eq, solver = build(points, ALL_SPOTS[:S], time_scale)
    y0, lam1 = fields(points, B, 7)
    eng = HipEngine(0)
    eng.configure(dtype=np.dtype(dtype), batch=B, **eq._engine_problem())
    eq._engine_upload(eng, T0, T0 + DT)
    solver.configure_engine(eng, eq)
    eng.set_state(y0.astype(dtype))
    lam = torch.as_tensor(lam1.astype(dtype)).to(DEV)
    grad = np.zeros((B, S, 7)) if host_grad else torch.zeros((B, S, 7), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    eng.gpe_adjoint_step(T0, DT, eng.state_device_ptr()[0], lam.data_ptr(), grad.ctypes.data if host_grad else grad.data_ptr())
    eng.sync()
    raw = grad if host_grad else grad.cpu().numpy()
    return SpotMap.user_gradient(spots_of(ALL_SPOTS[:S]), raw), lam.double().cpu().numpy()


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("points,B,S,time_scale", STEP_CASES)
def test_backward_substep_fp64(points, B, S, time_scale):
    per, lam0 = step_reference(points, B, S, time_scale, True)
    grad, lam = device_step(points, B, S, time_scale, np.float64)
    print(f"fp64 substep {points} B={B} S={S} ts={time_scale}: grad {rel(grad, per):.3e} lam0 {rel(lam, lam0):.3e}")
    # rounding of a few dozen transforms, relative to the largest component
    assert rel(grad, per) <= 1e-10
    assert rel(lam, lam0) <= 1e-10


@pytest.mark.parametrize("points,B,S,time_scale", STEP_CASES)
def test_backward_substep_fp32(points, B, S, time_scale):
    per, lam0 = step_reference(points, B, S, time_scale, True)
    per32, lam032 = step_reference(points, B, S, time_scale, False)
    grad, lam = device_step(points, B, S, time_scale, np.float32)
    ref_g, ref_l = rel(per32, per), rel(lam032, lam0)
    print(f"fp32 substep {points} B={B} S={S} ts={time_scale}: grad {rel(grad, per):.3e} (complex64 reference {ref_g:.3e}) "
          f"lam0 {rel(lam, lam0):.3e} (complex64 reference {ref_l:.3e})")
    # the gate is 8 x the distance of the reference at complex64 from itself at complex128 on this case (device
    # transforms round in another order).  The complex64 reference's distance,
    # measured on the CPU over these cases: gradient 1.0e-7 .. 3.2e-6, lam0 2.0e-7 .. 8.3e-6; the device's:
    # gradient 1.2e-7 .. 2.0e-6, lam0 2.0e-7 .. 4.9e-6 (at most 1.3 x the reference's on the same case)
    assert rel(grad, per) <= 8 * ref_g
    assert rel(lam, lam0) <= 8 * ref_l


def test_host_gradient_block_equals_the_device_one():
    case = STEP_CASES[3]
    g_dev, lam_dev = device_step(*case, np.float64)
    g_host, lam_host = device_step(*case, np.float64, host_grad=True)
    np.testing.assert_array_equal(g_dev, g_host)
    np.testing.assert_array_equal(lam_dev, lam_host)


# ---- the whole gradient -----------------------------------------------------------------------------------------------

POINTS, DT0 = (48, 40), 0.02
TS = np.array([0.1, 0.1 + 3 * DT0, 0.1 + 4.4 * DT0, 0.1 + 6.5 * DT0])  # a step edge, inside a step, a clipped 7th substep
P2 = ALL_SPOTS[:2]


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
    eq, solver = build(POINTS, P2, -1j)
    y0, _ = fields(POINTS, 2, 3)
    return R.solve_grad(R.Case.of(eq, solver, double), y0, P2, TS, DT0, objective)


def device_gradient(dtype, cap=None, monkeypatch=None):
    model = P.PDEModel(P.GPE2DTSControl, P.Domain(POINTS, BOX, "dimensionless"), P.StrangSplitting)
    y0, _ = fields(POINTS, 2, 3)
    y0 = y0.astype(dtype)
    if cap is not None:
        monkeypatch.setenv(CHUNK_BYTES_ENV, str(cap))
    obj = Recording()
    J, grad, lam0 = model.control_gradient(obj, y0, TS, parameters(P2), {"time_scale": -1j}, dt0=DT0)
    return model, y0, obj.ys, J, grad, lam0


def test_whole_gradient_fp64_and_its_bitwise_properties(monkeypatch):
    J_ref, ys_ref, g_ref, l_ref = solve_reference(True)
    model, y0, ys, J, grad, lam0 = device_gradient(np.float64)
    assert model.gpe_control_solver().last_chunks == 1
    print(f"fp64 whole gradient: J {abs(J - J_ref) / abs(J_ref):.3e} grad {rel(grad, g_ref):.3e} lam0 {rel(lam0, l_ref):.3e}")
    assert grad.shape == (2, 7) and lam0.shape == y0.shape
    assert rel(grad, g_ref) <= 1e-10
    assert rel(lam0, l_ref) <= 1e-10
    # the objective saw the array solve returns
    np.testing.assert_array_equal(ys, model.solve(parameters(P2), y0, TS, {"time_scale": -1j}, dt0=DT0))
    # a repeat gives the same bits
    _, _, _, J2, grad2, lam02 = device_gradient(np.float64)
    assert J2 == J
    np.testing.assert_array_equal(grad2, grad)
    np.testing.assert_array_equal(lam02, lam0)
    # three chunks (3 + 3 + 1 substeps) give the same bits as one
    m3, _, _, J3, grad3, lam03 = device_gradient(np.float64, cap=3 * y0.nbytes, monkeypatch=monkeypatch)
    assert m3.gpe_control_solver().last_chunks == 3
    assert J3 == J
    np.testing.assert_array_equal(grad3, grad)
    np.testing.assert_array_equal(lam03, lam0)


def test_whole_gradient_per_environment_sums_to_the_shared_one():
    model = P.PDEModel(P.GPE2DTSControl, P.Domain(POINTS, BOX, "dimensionless"), P.StrangSplitting)
    y0, _ = fields(POINTS, 2, 3)
    _, per, _ = model.control_gradient(objective, y0, TS, parameters(P2), {"time_scale": -1j}, dt0=DT0, per_environment=True)
    _, tot, _ = model.control_gradient(objective, y0, TS, parameters(P2), {"time_scale": -1j}, dt0=DT0)
    assert per.shape == (2, 2, 7)
    np.testing.assert_array_equal(per[0] + per[1], tot)


def test_whole_gradient_fp32():
    _, _, g_ref, l_ref = solve_reference(True)
    _, _, g32, l32 = solve_reference(False)
    _, _, _, _, grad, lam0 = device_gradient(np.float32)
    ref_g, ref_l = rel(g32, g_ref), rel(l32, l_ref)
    print(f"fp32 whole gradient: grad {rel(grad, g_ref):.3e} (complex64 reference {ref_g:.3e}) lam0 {rel(lam0, l_ref):.3e} "
          f"(complex64 reference {ref_l:.3e})")
    # 8 x the complex64 reference's own distance from complex128 on this case.  Measured on the CPU: gradient
    # 5.7e-7, lam0 1.4e-7; the device's: gradient 1.5e-6 (2.7 x), lam0 1.4e-7
    assert rel(grad, g_ref) <= 8 * ref_g
    assert rel(lam0, l_ref) <= 8 * ref_l


# ---- the library's refusals ---------------------------------------------------------------------------------------------


def refused(eng, lam, grad, psi0=None, match=None):
    """the engine turns PDEOPT_EINVAL into ValueError and every other status into PdeoptError"""
    with pytest.raises((ValueError, L.PdeoptError), match=match) as e:
        eng.gpe_adjoint_step(T0, DT, psi0 if psi0 is not None else eng.state_device_ptr()[0], lam.data_ptr(), grad.data_ptr())
    return L.EINVAL if isinstance(e.value, ValueError) else e.value.code


def test_library_refusals():
    points, B = (48, 40), 2
    eq, solver = build(points, ALL_SPOTS[:1], 1.0)
    lam = torch.zeros((B,) + points + (2,), dtype=torch.float64, device=DEV)
    grad = torch.zeros((B, 1, 7), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    # another equation
    eng = HipEngine(0)
    dom = P.Domain(points, BOX, "dimensionless")
    ch = P.CahnHilliard2DPeriodic(dom, 0.01, lambda c: c**3 - c, lambda c: 1.0)
    eng.configure(dtype=np.dtype(np.float64), batch=B, **ch._engine_problem())
    assert refused(eng, lam, grad, match="needs the GPE") == L.EINVAL
    # no spots set
    eng = HipEngine(0)
    eng.configure(dtype=np.dtype(np.float64), batch=B, **eq._engine_problem())
    eng.set_aux(L.AUX_GPE_POTENTIAL, eq.trap_potential())
    solver.configure_engine(eng, eq)
    eng.set_state(np.ones((B,) + points + (2,)))
    assert refused(eng, lam, grad, match="has set none") == L.ESTATE
    # overlapping buffers
    eq._engine_upload(eng, T0, T0 + DT)
    psi0 = eng.state_device_ptr()[0]
    with pytest.raises(ValueError, match="overlap"):
        eng.gpe_adjoint_step(T0, DT, psi0, psi0, grad.data_ptr())
    with pytest.raises(ValueError, match="overlap"):
        eng.gpe_adjoint_step(T0, DT, psi0, lam.data_ptr(), lam.data_ptr())
    # a potential from a host callable
    eng.set_aux_time_fn(L.AUX_GPE_POTENTIAL, lambda t: eq.trap_potential())
    assert refused(eng, lam, grad, match="host callable") == L.EINVAL
    eng.set_aux(L.AUX_GPE_POTENTIAL, eq.trap_potential())
    # a per-environment A_term
    eng.set_aux(L.AUX_GPE_A_TERM, np.stack([np.asarray(solver.A_term)] * B), per_env=True)
    assert refused(eng, lam, grad, match="shared by the batch") == L.EINVAL
    # and the supported call on the same engine still runs
    eng.set_aux(L.AUX_GPE_A_TERM, np.asarray(solver.A_term))
    eng.gpe_adjoint_step(T0, DT, psi0, lam.data_ptr(), grad.data_ptr())
    eng.sync()
    assert np.all(np.isfinite(grad.cpu().numpy()))


# ---- an optimisation ----------------------------------------------------------------------------------------------------

import gpe_control_problem as C  # noqa: E402  (the case and the recorded figure of the CPU reference run)


def test_optimisation_recovers_the_spot_position():
    model = P.PDEModel(P.GPE2DTSControl, C.domain(), P.StrangSplitting)
    fitted = model.optimize(C.objective, C.y0(), C.TS, {"lights": C.start_spots()}, C.other_parameters(), C.SOLVER_PARAMETERS,
                            max_steps=C.MAX_STEPS)
    hist = model.last_optimize_history
    print("J per accepted step:", " ".join(f"{v:.6e}" for v in hist))
    assert all(b < a for a, b in zip(hist, hist[1:]))
    assert hist[-1] <= 10 * C.REFERENCE_FINAL_J
    assert isinstance(fitted["lights"], GaussianSpots) and fitted["lights"].free == ("x0", "y0")
