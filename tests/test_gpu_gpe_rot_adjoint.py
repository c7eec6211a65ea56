"""The adjoint of the rotating-frame split step on the MI355X (csrc/gpe_rot_adjoint.hip, gpe_control.RotControlSolver,
PDEModel.rotation_gradient / optimize_rotation) against the torch autograd reference on the CPU
(tests/gpe_rot_adjoint_ref.py): one backward substep with per-environment k, e and omega, the gradient of a whole solve
with chunked recomputation, its bitwise properties, the library's refusals, and an optimisation end to end."""
import functools

import numpy as np
import pytest
import torch

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd import fit
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.gpe_control import CHUNK_BYTES_ENV, ROT_NAMES
from pde_opt_amd.utils import prepare_solver_params

import gpe_rot_adjoint_ref as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

BOX = ((-2.0, 2.0), (-1.5, 1.5))  # hx != hy
PARAMS = np.array([[1.3, 0.2, 0.6], [0.9, -0.1, -0.4], [2.1, 0.35, 0.85]])  # (k, e, omega) of environment 0, 1, 2
DT = 0.02


def equations(points, B):
    dom = P.Domain(tuple(points), BOX, "dimensionless")
    return [P.GPE2DTSRot(dom, *(float(v) for v in PARAMS[b])) for b in range(B)]


def solver_of(eq, time_scale):
    return P.RotatingStrangSplitting(**prepare_solver_params(P.RotatingStrangSplitting, {"time_scale": time_scale}, eq))


def fields(points, B, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B,) + tuple(points) + (2,)), rng.standard_normal((B,) + tuple(points) + (2,))


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- one backward substep ------------------------------------------------------------------------------------------------

# (64, 64): the grid of the forward step's register / LDS passes; (48, 40): ragged, no power of two; (64, 128): nx != ny
STEP_CASES = [((64, 64), 1, 1.0), ((64, 64), 3, -1j), ((48, 40), 3, 1.0), ((48, 40), 1, -1j), ((48, 40), 3, 0.3 - 1j),
              ((64, 128), 2, 1.0)]


@functools.lru_cache(maxsize=None)
def step_reference(points, B, time_scale, double):
    y0, lam1 = fields(points, B, 7)
    return A.step_vjp(A.Case(P.Domain(points, BOX, "dimensionless"), time_scale, double), y0, PARAMS[:B], DT, lam1)


def configured_engine(points, B, time_scale, dtype):
    eqs = equations(points, B)
    eng = HipEngine(0)
    eng.configure(dtype=np.dtype(dtype), batch=B, **eqs[0]._engine_problem())
    P.GPE2DTSRot._engine_upload_batch(eng, eqs, 0.0, DT)
    solver_of(eqs[0], time_scale).configure_engine(eng, eqs[0])
    return eng


def device_step(points, B, time_scale, dtype, host_grad=False):
    y0, lam1 = fields(points, B, 7)
    eng = configured_engine(points, B, time_scale, dtype)
    eng.set_state(y0.astype(dtype))
    lam = torch.as_tensor(lam1.astype(dtype)).to(DEV)
    grad = np.zeros((B, 3)) if host_grad else torch.zeros((B, 3), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    eng.gpe_rot_adjoint_step(DT, eng.state_device_ptr()[0], lam.data_ptr(), grad.ctypes.data if host_grad else grad.data_ptr())
    eng.sync()
    return (grad if host_grad else grad.cpu().numpy()), lam.double().cpu().numpy()


@pytest.mark.parametrize("points,B,time_scale", STEP_CASES)
def test_backward_substep_fp64(points, B, time_scale):
    g_ref, l_ref = step_reference(points, B, time_scale, True)
    grad, lam = device_step(points, B, time_scale, np.float64)
    errs = [rel(grad[:, j], g_ref[:, j]) for j in range(3)]
    print(f"fp64 substep {points} B={B} ts={time_scale}: lam0 {rel(lam, l_ref):.3e} " +
          " ".join(f"{n} {e:.3e}" for n, e in zip(ROT_NAMES, errs)))
    # rounding of a few dozen transforms, relative to the largest component of each quantity (the gate of
    # test_gpu_gpe_adjoint.py); the same order of operations in numpy on the CPU sits at <= 3e-13
    assert rel(lam, l_ref) <= 1e-10
    for e in errs:
        assert e <= 1e-10


@pytest.mark.parametrize("points,B,time_scale", STEP_CASES)
def test_backward_substep_fp32(points, B, time_scale):
    g_ref, l_ref = step_reference(points, B, time_scale, True)
    g32, l32 = step_reference(points, B, time_scale, False)
    grad, lam = device_step(points, B, time_scale, np.float32)
    gates = [rel(g32[:, j], g_ref[:, j]) for j in range(3)]
    errs = [rel(grad[:, j], g_ref[:, j]) for j in range(3)]
    print(f"fp32 substep {points} B={B} ts={time_scale}: lam0 {rel(lam, l_ref):.3e} (complex64 reference {rel(l32, l_ref):.3e}) " +
          " ".join(f"{n} {e:.3e} (complex64 reference {r:.3e})" for n, e, r in zip(ROT_NAMES, errs, gates)))
    # each quantity within 8 x the distance of the reference at complex64 from itself at complex128 on this case (device
    # transforms round in another order); the gate scales itself where a sum cancels (the k-gradient of the first case).
    # The complex64 reference's distance, measured on the CPU over these cases: lam0 1.7e-7 .. 5.3e-6, gradients
    # 4.4e-8 .. 3.0e-5.  The device's ratios to it, measured over these cases: lam0 0.07 .. 1.4, k 0.6 .. 2.3, e 0.06 .. 1.1,
    # omega 0.09 .. 3.9 (the largest at 48 x 40, B = 1, imaginary time: reference 3.1e-8, device 1.2e-7); DESIGN.md 4.12.
    assert rel(lam, l_ref) <= 8 * rel(l32, l_ref)
    for e, r in zip(errs, gates):
        assert e <= 8 * r


def test_host_gradient_block_equals_the_device_one():
    case = STEP_CASES[2]
    g_dev, lam_dev = device_step(*case, np.float64)
    g_host, lam_host = device_step(*case, np.float64, host_grad=True)
    np.testing.assert_array_equal(g_dev, g_host)
    np.testing.assert_array_equal(lam_dev, lam_host)


# ---- the whole gradient -----------------------------------------------------------------------------------------------

POINTS, DT0 = (48, 40), 0.02
TS = 0.1 + DT0 * np.array([0.0, 3.0, 4.4, 6.5])  # a step edge, a save inside a step, a clipped 7th substep
SHARED = dict(k=1.3, e=0.2, omega=0.6)
TIME_SCALE = 0.3 - 1j


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
    y0, _ = fields(POINTS, 2, 3)
    p = np.array([[SHARED[n] for n in ROT_NAMES]] * 2)
    J, ys, g, lam0 = A.solve_grad(A.Case(P.Domain(POINTS, BOX, "dimensionless"), TIME_SCALE, double), y0, p, TS, DT0, objective)
    return J, ys, g, lam0  # g: per environment (2, 3)


def model():
    return P.PDEModel(P.GPE2DTSRot, P.Domain(POINTS, BOX, "dimensionless"), P.RotatingStrangSplitting)


def device_gradient(dtype, cap=None, monkeypatch=None, per_environment=False):
    m = model()
    y0 = fields(POINTS, 2, 3)[0].astype(dtype)
    if cap is not None:
        monkeypatch.setenv(CHUNK_BYTES_ENV, str(cap))
    obj = Recording()
    J, grad, lam0 = m.rotation_gradient(obj, y0, TS, SHARED, {"time_scale": TIME_SCALE}, dt0=DT0, per_environment=per_environment)
    return m, y0, obj.ys, J, np.stack([grad[n] for n in ROT_NAMES], axis=-1), lam0


def test_whole_gradient_fp64_and_its_bitwise_properties(monkeypatch):
    J_ref, _, g_ref, l_ref = solve_reference(True)
    m, y0, ys, J, grad, lam0 = device_gradient(np.float64)
    assert m.rot_control_solver().last_chunks == 1
    tot = g_ref[0] + g_ref[1]
    errs = [abs(grad[j] - tot[j]) / abs(tot[j]) for j in range(3)]
    print(f"fp64 whole gradient: J {abs(J - J_ref) / abs(J_ref):.3e} lam0 {rel(lam0, l_ref):.3e} " +
          " ".join(f"{n} {e:.3e}" for n, e in zip(ROT_NAMES, errs)))
    assert grad.shape == (3,) and lam0.shape == y0.shape
    assert rel(lam0, l_ref) <= 1e-10
    for e in errs:
        assert e <= 1e-10
    # the objective saw the array solve returns
    np.testing.assert_array_equal(ys, m.solve(SHARED, y0, TS, {"time_scale": TIME_SCALE}, dt0=DT0))
    # a repeat gives the same bits
    _, _, _, J2, grad2, lam02 = device_gradient(np.float64)
    assert J2 == J
    np.testing.assert_array_equal(grad2, grad)
    np.testing.assert_array_equal(lam02, lam0)
    # three chunks (3 + 3 + 1 substeps) give the same bits as one
    m3, _, _, J3, grad3, lam03 = device_gradient(np.float64, cap=3 * y0.nbytes, monkeypatch=monkeypatch)
    assert m3.rot_control_solver().last_chunks == 3
    assert J3 == J
    np.testing.assert_array_equal(grad3, grad)
    np.testing.assert_array_equal(lam03, lam0)


def test_whole_gradient_per_environment_sums_to_the_shared_one():
    g_ref = solve_reference(True)[2]
    _, _, _, _, per, _ = device_gradient(np.float64, per_environment=True)
    _, _, _, _, tot, _ = device_gradient(np.float64)
    assert per.shape == (2, 3)
    np.testing.assert_array_equal(per[0] + per[1], tot)
    for j in range(3):
        assert rel(per[:, j], g_ref[:, j]) <= 1e-10


def test_whole_gradient_fp32():
    _, _, g_ref, l_ref = solve_reference(True)
    _, _, g32, l32 = solve_reference(False)
    _, _, _, _, grad, lam0 = device_gradient(np.float32)
    tot, tot32 = g_ref[0] + g_ref[1], g32[0] + g32[1]
    gates = [abs(tot32[j] - tot[j]) / abs(tot[j]) for j in range(3)]
    errs = [abs(grad[j] - tot[j]) / abs(tot[j]) for j in range(3)]
    print(f"fp32 whole gradient: lam0 {rel(lam0, l_ref):.3e} (complex64 reference {rel(l32, l_ref):.3e}) " +
          " ".join(f"{n} {e:.3e} (complex64 reference {r:.3e})" for n, e, r in zip(ROT_NAMES, errs, gates)))
    # 8 x the complex64 reference's own distance from complex128 on this case.  Measured ratios: lam0 1.4, k 0.09, e 2.9,
    # omega 0.05
    assert rel(lam0, l_ref) <= 8 * rel(l32, l_ref)
    for e, r in zip(errs, gates):
        assert e <= 8 * r


# ---- the library's refusals ---------------------------------------------------------------------------------------------


def refused(eng, lam, grad, psi0=None, match=None):
    """the engine turns PDEOPT_EINVAL into ValueError and every other status into PdeoptError"""
    with pytest.raises((ValueError, L.PdeoptError), match=match) as e:
        eng.gpe_rot_adjoint_step(DT, psi0 if psi0 is not None else eng.state_device_ptr()[0], lam.data_ptr(), grad.data_ptr())
    return L.EINVAL if isinstance(e.value, ValueError) else e.value.code


def test_library_refusals():
    points, B = (48, 40), 2
    eqs = equations(points, B)
    solver = solver_of(eqs[0], 1.0)
    lam1 = torch.as_tensor(fields(points, B, 7)[1]).to(DEV)
    lam = lam1.clone()
    grad = torch.zeros((B, 3), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    # another equation
    eng = HipEngine(0)
    dom = P.Domain(points, BOX, "dimensionless")
    ch = P.CahnHilliard2DPeriodic(dom, 0.01, lambda c: c**3 - c, lambda c: 1.0)
    eng.configure(dtype=np.dtype(np.float64), batch=B, **ch._engine_problem())
    assert refused(eng, lam, grad, match="needs the GPE") == L.EINVAL
    # the rotation not set
    eng = HipEngine(0)
    eng.configure(dtype=np.dtype(np.float64), batch=B, **eqs[0]._engine_problem())
    eng.set_aux(L.AUX_GPE_POTENTIAL, eqs[0].trap_potential())
    solver.configure_engine(eng, eqs[0])
    eng.set_state(np.ones((B,) + points + (2,)))
    assert refused(eng, lam, grad, match="pdeopt_set_gpe_rotation") == L.ESTATE
    P.GPE2DTSRot._engine_upload_batch(eng, eqs, 0.0, DT)
    psi0 = eng.state_device_ptr()[0]
    # spots set
    from pde_opt_amd.numerics.functions.lights import GaussianSpots

    tab = GaussianSpots.single(1.0, 0.1, 0.2, 0.5).table(1)
    eng.set_gpe_spots(np.broadcast_to(tab, (B,) + tab.shape), *eqs[0]._cell0())
    assert refused(eng, lam, grad, match="no light spots") == L.EINVAL
    eng.set_gpe_spots(None)
    # overlapping buffers
    with pytest.raises(ValueError, match="overlap"):
        eng.gpe_rot_adjoint_step(DT, psi0, psi0, grad.data_ptr())
    with pytest.raises(ValueError, match="overlap"):
        eng.gpe_rot_adjoint_step(DT, psi0, lam.data_ptr(), lam.data_ptr())
    # a potential from a host callable
    eng.set_aux_time_fn(L.AUX_GPE_POTENTIAL, lambda t: eqs[0].trap_potential())
    assert refused(eng, lam, grad, match="host callable") == L.EINVAL
    # every refusal left lam and grad untouched
    eng.sync()
    assert torch.equal(lam, lam1) and not grad.any()
    # and the supported call on the same engine still runs
    P.GPE2DTSRot._engine_upload_batch(eng, eqs, 0.0, DT)
    eng.gpe_rot_adjoint_step(DT, psi0, lam.data_ptr(), grad.data_ptr())
    eng.sync()
    assert np.all(np.isfinite(grad.cpu().numpy())) and not torch.equal(lam, lam1)


# ---- an optimisation ----------------------------------------------------------------------------------------------------

import gpe_rot_fit_problem as C  # noqa: E402  (the case; the CPU reference run that meets the same bounds is recorded there)


def test_optimisation_recovers_the_rotation_frequency():
    m = P.PDEModel(P.GPE2DTSRot, C.domain(), P.RotatingStrangSplitting)
    fitted = m.optimize_rotation(C.objective, C.y0(), C.TS, {"omega": C.OMEGA_START}, dict(k=C.K_GPE, e=C.E_GPE),
                                 max_steps=C.MAX_STEPS, dt0=C.DT0)
    hist = m.last_optimize_history
    print("J per accepted step:", " ".join(f"{v:.6e}" for v in hist), "omega", fitted["omega"])
    assert hist[-1] <= 1e-6 * hist[0]
    assert abs(fitted["omega"] - C.OMEGA_TRUE) <= 1e-3
    assert fitted["k"] == C.K_GPE and fitted["e"] == C.E_GPE
