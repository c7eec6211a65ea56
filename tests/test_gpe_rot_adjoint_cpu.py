"""CPU checks of the rotating-frame GPE's gradient entries and of their reference (tests/gpe_rot_adjoint_ref.py): the
torch step against the numpy step of tests/gpe_rot_ref.py, the refusals of ``rotation_gradient`` / ``optimize_rotation``
(no engine, no GPU), the three older entries that keep refusing, and the new ABI symbol."""
import os
import re

import numpy as np
import pytest
import torch

import pde_opt_amd as P
from pde_opt_amd import _lib as L

import gpe_rot_adjoint_ref as A
import gpe_rot_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
BOX = ((-2.0, 2.0), (-1.5, 1.5))
PARAMS = np.array([[1.3, 0.2, 0.6], [0.9, -0.1, -0.4], [2.1, 0.35, 0.85]])  # (k, e, omega) per environment


@pytest.mark.parametrize("points,time_scale", [((64, 64), 1.0), ((48, 40), -1j), ((48, 40), 0.3 - 1j), ((64, 128), 1.0)])
def test_torch_step_equals_the_numpy_step(points, time_scale):
    dom = P.Domain(points, BOX, "dimensionless")
    rng = np.random.default_rng(7)
    y0 = rng.standard_normal((3,) + points + (2,))
    out = A.step(A.Case(dom, time_scale), torch.as_tensor(y0), torch.as_tensor(PARAMS), 0.02).numpy()
    for b in range(3):
        want = RR.RotCase(dom, *PARAMS[b], time_scale).step(RR.from_pairs(y0[b]), 0.02)
        err = np.max(np.abs(RR.from_pairs(out[b]) - want)) / np.max(np.abs(want))
        assert err <= 1e-13, (b, err)


def test_reference_gradient_against_a_difference_quotient():
    """autograd of the torch step over (k, e, omega) against central differences of the numpy step"""
    dom = P.Domain((16, 12), BOX, "dimensionless")
    rng = np.random.default_rng(3)
    y0, lam1 = rng.standard_normal((1, 16, 12, 2)), rng.standard_normal((1, 16, 12, 2))
    g, _ = A.step_vjp(A.Case(dom, 0.3 - 1j), y0, PARAMS[:1], 0.02, lam1)
    J = lambda p: float(np.sum(RR.to_pairs(RR.RotCase(dom, *p, 0.3 - 1j).step(RR.from_pairs(y0[0]), 0.02)) * lam1[0]))
    for j in range(3):
        h = np.zeros(3)
        h[j] = 1e-5
        fd = (J(PARAMS[0] + h) - J(PARAMS[0] - h)) / 2e-5
        assert abs(fd - g[0, j]) <= 1e-7 * max(1.0, np.max(np.abs(g))), (j, fd, g[0, j])


# ---- refusals -----------------------------------------------------------------------------------------------------------

DOM = P.Domain((16, 16), ((-2.0, 2.0), (-2.0, 2.0)), "dimensionless")
Y0 = np.zeros((16, 16, 2))
TS = [0.0, 0.1]
OBJ = lambda ys: ys.sum()


def test_the_new_entries_refuse_another_equation_or_solver():
    m = P.PDEModel(P.GPE2DTSControl, DOM, P.StrangSplitting)
    params = dict(k=1.0, e=0.0, lights=lambda t, x, y: 0.0 * x)
    with pytest.raises(NotImplementedError, match="GPE2DTSRot with RotatingStrangSplitting"):
        m.rotation_gradient(OBJ, Y0, TS, params)
    with pytest.raises(NotImplementedError, match="GPE2DTSRot with RotatingStrangSplitting"):
        m.optimize_rotation(OBJ, Y0, TS, {"k": 1.0}, {"e": 0.0})
    ch = P.PDEModel(P.CahnHilliard2DPeriodic, DOM, P.RK4)
    with pytest.raises(NotImplementedError, match="CahnHilliard2DPeriodic"):
        ch.rotation_gradient(OBJ, np.zeros((16, 16)), TS, {})


def test_the_new_entries_refuse_unknown_names_and_adaptive_steps():
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    with pytest.raises(NotImplementedError, match=r"\['trap_factor'\].*subset of k, e and omega"):
        m.optimize_rotation(OBJ, Y0, TS, {"trap_factor": 1.0}, dict(k=1.0, e=0.0, omega=0.3))
    with pytest.raises(NotImplementedError, match="subset of k, e and omega"):
        m.optimize_rotation(OBJ, Y0, TS, {}, dict(k=1.0, e=0.0, omega=0.3))
    pid = P.PIDController(rtol=1e-3, atol=1e-6)
    with pytest.raises(NotImplementedError, match="PIDController.*ConstantStepSize"):
        m.rotation_gradient(OBJ, Y0, TS, dict(k=1.0, e=0.0, omega=0.3), stepsize_controller=pid)
    with pytest.raises(NotImplementedError, match="PIDController.*ConstantStepSize"):
        m.optimize_rotation(OBJ, Y0, TS, {"omega": 0.3}, dict(k=1.0, e=0.0), stepsize_controller=pid)


def test_the_three_older_entries_still_refuse_and_name_the_new_ones():
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    params = dict(k=1.0, e=0.0, omega=0.3)
    with pytest.raises(NotImplementedError, match="rotating.*rotation_gradient.*optimize_rotation"):
        m.control_gradient(OBJ, Y0, TS, params)
    with pytest.raises(NotImplementedError, match="rotating.*rotation_gradient.*optimize_rotation"):
        m.optimize(OBJ, Y0, TS, {"omega": 0.3}, {"k": 1.0, "e": 0.0})
    with pytest.raises(NotImplementedError, match="rotating.*rotation_gradient.*optimize_rotation"):
        m.train({"ys": [Y0, Y0], "ts": TS}, [[0, 1]], {"omega": 0.3}, {"k": 1.0, "e": 0.0}, {}, {}, 0.0)


# ---- ABI ----------------------------------------------------------------------------------------------------------------

def test_the_new_symbol_is_declared_and_bound():
    header = open(os.path.join(os.path.dirname(HERE), "include", "pdeopt_hip.h")).read()
    decl = re.search(r"int\s+pdeopt_gpe_rot_adjoint_step\s*\(([^)]*)\)\s*;", header)
    assert decl and len(decl.group(1).split(",")) == 5
    assert len(L._SIGNATURES["pdeopt_gpe_rot_adjoint_step"][1]) == 5
    assert hasattr(L.load_library(), "pdeopt_gpe_rot_adjoint_step")
    assert callable(P.HipEngine.gpe_rot_adjoint_step)
