"""CPU side of ImplicitEuler: the numpy reference checks itself (tests/implicit_ref.py: linearisation against central
differences, dense route against GMRES route, float32 Newton on the problems of the fp32 GPU tests), and the host logic
refuses what the solver does not cover before any engine work (through tests/fake_engine.py where an engine is asked
for)."""
import os
import re

import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd.utils import check_equation_solver_compatibility
from fake_engine import OracleEngine

import implicit_problems as Q
import implicit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQS = ("ch", "ac")


# ---- the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closures", list(Q.CLOSURES))
@pytest.mark.parametrize("eq", EQS)
def test_linearisation_agrees_with_a_central_difference(eq, closures):
    """(f(u + e v) - f(u - e v)) / 2e = J v + e^2 f'''[v, v, v] / 6 + rounding eps |f| / e: the second difference with a
    step twice as large measures the truncation term (it is 4 x as big), and the gate is that estimate plus the rounding
    term -- the difference's own error"""
    points = Q.GRIDS["8x12"]
    mu, mob = Q.CLOSURES[closures]
    u = Q.state(points, 1)
    v = np.random.default_rng(2).standard_normal(points)
    f = lambda w: R.rhs(eq, w, Q.H, Q.H, Q.KAPPA, mu, mob)
    e = 1e-4
    cd = (f(u + e * v) - f(u - e * v)) / (2 * e)
    cd2 = (f(u + 2 * e * v) - f(u - 2 * e * v)) / (4 * e)
    trunc = float(np.max(np.abs(cd2 - cd))) / 3.0
    rounding = 8 * np.finfo(np.float64).eps * float(np.max(np.abs(f(u)))) * (Q.KAPPA * (8 / Q.H**2) + 1) / e
    err = float(np.max(np.abs(R.jac(eq, u, v, Q.H, Q.H, Q.KAPPA, mu, mob) - cd)))
    assert err <= 2 * trunc + rounding, (err, trunc, rounding)
    assert err <= 1e-6 * float(np.max(np.abs(cd)))  # and the estimate itself is small: a wrong term would be O(1)


@pytest.mark.parametrize("closures", list(Q.CLOSURES))
@pytest.mark.parametrize("eq", EQS)
def test_dense_and_gmres_routes_agree(eq, closures):
    """both satisfy rms(G) <= tol = atol + rtol rms(y); G' = I - dt J has its smallest singular value near 1 on these
    problems (the stiff part is positive), so two such points are within about 2 tol of each other in rms; 10 x covers
    the non-normal part"""
    points = Q.GRIDS["8x12"]
    mu, mob = Q.CLOSURES[closures]
    y = Q.state(points, 1)
    dt = Q.step_size(eq, points, closures, y)
    rtol, atol = Q.TOL[np.float64]
    a, ita, ra = R.newton(eq, y, dt, Q.H, Q.H, Q.KAPPA, mu, mob, rtol, atol, "dense")
    b, itb, rb = R.newton(eq, y, dt, Q.H, Q.H, Q.KAPPA, mu, mob, rtol, atol, "gmres")
    tol = atol + rtol * R.rms(a)
    assert ra <= tol and rb <= tol
    assert R.rms(a - b) <= 10 * 2 * tol
    # and to the limit of the arithmetic: rms(G) <= 1e-13
    a13, _, r13 = R.newton(eq, y, dt, Q.H, Q.H, Q.KAPPA, mu, mob, 0.0, 1e-13, "dense")
    b13, _, s13 = R.newton(eq, y, dt, Q.H, Q.H, Q.KAPPA, mu, mob, 0.0, 1e-13, "gmres", krylov_rtol=1e-6)
    assert r13 <= 1e-13 and s13 <= 1e-13 and R.rms(a13 - b13) <= 1e-12


@pytest.mark.parametrize("closures", list(Q.CLOSURES))
@pytest.mark.parametrize("grid", ["16x32", "8x12"])
@pytest.mark.parametrize("eq", EQS)
def test_float32_newton_converges_on_the_gpu_tests_problems(eq, grid, closures):
    """the step 50 x the Euler limit keeps the fp32 rounding of dt f (1e-5 (dt / 1e-4) for Cahn-Hilliard at h = 0.01,
    kappa = 0.002: 8e-7 at dt = 8e-6) well below the fp32 tolerance 1e-6 + 1e-4 rms(y) = 5e-5"""
    points = Q.GRIDS[grid]
    mu, mob = Q.CLOSURES[closures]
    y = Q.state(points, 1, np.float32)
    dt = Q.step_size(eq, points, closures, y)
    rtol, atol = Q.TOL[np.float32]
    y1, its, res = R.newton(eq, y, dt, Q.H, Q.H, Q.KAPPA, mu, mob, rtol, atol, "gmres", max_newton=20)
    assert y1.dtype == np.float32 and 1 <= its <= 20 and res <= atol + rtol * R.rms(y1)
    f64 = R.rhs(eq, y1.astype(np.float64), Q.H, Q.H, Q.KAPPA, mu, mob)
    f32 = R.rhs(eq, y1, Q.H, Q.H, Q.KAPPA, mu, mob)
    assert R.rms(dt * (f32 - f64)) <= 0.1 * (atol + rtol * R.rms(y1))


def test_step_is_50_times_the_euler_limit():
    """explicit Euler at 1.2 x the limit grows, at 0.8 x it does not: the bound of implicit_ref.euler_limit is the limit of
    the stiffest mode to within that bracket"""
    points = Q.GRIDS["8x12"]
    for eq in EQS:
        mu, mob = Q.CLOSURES["poly"]
        y = Q.state(points, 1)
        lim = Q.step_size(eq, points, "poly", y) / Q.STEP_FACTOR
        amp = {}
        for fac in (0.8, 1.2):
            u = y.copy()
            for _ in range(200):
                u = u + fac * lim * R.rhs(eq, u, Q.H, Q.H, Q.KAPPA, mu, mob)
                if not np.isfinite(u).all() or np.max(np.abs(u)) > 1e6:
                    break
            amp[fac] = float(np.max(np.abs(u))) if np.isfinite(u).all() else np.inf
        assert amp[0.8] < 2.0 < amp[1.2], (eq, amp)


# ---- the interface ------------------------------------------------------------------------------------------------------
def test_error_class_and_exports():
    assert issubclass(P.ImplicitSolveError, RuntimeError)
    from pde_opt_amd.numerics import solvers

    assert solvers.ImplicitEuler is P.ImplicitEuler and solvers.ImplicitSolveError is P.ImplicitSolveError
    s = P.ImplicitEuler(1e-4, 1e-6)
    assert (s.krylov_rtol, s.restart, s.max_newton, s.max_krylov) == (1e-3, 20, 20, 200)
    assert s.integrator == L.INT_IMPLICIT_EULER == 6 and s.order() == 1


def test_symbols_in_header_and_binding():
    text = open(os.path.join(ROOT, "include", "pdeopt_hip.h")).read()
    for name in ("pdeopt_implicit_configure", "pdeopt_implicit_advance", "pdeopt_implicit_apply"):
        assert re.search(r"\bint " + name + r"\(", text) and name in L._SIGNATURES
    assert re.search(r"PDEOPT_INT_IMPLICIT_EULER = 6\b", text) and re.search(r"PDEOPT_ENOCONVERGE = -1\b", text)
    assert L.ENOCONVERGE == -1
    lib = L.load_library()
    assert all(hasattr(lib, n) for n in ("pdeopt_implicit_configure", "pdeopt_implicit_advance", "pdeopt_implicit_apply"))


def test_compatibility_check():
    check_equation_solver_compatibility(P.ImplicitEuler, P.CahnHilliard2DPeriodic)
    check_equation_solver_compatibility(P.ImplicitEuler, P.AllenCahn2DPeriodic)
    for cls in (P.CahnHilliard3DPeriodic, P.AllenCahn2DSmoothedBoundary, P.CahnHilliard2DSmoothedBoundary,
                P.AllenCahn2DPeriodicButlerVolmer, P.AllenCahn2DPeriodicButlerVolmerConstantCurrent,
                P.AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent, P.AdvectionDiffusion2D, P.GPE2DTSControl, P.GPE2DTSRot):
        with pytest.raises(NotImplementedError, match="CahnHilliard2DPeriodic and AllenCahn2DPeriodic only"):
            check_equation_solver_compatibility(P.ImplicitEuler, cls)
        with pytest.raises(NotImplementedError):
            P.PDEModel(cls, Q.domain((8, 12)), P.ImplicitEuler)


class _NoEngine(OracleEngine):
    """an engine that fails the test when it is touched: the refusals come before any engine work"""

    def configure(self, *a, **k):
        raise AssertionError("the engine was configured before the refusal")


def _solve(eq, controller=None, engine=None, solver=None):
    y = Q.state(eq.domain.points, 1)
    return P.diffeqsolve(eq, solver or P.ImplicitEuler(1e-4, 1e-6), t0=0.0, t1=1e-5, dt0=1e-6, y0=y,
                         stepsize_controller=controller, engine=engine or _NoEngine())


def test_refusals_before_any_engine_work():
    eq = Q.equation("ch", (8, 12), "poly")
    with pytest.raises(NotImplementedError, match="PIDController"):
        _solve(eq, P.PIDController(1e-3, 1e-6))
    with pytest.raises(NotImplementedError, match='derivs="fd"'):
        _solve(Q.equation("ac", (8, 12), "poly", derivs="fourier"))
    jit = P.CahnHilliard2DPeriodic(Q.domain((8, 12)), Q.KAPPA, lambda c: np.tanh(3 * c) + 0.5 * c, lambda c: 1.0 + c * c)
    assert jit._mu_desc.kind == L.CL_JIT
    with pytest.raises(NotImplementedError, match="run-time-compiled"):
        _solve(jit)
    padded = _NoEngine()
    padded.halo_layout = 4
    with pytest.raises(NotImplementedError, match="periodic layout"):
        _solve(eq, engine=padded)
    with pytest.raises(ValueError, match="restart"):
        _solve(eq, solver=P.ImplicitEuler(1e-4, 1e-6, restart=65))
    with pytest.raises(ValueError, match="rtol"):
        _solve(eq, solver=P.ImplicitEuler(0.0, 0.0))
    with pytest.raises(NotImplementedError, match="PIDController"):
        P.PDEModel(P.CahnHilliard2DPeriodic, Q.domain((8, 12)), P.ImplicitEuler).solve(
            dict(kappa=Q.KAPPA, mu=Q.CLOSURES["poly"][0], D=1.0), Q.state((8, 12), 1), [0.0, 1e-5],
            solver_parameters=dict(rtol=1e-4, atol=1e-6), stepsize_controller=P.PIDController(1e-3, 1e-6))


def test_a_module_as_mu_is_refused():
    torch = pytest.importorskip("torch")

    class Net(torch.nn.Module):
        def forward(self, c):
            return c

    model = P.PDEModel(P.CahnHilliard2DPeriodic, Q.domain((8, 12)), P.ImplicitEuler)
    with pytest.raises(NotImplementedError, match="torch.nn.Module"):
        model.solve(dict(kappa=Q.KAPPA, mu=Net(), D=1.0), Q.state((8, 12), 1), [0.0, 1e-5],
                    solver_parameters=dict(rtol=1e-4, atol=1e-6))
    with pytest.raises(NotImplementedError, match="implicit step"):
        model.mse_backward(dict(kappa=Q.KAPPA, mu=Net(), D=1.0), (None, None), dict(rtol=1e-4, atol=1e-6), [0.0, 1e-5], {}, 0.0)


def test_train_and_optimize_are_refused():
    model = P.PDEModel(P.AllenCahn2DPeriodic, Q.domain((8, 12)), P.ImplicitEuler)
    with pytest.raises(NotImplementedError, match="implicit step"):
        model.train({"ys": [], "ts": []}, [], {}, {}, dict(rtol=1e-4, atol=1e-6), {}, 0.0)
    with pytest.raises(NotImplementedError, match="implicit step"):
        model.optimize(lambda ys: ys.sum(), Q.state((8, 12), 1), [0.0, 1e-5], {"mu": None}, {}, dict(rtol=1e-4, atol=1e-6))


def test_pde_env_takes_the_solver_type_and_refuses_other_equations():
    with pytest.raises(NotImplementedError, match="CahnHilliard2DPeriodic and AllenCahn2DPeriodic only"):
        check_equation_solver_compatibility(P.ImplicitEuler, P.CahnHilliard3DPeriodic)
    # configure_engine, the door PDEEnv / VectorPDEEnv go through, refuses like diffeqsolve does
    with pytest.raises(NotImplementedError, match='derivs="fd"'):
        P.ImplicitEuler(1e-4, 1e-6).configure_engine(_NoEngine(), Q.equation("ch", (8, 12), "poly", derivs="fourier"))
