"""Time integrators.  Each class is a *descriptor*: it names a fused HIP integrator
(csrc/stencil.hip, csrc/spectral.hip) and carries its parameters; the stepping loop itself runs
on the GPU through ``pde_opt_amd.integrate.diffeqsolve``.

``SemiImplicitFourierSpectral`` and ``StrangSplitting`` keep the reference's constructor
signatures and the ``required_equation_attrs`` protocol (pde_opt/numerics/solvers.py:42-46,
84-89) so ``prepare_solver_params`` / ``check_equation_solver_compatibility`` (pde_opt/utils.py)
work unchanged.  ``Euler`` / ``RK4`` / ``Tsit5`` / ``ConstantStepSize`` / ``PIDController`` /
``SaveAt`` stand in for the diffrax objects of the same names used at the reference's call sites
(pde_env.py:293-303, tests/test_solvers.py:44-53,81-95).
"""

from __future__ import annotations

import dataclasses
from typing import Any, Callable, Optional, Sequence

import numpy as np

from .. import _lib as L


class AbstractSolver:
    """Base of every integrator descriptor."""

    integrator: int = -1
    required_equation_attrs: list = []

    def configure_engine(self, engine, equation) -> None:
        """push integrator parameters / spectral constants to the device"""

    def step(self, equation, t0, t1, y0):
        """One step on the GPU (for tests that poke ``solver.step`` like upstream's)."""
        from ..integrate import diffeqsolve

        sol = diffeqsolve(equation, self, t0=t0, t1=t1, dt0=t1 - t0, y0=y0)
        return sol.ys[-1]


class Euler(AbstractSolver):
    """Explicit Euler (diffrax.Euler)."""

    integrator = L.INT_EULER

    def order(self, terms=None):
        return 1


class RK4(AbstractSolver):
    """Classical 4-stage Runge-Kutta: four fused stencil+update kernels per substep.
    New relative to the reference (BASELINE.json configs 2, 3, 5)."""

    integrator = L.INT_RK4

    def order(self, terms=None):
        return 4


class Tsit5(AbstractSolver):
    """Tsitouras 5(4) (diffrax.Tsit5); adaptive with ``PIDController``."""

    integrator = L.INT_TSIT5

    def order(self, terms=None):
        return 5


@dataclasses.dataclass
class SemiImplicitFourierSpectral(AbstractSolver):
    """y1 = y0 + dt Re ifft( fft(rhs(y0)) / (1 + A dt fourier_symbol) )   (solvers.py:56-70)."""

    A: float
    fourier_symbol: Any
    fft: Optional[Callable] = None
    ifft: Optional[Callable] = None

    required_equation_attrs = ["fourier_symbol", "fft", "ifft"]
    integrator = L.INT_IMEX

    def order(self, terms=None):
        return 1

    def configure_engine(self, engine, equation):
        engine.set_integrator_params(imex_A=float(self.A))
        # a symbol this engine already holds (same table, same kappa: the per-step rebuild of PDEEnv.step) is
        # not uploaded again -- the library would also rebuild its spectral multiplier
        engine.set_aux(L.AUX_IMEX_SYMBOL, self.fourier_symbol, key=getattr(self.fourier_symbol, "key", None))

@dataclasses.dataclass
class StrangSplitting(AbstractSolver):
    """Strang split step with per-step renormalisation (solvers.py:99-122)."""

    A_term: Any
    dx: float
    fft: Optional[Callable] = None
    ifft: Optional[Callable] = None
    time_scale: complex = 1.0

    required_equation_attrs = ["A_term", "dx", "fft", "ifft"]
    integrator = L.INT_STRANG

    def order(self, terms=None):
        return 1

    @classmethod
    def check_equation_type(cls, equation_type):
        if getattr(equation_type, "_rotating_frame", False):
            raise ValueError(f"{equation_type.__name__} publishes the operator pair A_terms of the alternating-direction "
                             f"splitting, not one A_term: integrate it with RotatingStrangSplitting, not {cls.__name__}")

    def configure_engine(self, engine, equation):
        engine.set_integrator_params(time_scale=complex(self.time_scale), strang_dx=float(self.dx))
        engine.set_aux(L.AUX_GPE_A_TERM, self.A_term, key=getattr(self.A_term, "key", None))


@dataclasses.dataclass
class RotatingStrangSplitting(AbstractSolver):
    """Alternating-direction split step of the rotating-frame GPE (``GPE2DTSRot``), new relative to the reference, which
    publishes the operator pair ``A_terms`` but no solver for it.  With tau = dt * time_scale and
    ``L_x(s) v = ifft_x[exp(s A_x) fft_x v]``, ``L_y`` alike (transforms along ONE axis; ``(A_x, A_y) = A_terms``):

        psi1 = L_y(tau/2) L_x(tau/2) psi0;   b = B(psi0);   psi2 = psi1 exp(b tau)
        psi3 = psi2 / sqrt(dx^2 sum |psi2|^2);   psi4 = L_x(tau/2) L_y(tau/2) psi3

    ``b`` from the state before the half step and the renormalisation of every step are ``StrangSplitting``'s, so
    with ``omega = 0`` this is that solver's step with the kinetic ``A_term``.  DESIGN.md section 4.10."""

    dx: float
    time_scale: complex = 1.0
    A_terms: Any = None  # pulled off the equation like every required attribute; the kernels form the pair themselves

    required_equation_attrs = ["A_terms", "dx"]
    integrator = L.INT_STRANG_ROT

    def order(self, terms=None):
        return 1

    @classmethod
    def check_equation_type(cls, equation_type):
        if not getattr(equation_type, "_rotating_frame", False):
            raise ValueError(f"{cls.__name__} integrates the rotating-frame operator pair of GPE2DTSRot; "
                             f"{equation_type.__name__} does not publish one: "
                             + ("integrate it with StrangSplitting" if hasattr(equation_type, "A_term")
                                else "it has no split-step form"))

    def configure_engine(self, engine, equation):
        engine.set_integrator_params(time_scale=complex(self.time_scale), strang_dx=float(self.dx))


class ImplicitSolveError(RuntimeError):
    """A step of ``ImplicitEuler`` did not converge within ``max_newton`` / ``max_krylov``.  The message names the
    environment, the step and the last residual; the engine's state is the one the failing step started from."""


IMPLICIT_EULER_SUPPORT = ('CahnHilliard2DPeriodic or AllenCahn2DPeriodic with derivs="fd", closures of the in-kernel family '
                          "(polynomial / Legendre), ConstantStepSize, fp32 / fp64, the periodic layout")


@dataclasses.dataclass
class ImplicitEuler(AbstractSolver):
    """Implicit Euler ``y1 = y0 + dt f(y1, t1)`` by matrix-free Newton-GMRES on the GPU: the stand-in for
    ``diffrax.ImplicitEuler`` with a Newton root-find and ``lineax.GMRES`` inside (upstream's
    ``notebooks/test_implicit.ipynb``).  DESIGN.md section 4.21.

    Newton on ``G(y) = y - y0 - dt f(y)`` starts at ``y0`` and stops, per environment, when
    ``rms(G) <= atol + rtol rms(y)``.  Each linear solve ``(I - dt J_f(y)) delta = -G`` is GMRES restarted every ``restart``
    (at most 64) iterations and stops when its residual estimate is ``<= krylov_rtol ||G||_2``.  A step that needs more than
    ``max_newton`` linear solves, or a linear solve more than ``max_krylov`` iterations, raises ``ImplicitSolveError``.
    ``solution.stats`` carries ``newton_iterations``, ``krylov_iterations``, ``operator_applications`` and
    ``rhs_evaluations``: a list per environment, and their totals under ``"implicit_totals"``.

    ``precond="spectral"`` right-preconditions every GMRES solve with the symbol of the constant-coefficient part of the
    finite-difference operator at the Newton iterate (two batched real transforms and one multiply per Krylov iteration);
    ``solution.stats`` then also carries ``preconditioner_applications`` per environment.  The default ``None`` is the
    unpreconditioned solver.

    Runs ``IMPLICIT_EULER_SUPPORT``; everything else raises ``NotImplementedError`` before any engine work."""

    rtol: float
    atol: float
    krylov_rtol: float = 1e-3
    restart: int = 20
    max_newton: int = 20
    max_krylov: int = 200
    precond: Optional[str] = None

    integrator = L.INT_IMPLICIT_EULER

    def __post_init__(self):
        if self.precond not in L.IMPLICIT_PRECOND:
            raise ValueError(f'ImplicitEuler: precond = {self.precond!r} (None or "spectral")')

    def order(self, terms=None):
        return 1

    @classmethod
    def check_equation_type(cls, equation_type):
        from .equations.phase_field import AllenCahn2DPeriodic, CahnHilliard2DPeriodic

        if equation_type not in (CahnHilliard2DPeriodic, AllenCahn2DPeriodic):
            raise NotImplementedError(f"ImplicitEuler has a Jacobian action for CahnHilliard2DPeriodic and AllenCahn2DPeriodic only, "
                                      f"not {getattr(equation_type, '__name__', equation_type)}: the 3-D, smoothed-boundary, "
                                      "Butler-Volmer, advection-diffusion and GPE classes stay on their explicit or split-step solvers")

    def check_solve(self, equation, stepsize_controller=None, engine=None):
        """what ``diffeqsolve`` asks before it touches the engine"""
        self.check_equation_type(type(equation))
        if isinstance(stepsize_controller, PIDController):
            raise NotImplementedError("ImplicitEuler steps with ConstantStepSize: it has no error estimate for a PIDController "
                                      "(an adaptive step for this solver is not implemented)")
        if getattr(equation, "_mu_module", None) is not None:
            raise NotImplementedError("ImplicitEuler linearises mu inside the kernel: a torch.nn.Module as mu has no in-kernel "
                                      "derivative (it runs with SemiImplicitFourierSpectral or Euler)")
        if getattr(equation, "derivs", "fd") != "fd":
            raise NotImplementedError('ImplicitEuler linearises the finite-difference right-hand side: derivs="fd", not '
                                      f'"{equation.derivs}"')
        for d in (equation._mu_desc, equation._mob_desc):
            if d is not None and d.kind == L.CL_JIT:
                raise NotImplementedError("ImplicitEuler needs closures of the in-kernel family (polynomial / Legendre): a "
                                          "run-time-compiled closure has no derivative to linearise with")
        if engine is not None and getattr(engine, "halo_layout", 0):
            raise NotImplementedError("ImplicitEuler needs the periodic layout: its sums run over whole environments, a padded "
                                      "(decomposed) tile holds a part of one")
        if not (self.rtol >= 0 and self.atol >= 0 and self.rtol + self.atol > 0):
            raise ValueError(f"ImplicitEuler: rtol = {self.rtol}, atol = {self.atol} (non-negative, not both zero)")
        if not 1 <= int(self.restart) <= L.IMPLICIT_MAX_RESTART:
            raise ValueError(f"ImplicitEuler: restart = {self.restart} (1 .. {L.IMPLICIT_MAX_RESTART})")

    def configure_engine(self, engine, equation):
        self.check_solve(equation, None, engine)  # call sites that configure an engine themselves (PDEEnv) are refused alike
        engine.implicit_configure(self.rtol, self.atol, self.krylov_rtol, self.restart, self.max_newton, self.max_krylov)
        if self.precond is not None:
            engine.implicit_set_precond(self.precond)


def reject_implicit_gradients(solver_type, what: str) -> None:
    """``train`` / ``optimize`` / ``mse_backward`` differentiate the solve: there is no tangent or adjoint of the Newton-GMRES step"""
    if solver_type is ImplicitEuler:
        raise NotImplementedError(f"{what} differentiates the solve, and sensitivities through the implicit step are not "
                                  "implemented: ImplicitEuler is a forward solver (fit with Euler, RK4 or "
                                  "SemiImplicitFourierSpectral)")


# ---- step-size controllers / save specification (diffrax stand-ins) ---------------------------


class ConstantStepSize:
    pass


@dataclasses.dataclass
class PIDController:
    """diffrax.PIDController defaults: an I-controller (pcoeff = dcoeff = 0)."""

    rtol: float
    atol: float
    pcoeff: float = 0.0
    icoeff: float = 1.0
    dcoeff: float = 0.0
    safety: float = 0.9
    factormin: float = 0.2
    factormax: float = 10.0
    dtmin: Optional[float] = None
    dtmax: Optional[float] = None
    # new (batched solves): every environment runs its own controller -- own step size, own accept / reject --
    # instead of the whole batch stepping with the worst error norm (pdeopt_tsit5_trial_env)
    per_environment: bool = False


@dataclasses.dataclass
class SaveAt:
    t1: bool = False
    ts: Optional[Sequence[float]] = None
    t0: bool = False
