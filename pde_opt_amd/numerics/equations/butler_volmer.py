"""Allen-Cahn with Butler-Volmer kinetics, at a given voltage or at constant current, on the HIP engine.

Same dataclass surface as the reference (pde_opt/numerics/equations/allen_cahn.py:162-395): the three classes take
upstream's fields in upstream's order and publish upstream's attributes; ``rhs_fd(state, t)`` -- for the fixed-voltage
class also upstream's ``rhs_fd(state, t, v)`` -- and ``get_voltage(state)`` run on the GPU (csrc/butler_volmer.hip):

    mu  = mu_h(u) - kappa lap u                              periodic           (w = 1)
    mu  = mu_h(u) - kappa/psi div(psi grad u)                smoothed boundary  (w = psi; upstream has no wall term, f is unused)
    I+- = hx hy sum w j0(u) exp(+- mu / 2)                   y = (-C + sqrt(C^2 + 4 I+ I-)) / (2 I+),  v = 2 log y
    du/dt = j0(u) (exp(-alpha eta) - exp((1 - alpha) eta))   eta = mu + v

The constant-current right-hand side needs two sums over the whole environment before any cell's rate is known: two
launches per evaluation behind the ordinary stage launcher, so ``Euler``, ``RK4``, ``Tsit5`` (fixed step and
``PIDController``) work as for any equation.  ``derivs="fourier"`` raises ``NotImplementedError``: upstream's
``rhs_fourier`` of these classes refers to an ``R`` that does not exist.  ``mu`` and ``j0`` are closures of the in-kernel
family; ``j0`` alone may also be ``sqrt(polynomial)`` (``SQRT_WRAP``: the notebook's ``sqrt((1 - c) c)``).
"""

from __future__ import annotations

import dataclasses
from typing import Any

import numpy as np

from ... import _lib as L
from ..closures import JIT, UnsupportedClosureError, as_closure
from ..domains import Domain
from .base_eq import BaseEquation
from .phase_field import _install_spectral
from .smoothed_boundary import _norm_grad_over_psi

VOLTAGE_BATCH = 64  # states per upload of get_voltage on a stack


def _bv_closure(fn, name, sqrt_wrap=True):
    desc = as_closure(fn, sqrt_wrap=sqrt_wrap)
    if desc.kind == JIT:
        raise UnsupportedClosureError(f"{name} is outside the closure family the Butler-Volmer kernels evaluate (polynomial / "
                                      "Legendre series, logit prior, mixing entropy, exp or sqrt of those); run-time-compiled "
                                      "closures are not supported here")
    return desc


class _ButlerVolmer(BaseEquation):
    _equation_code = L.EQ_ALLEN_CAHN_BV
    _mode = L.BV_CONSTANT_CURRENT
    _value_name = "Crate"  # the per-environment number: the current, or the voltage

    def rhs(self, state, t):  # replaced in __post_init__, as upstream
        raise NotImplementedError("rhs method not implemented")

    def _init_common(self):
        if len(self.domain.points) != 2:
            raise ValueError(f"{type(self).__name__} needs a 2-D domain")
        if self.derivs == "fourier":
            raise NotImplementedError(f"{type(self).__name__}: derivs='fourier' is not implemented (upstream's rhs_fourier of the "
                                      "Butler-Volmer classes refers to an R that does not exist); use derivs='fd'")
        if self.derivs != "fd":
            raise ValueError(f"Invalid derivative type: {self.derivs}")
        self._mu_desc = _bv_closure(self.mu, "mu", sqrt_wrap=False)  # SQRT_WRAP is the exchange current's alone
        self._mob_desc = _bv_closure(self.j0, "j0")
        self.rhs = self.rhs_fd

    def _engine_problem(self):
        nx, ny = self.domain.points
        hx, hy = self.domain.dx
        return dict(equation=self._equation_code, nx=nx, ny=ny, hx=hx, hy=hy, kappa=float(self.kappa),
                    mu=self._mu_desc, mob=self._mob_desc, derivs=L.DERIVS_FD)

    def _value(self):
        return float(getattr(self, self._value_name))

    @classmethod
    def _engine_upload_batch(cls, engine, eqs, t: float = 0.0, t_end=None):
        eq0 = eqs[0]
        if any(float(e.alpha) != float(eq0.alpha) for e in eqs):
            raise ValueError(f"{cls.__name__}: alpha is shared by the environments of one batch")
        eq0._upload_fields(engine)
        engine.set_bv_params(float(eq0.alpha), cls._mode, [e._value() for e in eqs])

    def _engine_upload(self, engine, t: float = 0.0, t_end=None):
        self._upload_fields(engine)
        engine.set_bv_params(float(self.alpha), self._mode, self._value())

    def _upload_fields(self, engine):
        engine.set_time_terms(None)  # no voltage protocol left over from another equation on this engine

    def rhs_fd(self, state, t):
        return self._run_rhs(state, t)

    def get_voltage(self, state):
        """v of the constant-current constraint for one ``(nx, ny)`` state (a float) or a stack ``(n, nx, ny)`` (an array
        ``(n,)``), evaluated on the GPU in batches: what the notebook computes with ``jax.vmap(eq.get_voltage)(ys)``"""
        from ...engine import default_engine

        a = np.asarray(state)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        single = a.ndim == 2
        if single:
            a = a[None]
        if a.ndim != 3 or tuple(a.shape[1:]) != tuple(self.domain.points):
            raise ValueError(f"state shape {np.shape(state)} does not match domain points {self.domain.points}")
        eng = default_engine()
        out = np.empty(a.shape[0], dtype=np.float64)
        configured = None
        for lo in range(0, a.shape[0], VOLTAGE_BATCH):
            chunk = a[lo:lo + VOLTAGE_BATCH]
            if chunk.shape[0] != configured:  # once per distinct chunk size: the full chunks, then the remainder
                eng.configure(dtype=a.dtype, batch=chunk.shape[0], **self._engine_problem())
                self._engine_upload(eng, 0.0)
                configured = chunk.shape[0]
            eng.set_state(chunk)
            out[lo:lo + chunk.shape[0]] = eng.bv_voltage()
        return float(out[0]) if single else out


@_install_spectral
@dataclasses.dataclass
class AllenCahn2DPeriodicButlerVolmer(_ButlerVolmer):
    """du/dt = j0(u) (exp(-alpha (mu + v)) - exp((1 - alpha)(mu + v))) at a given voltage.  ``v`` (new, trailing): the
    voltage a solve uses -- a number, or a callable of ``t`` sampled on the host at every right-hand-side time."""

    domain: Domain
    kappa: float
    mu: Any
    j0: Any
    alpha: float
    derivs: str = "fd"
    v: Any = 0.0

    _mode = L.BV_VOLTAGE
    _value_name = "v"
    _per_env_controls = frozenset({"kappa", "mu", "j0", "v"})

    def __post_init__(self):
        self._init_common()

    def _value(self):
        return 0.0 if callable(self.v) else float(self.v)

    def _upload_fields(self, engine):
        if callable(self.v):  # the protocol v(t) is added to the per-environment number (0) at every stage time
            engine.set_time_terms(lambda t: (float(self.v(t)), 0.0, 0.0))
        else:
            engine.set_time_terms(None)

    def _time_dependent_rhs(self, t0: float = 0.0, t1=None) -> bool:
        return callable(self.v)

    def rhs_fd(self, state, t, v=None):
        """``rhs_fd(state, t, v)`` as upstream; without ``v`` the equation's own field is used"""
        if v is None:
            return self._run_rhs(state, t)
        return dataclasses.replace(self, v=float(v))._run_rhs(state, t)


@_install_spectral
@dataclasses.dataclass
class AllenCahn2DPeriodicButlerVolmerConstantCurrent(_ButlerVolmer):
    """the same rate with v solving the constant-current constraint h^2 sum du/dt = Crate (exact for alpha = 1/2)"""

    domain: Domain
    kappa: float
    mu: Any
    j0: Any
    alpha: float
    Crate: float
    derivs: str = "fd"

    _per_env_controls = frozenset({"kappa", "mu", "j0", "Crate"})

    def __post_init__(self):
        self._init_common()


@dataclasses.dataclass
class AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent(_ButlerVolmer):
    """constant current on a smoothed-boundary geometry: mu through the psi-weighted Laplacian, sums weighted by psi.
    ``f`` is accepted and unused, as upstream (the wall term is commented out there)."""

    domain: Domain
    kappa: float
    f: Any
    mu: Any
    j0: Any
    alpha: float
    Crate: float
    derivs: str = "fd"

    _equation_code = L.EQ_ALLEN_CAHN_SBM_BV
    _per_env_controls = frozenset({"kappa", "mu", "j0", "Crate"})

    def __post_init__(self):
        if self.domain.geometry is None or not hasattr(self.domain.geometry, "smooth"):
            raise ValueError("AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent needs domain.geometry.smooth (the level-set field psi)")
        self._init_common()
        self.psi = np.asarray(self.domain.geometry.smooth, dtype=np.float64)
        if self.psi.shape != tuple(self.domain.points):
            raise ValueError(f"psi shape {self.psi.shape} does not match domain points {self.domain.points}")
        self.sqrt_kappa = np.sqrt(self.kappa)
        self.hx, self.hy = self.domain.dx
        self.norm_grad_psi = _norm_grad_over_psi(self.psi, self.hx, self.hy)
        self.left_half = np.zeros_like(self.psi)
        self.left_half[:, :100] = 1.0  # allen_cahn.py:317 (published, unused)

    def _upload_fields(self, engine):
        engine.set_time_terms(None)
        engine.set_aux(L.AUX_SBM_PSI, self.psi)
