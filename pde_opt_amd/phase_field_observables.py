"""Free energy, dissipation and mass of a phase-field state, summed on the device.

The device sums eight numbers per environment over the resident state (``pdeopt_pf_observables``, csrc/pf_obs.hip;
DESIGN.md section 4.19).  With ``h = prod(dx)``, ``mu = mu_h(u) - kappa lap(u)`` the 5- / 7-point chemical potential of
the finite-difference right-hand side, ``grad_f`` the forward difference to the face and ``D_f`` the face average of
``D(u)``

    mass   = h sum u           u2  = h sum u^2          f_bulk = h sum f_h(u),  f_h' = mu_h, f_h(0) = 0
    f_grad = h sum kappa/2 sum_axes (grad_f u)^2        mu  = h sum mu          mu2 = h sum mu^2
    diss   = h sum_faces D_f (grad_f mu)^2  (Cahn-Hilliard),  h sum R(u) mu^2  (Allen-Cahn)
    nonfinite = number of cells whose u or mu is not finite

so that ``d(f_bulk + f_grad)/du_ij = h mu_ij`` and ``d(f_bulk + f_grad)/dt = -diss`` along ``u_t = rhs_fd(u)``, both to
rounding.  The host derives ``free_energy = f_bulk + f_grad``, ``mean = mass / |Omega|``, ``mu_mean = mu / |Omega|``,
``mu_variance = mu2 / |Omega| - mu_mean^2`` and ``dissipation = diss``.

Covered: ``CahnHilliard2DPeriodic``, ``AllenCahn2DPeriodic``, ``CahnHilliard3DPeriodic`` with ``derivs="fd"``; ``mu`` a
polynomial or a Legendre series, with or without the ``log(c / (1 - c))`` prior (the forms with a closed antiderivative);
``D`` / ``R`` any closure of the in-kernel family.
"""

from __future__ import annotations

import dataclasses
from typing import Any, Dict, Sequence, Union

import numpy as np

from . import _lib as L
from . import diagnostics as D
from . import fit
from .numerics import closures as CLS

RAW_NAMES = ("mass", "u2", "f_bulk", "f_grad", "mu", "mu2", "diss", "nonfinite")
DERIVED_NAMES = ("free_energy", "mean", "mu_mean", "mu_variance", "dissipation", "nonfinite")
REWARD_NAMES = RAW_NAMES + tuple(n for n in DERIVED_NAMES if n not in RAW_NAMES)

SUPPORT = ('the free energy is summed for CahnHilliard2DPeriodic, AllenCahn2DPeriodic and CahnHilliard3DPeriodic with '
           'derivs="fd" and a mu that is a polynomial or a Legendre series, with or without the log(c / (1 - c)) prior')


@dataclasses.dataclass
class PhaseFieldObservables:
    """one float64 array per name of ``RAW_NAMES`` and ``DERIVED_NAMES``: ``(B,)`` from ``free_energy``,
    ``(len(ts), B)`` from ``free_energy_trace``; ``volume`` is ``|Omega|``"""

    mass: np.ndarray
    u2: np.ndarray
    f_bulk: np.ndarray
    f_grad: np.ndarray
    mu: np.ndarray
    mu2: np.ndarray
    diss: np.ndarray
    nonfinite: np.ndarray
    free_energy: np.ndarray
    mean: np.ndarray
    mu_mean: np.ndarray
    mu_variance: np.ndarray
    dissipation: np.ndarray
    volume: float

    @classmethod
    def from_raw(cls, raw, volume: float) -> "PhaseFieldObservables":
        """``raw``: ``(..., 8)`` rows of ``HipEngine.pf_observables``; ``volume``: ``|Omega|`` of the domain"""
        raw = np.asarray(raw, dtype=np.float64)
        if raw.ndim < 2 or raw.shape[-1] != L.PF_OBS_COUNT:
            raise ValueError(f"raw observables have shape (..., {L.PF_OBS_COUNT}), got {raw.shape}")
        cols = {name: raw[..., i].copy() for i, name in enumerate(RAW_NAMES)}
        volume = float(volume)
        mu_mean = cols["mu"] / volume
        return cls(free_energy=cols["f_bulk"] + cols["f_grad"], mean=cols["mass"] / volume, mu_mean=mu_mean,
                   mu_variance=cols["mu2"] / volume - mu_mean**2, dissipation=cols["diss"].copy(), volume=volume, **cols)

    def __getitem__(self, name: str) -> np.ndarray:
        if name not in REWARD_NAMES:
            raise KeyError(name)
        return getattr(self, name)


def volume_of(domain) -> float:
    """``|Omega|``: the number of cells times the cell volume"""
    return float(np.prod(domain.points) * np.prod(domain.dx))


def antiderivative(desc, c):
    """``f_h(c) = int_0^c mu_h`` of a closure descriptor of the covered forms, on numpy arrays (what the kernels sum as
    ``f_bulk``; host utility).  Polynomial: ``sum a_k c^(k+1) / (k+1)``; Legendre series on ``x = 2c - 1``: ``a_0 c +
    sum_{k>=1} a_k (P_{k+1}(x) - P_{k-1}(x)) / (2 (2k + 1))``; the logit prior adds ``c ln c + (1 - c) ln(1 - c)``, taken
    as 0 at ``c = 0, 1``."""
    check_closures(desc, None)
    c = np.asarray(c, dtype=np.float64)
    a = np.asarray(desc.coef, dtype=np.float64)
    if desc.kind == CLS.POLY:
        r = sum(a[k] * c ** (k + 1) / (k + 1) for k in range(len(a)))
    else:
        x = 2.0 * c - 1.0
        r = a[0] * c
        pm, pc = np.ones_like(x), x
        for k in range(1, len(a)):
            pn = ((2 * k + 1) * x * pc - k * pm) / (k + 1)
            r = r + a[k] * (pn - pm) / (2 * (2 * k + 1))
            pm, pc = pc, pn
    if desc.flags & CLS.LOGIT_PRIOR:
        with np.errstate(divide="ignore", invalid="ignore"):
            r = r + np.where(c == 0, 0.0, c * np.log(c)) + np.where(c == 1, 0.0, (1 - c) * np.log(1 - c))
    return r


# ---- refusals: all of them need neither an engine nor a GPU -----------------------------------------------------------

def reject_unsupported(equation_type) -> None:
    """the three periodic phase-field classes have this free energy: say so before an engine exists"""
    from .numerics.equations.phase_field import AllenCahn2DPeriodic, CahnHilliard2DPeriodic, CahnHilliard3DPeriodic

    if equation_type not in (CahnHilliard2DPeriodic, AllenCahn2DPeriodic, CahnHilliard3DPeriodic):
        raise NotImplementedError(f"{getattr(equation_type, '__name__', equation_type)} has no free energy here: " + SUPPORT +
                                  " (the smoothed-boundary, Butler-Volmer, advection-diffusion and GPE classes are not covered)")


def check_closures(mu_desc, mob_desc) -> None:
    """``ValueError`` for closures the sums are not defined for (``mob_desc=None``: mu alone)"""
    if mu_desc.kind == CLS.JIT or (mob_desc is not None and mob_desc.kind == CLS.JIT):
        raise ValueError("a closure compiled at run time (outside the in-kernel family) has no antiderivative here: " + SUPPORT)
    for flag, name in ((CLS.MIX_ENTROPY, "the mixing entropy c log c + (1 - c) log(1 - c)"), (CLS.EXP_WRAP, "an exp(.) wrap")):
        if mu_desc.flags & flag:
            raise ValueError(f"mu with {name} has no closed-form antiderivative: " + SUPPORT)


def check_equation(eq) -> None:
    """``ValueError`` for an equation OBJECT of a covered class whose configuration is not covered"""
    reject_unsupported(type(eq))
    if getattr(eq, "_mu_module", None) is not None:
        raise ValueError("mu is a torch.nn.Module: a network has no antiderivative here: " + SUPPORT)
    if eq.derivs != "fd":
        raise ValueError(f'derivs="{eq.derivs}": the sums are discretised with the finite-difference right-hand side: ' + SUPPORT)
    check_closures(eq._mu_desc, eq._mob_desc)


# ---- PDEModel.free_energy / free_energy_trace ----------------------------------------------------------------------------

def _equations(model, parameters, batch):
    eqs = [model.equation_type(domain=model.domain, **fit.plain(p)) for p in D.parameter_sets(parameters, batch)]
    for eq in eqs:
        check_equation(eq)
    structure = {(e._mu_desc.kind, e._mu_desc.flags, len(e._mu_desc.coef), e._mob_desc.kind, e._mob_desc.flags, len(e._mob_desc.coef))
                 for e in eqs}
    if len(structure) != 1:
        raise ValueError("the environments of a batch share the closures' structure (kind, flags, number of coefficients); "
                         "only the coefficient values and kappa may differ")
    return eqs


def _load(model, eqs, solver, yb, t0=0.0, t1=None):
    """``diagnostics.load`` with the per-environment kappa and coefficients of ``eqs`` where there is one per environment"""
    per_env = None
    if len(eqs) > 1:
        probs = [e._engine_problem() for e in eqs]
        per_env = lambda eng: eng.set_env_params(0, kappa=[p["kappa"] for p in probs], mu_coef=[p["mu"].coef for p in probs],
                                                 mob_coef=[p["mob"].coef for p in probs])
    return D.load(model, eqs, solver, yb, t0, t1, per_env=per_env)


def free_energy(model, parameters: Union[Dict[str, Any], Sequence[Dict[str, Any]]], state) -> PhaseFieldObservables:
    """``PDEModel.free_energy``"""
    reject_unsupported(model.equation_type)
    yb, _ = D.batch_states(model, state)
    eqs = _equations(model, parameters, yb.shape[0])
    eng = _load(model, eqs, None, yb)
    return PhaseFieldObservables.from_raw(eng.pf_observables(), volume_of(model.domain))


def free_energy_trace(model, parameters, y0, ts, solver_parameters=None, dt0=1e-6) -> PhaseFieldObservables:
    """``PDEModel.free_energy_trace``"""
    reject_unsupported(model.equation_type)
    rows = D.trace_on_step_edges(
        model, parameters, y0, ts, solver_parameters, dt0, name="free_energy_trace",
        why="the energy of a linear interpolation of states is not an interpolation of energies",
        states=lambda y: D.batch_states(model, y)[0], equation=lambda yb: _equations(model, parameters, yb.shape[0])[0],
        equation_first=True, read=lambda eng: eng.pf_observables())  # 64 bytes per environment come back
    return PhaseFieldObservables.from_raw(rows, volume_of(model.domain))


def _reward(env, eng, eqs, eq0):
    """``("phase_field", name)``: a free-energy observable of the state after the step, summed on the device with the
    per-environment kappa and coefficients the engine carries (64 bytes per environment come back)"""
    return PhaseFieldObservables.from_raw(eng.pf_observables(), volume_of(env.domain))[env.device_reward[1]]


# precheck: derivs and closures of the equation OBJECT, refused before the engine is touched
DEVICE_REWARD = D.DeviceReward(REWARD_NAMES, reject_unsupported, _reward, precheck=check_equation)
