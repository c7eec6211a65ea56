"""Observables of a Gross-Pitaevskii state and the imaginary-time ground-state solve built on them.

The device sums eight numbers per environment over the resident wavefunction (``pdeopt_gpe_observables``,
csrc/gpe_obs.hip): with ``psi^x`` / ``psi^y`` the unnormalised transforms along x / y,
``Px = |psi^x|^2 / nx``, ``Py = |psi^y|^2 / ny``, ``kx, ky = domain.fft_mesh()`` and ``h^2 = dx[0] dx[1]``

    norm  = h^2 sum |psi|^2            e_pot = h^2 sum V |psi|^2            e_int = h^2 sum k/2 |psi|^4
    e_kin = h^2 [sum 1/2 (2 pi kx)^2 Px + sum 1/2 (2 pi ky)^2 Py]
    l_z   = h^2 [sum x (2 pi ky) Py - sum y (2 pi kx) Px]                   x2, y2 = h^2 sum x^2 |psi|^2, h^2 sum y^2 |psi|^2

(Bao & Cai 2012; the rotating frame: Bao & Wang 2006; ``l_z = <x p_y - y p_x>`` carries the signs of
``GPE2DTSRot.A_terms``).  The host derives

    energy = (kappa e_kin + e_pot + e_int - omega l_z) / norm,    mu = (kappa e_kin + e_pot + 2 e_int - omega l_z) / norm

with ``omega`` the equation's rotation frequency (0 for ``GPE2DTSControl``) and ``kappa = 1``, except ``kappa = 0`` for
a ``GPE2DTSControl`` with ``kinetic=False``, whose committed ``A_term`` is zero: its dynamics has no kinetic term
(``e_kin`` itself is still reported).
"""

from __future__ import annotations

import dataclasses
from typing import Any, Dict, Sequence, Union

import numpy as np

from . import _lib as L
from . import diagnostics as D
from .utils import prepare_solver_params

OBSERVABLE_NAMES = ("norm", "e_kin", "e_pot", "e_int", "l_z", "x2", "y2")
DERIVED_NAMES = ("energy", "mu")


@dataclasses.dataclass
class GpeObservables:
    """one ``(B,)`` float64 array per name of ``OBSERVABLE_NAMES``, plus ``energy`` and ``mu`` (per particle: divided
    by ``norm``) with the equation's ``omega`` and kinetic weight ``kappa`` folded in"""

    norm: np.ndarray
    e_kin: np.ndarray
    e_pot: np.ndarray
    e_int: np.ndarray
    l_z: np.ndarray
    x2: np.ndarray
    y2: np.ndarray
    energy: np.ndarray
    mu: np.ndarray
    omega: np.ndarray
    kappa: float

    @classmethod
    def from_raw(cls, raw, omega=0.0, kappa: float = 1.0) -> "GpeObservables":
        """``raw``: the ``(B, 8)`` rows of ``HipEngine.gpe_observables``"""
        raw = np.asarray(raw, dtype=np.float64)
        if raw.ndim != 2 or raw.shape[1] != L.GPE_OBS_COUNT:
            raise ValueError(f"raw observables have shape (B, {L.GPE_OBS_COUNT}), got {raw.shape}")
        cols = {name: raw[:, i].copy() for i, name in enumerate(OBSERVABLE_NAMES)}
        omega = np.broadcast_to(np.asarray(omega, dtype=np.float64), (raw.shape[0],)).copy()
        common = float(kappa) * cols["e_kin"] + cols["e_pot"] - omega * cols["l_z"]
        return cls(energy=(common + cols["e_int"]) / cols["norm"], mu=(common + 2.0 * cols["e_int"]) / cols["norm"],
                   omega=omega, kappa=float(kappa), **cols)

    def __getitem__(self, name: str) -> np.ndarray:
        if name not in OBSERVABLE_NAMES + DERIVED_NAMES:
            raise KeyError(name)
        return getattr(self, name)


@dataclasses.dataclass
class GroundState:
    """result of ``PDEModel.ground_state``: the relaxed ``state`` (shape of ``y0``), its ``observables``, per
    environment the step count ``steps`` at which the energy criterion was first met (the number of steps taken where
    it never was) and ``converged``, and ``history`` ``(n_checks, B, 2)`` = (energy, mu) at every check"""

    state: np.ndarray
    observables: GpeObservables
    steps: np.ndarray
    converged: np.ndarray
    history: np.ndarray


GROUND_STATE_SUPPORT = ("ground_state relaxes in ONE potential and ONE rotating frame: it supports omega_rate = 0 and lights "
                        "that do not depend on time (GaussianSpots with zero rates: a pinning beam, folded into the potential)")


def reject_moving_frame(parameters) -> None:
    """``ValueError`` for parameter sets a ground state does not belong to; needs no engine and no GPU"""
    for p in ([parameters] if isinstance(parameters, dict) else list(parameters)):
        if p.get("omega_rate"):
            raise ValueError(f"omega_rate={p['omega_rate']!r}: " + GROUND_STATE_SUPPORT)
        if getattr(p.get("lights"), "time_dependent", False):
            raise ValueError("time-dependent spots: " + GROUND_STATE_SUPPORT)


def reject_unsupported(equation_type) -> None:
    """the observables are those of the two GPE classes: say so before an engine exists"""
    from .numerics.equations.gross_pitaevskii import GPE2DTSControl, GPE2DTSRot

    if equation_type not in (GPE2DTSControl, GPE2DTSRot):
        raise NotImplementedError(f"energy, chemical potential and L_z are observables of GPE2DTSControl and GPE2DTSRot; "
                                  f"{getattr(equation_type, '__name__', equation_type)} has none")


def equation_weights(eqs, t: float = 0.0):
    """``(omega (B,), kappa)`` of the equations of a batch at local time ``t`` (a ``GPE2DTSRot`` with an ``omega_rate``
    rotates with ``omega + omega_rate t``)"""
    omega = np.asarray([float(getattr(e, "omega", 0.0)) + float(getattr(e, "omega_rate", 0.0)) * float(t) for e in eqs])
    kinetic = {bool(getattr(e, "kinetic", True)) for e in eqs}
    if len(kinetic) != 1:
        raise ValueError("all environments of a batch must share A_term (the `kinetic` switch)")
    return omega, 1.0 if kinetic.pop() else 0.0


def _states(model, state):
    return D.batch_states(model, state, trailing=(2,), complex_message="complex states are stored as (..., 2) real/imag pairs")


def _equations(model, parameters, batch):
    return [model.equation_type(domain=model.domain, **p) for p in D.parameter_sets(parameters, batch)]


def _load(model, eqs, solver, yb, t, t_end):
    """the model's engine configured for ``eqs`` (one: shared by the batch; else one per environment) and holding
    the states ``yb``"""
    batch = (lambda eng: type(eqs[0])._engine_upload_batch(eng, eqs, t, t_end)) if len(eqs) > 1 else None
    return D.load(model, eqs, solver, yb, t, t_end, upload=batch)


def observables(model, parameters: Union[Dict[str, Any], Sequence[Dict[str, Any]]], state, t: float = 0.0) -> GpeObservables:
    """``PDEModel.observables``"""
    reject_unsupported(model.equation_type)
    yb, _ = _states(model, state)
    eqs = _equations(model, parameters, yb.shape[0])
    omega, kappa = equation_weights(eqs, float(t))
    # t_end = t: a GaussianSpots control stays in its in-kernel form and is evaluated at t on the device
    eng = _load(model, eqs, None, yb, float(t), float(t))
    return GpeObservables.from_raw(eng.gpe_observables(float(t)), omega, kappa)


def ground_state(model, parameters, y0, dt, tol=1e-8, max_steps=100_000, check_every=25, solver_parameters=None) -> GroundState:
    """``PDEModel.ground_state``"""
    reject_unsupported(model.equation_type)
    if getattr(model.equation_type, "_rotating_frame", False):
        reject_moving_frame(parameters)
    solver_parameters = dict(solver_parameters or {})
    if complex(solver_parameters.setdefault("time_scale", -1j)) != -1j:
        raise ValueError(f"ground_state integrates in imaginary time (time_scale=-1j), got time_scale={solver_parameters['time_scale']!r}")
    dt, check_every, max_steps = float(dt), int(check_every), int(max_steps)
    if not dt > 0 or check_every < 1 or max_steps < 1:
        raise ValueError("ground_state needs dt > 0, check_every >= 1 and max_steps >= 1")
    yb, single = _states(model, y0)
    B = yb.shape[0]
    eqs = _equations(model, parameters, B)
    omega, kappa = equation_weights(eqs)
    solver = model.solver_type(**prepare_solver_params(model.solver_type, solver_parameters, eqs[0]))
    # t_end = None: a control that depends on time is frozen at t = 0 for the steps AND for the energy (a ground state
    # belongs to one potential); nothing is sampled per substep
    eng = _load(model, eqs, solver, yb, 0.0, None)
    steps = np.zeros(B, dtype=np.int64)
    converged = np.zeros(B, dtype=bool)
    history, done, prev, obs = [], 0, None, None
    while done < max_steps:
        n = min(check_every, max_steps - done)
        eng.advance(solver.integrator, dt, n, done * dt)
        done += n
        obs = GpeObservables.from_raw(eng.gpe_observables(0.0), omega, kappa)  # 64 bytes per environment come back
        history.append(np.stack([obs.energy, obs.mu], axis=-1))
        if prev is not None:
            newly = ~converged & (np.abs(obs.energy - prev) / (n * dt) <= tol)
            steps[newly] = done
            converged |= newly
        prev = obs.energy
        if converged.all():
            break
    steps[~converged] = done
    state = eng.get_state()
    return GroundState(state[0] if single else state, obs, steps, converged, np.stack(history))


def _reward(env, eng, eqs, eq0):
    """``("gpe", name)``: an observable of the GPE state, summed on the device (64 bytes per environment come back); the
    potential is the one a substep starting at the end of this step would use, energy and mu are in the frame of the
    step's end: Omega(step_dt) of an equation with an omega_rate"""
    from .pde_env import _ScalarControlBatch

    if isinstance(eqs, _ScalarControlBatch):
        omega, kappa = equation_weights([eq0], float(env.step_dt))
        if eqs.name == "omega":
            omega = np.asarray(eqs.values, dtype=np.float64)
    else:
        omega, kappa = equation_weights(eqs, float(env.step_dt))
    return GpeObservables.from_raw(eng.gpe_observables(float(env.step_dt)), omega, kappa)[env.device_reward[1]]


DEVICE_REWARD = D.DeviceReward(OBSERVABLE_NAMES + DERIVED_NAMES, reject_unsupported, _reward)
