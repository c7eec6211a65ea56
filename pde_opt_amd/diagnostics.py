"""The host path the device diagnostics share (``gpe_observables``, ``phase_field_observables``, ``structure_factor``;
DESIGN.md section 4.11): the states of a call as one batch, its parameter sets, the model's engine loaded with both, a
solve that reads one row per save point, and the record ``VectorPDEEnv`` looks a tuple device reward up by."""

from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np

from . import fit
from .utils import prepare_solver_params


class DeviceReward(NamedTuple):
    """``device_reward=(kind, name)`` of ``VectorPDEEnv``: the ``names`` a kind takes, ``reject(equation_type)`` for the
    classes it does not cover, ``evaluate(env, eng, eqs, eq0)`` = the ``(n,)`` rewards of the engine's resident states
    after a step, and ``precheck(eq0)``, run before the engine is touched"""

    names: Tuple[str, ...]
    reject: Callable
    evaluate: Callable
    precheck: Optional[Callable] = None


def engine_of(model):
    """the model's engine, created at its first use"""
    if model._engine is None:
        from .engine import HipEngine

        model._engine = HipEngine(model.device)
    return model._engine


def batch_states(model, state, trailing=(), complex_message=None, contiguous=False):
    """``(yb, single)``: ``state`` as fp32 / fp64 of shape ``(B,) + domain.points + trailing``, and whether it came without
    the ``(B,)``.  ``complex_message``: the ``ValueError`` a complex array gets (None: it is converted like any dtype)"""
    y = np.asarray(state)
    if complex_message is not None and np.iscomplexobj(y):
        raise ValueError(complex_message)
    if y.dtype not in (np.float32, np.float64):
        y = y.astype(np.float64)
    want = tuple(model.domain.points) + tuple(trailing)
    nd = len(want)
    if y.ndim not in (nd, nd + 1) or tuple(y.shape[-nd:]) != want:
        raise ValueError(f"state of shape {y.shape}: expected {want} or (B,) + that")
    single = y.ndim == nd
    yb = y[None] if single else y
    return (np.ascontiguousarray(yb) if contiguous else yb), single


def parameter_sets(parameters, batch):
    """one dict shared by the batch, or one per state"""
    plist = [parameters] if isinstance(parameters, dict) else list(parameters)
    if len(plist) not in (1, batch):
        raise ValueError(f"{len(plist)} parameter sets for {batch} states: one dict, or one per state")
    return plist


def load(model, eqs, solver, yb, t0=0.0, t1=None, per_env=None, upload=None):
    """the model's engine configured for ``eqs`` (one: shared by the batch; else one per environment) and holding the
    states ``yb``.  ``upload(eng)`` stands in for ``eqs[0]._engine_upload`` (a class with per-environment fields);
    ``per_env(eng)`` runs after the solver's configuration (per-environment numbers of the engine's table)"""
    eng = engine_of(model)
    eq0 = eqs[0]
    eng.configure(dtype=yb.dtype, batch=yb.shape[0], **eq0._engine_problem())
    if upload is None:
        eq0._engine_upload(eng, t0, t1)
    else:
        upload(eng)
    if solver is not None:
        solver.configure_engine(eng, eq0)
    if per_env is not None:
        per_env(eng)
    eng.set_state(yb)
    return eng


def trace_on_step_edges(model, parameters, y0, ts, solver_parameters, dt0, *, name, why, states, equation, equation_first,
                        read, prepare=None):
    """The solve of ``PDEModel.solve`` in constant steps of ``dt0`` with ``read(eng)`` at every save point: the stacked
    rows ``(len(ts), ...)``.  ``name``: the calling method's; ``why``: why a save point inside a step is refused;
    ``states(y0)``: the batch; ``equation(yb)``: the equation object, built and checked before ``ts`` is looked at
    (``equation_first``) or after every refusal that needs none; ``prepare(eng)``: uploads of the loaded engine"""
    from .numerics.solvers import RK4, Euler, SemiImplicitFourierSpectral

    if model.solver_type not in (Euler, RK4, SemiImplicitFourierSpectral):
        raise NotImplementedError(f"{name} steps with Euler, RK4 or SemiImplicitFourierSpectral (constant steps), "
                                  f"not {getattr(model.solver_type, '__name__', model.solver_type)}")
    if not isinstance(parameters, dict):
        raise ValueError(f"{name} runs the solve of PDEModel.solve: one parameter dict for the batch")
    yb = states(y0)
    eq = equation(yb) if equation_first else None
    ts = np.asarray(ts, dtype=np.float64)
    if ts.ndim != 1 or len(ts) < 1:
        raise ValueError("ts is a non-empty 1-D sequence of save times")
    t0, t1, dt = float(ts[0]), float(ts[-1]), float(dt0)

    def on_edges(q, theta):
        if theta is not None:
            raise ValueError(f"save point ts[{q}] = {ts[q]!r} lies inside a step of dt0 = {dt!r} (at {theta:.6g} of it): {why}; "
                             "put ts on step edges (ts[0] + k dt0, and ts[-1])")

    fit.walk_save_points(t0, t1, dt, ts, lambda *a: None, lambda: None, on_edges)  # dry run: refuse before an engine exists
    if eq is None:
        eq = equation(yb)
    solver = model.solver_type(**prepare_solver_params(model.solver_type, solver_parameters or {}, eq))
    eng = load(model, [eq], solver, yb, t0, t1)
    if prepare is not None:
        prepare(eng)
    rows = []
    fit.walk_save_points(t0, t1, dt, ts, lambda h, n, t: eng.advance(solver.integrator, h, n, t), lambda: None,
                         lambda q, theta: rows.append(read(eng)))
    return np.stack(rows)
