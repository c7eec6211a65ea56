"""PDEModel.solve on the HIP engine (the reference's pde_opt/pde_model.py:37-136).

``solve(parameters, y0, ts, solver_parameters, adjoint, dt0, max_steps, stepsize_controller)``
keeps the upstream signature and returns ``ys`` of shape ``(len(ts), *y0.shape)``; like upstream
it never throws on divergence (``throw=False``: NaNs are returned).  ``adjoint`` is accepted and
ignored: forward solves need no adjoint.

``train`` / ``residuals`` / ``mse`` / ``regularization`` (pde_model.py:138-460) fit closure coefficients to
trajectories: the derivative of the solve comes from forward-mode tangents advanced on the GPU next to the
trajectories (``pde_opt_amd.fit``; csrc/sens.hip) -- periodic Cahn-Hilliard in 2-D or 3-D (``mu`` / ``D``; IMEX or
Euler) and periodic 2-D Allen-Cahn (``mu`` / ``R``; Euler or RK4), with FD derivatives.
``optimize`` (pde_model.py:462-551) minimises a scalar objective of the saved solution over the same coefficients with
BFGS: the objective is a torch-differentiable callable or an object with ``value_and_grad(ys)``; its cotangent
``dJ/dys`` is contracted with the same tangents on the GPU (``pdeopt_sens_contract``).  Objectives in neither form, and
the equations / solvers / closures ``train`` refuses, raise ``NotImplementedError``.
"""

from __future__ import annotations

from typing import Any, Dict, Optional

import numpy as np

from . import fit
from .engine import HipEngine
from .integrate import diffeqsolve
from .numerics.solvers import ConstantStepSize, SaveAt
from .utils import check_equation_solver_compatibility, prepare_solver_params


class PDEModel:
    def __init__(self, equation_type, domain, solver_type, device: int = 0):
        self.equation_type = equation_type
        self.domain = domain
        self.solver_type = solver_type
        self.device = device
        check_equation_solver_compatibility(self.solver_type, self.equation_type)
        self._engine: Optional[HipEngine] = None

    def solve(
        self,
        parameters: Dict[str, Any],
        y0,
        ts,
        solver_parameters: Optional[Dict[str, Any]] = None,
        adjoint=None,
        dt0=0.000001,
        max_steps=1000000,
        stepsize_controller=None,
    ):
        equation = self.equation_type(domain=self.domain, **parameters)
        solver = self.solver_type(**prepare_solver_params(self.solver_type, solver_parameters or {}, equation))
        if self._engine is None:
            self._engine = HipEngine(self.device)
        ts = np.asarray(ts, dtype=np.float64)
        sol = diffeqsolve(
            equation, solver, t0=ts[0], t1=ts[-1], dt0=dt0, y0=y0, saveat=SaveAt(ts=ts),
            stepsize_controller=stepsize_controller or ConstantStepSize(), max_steps=max_steps,
            throw=False, engine=self._engine,
        )
        return sol.ys

    # -- fitting (pde_model.py:138-460) ----------------------------------------------------------------------------
    def regularization(self, parameters, weights, lambda_reg):
        """``lambda sum_i w_i p_i^2`` over the coefficient arrays named in ``weights``; None leaves are ignored"""
        return fit.regularization(parameters, weights, lambda_reg)

    def residual_single(self, parameters, solver_parameters, y0, values, ts, adjoint=None):
        """``values - solve(...)[1:]`` of one trajectory"""
        pred = self.solve(parameters, y0, ts, solver_parameters, adjoint=adjoint)
        return np.asarray(values) - pred[1:]

    def residuals(self, parameters, y0s__values, solver_parameters, ts, weights, lambda_reg, adjoint=None):
        """``(batch_residuals (B, T - 1, *spatial), reg)``: the B trajectories run as one batched solve"""
        y0s, values = y0s__values
        pred = self.solve(parameters, np.asarray(y0s), ts, solver_parameters, adjoint=adjoint)  # (T, B, *spatial)
        batch_residuals = np.asarray(values) - np.swapaxes(pred, 0, 1)[:, 1:]
        return batch_residuals, self.regularization(parameters, weights, lambda_reg)

    def mse(self, parameters, y0s__values, solver_parameters, ts, weights, lambda_reg, adjoint=None):
        """``mean(r^2) + reg``"""
        r, reg = self.residuals(parameters, y0s__values, solver_parameters, ts, weights, lambda_reg, adjoint)
        return float(np.mean(np.asarray(r, dtype=np.float64) ** 2)) + reg

    def _sens_engine(self):
        if getattr(self, "_sens_eng", None) is None:
            self._sens_eng = HipEngine(self.device)
        return self._sens_eng

    def train(self, data, inds, opt_parameters, other_parameters, solver_parameters, weights, lambda_reg,
              method="least_squares", max_steps=100):
        """Fit the closure coefficients in ``opt_parameters`` to ``data`` (pde_model.py:288-460).

        ``method="least_squares"``: Levenberg-Marquardt on the Gauss-Newton normal equations (the reference's
        optimistix.LevenbergMarquardt with ForwardMode); ``"mse"``: BFGS on ``mean(r^2) + reg``.  ``data["ys"][i]``
        is a state of shape ``spatial``: ``(nx, ny)`` for CahnHilliard2DPeriodic and AllenCahn2DPeriodic,
        ``(nx, ny, nz)`` for CahnHilliard3DPeriodic.  Returns ``{**fitted, **other_parameters}``; each fitted closure is the class it
        started as, with its ``prior_fn``."""
        fit.reject_unsupported(self)
        if method not in ("least_squares", "mse"):
            raise ValueError(f"method must be 'least_squares' or 'mse', got {method!r}")
        pmap = fit.ParamMap.of(opt_parameters, self.equation_type)
        y0s, values, ts = stack_training_data(data, inds)
        equation0 = self.equation_type(domain=self.domain, **{**opt_parameters, **other_parameters})
        fit.check_equation(equation0)
        frames = np.ascontiguousarray(np.swapaxes(values, 0, 1))  # (T - 1, B, *spatial)
        frames_key = object()
        sens_params = pmap.sens_params()
        P = len(sens_params)
        eng = self._sens_engine()

        def setup(p):
            params = {**pmap.build(p), **other_parameters}
            equation = self.equation_type(domain=self.domain, **params)
            solver = self.solver_type(**prepare_solver_params(self.solver_type, solver_parameters or {}, equation))
            return params, equation, solver

        def sums(p):
            _, equation, solver = setup(p)
            s, _ = fit.sensitivity_solve(eng, equation, solver, y0s, ts, sens_params, frames=frames,
                                         frames_key=frames_key)
            ssr, rdp, G = fit.unpack_sums(s, P)
            return (ssr,) + pmap.expand(rdp, G)

        def ssr(p):
            params, _, _ = setup(p)
            r, _ = self.residuals(params, (y0s, values), solver_parameters, ts, {}, 0.0)
            return float(np.sum(np.asarray(r, dtype=np.float64) ** 2))

        obj = fit.Objective(sums=sums, ssr=ssr, M=int(values.size), lambda_reg=float(lambda_reg),
                            w=fit.weight_vector(pmap, weights or {}))
        p0 = pmap.flatten(opt_parameters)
        if method == "least_squares":
            p, hist = fit.levenberg_marquardt(obj, p0, max_steps=max_steps)
        else:
            p, hist = fit.bfgs(obj, p0, max_steps=max_steps)
        self.last_train_history = hist
        return {**pmap.build(p), **other_parameters}

    def optimize(self, objective_function=None, y0=None, ts=None, opt_parameters=None, other_parameters=None,
                 solver_parameters=None, weights=None, lambda_reg=0.0, max_steps=100):
        """Minimise ``objective_function(solve(...)) + regularization(...)`` over the closure coefficients in
        ``opt_parameters`` with BFGS (pde_model.py:462-551).

        ``objective_function`` is a scalar function of the saved solution ``ys`` of shape ``(len(ts), *y0.shape)``:
        either a torch-differentiable callable (it receives ``ys`` as a float64 ``torch.Tensor`` and returns a 0-d
        tensor; the counterpart of the reference's JAX-compatible objective), or an object with
        ``value_and_grad(ys) -> (float, ndarray of ys.shape)`` and optionally ``value(ys) -> float`` for numpy users.
        Anything else raises ``NotImplementedError``.  ``y0`` is one state ``spatial`` or a batch ``(B, *spatial)``.

        One gradient is two passes: ``solve`` gives ``ys``, the objective ``J`` and ``g = dJ/dys``; a sensitivity solve
        (its base block is bitwise ``solve``) with ``g[1:]`` on the device gives ``dJ/dp_j = sum_q <g_q, dys_q/dp_j>``
        (``pdeopt_sens_contract``).  Trial points of the line search are forward solves.  The equations, solvers and
        closures are those of ``train``.  Returns ``{**fitted, **other_parameters}``; the objective after every
        accepted step is in ``last_optimize_history``."""
        value_and_grad, value, pmap = self._objective_functions(objective_function, y0, ts, opt_parameters, other_parameters,
                                                                solver_parameters, weights, lambda_reg)
        p, hist = fit.minimize_bfgs(value_and_grad, value, pmap.flatten(opt_parameters), max_steps=max_steps)
        self.last_optimize_history = hist
        return {**pmap.build(p), **(other_parameters or {})}

    def _objective_functions(self, objective_function, y0, ts, opt_parameters, other_parameters, solver_parameters, weights,
                             lambda_reg):
        """``(value_and_grad(p), value(p), ParamMap)`` of ``optimize``'s objective over the flat coefficient vector"""
        other_parameters, weights = other_parameters or {}, weights or {}
        probe = None
        if y0 is not None and ts is not None:
            y0 = np.asarray(y0)
            probe = np.broadcast_to(y0.astype(np.float64), (len(ts),) + y0.shape)
        objective = fit.as_objective(objective_function, probe)  # checked first: optimize() with nothing keeps raising
        if y0 is None or ts is None or not opt_parameters:
            raise ValueError("optimize needs y0, ts and opt_parameters")
        fit.reject_unsupported(self)
        pmap = fit.ParamMap.of(opt_parameters, self.equation_type)
        fit.check_equation(self.equation_type(domain=self.domain, **{**opt_parameters, **other_parameters}))
        spatial_ndim = len(self.domain.points)
        if y0.ndim not in (spatial_ndim, spatial_ndim + 1):
            raise ValueError(f"y0 of shape {y0.shape}: expected {tuple(self.domain.points)} or (B,) + that")
        y0s = y0 if y0.ndim == spatial_ndim + 1 else y0[None]
        ts = np.asarray(ts, dtype=np.float64)
        sens_params = pmap.sens_params()
        reg = fit.Objective(sums=None, ssr=None, M=0, lambda_reg=float(lambda_reg), w=fit.weight_vector(pmap, weights))

        def params_of(p):
            return {**pmap.build(p), **other_parameters}

        def value(p):
            return objective.value(self.solve(params_of(p), y0, ts, solver_parameters)) + reg.reg(p)

        def value_and_grad(p):
            params = params_of(p)
            equation = self.equation_type(domain=self.domain, **params)
            solver = self.solver_type(**prepare_solver_params(self.solver_type, solver_parameters or {}, equation))

            def contract(cotangents):
                return fit.sensitivity_solve(self._sens_engine(), equation, solver, y0s, ts, sens_params,
                                             cotangents=cotangents)[0]

            ys = self.solve(params, y0, ts, solver_parameters)
            J, grad = fit.objective_gradient(objective, ys, spatial_ndim, contract, pmap)
            return J + reg.reg(p), grad + reg.reg_grad(p)

        return value_and_grad, value, pmap


def stack_training_data(data, inds):
    """``(y0s, values, ts)`` of a training set, as the reference builds them (pde_model.py:378-390): trajectory b
    starts at ``data["ys"][inds[b][0]]`` and is compared at ``inds[b][1:]``; the times are those of ``inds[0]``
    relative to its first"""
    ys = data["ys"]
    y0s = np.stack([np.asarray(ys[ind[0]]) for ind in inds])
    values = np.stack([np.stack([np.asarray(ys[ind[i]]) for i in range(1, len(ind))]) for ind in inds])
    ts = np.array([float(data["ts"][inds[0][i]]) - float(data["ts"][inds[0][0]]) for i in range(len(inds[0]))])
    return y0s, values, ts
