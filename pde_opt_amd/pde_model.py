"""PDEModel.solve on the HIP engine (the reference's pde_opt/pde_model.py:37-136).

``solve(parameters, y0, ts, solver_parameters, adjoint, dt0, max_steps, stepsize_controller)``
keeps the upstream signature and returns ``ys`` of shape ``(len(ts), *y0.shape)``; like upstream
it never throws on divergence (``throw=False``: NaNs are returned).  ``adjoint`` is accepted and
ignored: forward solves need no adjoint.

``train`` / ``residuals`` / ``mse`` / ``regularization`` (pde_model.py:138-460) fit closure coefficients to
trajectories: the derivative of the solve comes from forward-mode tangents advanced on the GPU next to the
trajectories (``pde_opt_amd.fit``; csrc/sens.hip) -- periodic Cahn-Hilliard in 2-D or 3-D (``mu`` / ``D``; IMEX or
Euler) and periodic 2-D Allen-Cahn (``mu`` / ``R``; Euler or RK4), with FD derivatives.
``optimize`` (pde_model.py:462-551) keeps raising: its objective is an arbitrary function of the solution.
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

    def optimize(self, *a, **k):
        raise NotImplementedError(
            "PDEModel.optimize minimises an arbitrary function of the solution and needs its gradient; only "
            "train / residuals / mse (closure coefficients fitted to trajectories) are provided"
        )


def stack_training_data(data, inds):
    """``(y0s, values, ts)`` of a training set, as the reference builds them (pde_model.py:378-390): trajectory b
    starts at ``data["ys"][inds[b][0]]`` and is compared at ``inds[b][1:]``; the times are those of ``inds[0]``
    relative to its first"""
    ys = data["ys"]
    y0s = np.stack([np.asarray(ys[ind[0]]) for ind in inds])
    values = np.stack([np.stack([np.asarray(ys[ind[i]]) for i in range(1, len(ind))]) for ind in inds])
    ts = np.array([float(data["ts"][inds[0][i]]) - float(data["ts"][inds[0][0]]) for i in range(len(inds[0]))])
    return y0s, values, ts
