"""PDEModel.solve on the HIP engine (the reference's pde_opt/pde_model.py:37-136).

``solve(parameters, y0, ts, solver_parameters, adjoint, dt0, max_steps, stepsize_controller)``
keeps the upstream signature and returns ``ys`` of shape ``(len(ts), *y0.shape)``; like upstream
it never throws on divergence (``throw=False``: NaNs are returned).  ``adjoint`` is accepted and
ignored: forward solves need no adjoint.

``train`` / ``residuals`` / ``mse`` / ``regularization`` (pde_model.py:138-460) fit closure coefficients -- and
``kappa`` of the periodic classes, given as a ``TrainableScalar`` -- to trajectories: the derivative of the solve comes from forward-mode tangents advanced on the GPU next to the
trajectories (``pde_opt_amd.fit``; csrc/sens.hip) -- periodic Cahn-Hilliard in 2-D or 3-D (``mu`` / ``D``; IMEX or
Euler), periodic 2-D Allen-Cahn (``mu`` / ``R``; Euler or RK4) and the Butler-Volmer Allen-Cahn classes (``mu`` / ``j0``;
Euler or RK4; ``voltage_sensitivities`` and ``train(..., voltage_weight=...)`` add the voltage of a constant-current run), with
FD derivatives.
A ``torch.nn.Module`` as ``mu`` of CahnHilliard2DPeriodic (the reference's periodic CNN, optimization_neural_network.ipynb)
takes the field path of ``pde_opt_amd.fieldmu``: ``solve`` / ``residuals`` / ``mse`` run it forward, ``mse_backward``
fills the parameters' ``.grad`` by a discrete adjoint on the GPU, ``train(method="mse")`` drives BFGS with it.
``optimize`` (pde_model.py:462-551) minimises a scalar objective of the saved solution over the same coefficients with
BFGS: the objective is a torch-differentiable callable or an object with ``value_and_grad(ys)``; its cotangent
``dJ/dys`` is contracted with the same tangents on the GPU (``pdeopt_sens_contract``).  Objectives in neither form, and
the equations / solvers / closures ``train`` refuses, raise ``NotImplementedError``.
``GPE2DTSControl`` + ``StrangSplitting`` with ``GaussianSpots`` as ``lights``: ``control_gradient`` returns the
reverse-mode gradient of such an objective over the spots' numbers (a discrete adjoint of the Strang step on the GPU,
``pde_opt_amd.gpe_control``; csrc/gpe_adjoint.hip) and ``optimize(opt_parameters={"lights": spots})`` drives BFGS with it.
``GPE2DTSRot`` + ``RotatingStrangSplitting``: ``rotation_gradient`` returns the reverse-mode gradient over ``k``, ``e``,
``omega`` and the start state (a discrete adjoint of the alternating-direction split step, csrc/gpe_rot_adjoint.hip) and
``optimize_rotation`` drives BFGS with it; ``control_gradient``, ``optimize`` and ``train`` refuse that pair.
With ``lights`` or ``omega_rate`` (a stirred or ramped problem) ``stirring_gradient`` adds the gradient over ``omega_rate``
and the spots' numbers (csrc/gpe_rot_adjoint.hip) and ``optimize_stirring`` drives BFGS with it.
"""

from __future__ import annotations

import math
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
        parameters = fit.plain(parameters)  # a TrainableScalar (train's kappa) is its number to the equation
        equation = self.equation_type(domain=self.domain, **parameters)
        solver = self.solver_type(**prepare_solver_params(self.solver_type, solver_parameters or {}, equation))
        check_solve = getattr(solver, "check_solve", None)
        if check_solve is not None:  # (ImplicitEuler: refuses what it does not cover before any engine exists)
            check_solve(equation, stepsize_controller, self._engine)
        if getattr(equation, "_mu_module", None) is not None:  # a network as mu: torch evaluates it, the kernels take the field
            return self._fieldmu_solve(equation, solver, y0, ts, dt0, stepsize_controller)
        ts = np.asarray(ts, dtype=np.float64)
        if getattr(equation, "_rotating_frame", False):
            equation._lights_kind(float(ts[0]), float(ts[-1]))  # refuses a host-sampled lights before an engine exists
        if self._engine is None:
            self._engine = HipEngine(self.device)
        sol = diffeqsolve(
            equation, solver, t0=ts[0], t1=ts[-1], dt0=dt0, y0=y0, saveat=SaveAt(ts=ts),
            stepsize_controller=stepsize_controller or ConstantStepSize(), max_steps=max_steps,
            throw=False, engine=self._engine,
        )
        return sol.ys

    # -- observables of the GPE and the ground-state solve (pde_opt_amd.gpe_observables) ---------------------------------
    def observables(self, parameters, state, t=0.0):
        """Norm, energy terms, angular momentum, second moments, ``energy`` and ``mu`` of a GPE state (``GpeObservables``,
        every entry ``(B,)``), summed on the GPU: ``state`` is one ``(nx, ny, 2)`` field or a batch, ``parameters`` one
        dict shared by the batch or a sequence with one dict per state; the potential is taken at local time ``t`` as a
        substep starting there would.  ``GPE2DTSControl`` and ``GPE2DTSRot`` only.  After a ``solve``,
        ``model._engine.gpe_observables()`` reads the resident final state without an upload."""
        from . import gpe_observables

        return gpe_observables.observables(self, parameters, state, t)

    def ground_state(self, parameters, y0, dt, tol=1e-8, max_steps=100_000, check_every=25, solver_parameters=None):
        """Relax ``y0`` (one state or a batch; ``parameters`` as in ``observables``) in imaginary time
        (``time_scale=-1j``; any other ``solver_parameters["time_scale"]`` raises ``ValueError``) until the energy per
        particle stands still: blocks of ``check_every`` steps of ``dt``, one ``advance`` and one ``gpe_observables``
        call each (64 bytes per environment come back); environment b is converged when
        ``|energy_now - energy_prev| / (check_every dt) <= tol``.  The loop ends when every environment is, or at
        ``max_steps`` with ``converged=False`` where it is not.  Returns ``GroundState(state, observables, steps,
        converged, history)``.  A ``lights`` that depends on time is frozen at ``t = 0``, for the steps and for the energy
        alike: a ground state belongs to one potential.  ``GPE2DTSRot`` takes static spots (a pinning beam) and refuses
        moving spots and a nonzero ``omega_rate``.  The split step renormalises BETWEEN its half steps, so the returned state has
        ``norm = 1 + O(dt)``; ``energy`` and ``mu`` are already divided by it."""
        from . import gpe_observables

        return gpe_observables.ground_state(self, parameters, y0, dt, tol, max_steps, check_every, solver_parameters)

    # -- free energy of the phase-field classes (pde_opt_amd.phase_field_observables) ------------------------------------
    def free_energy(self, parameters, state):
        """Mass, bulk and gradient free energy, moments of the chemical potential, dissipation and a non-finite count of a
        phase-field state (``PhaseFieldObservables``, every entry ``(B,)``), summed on the GPU and consistent with the
        finite-difference right-hand side: ``d free_energy / dt = -dissipation`` along ``u_t = rhs_fd(u)``.  ``state`` is
        one field or a batch, ``parameters`` one dict shared by the batch or a sequence with one dict per state (same
        closure structure).  ``CahnHilliard2DPeriodic``, ``AllenCahn2DPeriodic`` and ``CahnHilliard3DPeriodic`` with
        ``derivs="fd"`` and a ``mu`` that has a closed antiderivative; everything else is refused with the reason
        (``observables`` and ``ground_state`` stay the GPE's).  After a ``solve``, ``model._engine.pf_observables()`` reads
        the resident final state without an upload."""
        from . import phase_field_observables

        return phase_field_observables.free_energy(self, parameters, state)

    def free_energy_trace(self, parameters, y0, ts, solver_parameters=None, dt0=0.000001):
        """The same quantities along a solve, entries of shape ``(len(ts), B)``: the constant-step solve of ``solve``
        (Euler, RK4 or SemiImplicitFourierSpectral) with 64 bytes per environment read back at each save point instead of
        the field.  Every ``ts`` must lie on a step edge (``ts[0] + k dt0``, or ``ts[-1]``): a save point inside a step is
        refused, because the energy of a linear interpolation of states is not an interpolation of energies."""
        from . import phase_field_observables

        return phase_field_observables.free_energy_trace(self, parameters, y0, ts, solver_parameters, dt0)

    # -- structure factor of the phase-field classes (pde_opt_amd.structure_factor) ------------------------------------------
    def structure_factor(self, state):
        """The shell-averaged structure factor ``S(k)`` of a real periodic field (``StructureFactor``: ``k``, ``counts``,
        ``power``, ``s`` and the scalars ``variance``, ``k1``, ``k2``, ``length = 2 pi / k1``, leading shape ``(B,)``),
        transformed and binned on the GPU: ``n_bins * 8`` bytes per environment come back instead of the field.  ``state``
        is one field or a batch; there are no parameters, S(k) depends on the state and the domain only.
        ``CahnHilliard2DPeriodic``, ``AllenCahn2DPeriodic`` and ``CahnHilliard3DPeriodic``; everything else raises
        ``NotImplementedError``."""
        from . import structure_factor

        return structure_factor.structure_factor(self, state)

    def structure_factor_trace(self, parameters, y0, ts, solver_parameters=None, dt0=0.000001):
        """The same along a solve, leading shape ``(len(ts), B)``: the constant-step solve of ``solve`` (Euler, RK4 or
        SemiImplicitFourierSpectral) with ``n_bins * 8`` bytes per environment read back at each save point instead of the
        field -- ``length`` over ``ts`` is the coarsening curve.  Every ``ts`` must lie on a step edge (``ts[0] + k dt0``,
        or ``ts[-1]``), as for ``free_energy_trace``."""
        from . import structure_factor

        return structure_factor.structure_factor_trace(self, parameters, y0, ts, solver_parameters, dt0)

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

    # -- a torch.nn.Module as mu (pde_opt_amd.fieldmu) -----------------------------------------------------------------
    def fieldmu_solver(self):
        """the solver of the module path (its ``chunk_bytes`` caps the states the backward sweep holds; its
        ``native_cnn = True`` evaluates and differentiates a ``PeriodicCNN`` in the library's own kernels, csrc/cnn.hip)"""
        if getattr(self, "_fieldmu", None) is None:
            from .fieldmu import FieldMuSolver

            self._fieldmu = FieldMuSolver(self.device)
        return self._fieldmu

    def _fieldmu_solve(self, equation, solver, y0, ts, dt0, stepsize_controller):
        y0 = np.asarray(y0)
        if y0.dtype not in (np.float32, np.float64):
            y0 = y0.astype(np.float64)
        single = y0.ndim == 2
        yb = y0[None] if single else y0
        if yb.ndim != 3 or tuple(yb.shape[1:]) != tuple(self.domain.points):
            raise ValueError(f"y0 shape {y0.shape} does not match domain points {self.domain.points}")
        ys = self.fieldmu_solver().solve(equation, solver, yb, np.asarray(ts, dtype=np.float64), float(dt0), stepsize_controller)
        return ys[:, 0] if single else ys

    def mse_backward(self, parameters, y0s__values, solver_parameters, ts, weights, lambda_reg, dt0=0.000001,
                     closure_grads=None) -> float:
        """``mse(...)`` for a ``torch.nn.Module`` as ``parameters["mu"]``, and its gradient: ``.grad`` of the module's
        parameters is set to the gradient of ``mean(r^2) + reg`` (a discrete adjoint of the solve on the GPU, see
        ``pde_opt_amd.fieldmu``; the loss is summed in fp64).  The entry for ``torch.optim`` users:

            opt.zero_grad(); loss = model.mse_backward(params, (y0s, values), sp, ts, weights, lam); opt.step()

        ``weights["mu"]``: None, a number, a flat array or a module of the same structure (the weights of
        ``lambda sum w p^2``).  Returns the loss as a float.

        ``closure_grads``: a dict asks for the joint gradient.  ``parameters["D"]`` must then be a
        ``DiffusionLegendrePolynomials``; on return ``closure_grads["D"]`` is the gradient of ``mean(r^2) + reg`` over its
        coefficients (fp64, in the order of ``D.expansion.params``), from the same backward sweep.  ``weights["D"]`` has
        the meaning ``fit.weight_vector`` gives a closure's weights; its share ``lambda sum w p^2`` is in the loss and
        ``2 lambda w p`` in the gradient.  ``.grad`` of the module is the same, bit for bit, with and without."""
        from . import fieldmu
        from .numerics.solvers import reject_implicit_gradients

        reject_implicit_gradients(self.solver_type, "mse_backward")
        module = parameters.get("mu")
        if not fieldmu.is_module(module):
            raise NotImplementedError("mse_backward differentiates a solve whose mu is a torch.nn.Module (" + fieldmu.FIELD_MU_SUPPORT
                                      + "); closure coefficients are fitted by train / optimize")
        equation = self.equation_type(domain=self.domain, **parameters)
        solver = self.solver_type(**prepare_solver_params(self.solver_type, solver_parameters or {}, equation))
        y0s, values = y0s__values
        y0s = np.asarray(y0s)
        if y0s.dtype not in (np.float32, np.float64):
            y0s = y0s.astype(np.float64)
        for q in module.parameters():
            q.grad = None
        loss = self.fieldmu_solver().mse_backward(equation, solver, y0s, np.asarray(values), np.asarray(ts, dtype=np.float64), float(dt0),
                                                  coef_grad=closure_grads is not None)
        if closure_grads is not None:
            loss, grad_D = loss
        w = fieldmu.weight_vector(module, (weights or {}).get("mu"))
        if lambda_reg and np.any(w != 0.0):
            p = fieldmu.flatten_params(module)
            loss += float(lambda_reg * np.sum(w * p * p))
            fieldmu.add_flat_grad(module, 2.0 * float(lambda_reg) * w * p)
        if closure_grads is not None:
            w_D = fit.weight_vector(fit.ParamMap.of({"D": parameters["D"]}, self.equation_type), _array_weights(weights))
            p_D = np.asarray(parameters["D"].expansion.params, dtype=np.float64)
            if lambda_reg and np.any(w_D != 0.0):
                loss += float(lambda_reg * np.sum(w_D * p_D * p_D))
                grad_D = grad_D + 2.0 * float(lambda_reg) * w_D * p_D
            closure_grads["D"] = grad_D
        return loss

    def _train_module(self, data, inds, opt_parameters, other_parameters, solver_parameters, weights, lambda_reg, method,
                      max_steps):
        """``train`` for a ``torch.nn.Module`` as ``opt_parameters["mu"]``: BFGS over its flattened parameters, followed by
        the coefficients of ``opt_parameters["D"]`` (a ``DiffusionLegendrePolynomials``) when that is given too"""
        from . import fieldmu
        from .numerics.functions.legendre import DiffusionLegendrePolynomials

        if method == "least_squares":
            raise NotImplementedError("a torch.nn.Module as mu is trained with method='mse' (reverse mode gives the gradient of "
                                      "the loss, not the Jacobian Levenberg-Marquardt needs)")
        joint = "D" in opt_parameters
        if not set(opt_parameters) <= {"mu", "D"} or (joint and not isinstance(opt_parameters["D"], DiffusionLegendrePolynomials)):
            raise ValueError("with a torch.nn.Module as mu, opt_parameters holds mu alone, or mu and D as a "
                             "DiffusionLegendrePolynomials: " + fieldmu.FIELD_MU_SUPPORT)
        module = opt_parameters["mu"]
        p0 = fieldmu.flatten_params(module)
        n_mu = len(p0)
        if joint:
            p0 = np.concatenate([p0, np.asarray(opt_parameters["D"].expansion.params, dtype=np.float64)])
        if len(p0) > fit.MAX_DENSE_BFGS_PARAMS:
            raise ValueError(f"mu{' and D have' if joint else ' has'} {len(p0)} parameters: train's BFGS keeps a dense inverse Hessian and takes at most "
                             f"{fit.MAX_DENSE_BFGS_PARAMS}; use PDEModel.mse_backward with a torch.optim optimiser")
        y0s, values, ts = stack_training_data(data, inds)
        weights = _array_weights(weights)  # mse and mse_backward must see the same regularisation

        def params_of(p):
            """the module updated in place, D rebuilt from the tail of the flat vector"""
            fieldmu.unflatten_params(module, p[:n_mu])
            fitted = {"mu": module}
            if joint:
                fitted["D"] = DiffusionLegendrePolynomials(np.array(p[n_mu:], dtype=np.float64))
            return {**fitted, **other_parameters}

        def value_and_grad(p):
            grads = {} if joint else None
            f = self.mse_backward(params_of(p), (y0s, values), solver_parameters, ts, weights, lambda_reg, closure_grads=grads)
            g = fieldmu.flatten_grads(module)
            return f, (np.concatenate([g, grads["D"]]) if joint else g)

        def value(p):
            return self.mse(params_of(p), (y0s, values), solver_parameters, ts, weights or {}, lambda_reg)

        p, hist = fit.minimize_bfgs(value_and_grad, value, p0, max_steps=max_steps)
        self.last_train_history = hist
        return params_of(p)

    def _sens_engine(self):
        if getattr(self, "_sens_eng", None) is None:
            self._sens_eng = HipEngine(self.device)
        return self._sens_eng

    def train(self, data, inds, opt_parameters, other_parameters, solver_parameters, weights, lambda_reg,
              method="least_squares", max_steps=100, voltage_weight=0.0):
        """Fit the closure coefficients in ``opt_parameters`` to ``data`` (pde_model.py:288-460).

        ``method="least_squares"``: Levenberg-Marquardt on the Gauss-Newton normal equations (the reference's
        optimistix.LevenbergMarquardt with ForwardMode); ``"mse"``: BFGS on ``mean(r^2) + reg``.  ``data["ys"][i]``
        is a state of shape ``spatial``: ``(nx, ny)`` for CahnHilliard2DPeriodic and AllenCahn2DPeriodic,
        ``(nx, ny, nz)`` for CahnHilliard3DPeriodic.  Returns ``{**fitted, **other_parameters}``; each fitted closure is the class it
        started as, with its ``prior_fn``.

        ``opt_parameters["kappa"] = TrainableScalar(value)`` (``numerics/functions/scalar.py``) fits the gradient-energy
        coefficient of the three periodic classes too, alone or next to closures; the optimiser moves ``log(kappa)`` and the
        returned dict holds a ``TrainableScalar``, which ``solve`` / ``residuals`` / ``mse`` take as it is.  A plain float
        among ``opt_parameters`` is refused.

        The Butler-Volmer Allen-Cahn classes train ``"mu"`` and ``"j0"`` (Legendre closures; Euler or RK4); their scalars
        ``alpha``, ``kappa``, ``Crate`` / ``v`` are not trainable and go in ``other_parameters``.  With ``data["vs"]`` -- the cell
        voltages aligned with ``data["ys"]`` -- and ``voltage_weight > 0`` a constant-current class fits the voltage curve
        too: the loss is ``mean(r_field^2) + voltage_weight mean(r_V^2) + reg`` with ``r_V`` at the same save points as the
        frames (``inds[b][1:]``), which must then fall on multiples of the step ``dt0 = 1e-6``.  Without ``"vs"`` or with
        weight 0 nothing changes; ``"vs"`` with a weight on a given-voltage class raises ``ValueError``.

        ``opt_parameters = {"mu": torch.nn.Module}`` (CahnHilliard2DPeriodic, ``method="mse"``): BFGS over the module's
        flattened parameters with the reverse-mode gradient of ``mse_backward``, for up to ``fit.MAX_DENSE_BFGS_PARAMS``
        parameters; the returned dict holds the trained module (the one passed in, updated in place).  With ``"D":
        DiffusionLegendrePolynomials`` next to it the mobility is trained too: the flat vector is the module's parameters
        followed by ``D``'s coefficients (the cap applies to the total), the gradient over both comes from one backward
        sweep (``mse_backward(..., closure_grads={})``), and the returned ``"D"`` is a new ``DiffusionLegendrePolynomials``.
        ``kappa`` stays in ``other_parameters``."""
        _reject_rotating(self)
        fit.reject_unsupported(self)
        if method not in ("least_squares", "mse"):
            raise ValueError(f"method must be 'least_squares' or 'mse', got {method!r}")
        if fit.is_torch_module(opt_parameters.get("mu")) and len(self.domain.points) == 2 and not fit._is_allen_cahn(self.equation_type):
            return self._train_module(data, inds, opt_parameters, other_parameters, solver_parameters, weights, lambda_reg,
                                      method, max_steps)
        pmap = fit.ParamMap.of(opt_parameters, self.equation_type)
        y0s, values, ts = stack_training_data(data, inds)
        v_obs = None  # (T - 1, B) observed voltages
        if voltage_weight and data.get("vs") is not None:
            if not fit._is_butler_volmer(self.equation_type, constant_current_only=True):
                raise ValueError(f"data['vs'] with voltage_weight = {voltage_weight!r}: {self.equation_type.__name__} does not solve "
                                 "for a voltage (only the constant-current Butler-Volmer classes do)")
            vs = data["vs"]
            v_obs = np.array([[float(vs[ind[i]]) for ind in inds] for i in range(1, len(inds[0]))], dtype=np.float64)
            w_v = float(voltage_weight) * values.size / v_obs.size  # mean(r_V^2) weighed against mean(r_field^2) = ssr / M
        equation0 = self.equation_type(domain=self.domain, **fit.plain({**opt_parameters, **other_parameters}))
        fit.check_equation(equation0)
        frames = np.ascontiguousarray(np.swapaxes(values, 0, 1))  # (T - 1, B, *spatial)
        frames_key = object()
        sens_params = pmap.sens_params()
        P = len(sens_params)
        eng = self._sens_engine()

        def setup(p):
            params = fit.plain({**pmap.build(p), **other_parameters})
            equation = self.equation_type(domain=self.domain, **params)
            solver = self.solver_type(**prepare_solver_params(self.solver_type, solver_parameters or {}, equation))
            return params, equation, solver

        def sums(p):
            if not pmap.feasible(p):  # kappa <= 0 under positive=False: a rejected step, never a solve
                return math.inf, np.zeros(pmap.size), np.zeros((pmap.size, pmap.size))
            _, equation, solver = setup(p)
            volt = [] if v_obs is not None else None
            s, _ = fit.sensitivity_solve(eng, equation, solver, y0s, ts, sens_params, frames=frames,
                                         frames_key=frames_key, voltages=volt)
            ssr, rdp, G = fit.unpack_sums(s, P)
            if volt is not None:
                vd = np.stack(volt[1:])  # (T - 1, B, 1 + P)
                ssr, rdp, G = fit.add_voltage_sums(ssr, rdp, G, v_obs - vd[..., 0], vd[..., 1:], w_v)
            return (ssr,) + pmap.scale_sums(p, *pmap.expand(rdp, G))

        def ssr(p):
            if not pmap.feasible(p):
                return math.inf
            params, equation, _ = setup(p)
            if v_obs is None:
                r, _ = self.residuals(params, (y0s, values), solver_parameters, ts, {}, 0.0)
                return float(np.sum(np.asarray(r, dtype=np.float64) ** 2))
            pred = self.solve(params, y0s, ts, solver_parameters)  # (T, B, nx, ny)
            r = values - np.swapaxes(pred, 0, 1)[:, 1:]
            r_v = v_obs - np.asarray(equation.get_voltage(pred[1:].reshape((-1,) + pred.shape[2:]))).reshape(v_obs.shape)
            return float(np.sum(np.asarray(r, dtype=np.float64) ** 2)) + w_v * float(np.sum(r_v ** 2))

        obj = fit.Objective(sums=sums, ssr=ssr, M=int(values.size), lambda_reg=float(lambda_reg),
                            w=fit.weight_vector(pmap, weights or {}))
        p0 = pmap.flatten(opt_parameters)
        if method == "least_squares":
            p, hist = fit.levenberg_marquardt(obj, p0, max_steps=max_steps)
        else:
            p, hist = fit.bfgs(obj, p0, max_steps=max_steps)
        self.last_train_history = hist
        return {**pmap.build(p), **other_parameters}

    def voltage_sensitivities(self, opt_parameters, other_parameters, y0s, ts, solver_parameters=None, dt0=0.000001):
        """``(V (T, B), dV (T, B, P_all))``: the voltage of the constant-current constraint at every ``ts[q]`` (``ts[0]``, the
        start, included) of the B trajectories from ``y0s`` ``(B, nx, ny)``, and its derivative with respect to every entry
        of ``opt_parameters`` (``"mu"`` / ``"j0"`` Legendre closures, in ``fit.ParamMap`` order), from the forward-mode
        tangents advanced on the GPU (``pdeopt_sens_bv_voltage``).  The constant-current Butler-Volmer classes only; the
        scalars (``alpha``, ``kappa``, ``Crate``) go in ``other_parameters``.  Every ``ts[q]`` must fall on a step edge
        (``ts[0] + k dt0``, or ``ts[-1]``), otherwise ``ValueError``: the voltage of a linearly interpolated state is not the
        interpolated voltage."""
        _reject_rotating(self)
        fit.reject_unsupported(self)
        if not fit._is_butler_volmer(self.equation_type, constant_current_only=True):
            raise NotImplementedError(f"voltage_sensitivities differentiates the constant-current constraint: "
                                      f"{self.equation_type.__name__} does not solve for a voltage")
        other_parameters = other_parameters or {}
        pmap = fit.ParamMap.of(opt_parameters, self.equation_type)
        equation = self.equation_type(domain=self.domain, **{**opt_parameters, **other_parameters})
        fit.check_equation(equation)
        solver = self.solver_type(**prepare_solver_params(self.solver_type, solver_parameters or {}, equation))
        y0s = np.asarray(y0s)
        if y0s.ndim != 3 or tuple(y0s.shape[1:]) != tuple(self.domain.points):
            raise ValueError(f"y0s of shape {y0s.shape}: expected (B,) + {tuple(self.domain.points)}")
        volt = []
        fit.sensitivity_solve(self._sens_engine(), equation, solver, y0s, ts, pmap.sens_params(), dt0=dt0, voltages=volt)
        vd = np.stack(volt)  # (T, B, 1 + n active)
        dV = np.zeros(vd.shape[:2] + (pmap.size,))
        dV[..., np.nonzero(pmap.active())[0]] = vd[..., 1:]
        return vd[..., 0].copy(), dV

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
        _reject_rotating(self)
        if _is_gpe(self.equation_type):
            return self._optimize_gpe(objective_function, y0, ts, opt_parameters, other_parameters, solver_parameters, weights,
                                      lambda_reg, max_steps)
        value_and_grad, value, pmap = self._objective_functions(objective_function, y0, ts, opt_parameters, other_parameters,
                                                                solver_parameters, weights, lambda_reg)
        p, hist = fit.minimize_bfgs(value_and_grad, value, pmap.flatten(opt_parameters), max_steps=max_steps)
        self.last_optimize_history = hist
        return {**pmap.build(p), **(other_parameters or {})}

    # -- gradient-based control of the GPE (pde_opt_amd.gpe_control) ---------------------------------------------------
    def gpe_control_solver(self):
        """the solver of the GPE's backward sweeps (its ``chunk_bytes`` caps the states a sweep holds)"""
        if getattr(self, "_gpe_control", None) is None:
            from .gpe_control import GpeControlSolver

            self._gpe_control = GpeControlSolver(self.device)
        return self._gpe_control

    def control_gradient(self, objective_function, y0, ts, parameters, solver_parameters=None, dt0=0.000001,
                         per_environment=False):
        """``(J, grad, lam0)`` of ``J = objective_function(solve(parameters, y0, ts, ...))`` for ``GPE2DTSControl`` +
        ``StrangSplitting`` whose ``parameters["lights"]`` is a ``GaussianSpots``: ``grad`` ``(S, 7)`` is ``dJ/d`` (amp0,
        amp_rate, x0, x_rate, y0, y_rate, width) of every spot in user units (``(B, S, 7)``, one block per state of a
        batch, with ``per_environment=True``; summed in order otherwise), ``lam0 = dJ/dy0`` in the shape of ``y0``
        (``(N, M, 2)`` or ``(B, N, M, 2)``).  The objective takes the forms of ``optimize``; ``ys`` is the array ``solve``
        returns, bit for bit.  A discrete adjoint of the solve on the GPU (``pde_opt_amd.gpe_control``): the entry for
        users with their own optimiser, as ``mse_backward`` is for ``torch.optim``."""
        from . import gpe_control

        gpe_control.reject_unsupported(self.equation_type, self.solver_type, parameters)
        J, (raw,), lam0 = self._reverse_gradient(self.gpe_control_solver, objective_function, y0, ts, parameters,
                                                 solver_parameters, dt0)
        grad = gpe_control.SpotMap.user_gradient(parameters["lights"], raw)
        return J, (grad if per_environment else fit.summed_in_order(grad)), lam0

    def _reverse_gradient(self, get_solver, objective_function, y0, ts, parameters, solver_parameters, dt0, check_equation=None):
        """What ``control_gradient``, ``rotation_gradient`` and ``stirring_gradient`` share: the solve, the objective and
        its cotangent, and the backward sweep of ``get_solver()`` (built when the sweep is reached).  Returns ``(J, blocks,
        lam0)``: ``blocks`` is what that solver's ``gradient`` returns before ``lam0``, per environment, and ``lam0`` has
        the shape of ``y0``.  ``check_equation(equation, ts)`` may refuse the equation once it is built."""
        y0 = np.asarray(y0)
        if y0.dtype not in (np.float32, np.float64):
            y0 = y0.astype(np.float64)
        ts = np.asarray(ts, dtype=np.float64)
        objective = fit.as_objective(objective_function, np.broadcast_to(y0.astype(np.float64), (len(ts),) + y0.shape))
        if y0.ndim not in (3, 4) or tuple(y0.shape[-3:]) != tuple(self.domain.points) + (2,):
            raise ValueError(f"y0 of shape {y0.shape}: expected {tuple(self.domain.points) + (2,)} or (B,) + that")
        equation = self.equation_type(domain=self.domain, **parameters)
        if check_equation is not None:
            check_equation(equation, ts)
        solver = self.solver_type(**prepare_solver_params(self.solver_type, solver_parameters or {}, equation))
        ys = self.solve(parameters, y0, ts, solver_parameters, dt0=dt0)
        J, g = objective.value_and_grad(ys)
        single = y0.ndim == 3
        cot = g[:, None] if single else g
        *blocks, lam0 = get_solver().gradient(equation, solver, y0[None] if single else y0, ts, float(dt0), cot)
        return J, blocks, (lam0[0] if single else lam0)

    def _penalised_bfgs(self, p0, w, lambda_reg, params_of, value_of, value_and_grad_of, max_steps, active=None):
        """BFGS (``fit.minimize_bfgs``) on ``J(p) + lambda_reg sum(w p^2)`` from ``p0``; the flat vector it ends at.
        ``value_of(params_of(p))`` is ``J`` from a forward solve (the trial points of the line search),
        ``value_and_grad_of(params_of(p))`` is ``(J, flat dJ/dp)``; entries outside ``active`` keep a zero gradient.  The
        objective after every accepted step goes to ``last_optimize_history``."""
        lam = float(lambda_reg)
        penalty = lambda p: lam * float(np.sum(w * p * p))

        def value(p):
            return value_of(params_of(p)) + penalty(p)

        def value_and_grad(p):
            J, g = value_and_grad_of(params_of(p))
            g = g + 2.0 * lam * w * p
            return J + penalty(p), (g if active is None else g * active)

        p, hist = fit.minimize_bfgs(value_and_grad, value, p0, max_steps=max_steps)
        self.last_optimize_history = hist
        return p

    def _optimize_gpe(self, objective_function, y0, ts, opt_parameters, other_parameters, solver_parameters, weights,
                      lambda_reg, max_steps):
        """``optimize`` over the numbers of ``opt_parameters["lights"]`` (a ``GaussianSpots``; its ``free`` names the
        numbers that move) with the reverse-mode gradient of ``control_gradient``; ``weights["lights"]``: a number or
        an ``(S, 7)`` array of the weights of ``lambda sum w p^2``"""
        from . import gpe_control

        other_parameters, weights = other_parameters or {}, weights or {}
        probe = None
        if y0 is not None and ts is not None:
            y0 = np.asarray(y0)
            probe = np.broadcast_to(y0.astype(np.float64), (len(ts),) + y0.shape)
        objective = fit.as_objective(objective_function, probe)
        if y0 is None or ts is None or not opt_parameters:
            raise ValueError("optimize needs y0, ts and opt_parameters")
        gpe_control.reject_unsupported(self.equation_type, self.solver_type, {**other_parameters, **opt_parameters},
                                       opt_names=opt_parameters)
        smap = gpe_control.SpotMap.of(opt_parameters["lights"])
        w = smap.weight_vector(weights.get("lights"))

        def value_and_grad(params):
            J, grad, _ = self.control_gradient(objective, y0, ts, params, solver_parameters)
            return J, grad.reshape(-1)

        p = self._penalised_bfgs(smap.flatten(opt_parameters["lights"]), w, lambda_reg,
                                 lambda p: {**other_parameters, "lights": smap.build(p)},
                                 lambda params: objective.value(self.solve(params, y0, ts, solver_parameters)),
                                 value_and_grad, max_steps, active=smap.active().reshape(-1))
        return {"lights": smap.build(p), **other_parameters}

    # -- gradients of the rotating-frame GPE (pde_opt_amd.gpe_control.RotControlSolver) -------------------------------
    def rot_control_solver(self):
        """the solver of the rotating-frame GPE's backward sweeps (its ``chunk_bytes`` caps the states a sweep holds)"""
        if getattr(self, "_rot_control", None) is None:
            from .gpe_control import RotControlSolver

            self._rot_control = RotControlSolver(self.device)
        return self._rot_control

    def rotation_gradient(self, objective_function, y0, ts, parameters, solver_parameters=None, dt0=0.000001,
                          per_environment=False, stepsize_controller=None):
        """``(J, {"k": ..., "e": ..., "omega": ...}, lam0)`` of ``J = objective_function(solve(parameters, y0, ts, ...))``
        for ``GPE2DTSRot`` + ``RotatingStrangSplitting``: the derivatives of ``J`` with respect to the interaction
        strength, the trap anisotropy and the rotation frequency (scalars; ``(B,)`` arrays, one entry per state of a
        batch, with ``per_environment=True``; summed in order otherwise) and ``lam0 = dJ/dy0`` in the shape of ``y0``
        (``(N, M, 2)`` or ``(B, N, M, 2)``).  The objective takes the forms of ``optimize``; ``ys`` is the array ``solve``
        returns, bit for bit.  A discrete adjoint of the solve on the GPU (csrc/gpe_rot_adjoint.hip), constant steps only.

        Because ``lam0`` comes back, segments with different ``omega`` chain: solve the segments forward, then call this
        on the last one with the real objective and on each earlier one with the linear objective ``<lam0 of the next
        segment, ys[-1]>`` -- the gradient of a piecewise-constant rotation schedule."""
        from . import gpe_control

        gpe_control.reject_unsupported_rotation(self.equation_type, self.solver_type, stepsize_controller=stepsize_controller,
                                                parameters=parameters)
        J, (grad,), lam0 = self._reverse_gradient(self.rot_control_solver, objective_function, y0, ts, parameters,
                                                  solver_parameters, dt0)
        return J, _named_gradient(grad, gpe_control.ROT_NAMES, per_environment), lam0

    def optimize_rotation(self, objective_function, y0, ts, opt_parameters, other_parameters, solver_parameters=None,
                          weights=None, lambda_reg=0.0, max_steps=100, dt0=0.000001, stepsize_controller=None):
        """Minimise ``objective_function(solve(...)) + lambda_reg sum_n weights[n] p_n^2`` over the numbers in
        ``opt_parameters``, any non-empty subset of ``{"k", "e", "omega"}`` of ``GPE2DTSRot`` (the rest fixed in
        ``other_parameters``), with BFGS (``fit.minimize_bfgs``) on the gradient of ``rotation_gradient``; trial points
        of the line search are forward solves.  Returns ``{**fitted, **other_parameters}``; the objective after every
        accepted step is in ``last_optimize_history``."""
        from . import gpe_control

        other_parameters, weights = other_parameters or {}, weights or {}
        gpe_control.reject_unsupported_rotation(self.equation_type, self.solver_type, opt_names=opt_parameters or {},
                                                stepsize_controller=stepsize_controller, parameters=other_parameters)
        if y0 is None or ts is None:
            raise ValueError("optimize_rotation needs y0 and ts")
        y0 = np.asarray(y0)
        objective = fit.as_objective(objective_function, np.broadcast_to(y0.astype(np.float64), (len(ts),) + y0.shape))
        names = [n for n in gpe_control.ROT_NAMES if n in opt_parameters]

        def params_of(p):
            return {**other_parameters, **{n: float(v) for n, v in zip(names, p)}}

        def value_and_grad(params):
            J, grad, _ = self.rotation_gradient(objective, y0, ts, params, solver_parameters, dt0=dt0)
            return J, np.array([grad[n] for n in names])

        p = self._penalised_bfgs(np.array([float(opt_parameters[n]) for n in names], dtype=np.float64),
                                 np.array([float(weights.get(n, 0.0)) for n in names]), lambda_reg, params_of,
                                 lambda params: objective.value(self.solve(params, y0, ts, solver_parameters, dt0=dt0)),
                                 value_and_grad, max_steps)
        return params_of(p)

    # -- gradients of the stirred, ramped rotating-frame GPE (pde_opt_amd.gpe_control.RotStirControlSolver) ------------
    def rot_stir_control_solver(self):
        """the solver of the stirred rotating-frame GPE's backward sweeps (its ``chunk_bytes`` caps the states a sweep
        holds)"""
        if getattr(self, "_rot_stir_control", None) is None:
            from .gpe_control import RotStirControlSolver

            self._rot_stir_control = RotStirControlSolver(self.device)
        return self._rot_stir_control

    def stirring_gradient(self, objective_function, y0, ts, parameters, solver_parameters=None, dt0=0.000001,
                          per_environment=False, stepsize_controller=None):
        """``(J, grad, lam0)`` of ``J = objective_function(solve(parameters, y0, ts, ...))`` for ``GPE2DTSRot`` +
        ``RotatingStrangSplitting`` with or without ``lights`` and ``omega_rate``: ``grad`` is a dict with ``"k"``, ``"e"``,
        ``"omega"``, ``"omega_rate"`` (floats; ``(B,)`` arrays, one entry per state of a batch, with
        ``per_environment=True``; summed in order otherwise) and, when ``parameters["lights"]`` is a ``GaussianSpots``,
        ``"lights"``: ``(S, 7)`` (``(B, S, 7)`` per environment), ``dJ/d`` (amp0, amp_rate, x0, x_rate, y0, y_rate, width)
        of every spot in user units.  A callable ``lights`` that does not depend on time is folded into the potential as
        the forward solve does and gets no entry; one that does is refused.  ``lam0 = dJ/dy0`` in the shape of ``y0``: it
        chains segments as in ``rotation_gradient``.  The objective takes the forms of ``optimize``; ``ys`` is the array
        ``solve`` returns, bit for bit.  A discrete adjoint of the solve on the GPU (csrc/gpe_rot_adjoint.hip),
        constant steps only."""
        from . import gpe_control
        from .numerics.functions.lights import GaussianSpots

        gpe_control.reject_unsupported_stirring(self.equation_type, self.solver_type, stepsize_controller=stepsize_controller,
                                                parameters=parameters)
        J, (grad, spot_grad), lam0 = self._reverse_gradient(
            self.rot_stir_control_solver, objective_function, y0, ts, parameters, solver_parameters, dt0,
            check_equation=lambda equation, ts: gpe_control.reject_time_dependent_lights(equation, ts[0], ts[-1]))
        out = _named_gradient(grad, gpe_control.STIR_NAMES, per_environment)
        if isinstance(parameters.get("lights"), GaussianSpots):
            user = gpe_control.SpotMap.user_gradient(parameters["lights"], spot_grad)
            out["lights"] = user if per_environment else fit.summed_in_order(user)
        return J, out, lam0

    def optimize_stirring(self, objective_function, y0, ts, opt_parameters, other_parameters, solver_parameters=None,
                          weights=None, lambda_reg=0.0, max_steps=100, dt0=0.000001, stepsize_controller=None):
        """Minimise ``objective_function(solve(...)) + lambda_reg sum w p^2`` over ``opt_parameters``, any non-empty
        subset of ``{"k", "e", "omega", "omega_rate", "lights"}`` of ``GPE2DTSRot`` (the rest fixed in
        ``other_parameters``), with BFGS (``fit.minimize_bfgs``) on the gradient of ``stirring_gradient``.  ``"lights"``
        must be a ``GaussianSpots``; its ``free`` names the numbers that move.  The flat vector is the scalars in that
        order, then ``SpotMap.flatten``; ``weights[name]`` is a number (``weights["lights"]``: a number or ``(S, 7)``).
        Trial points of the line search are forward solves.  Returns ``{**fitted, **other_parameters}``; the objective
        after every accepted step is in ``last_optimize_history``."""
        from . import gpe_control

        other_parameters, weights = other_parameters or {}, weights or {}
        gpe_control.reject_unsupported_stirring(self.equation_type, self.solver_type, opt_names=opt_parameters or {},
                                                stepsize_controller=stepsize_controller,
                                                parameters={**other_parameters, **(opt_parameters or {})},
                                                opt_parameters=opt_parameters or {})
        if y0 is None or ts is None:
            raise ValueError("optimize_stirring needs y0 and ts")
        y0 = np.asarray(y0)
        objective = fit.as_objective(objective_function, np.broadcast_to(y0.astype(np.float64), (len(ts),) + y0.shape))
        names = [n for n in gpe_control.STIR_NAMES if n in opt_parameters]
        smap = gpe_control.SpotMap.of(opt_parameters["lights"]) if "lights" in opt_parameters else None
        ns = len(names)
        w = np.array([float(weights.get(n, 0.0)) for n in names])
        active = np.ones(ns, dtype=bool)
        p0 = np.array([float(opt_parameters[n]) for n in names], dtype=np.float64)
        if smap is not None:
            w = np.concatenate([w, smap.weight_vector(weights.get("lights"))])
            active = np.concatenate([active, smap.active().reshape(-1)])
            p0 = np.concatenate([p0, smap.flatten(opt_parameters["lights"])])

        def params_of(p):
            out = {**other_parameters, **{n: float(v) for n, v in zip(names, p[:ns])}}
            if smap is not None:
                out["lights"] = smap.build(p[ns:])
            return out

        def value_and_grad(params):
            J, grad, _ = self.stirring_gradient(objective, y0, ts, params, solver_parameters, dt0=dt0)
            g = np.array([grad[n] for n in names], dtype=np.float64)
            if smap is not None:
                g = np.concatenate([g, np.asarray(grad["lights"]).reshape(-1)])
            return J, g

        p = self._penalised_bfgs(p0, w, lambda_reg, params_of,
                                 lambda params: objective.value(self.solve(params, y0, ts, solver_parameters, dt0=dt0)),
                                 value_and_grad, max_steps, active=active)
        return params_of(p)

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
        fit.check_equation(self.equation_type(domain=self.domain, **fit.plain({**opt_parameters, **other_parameters})))
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
            if not pmap.feasible(p):  # kappa <= 0 under positive=False: a failed line-search point, never a solve
                return math.inf
            return objective.value(self.solve(params_of(p), y0, ts, solver_parameters)) + reg.reg(p)

        def value_and_grad(p):
            if not pmap.feasible(p):
                return math.inf, np.full(pmap.size, np.nan)
            params = fit.plain(params_of(p))
            equation = self.equation_type(domain=self.domain, **params)
            solver = self.solver_type(**prepare_solver_params(self.solver_type, solver_parameters or {}, equation))

            def contract(cotangents):
                return fit.sensitivity_solve(self._sens_engine(), equation, solver, y0s, ts, sens_params,
                                             cotangents=cotangents)[0]

            ys = self.solve(params, y0, ts, solver_parameters)
            J, grad = fit.objective_gradient(objective, ys, spatial_ndim, contract, pmap)
            return J + reg.reg(p), grad * pmap.column_factors(p) + reg.reg_grad(p)

        return value_and_grad, value, pmap


def _named_gradient(grad, names, per_environment):
    """the library's block ``(B, len(names))`` as a dict: ``(B,)`` arrays per environment, floats of the sum in order otherwise"""
    if not per_environment:
        grad = fit.summed_in_order(grad)
    return {name: (grad[..., j].copy() if per_environment else float(grad[j])) for j, name in enumerate(names)}


def _array_weights(weights) -> dict:
    """``weights`` with a list or tuple under ``"D"`` as an array, which is what ``fit.regularization`` and
    ``fit.weight_vector`` take for a closure's coefficients"""
    weights = dict(weights or {})
    if isinstance(weights.get("D"), (list, tuple)):
        weights["D"] = np.asarray(weights["D"], dtype=np.float64)
    return weights


def _reject_rotating(model) -> None:
    """gradients of the rotating-frame GPE are out of scope: say so before anything else does"""
    from .gpe_control import reject_rotating

    reject_rotating(model.equation_type, model.solver_type)


def _is_gpe(equation_type) -> bool:
    from .numerics.equations.gross_pitaevskii import GPE2DTSControl

    return equation_type is GPE2DTSControl


def stack_training_data(data, inds):
    """``(y0s, values, ts)`` of a training set, as the reference builds them (pde_model.py:378-390): trajectory b
    starts at ``data["ys"][inds[b][0]]`` and is compared at ``inds[b][1:]``; the times are those of ``inds[0]``
    relative to its first"""
    ys = data["ys"]
    y0s = np.stack([np.asarray(ys[ind[0]]) for ind in inds])
    values = np.stack([np.stack([np.asarray(ys[ind[i]]) for i in range(1, len(ind))]) for ind in inds])
    ts = np.array([float(data["ts"][inds[0][i]]) - float(data["ts"][inds[0][0]]) for i in range(len(inds[0]))])
    return y0s, values, ts
