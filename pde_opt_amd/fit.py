"""Fitting closure coefficients to trajectories: the machinery behind ``PDEModel.train`` / ``residuals`` / ``mse``
(the reference's pde_opt/pde_model.py:138-460).

The reference differentiates the solve with diffrax's ``ForwardMode`` adjoint and hands the residuals to
optimistix (``LevenbergMarquardt`` / ``BFGS``).  Here the forward-mode tangents run on the GPU next to the
trajectories (``pdeopt_sens_advance``) and only the Gauss-Newton sums come back to the host
(``pdeopt_sens_accumulate``); the optimisers below work on those sums.

``PDEModel.optimize`` (pde_model.py:462-551) minimises a scalar objective ``J(ys)`` of the saved solution instead of a
residual against frames.  Its gradient ``dJ/dp_j = sum_q <dJ/dys[q], dys[q]/dp_j>`` contracts the cotangent field of
every save point with the same tangents (``pdeopt_sens_contract``): ``SolutionObjective`` / ``as_objective`` turn the
user's objective into ``(J, dJ/dys)``, ``objective_gradient`` assembles the gradient, ``minimize_bfgs`` is the BFGS of
``train(method="mse")`` on plain ``value_and_grad`` / ``value`` callables.

Covered: periodic Cahn-Hilliard in 2-D and 3-D (``mu`` / ``D``; IMEX or Euler), periodic 2-D Allen-Cahn (``mu`` /
``R``; Euler or RK4) and the three Butler-Volmer Allen-Cahn classes (``mu`` / ``j0``; Euler or RK4; at constant current
the voltage and its tangents are available at the save points, and ``train`` can fit a voltage curve next to the frames:
``add_voltage_sums``), all with ``derivs="fd"``.  The scalars of the Butler-Volmer classes (``alpha``, ``kappa``, ``Crate``,
``v``) are not trainable entries: they go in ``other_parameters``.

Also covered: the smoothed-boundary classes ``AllenCahn2DSmoothedBoundary`` (``mu`` / ``R``) and
``CahnHilliard2DSmoothedBoundary`` (``mu`` / ``D``) on a 2-D domain with Euler or RK4.  Their right-hand sides depend on
time through ``theta(t)`` and ``flux(t)``: every advance is told its start time, and the tangent kernel evaluates the
wall term at the stage times of the base solve.  ``f``, ``kappa``, ``theta`` and ``flux`` are fixed data
(``other_parameters``).

One scalar is trainable: ``kappa`` of the three periodic classes, as ``opt_parameters={"kappa": TrainableScalar(0.002)}``
(``numerics/functions/scalar.py``), alone or next to any mix of ``mu`` / ``D`` / ``R`` coefficients.  Its tangent is one
more environment (``L.SENS_KAPPA``); the optimiser's variable is ``log(kappa)`` (``positive=True``, the default), so the
sums the GPU returns for ``du/dkappa`` are scaled by ``kappa`` (``ParamMap.column_factors``) wherever they become
Jacobian columns, Gauss-Newton sums or gradients.  Under IMEX kappa moves the implicit operator: the sensitivity advance
then differentiates the operator too and runs rocFFT's transforms on every grid (csrc/sens.hip).  A plain float among
``opt_parameters`` stays refused; so does ``TrainableScalar`` for the smoothed-boundary and Butler-Volmer classes, whose
tangent kernels have no kappa term.
"""

from __future__ import annotations

import dataclasses
import math
from typing import Callable, List, Sequence, Tuple

import numpy as np

from . import _lib as L
from .integrate import constant_step_plan
from .numerics.closures import UnsupportedClosureError, is_torch_module
from .numerics.functions.legendre import ChemicalPotentialLegendrePolynomials, DiffusionLegendrePolynomials
from .numerics.functions.scalar import TrainableScalar

RTOL = ATOL = 1e-8  # optimistix tolerances of the reference's train (pde_model.py:398-401, 428-431)

# train(method="mse") with a torch.nn.Module as mu runs BFGS over the module's flattened parameters: the inverse-Hessian
# estimate is dense (8 n^2 bytes, O(n^2) work per step).  Above this many parameters train refuses and points to
# PDEModel.mse_backward, which fills .grad for any torch.optim optimiser.
MAX_DENSE_BFGS_PARAMS = 4096

# closure classes whose coefficient arrays are trainable, and the constructor argument that holds their role
# ("D" is Cahn-Hilliard's mobility, "R" Allen-Cahn's rate, "j0" the Butler-Volmer exchange current: the engine's second
# closure every time).
_ROLES = {"mu": L.SENS_MU, "D": L.SENS_MOB, "R": L.SENS_MOB, "j0": L.SENS_MOB}
# scalars of the equation that are trainable as a TrainableScalar, and their pdeopt_sens_role (coefficient index 0).
# Another scalar (alpha, Crate) would be a new entry here, a new pdeopt_sens_role and its term in the tangent kernels.
_SCALAR_ROLES = {"kappa": L.SENS_KAPPA}


# ---- parameters -----------------------------------------------------------------------------------------------------


class NotTrainableError(ValueError, NotImplementedError):
    """``opt_parameters`` names something the sensitivity path cannot train, or nothing at all.  A ``ValueError`` -- the
    argument is wrong -- and a ``NotImplementedError`` -- training that entry (a scalar such as kappa, alpha or Crate, a plain
    callable where a Legendre closure belongs) is not implemented: fits of equations without any sensitivity support have
    always been refused with the latter, and a caller who catches either keeps working as support grows."""


@dataclasses.dataclass
class ParamMap:
    """The trainable leaves of ``opt_parameters`` as one flat vector ``p``.  Entry ``j`` is coefficient ``index[j]``
    of the closure in role ``role[j]``, or -- for a ``TrainableScalar`` (size 1, role ``L.SENS_KAPPA``, index 0) -- the
    scalar's variable: ``log(value)`` when ``positive``, else the value.  ``closure_desc()`` folds a polynomial ``prior_fn`` into the series, so the
    kernel's coefficients are ``p`` plus a fixed offset; fitted closures are rebuilt from ``p`` itself (same class,
    same ``prior_fn``), which keeps the offset out of the returned values."""

    keys: List[str]
    templates: list
    sizes: List[int]
    # Allen-Cahn (periodic, Butler-Volmer, smoothed-boundary): mu_h itself, not only its gradient, enters the right-hand side
    mu_constant_active: bool = False

    @classmethod
    def of(cls, opt_parameters: dict, equation_type=None) -> "ParamMap":
        """``equation_type`` decides whether mu's constant coefficient has a tangent (Allen-Cahn, smoothed-boundary
        Allen-Cahn included) or is inert (Cahn-Hilliard -- the smoothed-boundary form too: a constant added to ``inner``
        drops out of ``grad(inner)`` -- and the default)"""
        keys, templates, sizes = [], [], []
        for key, value in opt_parameters.items():
            if key in _SBM_FIXED and _is_smoothed_boundary(equation_type):
                raise NotTrainableError(
                    f"opt_parameters[{key!r}]: {key} of {equation_type.__name__} is fixed data of the fit (the free energy of "
                    "the wall term, the gradient coefficient, the contact angle theta(t) and the boundary flux flux(t) have "
                    "no tangent kernel); pass it in other_parameters")
            if key in _SCALAR_ROLES and isinstance(value, TrainableScalar):
                if _is_butler_volmer(equation_type):
                    raise NotTrainableError(
                        f"opt_parameters[{key!r}]: {key} of {equation_type.__name__} is not trainable (the Butler-Volmer tangent "
                        "kernels have no kappa term: it is trainable for the periodic Cahn-Hilliard and Allen-Cahn classes only); "
                        "pass a number in other_parameters")
                keys.append(key)
                templates.append(value)
                sizes.append(1)
                continue
            if key not in _ROLES or not isinstance(value, (ChemicalPotentialLegendrePolynomials, DiffusionLegendrePolynomials)):
                raise NotTrainableError(
                    f"opt_parameters[{key!r}]: only the coefficient arrays of ChemicalPotentialLegendrePolynomials / "
                    "DiffusionLegendrePolynomials in the 'mu' and 'D' (Allen-Cahn: 'R', Butler-Volmer: 'j0') roles are trainable "
                    "(kappa and other scalars would move the implicit operator of the solver: kappa of the periodic classes is "
                    "trainable as a TrainableScalar, a plain number is fixed data); pass them in other_parameters")
            keys.append(key)
            templates.append(value)
            sizes.append(len(value.expansion.params))
        if not keys:
            raise NotTrainableError("opt_parameters holds no trainable closure")
        return cls(keys, templates, sizes, _is_allen_cahn(equation_type) or _is_butler_volmer(equation_type)
                   or _is_smoothed_boundary(equation_type, allen_cahn_only=True))

    @property
    def size(self) -> int:
        return sum(self.sizes)

    def all_params(self) -> List[Tuple[int, int]]:
        return [(_SCALAR_ROLES[k] if k in _SCALAR_ROLES else _ROLES[k], i) for k, n in zip(self.keys, self.sizes) for i in range(n)]

    def active(self) -> np.ndarray:
        """entries whose tangent is not identically zero.  For Cahn-Hilliard mu's constant coefficient is not: only
        grad mu enters the right-hand side, so its tangent is never solved for (its Jacobian column is exactly 0).
        Allen-Cahn's right-hand side holds mu itself: every entry is active.  A scalar (kappa) is active on every
        equation"""
        return np.array([self.mu_constant_active or not (role == L.SENS_MU and i == 0) for role, i in self.all_params()])

    def _scalars(self):
        """(offset in p, template) of every TrainableScalar entry"""
        o = 0
        for tpl, n in zip(self.templates, self.sizes):
            if isinstance(tpl, TrainableScalar):
                yield o, tpl
            o += n

    def column_factors(self, p: np.ndarray) -> np.ndarray:
        """``d value / d p`` per entry of ``p``: ``kappa`` for a positive scalar (its variable is the logarithm), 1
        elsewhere.  The tangents the GPU advances are derivatives with respect to the VALUES; multiplied by this they
        are the optimiser's columns."""
        s = np.ones(self.size)
        for o, tpl in self._scalars():
            s[o] = tpl.with_variable(p[o]).column_factor()
        return s

    def feasible(self, p: np.ndarray) -> bool:
        """can an equation be built at ``p``?  False when a ``positive=False`` kappa has a value ``<= 0`` (or any entry
        is not finite): such a trial is a rejected step / failed line-search point and is never sent to the engine"""
        if not np.all(np.isfinite(p)):
            return False
        return all(tpl.with_variable(p[o]).value > 0.0 for o, tpl in self._scalars())

    def scale_sums(self, p, rdp, G):
        """the sums over all entries (``expand``) turned from value-derivatives into variable-derivatives"""
        s = self.column_factors(p)
        return rdp * s, G * np.outer(s, s)

    def sens_params(self) -> List[Tuple[int, int]]:
        """the (role, coefficient) pairs of the tangents the GPU advances"""
        return [q for q, a in zip(self.all_params(), self.active()) if a]

    def expand(self, rdp, G):
        """the sums of the active tangents as sums over all entries (zero for the inert ones)"""
        act = np.nonzero(self.active())[0]
        r = np.zeros(self.size)
        g = np.zeros((self.size, self.size))
        r[act] = rdp
        g[np.ix_(act, act)] = G
        return r, g

    def flatten(self, params: dict) -> np.ndarray:
        return np.concatenate([np.array([params[k].variable()]) if isinstance(params[k], TrainableScalar)
                               else np.asarray(params[k].expansion.params, dtype=np.float64) for k in self.keys])

    def build(self, p: np.ndarray) -> dict:
        out, o = {}, 0
        for key, tpl, n in zip(self.keys, self.templates, self.sizes):
            coef = np.array(p[o:o + n], dtype=np.float64)
            o += n
            if isinstance(tpl, TrainableScalar):
                out[key] = tpl.with_variable(coef[0])
            elif isinstance(tpl, ChemicalPotentialLegendrePolynomials):
                out[key] = ChemicalPotentialLegendrePolynomials(coef, tpl.prior_fn)
            else:
                out[key] = DiffusionLegendrePolynomials(coef)
        return out


def plain(parameters: dict) -> dict:
    """``parameters`` with every ``TrainableScalar`` replaced by its float: what an equation class is built from"""
    return {k: (float(v) if isinstance(v, TrainableScalar) else v) for k, v in parameters.items()}


def _is_allen_cahn(equation_type) -> bool:
    from .numerics.equations.phase_field import AllenCahn2DPeriodic

    return isinstance(equation_type, type) and issubclass(equation_type, AllenCahn2DPeriodic)


_SBM_FIXED = ("f", "kappa", "theta", "flux")  # constructor arguments of the smoothed-boundary classes that are never trainable


def _is_smoothed_boundary(equation_type, allen_cahn_only=False) -> bool:
    from .numerics.equations.smoothed_boundary import AllenCahn2DSmoothedBoundary, CahnHilliard2DSmoothedBoundary

    classes = (AllenCahn2DSmoothedBoundary,) if allen_cahn_only else (AllenCahn2DSmoothedBoundary, CahnHilliard2DSmoothedBoundary)
    return isinstance(equation_type, type) and issubclass(equation_type, classes)


def _is_butler_volmer(equation_type, constant_current_only=False) -> bool:
    from .numerics.equations import butler_volmer as bv

    if not (isinstance(equation_type, type) and issubclass(equation_type, bv._ButlerVolmer)):
        return False
    return not constant_current_only or equation_type._mode == L.BV_CONSTANT_CURRENT


def _leaves(obj) -> list:
    """coefficient arrays of a closure, the flattened parameters of a torch.nn.Module, the array / number itself, or
    nothing (None, callables)"""
    if obj is None:
        return []
    if is_torch_module(obj):
        from .fieldmu import flatten_params

        return [flatten_params(obj)]
    if isinstance(obj, (ChemicalPotentialLegendrePolynomials, DiffusionLegendrePolynomials)):
        return [np.asarray(obj.expansion.params, dtype=np.float64)]
    if isinstance(obj, TrainableScalar):  # the optimiser's variable, as a one-coefficient closure's coefficient
        return [np.array([obj.variable()])]
    if isinstance(obj, (int, float, np.ndarray, np.number)):
        a = np.asarray(obj)
        return [a.astype(np.float64)] if np.issubdtype(a.dtype, np.inexact) or isinstance(obj, float) else []
    return []


def regularization(parameters: dict, weights: dict, lambda_reg: float) -> float:
    """``lambda sum_i w_i p_i^2`` over the coefficient arrays named in ``weights`` (pde_model.py:170-214); None
    leaves are ignored"""
    reg = 0.0
    for key, w in weights.items():
        for wl, pl in zip(_leaves(w), _leaves(parameters.get(key))):
            reg += float(lambda_reg) * float(np.sum(wl * pl ** 2))
    return reg


def weight_vector(pmap: ParamMap, weights: dict) -> np.ndarray:
    """the weights of the trainable entries, in ``p`` order (0 where ``weights`` names none)"""
    w = []
    for key, n in zip(pmap.keys, pmap.sizes):
        leaves = _leaves(weights.get(key))
        a = np.zeros(n)
        if leaves:
            src = np.broadcast_to(leaves[0], (n,)) if leaves[0].ndim == 0 else leaves[0][:n]
            a[: len(src)] = src
        w.append(a)
    return np.concatenate(w)


# ---- the sensitivity solve ------------------------------------------------------------------------------------------


def walk_save_points(t0: float, t1: float, dt: float, ts: Sequence[float], advance: Callable, snapshot: Callable,
                     visit: Callable):
    """The constant-step plan and save-point logic of ``integrate.diffeqsolve`` (SaveAt(ts=...), linear dense
    output): ``advance(dt, n, t)`` runs n substeps, ``snapshot()`` keeps the state at the start of a step that holds
    a save point, ``visit(q, theta)`` is called at save point q with ``theta = None`` on a step edge, else the
    position inside the last step."""
    n_full, rem = constant_step_plan(t0, t1, dt)
    total = n_full + (1 if rem > 0 else 0)

    def edge(i):
        return t1 if i >= total else t0 + i * dt

    def steps(first, count):
        full = max(0, min(first + count, n_full) - first)
        if full:
            advance(dt, full, t0 + first * dt)
        if first + count > n_full and rem > 0:
            advance(rem, 1, t0 + n_full * dt)  # the remainder step: another dt, another implicit multiplier

    done, inside = 0, None
    for q, tq in enumerate(float(t) for t in ts):
        if tq <= t0 or total == 0:
            k_end = 0
        else:
            k_end = min(total, max(1, int(math.ceil((tq - t0) / dt - 1e-9))))
        if k_end == 0 or abs(edge(k_end) - tq) <= 1e-12 * max(1.0, abs(tq)):
            steps(done, k_end - done)
            done, inside = k_end, None
            visit(q, None)
        else:
            a, b = edge(k_end - 1), edge(k_end)
            if inside != k_end:
                steps(done, k_end - 1 - done)
                snapshot()
                steps(k_end - 1, 1)
                done, inside = k_end, k_end
            visit(q, (tq - a) / (b - a))


def _configure(eng, equation, solver, y0s, pmap_params, t0, t1):
    B = y0s.shape[0]
    P = len(pmap_params)
    eng.configure(dtype=y0s.dtype, batch=(1 + P) * B, **equation._engine_problem())
    equation._engine_upload(eng, t0, t1)
    solver.configure_engine(eng, equation)
    eng.sens_configure(B, pmap_params)
    state = np.zeros(((1 + P) * B,) + y0s.shape[1:], dtype=y0s.dtype)
    state[:B] = y0s  # the tangents start at zero: the initial states are data
    eng.set_state(state)


def sensitivity_solve(eng, equation, solver, y0s, ts, sens_params, dt0=1e-6, fields=False, frames_key=None, frames=None,
                      cotangents=None, voltages=None):
    """Solve B trajectories and their P tangents through ``ts``.

    ``y0s`` ``(B, *spatial)``, with ``spatial`` ``(nx, ny)`` or ``(nx, ny, nz)``.  ``frames`` ``(T - 1, B, *spatial)``:
    the observed values at ``ts[1:]``; they are uploaded when ``frames_key`` differs from the engine's last upload.
    Returns the Gauss-Newton sums per trajectory summed over the save points, ``(B, 1 + P + P (P + 1) / 2)`` fp64
    (None without frames), and with ``fields=True`` the states of all ``(1 + P) B`` environments at every save point,
    ``(T, (1 + P) B, *spatial)``.

    ``cotangents`` ``(T - 1, B, *spatial)`` instead of ``frames``: ``dJ/dys`` of an objective at ``ts[1:]`` (``ts[0]``
    contributes nothing: the initial state is data).  They are uploaded at every call -- they change with every
    evaluation -- and the first return value is ``sum_q <cotangents[q], dys[q]/dp_j>`` per trajectory, ``(B, P)`` fp64.

    ``voltages``: a list that receives, per save point (``ts[0]`` included), the ``(B, 1 + P)`` array of the voltage of the
    constant-current constraint and its tangents ``dv/dp_j`` (``pdeopt_sens_bv_voltage``; the constant-current
    Butler-Volmer classes).  Every save point must then fall on a step edge -- the voltage of a linearly interpolated
    state is not the interpolated voltage -- otherwise ``ValueError``."""
    if frames is not None and cotangents is not None:
        raise ValueError("frames and cotangents share one device buffer: pass one of them")
    if _is_butler_volmer(type(equation)):
        if solver.integrator not in (L.INT_EULER, L.INT_RK4):
            raise NotImplementedError("Butler-Volmer sensitivities support Euler and RK4")
        if callable(getattr(equation, "v", None)):
            raise NotImplementedError("Butler-Volmer sensitivities are autonomous: a voltage protocol v(t) is not supported")
    elif _is_allen_cahn(type(equation)):
        if solver.integrator not in (L.INT_EULER, L.INT_RK4):
            raise NotImplementedError("Allen-Cahn sensitivities support Euler and RK4")
    elif _is_smoothed_boundary(type(equation)):
        if solver.integrator not in (L.INT_EULER, L.INT_RK4):
            raise NotImplementedError(f"{type(equation).__name__} sensitivities support Euler and RK4")
    elif solver.integrator not in (L.INT_IMEX, L.INT_EULER):
        raise NotImplementedError("sensitivities support SemiImplicitFourierSpectral (IMEX) and Euler")
    if voltages is not None and not _is_butler_volmer(type(equation), constant_current_only=True):
        raise ValueError(f"{type(equation).__name__} has no voltage to differentiate: only the constant-current Butler-Volmer "
                         "classes solve for one")
    y0s = np.asarray(y0s)
    if y0s.dtype not in (np.float32, np.float64):
        y0s = y0s.astype(np.float64)
    ts = np.asarray(ts, dtype=np.float64)
    t0, t1 = float(ts[0]), float(ts[-1])
    _configure(eng, equation, solver, y0s, sens_params, t0, t1)
    if frames is not None and (frames_key is None or getattr(eng, "_sens_frames_key", None) != frames_key):
        eng.sens_set_data(frames)
        eng._sens_frames_key = frames_key
    if cotangents is not None:
        eng.sens_set_data(cotangents)
        eng._sens_frames_key = None  # the frames of a fit are gone from the device
    reduce_at = eng.sens_accumulate if frames is not None else (eng.sens_contract if cotangents is not None else None)
    sums = [None]
    out = []

    def visit(q, theta):
        if voltages is not None:
            if theta is not None:
                raise ValueError(f"ts[{q}] = {ts[q]!r} is not on a step edge (dt0 = {dt0!r}): the voltage of an interpolated "
                                 "state is not the interpolated voltage; choose ts on multiples of dt0")
            voltages.append(eng.sens_bv_voltage())
        if fields:
            out.append(eng.get_state() if theta is None else eng.get_interpolated(theta))
        if reduce_at is not None and q >= 1:
            s = reduce_at(q - 1, 1.0 if theta is None else theta, theta is not None)
            sums[0] = s if sums[0] is None else sums[0] + s

    walk_save_points(t0, t1, float(dt0), ts,
                     lambda dt, n, t: eng.sens_advance(solver.integrator, dt, n, t), eng.snapshot, visit)
    return sums[0], (np.stack(out) if fields else None)


def unpack_sums(sums: np.ndarray, P: int):
    """``(sum r^2, sum_j r dpred_j [P], sum dpred_i dpred_j [P, P])`` of per-trajectory sums ``(B, K)``, summed over
    the trajectories in order"""
    tot = np.zeros(sums.shape[1])
    for row in sums:
        tot = tot + row
    ssr = float(tot[0])
    rdp = tot[1:1 + P].copy()
    G = np.zeros((P, P))
    iu = np.triu_indices(P)
    G[iu] = tot[1 + P:]
    G = G + np.triu(G, 1).T
    return ssr, rdp, G


def add_voltage_sums(ssr: float, rdp: np.ndarray, G: np.ndarray, r_v, dv, weight: float):
    """The Gauss-Newton sums of a fit with the voltage residuals added: ``r_v`` ``(n,)`` = observed - predicted voltage
    per trajectory and save point, ``dv`` ``(n, P)`` the predicted voltage's tangents, both in fp64; every voltage term
    is multiplied by ``weight`` (``train`` folds ``voltage_weight M / M_V`` into it, so that ``Objective.M`` stays the
    number of field residuals).  Returns ``(ssr + w sum r_v^2, rdp + w sum r_v dv_j, G + w sum dv_i dv_j)``."""
    r_v = np.asarray(r_v, dtype=np.float64).reshape(-1)
    dv = np.asarray(dv, dtype=np.float64).reshape(r_v.size, -1)
    w = float(weight)
    return ssr + w * float(r_v @ r_v), np.asarray(rdp) + w * (dv.T @ r_v), np.asarray(G) + w * (dv.T @ dv)


# ---- optimisers -------------------------------------------------------------------------------------------------------


@dataclasses.dataclass
class Objective:
    """What the optimisers need from a model: ``sums(p) -> (sum r^2, sum r dpred [P], sum dpred dpred^T [P, P])``
    (a sensitivity solve), ``ssr(p) -> sum r^2`` (a forward solve), the number M of residual entries, and the
    regularisation ``lambda sum w p^2``."""

    sums: Callable
    ssr: Callable
    M: int
    lambda_reg: float = 0.0
    w: np.ndarray = None

    def reg(self, p):
        return float(self.lambda_reg * np.sum(self.w * p * p)) if self.w is not None else 0.0

    def reg_grad(self, p):
        return 2.0 * self.lambda_reg * self.w * p if self.w is not None else np.zeros_like(p)


def _converged(p_old, p_new, f_old, f_new, rtol=RTOL, atol=ATOL):
    dp = np.all(np.abs(p_new - p_old) <= atol + rtol * np.abs(p_new))
    df = abs(f_new - f_old) <= atol + rtol * abs(f_new)
    return bool(dp and df)


def levenberg_marquardt(obj: Objective, p0, max_steps=100, rtol=RTOL, atol=ATOL):
    """Minimise ``1/2 (sum r^2 + reg^2)`` -- the objective optimistix.least_squares gives the residual pytree
    ``(batch_residuals, reg)`` -- on the normal equations.  Jacobian of r: ``-dpred``; of reg: ``2 lambda w p``.
    A column of zeros (mu's constant coefficient: grad of a constant is 0) leaves its entry where it started: the
    damping keeps the system regular and its right-hand side is 0.  Returns ``(p, history of objectives)``; like the
    reference's ``throw=False``, the last iterate when ``max_steps`` runs out."""
    p = np.array(p0, dtype=np.float64)

    def model(p):
        ssr, rdp, G = obj.sums(p)
        reg, g = obj.reg(p), obj.reg_grad(p)
        f = 0.5 * (ssr + reg * reg)
        JTJ = G + np.outer(g, g)
        JTr = -rdp + g * reg
        return f, JTJ, JTr

    f, JTJ, JTr = model(p)
    hist = [f]
    lam = 1e-3 * max(float(np.max(np.diag(JTJ))), 1e-300)
    for _ in range(max_steps):
        if not np.all(np.isfinite(JTr)) or not math.isfinite(f):
            break
        A = JTJ + lam * np.eye(len(p))
        step = -np.linalg.solve(A, JTr)
        pred_red = -(JTr @ step + 0.5 * step @ JTJ @ step)
        p_new = p + step
        f_new, JTJ_new, JTr_new = model(p_new)
        rho = (f - f_new) / pred_red if pred_red > 0 else -1.0
        if math.isfinite(f_new) and f_new <= f and rho > 0:
            done = _converged(p, p_new, f, f_new, rtol, atol)
            p, f, JTJ, JTr = p_new, f_new, JTJ_new, JTr_new
            hist.append(f)
            lam *= 1.0 / 3.0 if rho > 0.75 else (1.0 if rho > 0.25 else 2.0)
            if done:
                break
        else:
            lam *= 4.0
            if np.all(np.abs(step) <= atol + rtol * np.abs(p)):
                break
    return p, hist


def _bfgs_loop(value_and_grad, value, p, f, g, H, max_steps, rtol, atol):
    """BFGS from the point ``p`` with objective ``f``, gradient ``g`` and inverse-Hessian estimate ``H``:
    ``value_and_grad(p) -> (f, g)`` at accepted points, ``value(p) -> f`` at the trial points of the backtracking
    (Armijo) line search.  Returns ``(p, history of objectives)``."""
    hist = [f]
    for _ in range(max_steps):
        if not np.all(np.isfinite(g)) or not math.isfinite(f):
            break
        d = -(H @ g)
        slope = float(g @ d)
        if slope >= 0:  # not a descent direction: restart from the gradient
            d, slope = -g, -float(g @ g)
        if slope == 0.0:
            break
        a = 1.0
        f_new = value(p + a * d)
        while not (math.isfinite(f_new) and f_new <= f + 1e-4 * a * slope) and a > 1e-9:
            a *= 0.5
            f_new = value(p + a * d)
        if a <= 1e-9:  # no decrease along d: the objective is at its floating-point floor
            break
        p_new = p + a * d
        f_new, g_new = value_and_grad(p_new)
        s, y = p_new - p, g_new - g
        sy = float(s @ y)
        if sy > 0:
            rho = 1.0 / sy
            V = np.eye(len(p)) - rho * np.outer(s, y)
            H = V @ H @ V.T + rho * np.outer(s, s)
        done = _converged(p, p_new, f, f_new, rtol, atol)
        p, f, g = p_new, f_new, g_new
        hist.append(f)
        if done:
            break
    return p, hist


def bfgs(obj: Objective, p0, max_steps=100, rtol=RTOL, atol=ATOL):
    """Minimise ``mean(r^2) + reg`` (the reference's ``mse`` under optimistix.BFGS).  Gradient
    ``-(2 / M) sum r dpred + 2 lambda w p`` from the tangents; trial points of the backtracking (Armijo) line search
    are forward-only solves.  The inverse-Hessian estimate starts from the pseudo-inverse of the Gauss-Newton
    Hessian the same tangents give at the starting point (``2 / M sum dpred dpred^T + 2 lambda diag w``), so a
    direction with no gradient (mu's constant coefficient) is never moved."""
    p = np.array(p0, dtype=np.float64)

    def fg(p):
        ssr, rdp, G = obj.sums(p)
        return ssr / obj.M + obj.reg(p), -(2.0 / obj.M) * rdp + obj.reg_grad(p), G

    def f_only(p):
        return obj.ssr(p) / obj.M + obj.reg(p)

    f, g, G = fg(p)
    w = obj.w if obj.w is not None else np.zeros_like(p)
    H = np.linalg.pinv((2.0 / obj.M) * G + np.diag(2.0 * obj.lambda_reg * w), rcond=1e-12, hermitian=True)
    return _bfgs_loop(lambda q: fg(q)[:2], f_only, p, f, g, H, max_steps, rtol, atol)


def minimize_bfgs(value_and_grad: Callable, value: Callable, p0, max_steps=100, rtol=RTOL, atol=ATOL):
    """The BFGS of ``bfgs`` for a general objective: ``value_and_grad(p) -> (f, g)``, ``value(p) -> f``.  There is no
    Gauss-Newton Hessian to start from: the inverse-Hessian estimate starts at the identity, as optimistix.BFGS does
    (the reference's ``optimize``, pde_model.py:531-546).  A direction with no gradient is still never moved: the
    update leaves its row and column of the identity alone."""
    p = np.array(p0, dtype=np.float64)
    f, g = value_and_grad(p)
    return _bfgs_loop(value_and_grad, value, p, f, np.asarray(g, dtype=np.float64), np.eye(len(p)), max_steps, rtol, atol)


# ---- a general objective of the solution (PDEModel.optimize) -------------------------------------------------------------

OBJECTIVE_FORMS = ("objective_function must be a torch-differentiable callable (it receives the solution as a float64 "
                   "torch.Tensor of shape (len(ts), *y0.shape) and returns a 0-d tensor that depends on it) or an object "
                   "with value_and_grad(ys) -> (float, ndarray of ys.shape) and optionally value(ys) -> float")


class SolutionObjective:
    """``J(ys)`` of the saved solution ``ys`` ``(T, *y0.shape)`` with its cotangent: ``value_and_grad(ys) ->
    (J, dJ/dys)`` as ``(float, float64 array of ys.shape)``, ``value(ys) -> J``."""

    def __init__(self, value_and_grad: Callable, value: Callable = None):
        self._vg, self._v = value_and_grad, value

    def value_and_grad(self, ys):
        ys = np.asarray(ys)
        J, g = self._vg(ys)
        g = np.asarray(g, dtype=np.float64)
        if g.shape != ys.shape:
            raise ValueError(f"the objective's gradient has shape {g.shape}, the solution {ys.shape}")
        return float(J), g

    def value(self, ys):
        return float(self._v(np.asarray(ys))) if self._v is not None else self.value_and_grad(ys)[0]


def torch_objective(fn: Callable) -> SolutionObjective:
    """``fn(torch.Tensor) -> 0-d torch.Tensor`` as a SolutionObjective: the cotangent comes from torch.autograd.  The
    solution is handed over in float64 whatever the solve's dtype (the values are the solve's own)."""
    import torch

    def value_and_grad(ys):
        y = torch.tensor(np.asarray(ys, dtype=np.float64), requires_grad=True)
        J = fn(y)
        if not isinstance(J, torch.Tensor) or J.numel() != 1 or not J.requires_grad:
            raise NotImplementedError(OBJECTIVE_FORMS + f" (the callable returned {type(J).__name__})")
        (g,) = torch.autograd.grad(J.reshape(()), y)
        return float(J.detach()), g.numpy()

    def value(ys):
        with torch.no_grad():
            return float(fn(torch.tensor(np.asarray(ys, dtype=np.float64))))

    return SolutionObjective(value_and_grad, value)


def as_objective(objective_function, probe=None) -> SolutionObjective:
    """The two accepted forms of ``PDEModel.optimize``'s objective as a SolutionObjective; anything else raises
    ``NotImplementedError``.  A plain callable is tried once on ``probe`` (an array of the solution's shape) to see
    that torch can differentiate it."""
    if objective_function is None:
        raise NotImplementedError("PDEModel.optimize needs an objective: " + OBJECTIVE_FORMS)
    if callable(getattr(objective_function, "value_and_grad", None)):
        value = getattr(objective_function, "value", None)
        return SolutionObjective(objective_function.value_and_grad, value if callable(value) else None)
    if not callable(objective_function):
        raise NotImplementedError(OBJECTIVE_FORMS)
    obj = torch_objective(objective_function)
    if probe is not None:
        try:
            obj.value_and_grad(probe)
        except NotImplementedError:
            raise
        except Exception as e:  # numpy-only callables fail on a tensor that requires grad
            raise NotImplementedError(OBJECTIVE_FORMS + f" (torch could not differentiate it: {type(e).__name__}: {e})") from e
    return obj


def summed_in_order(rows):
    """the sum of ``rows[b]`` over the environments b = 0, 1, ...: one fixed order, the same bits on every run"""
    tot = np.zeros(rows.shape[1:])
    for row in rows:
        tot = tot + row
    return tot


def objective_gradient(objective: SolutionObjective, ys, spatial_ndim: int, contract: Callable, pmap: ParamMap):
    """``(J, dJ/dp)`` of ``J(ys)`` over all entries of ``p``, for ``ys`` ``(T, *spatial)`` or ``(T, B, *spatial)``.  The
    objective gives ``g = dJ/dys``; ``contract(g[1:] as (T - 1, B, *spatial)) -> (B, n active)``, the sums
    ``sum_q <g_q, dys_q/dp_j>``, is a sensitivity solve (frame 0's cotangent is dropped: the initial state is data); the
    trajectories are summed in order and the inert entries get 0."""
    ys = np.asarray(ys)
    J, g = objective.value_and_grad(ys)
    n_active = int(np.count_nonzero(pmap.active()))
    cot = g[1:].reshape((g.shape[0] - 1, -1) + g.shape[g.ndim - spatial_ndim:])
    per_traj = np.asarray(contract(np.ascontiguousarray(cot)), dtype=np.float64).reshape(-1, n_active)
    grad = np.zeros(pmap.size)
    grad[np.nonzero(pmap.active())[0]] = summed_in_order(per_traj)
    return J, grad


_SUPPORTED = ("CahnHilliard2DPeriodic on a 2-D domain or CahnHilliard3DPeriodic on a 3-D domain, or AllenCahn2DPeriodic or a "
              "Butler-Volmer Allen-Cahn class on a 2-D domain"
              ", or AllenCahn2DSmoothedBoundary or CahnHilliard2DSmoothedBoundary on a 2-D domain")


def reject_unsupported(model):
    """the configurations the sensitivity path covers: periodic Cahn-Hilliard in 2-D or 3-D with IMEX or Euler,
    periodic 2-D Allen-Cahn, the Butler-Volmer Allen-Cahn classes and the two smoothed-boundary classes with Euler or RK4,
    FD derivatives.  The equation / domain pair is checked here, before any equation is built.  The tangents always
    advance with constant steps: train / residuals / optimize take no step-size controller."""
    from .numerics.equations.phase_field import AllenCahn2DPeriodic, CahnHilliard2DPeriodic, CahnHilliard3DPeriodic
    from .numerics.solvers import RK4, Euler, SemiImplicitFourierSpectral, reject_implicit_gradients

    reject_implicit_gradients(model.solver_type, "train / residuals / optimize")
    dims = {CahnHilliard2DPeriodic: 2, CahnHilliard3DPeriodic: 3, AllenCahn2DPeriodic: 2}.get(model.equation_type)
    if _is_butler_volmer(model.equation_type) or _is_smoothed_boundary(model.equation_type):
        dims = 2
    if dims is None:
        raise NotImplementedError(f"train / residuals sensitivities support {_SUPPORTED}, not "
                                  f"{model.equation_type.__name__}")
    if len(model.domain.points) != dims:
        raise NotImplementedError(f"train / residuals sensitivities support {_SUPPORTED}, not "
                                  f"{model.equation_type.__name__} on a {len(model.domain.points)}-D domain")
    if (model.equation_type is AllenCahn2DPeriodic or _is_butler_volmer(model.equation_type)
            or _is_smoothed_boundary(model.equation_type)):
        if model.solver_type not in (Euler, RK4):
            raise NotImplementedError(f"train / residuals sensitivities of {model.equation_type.__name__} support the Euler and "
                                      f"RK4 solvers, not {model.solver_type.__name__}")
    elif model.solver_type not in (SemiImplicitFourierSpectral, Euler):
        raise NotImplementedError(f"train / residuals sensitivities support the SemiImplicitFourierSpectral and Euler "
                                  f"solvers, not {model.solver_type.__name__}")


def check_equation(equation):
    if getattr(equation, "_mu_module", None) is not None:
        from .numerics.equations.phase_field import FIELD_MU_SUPPORT

        raise NotImplementedError("forward-mode sensitivities (train of closure coefficients, optimize) do not run with a "
                                  "torch.nn.Module as mu, not even one held fixed among other_parameters: the module itself is "
                                  "trained, alone with D and kappa fixed or together with D, by train(opt_parameters={'mu': "
                                  "module[, 'D': DiffusionLegendrePolynomials]}, method='mse') or mse_backward, on " + FIELD_MU_SUPPORT)
    if _is_butler_volmer(type(equation)) and callable(getattr(equation, "v", None)):
        raise NotImplementedError("Butler-Volmer sensitivities are autonomous: a voltage protocol v(t) is not supported; pass a "
                                  "number as v")
    if getattr(equation, "derivs", "fd") != "fd":
        raise NotImplementedError('train sensitivities support derivs="fd" only (the tangent kernel differentiates the '
                                  'finite-difference right-hand side)')
    # (the smoothed-boundary classes: the free energy f of the wall term is differentiated in the kernel too)
    for d in (equation._mu_desc, equation._mob_desc, getattr(equation, "_f_desc", None)):
        if d is not None and d.kind == L.CL_JIT:
            raise UnsupportedClosureError("train sensitivities need closures of the in-kernel family (polynomial / "
                                          "Legendre series with the logit, mixing-entropy and exp forms)")
