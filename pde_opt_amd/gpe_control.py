"""Gradient-based control of the Gross-Pitaevskii equation: the reverse-mode (discrete adjoint) gradient of a scalar
objective of the saved solution over the numbers of the laser spots (``GaussianSpots``) that steer it -- the
reference's ``PDEModel.optimize`` on ``GPE2DTSControl`` + ``StrangSplitting``, which it differentiates with generic
reverse-mode AD (pde_model.py:462-551).

One scalar objective, a field-sized state, a few control numbers: reverse mode.  The forward pass is the library's Strang
step (``pdeopt_advance``), the backward sweep ``pdeopt_gpe_adjoint_step`` (csrc/gpe_adjoint.hip), one call per substep:
it takes the cotangent of a substep's end state to that of its start state and adds the spots' gradient on the device.
The backward sweep needs the state every substep started from: substep and save-point schedule, the split of a save
point's cotangent, the chunked recomputation and the stream rule are those of ``pde_opt_amd.reverse``, which the
network ``mu`` of ``pde_opt_amd.fieldmu`` shares.  The cotangents of the saved solution are known before the sweep: the
forward pass stops where the last chunk starts, a cotangent is uploaded when its state is reached, and the sweep ends
with ``dJ/dy0``.  A chunk holds at most ``PDEOPT_GPE_ADJOINT_CHUNK_BYTES`` (default 1 GiB;
``GpeControlSolver.chunk_bytes`` overrides it).

Covered: ``GPE2DTSControl`` whose ``lights`` is a ``GaussianSpots`` evaluated in-kernel, ``StrangSplitting`` with
``ConstantStepSize``, fp32 and fp64, one state or a batch sharing the spots.  torch (device tensors for the held states
and cotangents) is imported when a solver is built, not with the package.

The rotating-frame pair ``GPE2DTSRot`` + ``RotatingStrangSplitting`` has its own backward substep,
``pdeopt_gpe_rot_adjoint_step`` (csrc/gpe_rot_adjoint.hip): the gradient over k, e and omega of every environment and
over the start state.  ``RotControlSolver`` drives it with the same sweep (``GpeControlSolver._sweep``);
``PDEModel.rotation_gradient`` / ``optimize_rotation`` are its public entries.

With ``lights`` (Gaussian spots evaluated in-kernel) or ``omega_rate`` the backward substep is
``pdeopt_gpe_rot_stir_adjoint_step`` (csrc/gpe_rot_adjoint.hip): it adds the gradient over the rate and over the
seven numbers of every spot.  ``RotStirControlSolver`` drives it, the sweep carrying the spots' block as a second
gradient block; ``PDEModel.stirring_gradient`` / ``optimize_stirring`` are its public entries.
"""

from __future__ import annotations

import numpy as np

from . import _lib as L
from .numerics.functions.lights import SPOT_NUMBERS, GaussianSpot, GaussianSpots
from .reverse import StreamSolver, chunk_length, known_cotangent_sweep, schedule

CHUNK_BYTES_ENV = "PDEOPT_GPE_ADJOINT_CHUNK_BYTES"

GPE_CONTROL_SUPPORT = ("gradients of the GPE support GPE2DTSControl whose lights is a GaussianSpots (evaluated in-kernel: "
                       "time_dependent is not False) with StrangSplitting and ConstantStepSize; the optimisation variables are "
                       "the spots' numbers (opt_parameters = {'lights': GaussianSpots}), not k, e, trap_factor or another "
                       "lights callable; the rotating-frame GPE2DTSRot has its own entries, rotation_gradient and optimize_rotation")


class SpotMap:
    """The numbers of a ``GaussianSpots`` as one flat fp64 vector, ``SPOT_NUMBERS`` per spot in user units (the
    counterpart of ``fit.ParamMap``).  Entries that are not ``free`` keep a zero gradient, so BFGS never moves them."""

    def __init__(self, n_spots: int, free=None):
        self.n_spots = int(n_spots)
        self.free = None if free is None else tuple(n for n in SPOT_NUMBERS if n in free)

    @classmethod
    def of(cls, spots: GaussianSpots) -> "SpotMap":
        if not isinstance(spots, GaussianSpots):
            raise NotImplementedError(f"lights of type {type(spots).__name__}: " + GPE_CONTROL_SUPPORT)
        return cls(len(spots.spots), spots.free)

    @property
    def size(self) -> int:
        return 7 * self.n_spots

    def active(self) -> np.ndarray:
        """(S, 7) mask of the entries an optimiser may move"""
        row = np.array([self.free is None or n in self.free for n in SPOT_NUMBERS])
        return np.broadcast_to(row, (self.n_spots, 7)).copy()

    def flatten(self, spots: GaussianSpots) -> np.ndarray:
        if len(spots.spots) != self.n_spots:
            raise ValueError(f"{len(spots.spots)} spots, the map was built for {self.n_spots}")
        return np.array([[getattr(s, n) for n in SPOT_NUMBERS] for s in spots.spots], dtype=np.float64).reshape(-1)

    def build(self, p) -> GaussianSpots:
        p = np.asarray(p, dtype=np.float64)
        if p.shape != (self.size,):
            raise ValueError(f"flat spot vector of shape {p.shape}: {self.n_spots} spots have {self.size} numbers")
        return GaussianSpots([GaussianSpot(*(float(v) for v in row)) for row in p.reshape(self.n_spots, 7)], free=self.free)

    @staticmethod
    def user_gradient(spots: GaussianSpots, raw) -> np.ndarray:
        """the library's gradient block ``(..., S, 7)`` (last entry: d/d inv_two_w2) in user units (last entry: d/d width;
        inv_two_w2 = 1 / (2 w^2), so d inv_two_w2 / dw = -1 / w^3)"""
        g = np.array(raw, dtype=np.float64)
        w = np.array([s.width for s in spots.spots])
        g[..., 6] = g[..., 6] * (-1.0 / w**3)
        return g

    def weight_vector(self, w) -> np.ndarray:
        """regularisation weights of the flat vector: None (zeros), a number or an (S, 7) array"""
        if w is None:
            return np.zeros(self.size)
        return np.broadcast_to(np.asarray(w, dtype=np.float64), (self.n_spots, 7)).reshape(-1).copy()


ROTATING_GRADIENTS = ("control_gradient, optimize and train do not cover the rotating-frame GPE (GPE2DTSRot + "
                      "RotatingStrangSplitting): its gradients over k, e and omega and over the start state are "
                      "PDEModel.rotation_gradient, its optimisation over them PDEModel.optimize_rotation (the adjoint of the "
                      "alternating-direction split step, pde_opt_amd.gpe_control.RotControlSolver)")

ROTATION_GRADIENT_SUPPORT = ("rotation_gradient and optimize_rotation support GPE2DTSRot with RotatingStrangSplitting and "
                             "ConstantStepSize, without lights and with omega_rate = 0 (a frozen potential and a constant "
                             "Omega); the optimisation variables are a non-empty subset of k, e and omega; a stirred or ramped "
                             "equation has PDEModel.stirring_gradient and optimize_stirring")


def reject_rotating(equation_type, solver_type=None):
    """``NotImplementedError`` for any gradient of the rotating-frame GPE; needs no engine and no GPU"""
    if getattr(equation_type, "_rotating_frame", False) or getattr(solver_type, "integrator", None) == L.INT_STRANG_ROT:
        raise NotImplementedError(ROTATING_GRADIENTS)


def reject_unsupported(equation_type, solver_type, parameters=None, opt_names=None):
    """``NotImplementedError`` for what the GPE gradient does not cover; needs no engine and no GPU"""
    from .numerics.equations.gross_pitaevskii import GPE2DTSControl
    from .numerics.solvers import StrangSplitting

    reject_rotating(equation_type, solver_type)
    if equation_type is not GPE2DTSControl:
        raise NotImplementedError(f"{equation_type.__name__}: " + GPE_CONTROL_SUPPORT)
    if solver_type is not StrangSplitting:
        raise NotImplementedError(f"{solver_type.__name__}: " + GPE_CONTROL_SUPPORT)
    if opt_names is not None and set(opt_names) != {"lights"}:
        raise NotImplementedError(f"optimisation variables {sorted(opt_names)}: " + GPE_CONTROL_SUPPORT)
    if parameters is not None:
        if not isinstance(parameters.get("lights"), GaussianSpots):
            raise NotImplementedError(f"lights of type {type(parameters.get('lights')).__name__}: " + GPE_CONTROL_SUPPORT)
        if parameters.get("time_dependent") is False:
            raise NotImplementedError("time_dependent=False folds the spots into the potential: " + GPE_CONTROL_SUPPORT)


def _engine_setup(equation, solver, y0s, ts):
    """``(configure(engine), equations)`` for one equation shared by the batch ``y0s`` or a list with one per environment:
    ``configure`` sets the problem, the equations' numbers and tables and the solver up"""
    shared = not isinstance(equation, (list, tuple))
    eqs = [equation] if shared else list(equation)
    if not shared and len(eqs) != y0s.shape[0]:
        raise ValueError(f"{len(eqs)} equations for a batch of {y0s.shape[0]} states")
    t_first, t_last = float(ts[0]), float(ts[-1])

    def configure(eng):
        eng.configure(dtype=y0s.dtype, batch=y0s.shape[0], **eqs[0]._engine_problem())
        if shared:
            equation._engine_upload(eng, t_first, t_last)
        else:
            type(eqs[0])._engine_upload_batch(eng, eqs, t_first, t_last)
        solver.configure_engine(eng, eqs[0])

    return configure, eqs


class GpeControlSolver(StreamSolver):
    """One engine for the backward sweeps, bound to one torch stream (the stream rule of ``reverse.StreamSolver``)."""

    def __init__(self, device: int = 0):
        super().__init__(device, CHUNK_BYTES_ENV)

    def _sweep(self, configure, integrator, y0s, ts, dt0, cotangents, tails, adjoint_step):
        """The backward sweep the GPE adjoints share (``reverse.known_cotangent_sweep``): ``configure(engine)`` sets the
        problem up and ``adjoint_step(engine, t0, dt, psi0_ptr, lam_ptr, *block_ptrs)`` takes ``lam`` back one substep while
        it adds into the gradient blocks, one fp64 device block ``(B,) + tail`` per entry of ``tails`` (``None``: no such
        block, a null pointer).  Returns ``(blocks, lam0)``: the blocks in the order of ``tails`` (``None`` where the tail
        is) and ``dJ/dy0``, fp64 on the host."""
        eng = self.engine
        ts = np.asarray(ts, dtype=np.float64)
        steps, saves = schedule(ts, dt0)
        t_of = lambda i: float(ts[0]) + i * float(dt0)  # start time of substep i (integrate.diffeqsolve)
        with self._ordered(), self.torch.no_grad():
            configure(eng)
            eng.set_state(y0s)
            Y = eng.state_device_array().torch()
            blocks, lam0, self.last_chunks = known_cotangent_sweep(
                Y, len(steps), chunk_length(len(steps), Y.numel() * Y.element_size(), self._cap()), saves, cotangents, tails,
                lambda i: eng.advance(integrator, steps[i], 1, t_of(i)),
                lambda s, psi0, lam, *blocks: adjoint_step(eng, t_of(s), steps[s], psi0.data_ptr(), lam.data_ptr(),
                                                           *(0 if g is None else g.data_ptr() for g in blocks)))
            return [None if g is None else g.cpu().numpy() for g in blocks], lam0.double().cpu().numpy()

    def gradient(self, equation, solver, y0s, ts, dt0, cotangents):
        """``(grad (B, S, 7), lam0 (B, nx, ny, 2))`` for the cotangents ``dJ/dys`` ``(len(ts), B, nx, ny, 2)`` of the saved
        solution: ``grad`` is the library's block (per environment; last entry d/d inv_two_w2), ``lam0`` is ``dJ/dy0``.
        Both fp64 on the host; the sweep itself runs in the dtype of ``y0s``."""
        configure, _ = _engine_setup(equation, solver, y0s, ts)
        (grad,), lam0 = self._sweep(configure, solver.integrator, y0s, ts, dt0, cotangents, [(len(equation.lights.spots), 7)],
                                    lambda eng, t0, dt, psi0, lam, g: eng.gpe_adjoint_step(t0, dt, psi0, lam, g))
        return grad, lam0


ROT_NAMES = ("k", "e", "omega")  # the order of the library's gradient block (pdeopt_gpe_rot_adjoint_step)


def _reject_unsupported_rotating(support, allowed, equation_type, solver_type, opt_names, stepsize_controller):
    """what ``reject_unsupported_rotation`` and ``reject_unsupported_stirring`` share: the pair, the optimisation
    variables (a non-empty subset of ``allowed``) and the controller, each refused with ``support``"""
    from .numerics.solvers import ConstantStepSize, RotatingStrangSplitting

    if not getattr(equation_type, "_rotating_frame", False):
        raise NotImplementedError(f"{equation_type.__name__}: " + support)
    if solver_type is not RotatingStrangSplitting:
        raise NotImplementedError(f"{solver_type.__name__}: " + support)
    if opt_names is not None and (not set(opt_names) or not set(opt_names) <= set(allowed)):
        raise NotImplementedError(f"optimisation variables {sorted(opt_names)}: " + support)
    if stepsize_controller is not None and not isinstance(stepsize_controller, ConstantStepSize):
        raise NotImplementedError(f"{type(stepsize_controller).__name__}: " + support)


def reject_unsupported_rotation(equation_type, solver_type, opt_names=None, stepsize_controller=None, parameters=None):
    """``NotImplementedError`` for what the rotating-frame gradient does not cover; needs no engine and no GPU"""
    _reject_unsupported_rotating(ROTATION_GRADIENT_SUPPORT, ROT_NAMES, equation_type, solver_type, opt_names, stepsize_controller)
    if parameters is not None:
        if parameters.get("lights") is not None:
            raise NotImplementedError("an equation with lights: " + ROTATION_GRADIENT_SUPPORT)
        if parameters.get("omega_rate"):
            raise NotImplementedError(f"omega_rate={parameters['omega_rate']!r}: " + ROTATION_GRADIENT_SUPPORT)


class RotControlSolver(GpeControlSolver):
    """The backward sweeps of the rotating-frame GPE (``pdeopt_gpe_rot_adjoint_step``, csrc/gpe_rot_adjoint.hip): the
    stream rule, the schedule, the chunked recomputation and ``PDEOPT_GPE_ADJOINT_CHUNK_BYTES`` of
    ``GpeControlSolver``."""

    def gradient(self, equation, solver, y0s, ts, dt0, cotangents):
        """``(grad (B, 3), lam0 (B, nx, ny, 2))`` for the cotangents ``dJ/dys`` ``(len(ts), B, nx, ny, 2)`` of the saved
        solution: row b of ``grad`` is ``dJ/d(k, e, omega)`` of environment b, ``lam0`` is ``dJ/dy0``.  ``equation`` is
        one ``GPE2DTSRot`` shared by the batch or a list with one per environment (its own k, e, omega).  Both fp64 on
        the host; the sweep itself runs in the dtype of ``y0s``.  Constant steps only."""
        configure, _ = _engine_setup(equation, solver, y0s, ts)
        (grad,), lam0 = self._sweep(configure, solver.integrator, y0s, ts, dt0, cotangents, [(3,)],
                                    lambda eng, t0, dt, psi0, lam, g: eng.gpe_rot_adjoint_step(dt, psi0, lam, g))
        return grad, lam0


STIR_NAMES = ("k", "e", "omega", "omega_rate")  # the order of pdeopt_gpe_rot_stir_adjoint_step's gradient block

STIRRING_GRADIENT_SUPPORT = ("stirring_gradient and optimize_stirring support GPE2DTSRot with RotatingStrangSplitting and "
                             "ConstantStepSize; lights is None, a GaussianSpots (evaluated in-kernel, differentiated) or a "
                             "callable that does not depend on time (folded into the potential, not differentiated); the "
                             "optimisation variables are a non-empty subset of k, e, omega, omega_rate and lights (a "
                             "GaussianSpots)")


def reject_unsupported_stirring(equation_type, solver_type, opt_names=None, stepsize_controller=None, parameters=None,
                                opt_parameters=None):
    """``NotImplementedError`` for what the stirred rotating-frame gradient does not cover; needs no engine and no GPU"""
    _reject_unsupported_rotating(STIRRING_GRADIENT_SUPPORT, STIR_NAMES + ("lights",), equation_type, solver_type, opt_names,
                                 stepsize_controller)
    if opt_parameters is not None and "lights" in opt_parameters and not isinstance(opt_parameters["lights"], GaussianSpots):
        raise NotImplementedError(f"lights of type {type(opt_parameters['lights']).__name__} as an optimisation variable: "
                                  + STIRRING_GRADIENT_SUPPORT)
    lights = (parameters or {}).get("lights")
    if lights is not None and not isinstance(lights, GaussianSpots) and not callable(lights):
        raise NotImplementedError(f"lights of type {type(lights).__name__}: " + STIRRING_GRADIENT_SUPPORT)


def reject_time_dependent_lights(equation, t0, t1):
    """a callable ``lights`` of time that is no ``GaussianSpots`` has no gradient here (the forward solve raises
    ``ValueError`` for it; that stays): ``NotImplementedError`` before any engine work"""
    try:
        equation._lights_kind(float(t0), float(t1))
    except ValueError as e:
        raise NotImplementedError(f"{e} " + STIRRING_GRADIENT_SUPPORT) from None


class RotStirControlSolver(RotControlSolver):
    """The backward sweeps of the stirred, ramped rotating-frame GPE (``pdeopt_gpe_rot_stir_adjoint_step``,
    csrc/gpe_rot_adjoint.hip): ``GpeControlSolver._sweep`` with a second device block for the spots."""

    def gradient(self, equation, solver, y0s, ts, dt0, cotangents):
        """``(grad (B, 4), spot_grad (B, S, 7) or None, lam0 (B, nx, ny, 2))`` for the cotangents ``dJ/dys``
        ``(len(ts), B, nx, ny, 2)`` of the saved solution: row b of ``grad`` is ``dJ/d(k, e, omega, omega_rate)`` of
        environment b, ``spot_grad`` the library's block (last entry d/d inv_two_w2; ``None`` when no spots reach the
        kernels), ``lam0`` is ``dJ/dy0``.  ``equation`` is one ``GPE2DTSRot`` shared by the batch or a list with one per
        environment (its own k, e, omega, omega_rate and spots): spot tables travel padded to the largest count; where
        the counts differ the padding's rows are dropped and ``spot_grad`` is a list of ``(S_b, 7)`` arrays.  All fp64 on the host;
        the sweep itself runs in the dtype of ``y0s``.  Constant steps only."""
        configure, eqs = _engine_setup(equation, solver, y0s, ts)
        kinds = [e._lights_kind(float(ts[0]), float(ts[-1])) for e in eqs]
        counts = [len(e.lights.spots) for e in eqs] if all(k == "spots" for k in kinds) else None
        (grad, spot_grad), lam0 = self._sweep(
            configure, solver.integrator, y0s, ts, dt0, cotangents, [(4,), (max(counts), 7) if counts else None],
            lambda eng, t0, dt, psi0, lam, g, sg: eng.gpe_rot_stir_adjoint_step(t0, dt, psi0, lam, g, sg))
        if counts and len(set(counts)) > 1:  # drop the padding: zero-amplitude spots that stand for none
            spot_grad = [spot_grad[b, :n].copy() for b, n in enumerate(counts)]
        return grad, spot_grad, lam0
