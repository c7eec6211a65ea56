"""Cahn-Hilliard with a neural-network chemical potential: the forward solve and the reverse-mode (discrete adjoint)
gradient of ``mean(r^2)`` over the network's parameters (the reference's ``train(method="mse")`` with a periodic CNN as
``mu``: docs/notebooks/optimization_neural_network.ipynb, notebooks/optimize_nn_script.py; it differentiates the solve
with diffrax's ``RecursiveCheckpointAdjoint``, pde_model.py:429-460).

The split: the network ``N`` and its vector-Jacobian products belong to torch on the device; the stencil, its transpose
and the IMEX operator are HIP kernels (csrc/fieldmu.hip).  Per substep torch evaluates ``mu_h = N(u)`` and the library
advances ``u += dt S f(u, mu_h)`` (``pdeopt_fieldmu_step``).  Going back, the library turns the cotangent ``lam`` of the
new state into ``lam += g_u`` and the cotangent ``g_mu`` of ``mu_h`` (``pdeopt_fieldmu_adjoint_step``), and
``mu_h.backward(g_mu)`` adds the network's share to ``lam`` and to the parameters' ``.grad``.  The cost does not depend
on the number of parameters.  The engine and the solver's torch work share one stream, so nothing synchronises inside
the substep loop; the caller's own stream is ordered against it on entry and exit of every call (``FieldMuSolver``).

Substep and save-point schedule: ``fit.walk_save_points``, the one of ``integrate.diffeqsolve`` and of the forward-mode
sensitivities (constant steps, a clipped last step, save points inside a step interpolated linearly).  The backward
sweep needs the state at the start of every substep: the schedule, the split of a save point's cotangent, the chunked
recomputation and the stream rule are those of ``pde_opt_amd.reverse``, which the GPE's gradients share.  The residuals
and with them the cotangents come from the states of the forward pass, so that pass runs to the last substep and visits
every state; ``dJ/dy0`` has no use here and is not formed.  A chunk holds at most ``PDEOPT_FIELDMU_CHUNK_BYTES``
(default 1 GiB; ``FieldMuSolver.chunk_bytes`` overrides it).

Covered: ``CahnHilliard2DPeriodic`` with ``derivs="fd"``, ``SemiImplicitFourierSpectral`` or ``Euler`` with
``ConstantStepSize``, fp32 and fp64, ``D`` a closure of the in-kernel family, ``kappa`` fixed.

Joint training of ``D``.  With ``D`` a ``DiffusionLegendrePolynomials``, ``mse_backward(..., coef_grad=True)`` also returns
the gradient over its coefficients (the reference's ``train`` with ``init_params = {"mu": model, "D": ...}``: both are
leaves of one pytree there).  The adjoint kernel already forms the cotangent ``g_D`` of ``D`` at every cell; a variant of
it (``pdeopt_fieldmu_adjoint_step_coef``) also sums ``g_D(o) dD/dcoef_k(u(o))`` over the cells in fp64, one partial sum
per workgroup and coefficient, added to a slot that workgroup alone owns; the slots are summed in a fixed order when the
gradient is read (``pdeopt_fieldmu_coef_grad_read``).  No extra forward pass, no tangent fields, no launch more per
substep, no atomics: the bits do not depend on the run or on the chunking, and the cost does not depend on the network.
``PDEModel.mse_backward(..., closure_grads={})`` and ``PDEModel.train`` with ``opt_parameters = {"mu": module, "D":
DiffusionLegendrePolynomials}`` build on it.  ``kappa`` stays fixed: it would move the implicit operator of the IMEX step.

``FieldMuSolver.native_cnn`` (off by default; ``PDEOPT_FIELDMU_NATIVE_CNN=1`` sets the default) moves the network into
the library as well: a ``PeriodicCNN`` of the family ``numerics.functions.cnn.native_spec`` accepts is evaluated by
``pdeopt_cnn_forward`` and differentiated by ``pdeopt_cnn_vjp`` (csrc/cnn.hip), no autograd graph is built, and the
parameter gradient accumulates in fp64 on the device over the sweep and is read once.  A module outside that family is
refused while the switch is on; there is no fallback to torch.

``FieldMuSolver.native_mixer`` (off by default; ``PDEOPT_FIELDMU_NATIVE_MIXER=1`` sets the default) is the same switch for
a ``Mixer2d`` of the family ``numerics.functions.mixer.native_spec`` accepts (``pdeopt_mixer_forward``,
``pdeopt_mixer_vjp``, csrc/mixer.hip).  ``native_cnn`` is asked first: with both on, a module that is not a
``PeriodicCNN`` is refused.

torch is imported when a solver is built, not with the package.
"""

from __future__ import annotations

import os

import numpy as np

from . import _lib as L
from .numerics.closures import is_torch_module as is_module  # noqa: F401  (the detection, for callers of this module)
from .numerics.equations.phase_field import FIELD_MU_SUPPORT
from .reverse import StreamSolver, add_save_cotangent, backward_pass, chunk_length, forward_pass, schedule
from .reverse import split_save_cotangent  # noqa: F401  (with schedule and chunk_length: callers and tests import them from here)

CHUNK_BYTES_ENV = "PDEOPT_FIELDMU_CHUNK_BYTES"
NATIVE_CNN_ENV = "PDEOPT_FIELDMU_NATIVE_CNN"
NATIVE_MIXER_ENV = "PDEOPT_FIELDMU_NATIVE_MIXER"


# ---- parameters as one flat vector --------------------------------------------------------------------------------------


def flatten_params(module) -> np.ndarray:
    """the module's parameters, in ``module.parameters()`` order, as one fp64 vector"""
    parts = [p.detach().double().reshape(-1).cpu().numpy() for p in module.parameters()]
    return np.concatenate(parts) if parts else np.zeros(0)


def flatten_grads(module) -> np.ndarray:
    """the parameters' ``.grad`` in the same order (zeros where a parameter has none)"""
    parts = [(p.grad if p.grad is not None else p.new_zeros(p.shape)).detach().double().reshape(-1).cpu().numpy()
             for p in module.parameters()]
    return np.concatenate(parts) if parts else np.zeros(0)


def unflatten_params(module, p) -> None:
    """write the flat vector back into the module's parameters (their dtype and device)"""
    import torch

    p = np.asarray(p, dtype=np.float64)
    n = sum(q.numel() for q in module.parameters())
    if p.shape != (n,):
        raise ValueError(f"flat parameter vector of shape {p.shape}: the module has {n} parameters")
    o = 0
    with torch.no_grad():
        for q in module.parameters():
            q.copy_(torch.as_tensor(p[o:o + q.numel()]).reshape(q.shape))
            o += q.numel()


def add_flat_grad(module, g) -> None:
    """add the flat vector ``g`` to the parameters' ``.grad``"""
    import torch

    o = 0
    for q in module.parameters():
        part = torch.as_tensor(np.asarray(g[o:o + q.numel()], dtype=np.float64)).reshape(q.shape).to(device=q.device, dtype=q.dtype)
        q.grad = part if q.grad is None else q.grad + part
        o += q.numel()


def weight_vector(module, w) -> np.ndarray:
    """regularisation weights of the flat vector: ``w`` is None (zeros), a number, a flat array, or a module of the same
    structure whose parameters are the weights"""
    n = sum(q.numel() for q in module.parameters())
    if w is None:
        return np.zeros(n)
    w = flatten_params(w) if is_module(w) else np.asarray(w, dtype=np.float64)
    return np.broadcast_to(w, (n,)).copy()


# ---- the solver ---------------------------------------------------------------------------------------------------------


def _reject(equation, solver, controller=None):
    from .numerics.solvers import ConstantStepSize

    if getattr(equation, "_mu_module", None) is None:
        raise NotImplementedError("a torch.nn.Module as mu is supported for " + FIELD_MU_SUPPORT)
    if equation.derivs != "fd":
        raise NotImplementedError(f'a torch.nn.Module as mu needs derivs="fd", not {equation.derivs!r}: ' + FIELD_MU_SUPPORT)
    if solver.integrator not in (L.INT_IMEX, L.INT_EULER):
        raise NotImplementedError(f"a torch.nn.Module as mu does not run with {type(solver).__name__}: " + FIELD_MU_SUPPORT)
    if controller is not None and not isinstance(controller, ConstantStepSize):
        raise NotImplementedError("a torch.nn.Module as mu needs ConstantStepSize: " + FIELD_MU_SUPPORT)
    if solver.integrator == L.INT_IMEX and np.any(np.imag(np.asarray(solver.fourier_symbol)) != 0.0):
        raise NotImplementedError("the adjoint of the IMEX step reuses its operator, which needs a real fourier_symbol")


class FieldMuSolver(StreamSolver):
    """One engine for solves whose ``mu`` is a ``torch.nn.Module``, on one torch stream (the stream rule of
    ``reverse.StreamSolver``: the ``.grad`` a call wrote is ready for what the caller enqueues next)."""

    def __init__(self, device: int = 0):
        super().__init__(device, CHUNK_BYTES_ENV)
        # evaluate and differentiate a PeriodicCNN mu in the library (csrc/cnn.hip) instead of in torch
        self.native_cnn = os.environ.get(NATIVE_CNN_ENV, "0") not in ("", "0")
        self._cnn = None  # the library's handle of the last native network
        # the same for a Mixer2d mu (csrc/mixer.hip)
        self.native_mixer = os.environ.get(NATIVE_MIXER_ENV, "0") not in ("", "0")
        self._mixer = None
        self._coef_pending = False  # the engine's coefficient-gradient slots hold sums of a sweep that did not finish

    # -- set-up ---------------------------------------------------------------------------------------------------------
    def _prepare(self, equation, solver, y0s, t0, t1):
        """configure the engine, upload the state; returns ``(Y, mu_of)``: the state as a tensor ``(B, nx, ny)`` over the
        engine's own buffer, and ``mu_of(u) -> mu_h`` ``(B, nx, ny)``, contiguous.  With ``native_cnn`` or ``native_mixer`` the
        library evaluates the network: ``mu_of`` fills and returns one buffer, and ``self._net()`` holds this call's
        parameters"""
        torch = self.torch
        eng = self.engine
        eng.configure(dtype=y0s.dtype, batch=y0s.shape[0], **equation._engine_problem(field_mu=True))
        equation._engine_upload(eng, t0, t1)
        solver.configure_engine(eng, equation)
        eng.set_state(y0s)
        Y = eng.state_device_array().torch()
        module = equation._mu_module
        for name, p in module.named_parameters():
            if p.dtype != Y.dtype or p.device != Y.device:
                raise ValueError(f"mu's parameter {name} is {p.dtype} on {p.device}; the solve runs in {Y.dtype} on {Y.device}")
        if self.native_cnn or self.native_mixer:
            net = self._native(module)
            mu_h = torch.empty_like(Y)

            def native_mu(u):
                net.forward(u.data_ptr(), mu_h.data_ptr())
                return mu_h

            return Y, native_mu
        call = as_field_call(module, Y)
        return Y, lambda u: call(u).reshape(u.shape).contiguous()

    def _net(self):
        """the library's handle of the network it evaluates and differentiates, or None: torch does"""
        if self.native_cnn:
            return self._cnn
        return self._mixer if self.native_mixer else None

    def _native(self, module):
        """the library's handle of ``module`` with its current parameters uploaded; refuses what csrc/cnn.hip (``native_cnn``,
        asked first) or csrc/mixer.hip (``native_mixer``) does not cover, and a mixer made for another grid than the engine's"""
        if self.native_cnn:
            from .numerics.functions import cnn as C

            self._cnn = self._handle(module, self._cnn, C, "native_cnn",
                                     lambda spec: (spec[0], C.NATIVE_ACTIVATIONS.index(spec[1])),
                                     lambda net: (net.channels, net.activation), self.engine.cnn)
            return self._cnn
        from .numerics.functions import mixer as M

        def make(grid, sizes, act):
            if grid != (self.engine.problem.nx, self.engine.problem.ny):
                raise ValueError(f"mu is a Mixer2d for a {grid[0]} x {grid[1]} grid; the solve runs on "
                                 f"{self.engine.problem.nx} x {self.engine.problem.ny}")
            return self.engine.mixer(*sizes, act)

        self._mixer = self._handle(module, self._mixer, M, "native_mixer",
                                   lambda spec: (spec[0], spec[1:6], M.NATIVE_ACTIVATIONS.index(spec[6])),
                                   lambda net: (net.grid, net.sizes, net.activation), make)
        return self._mixer

    @staticmethod
    def _handle(module, held, family, switch, key_of_spec, key_of_handle, make):
        """``held`` if it is a handle of ``module``'s structure, else a new one from ``make(*key)`` in its place (``held`` is
        closed once the new one exists: a ``make`` that refuses leaves it as it was); the parameters are uploaded either
        way.  ``family`` is the module of ``numerics.functions`` that says what the library covers"""
        spec = family.native_spec(module)
        if spec is None:
            raise NotImplementedError(f"{switch} is on and mu is not a network the library evaluates: {family.native_refusal(module)} "
                                      f"(there is no fallback to torch: set {switch} = False)")
        key = key_of_spec(spec)
        if held is None or key_of_handle(held) != key:
            new = make(*key)
            if held is not None:
                held.close()
            held = new
        held.set_params(flatten_params(module))
        return held

    # -- forward --------------------------------------------------------------------------------------------------------
    def solve(self, equation, solver, y0s, ts, dt0, controller=None) -> np.ndarray:
        """the saved states ``(len(ts), B, nx, ny)`` in the dtype of ``y0s``"""
        _reject(equation, solver, controller)
        torch = self.torch
        steps, saves = schedule(ts, dt0)
        need_prev = {i - 1 for i, theta in saves if theta is not None}
        by_index = {}
        for q, (i, theta) in enumerate(saves):
            by_index.setdefault(i, []).append((q, theta))
        out = [None] * len(saves)
        with self._ordered(), torch.no_grad():
            Y, mu_of = self._prepare(equation, solver, y0s, float(ts[0]), float(ts[-1]))
            prev = None
            for i in range(len(steps) + 1):
                for q, theta in by_index.get(i, ()):
                    out[q] = Y.clone() if theta is None else prev + theta * (Y - prev)
                if i == len(steps):
                    break
                if i in need_prev:
                    prev = Y.clone()
                self.engine.fieldmu_step(solver.integrator, steps[i], mu_of(Y).data_ptr())
            res = torch.stack(out).cpu().numpy()
        return res

    # -- reverse ----------------------------------------------------------------------------------------------------------
    def mse_backward(self, equation, solver, y0s, values, ts, dt0, coef_grad: bool = False):
        """``mean(r^2)`` of ``r = values - solve(...)[1:]`` (``values`` ``(B, T - 1, nx, ny)``), summed in fp64; the
        gradient is ADDED to ``.grad`` of the module's parameters.  With ``coef_grad`` the return value is ``(loss,
        grad_D)``: ``grad_D`` is the gradient over the coefficients of ``equation.D``, a ``DiffusionLegendrePolynomials``, as
        an fp64 array in the order of ``D.expansion.params``"""
        _reject(equation, solver)
        if coef_grad:
            from .numerics.functions.legendre import DiffusionLegendrePolynomials

            if not isinstance(equation.D, DiffusionLegendrePolynomials):
                raise NotImplementedError(f"coef_grad differentiates over the coefficients of a DiffusionLegendrePolynomials as D, "
                                          f"not {type(equation.D).__name__}")
            n_coef = len(equation.D.expansion.params)
        adjoint_step = self.engine.fieldmu_adjoint_step_coef if coef_grad else self.engine.fieldmu_adjoint_step
        torch = self.torch
        integ = solver.integrator
        steps, saves = schedule(ts, dt0)
        N = len(steps)
        need_prev = {i - 1 for i, theta in saves if theta is not None}
        by_index = {}
        for q, (i, theta) in enumerate(saves):
            if q >= 1:  # ts[0] is the initial state: data
                by_index.setdefault(i, []).append((q, theta))
        with self._ordered(), torch.no_grad(), _deterministic(torch):
            Y, mu_of = self._prepare(equation, solver, y0s, float(ts[0]), float(ts[-1]))
            net = self._net()
            if net is not None and net.pending:
                net.grad_read(reset=True)
            if coef_grad:  # (a configure zeroes the slots too; this does not rely on _prepare being one)
                if self._coef_pending:
                    self.engine.fieldmu_coef_grad_read(n_coef, reset=True)
                self._coef_pending = True
            vals = torch.as_tensor(np.ascontiguousarray(np.swapaxes(values, 0, 1)), dtype=Y.dtype).to(Y.device)  # (T - 1, B, ...)
            M = vals.numel()
            chunk = chunk_length(N, Y.numel() * Y.element_size(), self._cap())
            cot = {}
            ssr = torch.zeros((), dtype=torch.float64, device=Y.device)
            prev = None

            def step(i):
                self.engine.fieldmu_step(integ, steps[i], mu_of(Y).data_ptr())

            def residuals(i):
                """the residuals of the saves on state ``i`` and their cotangents; the state an interpolated save needs"""
                nonlocal ssr, prev
                for q, theta in by_index.get(i, ()):
                    pred = Y if theta is None else prev + theta * (Y - prev)
                    r = vals[q - 1] - pred
                    ssr += (r.double() ** 2).sum()
                    add_save_cotangent(cot, i, theta, r * (-2.0 / M))  # d mean(r^2) / d pred
                if i in need_prev:
                    prev = Y.clone()

            def adjoint(s, u, lam):
                """the library's share of the substep, then the network's"""
                if net is not None:
                    adjoint_step(integ, steps[s], u.data_ptr(), mu_of(u).data_ptr(), lam.data_ptr(), gmu.data_ptr())
                    net.vjp(u.data_ptr(), gmu.data_ptr(), lam.data_ptr())
                    return
                u.requires_grad_(True)
                with torch.enable_grad():
                    mu = mu_of(u)
                adjoint_step(integ, steps[s], u.data_ptr(), mu.data_ptr(), lam.data_ptr(), gmu.data_ptr())
                mu.backward(gmu)
                lam += u.grad

            starts = forward_pass(Y, N, chunk, step, visit=residuals)
            gmu = torch.empty_like(Y)
            self.last_chunks = len(starts)
            backward_pass(Y, starts, N, chunk, step, adjoint, lambda s: cot.get(s) if s > 0 else None)  # dJ/dy0 has no use
            loss = float(ssr.item()) / M
            if net is not None:
                add_flat_grad(equation._mu_module, net.grad_read(reset=True))
            if coef_grad:
                grad_D = self.engine.fieldmu_coef_grad_read(n_coef, reset=True)
                self._coef_pending = False
        return (loss, grad_D) if coef_grad else loss


class _deterministic:
    """torch's deterministic convolution algorithms for the duration (identical bits on a repeat), then as before"""

    def __init__(self, torch):
        self.b = torch.backends.cudnn

    def __enter__(self):
        self.saved = (self.b.deterministic, self.b.benchmark)
        self.b.deterministic, self.b.benchmark = True, False

    def __exit__(self, *exc):
        self.b.deterministic, self.b.benchmark = self.saved


def as_field_call(module, like):
    """``call(u (B, nx, ny)) -> mu_h`` with ``B nx ny`` entries: the module applied to ``(B, 1, nx, ny)``, or -- a module
    written for one field ``(nx, ny)`` -- to every trajectory in turn.  Decided by one trial call on a constant field shaped like ``like``."""
    import torch

    B, nx, ny = like.shape
    probe = torch.full((B, 1, nx, ny), 0.5, dtype=like.dtype, device=like.device)
    want = "mu must map a (B, 1, nx, ny) tensor (or one (nx, ny) field) to the same shape"
    with torch.no_grad():
        try:
            batched = tuple(module(probe).shape)
        except Exception as e:  # a module written for one field may fail in any way on four axes: kept for the message
            batched = e
        if batched == (B, 1, nx, ny):
            return lambda u: module(u[:, None])
        first = (f"the batched call raised {type(batched).__name__}: {batched}" if isinstance(batched, Exception)
                 else f"the batched call returned shape {batched}")
        try:
            single = tuple(module(probe[0, 0]).shape)
        except Exception as e:
            raise ValueError(f"{want}; {first}; the call on one field raised {type(e).__name__}: {e}") from e
    if single != (nx, ny):
        raise ValueError(f"{want}; {first}; the call on one field returned shape {single}")
    return lambda u: torch.stack([module(u[b]) for b in range(u.shape[0])])
