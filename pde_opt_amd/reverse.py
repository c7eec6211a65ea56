"""What the reverse-mode (discrete adjoint) gradients share: the schedule of substeps and save points, the split of a
save point's cotangent, the chunked recomputation of the states a backward sweep needs, and the stream rule of the
solvers that run it (``fieldmu.FieldMuSolver``, ``gpe_control.GpeControlSolver`` and its subclasses).

A backward sweep needs the state every substep started from.  ``forward_pass`` keeps one state per chunk of substeps;
``backward_pass`` restores each chunk's start, runs the chunk again and holds it, and walks it backwards;
``known_cotangent_sweep`` is the two for cotangents that do not depend on the pass.  A chunk holds
at most the solver's cap in bytes (``StreamSolver._cap``), so a long solve costs one extra forward pass instead of
unbounded memory.  The two passes are plain functions of tensors: everything that touches a device pointer or a stream
is in the callbacks, so they run on CPU tensors as well (tests/test_reverse_cpu.py).

torch is imported when a solver is built, not with the package.
"""

from __future__ import annotations

import contextlib
import os

import numpy as np

from .fit import walk_save_points

DEFAULT_CHUNK_BYTES = 1 << 30


# ---- schedule ---------------------------------------------------------------------------------------------------------


def schedule(ts, dt0):
    """``(steps, saves)``: the step sizes of the substeps in order, and per save point ``(i, theta)``: the save is the
    state after ``i`` substeps (``theta`` None), or ``y[i - 1] + theta (y[i] - y[i - 1])`` inside substep ``i``"""
    ts = np.asarray(ts, dtype=np.float64)
    steps, saves = [], []
    walk_save_points(float(ts[0]), float(ts[-1]), float(dt0), ts,
                     lambda dt, n, t: steps.extend([float(dt)] * int(n)), lambda: None,
                     lambda q, theta: saves.append((len(steps), theta)))
    return steps, saves


def split_save_cotangent(g, theta):
    """cotangents ``(of y[i - 1], of y[i])`` of a save ``(1 - theta) y[i - 1] + theta y[i]`` with cotangent ``g``; a save on
    a step edge (``theta`` None) belongs to ``y[i]`` alone"""
    if theta is None:
        return None, g
    return (1.0 - theta) * g, theta * g


def add_save_cotangent(cot, i, theta, g):
    """add the cotangent ``g`` of the save ``(i, theta)`` to ``cot``, the cotangents of the states by substep index"""
    g_prev, g_cur = split_save_cotangent(g, theta)
    for k, g in ((i - 1, g_prev), (i, g_cur)):
        if g is not None:
            cot[k] = g if k not in cot else cot[k] + g


def chunk_length(n_steps: int, state_bytes: int, cap_bytes: int) -> int:
    """substeps per chunk: as many start states as ``cap_bytes`` holds, at least one"""
    return max(1, min(max(1, n_steps), int(cap_bytes) // max(1, int(state_bytes))))


# ---- the chunked recomputation ----------------------------------------------------------------------------------------


def forward_pass(Y, n_steps, chunk, step, visit=None):
    """Run the substeps forward in ``Y`` (``step(i)`` advances it in place from substep ``i``'s start to its end) and
    return ``{i: copy of Y}`` at the first substep ``i`` of every chunk.  Without ``visit`` the pass ends where the last
    chunk starts: ``backward_pass`` runs that chunk itself.  With it, ``visit(i)`` sees ``Y`` after ``i`` substeps, for
    every ``i`` up to ``n_steps``, before ``step(i)``: for a caller whose cotangents come from the states themselves."""
    stop = n_steps if visit is not None else (max(n_steps, 1) - 1) // chunk * chunk
    starts = {}
    for i in range(stop + 1):
        if visit is not None:
            visit(i)
        if i == n_steps:
            break
        if i % chunk == 0:
            starts[i] = Y.clone()
        if i < stop:
            step(i)
    return starts


def backward_pass(Y, starts, n_steps, chunk, step, adjoint, cot_at):
    """Walk the substeps backwards and return ``lam``, the cotangent of the initial state.  ``starts`` is what
    ``forward_pass`` returned (emptied here, chunk by chunk).  For every chunk, last first: restore its start into ``Y``,
    run it again with ``step`` and hold the start state of each of its substeps; then, from its last substep ``s`` to its
    first, ``adjoint(s, u_s, lam)`` takes ``lam`` in place from the cotangent of substep ``s``'s end state to that of its
    start state ``u_s`` (and adds whatever parameter gradients the caller keeps), and the save points' share
    ``cot_at(s)`` of that state is added: a tensor like ``Y``, or None.  ``cot_at(n_steps)`` starts ``lam`` and becomes
    it: it must be the caller's to give away.  Without a substep ``lam`` is ``cot_at(0)``."""
    g = cot_at(n_steps) if n_steps > 0 else None
    lam = g if g is not None else Y.new_zeros(Y.shape)
    for s0 in sorted(starts, reverse=True):
        s1 = min(n_steps, s0 + chunk)
        Y.copy_(starts.pop(s0))
        held = []
        for s in range(s0, s1):
            held.append(Y.clone())
            if s + 1 < s1:
                step(s)
        for s in range(s1 - 1, s0 - 1, -1):
            adjoint(s, held.pop(), lam)
            g = cot_at(s)
            if g is not None:
                lam += g
    if n_steps == 0:
        g = cot_at(0)
        if g is not None:
            lam += g
    return lam


def known_cotangent_sweep(Y, n_steps, chunk, saves, cotangents, tails, step, adjoint):
    """The two passes for a caller that knows the cotangents of its saves beforehand: ``cotangents[q]`` is a host array,
    the cotangent of save ``saves[q] = (i, theta)``.  The forward pass stops where the last chunk starts, a cotangent goes
    to ``Y``'s device and dtype when the sweep reaches its state, one at a time, and the one of the initial state is
    added too: ``lam0`` is ``dJ/dy0``.  ``adjoint(s, u_s, lam, *blocks)`` also adds into the gradient blocks, one fp64
    tensor ``(B,) + tail`` per entry of ``tails``, ``None`` where the tail is.  Returns ``(blocks, lam0, chunks)``; a
    sweep over no substep counts as one chunk."""
    import torch

    cot = {}
    for (i, theta), g in zip(saves, cotangents):
        add_save_cotangent(cot, i, theta, np.asarray(g, dtype=np.float64))
    starts = forward_pass(Y, n_steps, chunk, step)
    chunks = max(1, len(starts))
    blocks = [None if tail is None else Y.new_zeros((Y.shape[0],) + tuple(tail), dtype=torch.float64) for tail in tails]

    def cot_at(s):  # (copy: a tensor of its own also where Y lives on the host; a transfer to a device is one anyway)
        return torch.as_tensor(np.ascontiguousarray(cot[s])).to(device=Y.device, dtype=Y.dtype, copy=True) if s in cot else None

    lam0 = backward_pass(Y, starts, n_steps, chunk, step, lambda s, u, lam: adjoint(s, u, lam, *blocks), cot_at)
    return blocks, lam0, chunks


# ---- the stream rule --------------------------------------------------------------------------------------------------


class StreamSolver:
    """One engine bound to one torch stream, and the cap of a backward sweep's chunks.

    Stream rule.  The engine is bound to ``self.stream`` for its lifetime: torch's current stream at construction, or a
    stream of the solver's own when that is the legacy default stream (it has no handle the library could borrow).  All
    of the solver's torch work and every library launch of a call run on ``self.stream``, so nothing synchronises inside
    the substep loop.  Every call reads the caller's current stream anew: on entry ``self.stream`` waits for it (what
    the caller has enqueued -- an optimiser step on the parameters, a module it has just modified -- is finished before
    the solver reads it), on exit it waits for ``self.stream`` (what the solver wrote is ready for what the caller
    enqueues next).  Both are device-side waits (``Stream.wait_stream``), not host synchronisation."""

    def __init__(self, device: int, chunk_bytes_env: str, default_chunk_bytes: int = DEFAULT_CHUNK_BYTES):
        import torch

        from .engine import HipEngine

        self.torch = torch
        self.device = torch.device("cuda", int(device))
        cur = torch.cuda.current_stream(self.device)
        self.stream = cur if cur.cuda_stream else torch.cuda.Stream(self.device)
        self.engine = HipEngine(int(device), stream=self.stream.cuda_stream)
        self._chunk_bytes_env, self._default_chunk_bytes = chunk_bytes_env, int(default_chunk_bytes)
        self.chunk_bytes = None  # None: the environment variable, else the default
        self.last_chunks = 0     # chunks of the last backward sweep

    @contextlib.contextmanager
    def _ordered(self):
        """run the body on ``self.stream``, ordered after and before the caller's current stream (the stream rule)"""
        torch = self.torch
        caller = torch.cuda.current_stream(self.device)
        if caller != self.stream:
            self.stream.wait_stream(caller)
        try:
            with torch.cuda.stream(self.stream):
                yield
        finally:
            if caller != self.stream:
                caller.wait_stream(self.stream)

    def _cap(self) -> int:
        if self.chunk_bytes is not None:
            return int(self.chunk_bytes)
        return int(os.environ.get(self._chunk_bytes_env, self._default_chunk_bytes))
