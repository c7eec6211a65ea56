"""The shell-averaged structure factor S(k) of a real periodic field and the coarsening length taken from it.

The device transforms the resident state and sums ``w |u^|^2`` over shells of width ``dk`` (``pdeopt_structure_factor``,
csrc/structure_factor.hip).  On a ``Domain`` with ``points = (n_0, .., n_{d-1})``, box lengths
``L_a`` and ``N = prod(n_a)`` cells

    dk     = max_a(2 pi / L_a)                                   the shell width
    t_a[i] = (2 pi fftfreq(n_a, L_a / n_a)[i] / dk)^2            the axis tables, fp64, built here and uploaded
    u^     = rfftn(u), unnormalised, the last axis halved: m = 0 .. n_last / 2
    b      = (int)floor(sqrt(q) + 0.5),  q = t_0[i] + t_1[m]  or  (t_0[i] + t_1[j]) + t_2[m]
    w      = 1 for m = 0 and, n_last even, m = n_last / 2, else 2;  0 for the zero mode (the mean drops out)
    P_b    = sum over shell b of w |u^|^2                        what comes back: n_bins doubles per environment

and the host, from the same tables, derives ``counts_b = sum w`` (they add up to ``N - 1``), ``S_b = P_b / (counts_b N)``
(0 for an empty shell), ``k_b = b dk``, ``variance = sum_b P_b / N^2`` (Parseval: the variance of ``u``),
``k1 = sum k S / sum S``, ``k2 = sqrt(sum k^2 S / sum S)`` and ``length = 2 pi / k1``.

Covered: ``CahnHilliard2DPeriodic``, ``AllenCahn2DPeriodic`` and ``CahnHilliard3DPeriodic`` with any ``derivs`` and any
``mu``: S(k) depends on the state and the domain only.
"""

from __future__ import annotations

import dataclasses
from typing import Tuple

import numpy as np

from . import _lib as L
from . import diagnostics as D
from . import fit

REWARD_NAMES = ("length", "k1", "k2", "variance")
MAX_BINS = 4096  # the four waves' shell arrays of the binning kernel fit in LDS up to here

SUPPORT = ("the structure factor is that of the real periodic phase-field classes CahnHilliard2DPeriodic, AllenCahn2DPeriodic "
           "and CahnHilliard3DPeriodic")


@dataclasses.dataclass(frozen=True)
class ShellTables:
    """``shell_tables(domain)``: the axis ``tables`` and ``n_bins`` the device takes, and what the host derives from the
    same tables: the shell width ``dk``, ``k_b = b dk``, the weighted mode ``counts`` per shell and the cells ``n``"""

    tables: Tuple[np.ndarray, ...]
    n_bins: int
    dk: float
    k: np.ndarray
    counts: np.ndarray
    n: int
    key: tuple


_TABLES: dict = {}


def shell_tables(domain) -> ShellTables:
    """the shells of ``domain`` (kept per grid: the counts walk the whole half spectrum once)"""
    points = tuple(int(n) for n in domain.points)
    lengths = tuple(float(v) for v in domain.L)
    key = ("sk", points, lengths)
    hit = _TABLES.get(key)
    if hit is not None:
        return hit
    if len(points) not in (2, 3) or min(points) < 2:
        raise ValueError(f"the structure factor needs a 2-D or 3-D grid with at least 2 points along every axis, got {points}")
    dk = max(2.0 * np.pi / v for v in lengths)
    tables = tuple((2.0 * np.pi * np.fft.fftfreq(n, v / n) / dk) ** 2 for n, v in zip(points, lengths))
    qmax = tables[0].max()
    for t in tables[1:]:
        qmax = qmax + t.max()
    n_bins = 1 + int(np.floor(np.sqrt(qmax) + 0.5))
    if n_bins > MAX_BINS:
        raise ValueError(f"{n_bins} shells on the grid {points}: the binning kernel holds at most {MAX_BINS}")
    n_last = points[-1]
    nh = n_last // 2 + 1
    q = tables[0]
    for t in tables[1:-1]:
        q = q[..., None] + t
    q = q[..., None] + tables[-1][:nh]
    b = np.floor(np.sqrt(q) + 0.5).astype(np.int64)
    w = np.full(nh, 2.0)
    w[0] = 1.0
    if n_last % 2 == 0:
        w[-1] = 1.0
    w = np.broadcast_to(w, b.shape).copy()
    w[(0,) * len(points)] = 0.0
    counts = np.bincount(b.ravel(), weights=w.ravel(), minlength=n_bins)
    out = ShellTables(tables=tables, n_bins=n_bins, dk=float(dk), k=np.arange(n_bins) * dk, counts=counts,
                      n=int(np.prod(points)), key=key)
    _TABLES[key] = out
    return out


@dataclasses.dataclass
class StructureFactor:
    """``k``, ``counts`` of shape ``(n_bins,)``; ``power`` (the device's ``P_b``) and ``s`` with a leading ``(B,)`` from
    ``structure_factor`` or ``(len(ts), B)`` from ``structure_factor_trace``; ``variance``, ``k1``, ``k2``, ``length`` of
    that leading shape; ``dk`` the shell width"""

    k: np.ndarray
    counts: np.ndarray
    power: np.ndarray
    s: np.ndarray
    variance: np.ndarray
    k1: np.ndarray
    k2: np.ndarray
    length: np.ndarray
    dk: float

    @classmethod
    def from_power(cls, power, k, counts, n: int, dk: float) -> "StructureFactor":
        """``power``: ``(..., n_bins)`` rows of ``HipEngine.structure_factor``; ``k``, ``counts``, ``n``, ``dk`` of
        ``shell_tables``"""
        power = np.asarray(power, dtype=np.float64)
        k = np.asarray(k, dtype=np.float64)
        counts = np.asarray(counts, dtype=np.float64)
        if power.ndim < 2 or power.shape[-1] != len(k) or counts.shape != k.shape:
            raise ValueError(f"shell sums have shape (..., {len(k)}), got {power.shape} (counts {counts.shape})")
        s = np.where(counts > 0, power / (np.where(counts > 0, counts, 1.0) * n), 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            total = s.sum(axis=-1)
            k1 = (k * s).sum(axis=-1) / total
            k2 = np.sqrt((k * k * s).sum(axis=-1) / total)
            length = 2.0 * np.pi / k1
        return cls(k=k, counts=counts, power=power, s=s, variance=power.sum(axis=-1) / float(n) ** 2, k1=k1, k2=k2,
                   length=length, dk=float(dk))

    def __getitem__(self, name: str) -> np.ndarray:
        if name not in REWARD_NAMES:
            raise KeyError(name)
        return getattr(self, name)


# ---- refusals: all of them need neither an engine nor a GPU -----------------------------------------------------------

def _equation_code(equation_type) -> int:
    from .numerics.equations.phase_field import AllenCahn2DPeriodic, CahnHilliard2DPeriodic, CahnHilliard3DPeriodic

    codes = {CahnHilliard2DPeriodic: L.EQ_CAHN_HILLIARD, AllenCahn2DPeriodic: L.EQ_ALLEN_CAHN, CahnHilliard3DPeriodic: L.EQ_CAHN_HILLIARD_3D}
    if equation_type not in codes:
        raise NotImplementedError(f"{getattr(equation_type, '__name__', equation_type)} has no structure factor here: " + SUPPORT +
                                  " (the smoothed-boundary, Butler-Volmer, advection-diffusion and GPE classes are not covered)")
    return codes[equation_type]


def reject_unsupported(equation_type) -> None:
    """the three periodic phase-field classes have this structure factor: say so before an engine exists"""
    _equation_code(equation_type)


def _states(model, state) -> np.ndarray:
    return D.batch_states(model, state, complex_message="the structure factor is that of a real field, got a complex state",
                          contiguous=True)[0]


def from_engine(eng, tabs: ShellTables, rows=None) -> StructureFactor:
    """the resident state's structure factor (``rows``: shell sums already fetched, any leading shape)"""
    power = eng.structure_factor() if rows is None else rows
    return StructureFactor.from_power(power, tabs.k, tabs.counts, tabs.n, tabs.dk)


def upload_tables(eng, tabs: ShellTables) -> None:
    """once per engine and grid: the engine keeps them until its grid changes"""
    eng.sk_configure(tabs.tables, tabs.n_bins, key=tabs.key)


# ---- PDEModel.structure_factor / structure_factor_trace ---------------------------------------------------------------

def structure_factor(model, state) -> StructureFactor:
    """``PDEModel.structure_factor``"""
    code = _equation_code(model.equation_type)
    tabs = shell_tables(model.domain)
    yb = _states(model, state)
    eng = D.engine_of(model)
    n, h = tuple(model.domain.points), tuple(model.domain.dx)
    extra = dict(nz=n[2], hz=h[2]) if len(n) == 3 else {}
    eng.configure(equation=code, dtype=yb.dtype, nx=n[0], ny=n[1], batch=yb.shape[0], hx=h[0], hy=h[1], **extra)
    eng.set_state(yb)
    upload_tables(eng, tabs)
    return from_engine(eng, tabs)


def structure_factor_trace(model, parameters, y0, ts, solver_parameters=None, dt0=1e-6) -> StructureFactor:
    """``PDEModel.structure_factor_trace``"""
    reject_unsupported(model.equation_type)

    def states(y):
        shell_tables(model.domain)  # the grid is looked at before the state
        return _states(model, y)

    rows = D.trace_on_step_edges(
        model, parameters, y0, ts, solver_parameters, dt0, name="structure_factor_trace",
        why="the spectrum of a linear interpolation of states is not the state's at that time", states=states,
        equation=lambda yb: model.equation_type(domain=model.domain, **fit.plain(parameters)), equation_first=False,
        prepare=lambda eng: upload_tables(eng, shell_tables(model.domain)),
        read=lambda eng: eng.structure_factor())  # n_bins * 8 bytes per environment come back
    return from_engine(None, shell_tables(model.domain), rows)


def _reward(env, eng, eqs, eq0):
    """``("structure_factor", name)``: the coarsening length, a moment of S(k) or the variance of the state after the
    step, transformed and binned on the device (n_bins * 8 bytes per environment come back); the shell tables travel
    once per shard engine"""
    tabs = shell_tables(env.domain)
    upload_tables(eng, tabs)
    return from_engine(eng, tabs)[env.device_reward[1]]


DEVICE_REWARD = D.DeviceReward(REWARD_NAMES, reject_unsupported, _reward)
