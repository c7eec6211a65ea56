"""Cahn-Hilliard and Allen-Cahn equations with periodic boundaries, 2-D, on the HIP engine.

Same dataclass surface as the reference (pde_opt/numerics/equations/cahn_hilliard.py:31-109,
allen_cahn.py:27-84): fields ``domain, kappa, mu, D|R, derivs``; published attributes
``kx, ky, two_pi_i_kx, ..., two_pi_i_k_2, fft, ifft`` (+ ``two_pi_i_k_4, fourier_symbol`` for CH);
``rhs(state, t)``.  ``mu`` / ``D`` / ``R`` may be any callable the closure tracer understands
(numerics/closures.py), a Legendre closure object, a number, or a ``ClosureDesc``.

``rhs`` runs on the GPU: the fused stencil kernels (csrc/stencil_*.hpp) for ``derivs="fd"``, batched
rocFFT transforms + pointwise kernels (csrc/spectral.hip) for ``derivs="fourier"``.
"""

from __future__ import annotations

import dataclasses
from typing import Any

import numpy as np

from ... import _lib as L
from ..closures import UnsupportedClosureError, as_closure, is_torch_module
from ..domains import Domain
from .base_eq import BaseEquation


_SPECTRAL_NAMES = ("kx", "ky", "two_pi_i_kx", "two_pi_i_ky", "two_pi_i_kx_2", "two_pi_i_ky_2",
                   "two_pi_i_k_2", "two_pi_i_k_4")
_spectral_cache: dict = {}
_table_serial = iter(range(1, 1 << 62))  # identity of a table in upload keys (id() may be reused after eviction)


def spectral_table(domain) -> dict:
    """Wave-number meshes shared by CH, AC and the GPE (cahn_hilliard.py:65-73, allen_cahn.py:58-65),
    built once per (points, box) and shared by every equation object on that grid: PDEEnv.step
    constructs a new equation per step (pde_env.py:286) and must not pay for 1024^2 meshes each time."""
    key = (tuple(domain.points), tuple(tuple(b) for b in domain.box))
    tab = _spectral_cache.get(key)
    if tab is None:
        kx, ky = domain.fft_mesh()
        ikx, iky = 2j * np.pi * kx, 2j * np.pi * ky
        k2 = ikx**2 + iky**2
        tab = dict(_serial=next(_table_serial), kx=kx, ky=ky, two_pi_i_kx=ikx, two_pi_i_ky=iky, two_pi_i_kx_2=ikx**2,
                   two_pi_i_ky_2=iky**2, two_pi_i_k_2=k2, two_pi_i_k_4=k2**2)
        if len(_spectral_cache) > 8:
            _spectral_cache.clear()
        _spectral_cache[key] = tab
    return tab


class KeyedArray(np.ndarray):
    """ndarray that remembers what it was built from (``key``), so a consumer that has already uploaded the same
    field can skip the transfer: PDEEnv.step rebuilds the equation and the solver every step (pde_env.py:286-291),
    and an unchanged 1024^2 ``fourier_symbol`` would otherwise cost an 8 MiB upload plus a multiplier rebuild."""

    key = None

    def __array_finalize__(self, obj):
        self.key = None  # views and results of arithmetic are new data


def keyed(arr: np.ndarray, key) -> KeyedArray:
    out = np.asarray(arr).view(KeyedArray)
    out.key = key
    return out


class _Spectral:
    """Published spectral attribute, computed on first access (class access keeps ``hasattr`` true
    for ``check_equation_solver_compatibility``)."""

    def __init__(self, name):
        self.name = name

    def __get__(self, obj, cls=None):
        if obj is None:
            return self
        return spectral_table(obj.domain)[self.name]


def _install_spectral(cls):
    for name in _SPECTRAL_NAMES:
        setattr(cls, name, _Spectral(name))
    # published for signature compatibility with the solvers; the HIP integrators use rocFFT
    cls.fft = staticmethod(np.fft.fftn)
    cls.ifft = staticmethod(np.fft.ifftn)
    return cls


# what a torch.nn.Module as mu runs on (pde_opt_amd.fieldmu)
FIELD_MU_SUPPORT = ('CahnHilliard2DPeriodic with derivs="fd", SemiImplicitFourierSpectral or Euler with ConstantStepSize, '
                    'fp32 / fp64, D a DiffusionLegendrePolynomials (trainable) or a fixed in-kernel closure, kappa fixed')


def _select_rhs(eq):
    if eq.derivs == "fd":
        eq.rhs = eq.rhs_fd
    elif eq.derivs == "fourier":
        eq.rhs = eq.rhs_fourier
    else:
        raise ValueError(f"Invalid derivative type: {eq.derivs}")


@_install_spectral
@dataclasses.dataclass
class CahnHilliard2DPeriodic(BaseEquation):
    """du/dt = div( D(u) grad( mu_h(u) - kappa lap u ) )."""

    domain: Domain
    kappa: float
    mu: Any
    D: Any
    derivs: str = "fd"

    @property
    def fourier_symbol(self):
        """kappa (2 pi i k)^4, the stiff linear symbol of the IMEX solver (cahn_hilliard.py:74)"""
        tab = spectral_table(self.domain)
        key = ("kappa_k4", float(self.kappa))
        hit = tab.get("_symbol")
        if hit is None or hit.key[-1] != key:
            hit = tab["_symbol"] = keyed(self.kappa * tab["two_pi_i_k_4"], (tab["_serial"], key))
        return hit

    _per_env_controls = frozenset({"kappa", "mu", "D"})
    _scalar_controls = frozenset({"kappa"})  # stored as given: fourier_symbol / _engine_problem read it when asked

    def rhs(self, state, t):  # replaced in __post_init__, as upstream
        raise NotImplementedError("rhs method not implemented")

    def __post_init__(self):
        if len(self.domain.points) != 2:
            raise ValueError("CahnHilliard2DPeriodic needs a 2-D domain")
        if is_torch_module(self.D):
            raise UnsupportedClosureError("a torch.nn.Module is supported as mu only; D stays a closure of the in-kernel family")
        # a network as mu is no closure: the kernels take the field it returns (pde_opt_amd.fieldmu)
        self._mu_module = self.mu if is_torch_module(self.mu) else None
        self._mu_desc = None if self._mu_module is not None else as_closure(self.mu)
        self._mob_desc = as_closure(self.D)
        _select_rhs(self)

    def _engine_problem(self, field_mu: bool = False):
        """``field_mu``: the caller feeds mu_h to the kernels as a field (the problem's own mu closure is not read)"""
        if self._mu_module is not None and not field_mu:
            raise UnsupportedClosureError("mu is a torch.nn.Module: it runs through PDEModel.solve / residuals / mse / "
                                          "mse_backward / train(method='mse') (" + FIELD_MU_SUPPORT + "), not through rhs or diffeqsolve")
        nx, ny = self.domain.points
        hx, hy = self.domain.dx
        return dict(equation=L.EQ_CAHN_HILLIARD, nx=nx, ny=ny, hx=hx, hy=hy, kappa=float(self.kappa),
                    mu=self._mu_desc, mob=self._mob_desc,
                    derivs=L.DERIVS_FOURIER if self.derivs == "fourier" else L.DERIVS_FD)

    def rhs_fd(self, state, t):
        return self._run_rhs(state, t)

    def rhs_fourier(self, state, t):
        return self._run_rhs(state, t)  # 7 batched rocFFT transforms (cahn_hilliard.py:82-87)


@_install_spectral
@dataclasses.dataclass
class AllenCahn2DPeriodic(BaseEquation):
    """du/dt = -R(u) ( mu_h(u) - kappa lap u )."""

    domain: Domain
    kappa: float
    mu: Any
    R: Any
    derivs: str = "fd"

    _per_env_controls = frozenset({"kappa", "mu", "R"})
    _scalar_controls = frozenset({"kappa"})  # stored as given: fourier_symbol / _engine_problem read it when asked

    def rhs(self, state, t):
        raise NotImplementedError("rhs method not implemented")

    def __post_init__(self):
        if len(self.domain.points) != 2:
            raise ValueError("AllenCahn2DPeriodic needs a 2-D domain")
        self._mu_desc = as_closure(self.mu)
        self._mob_desc = as_closure(self.R)
        _select_rhs(self)

    def _engine_problem(self):
        nx, ny = self.domain.points
        hx, hy = self.domain.dx
        return dict(equation=L.EQ_ALLEN_CAHN, nx=nx, ny=ny, hx=hx, hy=hy, kappa=float(self.kappa),
                    mu=self._mu_desc, mob=self._mob_desc,
                    derivs=L.DERIVS_FOURIER if self.derivs == "fourier" else L.DERIVS_FD)

    def rhs_fd(self, state, t):
        return self._run_rhs(state, t)

    def rhs_fourier(self, state, t):
        return self._run_rhs(state, t)  # 3 batched rocFFT transforms (allen_cahn.py:74-79)


@dataclasses.dataclass
class CahnHilliard3DPeriodic(BaseEquation):
    """du/dt = div( D(u) grad( mu_h(u) - kappa lap u ) ) on a periodic 3-D box
    (pde_opt/numerics/equations/cahn_hilliard.py:113-200).  Fields are ``(Nx, Ny, Nz)`` (or batched
    ``(B, Nx, Ny, Nz)``); ``rhs_fd`` runs in two HIP passes (csrc/stencil_generic.hpp, CH-3D), ``rhs_fourier``
    (:167-175) on 9 batched rocFFT 3-D transforms with the pointwise operators between them
    (csrc/spectral.hip), the IMEX solver on rocFFT's 3-D real<->hermitian plans."""

    domain: Domain
    kappa: float
    mu: Any
    D: Any
    derivs: str = "fd"
    # class-level placeholders, as upstream (cahn_hilliard.py:138-140): check_equation_solver_compatibility
    # looks the solver's required attributes up on the CLASS
    fft = None
    ifft = None
    fourier_symbol = None
    _per_env_controls = frozenset({"kappa", "mu", "D"})
    # (no _scalar_controls: __post_init__ derives fourier_symbol from kappa)

    def rhs(self, state, t):  # replaced in __post_init__, as upstream
        raise NotImplementedError("rhs method not implemented")

    def __post_init__(self):
        if len(self.domain.points) != 3:
            raise ValueError("CahnHilliard3DPeriodic needs a 3-D domain")
        self.kx, self.ky, self.kz = self.domain.fft_mesh()
        self.two_pi_i_kx = 2j * np.pi * self.kx
        self.two_pi_i_ky = 2j * np.pi * self.ky
        self.two_pi_i_kz = 2j * np.pi * self.kz
        self.two_pi_i_kx_2 = self.two_pi_i_kx**2
        self.two_pi_i_ky_2 = self.two_pi_i_ky**2
        self.two_pi_i_kz_2 = self.two_pi_i_kz**2
        self.two_pi_i_k_2 = self.two_pi_i_kx_2 + self.two_pi_i_ky_2 + self.two_pi_i_kz_2
        self.two_pi_i_k_4 = self.two_pi_i_k_2**2
        self.fft = np.fft.fftn
        self.ifft = np.fft.ifftn
        self.fourier_symbol = self.kappa * self.two_pi_i_k_4
        self._mu_desc = as_closure(self.mu)
        self._mob_desc = as_closure(self.D)
        if self.derivs == "fd":
            self.rhs = self.rhs_fd
        elif self.derivs == "fourier":
            self.rhs = self.rhs_fourier
        else:
            raise ValueError(f"Invalid derivative type: {self.derivs}")

    _state_trailing = ()

    def _engine_problem(self):
        nx, ny, nz = self.domain.points
        hx, hy, hz = self.domain.dx
        return dict(equation=L.EQ_CAHN_HILLIARD_3D, nx=nx, ny=ny, nz=nz, hx=hx, hy=hy, hz=hz,
                    kappa=float(self.kappa), mu=self._mu_desc, mob=self._mob_desc,
                    derivs=L.DERIVS_FOURIER if self.derivs == "fourier" else L.DERIVS_FD)

    def rhs_fd(self, state, t):
        return self._run_rhs(state, t)

    def rhs_fourier(self, state, t):
        return self._run_rhs(state, t)  # 9 batched rocFFT 3-D transforms (cahn_hilliard.py:167-175)
