"""The problems the smoothed-boundary sensitivity tests share (tests/test_sbm_sens_cpu.py, test_gpu_sbm_sens.py,
test_gpu_sbm_fit.py): closures, shapes, states and the matching ``sbm_sens_ref.Problem`` / equation objects."""
import types

import numpy as np

import sbm_sens_ref as S
from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, ClosureDesc, as_closure
from util import SBM_F, SBM_FLUX, SBM_THETA, sbm_psi

KAPPA = 1.5
PARAMS = [(S.MU_ROLE, 0), (S.MU_ROLE, 2), (S.MOB_ROLE, 0), (S.MOB_ROLE, 1)]
# regular-solution-like mu: a Legendre series under the logit prior (log(c / (1 - c)) + 3 (1 - 2c) is the series (0, -3))
MU = ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.2, -3.0, 0.4))
MOBS = {
    "legendre": ClosureDesc(LEGENDRE, 0, (0.8, 0.2)),
    "exp_legendre": ClosureDesc(LEGENDRE, EXP_WRAP, (-0.3, 0.2)),
}
F = as_closure(SBM_F)  # c ln c + (1 - c) ln(1 - c) + 3 c (1 - c) + 0.059: positive on [0.1, 0.9] (0.0039 at the ends)

# shape -> (points, (hx, hy)); the tangent kernels' tile is 16 x 32
SHAPES = {
    "8x8": ((8, 8), (1.0, 1.0)),        # smaller than a tile both ways: the wrap takes the modulo path
    "16x32": ((16, 32), (1.0, 1.0)),    # exactly one tile: the ring wraps onto the tile itself
    "33x47": ((33, 47), (1.0, 1.0)),    # partial tiles and an odd row length
    "64x64": ((64, 64), (1.0, 2.0)),    # several full tiles, hx != hy
    "67x40": ((67, 40), (1.0, 1.0)),    # Cahn-Hilliard's mask left_half[:50, :] takes both values
    "24x120": ((24, 120), (1.0, 1.0)),  # Allen-Cahn's mask left_half[:, :100] takes both values
}
# dt of the trajectory tests (GPU: 200 substeps at 64^2), inside the explicit stability bound of the stiffer problem,
# Cahn-Hilliard (dt <~ h^4 / (16 kappa D) ~ 0.05 at h = 1, kappa = 1.5, D <= 1; the wall term and 1 / psi <= 20 tighten
# it); Allen-Cahn is not conservative: 200 steps of 2^-8 keep the state well inside (0, 1).  Powers of two, and a start
# time that is one: every stage time t0 + s dt (+ dt / 2) is exact, so a split advance sees the same times bit for bit.
# tests/test_sbm_sens_cpu.py checks both on the oracle.
TRAJ_DT = {"ac": 2.0 ** -8, "ch": 2.0 ** -9}
TRAJ_T0 = 2.0 ** -5
SHAPES_OF = {"ac": ["8x8", "16x32", "33x47", "64x64", "24x120"], "ch": ["8x8", "16x32", "33x47", "64x64", "67x40"]}


def problem(eq, shape, mob="legendre", theta=SBM_THETA, flux=SBM_FLUX, mu=MU):
    points, (hx, hy) = SHAPES[shape] if isinstance(shape, str) else shape
    return S.Problem(eq, sbm_psi(*points), hx, hy, KAPPA, F, mu, MOBS[mob] if isinstance(mob, str) else mob, theta, flux,
                     S.left_half(eq, points))


def domain(P, p):
    nx, ny = p.psi.shape
    return P.Domain((nx, ny), ((0.0, nx * p.hx), (0.0, ny * p.hy)), "dimensionless", geometry=types.SimpleNamespace(smooth=p.psi))


def equation(P, p, mu=None, mob=None):
    """the package's equation object of a reference problem (closures may be replaced, e.g. by Legendre classes)"""
    mu, mob = mu if mu is not None else p.mu, mob if mob is not None else p.mob
    if p.eq == "ac":
        return P.AllenCahn2DSmoothedBoundary(domain(P, p), p.kappa, SBM_F, mu, mob, p.theta)
    return P.CahnHilliard2DSmoothedBoundary(domain(P, p), p.kappa, SBM_F, mu, mob, p.theta, p.flux)


def state(points, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return np.clip(0.5 + 0.1 * rng.standard_normal(points), 0.1, 0.9).astype(dtype)


def smooth_state(points, seed):
    """a few long waves around 0.5: a state a trajectory test can advance for hundreds of steps"""
    nx, ny = points
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx) / nx, np.arange(ny) / ny, indexing="ij")
    u = 0.5 + 0.0 * x
    for _ in range(4):
        kx, ky = rng.integers(1, 4, size=2)
        u = u + 0.05 * rng.standard_normal() * np.cos(2 * np.pi * (kx * x + ky * y) + rng.uniform(0, 2 * np.pi))
    return np.clip(u, 0.1, 0.9)


def rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
