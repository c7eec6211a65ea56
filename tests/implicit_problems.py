"""The problems the implicit Euler tests share (tests/test_implicit_cpu.py, tests/test_gpu_implicit.py): grids, closure
classes, seeded states, the step 50 x the explicit Euler limit and the tolerances per dtype."""
import numpy as np

import pde_opt_amd as P
from pde_opt_amd.numerics.closures import LEGENDRE, LOGIT_PRIOR, POLY, ClosureDesc

import implicit_ref as R

H, KAPPA = 0.01, 0.002
GRIDS = {"16x32": (16, 32), "8x12": (8, 12), "33x130": (33, 130), "64x64": (64, 64)}
# (mu, mobility): a polynomial mu with a constant mobility; the Legendre mu under the logit prior; a non-constant
# polynomial mobility, so that D' / R' are exercised
CLOSURES = {
    "poly": (ClosureDesc(POLY, 0, (0.0, -1.0, 0.0, 1.0)), ClosureDesc(POLY, 0, (1.0,))),
    "legendre_logit": (ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.2, -1.0, 0.4)), ClosureDesc(POLY, 0, (1.0,))),
    "poly_mob": (ClosureDesc(POLY, 0, (0.0, -1.0, 0.0, 1.0)), ClosureDesc(POLY, 0, (1.0, 0.1, 0.2))),
}
# Newton tolerances per dtype (rtol, atol): the issue's
TOL = {np.float64: (1e-10, 1e-12), np.float32: (1e-4, 1e-6)}
STEP_FACTOR = 50.0


def domain(points):
    nx, ny = points
    return P.Domain(points, ((0.0, H * nx), (0.0, H * ny)), "dimensionless")


def equation(eq, points, closures, derivs="fd"):
    mu, mob = CLOSURES[closures]
    cls = P.CahnHilliard2DPeriodic if eq == "ch" else P.AllenCahn2DPeriodic
    return cls(domain(points), KAPPA, mu, mob, derivs=derivs)


def state(points, seed, dtype=np.float64):
    """seeded uniform noise in [0.2, 0.8]"""
    return np.random.default_rng(seed).uniform(0.2, 0.8, points).astype(dtype)


def step_size(eq, points, closures, u):
    """50 x the explicit Euler stability limit of the problem at u (implicit_ref.euler_limit says how it is bounded)"""
    mu, mob = CLOSURES[closures]
    return STEP_FACTOR * R.euler_limit(eq, np.asarray(u, np.float64), H, H, KAPPA, mu, mob)
