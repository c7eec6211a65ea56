"""Fit the chemical potential and the mobility of a particle of arbitrary shape to frames with PDEModel.train.

Synthetic data: Cahn-Hilliard inside a disc by the smoothed-boundary method (CahnHilliard2DSmoothedBoundary: the level set
psi, a contact angle theta(t) that ramps during the run, a boundary flux), solved with RK4 from known Legendre
coefficients of ``mu`` (under the logit prior) and of ``D`` (exp-wrapped).  The fit starts from perturbed coefficients and
is driven by GPU forward-mode sensitivities (Levenberg-Marquardt); the tangents see theta(t) and flux(t) at the stage times
of the solve.  ``f``, ``kappa``, ``theta`` and ``flux`` are fixed data.  mu's constant coefficient is inert (only grad(inner)
enters a Cahn-Hilliard right-hand side) and stays where it started.

``--quick`` shortens the data window (100 substeps per trajectory instead of 400) and the number of optimiser steps."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout
import time
import types

import numpy as np

from pde_opt_amd import RK4, CahnHilliard2DSmoothedBoundary, Domain, PDEModel
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials, DiffusionLegendrePolynomials

quick = "--quick" in sys.argv

NX, NY = 67, 40
x, y = np.meshgrid(np.arange(NX) + 0.5, np.arange(NY) + 0.5, indexing="ij")
r = np.sqrt((x - 0.5 * NX) ** 2 + (y - 0.5 * NY) ** 2)
psi = 0.05 + 0.95 * 0.5 * (1.0 + np.tanh((0.3 * min(NX, NY) - r) / 2.5))  # a disc, psi in (0.05, 1]
domain = Domain((NX, NY), ((0.0, float(NX)), (0.0, float(NY))), "dimensionless", geometry=types.SimpleNamespace(smooth=psi))
model = PDEModel(equation_type=CahnHilliard2DSmoothedBoundary, domain=domain, solver_type=RK4)


def logit(c):
    return np.log(c / (1.0 - c))


def free_energy(c):
    return c * np.log(c) + (1.0 - c) * np.log(1.0 - c) + 3.0 * c * (1.0 - c) + 0.059


span = 1e-4 if quick else 4e-4
fixed = {"kappa": 1.5, "f": free_energy,
         "theta": lambda t: np.pi / 2 - 0.8 * t / span,    # the contact angle ramps from 90 to 44 degrees
         "flux": lambda t: 0.02}
mu_true, D_true = np.array([0.0, -3.0, 0.3]), np.array([np.log(1000.0), 0.3])
truth = {**fixed, "mu": ChemicalPotentialLegendrePolynomials(mu_true, logit), "D": DiffusionLegendrePolynomials(D_true)}

rng = np.random.default_rng(0)


def smooth_state():
    u = 0.5 + np.zeros((NX, NY))
    for _ in range(4):
        kx, ky = rng.integers(1, 4, 2)
        u += 0.05 * rng.standard_normal() * np.cos(2 * np.pi * (kx * x / NX + ky * y / NY) + rng.uniform(0, 6))
    return np.clip(u, 0.1, 0.9)


# two trajectories, each observed at three later times (dt0 = 1e-6, the step PDEModel.train uses)
B = 2
ts = np.linspace(0.0, span, 4)
y0s = np.stack([smooth_state() for _ in range(B)])
t0 = time.perf_counter()
sol = model.solve(truth, y0s, ts, {})  # (T, B, NX, NY)
print(f"data: {B} trajectories of {NX}x{NY}, {len(ts) - 1} frames up to t = {ts[-1]:g}, {time.perf_counter() - t0:.2f} s")

data = {"ys": [sol[q, b] for b in range(B) for q in range(len(ts))], "ts": np.tile(ts, B)}
inds = [[b * len(ts) + q for q in range(len(ts))] for b in range(B)]

init = {"mu": ChemicalPotentialLegendrePolynomials(np.array([0.0, -2.6, 0.2]), logit),
        "D": DiffusionLegendrePolynomials(np.array([np.log(800.0), 0.2]))}
t0 = time.perf_counter()
res = model.train(data, inds, init, fixed, {}, {}, 0.0, method="least_squares", max_steps=5 if quick else 100)
hist = model.last_train_history
mu_fit, D_fit = np.asarray(res["mu"].expansion.params), np.asarray(res["D"].expansion.params)
print(f"least_squares: {len(hist) - 1} steps, {time.perf_counter() - t0:.2f} s, objective {hist[0]:.3e} -> {hist[-1]:.3e}")
print(f"  mu {np.round(mu_fit, 6)} (true {mu_true}),  D {np.round(D_fit, 6)} (true {np.round(D_true, 6)})")
if not np.all(np.isfinite(mu_fit)) or not np.all(np.isfinite(D_fit)) or not hist[-1] < hist[0]:
    sys.exit("the fit did not reduce its objective")
