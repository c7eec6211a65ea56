"""Fit the chemical potential and the rate of an Allen-Cahn equation to trajectories with PDEModel.train.

Synthetic data: 64^2 trajectories of du/dt = -R(u) (mu_h(u) - kappa lap u) with known Legendre coefficients of ``mu``
(under the logit prior) and of ``R`` (exp-wrapped).  Both fits start from perturbed coefficients and are driven by GPU
forward-mode sensitivities: ``least_squares`` (Levenberg-Marquardt) and ``mse`` (BFGS), on the RK4 solver.  Unlike
Cahn-Hilliard, Allen-Cahn sees mu itself, so mu's constant coefficient is fitted too.

``--quick`` shortens the data window (100 substeps per trajectory instead of 400) and the number of optimiser steps."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout
import time

import numpy as np

from pde_opt_amd import RK4, AllenCahn2DPeriodic, Domain, PDEModel
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials, DiffusionLegendrePolynomials

quick = "--quick" in sys.argv

N = 64
domain = Domain((N, N), ((0.0, 1.0), (0.0, 1.0)), "dimensionless")
model = PDEModel(equation_type=AllenCahn2DPeriodic, domain=domain, solver_type=RK4)


def logit(c):
    return np.log(c / (1.0 - c))


mu_true, R_true = np.array([0.1, -3.0, 0.3]), np.array([np.log(1000.0), 0.3])
truth = {"kappa": 0.002, "mu": ChemicalPotentialLegendrePolynomials(mu_true, logit), "R": DiffusionLegendrePolynomials(R_true)}

rng = np.random.default_rng(0)
x = np.arange(N) / N


def smooth_state():
    u = 0.5 + np.zeros((N, N))
    for _ in range(6):
        kx, ky = rng.integers(1, 4, 2)
        u += 0.05 * rng.standard_normal() * np.cos(2 * np.pi * (kx * x[:, None] + ky * x[None, :]) + rng.uniform(0, 6))
    return u


# three trajectories, each observed at three later times (dt0 = 1e-6, the step PDEModel.train uses)
B = 3
span = 1e-4 if quick else 4e-4
ts = np.linspace(0.0, span, 4)
y0s = np.stack([smooth_state() for _ in range(B)])
t0 = time.perf_counter()
sol = model.solve(truth, y0s, ts, {})  # (T, B, N, N)
print(f"data: {B} trajectories of {N}x{N}, {len(ts) - 1} frames up to t = {ts[-1]:g}, {time.perf_counter() - t0:.2f} s")

data = {"ys": [sol[q, b] for b in range(B) for q in range(len(ts))], "ts": np.tile(ts, B)}
inds = [[b * len(ts) + q for q in range(len(ts))] for b in range(B)]

for method in ("least_squares", "mse"):
    init = {"mu": ChemicalPotentialLegendrePolynomials(np.array([0.0, -2.6, 0.2]), logit),
            "R": DiffusionLegendrePolynomials(np.array([np.log(800.0), 0.2]))}
    t0 = time.perf_counter()
    res = model.train(data, inds, init, {"kappa": 0.002}, {}, {}, 0.0, method=method, max_steps=5 if quick else 100)
    hist = model.last_train_history
    mu_fit, R_fit = np.asarray(res["mu"].expansion.params), np.asarray(res["R"].expansion.params)
    print(f"{method}: {len(hist) - 1} steps, {time.perf_counter() - t0:.2f} s, objective {hist[0]:.3e} -> {hist[-1]:.3e}")
    print(f"  mu {np.round(mu_fit, 6)} (true {mu_true}),  R {np.round(R_fit, 6)} (true {np.round(R_true, 6)})")
    if not np.all(np.isfinite(mu_fit)) or not np.all(np.isfinite(R_fit)) or not hist[-1] < hist[0]:
        sys.exit("the fit did not reduce its objective")
