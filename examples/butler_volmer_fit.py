"""Learn reaction kinetics from a constant-current run: fit the chemical potential ``mu`` and the exchange current ``j0`` of
AllenCahn2DPeriodicButlerVolmerConstantCurrent to frames AND to the voltage curve with PDEModel.train.

Synthetic data: trajectories of du/dt = j0(u) (exp(-alpha eta) - exp((1 - alpha) eta)), eta = mu + v, with v solving the
constant-current constraint, from known Legendre coefficients of ``mu`` (under the logit prior) and ``j0`` (exp-wrapped).
The fit starts from perturbed coefficients and is driven by GPU forward-mode sensitivities (Levenberg-Marquardt on RK4).

At constant current the frames alone cannot see mu's constant coefficient -- the voltage absorbs a shift of mu -- so the
first fit leaves it where it started; with ``data["vs"]`` and ``voltage_weight`` the voltage curve pins it down, and
``voltage_sensitivities`` returns the fitted curve.  The scalars (alpha, kappa, Crate) are not trainable: other_parameters.

``--quick`` halves the grid, shortens the data window and caps the optimiser steps."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout
import time

import numpy as np

from pde_opt_amd import RK4, AllenCahn2DPeriodicButlerVolmerConstantCurrent, Domain, PDEModel
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials, DiffusionLegendrePolynomials

quick = "--quick" in sys.argv

N, H = (32 if quick else 64), 0.01
domain = Domain((N, N), ((0.0, N * H), (0.0, N * H)), "dimensionless")
model = PDEModel(equation_type=AllenCahn2DPeriodicButlerVolmerConstantCurrent, domain=domain, solver_type=RK4)


def logit(c):
    return np.log(c / (1.0 - c))


mu_true, j0_true = np.array([0.1, -3.0, 0.2]), np.array([np.log(200.0), 0.15])
other = {"kappa": 0.002, "alpha": 0.5, "Crate": 50.0 * (N * H) ** 2}  # a mean filling rate of 50 per unit time
truth = {"mu": ChemicalPotentialLegendrePolynomials(mu_true, logit), "j0": DiffusionLegendrePolynomials(j0_true), **other}

rng = np.random.default_rng(0)
x = np.arange(N) / N


def smooth_state():
    u = 0.2 + np.zeros((N, N))
    for _ in range(6):
        kx, ky = rng.integers(1, 4, 2)
        u += 0.02 * rng.standard_normal() * np.cos(2 * np.pi * (kx * x[:, None] + ky * x[None, :]) + rng.uniform(0, 6))
    return u


# two trajectories, each observed at three later times that fall on steps of dt0 = 1e-6, the step PDEModel.train uses
B = 2
steps = (30, 60, 100) if quick else (100, 250, 400)
ts = np.array([0.0] + [k * 1e-6 for k in steps])
y0s = np.stack([smooth_state() for _ in range(B)])
t0 = time.perf_counter()
sol = model.solve(truth, y0s, ts, {})  # (T, B, N, N)
equation = AllenCahn2DPeriodicButlerVolmerConstantCurrent(domain=domain, **truth)
vs = np.stack([equation.get_voltage(sol[q]) for q in range(len(ts))])  # (T, B)
print(f"data: {B} trajectories of {N}x{N}, {len(ts) - 1} frames up to t = {ts[-1]:g}, voltage {vs[0, 0]:.4f} -> {vs[-1, 0]:.4f}, "
      f"{time.perf_counter() - t0:.2f} s")

data = {"ys": [sol[q, b] for b in range(B) for q in range(len(ts))], "ts": np.tile(ts, B),
        "vs": [vs[q, b] for b in range(B) for q in range(len(ts))]}
inds = [[b * len(ts) + q for q in range(len(ts))] for b in range(B)]

for weight in (0.0, 1.0):
    init = {"mu": ChemicalPotentialLegendrePolynomials(np.array([0.3, -2.7, 0.3]), logit),
            "j0": DiffusionLegendrePolynomials(np.array([np.log(150.0), 0.1]))}
    t0 = time.perf_counter()
    res = model.train(data, inds, init, other, {}, {}, 0.0, method="least_squares", max_steps=8 if quick else 100,
                      voltage_weight=weight)
    hist = model.last_train_history
    mu_fit, j0_fit = np.asarray(res["mu"].expansion.params), np.asarray(res["j0"].expansion.params)
    V, _ = model.voltage_sensitivities({"mu": res["mu"], "j0": res["j0"]}, other, y0s, ts)
    print(f"voltage_weight = {weight}: {len(hist) - 1} steps, {time.perf_counter() - t0:.2f} s, objective {hist[0]:.3e} -> {hist[-1]:.3e}")
    print(f"  mu {np.round(mu_fit, 6)} (true {mu_true}),  j0 {np.round(j0_fit, 6)} (true {np.round(j0_true, 6)})")
    print(f"  voltage curve: max |V_fit - V_data| = {np.max(np.abs(V - vs)):.3e}")
    if not np.all(np.isfinite(mu_fit)) or not np.all(np.isfinite(j0_fit)) or not hist[-1] < hist[0]:
        sys.exit("the fit did not reduce its objective")
