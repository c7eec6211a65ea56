"""docs/notebooks/optimization_3D.ipynb on the MI355X: fit a Legendre chemical potential and mobility to 3-D
Cahn-Hilliard data with PDEModel.train (Levenberg-Marquardt on GPU forward-mode sensitivities).

The full run is the notebook's (32^3, ts = linspace(0, 0.2, 100), dt0 = 1e-6, 100 LM steps); ``--quick`` keeps the grid
and the set-up but uses a data window ten times shorter and 3 LM steps."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout
import time

import numpy as np

from pde_opt_amd import CahnHilliard3DPeriodic, Domain, PDEModel, SemiImplicitFourierSpectral
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials, DiffusionLegendrePolynomials

quick = "--quick" in sys.argv

Nx = Ny = Nz = 32
Lx = Ly = Lz = 0.01 * Nx

domain = Domain(
    (Nx, Ny, Nz),
    (
        (-Lx / 2, Lx / 2),
        (-Ly / 2, Ly / 2),
        (-Lz / 2, Lz / 2),
    ),
    "dimensionless",
)

opt_model = PDEModel(
    equation_type=CahnHilliard3DPeriodic,
    domain=domain,
    solver_type=SemiImplicitFourierSpectral,
)

params = {"kappa": 0.002, "mu": lambda c: np.log(c / (1.0 - c)) + 3.0 * (1.0 - 2.0 * c), "D": lambda c: 0.15 * np.ones_like(c)}

solver_params = {"A": 0.5}

y0 = np.clip(0.01 * np.random.default_rng(0).standard_normal((Nx, Ny, Nz)) + 0.5, 0.0, 1.0)
ts = np.linspace(0.0, 0.02 if quick else 0.2, 100)
t0 = time.perf_counter()
sol = opt_model.solve(params, y0, ts, solver_params, dt0=0.000001, max_steps=1000000)
print(f"data: {len(ts)} saves of {Nx}x{Ny}x{Nz} up to t = {ts[-1]}, {time.perf_counter() - t0:.2f} s")

chem_pot_model = ChemicalPotentialLegendrePolynomials(np.zeros(6), lambda x: np.log(x / (1.0 - x)))
diffusivity_model = DiffusionLegendrePolynomials(np.log(0.05) * np.ones(1))

data = {}
data["ys"] = sol
data["ts"] = ts

inds = [[30, 40, 50], [50, 60, 70], [70, 80, 90]]

init_params = {
    "mu": chem_pot_model,
    "D": diffusivity_model,
}

static_params = {
    "kappa": 0.002,
}

solver_parameters = {
    "A": 0.5,
}

weights = {
    "mu": ChemicalPotentialLegendrePolynomials(np.array([0, 2, 6, 12, 20, 30])),
    "D": DiffusionLegendrePolynomials(np.array([0])),
}

lambda_reg = 0.0

t0 = time.perf_counter()
res = opt_model.train(data, inds, init_params, static_params, solver_parameters, weights, lambda_reg,
                      method="least_squares", max_steps=3 if quick else 100)
t_train = time.perf_counter() - t0
hist = opt_model.last_train_history
print(f"train: {len(hist) - 1} accepted LM steps in {t_train:.2f} s; objective {hist[0]:.3e} -> {hist[-1]:.3e}")

# the ground truth in the same basis: log(c / (1 - c)) + 3 (1 - 2c) = logit prior - 3 P_1(2c - 1); D = exp(log 0.15)
mu_fit, d_fit = np.asarray(res["mu"].expansion.params), np.asarray(res["D"].expansion.params)
print("mu coefficients:", np.array2string(mu_fit, precision=6), " (ground truth [0, -3, 0, 0, 0, 0])")
print("D coefficients: ", np.array2string(d_fit, precision=6), f" (ground truth [{np.log(0.15):.6f}])")
cs = np.linspace(0.01, 0.99, 100)
mu_gt, d_gt = params["mu"](cs), params["D"](cs)
mu_opt, d_opt = res["mu"](cs), res["D"](cs)
idx_05 = np.argmin(np.abs(cs - 0.5))  # mu is fitted up to a constant: compare shifted to c = 0.5
print("max |mu - mu_gt| (shifted):", float(np.max(np.abs((mu_opt - mu_opt[idx_05]) - (mu_gt - mu_gt[idx_05])))))
print("max |D - D_gt|:", float(np.max(np.abs(d_opt - d_gt))))
assert np.all(np.isfinite(mu_fit)) and np.all(np.isfinite(d_fit))
assert hist[-1] <= hist[0]

opt_sol = opt_model.solve(res, y0, ts, solver_parameters, dt0=0.000001, max_steps=1000000)
print("max |u_opt - u_gt| over the run:", float(np.max(np.abs(np.asarray(opt_sol) - np.asarray(sol)))))
