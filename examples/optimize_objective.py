"""Tune closure coefficients so that a scalar of the final state reaches a target, with PDEModel.optimize.

A CahnHilliard2DPeriodic field starts as noise around c = 0.5 and is solved for a short time.  The objective is the
miss of the second moment ``mean(c^2)`` of the last saved state against a target, in units of the miss of the starting
coefficients (so J = 1 at the start: BFGS stops on absolute tolerances of 1e-8), written with torch:

    J(ys) = ((mean(ys[-1]^2) - target) / (start - target))^2

The target is the second moment the "true" coefficients of ``mu`` (Legendre series under the logit prior) and ``D``
(exp-wrapped) give; the optimisation starts from perturbed ones.  No frame of the true trajectory is used: one number
constrains the coefficients, so the optimiser finds *a* set that reaches the target, not the true one.  The gradient of
J comes from ``torch.autograd`` (dJ/dys) contracted with the GPU's forward-mode tangents (dys/dp).

``--quick`` runs 32^2 for 200 substeps instead of 64^2 for 1000."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout
import time

import numpy as np
import torch

from pde_opt_amd import CahnHilliard2DPeriodic, Domain, PDEModel, SemiImplicitFourierSpectral
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials, DiffusionLegendrePolynomials

quick = "--quick" in sys.argv
N, SUBSTEPS = (32, 200) if quick else (64, 1000)
# The same optimisation through the fp64 numpy tangents (`python tests/optimize_ref.py --example`) at the quick size:
#   J = 1.0, 2.9e-01, 8.6e-04, 4.7e-04, 1.6e-05, 1.8e-07, 9.4e-11, 5.90e-16, 4.05e-22   (8 BFGS steps)
# The last step is the one BFGS's stopping rule (|dp| <= 1e-8 (1 + |p|)) may or may not still take, and 4e-22 is the
# rounding floor of mean(c^2); what every run must reach before that rule can fire is the value before it.  Required:
# 10 x that value (the 10 x rule of DESIGN 4.9).
REQUIRED_FACTOR = 10 * 5.90e-16

L = 0.01 * N
domain = Domain((N, N), ((-L / 2, L / 2), (-L / 2, L / 2)), "dimensionless")
model = PDEModel(equation_type=CahnHilliard2DPeriodic, domain=domain, solver_type=SemiImplicitFourierSpectral)


def logit(c):
    return np.log(c / (1.0 - c))


KAPPA = 0.002
MU_TRUE, D_TRUE = np.array([0.0, -3.0, 0.2]), np.array([-1.0, 0.2])
MU_INIT, D_INIT = np.array([0.0, -2.6, 0.1]), np.array([-1.4, 0.1])
y0 = np.clip(0.5 + 0.05 * np.random.default_rng(0).standard_normal((N, N)), 0.05, 0.95)
ts = np.array([0.0, SUBSTEPS * 1e-6])  # dt0 = 1e-6, the step PDEModel.solve uses

truth = {"kappa": KAPPA, "mu": ChemicalPotentialLegendrePolynomials(MU_TRUE, logit), "D": DiffusionLegendrePolynomials(D_TRUE)}
target = float(np.mean(model.solve(truth, y0, ts, {"A": 0.5})[-1] ** 2))


init = {"mu": ChemicalPotentialLegendrePolynomials(MU_INIT, logit), "D": DiffusionLegendrePolynomials(D_INIT)}
start = float(np.mean(model.solve({**init, "kappa": KAPPA}, y0, ts, {"A": 0.5})[-1] ** 2))


def objective(ys):  # ys: torch.Tensor (len(ts), N, N)
    return ((torch.mean(ys[-1] ** 2) - target) / (start - target)) ** 2


t0 = time.perf_counter()
res = model.optimize(objective, y0, ts, init, {"kappa": KAPPA}, {"A": 0.5}, {}, 0.0, max_steps=100)
hist = model.last_optimize_history
got = float(np.mean(model.solve(res, y0, ts, {"A": 0.5})[-1] ** 2))
print(f"{N}x{N}, {SUBSTEPS} substeps: {len(hist) - 1} BFGS steps, {time.perf_counter() - t0:.2f} s")
print(f"  mean(c^2) at t = {ts[-1]:g}: start {start:.8f}, target {target:.8f}, reached {got:.8f}")
print(f"  objective {hist[0]:.3e} -> {hist[-1]:.3e}")
print(f"  mu {np.round(res['mu'].expansion.params, 6)},  D {np.round(res['D'].expansion.params, 6)}")
if not (np.isfinite(hist[-1]) and hist[-1] <= REQUIRED_FACTOR * hist[0]):
    sys.exit(f"the objective fell by {hist[-1] / hist[0]:.1e}, not by {REQUIRED_FACTOR:.0e}")
