"""Train a neural-network chemical potential from trajectories (upstream's docs/notebooks/optimization_neural_network.ipynb,
run as notebooks/optimize_nn_script.py runs it: a first-order optimiser with step 1e-2 on the mse).

A CahnHilliard2DPeriodic field is solved with a "true" chemical potential (Legendre series under the logit prior).  A
periodic CNN then takes the place of ``mu`` and is trained so that short solves from frames of that trajectory land on
the frames that follow.  The CNN runs in torch on the GPU; the stencil, the IMEX operator and their transposes are HIP
kernels (pde_opt_amd.fieldmu).  ``PDEModel.mse_backward`` fills ``.grad`` of the CNN's parameters by a discrete adjoint
of the solve, whose cost does not depend on the number of parameters, and ``torch.optim.Adam`` takes the step.

``--quick`` runs 32^2 with a small CNN for 20 optimiser steps instead of 64^2 with the notebook's CNN for 200.
``--native-cnn`` evaluates and differentiates the CNN in the library's own HIP kernels instead of torch
(``model.fieldmu_solver().native_cnn = True``; experimental, off by default)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout
import time

import numpy as np
import torch

from pde_opt_amd import CahnHilliard2DPeriodic, Domain, PDEModel, SemiImplicitFourierSpectral
from pde_opt_amd.numerics.functions.cnn import PeriodicCNN
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials, DiffusionLegendrePolynomials

quick = "--quick" in sys.argv
N, HIDDEN, STEPS = (32, (8, 8), 20) if quick else (64, (32, 64, 64), 200)

L = 0.01 * N
domain = Domain((N, N), ((-L / 2, L / 2), (-L / 2, L / 2)), "dimensionless")
model = PDEModel(equation_type=CahnHilliard2DPeriodic, domain=domain, solver_type=SemiImplicitFourierSpectral)


def logit(c):
    return np.log(c / (1.0 - c))


KAPPA = 0.002
D = DiffusionLegendrePolynomials(np.array([0.0]))
truth = {"kappa": KAPPA, "mu": ChemicalPotentialLegendrePolynomials(np.array([0.0, -3.0]), logit), "D": D}
y0 = np.clip(0.5 + 0.05 * np.random.default_rng(0).standard_normal((N, N)), 0.05, 0.95)
frames = model.solve(truth, y0, np.linspace(0.0, 4e-4, 9), {"A": 0.5})  # 9 frames, 50 substeps apart

# three trajectories: from frames 2, 4 and 6, each compared with the two frames that follow
inds = [[2, 3, 4], [4, 5, 6], [6, 7, 8]]
y0s = np.stack([frames[i[0]] for i in inds])
values = np.stack([np.stack([frames[j] for j in i[1:]]) for i in inds])
ts = np.array([0.0, 5e-5, 1e-4])

torch.manual_seed(0)
cnn = PeriodicCNN(1, HIDDEN, 1).double().to("cuda")
if "--native-cnn" in sys.argv:
    model.fieldmu_solver().native_cnn = True
params = {"kappa": KAPPA, "mu": cnn, "D": D}
opt = torch.optim.Adam(cnn.parameters(), lr=1e-2)
n_par = sum(p.numel() for p in cnn.parameters())
print(f"{N}x{N}, PeriodicCNN(1, {HIDDEN}, 1): {n_par} parameters, {len(inds)} trajectories x 100 substeps")

t0 = time.perf_counter()
losses = []
for it in range(STEPS):
    losses.append(model.mse_backward(params, (y0s, values), {"A": 0.5}, ts, {}, 0.0))  # sets .grad
    opt.step()
    if it % max(1, STEPS // 10) == 0:
        print(f"  step {it:4d}  mse {losses[-1]:.6e}")
final = model.mse(params, (y0s, values), {"A": 0.5}, ts, {}, 0.0)
print(f"loss {losses[0]:.6e} -> {final:.6e} in {STEPS} Adam steps, {time.perf_counter() - t0:.1f} s")
if not (np.isfinite(final) and final < losses[0]):
    sys.exit("the loss did not decrease")
