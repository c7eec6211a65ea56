"""Fit an MLP-mixer chemical potential to trajectories (the reference's Mixer2d, pde_opt/numerics/functions/mixer_mlp.py, in
the role its notebooks give the periodic CNN: examples/optimization_neural_network.py).

A CahnHilliard2DPeriodic field is solved with a "true" chemical potential (Legendre series under the logit prior).  A
``Mixer2d`` then takes the place of ``mu`` and is fitted so that short solves from frames of that trajectory land on the
frames that follow: ``PDEModel.mse_backward`` fills ``.grad`` of the mixer's parameters by a discrete adjoint of the solve
and ``torch.optim.Adam`` takes the step.  The mixer and its vector-Jacobian product run in the library's own HIP kernels
(csrc/mixer.hip, ``model.fieldmu_solver().native_mixer = True``); ``--torch`` leaves them to torch.

``--quick`` runs 32^2 with patch 4 for 15 optimiser steps instead of 64^2 with patch 8 for 100."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout
import time

import numpy as np
import torch

from pde_opt_amd import CahnHilliard2DPeriodic, Domain, PDEModel, SemiImplicitFourierSpectral
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials, DiffusionLegendrePolynomials
from pde_opt_amd.numerics.functions.mixer import Mixer2d

quick = "--quick" in sys.argv
N, PATCH, HIDDEN, MIX, BLOCKS, STEPS = (32, 4, 8, (16, 16), 2, 15) if quick else (64, 8, 32, (64, 64), 4, 100)

L = 0.01 * N
domain = Domain((N, N), ((-L / 2, L / 2), (-L / 2, L / 2)), "dimensionless")
model = PDEModel(equation_type=CahnHilliard2DPeriodic, domain=domain, solver_type=SemiImplicitFourierSpectral)


def logit(c):
    return np.log(c / (1.0 - c))


KAPPA = 0.002
D = DiffusionLegendrePolynomials(np.array([0.0]))
truth = {"kappa": KAPPA, "mu": ChemicalPotentialLegendrePolynomials(np.array([0.0, -3.0]), logit), "D": D}
y0 = np.clip(0.5 + 0.05 * np.random.default_rng(0).standard_normal((N, N)), 0.05, 0.95)
frames = model.solve(truth, y0, np.linspace(0.0, 2e-4, 5), {"A": 0.5})  # 5 frames, 50 substeps apart

# two trajectories: from frames 1 and 2, each compared with the two frames that follow
inds = [[1, 2, 3], [2, 3, 4]]
y0s = np.stack([frames[i[0]] for i in inds])
values = np.stack([np.stack([frames[j] for j in i[1:]]) for i in inds])
ts = np.array([0.0, 5e-5, 1e-4])

torch.manual_seed(0)
mixer = Mixer2d((1, N, N), PATCH, HIDDEN, MIX[0], MIX[1], BLOCKS).double().to("cuda")
model.fieldmu_solver().native_mixer = "--torch" not in sys.argv
params = {"kappa": KAPPA, "mu": mixer, "D": D}
opt = torch.optim.Adam(mixer.parameters(), lr=1e-2)
n_par = sum(p.numel() for p in mixer.parameters())
print(f"{N}x{N}, Mixer2d(patch {PATCH}, hidden {HIDDEN}, mix {MIX}, {BLOCKS} blocks): {n_par} parameters, "
      f"{len(inds)} trajectories x 100 substeps, {'torch' if '--torch' in sys.argv else 'native'}")

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
