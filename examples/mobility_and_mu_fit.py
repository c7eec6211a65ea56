"""Fit the chemical potential AND the mobility of Cahn-Hilliard when neither is known (the reference's
``train(..., init_params={"mu": model, "D": DiffusionLegendrePolynomials(...)}, method="mse")``: both are leaves of one
pytree there).

Frames are generated on a small grid from a known ``mu`` (Legendre series under the logit prior) and a known
``D = exp(Legendre)``.  A small ``PeriodicCNN`` then takes the place of ``mu`` and a two-coefficient ``D`` starts from the
wrong values; ``PDEModel.train`` runs BFGS over the flat vector [CNN parameters, D coefficients].  One backward sweep
gives both gradients: the adjoint kernel that hands the network its cotangent also sums the cotangent of ``D`` against
the Legendre basis (csrc/fieldmu.hip, ``pdeopt_fieldmu_adjoint_step_coef``).  The network and its vector-Jacobian product
run in the library's own kernels (``native_cnn``); ``--torch`` leaves them to torch.

``--quick`` runs 10 BFGS steps instead of 40."""
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
NX, NY, STEPS = 16, 32, (10 if quick else 40)

domain = Domain((NX, NY), ((0.0, 0.01 * NX), (0.0, 0.01 * NY)), "dimensionless")
model = PDEModel(equation_type=CahnHilliard2DPeriodic, domain=domain, solver_type=SemiImplicitFourierSpectral)


def logit(c):
    return np.log(c / (1.0 - c))


KAPPA = 0.002
D_TRUE = np.array([-0.3, 0.2])
truth = {"kappa": KAPPA, "mu": ChemicalPotentialLegendrePolynomials(np.array([0.0, -3.0, 0.4]), logit),
         "D": DiffusionLegendrePolynomials(D_TRUE)}
y0 = np.clip(0.5 + 0.05 * np.random.default_rng(0).standard_normal((NX, NY)), 0.05, 0.95)
ts = np.linspace(0.0, 8e-5, 5)  # 5 frames, 20 substeps apart
data = {"ys": list(model.solve(truth, y0, ts, {"A": 0.5})), "ts": list(ts)}
inds = [[1, 2, 3], [2, 3, 4]]  # two trajectories: from frames 1 and 2, each compared with the two frames that follow

torch.manual_seed(0)
cnn = PeriodicCNN(1, (4,), 1).double().to("cuda")
model.fieldmu_solver().native_cnn = "--torch" not in sys.argv
D_start = DiffusionLegendrePolynomials(np.array([0.0, 0.0]))
n_par = sum(p.numel() for p in cnn.parameters())
print(f"{NX}x{NY}, PeriodicCNN(1, (4,), 1): {n_par} parameters + {len(D_TRUE)} coefficients of D, {len(inds)} trajectories x 40 "
      f"substeps, {'torch' if '--torch' in sys.argv else 'native'}")

t0 = time.perf_counter()
fitted = model.train(data, inds, {"mu": cnn, "D": D_start}, {"kappa": KAPPA}, {"A": 0.5}, {}, 0.0, method="mse", max_steps=STEPS)
hist = model.last_train_history
for it in range(0, len(hist), max(1, len(hist) // 10)):
    print(f"  step {it:4d}  mse {hist[it]:.6e}")
print(f"D coefficients {D_start.expansion.params} -> {fitted['D'].expansion.params} (the frames were made with {D_TRUE})")
print(f"loss {hist[0]:.6e} -> {hist[-1]:.6e} in {len(hist) - 1} BFGS steps, {time.perf_counter() - t0:.1f} s")
if not (np.isfinite(hist[-1]) and hist[-1] < hist[0]):
    sys.exit("the loss did not decrease")
