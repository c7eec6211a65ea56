"""Fit the gradient-energy coefficient kappa together with the chemical potential with PDEModel.train.

kappa sets the interface width of a phase-field model.  It is a scalar of the equation, not a closure coefficient: it is
made trainable by wrapping it, ``opt_parameters={"kappa": TrainableScalar(0.003), ...}`` (a plain float stays fixed data).
The optimiser moves log(kappa), so kappa stays positive whatever step it takes.

Synthetic data: two 64^2 trajectories of CahnHilliard2DPeriodic under the semi-implicit Fourier solver with kappa = 0.002
and mu = logit + Legendre series (0, -3, 0.3).  The fit starts from kappa = 0.003 and wrong mu coefficients and recovers
kappa and the two mu coefficients that move the solution (a constant added to mu does not) by Levenberg-Marquardt on GPU
forward-mode sensitivities.  Under IMEX kappa also moves the implicit operator 1 + A dt kappa K2^2; the sensitivity solve
differentiates that too.  One call of ``train`` per iteration, restarted from the last result, to print kappa as it moves.

``--quick`` shrinks the grid to 32^2, the data window to 100 substeps and the fit to 4 iterations."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout
import time

import numpy as np

from pde_opt_amd import CahnHilliard2DPeriodic, Domain, PDEModel, SemiImplicitFourierSpectral
from pde_opt_amd.numerics.functions import TrainableScalar
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials, DiffusionLegendrePolynomials

quick = "--quick" in sys.argv

N = 32 if quick else 64
domain = Domain((N, N), ((-0.005 * N, 0.005 * N), (-0.005 * N, 0.005 * N)), "dimensionless")  # h = 0.01
model = PDEModel(equation_type=CahnHilliard2DPeriodic, domain=domain, solver_type=SemiImplicitFourierSpectral)
solver_parameters = {"A": 0.5}


def logit(c):
    return np.log(c / (1.0 - c))


KAPPA_TRUE, KAPPA_START = 0.002, 0.003
mu_true = np.array([0.0, -3.0, 0.3])
D = DiffusionLegendrePolynomials(np.array([-1.0, 0.2]))
truth = {"kappa": KAPPA_TRUE, "mu": ChemicalPotentialLegendrePolynomials(mu_true, logit), "D": D}

rng = np.random.default_rng(0)
x = np.arange(N) / N


def smooth_state():
    u = 0.5 + np.zeros((N, N))
    for _ in range(6):
        kx, ky = rng.integers(1, 4, 2)
        u += 0.04 * rng.standard_normal() * np.cos(2 * np.pi * (kx * x[:, None] + ky * x[None, :]) + rng.uniform(0, 6))
    return u


# two trajectories, each observed at two later times (dt0 = 1e-6, the step PDEModel.train uses)
B = 2
ts = np.array([0.0, 0.5, 1.0]) * (1e-4 if quick else 4e-4)
y0s = np.stack([smooth_state() for _ in range(B)])
t0 = time.perf_counter()
sol = model.solve(truth, y0s, ts, solver_parameters)  # (T, B, N, N)
print(f"data: {B} trajectories of {N}x{N}, {len(ts) - 1} frames up to t = {ts[-1]:g}, {time.perf_counter() - t0:.2f} s")

data = {"ys": [sol[q, b] for b in range(B) for q in range(len(ts))], "ts": np.tile(ts, B)}
inds = [[b * len(ts) + q for q in range(len(ts))] for b in range(B)]

fitted = {"kappa": TrainableScalar(KAPPA_START), "mu": ChemicalPotentialLegendrePolynomials(np.array([0.0, -2.6, 0.2]), logit)}
print(f"iteration 0: kappa = {fitted['kappa'].value:.6e}, mu = {np.asarray(fitted['mu'].expansion.params)}")
t0 = time.perf_counter()
first = last = None
for it in range(1, (4 if quick else 12) + 1):
    res = model.train(data, inds, fitted, {"D": D}, solver_parameters, {}, 0.0, method="least_squares", max_steps=1)
    fitted = {"kappa": res["kappa"], "mu": res["mu"]}
    hist = model.last_train_history
    first, last = hist[0] if first is None else first, hist[-1]
    print(f"iteration {it}: kappa = {fitted['kappa'].value:.6e}, mu = {np.round(np.asarray(fitted['mu'].expansion.params), 6)}, "
          f"objective {hist[-1]:.3e}")
    if hist[-1] <= 1e-24:
        break
print(f"{time.perf_counter() - t0:.2f} s; objective {first:.3e} -> {last:.3e}")
kappa_fit = fitted["kappa"].value
print(f"kappa: start {KAPPA_START}, fitted {kappa_fit:.9e}, true {KAPPA_TRUE}")
print(f"mu: fitted {np.round(np.asarray(fitted['mu'].expansion.params), 9)}, true {mu_true}")
# the fitted dict goes back into solve as it is
check = model.solve({**fitted, "D": D}, y0s, ts, solver_parameters)
print(f"max |solve(fitted) - data| = {np.max(np.abs(check - sol)):.3e}")
if not np.isfinite(kappa_fit) or not abs(kappa_fit - KAPPA_TRUE) < abs(KAPPA_START - KAPPA_TRUE):
    sys.exit("the fitted kappa is not closer to the truth than the start")
print(f"KAPPA_FIT {kappa_fit!r}")
