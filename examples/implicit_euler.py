"""Implicit Euler by Newton-GMRES: upstream's notebooks/test_implicit.ipynb with the imports switched
(``diffrax.ImplicitEuler`` + Newton + ``lineax.GMRES``  ->  ``pde_opt_amd.ImplicitEuler``).

First half: Cahn-Hilliard on a 64^2 periodic grid with mu_h = c^3 - c, once with ``ImplicitEuler`` and once with
``SemiImplicitFourierSpectral``, both to the same time: the step counts and the rms difference of the two solutions.
Second half: Allen-Cahn on a 128^2 grid with the logarithmic potential mu_h = log(c / (1 - c)) + 3 (1 - 2c) and a constant
rate R, under ``ImplicitEuler`` with a fixed step: min / max / mean per save point and the iteration counts of the solve.

``--quick`` shrinks both runs (32^2 / 64^2, fewer steps)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout

import numpy as np

from pde_opt_amd import (AllenCahn2DPeriodic, CahnHilliard2DPeriodic, Domain, ImplicitEuler, SaveAt,
                         SemiImplicitFourierSpectral, diffeqsolve)
from pde_opt_amd.utils import prepare_solver_params

quick = "--quick" in sys.argv
rng = np.random.default_rng(0)

# ---- Cahn-Hilliard: implicit Euler next to the semi-implicit Fourier step ------------------------------------------------
N = 32 if quick else 64
domain = Domain((N, N), ((0.0, 0.01 * N), (0.0, 0.01 * N)), "dimensionless")  # h = 0.01
eq = CahnHilliard2DPeriodic(domain, 0.002, lambda c: c**3 - c, lambda c: 1.0)
y0 = 0.05 * rng.standard_normal((N, N))
DT_IMEX, DT_IMPLICIT = 1e-6, 2e-5
T = (5 if quick else 20) * DT_IMPLICIT
implicit = diffeqsolve(eq, ImplicitEuler(rtol=1e-8, atol=1e-10), t0=0.0, t1=T, dt0=DT_IMPLICIT, y0=y0)
imex = diffeqsolve(eq, SemiImplicitFourierSpectral(**prepare_solver_params(SemiImplicitFourierSpectral, {"A": 0.5}, eq)),
                   t0=0.0, t1=T, dt0=DT_IMEX, y0=y0)
diff = float(np.sqrt(np.mean((implicit.ys[-1] - imex.ys[-1]) ** 2)))
print(f"Cahn-Hilliard {N}x{N} to t = {T:.1e}")
print(f"  ImplicitEuler               {implicit.stats['num_steps']:5d} steps of {DT_IMPLICIT:.0e}   {implicit.stats['implicit_totals']}")
print(f"  SemiImplicitFourierSpectral {imex.stats['num_steps']:5d} steps of {DT_IMEX:.0e}")
print(f"  rms difference {diff:.3e}   (rms of the solution {float(np.sqrt(np.mean(imex.ys[-1] ** 2))):.3e})")
assert np.isfinite(implicit.ys).all() and diff < 0.1 * float(np.sqrt(np.mean(imex.ys[-1] ** 2)))
assert abs(float(implicit.ys[-1].mean()) - float(y0.mean())) < 1e-12, "Cahn-Hilliard conserves the mean"
# the same solve with the spectral preconditioner: the same solution to the Newton tolerance, in far fewer Krylov iterations
pre = diffeqsolve(eq, ImplicitEuler(rtol=1e-8, atol=1e-10, precond="spectral"), t0=0.0, t1=T, dt0=DT_IMPLICIT, y0=y0)
pdiff = float(np.sqrt(np.mean((pre.ys[-1] - implicit.ys[-1]) ** 2)))
print(f"  ImplicitEuler(precond=\"spectral\") {pre.stats['implicit_totals']}, "
      f"{sum(pre.stats['preconditioner_applications'])} applications of M^-1; rms distance from the unpreconditioned solve {pdiff:.3e}")
assert pre.stats["implicit_totals"]["krylov_iterations"] < implicit.stats["implicit_totals"]["krylov_iterations"]
assert pdiff < 1e-6 and abs(float(pre.ys[-1].mean()) - float(y0.mean())) < 1e-12

# ---- Allen-Cahn with the logarithmic potential -------------------------------------------------------------------------
M = 64 if quick else 128
domain = Domain((M, M), ((0.0, 0.01 * M), (0.0, 0.01 * M)), "dimensionless")
eq = AllenCahn2DPeriodic(domain, 0.002, lambda c: np.log(c / (1.0 - c)) + 3.0 * (1.0 - 2.0 * c), lambda c: 1.0)
y0 = 0.5 + 0.05 * rng.standard_normal((M, M))
DT, SAVES, PER_SAVE = 0.02, 5, (1 if quick else 4)
ts = [DT * PER_SAVE * (q + 1) for q in range(SAVES)]
sol = diffeqsolve(eq, ImplicitEuler(rtol=1e-8, atol=1e-10), t0=0.0, t1=ts[-1], dt0=DT, y0=y0, saveat=SaveAt(ts=ts))
print(f"Allen-Cahn {M}x{M}, logarithmic potential, {sol.stats['num_steps']} implicit Euler steps of {DT}")
print(f"{'t':>8} {'min':>10} {'max':>10} {'mean':>10}")
for t, y in zip(sol.ts, sol.ys):
    print(f"{t:8.3f} {y.min():10.6f} {y.max():10.6f} {y.mean():10.6f}")
print("stats:", {k: sol.stats[k] for k in ("newton_iterations", "krylov_iterations", "operator_applications", "rhs_evaluations")})
assert np.isfinite(sol.ys).all() and 0.0 < sol.ys.min() and sol.ys.max() < 1.0
print("ok")
