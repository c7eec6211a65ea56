"""notebooks/run_butler_volmer_sbm.ipynb with the imports switched: a smoothed-boundary disc charged at constant current
under Tsit5 + PIDController(1e-4, 1e-6), then the voltage of every saved frame.

    python examples/butler_volmer_sbm.py            # the notebook: 100^2, t in [0, 10], 200 frames
    python examples/butler_volmer_sbm.py --quick    # a short prefix on 48^2
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout

import numpy as np

from pde_opt_amd import (AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent, Domain, PIDController, SaveAt, Shape, Tsit5,
                         diffeqsolve)

quick = "--quick" in sys.argv
N = 48 if quick else 100
binary_mask = np.zeros((N, N))
y, x = np.ogrid[:N, :N]
binary_mask[np.sqrt((x - N // 2) ** 2 + (y - N // 2) ** 2) <= 0.3 * N] = 1
shape = Shape(binary=binary_mask, dx=(1.0, 1.0), smooth_epsilon=3.0, smooth_curvature=0.008, smooth_dt=0.01,
              smooth_tf=20.0 if quick else 100.0)

Lx = Ly = 0.01 * N
domain = Domain((N, N), ((-Lx / 2, Lx / 2), (-Ly / 2, Ly / 2)), "dimensionless", shape)
t_final, frames = (0.5, 6) if quick else (10.0, 200)
ts_save = np.linspace(0.0, t_final, frames)

eq = AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent(
    domain,
    0.002,
    lambda c: c * np.log(c) + (1.0 - c) * np.log(1.0 - c) + 3.0 * c * (1.0 - c) + 0.059,
    lambda c: np.log(c / (1.0 - c)) + 3.0 * (1.0 - 2.0 * c),
    lambda c: np.sqrt((1.0 - c) * c),
    0.5,
    0.02,
    derivs="fd",
)

u0 = np.clip(0.1 + 0.1 * np.random.default_rng(0).standard_normal((N, N)), 0.05, 1.0)
solution = diffeqsolve(eq, Tsit5(), t0=0.0, t1=t_final, dt0=1e-6, y0=u0,
                       stepsize_controller=PIDController(rtol=1e-4, atol=1e-6), saveat=SaveAt(ts=ts_save), max_steps=1000000)
psi = np.asarray(domain.geometry.smooth)
filling = np.sum(solution.ys * psi[None], axis=(1, 2)) / np.sum(psi)
voltages = eq.get_voltage(solution.ys)  # the notebook's jax.vmap(eq.get_voltage)(solution.ys)
print(f"{solution.stats['num_accepted_steps']} accepted, {solution.stats['num_rejected_steps']} rejected steps; kernel {solution.stats['kernel']}")
for t, c, v in zip(solution.ts, filling, voltages):
    print(f"t = {t:7.3f}   filling {c:.5f}   voltage {v:+.5f}")
assert np.all(np.isfinite(solution.ys)) and np.all(np.isfinite(voltages))
assert np.all(np.diff(filling) > 0)  # constant charging current
print("ok")
