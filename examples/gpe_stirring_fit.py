"""How fast was the beam moved, how fast was the trap spun up?  A condensate starts from a known state in a rotating
trap (GPE2DTSRot) whose rotation ramps up, Omega(t) = omega + omega_rate t, while a repulsive laser spot travels through
it (``lights``: a GaussianSpots evaluated in-kernel); only the final state is observed.
``PDEModel.optimize_stirring`` recovers the spot's ``x_rate`` and ``omega_rate`` with BFGS on the gradient of
``PDEModel.stirring_gradient``: a discrete adjoint of the stirred alternating-direction split step on the GPU
(csrc/gpe_rot_adjoint.hip).

    python examples/gpe_stirring_fit.py [--points 64] [--substeps 20]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout

import numpy as np

from pde_opt_amd import Domain, GPE2DTSRot, PDEModel, RotatingStrangSplitting
from pde_opt_amd.numerics.functions.lights import GaussianSpot, GaussianSpots

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=64)
ap.add_argument("--substeps", type=int, default=20)
args = ap.parse_args()

domain = Domain((args.points, args.points), ((-4.0, 4.0), (-4.0, 4.0)), "dimensionless")
X, Y = domain.mesh()
h2 = domain.dx[0] ** 2
psi = (1.0 + 0.6 * X + 0.4j * Y) * np.exp(-((X - 0.5) ** 2 + (Y + 0.3) ** 2) / 2.5)
psi /= np.sqrt(np.sum(np.abs(psi) ** 2) * h2)
y0 = np.stack([psi.real, psi.imag], axis=-1)

FIXED = dict(k=10.0, e=0.1, omega=0.3)
TRUE = dict(omega_rate=0.8, x_rate=1.0)
START = dict(omega_rate=0.5, x_rate=0.7)
DT0 = 0.02
TS = np.array([0.0, args.substeps * DT0])


def beam(x_rate):
    """amplitude 4, width 0.6, starting at (-0.5, 0.3), drifting in y at -0.4; only its speed along x is free"""
    return GaussianSpots([GaussianSpot(4.0, 0.0, -0.5, float(x_rate), 0.3, -0.4, 0.6)], free=("x_rate",))


model = PDEModel(GPE2DTSRot, domain, RotatingStrangSplitting)
target = model.solve(dict(FIXED, omega_rate=TRUE["omega_rate"], lights=beam(TRUE["x_rate"])), y0, TS, dt0=DT0)[-1]


class StateMismatch:
    """h^2 sum |psi_T - target|^2 and its cotangent, in numpy"""

    def value_and_grad(self, ys):
        r = ys[-1] - target
        g = np.zeros_like(ys)
        g[-1] = 2.0 * h2 * r
        return float(h2 * np.sum(r * r)), g


print(f"target: omega_rate = {TRUE['omega_rate']}, x_rate = {TRUE['x_rate']}")
print(f"start : omega_rate = {START['omega_rate']}, x_rate = {START['x_rate']}")
fitted = model.optimize_stirring(StateMismatch(), y0, TS, {"omega_rate": START["omega_rate"], "lights": beam(START["x_rate"])},
                                 FIXED, max_steps=40, dt0=DT0)
hist = model.last_optimize_history
for i, J in enumerate(hist):
    print(f"  iteration {i:2d}: J = {J:.6e}")
got = dict(omega_rate=fitted["omega_rate"], x_rate=fitted["lights"].spots[0].x_rate)
print(f"fitted: omega_rate = {got['omega_rate']:.8f}, x_rate = {got['x_rate']:.8f}")
assert hist[-1] <= 1e-6 * hist[0]
assert abs(got["omega_rate"] - TRUE["omega_rate"]) <= 1e-3 and abs(got["x_rate"] - TRUE["x_rate"]) <= 1e-3
print("ok")
