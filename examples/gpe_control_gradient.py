"""Gradient-based laser control of a condensate: steer one repulsive Gaussian spot so that the final density of an
imaginary-time Gross-Pitaevskii solve overlaps a displaced target.

    python examples/gpe_control_gradient.py [--quick]

``PDEModel.optimize`` drives BFGS over the spot's position with the reverse-mode gradient of
``PDEModel.control_gradient`` (a discrete adjoint of the Strang split step on the GPU).  The target is the final density
for a spot at a known position, so the optimum is J = 0 at that position.  Prints J after every accepted step.
"""
import argparse

import numpy as np

import pde_opt_amd as P
from pde_opt_amd.numerics.functions.lights import GaussianSpots

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="64 x 64 grid and 6 BFGS steps instead of 128 x 128 and 20")
args = ap.parse_args()

n = 64 if args.quick else 128
domain = P.Domain((n, n), ((-4.0, 4.0), (-4.0, 4.0)), "dimensionless")
model = P.PDEModel(P.GPE2DTSControl, domain, P.StrangSplitting)
other = dict(k=1.0, e=0.0, trap_factor=1.0, kinetic=True)
# optimize steps with solve's default dt0 = 1e-6: time_scale turns that into an imaginary-time step of 0.05
solver_parameters = {"time_scale": -5e4j}
ts = np.array([0.0, 10e-6])


def spot(x, y):
    return GaussianSpots(GaussianSpots.single(3.0, x, y, 0.7).spots, free=("x0", "y0"))


X, Y = domain.mesh()
psi = np.exp(-0.5 * (X**2 + Y**2))
psi /= np.sqrt(np.sum(psi**2) * domain.dx[0] ** 2)
y0 = np.stack([psi, np.zeros_like(psi)], axis=-1)

true_xy, start_xy = (0.6, -0.4), (0.1, 0.2)
final = model.solve(dict(other, lights=spot(*true_xy)), y0, ts, solver_parameters)[-1]
target = final[..., 0] ** 2 + final[..., 1] ** 2
h2 = domain.dx[0] ** 2


class Overlap:
    """J = h^2 sum (|psi(T)|^2 - target)^2 and its cotangent dJ/dys"""

    def value_and_grad(self, ys):
        d = ys[-1, ..., 0] ** 2 + ys[-1, ..., 1] ** 2 - target
        g = np.zeros_like(ys, dtype=np.float64)
        g[-1] = 4.0 * h2 * d[..., None] * ys[-1]
        return float(h2 * np.sum(d * d)), g


J0, grad, _ = model.control_gradient(Overlap(), y0, ts, dict(other, lights=spot(*start_xy)), solver_parameters)
print(f"start {start_xy}: J = {J0:.6e}, dJ/d(x0, y0) = ({grad[0, 2]:+.4e}, {grad[0, 4]:+.4e})")
fitted = model.optimize(Overlap(), y0, ts, {"lights": spot(*start_xy)}, other, solver_parameters, max_steps=6 if args.quick else 20)
for i, J in enumerate(model.last_optimize_history):
    print(f"step {i}: J = {J:.6e}")
s = fitted["lights"].spots[0]
print(f"fitted position ({s.x0:+.5f}, {s.y0:+.5f}), true {true_xy}")
