"""Ground states through ``PDEModel.ground_state``: imaginary time until the energy per particle stands still, with the
energy, the chemical potential and L_z summed on the GPU (64 bytes per look instead of the field).

1. The Thomas-Fermi problem of examples/thomas_fermi.py in dimensionless form: a trapped condensate with strong
   repulsion; its chemical potential approaches sqrt(k / pi).
2. A condensate in a rotating, slightly elliptic trap (GPE2DTSRot), two rotation frequencies relaxed side by side as
   one batch.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout

import numpy as np

from pde_opt_amd import Domain, GPE2DTSControl, GPE2DTSRot, PDEModel, RotatingStrangSplitting, StrangSplitting

domain = Domain((128, 128), ((-8.0, 8.0), (-8.0, 8.0)), "dimensionless")
X, Y = domain.mesh()
start = np.exp(-((X - 0.7) ** 2 + (Y + 0.4) ** 2) / 3)
y0 = np.stack([start, 0 * start], axis=-1)


def report(tag, gs, b=0):
    o = gs.observables
    print(f"{tag}: {int(gs.steps[b])} steps, converged {bool(gs.converged[b])}, energy {o.energy[b]:.8f}, mu {o.mu[b]:.8f}, "
          f"L_z {o.l_z[b] / o.norm[b]:+.6f}, norm {o.norm[b]:.6f}")


# 1. Thomas-Fermi
k = 500.0
model = PDEModel(GPE2DTSControl, domain, StrangSplitting)
gs = model.ground_state(dict(k=k, e=0.0, lights=lambda t, x, y: 0.0 * x, kinetic=True), y0, dt=2e-3, tol=1e-6, max_steps=20_000)
report("Thomas-Fermi", gs)
mu_tf = np.sqrt(k / np.pi)
print(f"  mu / mu_TF = {gs.observables.mu[0] / mu_tf:.4f}")
assert gs.converged[0] and abs(gs.observables.mu[0] / mu_tf - 1.0) < 0.1
assert np.all(np.diff(gs.history[:, 0, 0]) <= 1e-9)  # imaginary time never raises the energy

# 2. two rotation frequencies, one batch
model = PDEModel(GPE2DTSRot, domain, RotatingStrangSplitting)
omegas = (0.0, 0.3)
gs = model.ground_state([dict(k=100.0, e=0.1, omega=w) for w in omegas], np.stack([y0, y0]), dt=2e-3, tol=1e-6,
                        max_steps=20_000)
for b, w in enumerate(omegas):
    report(f"rotating trap, omega = {w}", gs, b)
assert np.all(np.isfinite(gs.history)) and np.all(np.diff(gs.history[:, :, 0], axis=0) <= 1e-9)
print("ok")
