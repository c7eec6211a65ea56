"""Watch a spinodal decomposition coarsen: the length L(t) = 2 pi / <k> from the structure factor, no field read back.

A regular-solution Cahn-Hilliard model (mu_h = log(c / (1 - c)) + 3 (1 - 2c), D = c (1 - c)) is quenched from c = 0.5 plus
noise on a 256^2 periodic grid and integrated with the semi-implicit Fourier solver.  ``PDEModel.structure_factor_trace``
runs the solve of ``PDEModel.solve`` and, at each save point, transforms the resident state and sums |u^|^2 over shells
of width dk = 2 pi / L_box on the GPU: one row of shell sums per environment comes back instead of the field.  The host
normalises them to S(k) and takes the first moment <k> = sum k S / sum S.  The save points double in time, so the slope
of log L over log t between them is the coarsening exponent; late-stage Cahn-Hilliard coarsening tends to 1/3 (with the
degenerate mobility used here, transport along the interfaces slows it towards 1/4).

``--quick`` shrinks the grid to 128^2 and the run to 51200 steps (one doubling fewer)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout

import numpy as np

from pde_opt_amd import CahnHilliard2DPeriodic, Domain, PDEModel, SemiImplicitFourierSpectral

quick = "--quick" in sys.argv

N, FIRST, DOUBLINGS, DT = (128, 3200, 4, 1e-5) if quick else (256, 3200, 5, 1e-5)
domain = Domain((N, N), ((0.0, 0.01 * N), (0.0, 0.01 * N)), "dimensionless")  # h = 0.01
params = dict(kappa=0.002, mu=lambda c: np.log(c / (1.0 - c)) + 3.0 * (1.0 - 2.0 * c), D=lambda c: c * (1.0 - c))

rng = np.random.default_rng(0)
y0 = (0.5 + 0.02 * rng.standard_normal((2, N, N))).astype(np.float32)  # two quenches, one batch

model = PDEModel(CahnHilliard2DPeriodic, domain, SemiImplicitFourierSpectral)
steps = np.concatenate([[0], FIRST * 2 ** np.arange(DOUBLINGS + 1)])
ts = steps * DT  # every save point on a step edge
trace = model.structure_factor_trace(params, y0, ts, solver_parameters={"A": 0.5}, dt0=DT)

print(f"{'t':>10} {'length':>12} {'<k>':>12} {'sqrt<k^2>':>12} {'variance':>12}")
for q, t in enumerate(ts):
    print(f"{t:10.3e} {trace.length[q, 0]:12.5e} {trace.k1[q, 0]:12.5e} {trace.k2[q, 0]:12.5e} {trace.variance[q, 0]:12.5e}")
assert np.all(np.isfinite(trace.length))
assert np.all(np.diff(trace.length, axis=0) > 0), "the pattern coarsens: the length grows from save point to save point"
late = slice(-4, None)
for b in range(y0.shape[0]):
    exponent = np.polyfit(np.log(ts[late]), np.log(trace.length[late, b]), 1)[0]
    print(f"quench {b}: length ~ t^{exponent:.3f} over the last {len(ts[late])} save points")
    assert exponent > 0
peak = trace.k[np.argmax(trace.s[-1, 0])]
print(f"S(k) of quench 0 peaks at k = {peak:.4g} (wave length {2 * np.pi / peak:.4g}) at t = {ts[-1]:.3g}")
print("ok")
