"""Watch the free energy of a spinodal decomposition fall, without reading a field back.

A regular-solution Cahn-Hilliard model (mu_h = log(c / (1 - c)) + 3 (1 - 2c), D = c (1 - c)) is quenched from c = 0.5 plus
noise on a 128^2 periodic grid and integrated with the semi-implicit Fourier solver.  ``PDEModel.free_energy_trace`` runs
the solve of ``PDEModel.solve`` and, at each save point, sums the free energy F = F_bulk + F_grad, the dissipation
-dF/dt and the moments of the chemical potential on the GPU: 64 bytes per environment come back instead of the field.
The sums are consistent with the finite-difference right-hand side, so between two save points F falls by about the
dissipation times the time between them, and the variance of mu tends to 0 as the state approaches a steady one.

The same numbers reward a ``VectorPDEEnv``: ``device_reward=("phase_field", "free_energy")`` evaluates F of every
environment's state after the step, with that environment's controlled kappa.

``--quick`` shrinks the grid to 32^2 (64^2 for the episode) and the run to 400 steps."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # run from a checkout

import numpy as np

from pde_opt_amd import CahnHilliard2DPeriodic, Domain, PDEModel, SemiImplicitFourierSpectral, VectorPDEEnv

quick = "--quick" in sys.argv

N = 32 if quick else 128
STEPS, SAVES, DT = (400, 4, 1e-5) if quick else (5000, 10, 1e-5)
domain = Domain((N, N), ((0.0, 0.01 * N), (0.0, 0.01 * N)), "dimensionless")  # h = 0.01
params = dict(kappa=0.002, mu=lambda c: np.log(c / (1.0 - c)) + 3.0 * (1.0 - 2.0 * c), D=lambda c: c * (1.0 - c))

rng = np.random.default_rng(0)
y0 = (0.5 + 0.02 * rng.standard_normal((2, N, N))).astype(np.float32)  # two quenches, one batch

model = PDEModel(CahnHilliard2DPeriodic, domain, SemiImplicitFourierSpectral)
ts = np.arange(SAVES + 1) * (STEPS // SAVES) * DT  # every save point on a step edge
trace = model.free_energy_trace(params, y0, ts, solver_parameters={"A": 0.5}, dt0=DT)

print(f"{'t':>10} {'free energy':>14} {'dissipation':>14} {'mu variance':>14} {'mean c':>10}")
for q, t in enumerate(ts):
    print(f"{t:10.3e} {trace.free_energy[q, 0]:14.6e} {trace.dissipation[q, 0]:14.6e} {trace.mu_variance[q, 0]:14.6e} {trace.mean[q, 0]:10.6f}")
assert np.all(trace.nonfinite == 0)
assert np.all(trace.free_energy[-1] < trace.free_energy[0]), "the quench lowers the free energy"
assert np.allclose(trace.mean, trace.mean[0], rtol=1e-4), "Cahn-Hilliard conserves the mean concentration"
# F falls at the dissipation rate: the drop over a segment lies between the segment's smallest and largest rate x its length
drop = -np.diff(trace.free_energy[:, 0]) / np.diff(ts)
print("  -dF/dt per segment:", " ".join(f"{v:.4e}" for v in drop))

# ---- one episode rewarded by the free energy ---------------------------------------------------------------------------
B = 4
NE = max(N, 64)  # a per-environment kappa under the semi-implicit solver runs on grids of 64 .. 1024
env_domain = Domain((NE, NE), ((0.0, 0.01 * NE), (0.0, 0.01 * NE)), "dimensionless")
env = VectorPDEEnv(
    B, CahnHilliard2DPeriodic, env_domain, SemiImplicitFourierSpectral, end_time=5 * 20 * DT, step_dt=20 * DT, numeric_dt=DT,
    state_to_observation_func=lambda s: s, reward_function=None,
    reset_func=lambda dom, seed=0: (0.5 + 0.02 * np.random.default_rng(seed).standard_normal(dom.points)).astype(np.float32),
    reset_control_value=0.002, update_control_value=lambda action, old: float(np.clip(old * (1.0 + 0.2 * float(np.ravel(action)[0])), 5e-4, 8e-3)),
    update_control_parameter=lambda old, new: new, action_space_config={"shape": (1,)},
    static_equation_parameters=dict(mu=params["mu"], D=params["D"]), control_equation_parameter_name="kappa",
    solver_parameters={"A": 0.5}, device_reward=("phase_field", "free_energy"), fetch_observations=False)
env.reset(seed=1)
total = np.zeros(B)
for step in range(5):
    actions = rng.uniform(-1.0, 1.0, (B, 1))
    _, rewards, terminated, _, _ = env.step(actions)
    total += -np.asarray(rewards)  # "reach the low-energy state": the reward is -F
    print(f"env step {step}: free energy per environment", " ".join(f"{r:.5e}" for r in rewards))
assert np.all(np.isfinite(total))
env.close()
print("ok")
