"""The optimisation case of tests/test_gpu_gpe_adjoint.py: one repulsive spot whose position is free, the target the final
density for a known position.  A helper, not a test.  Chosen on the CPU so that the reference gradient
(tests/gpe_adjoint_ref.py at complex128) driving fit.minimize_bfgs lowers J more than 100-fold within MAX_STEPS:
``PYTHONPATH=. python tests/gpe_control_problem.py`` prints that run."""
import functools

import numpy as np
import torch

import pde_opt_amd as P
from pde_opt_amd.gpe_control import SpotMap
from pde_opt_amd.numerics.functions.lights import GaussianSpots
from pde_opt_amd.utils import prepare_solver_params

POINTS, BOX = (64, 64), ((-4.0, 4.0), (-4.0, 4.0))
# PDEModel.optimize steps with dt0 = 1e-6 (its default, as solve's): time_scale carries the imaginary-time step 0.05
SOLVER_PARAMETERS = {"time_scale": -5e4j}
DT0 = 1e-6
TS = np.array([0.0, 10e-6])
AMP, WIDTH = 3.0, 0.7
TRUE_XY, START_XY = (0.6, -0.4), (0.1, 0.2)
MAX_STEPS = 8
# final J of the CPU reference run below: 2.743072e-02 at the start, 8 accepted steps (20 steps reach 2.0e-22)
REFERENCE_FINAL_J = 2.815316e-09


def domain():
    return P.Domain(POINTS, BOX, "dimensionless")


def other_parameters():
    return dict(k=1.0, e=0.0, trap_factor=1.0, kinetic=True)


def spots_at(xy, free=("x0", "y0")):
    s = GaussianSpots.single(AMP, xy[0], xy[1], WIDTH)
    return GaussianSpots(s.spots, free=free)


def start_spots():
    return spots_at(START_XY)


def y0():
    X, Y = domain().mesh()
    psi = np.exp(-0.5 * (X**2 + Y**2))
    psi = psi / np.sqrt(np.sum(psi**2) * domain().dx[0] ** 2)
    return np.stack([psi, np.zeros_like(psi)], axis=-1)


def reference_case():
    import gpe_adjoint_ref as R

    eq = P.GPE2DTSControl(domain(), lights=start_spots(), **other_parameters())
    solver = P.StrangSplitting(**prepare_solver_params(P.StrangSplitting, SOLVER_PARAMETERS, eq))
    return R.Case.of(eq, solver)


@functools.lru_cache(maxsize=None)
def target():
    import gpe_adjoint_ref as R

    p = SpotMap(1).flatten(spots_at(TRUE_XY)).reshape(1, 7)
    ys = R.solve(reference_case(), torch.as_tensor(y0()), torch.as_tensor(p), TS, DT0)
    return (ys[-1, ..., 0] ** 2 + ys[-1, ..., 1] ** 2).detach()


def objective(ys):
    dens = ys[-1, ..., 0] ** 2 + ys[-1, ..., 1] ** 2
    return ((dens - target()) ** 2).sum() * domain().dx[0] ** 2


def reference_run():
    """fit.minimize_bfgs over the free numbers with the CPU reference's gradient: the history of J"""
    import gpe_adjoint_ref as R
    from pde_opt_amd import fit

    case, smap = reference_case(), SpotMap.of(start_spots())
    active = smap.active().reshape(-1)

    def vg(p):
        J, _, g, _ = R.solve_grad(case, y0(), p.reshape(1, 7), TS, DT0, objective)
        return J, g.reshape(-1) * active

    return fit.minimize_bfgs(vg, lambda p: vg(p)[0], smap.flatten(start_spots()), max_steps=MAX_STEPS)


if __name__ == "__main__":
    p, hist = reference_run()
    print("J per accepted step:", " ".join(f"{v:.6e}" for v in hist))
    print("fitted:", p)
