"""The optimisation case of tests/test_gpu_gpe_rot_stir_adjoint.py: recover the spin-up rate and the speed of the stirring
beam that took a known start state to a given final state.  A helper, not a test.  Confirmed on the CPU: the reference
gradient (tests/gpe_rot_stir_adjoint_ref.py at complex128) driving fit.minimize_bfgs over (omega_rate, x_rate) meets the
bounds of the test, J_final <= 1e-6 J_initial and both numbers to 1e-3, on this horizon and start;
``PYTHONPATH=. python tests/gpe_rot_stir_fit_problem.py`` prints that run."""
import functools

import numpy as np
import torch

import pde_opt_amd as P
from pde_opt_amd.numerics.functions.lights import GaussianSpot, GaussianSpots

import gpe_rot_ref as RR

POINTS, BOX = (64, 64), ((-4.0, 4.0), (-4.0, 4.0))
K_GPE, E_GPE, OMEGA = 10.0, 0.1, 0.3
RATE_TRUE, RATE_START = 0.8, 0.5
XRATE_TRUE, XRATE_START = 1.0, 0.7
AMP, X0, Y0, YRATE, WIDTH = 4.0, -0.5, 0.3, -0.4, 0.6  # the beam's fixed numbers
DT0 = 0.02
TS = np.array([0.0, 20 * DT0])  # 20 substeps
MAX_STEPS = 40
# the CPU reference run below: J 2.914244e-03 at the start, 1.192048e-06 after 2 accepted steps, 3.4e-22 after 13;
# omega_rate 0.8 to 1.6e-10, x_rate 1.0 to 1.2e-11


def domain():
    return P.Domain(POINTS, BOX, "dimensionless")


def y0():
    return RR.to_pairs(RR.smooth_state(domain(), 5)[0])


def lights(x_rate):
    """the beam with a given speed along x; only x_rate is free"""
    return GaussianSpots([GaussianSpot(AMP, 0.0, X0, float(x_rate), Y0, YRATE, WIDTH)], free=("x_rate",))


def fixed():
    return dict(k=K_GPE, e=E_GPE, omega=OMEGA)


def _row(x_rate):
    return torch.tensor([[list(lights(x_rate).spots[0].row())]], dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def target():
    import gpe_rot_stir_adjoint_ref as A

    p = torch.tensor([[K_GPE, E_GPE, OMEGA, RATE_TRUE]], dtype=torch.float64)
    return A.solve(A.Case(domain()), torch.as_tensor(y0()[None]), p, _row(XRATE_TRUE), TS, DT0)[-1, 0].detach()


def objective(ys):
    """h^2 sum |psi_T - target|^2 of one state (ys: (len(TS), nx, ny, 2))"""
    return ((ys[-1] - target()) ** 2).sum() * domain().dx[0] ** 2


def reference_run():
    """fit.minimize_bfgs over (omega_rate, x_rate) with the CPU reference's gradient: (the two numbers, the history of J)"""
    import gpe_rot_stir_adjoint_ref as A
    from pde_opt_amd import fit

    case = A.Case(domain())

    def vg(p):
        J, _, g, gs, _ = A.solve_grad(case, y0()[None], [[K_GPE, E_GPE, OMEGA, p[0]]], _row(p[1]).numpy(), TS, DT0,
                                      lambda ys: objective(ys[:, 0]))
        return J, np.array([g[0, 3], gs[0, 0, 3]])

    return fit.minimize_bfgs(vg, lambda p: vg(p)[0], np.array([RATE_START, XRATE_START]), max_steps=MAX_STEPS)


if __name__ == "__main__":
    p, hist = reference_run()
    print("J per accepted step:", " ".join(f"{v:.6e}" for v in hist))
    print("fitted (omega_rate, x_rate):", p, "errors", abs(p[0] - RATE_TRUE), abs(p[1] - XRATE_TRUE))
