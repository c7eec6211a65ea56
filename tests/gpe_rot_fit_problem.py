"""The optimisation case of tests/test_gpu_gpe_rot_adjoint.py: recover the rotation frequency that took a known start
state to a given final state.  A helper, not a test.  Confirmed on the CPU: the reference gradient
(tests/gpe_rot_adjoint_ref.py at complex128) driving fit.minimize_bfgs meets both bounds of the test, J_final <=
1e-6 J_initial and |omega - OMEGA_TRUE| <= 1e-3, on this horizon and start;
``PYTHONPATH=. python tests/gpe_rot_fit_problem.py`` prints that run."""
import functools

import numpy as np
import torch

import pde_opt_amd as P

import gpe_rot_ref as RR

POINTS, BOX = (64, 64), ((-4.0, 4.0), (-4.0, 4.0))
K_GPE, E_GPE = 10.0, 0.1
OMEGA_TRUE, OMEGA_START = 0.6, 0.45
DT0 = 0.02
TS = np.array([0.0, 10 * DT0])  # 10 substeps
MAX_STEPS = 30
# the CPU reference run below: J 1.941959e-03 at the start, 2.8e-30 after 5 accepted steps, omega 0.6 to 1e-16


def domain():
    return P.Domain(POINTS, BOX, "dimensionless")


def y0():
    return RR.to_pairs(RR.smooth_state(domain(), 5)[0])


def parameters(omega):
    return dict(k=K_GPE, e=E_GPE, omega=float(omega))


@functools.lru_cache(maxsize=None)
def target():
    import gpe_rot_adjoint_ref as A

    p = torch.tensor([[K_GPE, E_GPE, OMEGA_TRUE]], dtype=torch.float64)
    return A.solve(A.Case(domain()), torch.as_tensor(y0()[None]), p, TS, DT0)[-1, 0].detach()


def objective(ys):
    """h^2 sum |psi_T - target|^2 of one state (ys: (len(TS), nx, ny, 2))"""
    return ((ys[-1] - target()) ** 2).sum() * domain().dx[0] ** 2


def reference_run():
    """fit.minimize_bfgs over omega with the CPU reference's gradient: (omega, the history of J)"""
    import gpe_rot_adjoint_ref as A
    from pde_opt_amd import fit

    case = A.Case(domain())

    def vg(p):
        J, _, g, _ = A.solve_grad(case, y0()[None], [[K_GPE, E_GPE, p[0]]], TS, DT0, lambda ys: objective(ys[:, 0]))
        return J, g[0, 2:3]

    return fit.minimize_bfgs(vg, lambda p: vg(p)[0], np.array([OMEGA_START]), max_steps=MAX_STEPS)


if __name__ == "__main__":
    p, hist = reference_run()
    print("J per accepted step:", " ".join(f"{v:.6e}" for v in hist))
    print("fitted omega:", p, "error", abs(p[0] - OMEGA_TRUE))
