"""The synthetic smoothed-boundary fitting problems of tests/test_gpu_sbm_fit.py, and the same fits on the CPU: fp64 numpy
tangents (tests/sbm_sens_ref.py) under fit.levenberg_marquardt.  Test infrastructure only.

    python tests/sbm_fit_problem.py      # prints the CPU fits' coefficient error and final ssr / M

The GPU test gates PDEModel.train at 10 x the values this prints (they are written next to the gates)."""
import os
import sys

import numpy as np

DT0 = 1e-6                                  # PDEModel.train's step size
TS = np.array([0.0, 1e-4, 2e-4])            # 200 RK4 substeps, 2 observed frames
KAPPA = 1.5
# the second closure is exp-wrapped: exp(6.9 + ...) ~ 1000 is the rate that makes 2e-4 a long time on a unit-spacing grid
# (dt0 R = 1e-3: inside the explicit bound checked for dt = 2^-8 / 2^-9 at rates of O(1) in tests/test_sbm_sens_cpu.py)
PROBLEMS = {
    # eq: (points, mu_true, mob_true, mu_init, mob_init)
    "ac": ((32, 120), (0.1, -3.0, 0.3), (6.9, 0.3), (0.0, -2.6, 0.2), (6.7, 0.2)),
    "ch": ((67, 40), (0.0, -3.0, 0.3), (6.9, 0.3), (0.0, -2.6, 0.2), (6.7, 0.2)),
}
SEEDS = (21, 22)


def logit(c):
    return np.log(c / (1.0 - c))


def theta_poly(t):  # a ramp: a polynomial in t (the in-kernel form)
    return np.pi / 2 - 2000.0 * t


def theta_callable(t):  # the same ramp bent by a sine: no polynomial, evaluated on the host per stage time
    return np.pi / 2 - 0.4 * np.sin(5000.0 * t)


def flux(t):
    return 0.02 * (1.0 + 3000.0 * t)


def y0s(eq):
    import sbm_sens_problem as Q

    return np.stack([Q.smooth_state(PROBLEMS[eq][0], s) for s in SEEDS])


def active(eq):
    """the (role, coefficient) pairs with a tangent: mu's constant is inert for Cahn-Hilliard"""
    import sbm_sens_ref as S

    mu = [(S.MU_ROLE, k) for k in range(3) if not (eq == "ch" and k == 0)]
    return mu + [(S.MOB_ROLE, 0), (S.MOB_ROLE, 1)]


def reference_problem(eq, p, theta=theta_poly):
    """the sbm_sens_ref.Problem of the coefficient vector p = (mu a0, a1, a2, mob c0, c1)"""
    import sbm_sens_problem as Q
    from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, ClosureDesc

    mu, mob = ClosureDesc(LEGENDRE, LOGIT_PRIOR, tuple(p[:3])), ClosureDesc(LEGENDRE, EXP_WRAP, tuple(p[3:]))
    return Q.problem(eq, (PROBLEMS[eq][0], (1.0, 1.0)), mob=mob, mu=mu, theta=theta, flux=flux)


def cpu_fit(eq):
    """the least-squares fit through the numpy reference: (max |p - p_true|, final ssr / M, objective evaluations)"""
    import sbm_sens_ref as S
    from pde_opt_amd import fit

    points, mu_true, mob_true, mu_init, mob_init = PROBLEMS[eq]
    params = active(eq)
    idx = [k if r == S.MU_ROLE else 3 + k for r, k in params]  # positions of the active entries in p
    steps = [int(round((b - a) / DT0)) for a, b in zip(TS[:-1], TS[1:])]
    starts = y0s(eq)

    def run(p, with_tangents):
        pr = reference_problem(eq, p)
        out = []
        for u in starts:
            dus = [np.zeros_like(u) for _ in params] if with_tangents else []
            frames, s = [], 0
            for n in steps:
                for _ in range(n):
                    u, dus = S.step(pr, u, dus, params if with_tangents else [], s * DT0, DT0, "rk4")
                    s += 1
                frames.append((u, dus))
            out.append(frames)
        return out

    p_true = np.array(mu_true + mob_true)
    data = [[u for u, _ in frames] for frames in run(p_true, False)]
    M = len(starts) * len(steps) * points[0] * points[1]
    count = [0]

    def sums(p):
        count[0] += 1
        ssr, rdp, G = 0.0, np.zeros(5), np.zeros((5, 5))
        for frames, vals in zip(run(p, True), data):
            for (u, dus), v in zip(frames, vals):
                r = v - u
                ssr += float(np.sum(r * r))
                rdp[idx] += np.array([np.sum(r * d) for d in dus])
                G[np.ix_(idx, idx)] += np.array([[np.sum(a * b) for b in dus] for a in dus])
        return ssr, rdp, G

    def ssr(p):
        count[0] += 1
        return float(sum(np.sum((v - u) ** 2) for frames, vals in zip(run(p, False), data) for (u, _), v in zip(frames, vals)))

    obj = fit.Objective(sums=sums, ssr=ssr, M=M, lambda_reg=0.0, w=np.zeros(5))
    p, _ = fit.levenberg_marquardt(obj, np.array(mu_init + mob_init), max_steps=100)
    return float(np.max(np.abs(p - p_true)[idx])), ssr(p) / M, count[0]


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(here, ".."), here]
    for eq in ("ac", "ch"):
        err, final, evals = cpu_fit(eq)
        print(f"{eq}: max |p - p_true| = {err:.3e}, ssr / M = {final:.3e}, {evals} solves")
