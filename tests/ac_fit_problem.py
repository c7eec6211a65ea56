"""The synthetic Allen-Cahn fitting problem of tests/test_gpu_sens_ac.py, and the same fit on the CPU: fp64 numpy
tangents (tests/sens_ref_ac.py) under fit.levenberg_marquardt / fit.bfgs.  Test infrastructure only.

    python tests/ac_fit_problem.py      # prints the CPU fit's coefficient error and final ssr / M per method

The GPU test gates PDEModel.train at 10 x the values this prints (they are written next to the gates)."""
import os
import sys

import numpy as np

N = 32
KAPPA = 0.002
DT0 = 1e-6                                  # PDEModel.train's step size
TS = np.array([0.0, 1e-4, 2e-4, 3e-4])      # 300 RK4 substeps, 3 observed frames
MU_TRUE, R_TRUE = (0.1, -3.0, 0.3), (6.9, 0.3)   # R = exp(6.9 + 0.3 P_1(2c - 1)) ~ 1000: the rate that makes 3e-4 a long time
MU_INIT, R_INIT = (0.0, -2.6, 0.2), (6.7, 0.2)
SEEDS = (21, 22, 23)


def logit(c):
    return np.log(c / (1.0 - c))


def smooth_state(n, seed):
    """a smooth random field around 0.5 (a few Fourier modes)"""
    rng = np.random.default_rng(seed)
    x = np.arange(n) / n
    u = 0.5 + np.zeros((n, n))
    for _ in range(6):
        kx, ky = rng.integers(1, 4, 2)
        u += 0.05 * rng.standard_normal() * np.cos(2 * np.pi * (kx * x[:, None] + ky * x[None, :]) + rng.uniform(0, 6))
    return u


def y0s():
    return np.stack([smooth_state(N, s) for s in SEEDS])


def cpu_fit(method):
    """the fit through the numpy reference: (max |p - p_true|, final ssr / M, objective evaluations)"""
    import sens_ref_ac as S
    from pde_opt_amd import fit
    from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, ClosureDesc

    h = 1.0 / N
    params = [(S.MU_ROLE, 0), (S.MU_ROLE, 1), (S.MU_ROLE, 2), (S.R_ROLE, 0), (S.R_ROLE, 1)]
    steps = [int(round((b - a) / DT0)) for a, b in zip(TS[:-1], TS[1:])]
    starts = y0s()

    def descs(p):
        return ClosureDesc(LEGENDRE, LOGIT_PRIOR, tuple(p[:3])), ClosureDesc(LEGENDRE, EXP_WRAP, tuple(p[3:]))

    def run(p, with_tangents):
        mu, R = descs(p)
        out = []
        for u in starts:
            dus = [np.zeros_like(u) for _ in params] if with_tangents else []
            frames = []
            for n in steps:
                for _ in range(n):
                    u, dus = S.step(u, dus, params if with_tangents else [], DT0, h, h, KAPPA, mu, R, "rk4")
                frames.append((u, dus))
            out.append(frames)
        return out

    p_true = np.array(MU_TRUE + R_TRUE)
    data = [[u for u, _ in frames] for frames in run(p_true, False)]
    M = len(starts) * len(steps) * N * N
    count = [0]

    def sums(p):
        count[0] += 1
        ssr, rdp, G = 0.0, np.zeros(5), np.zeros((5, 5))
        for frames, vals in zip(run(p, True), data):
            for (u, dus), v in zip(frames, vals):
                r = v - u
                ssr += float(np.sum(r * r))
                rdp += np.array([np.sum(r * d) for d in dus])
                G += np.array([[np.sum(a * b) for b in dus] for a in dus])
        return ssr, rdp, G

    def ssr(p):
        count[0] += 1
        return float(sum(np.sum((v - u) ** 2) for frames, vals in zip(run(p, False), data) for (u, _), v in zip(frames, vals)))

    obj = fit.Objective(sums=sums, ssr=ssr, M=M, lambda_reg=0.0, w=np.zeros(5))
    p0 = np.array(MU_INIT + R_INIT)
    p, _ = (fit.levenberg_marquardt if method == "least_squares" else fit.bfgs)(obj, p0, max_steps=100)
    return float(np.max(np.abs(p - p_true))), ssr(p) / M, count[0]


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    for method in ("least_squares", "mse"):
        err, final, evals = cpu_fit(method)
        print(f"{method}: max |p - p_true| = {err:.3e}, ssr / M = {final:.3e}, {evals} solves")
