"""The synthetic kappa fitting problems of tests/test_gpu_sens_kappa.py, and the same fits on the CPU: fp64 numpy
tangents (tests/sens_kappa_ref.py) under fit.levenberg_marquardt, with log(kappa) as the variable and the kappa column
scaled by kappa, as PDEModel.train does.  Test infrastructure only.

    python tests/kappa_fit_problem.py      # prints the CPU fits' final sum of squared residuals

The GPU test gates PDEModel.train's final ssr at 10 x the values this prints (they are written next to the gates)."""
import math
import os
import sys

import numpy as np

SHAPE = (16, 32)
BOX = ((-0.08, 0.08), (-0.16, 0.16))        # h = 0.01 both ways
DT0 = 1e-6                                  # PDEModel.train's step size
TS = np.array([0.0, 1e-4, 2e-4])            # 200 substeps, 2 observed frames
KAPPA_TRUE, KAPPA_INIT = 0.002, 0.003
SEEDS = (31, 32)
# name -> (reference equation, integrator, mu truth, mu start, the fixed second closure's coefficients)
CASES = {
    "ch_imex": ("ch2d", "imex", (0.0, -3.0), (0.0, -2.6), (-1.0, 0.2)),
    "ac_rk4": ("ac2d", "rk4", (0.1, -3.0), (0.0, -2.6), (6.9, 0.3)),
}


def logit(c):
    return np.log(c / (1.0 - c))


def smooth_state(seed):
    rng = np.random.default_rng(seed)
    x = [np.arange(n) / n for n in SHAPE]
    u = 0.5 + np.zeros(SHAPE)
    for _ in range(6):
        kx, ky = rng.integers(1, 3, 2)
        u += 0.04 * rng.standard_normal() * np.cos(2 * np.pi * (kx * x[0][:, None] + ky * x[1][None, :]) + rng.uniform(0, 6))
    return u


def y0s():
    return np.stack([smooth_state(s) for s in SEEDS])


def cpu_fit(name):
    """the fit through the numpy reference: (fitted kappa, fitted mu coefficients, final ssr, objective evaluations)"""
    import sens_kappa_ref as K
    from pde_opt_amd import fit
    from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, ClosureDesc

    eq, integrator, mu_true, mu_init, second = CASES[name]
    h = tuple((b - a) / n for (a, b), n in zip(BOX, SHAPE))
    mob = ClosureDesc(LEGENDRE, EXP_WRAP, second)
    # Cahn-Hilliard: mu's constant coefficient has no tangent (PDEModel.train leaves it where it starts)
    mu_idx = [1] if eq == "ch2d" else [0, 1]
    params = [(K.KAPPA_ROLE, 0)] + [(K.MU_ROLE, k) for k in mu_idx]
    steps = [int(round((b - a) / DT0)) for a, b in zip(TS[:-1], TS[1:])]
    starts = y0s()

    def unpack(p, base):
        c = list(base)
        for k, v in zip(mu_idx, p[1:]):
            c[k] = v
        return math.exp(p[0]), ClosureDesc(LEGENDRE, LOGIT_PRIOR, tuple(c))

    def run(kappa, mu, with_tangents):
        sym = K.symbol_of(SHAPE, h, kappa) if integrator == "imex" else None
        out = []
        for u in starts:
            dus = [np.zeros_like(u) for _ in params] if with_tangents else []
            frames = []
            for n in steps:
                for _ in range(n):
                    u, dus = K.step(eq, u, dus, params if with_tangents else [], DT0, h, kappa, mu, mob, integrator, 0.5, sym)
                frames.append((u, dus))
            out.append(frames)
        return out

    data = [[u for u, _ in frames] for frames in run(KAPPA_TRUE, ClosureDesc(LEGENDRE, LOGIT_PRIOR, mu_true), False)]
    P = len(params)
    count = [0]

    def sums(p):
        count[0] += 1
        kappa, mu = unpack(p, mu_init)
        ssr, rdp, G = 0.0, np.zeros(P), np.zeros((P, P))
        for frames, vals in zip(run(kappa, mu, True), data):
            for (u, dus), v in zip(frames, vals):
                r = v - u
                ssr += float(np.sum(r * r))
                rdp += np.array([np.sum(r * d) for d in dus])
                G += np.array([[np.sum(a * b) for b in dus] for a in dus])
        s = np.ones(P)
        s[0] = kappa  # d kappa / d log kappa
        return ssr, rdp * s, G * np.outer(s, s)

    def ssr(p):
        count[0] += 1
        kappa, mu = unpack(p, mu_init)
        return float(sum(np.sum((v - u) ** 2) for frames, vals in zip(run(kappa, mu, False), data) for (u, _), v in zip(frames, vals)))

    obj = fit.Objective(sums=sums, ssr=ssr, M=len(starts) * len(steps) * SHAPE[0] * SHAPE[1], lambda_reg=0.0, w=np.zeros(P))
    p0 = np.array([math.log(KAPPA_INIT)] + [mu_init[k] for k in mu_idx])
    p, _ = fit.levenberg_marquardt(obj, p0, max_steps=100)
    return math.exp(p[0]), p[1:], ssr(p), count[0]


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    for name in CASES:
        kappa, mu, final, evals = cpu_fit(name)
        print(f"{name}: kappa = {kappa:.12e}, mu = {np.array2string(np.asarray(mu), precision=12)}, ssr = {final:.3e}, {evals} solves")
