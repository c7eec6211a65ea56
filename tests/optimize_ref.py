"""CPU stand-ins for PDEModel.optimize: the numpy tangent references (tests/sens_ref.py, sens_ref3d.py, sens_ref_ac.py)
in the engine's place under the product's own gradient assembly and BFGS (fit.objective_gradient, fit.minimize_bfgs),
the way tests/ac_fit_problem.py::cpu_fit stands them in for PDEModel.train.  Test infrastructure only.

    python tests/optimize_ref.py      # prints what the GPU tests of tests/test_gpu_optimize.py are gated against

``stepper(u, dus, params) -> (u, dus)`` is one step of a state and its tangents; every save point is a step edge."""
import os
import sys

import numpy as np

import ac_fit_problem as F


def frames_of(stepper, u0, params, steps):
    """[(u, dus)] at the end of each run of ``steps[q]`` steps from ``u0`` (tangents start at zero)"""
    u, dus = u0, [np.zeros_like(u0) for _ in params]
    out = []
    for n in steps:
        for _ in range(n):
            u, dus = stepper(u, dus, params)
        out.append((u, dus))
    return out


def solution(stepper, y0s, steps):
    """``ys`` ``(T, B, *spatial)`` of the forward trajectories: what PDEModel.solve returns for batched ``y0``"""
    per_traj = [[u0] + [u for u, _ in frames_of(stepper, u0, [], steps)] for u0 in y0s]
    return np.stack([np.stack([tr[q] for tr in per_traj]) for q in range(len(steps) + 1)])


def contractor(stepper, y0s, params, steps):
    """``contract(cotangents (T - 1, B, *spatial)) -> (B, P)``: what fit.sensitivity_solve(cotangents=...) returns"""
    def contract(cot):
        out = np.zeros((len(y0s), len(params)))
        for b, u0 in enumerate(y0s):
            for q, (_, dus) in enumerate(frames_of(stepper, u0, params, steps)):
                out[b] += [float(np.sum(cot[q, b] * d)) for d in dus]
        return out

    return contract


def value_and_grad_fns(fit, objective, make_stepper, y0s, params, steps, pmap):
    """``(value_and_grad(p), value(p))`` of ``objective(solution)`` through the numpy tangents"""
    def value_and_grad(p):
        st = make_stepper(p)
        return fit.objective_gradient(objective, solution(st, y0s, steps), y0s.ndim - 1, contractor(st, y0s, params, steps), pmap)

    def value(p):
        return objective.value(solution(make_stepper(p), y0s, steps))

    return value_and_grad, value


# ---- the Allen-Cahn problem of tests/ac_fit_problem.py ----------------------------------------------------------------


def ac_params():
    import sens_ref_ac as S

    return [(S.MU_ROLE, 0), (S.MU_ROLE, 1), (S.MU_ROLE, 2), (S.R_ROLE, 0), (S.R_ROLE, 1)]


def ac_stepper(p, n=F.N, dt=F.DT0, integrator="rk4"):
    import sens_ref_ac as S
    from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, ClosureDesc

    mu, R = ClosureDesc(LEGENDRE, LOGIT_PRIOR, tuple(p[:3])), ClosureDesc(LEGENDRE, EXP_WRAP, tuple(p[3:]))
    h = 1.0 / n
    return lambda u, dus, params: S.step(u, dus, params, dt, h, h, F.KAPPA, mu, R, integrator)


def ac_pmap():
    import pde_opt_amd as P
    from pde_opt_amd import fit
    from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
    from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg

    return fit.ParamMap.of({"mu": ChemLeg(np.array(F.MU_INIT), F.logit), "R": DiffLeg(np.array(F.R_INIT))}, P.AllenCahn2DPeriodic)


def cpu_train_mse(fit):
    """``train(method="mse")`` of tests/ac_fit_problem.py through the numpy tangents (cpu_fit, returning the fitted
    vector and the history) under the ``fit`` module given"""
    steps = [int(round((b - a) / F.DT0)) for a, b in zip(F.TS[:-1], F.TS[1:])]
    params, starts = ac_params(), F.y0s()
    data = [[u for u, _ in frames_of(ac_stepper(np.array(F.MU_TRUE + F.R_TRUE)), u0, [], steps)] for u0 in starts]
    M = len(starts) * len(steps) * F.N * F.N

    def sums(p):
        ssr, rdp, G = 0.0, np.zeros(5), np.zeros((5, 5))
        for u0, vals in zip(starts, data):
            for (u, dus), v in zip(frames_of(ac_stepper(p), u0, params, steps), vals):
                r = v - u
                ssr += float(np.sum(r * r))
                rdp += np.array([np.sum(r * d) for d in dus])
                G += np.array([[np.sum(a * b) for b in dus] for a in dus])
        return ssr, rdp, G

    def ssr(p):
        return float(sum(np.sum((v - u) ** 2) for u0, vals in zip(starts, data)
                         for (u, _), v in zip(frames_of(ac_stepper(p), u0, [], steps), vals)))

    obj = fit.Objective(sums=sums, ssr=ssr, M=M, lambda_reg=0.0, w=np.zeros(5))
    return fit.bfgs(obj, np.array(F.MU_INIT + F.R_INIT), max_steps=100)


# The end-to-end problem of tests/test_gpu_optimize.py: the trajectories of ac_fit_problem.py, observed through
# J = mean((ys[-1] - target)^2) (+ the same at the middle save point with E2E_FRAMES = (1, 2)).
E2E_TS = np.array([0.0, 1.5e-4, 3e-4])  # 300 RK4 substeps
E2E_FRAMES = (2,)


class FrameTarget:
    """``J(ys) = sum over the frames q of mean((ys[q] - target[q])^2)``, as a numpy objective"""

    def __init__(self, target, frames=E2E_FRAMES):
        self.target, self.frames = target, frames

    def value_and_grad(self, ys):
        g = np.zeros(ys.shape)
        J = 0.0
        for q in self.frames:
            r = ys[q] - self.target[q]
            J += float(np.mean(r * r))
            g[q] = 2.0 * r / r.size
        return J, g


def cpu_optimize_ac(frames=E2E_FRAMES, max_steps=100):
    """the end-to-end optimisation on the CPU: ``(max |p - p_true|, final objective, history)``"""
    from pde_opt_amd import fit

    steps = [int(round((b - a) / F.DT0)) for a, b in zip(E2E_TS[:-1], E2E_TS[1:])]
    y0s, params, p_true = F.y0s(), ac_params(), np.array(F.MU_TRUE + F.R_TRUE)
    objective = fit.as_objective(FrameTarget(solution(ac_stepper(p_true), y0s, steps), frames))
    vg, v = value_and_grad_fns(fit, objective, ac_stepper, y0s, params, steps, ac_pmap())
    p, hist = fit.minimize_bfgs(vg, v, np.array(F.MU_INIT + F.R_INIT), max_steps=max_steps)
    return float(np.max(np.abs(p - p_true))), v(p), hist


# ---- the quick problem of examples/optimize_objective.py ---------------------------------------------------------------


def ch_stepper_factory(dom, kappa, n_mu, dt=1e-6, A=0.5):
    """``p -> stepper`` of CahnHilliard2DPeriodic (Legendre mu under the logit prior, exp-wrapped Legendre D) with IMEX"""
    import pde_opt_amd as P
    import sens_ref as S
    from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, ClosureDesc

    hx, hy = dom.dx
    symbol = P.CahnHilliard2DPeriodic(dom, kappa, lambda c: c, lambda c: c).fourier_symbol

    def make(p):
        mu, D = ClosureDesc(LEGENDRE, LOGIT_PRIOR, tuple(p[:n_mu])), ClosureDesc(LEGENDRE, EXP_WRAP, tuple(p[n_mu:]))
        return lambda u, dus, params: S.step(u, dus, params, dt, hx, hy, kappa, mu, D, "imex", A, np.asarray(symbol))

    return make


class SecondMoment:
    """``J(ys) = ((mean(ys[-1]^2) - target) / scale)^2``"""

    def __init__(self, target, scale):
        self.target, self.scale = target, scale

    def value_and_grad(self, ys):
        m = (float(np.mean(ys[-1] ** 2)) - self.target) / self.scale
        g = np.zeros(ys.shape)
        g[-1] = 2.0 * m * 2.0 * ys[-1] / (ys[-1].size * self.scale)
        return m * m, g


def cpu_example(n=32, substeps=200):
    """examples/optimize_objective.py --quick on the CPU: the history of objectives"""
    import pde_opt_amd as P
    import sens_ref as S
    from pde_opt_amd import fit
    from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg
    from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg

    L_ = 0.01 * n
    dom = P.Domain((n, n), ((-L_ / 2, L_ / 2),) * 2, "dimensionless")
    make = ch_stepper_factory(dom, 0.002, 3)
    y0s = np.clip(0.5 + 0.05 * np.random.default_rng(0).standard_normal((n, n)), 0.05, 0.95)[None]
    p_true, p0 = np.array([0.0, -3.0, 0.2, -1.0, 0.2]), np.array([0.0, -2.6, 0.1, -1.4, 0.1])
    pmap = fit.ParamMap.of({"mu": ChemLeg(p0[:3], F.logit), "D": DiffLeg(p0[3:])}, P.CahnHilliard2DPeriodic)
    params = [(S.MU_ROLE, 1), (S.MU_ROLE, 2), (S.MOB_ROLE, 0), (S.MOB_ROLE, 1)]
    assert pmap.sens_params() == params
    target = float(np.mean(solution(make(p_true), y0s, [substeps])[-1] ** 2))
    scale = float(np.mean(solution(make(p0), y0s, [substeps])[-1] ** 2)) - target
    vg, v = value_and_grad_fns(fit, fit.as_objective(SecondMoment(target, scale)), make, y0s, params, [substeps], pmap)
    return fit.minimize_bfgs(vg, v, p0, max_steps=100)[1]


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    hist = cpu_example()
    print(f"example --quick: J {hist[0]:.3e} -> {hist[-1]:.3e} (factor {hist[-1] / hist[0]:.1e}), {len(hist) - 1} steps")
    if "--example" in sys.argv:
        sys.exit(0)
    for frames in ((2,), (1, 2)):
        err, final, hist = cpu_optimize_ac(frames)
        print(f"frames {frames}: max |p - p_true| = {err:.3e}, J = {final:.3e}, {len(hist) - 1} steps (J0 = {hist[0]:.3e})")
