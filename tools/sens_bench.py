"""Cost of forward-mode sensitivities against the forward solve (PDEModel.train's inner loop).

For each case (grid, trajectories B, dtype, P tangents) it times, with device events:
  fwd_ms_per_substep   a forward IMEX substep of the B trajectories (pdeopt_advance)
  sens_ms_per_substep  a substep of the B trajectories + their P tangents (pdeopt_sens_advance)
and, on the host clock around calls that end in a device synchronise,
  lm_iter_ms           one Levenberg-Marquardt iteration: a sensitivity solve through 2 save points with the
                       Gauss-Newton sums, plus the normal-equation solve (lm_substeps substeps per solve)
2-D cases run CahnHilliard2DPeriodic on [0, 1]^2; 3-D cases run CahnHilliard3DPeriodic on the box of
docs/notebooks/optimization_3D.ipynb (edge 0.01 n), whose fit spans 40400 substeps per sensitivity solve at 32^3.
Allen-Cahn rows (AllenCahn2DPeriodic on [0, 1]^2, Euler and RK4) time the same two substeps; their forward substep
is whatever pdeopt_advance picks for the B trajectories.
``--optimize`` times PDEModel.optimize's inner loop instead, on the host clock around calls that end in a device
synchronise (CahnHilliard2DPeriodic 128^2 x 1, IMEX, P = 3 / 7, `substeps` substeps to one save point):
  forward_ms   one forward solve (PDEModel.solve): what a line-search trial point costs
  gradient_ms  one gradient evaluation: a forward solve, the objective's cotangent, its upload and a sensitivity solve
               with the contraction (pdeopt_sens_contract)
``--sbm`` times the smoothed-boundary classes (AllenCahn2DSmoothedBoundary, CahnHilliard2DSmoothedBoundary inside a disc,
ramped theta(t), RK4): an RK4 sensitivity substep at P = 3 and P = 7 next to the forward RK4 substep of the same problem
in the same run, 128^2 x 3 and 1024^2 x 8.
``--kappa`` times an IMEX sensitivity substep of CahnHilliard2DPeriodic with kappa among the P = 3 tangents (kappa, mu a1,
D c0: the rocFFT loop with sens_imex_mul_kappa_kernel on every grid) next to P = 3 without it (mu a1, a2, D c0: the
parent's code path, the hand-written FFT passes on these grids) in the same run, 128^2 x 3 and 1024^2 x 8, and -- to
separate the reroute from the new kernels -- the closure-only tangents forced through the rocFFT loop as well.
Prints one JSON line.  usage: python tools/sens_bench.py [--quick] [--ac-only | --optimize | --sbm | --kappa]
"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import pde_opt_amd as P  # noqa: E402
from pde_opt_amd import _lib as L  # noqa: E402
from pde_opt_amd import fit  # noqa: E402
from pde_opt_amd.numerics.functions.legendre import ChemicalPotentialLegendrePolynomials as ChemLeg  # noqa: E402
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials as DiffLeg  # noqa: E402

KAPPA, DT = 0.002, 1e-6


def logit(c):
    return np.log(c / (1.0 - c))


def closures(P_):
    """P = 3: mu a1, a2 + D c0;  P = 6: mu a1..a5 + D c0 (the 3-D notebook's fit);  P = 7: mu a1..a5 + D c0, c1
    (mu's a0 has no tangent)"""
    if P_ == 3:
        return {"mu": ChemLeg(np.array([0.0, -3.0, 0.1]), logit), "D": DiffLeg(np.array([0.0]))}
    if P_ == 6:
        return {"mu": ChemLeg(np.array([0.0, -3.0, 0.1, 0.0, 0.0, 0.0]), logit), "D": DiffLeg(np.array([np.log(0.15)]))}
    return {"mu": ChemLeg(np.array([0.0, -3.0, 0.1, 0.0, 0.0, 0.0]), logit), "D": DiffLeg(np.array([0.0, 0.1]))}


def timed(eng, fn, reps):
    fn()  # warm-up: code objects, multipliers, buffers
    eng.timer_start()
    for _ in range(reps):
        fn()
    return eng.timer_stop() / reps


def case(n, B, dtype, P_, nsub, lm_substeps, dims=2):
    if dims == 2:
        dom = P.Domain((n, n), ((0.0, 1.0), (0.0, 1.0)), "dimensionless")
    else:
        dom = P.Domain((n,) * 3, ((-0.005 * n, 0.005 * n),) * 3, "dimensionless")
    opt = closures(P_)
    eq = (P.CahnHilliard2DPeriodic if dims == 2 else P.CahnHilliard3DPeriodic)(dom, KAPPA, **opt)
    solver = P.SemiImplicitFourierSpectral(A=0.5, fourier_symbol=eq.fourier_symbol)
    rng = np.random.default_rng(0)
    y0s = np.clip(0.5 + 0.05 * rng.standard_normal((B,) + dom.points), 0.05, 0.95).astype(dtype)
    pm = fit.ParamMap.of(opt)
    sp = pm.sens_params()
    assert len(sp) == P_

    fwd = P.HipEngine()
    fwd.configure(dtype=dtype, batch=B, **eq._engine_problem())
    eq._engine_upload(fwd, 0.0, 1.0)
    solver.configure_engine(fwd, eq)
    fwd.set_state(y0s)
    t_fwd = timed(fwd, lambda: fwd.advance(L.INT_IMEX, DT, nsub), 3) / nsub

    sens = P.HipEngine()
    fit._configure(sens, eq, solver, y0s, sp, 0.0, 1.0)
    t_sens = timed(sens, lambda: sens.sens_advance(L.INT_IMEX, DT, nsub), 3) / nsub

    ts = np.array([0.0, 0.5, 1.0]) * lm_substeps * DT
    frames = np.stack([y0s, y0s]).astype(dtype)
    key = object()

    def lm_iteration():
        s, _ = fit.sensitivity_solve(sens, eq, solver, y0s, ts, sp, dt0=DT, frames=frames, frames_key=key)
        ssr, rdp, G = fit.unpack_sums(s, P_)
        np.linalg.solve(G + 1e-3 * np.eye(P_), rdp)

    lm_iteration()
    t0 = time.perf_counter()
    for _ in range(2):
        lm_iteration()
    t_lm = (time.perf_counter() - t0) / 2 * 1e3
    return {"n": n, "dims": dims, "B": B, "dtype": np.dtype(dtype).name, "P": P_, "fwd_ms_per_substep": t_fwd,
            "sens_ms_per_substep": t_sens, "sens_over_fwd": t_sens / t_fwd, "lm_iter_ms": t_lm,
            "lm_substeps": lm_substeps}


def ac_closures(P_):
    """P = 3: mu a0, a1 + R c0;  P = 7: mu a0..a4 + R c0, c1 (for Allen-Cahn mu's a0 has a tangent)"""
    if P_ == 3:
        return {"mu": ChemLeg(np.array([0.0, -3.0]), logit), "R": DiffLeg(np.array([0.0]))}
    return {"mu": ChemLeg(np.array([0.0, -3.0, 0.1, 0.0, 0.0]), logit), "R": DiffLeg(np.array([0.0, 0.1]))}


def ac_case(n, B, dtype, P_, integrator, nsub):
    dom = P.Domain((n, n), ((0.0, 1.0), (0.0, 1.0)), "dimensionless")
    opt = ac_closures(P_)
    eq = P.AllenCahn2DPeriodic(dom, KAPPA, **opt)
    solver = P.Euler() if integrator == "euler" else P.RK4()
    rng = np.random.default_rng(0)
    y0s = np.clip(0.5 + 0.05 * rng.standard_normal((B,) + dom.points), 0.05, 0.95).astype(dtype)
    sp = fit.ParamMap.of(opt, P.AllenCahn2DPeriodic).sens_params()
    assert len(sp) == P_

    fwd = P.HipEngine()
    fwd.configure(dtype=dtype, batch=B, **eq._engine_problem())
    eq._engine_upload(fwd, 0.0, 1.0)
    fwd.set_state(y0s)
    t_fwd = timed(fwd, lambda: fwd.advance(solver.integrator, DT, nsub), 3) / nsub
    kernel = fwd.last_kernel()

    sens = P.HipEngine()
    fit._configure(sens, eq, solver, y0s, sp, 0.0, 1.0)
    t_sens = timed(sens, lambda: sens.sens_advance(solver.integrator, DT, nsub), 3) / nsub
    return {"equation": "allen_cahn", "integrator": integrator, "n": n, "B": B, "dtype": np.dtype(dtype).name, "P": P_,
            "fwd_ms_per_substep": t_fwd, "fwd_kernel": kernel, "sens_ms_per_substep": t_sens, "sens_over_fwd": t_sens / t_fwd}


def ac_rows(quick):
    rows = []
    for n, B, nsub, Ps in ((128, 3, 200, (3, 7)), (1024, 8, 20, (3, 7))):
        for dtype in (np.float32, np.float64):
            for integrator in ("euler", "rk4"):
                for P_ in Ps:
                    if quick and (n > 128 or P_ > 3):
                        continue
                    rows.append(ac_case(n, B, dtype, P_, integrator, nsub))
    return rows


def sbm_case(kind, n, B, dtype, P_, nsub):
    import types

    x = np.arange(n) + 0.5
    X, Y = np.meshgrid(x, x, indexing="ij")
    psi = 0.05 + 0.95 * 0.5 * (1.0 + np.tanh((0.3 * n - np.sqrt((X - 0.5 * n) ** 2 + (Y - 0.5 * n) ** 2)) / 2.5))
    dom = P.Domain((n, n), ((0.0, float(n)), (0.0, float(n))), "dimensionless", geometry=types.SimpleNamespace(smooth=psi))
    f = lambda c: c * np.log(c) + (1.0 - c) * np.log(1.0 - c) + 3.0 * c * (1.0 - c) + 0.059  # noqa: E731
    theta = lambda t: np.pi / 2 - 10.0 * t  # noqa: E731
    # P = 3 / 7 active tangents: Allen-Cahn counts mu's a0, Cahn-Hilliard does not
    n_mu = {("ac", 3): 2, ("ac", 7): 5, ("ch", 3): 3, ("ch", 7): 6}[kind, P_]
    mu = ChemLeg(np.array([0.0, -3.0, 0.1, 0.0, 0.0, 0.0][:n_mu]), logit)
    mob = DiffLeg(np.array([0.8] if P_ == 3 else [0.8, 0.1]))
    if kind == "ac":
        cls, opt = P.AllenCahn2DSmoothedBoundary, {"mu": mu, "R": mob}
        eq = cls(dom, 1.5, f, mu, mob, theta)
    else:
        cls, opt = P.CahnHilliard2DSmoothedBoundary, {"mu": mu, "D": mob}
        eq = cls(dom, 1.5, f, mu, mob, theta, lambda t: 0.02)
    solver, dt = P.RK4(), 1e-3
    rng = np.random.default_rng(0)
    y0s = np.clip(0.5 + 0.05 * rng.standard_normal((B, n, n)), 0.1, 0.9).astype(dtype)
    sp = fit.ParamMap.of(opt, cls).sens_params()
    assert len(sp) == P_

    fwd = P.HipEngine()
    fwd.configure(dtype=dtype, batch=B, **eq._engine_problem())
    eq._engine_upload(fwd, 0.0, 1.0)
    fwd.set_state(y0s)
    t_fwd = timed(fwd, lambda: fwd.advance(solver.integrator, dt, nsub), 3) / nsub
    kernel = fwd.last_kernel

    sens = P.HipEngine()
    fit._configure(sens, eq, solver, y0s, sp, 0.0, 1.0)
    t_sens = timed(sens, lambda: sens.sens_advance(solver.integrator, dt, nsub), 3) / nsub
    return {"equation": kind + "_sbm", "integrator": "rk4", "n": n, "B": B, "dtype": np.dtype(dtype).name, "P": P_,
            "fwd_us_per_substep": 1e3 * t_fwd, "fwd_kernel": kernel, "sens_us_per_substep": 1e3 * t_sens,
            "sens_kernel": sens.last_kernel, "sens_over_fwd": t_sens / t_fwd}


def sbm_rows(quick):
    rows = []
    for n, B, nsub in ((128, 3, 100), (1024, 8, 10)):
        for kind in ("ac", "ch"):
            for dtype in (np.float32, np.float64):
                for P_ in (3, 7):
                    if quick and (n > 128 or P_ > 3):
                        continue
                    rows.append(sbm_case(kind, n, B, dtype, P_, nsub))
    return rows


def kappa_case(n, B, dtype, nsub):
    from pde_opt_amd.numerics.functions import TrainableScalar

    dom = P.Domain((n, n), ((0.0, 1.0), (0.0, 1.0)), "dimensionless")
    rng = np.random.default_rng(0)
    y0s = np.clip(0.5 + 0.05 * rng.standard_normal((B,) + dom.points), 0.05, 0.95).astype(dtype)
    row = {"equation": "cahn_hilliard", "integrator": "imex", "n": n, "B": B, "dtype": np.dtype(dtype).name, "P": 3}
    with_kappa = {"kappa": TrainableScalar(KAPPA), "mu": ChemLeg(np.array([0.0, -3.0]), logit), "D": DiffLeg(np.array([0.0]))}
    for name, opt, rocfft in (("without_kappa", closures(3), False), ("without_kappa_rocfft", closures(3), True),
                              ("with_kappa", with_kappa, False)):
        eq = P.CahnHilliard2DPeriodic(dom, **fit.plain({"kappa": KAPPA, **opt}))
        solver = P.SemiImplicitFourierSpectral(A=0.5, fourier_symbol=eq.fourier_symbol)
        sp = fit.ParamMap.of(opt, P.CahnHilliard2DPeriodic).sens_params()
        assert len(sp) == 3 and ((L.SENS_KAPPA, 0) in sp) == (name == "with_kappa")
        sens = P.HipEngine()
        if rocfft:
            sens._check(sens._lib.pdeopt_set_option(sens._h, L.OPT_IMEX_LDS_FFT, -1))  # rocFFT's transforms on every grid
        fit._configure(sens, eq, solver, y0s, sp, 0.0, 1.0)
        row[name + "_us_per_substep"] = 1e3 * timed(sens, lambda: sens.sens_advance(L.INT_IMEX, DT, nsub), 5) / nsub
        row[name + "_kernel"] = sens.last_kernel
        sens.close()
    row["with_over_without"] = row["with_kappa_us_per_substep"] / row["without_kappa_us_per_substep"]
    row["with_over_without_rocfft"] = row["with_kappa_us_per_substep"] / row["without_kappa_rocfft_us_per_substep"]
    return row


def kappa_rows(quick):
    return [kappa_case(n, B, dtype, nsub) for n, B, nsub in ((128, 3, 200), (1024, 8, 20)) for dtype in (np.float32, np.float64)
            if not (quick and n > 128)]


class _SecondMoment:
    """J = mean(ys[-1]^2) with its cotangent, in numpy (the objective's own cost stays out of the comparison)"""

    def value_and_grad(self, ys):
        g = np.zeros(ys.shape)
        g[-1] = 2.0 * ys[-1] / ys[-1].size
        return float(np.mean(np.asarray(ys[-1], dtype=np.float64) ** 2)), g


def optimize_case(n, dtype, P_, substeps, reps=5):
    dom = P.Domain((n, n), ((0.0, 1.0), (0.0, 1.0)), "dimensionless")
    opt = closures(P_)
    model = P.PDEModel(P.CahnHilliard2DPeriodic, dom, P.SemiImplicitFourierSpectral)
    y0 = np.clip(0.5 + 0.05 * np.random.default_rng(0).standard_normal(dom.points), 0.05, 0.95).astype(dtype)
    ts = np.array([0.0, substeps * DT])
    vg, v, pmap = model._objective_functions(_SecondMoment(), y0, ts, opt, {"kappa": KAPPA}, {"A": 0.5}, {}, 0.0)
    p = pmap.flatten(opt)

    def clock(fn):
        fn()  # warm-up: code objects, multipliers, buffers
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) / reps * 1e3

    t_fwd, t_grad = clock(lambda: v(p)), clock(lambda: vg(p))
    return {"n": n, "B": 1, "dtype": np.dtype(dtype).name, "P": P_, "substeps": substeps, "forward_ms": t_fwd,
            "gradient_ms": t_grad, "gradient_over_forward": t_grad / t_fwd}


def main():
    quick = "--quick" in sys.argv
    if "--optimize" in sys.argv:
        rows = [optimize_case(128, dtype, P_, 200 if quick else 4040) for dtype in (np.float32, np.float64)
                for P_ in ((3,) if quick else (3, 7))]
        print(json.dumps({"tool": "sens_bench", "mode": "optimize", "dt": DT, "cases": rows}))
        return
    if "--sbm" in sys.argv:
        print(json.dumps({"tool": "sens_bench", "mode": "sbm", "cases": sbm_rows(quick)}))
        return
    if "--kappa" in sys.argv:
        print(json.dumps({"tool": "sens_bench", "mode": "kappa", "dt": DT, "cases": kappa_rows(quick)}))
        return
    if "--ac-only" in sys.argv:
        print(json.dumps({"tool": "sens_bench", "dt": DT, "cases": ac_rows(quick)}))
        return
    rows = []
    for n, B, nsub, lm in ((128, 3, 200, 4040), (1024, 8, 20, 100)):
        for dtype in (np.float32, np.float64):
            for P_ in (3, 7):
                if quick and (n > 128 or P_ > 3):
                    continue
                rows.append(case(n, B, dtype, P_, nsub, lm))
    # 3-D: the notebook's fit (32^3 x 3, P = 6, 40400 substeps per sensitivity solve) and 64^3 x 3
    for n, B, nsub, lm in ((32, 3, 200, 40400), (64, 3, 100, 4040)):
        for dtype in (np.float32, np.float64):
            if quick and n > 32:
                continue
            rows.append(case(n, B, dtype, 6, nsub // 4 if quick else nsub, 404 if quick else lm, dims=3))
    print(json.dumps({"tool": "sens_bench", "dt": DT, "cases": rows + ac_rows(quick)}))


if __name__ == "__main__":
    main()
