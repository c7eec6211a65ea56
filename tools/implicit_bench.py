"""Cost of the implicit Euler step (csrc/implicit.hip) on the GPU, written to profiles/implicit_euler.json.

  per iteration   one implicit Euler step of Cahn-Hilliard (regular-solution mu, D = c (1 - c)) at 128^2 x 1 and
                  1024^2 x 8, fp32 and fp64, at 50 x the explicit Euler limit: wall time of the step over its Krylov
                  iterations and over its Newton iterations, next to one RK4 substep of the same problem in the same run
  time to t_final Cahn-Hilliard 256^2 (fp32) to a fixed t_final under ImplicitEuler, RK4 and SemiImplicitFourierSpectral,
                  each at the largest step it stays stable with: the step is doubled until the solution leaves [-2, 2] or
                  holds a NaN (a plain failure of the solve, reported as such), the last good one is timed

Warm-up run first, then REPEATS timed runs: the median and the min / max spread are recorded.  (The shader clock is not: over windows this
short the reading of ``timer_clock_hz`` is not usable.)  Usage: python tools/implicit_bench.py [--quick] [--out FILE]

``--precond``: the same cases with ``precond="spectral"`` next to the unpreconditioned solver in the same run (Krylov
iterations per Newton iterate and microseconds per Krylov iteration of both), and the 256^2 comparison with both variants
of ImplicitEuler next to RK4 and SemiImplicitFourierSpectral, written to profiles/implicit_euler_precond.json."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.utils import prepare_solver_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS = 5
H, KAPPA = 0.01, 0.002
MU = lambda c: np.log(c / (1.0 - c)) + 3.0 * (1.0 - 2.0 * c)  # noqa: E731
MOB = lambda c: c * (1.0 - c)  # noqa: E731


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def equation(n):
    return P.CahnHilliard2DPeriodic(P.Domain((n, n), ((0.0, H * n), (0.0, H * n)), "dimensionless"), KAPPA, MU, MOB)


def per_iteration(eng, n, batch, dtype, precond=None):
    eq = equation(n)
    y0 = np.clip(0.5 + 0.05 * np.random.default_rng(0).standard_normal((batch, n, n)), 0.1, 0.9).astype(dtype)
    lam = 8.0 / H**2
    dt_euler = 2.0 / (0.25 * (KAPPA * lam * lam + 6.0 * lam))  # D <= 1/4, |mu_h'| <= 6 on [0.1, 0.9]
    dt = 50.0 * dt_euler
    tol = (1e-4, 1e-6) if dtype == np.float32 else (1e-8, 1e-10)
    eng.configure(dtype=dtype, batch=batch, **eq._engine_problem())
    eng.implicit_configure(*tol, max_krylov=2000)
    eng.implicit_set_precond(precond)
    wall, stats = [], None
    for rep in range(REPEATS + 1):
        eng.set_state(y0)
        eng.sync()
        t = time.perf_counter()
        stats = eng.implicit_advance(dt, 1)
        eng.sync()
        if rep:
            wall.append((time.perf_counter() - t) * 1e6)
    newton, krylov = int(stats[:, 0].max()), int(stats[:, 1].max())
    rk4 = []
    for rep in range(REPEATS + 1):
        eng.set_state(y0)
        eng.timer_start()
        eng.advance(L.INT_RK4, 0.25 * dt_euler, 50)
        ms = eng.timer_stop()
        if rep:
            rk4.append(ms * 1e3 / 50)
    w = spread(wall)
    return {"grid": n, "batch": batch, "dtype": np.dtype(dtype).name, "precond": precond, "dt": dt, "dt_over_euler_limit": 50.0,
            "newton_iterations": newton, "krylov_iterations": krylov, "krylov_per_newton": krylov / max(newton, 1), "step_us": w,
            "us_per_krylov_iteration": {k: v / max(krylov, 1) for k, v in w.items()},
            "us_per_newton_iteration": {k: v / max(newton, 1) for k, v in w.items()},
            "rk4_substep_us": spread(rk4)}


def largest_stable_step(solve, dt0, t_final):
    """double dt until the solve's range leaves [-2, 2], a NaN appears or the solver gives up; the last good step"""
    dt, good = dt0, None
    while dt <= t_final:
        try:
            y = solve(dt)
            ok = bool(np.isfinite(y).all() and y.min() >= -2.0 and y.max() <= 2.0)
        except (P.ImplicitSolveError, RuntimeError, ValueError):
            ok = False
        if not ok:
            break
        good, dt = dt, 2.0 * dt
    return good


def time_to_final(eng, n, t_final, precond=False):
    eq = equation(n)
    y0 = np.clip(0.5 + 0.05 * np.random.default_rng(1).standard_normal((n, n)), 0.1, 0.9).astype(np.float32)
    solvers = {
        "ImplicitEuler": P.ImplicitEuler(1e-4, 1e-6, max_krylov=2000),
        **({"ImplicitEuler(precond=spectral)": P.ImplicitEuler(1e-4, 1e-6, max_krylov=2000, precond="spectral")} if precond else {}),
        "RK4": P.RK4(),
        "SemiImplicitFourierSpectral": P.SemiImplicitFourierSpectral(**prepare_solver_params(P.SemiImplicitFourierSpectral, {"A": 0.5}, eq)),
    }
    out = {}
    for name, solver in solvers.items():
        solve = lambda dt: P.diffeqsolve(eq, solver, t0=0.0, t1=t_final, dt0=dt, y0=y0, engine=eng, max_steps=None).ys[-1]  # noqa: E731
        dt = largest_stable_step(solve, 1e-7, t_final)
        if dt is None:
            out[name] = {"stable_dt": None}
            continue
        wall = []
        for rep in range(REPEATS + 1):
            t = time.perf_counter()
            solve(dt)
            if rep:
                wall.append(time.perf_counter() - t)
        out[name] = {"stable_dt": dt, "steps": int(np.ceil(t_final / dt - 1e-9)), "wall_s": spread(wall)}
    return {"grid": n, "dtype": "float32", "t_final": t_final, "solvers": out}


def main():
    quick, precond = "--quick" in sys.argv, "--precond" in sys.argv
    eng = HipEngine()
    cases = [(128, 1)] if quick else [(128, 1), (1024, 8)]
    result = {"what": "implicit Euler (Newton-GMRES, restart 20, CGS2) on Cahn-Hilliard, regular-solution mu, D = c (1 - c)",
              "repeats": REPEATS, "per_iteration": [], "time_to_final": None}
    for n, b in cases:
        for dtype in (np.float32, np.float64):
            for pc in ((None, "spectral") if precond else (None,)):
                row = per_iteration(eng, n, b, dtype, pc)
                print(json.dumps(row), flush=True)
                result["per_iteration"].append(row)
    result["time_to_final"] = time_to_final(eng, 64 if quick else 256, 2e-5 if quick else 2e-4, precond)
    print(json.dumps(result["time_to_final"]), flush=True)
    default = "implicit_euler_precond.json" if precond else "implicit_euler.json"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", default)
    if not quick or "--out" in sys.argv:
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
