"""Microseconds per Tsit5 trial step of the Butler-Volmer notebook problem (100^2 smoothed-boundary disc at constant
current, fp32 and fp64) next to a host-driven trial step of AllenCahn2DSmoothedBoundary on the same grid in the same run,
and microseconds per right-hand side at 1024^2 x 8 next to the Allen-Cahn stage kernel there.  HIP events around a
window of calls, WARMUP + ROUNDS windows, the medians reported.

    python tools/bv_bench.py [--out profiles/butler_volmer.json]

``--sens``: microseconds per RK4 substep of the forward-mode sensitivity advance (state + P tangents, P = 3 and P = 7:
Legendre coefficients of mu and j0) next to microseconds per RK4 substep of the plain forward advance of the same B
trajectories in the same run, at constant current, for 128^2 x 3 and 1024^2 x 8.

    python tools/bv_bench.py --sens [--out profiles/butler_volmer_sens.json]
"""
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pde_opt_amd as P  # noqa: E402
from pde_opt_amd.engine import HipEngine  # noqa: E402

WARMUP, ROUNDS, TRIALS, CALLS = 2, 7, 50, 50
H, KAPPA = 0.01, 0.002
MU = lambda c: np.log(c / (1.0 - c)) + 3.0 * (1.0 - 2.0 * c)  # noqa: E731
J0 = lambda c: np.sqrt((1.0 - c) * c)  # noqa: E731
F = lambda c: c * np.log(c) + (1.0 - c) * np.log(1.0 - c) + 3.0 * c * (1.0 - c) + 0.059  # noqa: E731


def windows(eng, fn, count):
    out = []
    for _ in range(WARMUP + ROUNDS):
        eng.timer_start()
        fn()
        out.append(eng.timer_stop() * 1e3 / count)  # ms per window -> us per item
    return float(np.median(out[WARMUP:]))


def disc(n, floor=1e-6):
    x = np.arange(n) + 0.5
    X, Y = np.meshgrid(x, x, indexing="ij")
    r = np.sqrt((X - 0.5 * n) ** 2 + (Y - 0.5 * n) ** 2)
    return floor + (1.0 - floor) * 0.5 * (1.0 + np.tanh((0.3 * n - r) / 2.5))


def domain(n, psi=None):
    geo = None if psi is None else types.SimpleNamespace(smooth=psi)
    return P.Domain((n, n), ((-H * n / 2, H * n / 2), (-H * n / 2, H * n / 2)), "dimensionless", geo)


def load(eng, eq, y0):
    eng.configure(dtype=y0.dtype, batch=y0.shape[0], **eq._engine_problem())
    eq._engine_upload(eng, 0.0, 1.0)
    eng.set_state(y0)


def trial_case(dtype):
    """a smooth state (rates of order one), trial steps of 1e-5 that are never committed: every window repeats the same work"""
    n = 100
    psi = disc(n)
    x = np.arange(n) * H
    y0 = (0.15 + 0.05 * np.sin(2 * np.pi * x / (n * H))[:, None] * np.cos(2 * np.pi * x / (n * H))[None, :]).astype(dtype)[None]
    eng = HipEngine(0)
    eng.set_small_persist(-1)  # the host-driven loop for the comparison equation too
    row = {"shape": [n, n], "batch": 1, "dtype": np.dtype(dtype).name, "trials_per_window": TRIALS}

    def trials():
        for _ in range(TRIALS):
            eng.tsit5_trial(0.0, 1e-5, 1e-4, 1e-6)
            eng.tsit5_commit(False)

    bv = P.AllenCahn2DSmoothedBoundaryButlerVolmerConstantCurrent(domain(n, psi), KAPPA, F, MU, J0, 0.5, 0.02)
    load(eng, bv, y0)
    row["bv_trial_us"] = windows(eng, trials, TRIALS)
    row["bv_kernel"] = eng.last_kernel
    ac = P.AllenCahn2DSmoothedBoundary(domain(n, psi), KAPPA, F, MU, lambda c: 1.0 + 0.0 * c, lambda t: np.pi / 2)
    load(eng, ac, y0)
    row["ac_sbm_trial_us"] = windows(eng, trials, TRIALS)
    row["ac_sbm_kernel"] = eng.last_kernel
    eng.close()
    return row


def rhs_case(dtype, n=1024, batch=8):
    y0 = np.clip(0.3 + 0.05 * np.random.default_rng(0).standard_normal((batch, n, n)), 0.05, 0.95).astype(dtype)
    eng = HipEngine(0)
    row = {"shape": [n, n], "batch": batch, "dtype": np.dtype(dtype).name, "calls_per_window": CALLS}

    def calls():
        for _ in range(CALLS):
            eng.rhs(fetch=False)

    bv = P.AllenCahn2DPeriodicButlerVolmerConstantCurrent(domain(n), KAPPA, MU, J0, 0.5, 0.02)
    load(eng, bv, y0)
    row["bv_rhs_us"] = windows(eng, calls, CALLS)
    row["bv_kernel"] = eng.last_kernel
    ac = P.AllenCahn2DPeriodic(domain(n), KAPPA, MU, lambda c: 1.0 + 0.0 * c)
    load(eng, ac, y0)
    row["ac_rhs_us"] = windows(eng, calls, CALLS)
    row["ac_kernel"] = eng.last_kernel
    eng.close()
    return row


def sens_case(dtype, n, batch, substeps):
    """a smooth state (rates of order one), RK4 substeps of 1e-6: windows of `substeps` substeps, forward and with tangents"""
    from pde_opt_amd import _lib as L
    from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, ClosureDesc

    mu = ClosureDesc(LEGENDRE, LOGIT_PRIOR, (0.1, -3.0, 0.2, 0.05))
    j0 = ClosureDesc(LEGENDRE, EXP_WRAP, (-0.9, 0.15, 0.05))
    x = np.arange(n) / n
    u = 0.15 + 0.05 * np.sin(2 * np.pi * x)[:, None] * np.cos(2 * np.pi * x)[None, :]
    y0 = np.stack([u + 0.01 * b for b in range(batch)]).astype(dtype)
    eq = P.AllenCahn2DPeriodicButlerVolmerConstantCurrent(domain(n), KAPPA, mu, j0, 0.5, 0.02)
    eng = HipEngine(0)
    row = {"shape": [n, n], "batch": batch, "dtype": np.dtype(dtype).name, "substeps_per_window": substeps, "integrator": "rk4"}
    load(eng, eq, y0)
    row["forward_substep_us"] = windows(eng, lambda: eng.advance(L.INT_RK4, 1e-6, substeps), substeps)
    row["forward_kernel"] = eng.last_kernel
    for params in ([(0, 0), (0, 1), (1, 0)], [(0, k) for k in range(4)] + [(1, k) for k in range(3)]):
        Pn = len(params)
        eng.configure(dtype=y0.dtype, batch=(1 + Pn) * batch, **eq._engine_problem())
        eq._engine_upload(eng, 0.0, 1.0)
        eng.sens_configure(batch, params)
        eng.set_state(np.concatenate([y0, np.zeros((Pn * batch, n, n), dtype=dtype)]))
        row[f"sens_substep_us_P{Pn}"] = windows(eng, lambda: eng.sens_advance(L.INT_RK4, 1e-6, substeps), substeps)
        row[f"sens_over_forward_P{Pn}"] = row[f"sens_substep_us_P{Pn}"] / row["forward_substep_us"]
    row["sens_kernel"] = eng.last_kernel
    eng.close()
    return row


if __name__ == "__main__":
    if "--sens" in sys.argv:
        rows = [sens_case(dt, n, b, k) for n, b, k in ((128, 3, 50), (1024, 8, 10)) for dt in (np.float32, np.float64)]
        for r in rows:
            print(json.dumps(r))
        if "--out" in sys.argv:
            with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
                json.dump({"tool": "tools/bv_bench.py --sens", "rows": rows}, f, indent=1)
        sys.exit(0)
    rows = [trial_case(np.float32), trial_case(np.float64), rhs_case(np.float32), rhs_case(np.float64)]
    for r in rows:
        print(json.dumps(r))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump({"tool": "tools/bv_bench.py", "rows": rows}, f, indent=1)
