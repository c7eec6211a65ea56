"""Microseconds per ``structure_factor`` call, next to the call with its binning kernels skipped (the real-to-hermitian
transform, the copy of the rows and the synchronise alone: ``PDEOPT_OPT_DEBUG_ABLATE`` bit 0x10000) and to one RK4
substep of the same problem, all in the same run: 1024^2 x 32, 128^2 x 3 and 128^3 x 8 fp32 Cahn-Hilliard
(regular-solution mu, D = c (1 - c)).  HIP events around a window of calls (a call ends in its own device-to-host copy and
synchronise), WARMUP + ROUNDS windows, the medians reported.  ``binning_x_transform`` is the binning pass (the
difference of the two) as a multiple of the transform alone.

    python tools/sk_bench.py [--out profiles/structure_factor.json]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pde_opt_amd as P  # noqa: E402
from pde_opt_amd import _lib as L  # noqa: E402
from pde_opt_amd import structure_factor as SK  # noqa: E402
from pde_opt_amd.engine import HipEngine  # noqa: E402

WARMUP, ROUNDS, STEPS, CALLS, DT = 2, 7, 20, 20, 1e-7
ABLATE_BINNING = 0x10000


def windows(eng, fn, count):
    out = []
    for _ in range(WARMUP + ROUNDS):
        eng.timer_start()
        fn()
        out.append(eng.timer_stop() * 1e3 / count)  # ms per window -> us per item
    return float(np.median(out[WARMUP:]))


def case(points, batch):
    dom = P.Domain(tuple(points), tuple((0.0, 0.01 * n) for n in points), "dimensionless")
    cls = P.CahnHilliard3DPeriodic if len(points) == 3 else P.CahnHilliard2DPeriodic
    eq = cls(domain=dom, kappa=0.002, mu=lambda c: np.log(c / (1.0 - c)) + 3.0 * (1.0 - 2.0 * c), D=lambda c: c * (1.0 - c))
    solver = P.RK4()
    rng = np.random.default_rng(0)
    y0 = (0.5 + 0.02 * rng.standard_normal((batch,) + tuple(points))).astype(np.float32)
    eng = HipEngine(0)
    eng.configure(dtype=np.float32, batch=batch, **eq._engine_problem())
    eq._engine_upload(eng, 0.0, 1.0)
    solver.configure_engine(eng, eq)
    eng.set_state(y0)
    tabs = SK.shell_tables(dom)
    SK.upload_tables(eng, tabs)
    row = {"shape": list(points), "batch": batch, "dtype": "float32", "n_bins": tabs.n_bins, "steps_per_window": STEPS,
           "calls_per_window": CALLS}
    row["rk4_substep_us"] = windows(eng, lambda: eng.advance(solver.integrator, DT, STEPS), STEPS)
    row["rk4_kernel"] = eng.last_kernel

    def calls():
        for _ in range(CALLS):
            eng.structure_factor()

    row["structure_factor_us_per_call"] = windows(eng, calls, CALLS)
    row["structure_factor_kernel"] = eng.last_kernel
    eng._check(eng._lib.pdeopt_set_option(eng._h, L.OPT_DEBUG_ABLATE, ABLATE_BINNING))
    row["transform_alone_us_per_call"] = windows(eng, calls, CALLS)
    eng._check(eng._lib.pdeopt_set_option(eng._h, L.OPT_DEBUG_ABLATE, 0))
    row["binning_us_per_call"] = row["structure_factor_us_per_call"] - row["transform_alone_us_per_call"]
    row["binning_x_transform"] = row["binning_us_per_call"] / row["transform_alone_us_per_call"]
    row["calls_per_substep"] = row["structure_factor_us_per_call"] / row["rk4_substep_us"]
    row["bytes_back_per_environment"] = 8 * tabs.n_bins
    eng.close()
    return row


if __name__ == "__main__":
    rows = [case((1024, 1024), 32), case((128, 128), 3), case((128, 128, 128), 8)]
    for r in rows:
        print(json.dumps(r))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump({"tool": "tools/sk_bench.py", "rows": rows}, f, indent=1)
