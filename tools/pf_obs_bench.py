"""Microseconds per ``pf_observables`` call next to microseconds per RK4 substep of the same problem in the same run:
1024^2 x 32 fp32, 128^2 x 3 fp32 and 128^3 x 8 fp32 Cahn-Hilliard (regular-solution mu, D = c (1 - c)).  HIP events around
a window of calls (a call ends in its own device-to-host copy and synchronise), WARMUP + ROUNDS windows, the medians
reported.  ``floor_us`` is one read of the field at the 8.0 TB/s HBM rate of the project's roofline;
``x_floor`` is the call as a multiple of it.

    python tools/pf_obs_bench.py [--out profiles/pf_obs.json]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pde_opt_amd as P  # noqa: E402
from pde_opt_amd.engine import HipEngine  # noqa: E402

WARMUP, ROUNDS, STEPS, CALLS, DT = 2, 7, 20, 20, 1e-7
HBM_BYTES_PER_S = 8.0e12


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
    row = {"shape": list(points), "batch": batch, "dtype": "float32", "steps_per_window": STEPS, "calls_per_window": CALLS}
    row["rk4_substep_us"] = windows(eng, lambda: eng.advance(solver.integrator, DT, STEPS), STEPS)
    row["rk4_kernel"] = eng.last_kernel

    def calls():
        for _ in range(CALLS):
            eng.pf_observables()

    row["observables_us_per_call"] = windows(eng, calls, CALLS)
    row["observables_kernel"] = eng.last_kernel
    row["floor_us"] = y0.nbytes / HBM_BYTES_PER_S * 1e6
    row["x_floor"] = row["observables_us_per_call"] / row["floor_us"]
    row["calls_per_substep"] = row["observables_us_per_call"] / row["rk4_substep_us"]
    eng.close()
    return row


if __name__ == "__main__":
    rows = [case((1024, 1024), 32), case((128, 128), 3), case((128, 128, 128), 8)]
    for r in rows:
        print(json.dumps(r))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump({"tool": "tools/pf_obs_bench.py", "rows": rows}, f, indent=1)
