"""Microseconds per ``gpe_observables`` call next to microseconds per step of the rotating split step on the same state
in the same run: 256^2 x 1 and 512^2 x 128 environments, fp32.  HIP events around a window of calls (a call ends in its
own device-to-host copy and synchronise), WARMUP + ROUNDS windows, the medians reported.

    python tools/gpe_obs_bench.py [--out profiles/gpe_observables.json]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pde_opt_amd as P  # noqa: E402
from pde_opt_amd.engine import HipEngine  # noqa: E402

WARMUP, ROUNDS, STEPS, CALLS, DT = 2, 7, 50, 50, 1e-3
K, E, OMEGA = 1000.0, 0.0, 0.7


def windows(eng, fn, count):
    out = []
    for _ in range(WARMUP + ROUNDS):
        eng.timer_start()
        fn()
        out.append(eng.timer_stop() * 1e3 / count)  # ms per window -> us per item
    return float(np.median(out[WARMUP:]))


def case(n, batch):
    dom = P.Domain((n, n), ((-12.0, 12.0), (-12.0, 12.0)), "dimensionless")
    x, y = dom.mesh()
    psi = np.exp(-(x**2 + y**2) / 32.0)
    psi = psi / np.sqrt(np.sum(psi**2) * dom.dx[0] ** 2)
    y0 = np.broadcast_to(np.stack([psi, 0 * psi], axis=-1), (batch, n, n, 2)).astype(np.float32).copy()
    eq, solver = P.GPE2DTSRot(dom, K, E, OMEGA), P.RotatingStrangSplitting(dom.dx[0])
    eng = HipEngine(0)
    eng.configure(dtype=np.float32, batch=batch, **eq._engine_problem())
    eq._engine_upload(eng, 0.0, 1.0)
    solver.configure_engine(eng, eq)
    eng.set_state(y0)
    row = {"shape": [n, n], "batch": batch, "dtype": "float32", "steps_per_window": STEPS, "calls_per_window": CALLS}
    row["step_us"] = windows(eng, lambda: eng.advance(solver.integrator, DT, STEPS), STEPS)
    row["step_kernel"] = eng.last_kernel

    def calls():
        for _ in range(CALLS):
            eng.gpe_observables()

    row["observables_us_per_call"] = windows(eng, calls, CALLS)
    row["observables_kernel"] = eng.last_kernel
    row["calls_per_step"] = row["observables_us_per_call"] / row["step_us"]
    eng.close()
    return row


if __name__ == "__main__":
    rows = [case(256, 1), case(512, 128)]
    for r in rows:
        print(json.dumps(r))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump({"tool": "tools/gpe_obs_bench.py", "rows": rows}, f, indent=1)
