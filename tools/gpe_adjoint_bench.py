"""Time one gradient of the GPE control path (pde_opt_amd.gpe_control: the recomputation forward pass + the backward
sweep of csrc/gpe_adjoint.hip) against one forward solve of the same length, at 256^2 x 1 and 512^2 x 8, fp32 and fp64.

Wall-clock around whole calls, each ended by a device synchronisation (both calls return host arrays); the first calls
are discarded as warm-up (code objects, rocFFT plans, the spectral multipliers); median, min and max of ROUNDS calls.
Needs an MI355X.

    PYTHONPATH=. python tools/gpe_adjoint_bench.py [--json out.json]
"""
import json
import sys
import time

import numpy as np

import pde_opt_amd as P
from pde_opt_amd.gpe_control import GpeControlSolver
from pde_opt_amd.numerics.functions.lights import GaussianSpots
from pde_opt_amd.utils import prepare_solver_params

WARMUP, ROUNDS, STEPS, DT = 2, 7, 20, 1e-3


def timed(fn):
    out = []
    for _ in range(WARMUP + ROUNDS):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    out = out[WARMUP:]
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def case(n, B, dtype):
    dom = P.Domain((n, n), ((-4.0, 4.0), (-4.0, 4.0)), "dimensionless")
    spots = GaussianSpots.moving(3.0, (-0.5, 0.0), (0.5, 0.3), STEPS * DT, 0.7) + GaussianSpots.single(-1.0, 0.2, -0.4, 0.9)
    params = dict(k=1.0, e=0.0, lights=spots, trap_factor=1.0, kinetic=True)
    eq = P.GPE2DTSControl(dom, **params)
    solver = P.StrangSplitting(**prepare_solver_params(P.StrangSplitting, {"time_scale": 1.0}, eq))
    model = P.PDEModel(P.GPE2DTSControl, dom, P.StrangSplitting)
    X, Y = dom.mesh()
    psi = np.exp(-0.5 * (X**2 + Y**2))
    y0 = np.broadcast_to(np.stack([psi, np.zeros_like(psi)], axis=-1), (B, n, n, 2)).astype(dtype)
    ts = np.array([0.0, STEPS * DT])
    cot = np.zeros((2, B, n, n, 2))
    cot[-1] = 1.0
    gs = GpeControlSolver(0)
    return {"forward solve": timed(lambda: model.solve(params, y0, ts, {"time_scale": 1.0}, dt0=DT)),
            "gradient (recomputation + backward sweep)": timed(lambda: gs.gradient(eq, solver, y0, ts, DT, cot))}


if __name__ == "__main__":
    results = {}
    for n, B in ((256, 1), (512, 8)):
        for dtype in (np.float32, np.float64):
            key = f"{n}x{n}x{B} {np.dtype(dtype).name} {STEPS} substeps"
            results[key] = case(n, B, dtype)
            for name, (med, lo, hi) in results[key].items():
                print(f"{key:34s} {name:42s} {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f})")
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(results, f, indent=1)
