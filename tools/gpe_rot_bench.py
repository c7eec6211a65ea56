"""Microseconds per step of the rotating-frame split step (GPE2DTSRot + RotatingStrangSplitting) next to the existing
non-rotating step (GPE2DTSControl(kinetic=True) + StrangSplitting) on the same shapes in the same run: 512^2 x 128
environments fp32 and 256^2 x 1.  HIP events around STEPS steps, WARMUP + ROUNDS windows, the median reported.

    python tools/gpe_rot_bench.py [--out profiles/gpe_rot.json]

``--stir``: the stirred, ramped step (two moving ``GaussianSpots`` plus an ``omega_rate``, csrc/gpe_rot.hip) next
to the plain rotating step instead, same shapes, same run:

    python tools/gpe_rot_bench.py --stir [--out profiles/gpe_rot_stir.json]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pde_opt_amd as P  # noqa: E402
from pde_opt_amd.engine import HipEngine  # noqa: E402

WARMUP, ROUNDS, STEPS, DT = 2, 7, 50, 1e-3
K, E, OMEGA = 1000.0, 0.0, 0.7


def timed(eng, integrator):
    out = []
    for _ in range(WARMUP + ROUNDS):
        eng.timer_start()
        eng.advance(integrator, DT, STEPS)
        out.append(eng.timer_stop() * 1e3 / STEPS)  # ms per window -> us per step
    return float(np.median(out[WARMUP:]))


def stir_lights():
    from pde_opt_amd.numerics.functions.lights import GaussianSpot, GaussianSpots

    return GaussianSpots([GaussianSpot(4.0, 0.5, -1.5, 2.0, 0.8, -1.0, 0.6), GaussianSpot(-3.0, 1.0, 1.2, -1.5, -0.9, 2.5, 0.5)])


def case(n, batch, stir=False):
    dom = P.Domain((n, n), ((-12.0, 12.0), (-12.0, 12.0)), "dimensionless")
    x, y = dom.mesh()
    psi = np.exp(-(x**2 + y**2) / 32.0)
    psi = psi / np.sqrt(np.sum(psi**2) * dom.dx[0] ** 2)
    y0 = np.broadcast_to(np.stack([psi, 0 * psi], axis=-1), (batch, n, n, 2)).astype(np.float32).copy()
    row = {"shape": [n, n], "batch": batch, "dtype": "float32", "steps_per_window": STEPS}
    rotating = ("rotating", P.GPE2DTSRot(dom, K, E, OMEGA), P.RotatingStrangSplitting(dom.dx[0]))
    if stir:
        other = ("stirred", P.GPE2DTSRot(dom, K, E, OMEGA, stir_lights(), 0.3), P.RotatingStrangSplitting(dom.dx[0]))
    else:
        c = P.GPE2DTSControl(dom, K, E, lambda t, xx, yy: 0.0 * xx, kinetic=True)
        other = ("strang", c, P.StrangSplitting(c.A_term, c.dx))
    for name, eq, solver in (rotating, other):
        eng = HipEngine(0)
        eng.configure(dtype=np.float32, batch=batch, **eq._engine_problem())
        eq._engine_upload(eng, 0.0, 1.0)
        solver.configure_engine(eng, eq)
        eng.set_state(y0)
        row[name + "_us_per_step"] = timed(eng, solver.integrator)
        row[name + "_kernel"] = eng.last_kernel
    if stir:
        row["ratio"] = row["stirred_us_per_step"] / row["rotating_us_per_step"]
    else:
        row["ratio"] = row["rotating_us_per_step"] / row["strang_us_per_step"]
    return row


if __name__ == "__main__":
    stir = "--stir" in sys.argv
    rows = [case(512, 128, stir), case(256, 1, stir)]
    for r in rows:
        print(json.dumps(r))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump({"tool": "tools/gpe_rot_bench.py" + (" --stir" if stir else ""), "rows": rows}, f, indent=1)
