"""Time one backward substep of the rotating-frame split step (pdeopt_gpe_rot_adjoint_step, csrc/gpe_rot_adjoint.hip)
next to one forward step of the same problem in the same run, at 256^2 x 1 and 512^2 x 8, fp32 and fp64.

Device time between events on the engine's stream around a round of calls in a row (the backward substep with a device
gradient block, so nothing synchronises in between), a round sized to about ROUND_MS; the first WARMUP rounds are
discarded (code objects, rocFFT plans, the kinetic tables); median, min and max of ROUNDS rounds, and the shader clock
the chip held during the median round (the engine's stamps; "n/a" where the two stamps of a round disagree, as they can
when they land on different dies).
The forward step is timed twice: as the solver runs it (n steps per call: 2 fused passes per step) and one step per call
as the recomputation of a gradient runs it.  The backward substep is 15 batched 1-D rocFFT transforms + 1 copy + 11
passes over the field (27 launches).  Needs an MI355X.

``--stir`` times the stirred backward substep instead (pdeopt_gpe_rot_stir_adjoint_step, csrc/gpe_rot_adjoint.hip:
two moving spots and a ramp of Omega, device blocks) next to the plain backward substep of the frozen problem, in the
same run and binary, plain - stirred - plain, so a drift of the clock shows.

    PYTHONPATH=. python tools/gpe_rot_adjoint_bench.py [--stir] [--json out.json]
"""
import json
import sys

import numpy as np
import torch

import pde_opt_amd as P
from pde_opt_amd.engine import HipEngine
from pde_opt_amd.utils import prepare_solver_params

WARMUP, ROUNDS, ROUND_MS, DT = 3, 9, 50.0, 1e-3


def timed(eng, fn):
    """(median, min, max) microseconds per step of fn(reps), and the clock of the median round in MHz (0: not measured)"""
    eng.timer_start()
    fn(10)
    reps = max(10, int(ROUND_MS / (eng.timer_stop() / 10)))
    rows = []
    for _ in range(WARMUP + ROUNDS):
        eng.timer_start()
        fn(reps)
        ms = eng.timer_stop()
        mhz = eng.timer_clock_hz() / 1e6
        rows.append((ms * 1e3 / reps, mhz if 500.0 <= mhz <= 3000.0 else 0.0))
    rows = sorted(rows[WARMUP:])
    return rows[len(rows) // 2][0], rows[0][0], rows[-1][0], rows[len(rows) // 2][1]


def case(n, B, dtype):
    dom = P.Domain((n, n), ((-6.0, 6.0), (-6.0, 6.0)), "dimensionless")
    eq = P.GPE2DTSRot(dom, 50.0, 0.1, 0.6)
    solver = P.RotatingStrangSplitting(**prepare_solver_params(P.RotatingStrangSplitting, {"time_scale": 1.0}, eq))
    X, Y = dom.mesh()
    psi = np.exp(-0.5 * (X**2 + Y**2)) * (1.0 + 0.3 * X)
    psi /= np.sqrt(np.sum(psi**2) * dom.dx[0] ** 2)
    y0 = np.broadcast_to(np.stack([psi, np.zeros_like(psi)], axis=-1), (B, n, n, 2)).astype(dtype)
    eng = HipEngine(0)
    eng.configure(dtype=np.dtype(dtype), batch=B, **eq._engine_problem())
    eq._engine_upload(eng, 0.0, DT)
    solver.configure_engine(eng, eq)
    eng.set_state(y0)
    dev = torch.device("cuda", 0)
    psi0 = torch.as_tensor(y0).to(dev)
    lam = torch.ones_like(psi0)
    grad = torch.zeros((B, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def backward(reps):
        for _ in range(reps):
            eng.gpe_rot_adjoint_step(DT, psi0.data_ptr(), lam.data_ptr(), grad.data_ptr())

    def forward_single(reps):
        for _ in range(reps):
            eng.advance(solver.integrator, DT, 1)

    out = {"forward step (n per call)": timed(eng, lambda reps: eng.advance(solver.integrator, DT, reps)),
           "forward step (1 per call)": timed(eng, forward_single)}
    out["forward kernel"] = eng.last_kernel
    out["backward substep"] = timed(eng, backward)
    return out


def stir_case(n, B, dtype):
    from pde_opt_amd.numerics.functions.lights import GaussianSpot, GaussianSpots

    dom = P.Domain((n, n), ((-6.0, 6.0), (-6.0, 6.0)), "dimensionless")
    spots = GaussianSpots([GaussianSpot(3.0, 0.5, -0.6, 0.8, 0.3, -0.4, 0.7), GaussianSpot(-2.0, 1.0, 0.7, -0.5, -0.45, 0.6, 0.5)])
    X, Y = dom.mesh()
    psi = np.exp(-0.5 * (X**2 + Y**2)) * (1.0 + 0.3 * X)
    psi /= np.sqrt(np.sum(psi**2) * dom.dx[0] ** 2)
    y0 = np.broadcast_to(np.stack([psi, np.zeros_like(psi)], axis=-1), (B, n, n, 2)).astype(dtype)
    dev = torch.device("cuda", 0)
    psi0 = torch.as_tensor(y0).to(dev)
    lam = torch.ones_like(psi0)
    g3 = torch.zeros((B, 3), dtype=torch.float64, device=dev)
    g4 = torch.zeros((B, 4), dtype=torch.float64, device=dev)
    sg = torch.zeros((B, 2, 7), dtype=torch.float64, device=dev)

    def engine(**stir):
        eq = P.GPE2DTSRot(dom, 50.0, 0.1, 0.6, **stir)
        solver = P.RotatingStrangSplitting(**prepare_solver_params(P.RotatingStrangSplitting, {"time_scale": 1.0}, eq))
        eng = HipEngine(0)
        eng.configure(dtype=np.dtype(dtype), batch=B, **eq._engine_problem())
        eq._engine_upload(eng, 0.0, 1.0)
        solver.configure_engine(eng, eq)
        eng.set_state(y0)
        return eng

    plain_eng, stir_eng = engine(), engine(lights=spots, omega_rate=0.9)
    torch.cuda.synchronize()

    def plain(reps):
        for _ in range(reps):
            plain_eng.gpe_rot_adjoint_step(DT, psi0.data_ptr(), lam.data_ptr(), g3.data_ptr())

    def stirred(reps):
        for _ in range(reps):
            stir_eng.gpe_rot_stir_adjoint_step(0.3, DT, psi0.data_ptr(), lam.data_ptr(), g4.data_ptr(), sg.data_ptr())

    out = {"plain backward substep": timed(plain_eng, plain), "stirred backward substep": timed(stir_eng, stirred),
           "plain backward substep again": timed(plain_eng, plain)}
    out["stirred / plain"] = out["stirred backward substep"][0] / (0.5 * (out["plain backward substep"][0] +
                                                                          out["plain backward substep again"][0]))
    return out


if __name__ == "__main__":
    results = {}
    for n, B in ((256, 1), (512, 8)):
        for dtype in (np.float32, np.float64):
            key = f"{n}x{n}x{B} {np.dtype(dtype).name}"
            results[key] = stir_case(n, B, dtype) if "--stir" in sys.argv else case(n, B, dtype)
            for name, v in results[key].items():
                if isinstance(v, tuple):
                    clock = f"{v[3]:.0f} MHz" if v[3] else "clock n/a"
                    print(f"{key:20s} {name:28s} {v[0]:9.1f} us  (min {v[1]:.1f}, max {v[2]:.1f}; {clock})")
                elif isinstance(v, float):
                    print(f"{key:20s} {name:28s} {v:9.3f}")
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(results, f, indent=1)
