"""Time one forward substep and one adjoint substep of the field-mu path (pde_opt_amd.fieldmu, csrc/fieldmu.hip), each
split into the library's launches and torch's share (the CNN forward; its backward), at 32^2 x 3 and 128^2 x 3 with the
notebook's PeriodicCNN(1, (32, 64, 64), 1), fp32 and fp64.

HIP events on the stream the engine and torch share; the first rounds are discarded as warm-up; the number of calls in a
timed window is set per case from a trial window so that the window lasts about 50 ms.  Needs an MI355X.

    PYTHONPATH=. python tools/fieldmu_bench.py [--json out.json]
"""
import json
import sys

import numpy as np
import torch

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd.fieldmu import FieldMuSolver
from pde_opt_amd.numerics.functions.cnn import PeriodicCNN
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials

WARMUP, ROUNDS, WINDOW_MS = 3, 7, 50.0


def window(stream, fn, reps):
    """milliseconds of `reps` calls of fn between two events on the stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def timed(stream, fn):
    """(median, min, max) over ROUNDS windows of the mean time of a call of fn, in microseconds"""
    window(stream, fn, 3)  # first launches load code objects and pick algorithms
    reps = max(3, int(np.ceil(WINDOW_MS / max(window(stream, fn, 10) / 10, 1e-4))))
    out = [window(stream, fn, reps) * 1e3 / reps for _ in range(WARMUP + ROUNDS)][WARMUP:]
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def case(n, B, dtype):
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    dom = P.Domain((n, n), ((0.0, 0.01 * n), (0.0, 0.01 * n)), "dimensionless")
    cnn = PeriodicCNN(1, (32, 64, 64), 1).to(tdt).to("cuda")
    eq = P.CahnHilliard2DPeriodic(dom, 0.002, cnn, DiffusionLegendrePolynomials(np.array([0.0])))
    solver = P.SemiImplicitFourierSpectral(A=0.5, fourier_symbol=eq.fourier_symbol)
    fm = FieldMuSolver(0)
    y0 = np.clip(0.5 + 0.05 * np.random.default_rng(0).standard_normal((B, n, n)), 0.05, 0.95).astype(dtype)
    res = {}
    with torch.cuda.stream(fm.stream):
        Y, mu_of = fm._prepare(eq, solver, y0, 0.0, 1.0)
        u0 = Y.clone()
        dt = 1e-6
        with torch.no_grad():
            mu = mu_of(Y)
            res["forward: library (rhs + IMEX)"] = timed(fm.stream, lambda: fm.engine.fieldmu_step(L.INT_IMEX, dt, mu.data_ptr()))
            Y.copy_(u0)
            res["forward: torch (CNN)"] = timed(fm.stream, lambda: mu_of(Y))
        lam, gmu = torch.randn_like(Y), torch.empty_like(Y)
        u = u0.clone().requires_grad_(True)
        mu_g = mu_of(u)
        res["adjoint: library (IMEX + adjoint kernel)"] = timed(
            fm.stream, lambda: fm.engine.fieldmu_adjoint_step(L.INT_IMEX, dt, u.data_ptr(), mu_g.data_ptr(), lam.data_ptr(), gmu.data_ptr()))

        def torch_part():
            u.grad = None
            mu_of(u).backward(gmu)

        res["adjoint: torch (CNN forward + backward)"] = timed(fm.stream, torch_part)
    return res


if __name__ == "__main__":
    results = {}
    for n in (32, 128):
        for dtype in (np.float32, np.float64):
            key = f"{n}x{n}x3 {np.dtype(dtype).name}"
            results[key] = case(n, 3, dtype)
            for name, (med, lo, hi) in results[key].items():
                print(f"{key:18s} {name:45s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f})")
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(results, f, indent=1)
