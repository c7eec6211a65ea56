"""Time one forward substep and one adjoint substep of the field-mu path (pde_opt_amd.fieldmu, csrc/fieldmu.hip), each
split into the library's launches and torch's share (the CNN forward; its backward), at 32^2 x 3 and 128^2 x 3 with the
notebook's PeriodicCNN(1, (32, 64, 64), 1), fp32 and fp64.

HIP events on the stream the engine and torch share; the first rounds are discarded as warm-up; the number of calls in a
timed window is set per case from a trial window so that the window lasts about 50 ms.  Needs an MI355X.

    PYTHONPATH=. python tools/fieldmu_bench.py [--json out.json]

``--native-cnn``: instead, the CNN's share of a forward and of a backward substep at 128^2 x 3, evaluated by torch and by
the library's own kernels (csrc/cnn.hip, ``FieldMuSolver.native_cnn``) on the same state in one run, fp32 and fp64, with
the shader clock held during the native windows.  The backward share is what the sweep runs per substep: torch's forward
under autograd + backward, or ``pdeopt_cnn_forward`` (mu_h for the adjoint kernel) + ``pdeopt_cnn_vjp``.

``--native-mixer``: the same comparison for ``Mixer2d((1, 128, 128), 8, 32, 128, 64, 4)`` (patch 8: 32 x 256 activations),
torch against csrc/mixer.hip (``FieldMuSolver.native_mixer``).
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
from pde_opt_amd.numerics.functions.mixer import Mixer2d

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


def native_case(n, B, dtype, mixer=False):
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    dom = P.Domain((n, n), ((0.0, 0.01 * n), (0.0, 0.01 * n)), "dimensionless")
    cnn = (Mixer2d((1, n, n), 8, 32, 128, 64, 4) if mixer else PeriodicCNN(1, (32, 64, 64), 1)).to(tdt).to("cuda")
    eq = P.CahnHilliard2DPeriodic(dom, 0.002, cnn, DiffusionLegendrePolynomials(np.array([0.0])))
    solver = P.SemiImplicitFourierSpectral(A=0.5, fourier_symbol=eq.fourier_symbol)
    fm = FieldMuSolver(0)
    y0 = np.clip(0.5 + 0.05 * np.random.default_rng(0).standard_normal((B, n, n)), 0.05, 0.95).astype(dtype)
    res = {}
    with torch.cuda.stream(fm.stream):
        Y, mu_of = fm._prepare(eq, solver, y0, 0.0, 1.0)
        u0 = Y.clone()
        gmu, lam = torch.randn_like(Y), torch.zeros_like(Y)
        with torch.no_grad():
            res["forward: torch"] = timed(fm.stream, lambda: mu_of(u0))
        u = u0.clone().requires_grad_(True)

        def torch_backward():
            u.grad = None
            mu_of(u).backward(gmu)

        res["backward: torch (forward + backward)"] = timed(fm.stream, torch_backward)
        fm.native_cnn, fm.native_mixer = not mixer, mixer
        _, native_mu = fm._prepare(eq, solver, y0, 0.0, 1.0)
        net = fm._mixer if mixer else fm._cnn

        def native_backward():
            native_mu(u0)
            net.vjp(u0.data_ptr(), gmu.data_ptr(), lam.data_ptr())

        fm.engine.timer_start()
        res["forward: native"] = timed(fm.stream, lambda: native_mu(u0))
        res["backward: native (forward + vjp)"] = timed(fm.stream, native_backward)
        res["backward: native (vjp alone)"] = timed(fm.stream, lambda: net.vjp(u0.data_ptr(), gmu.data_ptr(), lam.data_ptr()))
        fm.engine.timer_stop()
        res["shader clock during the native windows, MHz"] = fm.engine.timer_clock_hz() / 1e6
        net.grad_read(reset=True)
    return res


if __name__ == "__main__":
    results = {}
    native = "--native-cnn" in sys.argv or "--native-mixer" in sys.argv
    if native:
        for dtype in (np.float32, np.float64):
            key = f"128x128x3 {np.dtype(dtype).name}"
            results[key] = native_case(128, 3, dtype, mixer="--native-mixer" in sys.argv)
            for name, v in results[key].items():
                print(f"{key:18s} {name:45s} " + (f"{v:9.0f}" if np.isscalar(v) else f"{v[0]:9.1f} us  (min {v[1]:.1f}, max {v[2]:.1f})"),
                      flush=True)
    for n in () if native else (32, 128):
        for dtype in (np.float32, np.float64):
            key = f"{n}x{n}x3 {np.dtype(dtype).name}"
            results[key] = case(n, 3, dtype)
            for name, (med, lo, hi) in results[key].items():
                print(f"{key:18s} {name:45s} {med:9.1f} us  (min {lo:.1f}, max {hi:.1f})")
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(results, f, indent=1)
