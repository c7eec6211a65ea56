"""Per-phase cycle profile of ch_rk4_quad_kernel from in-kernel clock stamps (csrc/stencil_fused_ch4.hpp, PDEOPT_CH4_STAMPS).

    tools/mkvariant.sh ch4stamps -DPDEOPT_CH4_STAMPS [-DPDEOPT_CH4_RING_CELLS=0 -DPDEOPT_CH4_HOIST=0]
    python tools/ch4_phase_profile.py --lib variants/lib_ch4stamps.so --label "..." [--out profiles/r05_ch4_phase_cycles.txt]

Runs the headline shape (bench.py's ch_rk4_1024_f32: 32 environments of 1024^2, two groups side by side) for a few RK4
substeps on the profiling build of the library and reads the stamps of the LAST substep: lane 0 of every wave stored
s_memtime at entry, at the end of its own work in each phase, after the barrier that ends the phase, and after its
first trip in the mu passes and rings.  The stamps cost cycles of their own (about 40 each, 26 per wave), their waits
forbid overlaps the shipped kernel has, and the profiling build of this 64-register kernel spills about 20 registers
to scratch: read the SHARES and the differences, not the total.

Per phase (one row), over the workgroups of the batch:
  interval     barrier to barrier (entry to the first barrier for the load; last barrier to the last wave's end for k4)
  last / med   the time from the phase's start to the end of the own work of the slowest / the median wave of a workgroup
  idle         last - med: what the median wave waits at the barrier for
  own / help   the median owner wave (waves 0-7: they march) and helper wave (8-15: they take the rings)
  trip 2+      the part of `last` after that wave's first trip (mu passes and stage 1's ring: the ragged trips)
all as medians over the workgroups, in s_memtime ticks (shader cycles).
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ["load", "mu1 (tile+7)", "k1 + ring", "mu2 (tile+5)", "k2 + ring", "mu3 (tile+3)", "k3 + ring", "mu4 (tile+1)", "k4 + store"]
SLOTS, WAVES = 32, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="a library built with -DPDEOPT_CH4_STAMPS")
    ap.add_argument("--label", default="")
    ap.add_argument("--substeps", type=int, default=6)
    ap.add_argument("--out", default=None, help="append the table to this file")
    args = ap.parse_args()
    os.environ["PDEOPT_LIB"] = os.path.abspath(args.lib)

    import torch

    import bench
    import pde_opt_amd as P
    from pde_opt_amd import _lib as L

    w = bench.WORKLOADS["ch_rk4_1024_f32"]
    eq, y0, solver = bench.make_problem(P, "ch_rk4_1024_f32", w["batch"], 0)
    tiles = (w["n"] // 32) * (w["n"] // 128)
    nwg = w["batch"] * tiles
    buf = torch.zeros(nwg * WAVES * SLOTS, dtype=torch.int64, device="cuda")
    lib = ctypes.CDLL(L.LIB_PATH)
    lib.pdeopt_ch4_set_stamps.argtypes = [ctypes.c_void_p]
    lib.pdeopt_ch4_set_stamps.restype = None
    lib.pdeopt_ch4_set_stamps(ctypes.c_void_p(buf.data_ptr()))

    eng = P.HipEngine(0)
    eng.configure(dtype=y0.dtype, batch=w["batch"], **eq._engine_problem())
    eq._engine_upload(eng, 0.0, w["dt"] * args.substeps)
    solver.configure_engine(eng, eq)
    eng.set_state(y0)
    eng.advance(solver.integrator, w["dt"], args.substeps, 0.0)
    eng.sync()
    kern = eng.last_kernel
    eng.close()
    torch.cuda.synchronize()
    st = buf.cpu().numpy().reshape(nwg, WAVES, SLOTS).astype(np.int64)
    assert "rk4_quad" in kern and "rows32" in kern, kern
    assert (st[:, :, 0] > 0).all() and (st[:, :, 25] > 0).all(), "a wave left no stamps: not the profiling build?"

    done = st[:, :, 1:26:3]                                                # (wg, wave, 9) own work finished
    start = np.concatenate([st[:, :, :1], st[:, :, 2:24:3]], axis=2)       # entry, then past barrier p - 1
    mid = st[:, :, 3:27:3]                                                 # first trip finished (0: the wave took none)
    mid = np.concatenate([mid, np.zeros_like(mid[:, :, :1])], axis=2)[:, :, :9]
    wg_start = np.concatenate([st[:, :, 0].min(axis=1, keepdims=True), np.median(st[:, :, 2:24:3], axis=1)], axis=1)  # (wg, 9)
    wg_end = np.concatenate([wg_start[:, 1:], st[:, :, 25].max(axis=1, keepdims=True)], axis=1)
    interval = wg_end - wg_start
    work = done - start                                                    # (wg, wave, 9)
    last_w = work.argmax(axis=1)                                           # (wg, 9) the slowest wave
    last = np.take_along_axis(work, last_w[:, None, :], axis=1)[:, 0, :]
    med = np.median(work, axis=1)
    own, helper = np.median(work[:, : WAVES // 2], axis=1), np.median(work[:, WAVES // 2:], axis=1)
    mid_last = np.take_along_axis(mid, last_w[:, None, :], axis=1)[:, 0, :]
    done_last = np.take_along_axis(done, last_w[:, None, :], axis=1)[:, 0, :]
    trip2 = np.where(mid_last > 0, done_last - mid_last, 0)

    m = lambda a: float(np.median(a))
    total = m(interval.sum(axis=1))
    lines = [f"== {args.label or os.path.basename(args.lib)}: {kern}, {w['batch']} x {w['n']}^2, substep {args.substeps} of {args.substeps}, "
             f"{nwg} workgroups x {WAVES} waves",
             f"{'phase':<14}{'interval':>9}{'share':>7}{'last':>8}{'med':>8}{'idle':>7}{'own':>8}{'help':>8}{'trip 2+':>9}"]
    for p, name in enumerate(PHASES):
        lines.append(f"{name:<14}{m(interval[:, p]):>9.0f}{100 * m(interval[:, p]) / total:>6.1f}%{m(last[:, p]):>8.0f}{m(med[:, p]):>8.0f}"
                     f"{m(last[:, p] - med[:, p]):>7.0f}{m(own[:, p]):>8.0f}{m(helper[:, p]):>8.0f}{m(trip2[:, p]):>9.0f}")
    ragged = [1, 2, 3, 5, 7]
    lines.append(f"{'tile':<14}{total:>9.0f}   sum of idle {sum(m(last[:, p] - med[:, p]) for p in range(9)):.0f}, of trip 2+ in the mu passes "
                 f"and stage 1's ring {sum(m(trip2[:, p]) for p in ragged):.0f} ({100 * sum(m(trip2[:, p]) for p in ragged) / total:.1f} % of the tile)")
    lines.append(f"entry to first barrier (exposed tile load + workgroup start-up): {m(interval[:, 0]):.0f} = {100 * m(interval[:, 0]) / total:.1f} % of the tile")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
