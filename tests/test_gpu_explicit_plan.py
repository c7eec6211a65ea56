"""What the explicit fixed-step advance decides (csrc/stencil.hip: plan_explicit -- the kernel family, the environment
groups, the two-stream schedule, the hipGraph replay), row by row on tiny problems.

Every row asserts last_kernel, last_groups, last_group_streams and the stage launches of the advance against literals
RECORDED from the library as it was before the plan existed (PDEOPT_LIB selects a library): the refactor that introduced
the plan may not change a decision, and the test passes unchanged against both libraries.  The automatic cache grouping
(a batch beyond the 256 MiB Infinity Cache, or beyond 2 M cells) needs the headline batches: test_gpu_groups.py has it.
"""
import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from test_gpu_groups import _advance
from util import MOB, MU, SBM_F, SBM_THETA, sbm_domain, sbm_psi, std_domain, white_noise_state

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TILED = {"small_persist": -1}  # keep the one-launch kernels out: the tiled families are under test

# id: (equation, dtype, shape, batch, integrator, substeps, set_group_envs, options,
#      (last_kernel, last_groups, last_group_streams, stage launches))
ROWS = {
    # the one-launch kernels, automatic policy
    "small_64x64": ("ch", F32, (64, 64), 2, L.INT_RK4, 4, 0, {},
        ("small_persist<f32,CH,logit,1x1024 threads,1 vec/thread,2 inputs>", 1, 1, 1)),
    "coop_128x128": ("ch", F32, (128, 128), 2, L.INT_RK4, 9, 0, {},
        ("rk4_coop<f32,CH,fixed closures,8x8 workgroups>", 1, 1, 1)),
    # RK4 families of Cahn-Hilliard fp32 64 x 128
    "ch_single": ("ch", F32, (64, 128), 3, L.INT_RK4, 4, 0, TILED,
        ("rk4_quad<f32,CH,logit,rows32>", 1, 1, 4)),
    "ch_pairs": ("ch", F32, (64, 128), 3, L.INT_RK4, 4, 0, dict(TILED, fuse_stages=1),
        ("stage_pair<f32,CH,logit,rows32>", 1, 1, 8)),
    "ch_stage": ("ch", F32, (64, 128), 3, L.INT_RK4, 4, 0, dict(TILED, fuse_stages=-1),
        ("stage_tiled<f32,CH,logit,rows16>", 1, 1, 16)),
    "ch_generic": ("ch", F32, (64, 128), 3, L.INT_RK4, 4, 0, dict(TILED, kernel_path=L.PATH_GENERIC),
        ("stage_generic<CH>", 1, 1, 16)),
    "ch_f64_pairs": ("ch", F64, (64, 128), 3, L.INT_RK4, 4, 0, TILED,
        ("stage_pair<f64,CH,logit,rows32>", 1, 1, 8)),
    "ac_single": ("ac", F32, (64, 128), 3, L.INT_RK4, 4, 0, TILED,
        ("rk4_quad<f32,AC,poly,rows32>", 1, 1, 4)),
    "ch_ragged_48x40": ("ch", F32, (48, 40), 3, L.INT_RK4, 4, 0, TILED,
        ("stage_pair<f32,CH,logit,rows16>", 1, 1, 8)),
    # Euler: pairs plus the odd tail, one substep alone, no pair kernels
    "euler_5": ("ch", F32, (64, 128), 3, L.INT_EULER, 5, 0, TILED,
        ("stage_tiled<f32,CH,logit,rows16>", 1, 1, 3)),
    "euler_1": ("ch", F32, (64, 128), 3, L.INT_EULER, 1, 0, TILED,
        ("stage_tiled<f32,CH,logit,rows16>", 1, 1, 1)),
    "euler_generic": ("ch", F32, (64, 128), 3, L.INT_EULER, 4, 0, dict(TILED, kernel_path=L.PATH_GENERIC),
        ("stage_generic<CH>", 1, 1, 4)),
    # hipGraph replay, 16 substeps per graph.  32 substeps: two replays, and the name says so; 40: the 8 substeps
    # launched after the replays leave their own name behind.  The launch counts do not depend on the replay.
    "graph_32": ("ch", F32, (64, 128), 2, L.INT_RK4, 32, 0, TILED,
        ("rk4_quad<f32,CH,logit,rows32>+hipGraph", 1, 1, 32)),
    "no_graph_32": ("ch", F32, (64, 128), 2, L.INT_RK4, 32, 0, dict(TILED, graph=-1),
        ("rk4_quad<f32,CH,logit,rows32>", 1, 1, 32)),
    "graph_40": ("ch", F32, (64, 128), 2, L.INT_RK4, 40, 0, TILED,
        ("rk4_quad<f32,CH,logit,rows32>", 1, 1, 40)),
    "no_graph_40": ("ch", F32, (64, 128), 2, L.INT_RK4, 40, 0, dict(TILED, graph=-1),
        ("rk4_quad<f32,CH,logit,rows32>", 1, 1, 40)),
    "euler_graph_32": ("ch", F32, (64, 128), 2, L.INT_EULER, 32, 0, TILED,
        ("stage_pair<f32,CH,logit,rows32>+hipGraph", 1, 1, 16)),
    # caller-chosen groups, one after the other and two side by side (the fifth environment's group runs alone)
    "groups_2_of_5": ("ch", F32, (64, 128), 5, L.INT_RK4, 4, 2, TILED,
        ("rk4_quad<f32,CH,logit,rows32>", 3, 1, 12)),
    "streams_2_of_5": ("ch", F32, (64, 128), 5, L.INT_RK4, 4, 2, dict(TILED, group_streams=2),
        ("rk4_quad<f32,CH,logit,rows32>", 3, 2, 12)),
    # host-evaluated time terms: the whole batch per sweep whatever was asked for, and no graph
    "sbm_timed": ("ac_sbm", F32, (48, 40), 3, L.INT_RK4, 32, 2, dict(TILED, group_streams=2),
        ("sbm_tiled<f32,AC-SBM>", 1, 1, 128)),
    # 3-D: groups, never side by side
    "ch3d": ("ch3d", F64, (16, 12, 20), 2, L.INT_RK4, 4, 1, dict(TILED, group_streams=2),
        ("stage_generic<CH-3D,logit>", 2, 1, 32)),
}


def run_row(name):
    """-> (final state, (last_kernel, last_groups, last_group_streams, stage launches)) of row `name`"""
    kind, dtype, shape, batch, integ, n, group, opts, _ = ROWS[name]
    rng = np.random.default_rng(sorted(ROWS).index(name))
    if kind == "ch":
        eq, noise, dt = P.CahnHilliard2DPeriodic(std_domain(P, *shape), 0.002, MU["regsol"], MOB["c1mc"]), "c", 2e-7
    elif kind == "ac":
        eq, noise, dt = P.AllenCahn2DPeriodic(std_domain(P, *shape), 0.002, MU["cubic"], MOB["one_plus_sq"]), "sym", 5e-5
    elif kind == "ac_sbm":
        dom = sbm_domain(P, sbm_psi(*shape))
        eq, noise, dt = P.AllenCahn2DSmoothedBoundary(dom, 1.5, SBM_F, MU["regsol"], MOB["c1mc"], SBM_THETA), "c", 2e-3
    else:
        nx, ny, nz = shape
        dom = P.Domain(shape, ((-0.005 * nx, 0.005 * nx), (-0.005 * ny, 0.005 * ny), (0.0, 0.012 * nz)), "dimensionless")
        eq, noise, dt = P.CahnHilliard3DPeriodic(dom, 0.002, MU["regsol"], MOB["c1mc"]), "c", 1e-7
    y0 = white_noise_state(rng, (batch,) + shape, dtype, noise)
    counters = {}
    out, groups, kernel = _advance(eq, None, y0, integ, dt, n, group, counters=counters, **opts)
    assert np.isfinite(out).all() and np.any(out != y0), name
    return out, (kernel, groups, counters["streams"], counters["launches"])


@pytest.mark.parametrize("name", list(ROWS))
def test_decisions_are_the_recorded_ones(name):
    _, got = run_row(name)
    print(name, got)
    assert got == ROWS[name][-1], (name, got)


def test_graph_replay_changes_the_name_only():
    """the rows with and without the replay issue the same launches; only a replay that ends the advance names it"""
    with_graph, without = ROWS["graph_32"][-1], ROWS["no_graph_32"][-1]
    assert with_graph[0] == without[0] + "+hipGraph" and with_graph[1:] == without[1:]
    assert ROWS["graph_40"][-1] == ROWS["no_graph_40"][-1]
    assert [k for k, r in ROWS.items() if r[-1][0].endswith("+hipGraph")] == ["graph_32", "euler_graph_32"]
