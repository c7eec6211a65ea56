"""bench.py's workload definitions on the CPU: every adaptive workload builds its problem and its parity / CPU-baseline leg
(the same solve driven step by step on the numpy oracle) runs; the 3-D workload's problem has the shape the line reports."""
import numpy as np
import pytest

import bench
import pde_opt_amd as P
from fake_engine import OracleEngine


@pytest.mark.parametrize("name", sorted(bench.ADAPTIVE))
def test_adaptive_workload_problem_and_oracle_leg(name):
    w = bench.ADAPTIVE[name]
    eq, y0 = bench.adaptive_problem(P, name)
    assert y0.shape == (w["n"], w["n"]) and np.all(np.isfinite(y0))
    ctl = P.PIDController(rtol=w["rtol"], atol=w["atol"])
    t1 = w["t1"] / 20  # a prefix: the bench line runs the whole span
    sol = P.diffeqsolve(eq, P.Tsit5(), 0.0, t1, w["dt0"], y0.astype(np.float64), stepsize_controller=ctl, engine=OracleEngine(),
                        saveat=P.SaveAt(ts=np.linspace(0.0, t1, 2)))
    assert sol.stats["num_accepted_steps"] > 5 and np.all(np.isfinite(sol.ys))
    # the notebook's problem: phase boundary at mid-width inside a disc-shaped level set / a steady velocity field
    if name.startswith("ch_sbm"):
        assert eq.psi.shape == y0.shape and 0.0 < eq.psi.min() < 0.01 and eq.psi.max() > 0.99
        assert abs(float(y0[:, : w["n"] // 2].mean()) - 0.1) < 1e-12 and abs(float(y0[:, w["n"] // 2:].mean()) - 0.9) < 1e-12


def test_3d_workload_problem():
    w = dict(bench.WORKLOADS["ch3d_rk4_128_f32"])
    bench.WORKLOADS["_ch3d_small"] = dict(w, n=12)
    try:
        eq, y0, solver = bench.make_problem(P, "_ch3d_small", 2, 0)
    finally:
        del bench.WORKLOADS["_ch3d_small"]
    assert y0.shape == (2, 12, 12, 12) and y0.dtype == np.float32 and len(eq.domain.points) == 3
    assert solver.integrator == P.RK4().integrator


def test_dump_outputs_budget_dtype_and_fixed_sample(tmp_path):
    """--dump-outputs: float32 kept, anything else as float64, at most the budget in all; an output above its share is
    a seed-0 sample (whole environments in index order, or single elements of a one-axis array), the same every run"""
    rng = np.random.default_rng(1)
    arrays = {"state": rng.standard_normal((32, 16, 16)).astype(np.float32), "big": rng.standard_normal(5000), "count": np.arange(3)}
    budget = 30000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert (got["state"].dtype, got["big"].dtype, got["count"].dtype) == (np.float32, np.float64, np.float64)
    assert sum(a.nbytes for a in got.values()) <= budget
    np.testing.assert_array_equal(got["count"], [0, 1, 2])
    envs = [int(np.flatnonzero((arrays["state"] == s).all(axis=(1, 2)))[0]) for s in got["state"]]
    assert len(envs) > 1 and envs == sorted(envs)
    assert 0 < got["big"].size < 5000 and np.isin(got["big"], arrays["big"]).all()
    for n in arrays:
        np.testing.assert_array_equal(np.load(tmp_path / "b" / f"{n}.npy"), got[n])


def test_single_process_plain_run_dumps_outputs_without_the_full_legs(tmp_path):
    """a plain run (no --full) times the steps and writes the outputs; the parity spot is a --full leg"""
    import argparse
    import contextlib
    import io

    args = argparse.Namespace(workload="ch_rk4_64_f32_small", batch_per_gpu=1, gpus=2, steps=1, warmup=0, no_parity_spot=False,
                              full=False, dump_outputs=str(tmp_path))
    with contextlib.redirect_stdout(io.StringIO()):
        line = bench.run_single_process(args, P, engines=[OracleEngine(), OracleEngine()])
    assert "parity_spot_ok" not in line and line["ms_per_step"] > 0 and line["steps"] == 1
    state, reward = np.load(tmp_path / "state.npy"), np.load(tmp_path / "reward.npy")
    assert state.shape == (2, 64, 64) and reward.shape == (2,) and np.isfinite(state).all() and np.isfinite(reward).all()
