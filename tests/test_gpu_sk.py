"""The structure factor on the MI355X (csrc/structure_factor.hip) against its numpy reference (tests/sk_ref.py).

Inputs: white noise on a mean, ``0.5 + 0.1 standard_normal`` -- broadband, every shell populated, a large zero mode.
Grids: 37 x 130 (nh = 66 spills two lanes into a second chunk of 64; 37 rows are no multiple of the 32-row block),
24 x 33 with L = (1, 1.7) (odd last axis: no Nyquist column; nh = 17 < 64; unequal tables), 64 x 64, 12 x 10 x 18 and
9 x 16 x 34 with L = (1, 0.8, 1.3).

Gates.  fp64: every shell within 1e-12 x max_b P_b of the reference, the project's usual fp64 margin over a transform's
eps log N.  fp32: the distance in the same norm, max_b |P - P_ref| / max_b P_ref, is measured against the reference's own
float32 error -- the same sums from ``torch.fft.rfftn`` on the CPU at complex64 against the fp64 reference, on the same
float32 inputs -- and gated at twice the measured ratio FP32_RATIO."""
import ctypes as C

import numpy as np
import pytest

import pde_opt_amd as P
import sk_ref as R
from pde_opt_amd import _lib as L
from pde_opt_amd import structure_factor as SK
from pde_opt_amd.engine import HipEngine

pytestmark = pytest.mark.gpu

# worst ratio (device distance) / (complex64 CPU reference's distance) over the five grids and three environments,
# measured on one MI355X: 1.61 on 12 x 10 x 18 (the others between 0.55 and 1.52; distances 5e-8 .. 6e-7)
FP32_RATIO = 1.61

EQ_CODE = {2: L.EQ_CAHN_HILLIARD, 3: L.EQ_CAHN_HILLIARD_3D}


@pytest.fixture(scope="module")
def engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


def domain(points, lengths):
    return P.Domain(tuple(points), tuple((0.0, v) for v in lengths), "dimensionless")


def load(engine, points, lengths, states):
    dom = domain(points, lengths)
    h = dom.dx
    kw = dict(nz=points[2], hz=h[2]) if len(points) == 3 else {}
    engine.configure(equation=EQ_CODE[len(points)], dtype=states.dtype, nx=points[0], ny=points[1], batch=len(states), hx=h[0], hy=h[1], **kw)
    engine.set_state(states)
    tabs = SK.shell_tables(dom)
    SK.upload_tables(engine, tabs)
    return tabs


def complex64_reference(u32, lengths):
    """the reference's own float32 error: the transform at complex64 on the CPU, the squares and the sums in fp64"""
    torch = pytest.importorskip("torch")
    points = u32.shape[1:]
    b, w, n_bins, _ = R.half_bins(points, lengths)
    uh = torch.fft.rfftn(torch.from_numpy(u32), dim=tuple(range(1, u32.ndim))).numpy()
    assert uh.dtype == np.complex64
    return R.shell_sums(uh.real.astype(np.float64) ** 2 + uh.imag.astype(np.float64) ** 2, b, w, n_bins)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("points,lengths", R.GRIDS)
def test_parity_determinism_and_ranges(engine, points, lengths, dtype):
    states = R.white_noise(points, 3, seed=sum(points)).astype(dtype)
    tabs = load(engine, points, lengths, states)
    got = engine.structure_factor()
    assert got.shape == (3, tabs.n_bins) and engine.last_kernel.startswith("structure_factor<")
    # determinism: a repeat and a sub-range give the same bits
    assert np.array_equal(engine.structure_factor(), got)
    assert np.array_equal(engine.structure_factor(env_first=1, env_count=2), got[1:3])
    assert np.array_equal(engine.structure_factor(env_first=2), got[2:])
    assert np.array_equal(engine.get_state(), states)  # the state is not modified
    want, counts, _ = R.power(states, lengths)
    assert np.array_equal(counts, tabs.counts)
    scale = want.max(axis=1)
    dist = np.abs(got - want).max(axis=1) / scale
    if dtype == np.float64:
        print(points, "fp64 distance / 1e-12:", dist / 1e-12)
        assert np.all(dist <= 1e-12)
    else:
        own = np.abs(complex64_reference(states, lengths) - want).max(axis=1) / scale
        print(points, "fp32 distance:", dist, "complex64 reference's:", own, "ratio:", dist / own)
        assert np.all(dist <= 2.0 * FP32_RATIO * own)
    # Parseval: the shell sums add up to N^2 var(u)
    sf = SK.from_engine(engine, tabs, got)
    n = int(np.prod(points))
    eps = np.finfo(dtype).eps
    var = states.astype(np.float64).reshape(3, -1).var(axis=1)
    assert np.all(np.abs(sf.variance - var) <= 8 * eps * np.log2(n) * (var + 0.25))  # (0.25: the mean's square, removed by hand)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_plane_wave_sits_in_one_shell(engine, dtype):
    """Rounding leaves at most (c eps log2 N)^2 sum u^2 per mode beside the wave, c a small constant of the transform; over all
    modes, against the peak N^2 0.02 with sum u^2 = 0.11 N, that is 5.5 (c eps log2 N)^2: 1e-20 holds in fp64 as on the
    reference, and c = 4 gives 4e-11 in fp32, to which the input's own rounding (eps / 2 of 0.5 per cell, white) adds
    (0.5 eps / 2)^2 / 0.02 = 1e-14"""
    u = R.plane_wave().astype(dtype)
    tabs = load(engine, u.shape, (1.0, 1.0), np.stack([u, u, u]))
    p = engine.structure_factor()
    peak = u.size**2 * 0.02
    assert np.all(np.abs(p[:, 5] - peak) <= 64 * np.finfo(dtype).eps * peak)
    others = np.delete(p, 5, axis=1)
    bound = 1e-20 if dtype == np.float64 else 5.5 * (4 * np.finfo(np.float32).eps * np.log2(u.size)) ** 2 + 1e-14
    print(np.dtype(dtype).name, "largest other shell / peak:", others.max() / peak, "bound", bound)
    assert np.all(others <= bound * peak)
    sf = SK.from_engine(engine, tabs, p)
    np.testing.assert_allclose(sf.length, 0.2, rtol=1e-6)


CH = dict(kappa=1e-3, mu=lambda c: np.log(c / (1.0 - c)) + 3.0 * (1.0 - 2.0 * c), D=lambda c: c * (1.0 - c))


def test_trace_rows_are_structure_factor_of_the_frames(engine):
    """IMEX on 64 x 64, 3 save points on step edges: ``solve`` issues the same advance calls for the same segments"""
    dom = domain((64, 64), (1.0, 1.0))
    y0 = R.white_noise((64, 64), 3, seed=5)
    assert 0.05 < y0.min() and y0.max() < 0.95  # inside the logarithm's domain
    m = P.PDEModel(P.CahnHilliard2DPeriodic, dom, P.SemiImplicitFourierSpectral)
    m._engine = engine
    dt = 5e-6
    ts = np.arange(3) * (20 * dt)
    trace = m.structure_factor_trace(CH, y0, ts, solver_parameters={"A": 0.5}, dt0=dt)
    assert trace.power.shape == (3, 3, SK.shell_tables(dom).n_bins) and trace.length.shape == (3, 3)
    frames = m.solve(CH, y0, ts, solver_parameters={"A": 0.5}, dt0=dt)
    for q in range(3):
        at = m.structure_factor(frames[q])
        assert np.array_equal(trace.power[q], at.power), q
        assert np.array_equal(trace.length[q], at.length), q
    assert np.all(np.isfinite(trace.length)) and np.all(trace.variance[-1] != trace.variance[0])


@pytest.mark.parametrize("points", [(64, 64), (48, 40)])
def test_a_call_between_advances_leaves_the_next_step_bitwise_unchanged(engine, points):
    """the hermitian work field is scratch between steps (64 x 64 steps with the hand-written passes, 48 x 40 with the
    rocFFT plans whose work field the call shares)"""
    from pde_opt_amd.phase_field_observables import _load
    from pde_opt_amd.utils import prepare_solver_params

    dom = domain(points, (1.0, 1.0))
    y0 = R.white_noise(points, 3, seed=7)
    assert 0.05 < y0.min() and y0.max() < 0.95  # inside the logarithm's domain
    m = P.PDEModel(P.CahnHilliard2DPeriodic, dom, P.SemiImplicitFourierSpectral)
    m._engine = engine
    eq = P.CahnHilliard2DPeriodic(domain=dom, **CH)
    solver = P.SemiImplicitFourierSpectral(**prepare_solver_params(P.SemiImplicitFourierSpectral, {"A": 0.5}, eq))
    tabs = SK.shell_tables(dom)
    dt = 5e-6

    def run(observe):
        eng = _load(m, [eq], solver, y0, 0.0, 5 * dt)
        rows = []
        for first, n in ((0, 2), (2, 3)):
            if observe:
                SK.upload_tables(eng, tabs)
                rows.append(eng.structure_factor())
            eng.advance(solver.integrator, dt, n, first * dt)
        return eng.get_state(), rows

    plain, _ = run(False)
    watched, rows = run(True)
    assert np.array_equal(plain, watched)
    assert not np.array_equal(plain, y0) and not np.array_equal(rows[0], rows[1])


def test_the_device_reward_is_the_length_of_the_fetched_states(engine):
    dom = domain((64, 64), (1.0, 1.0))  # (a per-environment kappa under IMEX needs >= 64)
    y0 = R.white_noise((64, 64), 3, seed=5)
    env = P.VectorPDEEnv(3, P.CahnHilliard2DPeriodic, dom, P.SemiImplicitFourierSpectral, end_time=1.0, step_dt=2e-4, numeric_dt=5e-6,
                         state_to_observation_func=lambda s: s, reward_function=None,
                         reset_func=lambda d, seed=0: y0[seed % 3], reset_control_value=1e-3,
                         update_control_value=lambda a, v: v * (1.0 + 0.5 * float(np.ravel(a)[0])), update_control_parameter=lambda old, new: new,
                         action_space_config={"shape": (1,)}, static_equation_parameters=dict(mu=CH["mu"], D=CH["D"]),
                         control_equation_parameter_name="kappa", solver_parameters={"A": 0.5}, device_reward=("structure_factor", "length"),
                         fetch_observations=False, engine=engine)
    env.reset(seed=0)
    m = P.PDEModel(P.CahnHilliard2DPeriodic, dom, P.SemiImplicitFourierSpectral)  # (an engine of its own)
    for _ in range(2):
        _, rewards, *_ = env.step(np.array([[0.0], [0.4], [-0.4]]))
        want = m.structure_factor(env.states).length  # fetched separately
        assert np.array_equal(np.asarray(rewards), want)
    assert len(set(np.asarray(rewards))) == 3 and np.all(np.isfinite(rewards))


def test_the_c_calls_refuse_what_they_do_not_cover(engine):
    lib, h = engine._lib, engine._h
    out = np.zeros((3, 64))
    err = lambda: lib.pdeopt_last_error(h)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda first=0, count=1: lib.pdeopt_structure_factor(h, first, count, ptr(out))
    tabs = SK.shell_tables(domain((16, 16), (1.0, 1.0)))
    conf = lambda n_bins=tabs.n_bins, t=tabs.tables: lib.pdeopt_sk_configure(h, ptr(t[0]), ptr(t[1]), None, n_bins)
    # a complex state
    engine.configure(equation=L.EQ_GPE, dtype=np.float64, nx=16, ny=16, batch=1, hx=1.0, hy=1.0)
    assert conf() == L.EINVAL and b"complex" in err()
    assert call() == L.EINVAL and b"complex" in err()
    # the padded layout
    engine.set_halo_layout(4)
    engine.configure(equation=L.EQ_CAHN_HILLIARD, dtype=np.float64, nx=16, ny=16, batch=1, hx=1.0, hy=1.0)
    assert conf() == L.EINVAL and b"padded" in err()
    assert call() == L.EINVAL and b"padded" in err()
    engine.set_halo_layout(0)
    engine.configure(equation=L.EQ_CAHN_HILLIARD, dtype=np.float64, nx=16, ny=16, batch=3, hx=1.0, hy=1.0)
    # no tables yet
    assert call() == L.ESTATE and b"pdeopt_sk_configure" in err()
    # an n_bins the tables do not imply, a table for a third axis, more shells than the kernel holds, a decreasing table
    assert conf(tabs.n_bins + 1) == L.EINVAL and b"imply" in err()
    assert lib.pdeopt_sk_configure(h, ptr(tabs.tables[0]), ptr(tabs.tables[1]), ptr(tabs.tables[1]), tabs.n_bins) == L.EINVAL
    wide = np.zeros(16)
    wide[1] = 1.7e7
    assert conf(4124, (wide, np.zeros(16))) == L.EINVAL and b"4096" in err()  # 1 + floor(sqrt(1.7e7) + 0.5)
    down = tabs.tables[1].copy()
    down[3] = 0.0
    assert conf(t=(tabs.tables[0], down)) == L.EINVAL and b"decreases" in err()
    assert call() == L.ESTATE  # none of the refused calls left tables behind
    assert conf() == L.OK and call(0, 3) == L.OK
    # a bad range
    assert call(2, 2) == L.EINVAL and call(-1, 1) == L.EINVAL
    # another grid drops the tables
    engine.configure(equation=L.EQ_CAHN_HILLIARD, dtype=np.float64, nx=16, ny=20, batch=3, hx=1.0, hy=1.0)
    assert call() == L.ESTATE and b"pdeopt_sk_configure" in err()


def test_state_error_before_configure():
    eng = HipEngine(0)
    try:
        out, t = np.zeros((1, 8)), np.zeros(8)
        assert eng._lib.pdeopt_structure_factor(eng._h, 0, 1, out.ctypes.data_as(C.c_void_p)) == L.ESTATE
        assert eng._lib.pdeopt_sk_configure(eng._h, t.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), None, 1) == L.ESTATE
    finally:
        eng.close()
