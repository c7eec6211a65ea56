"""Fixed-step explicit Euler / RK4 for ONE environment on several compute units (csrc/stencil_coop_adaptive.hpp, MODE 1;
VERDICT r3 Weak #6): the communication-avoiding tiling of the adaptive kernel -- tile + 8 halo in LDS, as many substeps per
exchange as the halo pays for, one neighbour exchange per round -- for single environments of 96^2 - 320^2 cells, which the
tiled kernels advance at two dependent launches per substep whatever their size.

Gates: the CPU oracle on the same inputs (fp64 1e-9 of the increment; fp32 the state's rounding), and the tiled path on the
same GPU (fp64: rounding of a different association only)."""
import numpy as np
import pytest

import pde_opt_amd as P
from oracle import np_oracle as O
from pde_opt_amd import _lib as L
from util import MOB, MU, SBM_F, SBM_FLUX, SBM_THETA, inc_tol_f32, rel_l2, sbm_domain, sbm_psi, std_domain

pytestmark = pytest.mark.gpu


def _advance(eq, y0, integ, dt, n, opt, t0=0.0, kappas=None):
    eng = P.HipEngine()
    eng.set_small_persist(opt)
    eng.configure(dtype=y0.dtype, batch=y0.shape[0], **eq._engine_problem())
    eq._engine_upload(eng, t0, dt * n)
    if kappas is not None:
        eng.set_env_params(0, kappa=kappas)
    eng.set_state(y0)
    eng.advance(integ, dt, n, t0)
    out, kern = eng.get_state(), eng.last_kernel
    eng.close()
    return out, kern


def _check(got, ref, y0, dtype, kern):
    inc_g, inc_w = got.astype(np.float64) - y0, ref - y0
    if dtype is np.float64:
        assert rel_l2(inc_g, inc_w) < 1e-9, (kern, rel_l2(inc_g, inc_w))
    else:
        assert np.max(np.abs(got - ref)) < 2e-6, (kern, float(np.max(np.abs(got - ref))))
        assert rel_l2(inc_g, inc_w) < inc_tol_f32(ref, y0), (kern, rel_l2(inc_g, inc_w))


# square, a ragged split (100 = 7 x 14.3), non-square, a grid on several XCDs, one the one-CU kernel also takes (forced)
@pytest.mark.parametrize("shape", [(128, 128), (100, 100), (72, 120), (256, 256), (64, 64)], ids=str)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["ch", "ac"])
def test_periodic_fixed_step_vs_oracle_and_tiled_path(shape, dtype, kind):
    nx, ny = shape
    dom = std_domain(P, nx, ny)
    rng = np.random.default_rng(nx * 1000 + ny)
    if kind == "ch":
        eq = P.CahnHilliard2DPeriodic(dom, 0.002, MU["regsol"], MOB["c1mc"])
        y0 = np.clip(0.5 + 0.05 * rng.standard_normal((2, nx, ny)), 0.05, 0.95).astype(dtype)
        f = lambda kap: (lambda t, u: O.ch_rhs_fd(u, *dom.dx, kap, MU["regsol"], MOB["c1mc"]))
        dt = 2e-7
    else:
        eq = P.AllenCahn2DPeriodic(dom, 0.002, MU["cubic"], MOB["one"])
        y0 = (0.1 * rng.standard_normal((2, nx, ny))).astype(dtype)
        f = lambda kap: (lambda t, u: O.ac_rhs_fd(u, *dom.dx, kap, MU["cubic"], MOB["one"]))
        dt = 5e-5
    kappas = [0.002, 0.0026]  # per-environment control values ride along
    # RK4: 9 substeps = 9 rounds (CH) / 4.5 (AC: two substeps per exchange, the last round half full); Euler: 11 = 2.75 / 1.4 rounds
    for integ, step, n, tag in ((L.INT_RK4, O.rk4_step, 9, "rk4_coop"), (L.INT_EULER, O.euler_step, 11, "euler_coop")):
        got, kern = _advance(eq, y0, integ, dt, n, 2, kappas=kappas)
        assert kern.startswith(tag) and "workgroups" in kern, kern
        tiled, kern_t = _advance(eq, y0, integ, dt, n, -1, kappas=kappas)
        assert "coop" not in kern_t, kern_t
        for b in range(2):
            ref = y0[b].astype(np.float64)
            for i in range(n):
                ref = step(f(kappas[b]), i * dt, ref, dt)
            _check(got[b], ref, y0[b].astype(np.float64), dtype, kern)
        if dtype is np.float64:
            assert rel_l2(got - y0, tiled - y0) < 1e-11, (kern, kern_t)
        else:
            assert np.max(np.abs(got - tiled)) < 5e-7, (kern, kern_t, float(np.max(np.abs(got - tiled))))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,shape", [("ch", (100, 100)), ("ac", (72, 120))])
@pytest.mark.parametrize("integ", ["rk4", "euler"])
def test_smoothed_boundary_fixed_step_with_time_dependent_contact_angle(kind, shape, dtype, integ):
    """theta(t), flux(t) (a quadratic / linear in t: notebooks/smooth_boundary.ipynb:262) evaluated by the kernel at its own
    stage times t, t + dt / 2, t + dt of every substep of a round"""
    psi = sbm_psi(*shape)
    dom = sbm_domain(P, psi)
    rng = np.random.default_rng(5)
    y0 = np.clip(0.5 + 0.1 * rng.standard_normal((1,) + shape), 0.1, 0.9).astype(dtype)
    if kind == "ac":
        eq = P.AllenCahn2DSmoothedBoundary(dom, 1.5, SBM_F, MU["regsol"], MOB["c1mc"], SBM_THETA)
        f = lambda t, u: O.ac_sbm_rhs(u, psi, 1.0, 1.0, 1.5, SBM_F, MU["regsol"], MOB["c1mc"], SBM_THETA(t), eq.left_half)
        dt = 2e-2
    else:
        eq = P.CahnHilliard2DSmoothedBoundary(dom, 1.5, SBM_F, MU["regsol"], MOB["c1mc"], SBM_THETA, SBM_FLUX)
        f = lambda t, u: O.ch_sbm_rhs(u, psi, 1.0, 1.0, 1.5, SBM_F, MU["regsol"], MOB["c1mc"], SBM_THETA(t), SBM_FLUX(t), eq.left_half)
        dt = 2e-3
    t0, n = 0.03, 9
    code, step = (L.INT_RK4, O.rk4_step) if integ == "rk4" else (L.INT_EULER, O.euler_step)
    got, kern = _advance(eq, y0, code, dt, n, 2, t0=t0)
    assert kern.startswith(integ + "_coop") and "SBM" in kern, kern
    ref = y0[0].astype(np.float64)
    for i in range(n):
        ref = step(f, t0 + i * dt, ref, dt)
    if dtype is np.float64:
        assert rel_l2(got[0] - y0[0], ref - y0[0]) < 1e-9
    else:
        assert np.max(np.abs(got[0] - ref)) < 5e-6 and rel_l2(got[0].astype(np.float64) - y0[0], ref - y0[0]) < 2e-3


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_advection_diffusion_fixed_step(dtype):
    nx, ny = 96, 128
    dom = P.Domain((nx, ny), ((0.0, 0.02 * nx), (0.0, 0.02 * ny)), "dimensionless")

    def velocity(t, x, y):
        g = np.exp(-((x - 0.9) ** 2 + (y - 1.2) ** 2) / (2 * 0.05))
        return -0.1 * (x - 0.9) / 0.05 * g, -0.1 * (y - 1.2) / 0.05 * g

    eq = P.AdvectionDiffusion2D(dom, velocity, 0.1, time_dependent=False)
    rng = np.random.default_rng(2)
    y0 = (0.5 + 0.01 * rng.standard_normal((1, nx, ny))).astype(dtype)
    for code, n, tag in ((L.INT_RK4, 10, "rk4_coop"), (L.INT_EULER, 17, "euler_coop")):
        got, kern = _advance(eq, y0, code, 2e-4, n, 2)
        assert kern.startswith(tag) and ",AD," in kern, kern
        want, kern_t = _advance(eq, y0, code, 2e-4, n, -1)
        assert "coop" not in kern_t
        if dtype is np.float64:
            assert rel_l2(got - y0, want - y0) < 1e-11
        else:
            assert np.max(np.abs(got - want)) < 5e-7
        assert abs(float(got.astype(np.float64).mean() - y0.astype(np.float64).mean())) < (1e-12 if dtype is np.float64 else 1e-6)


@pytest.mark.parametrize("dtype,shape", [(np.float32, (96, 96)), (np.float64, (64, 64))], ids=["f32-96", "f64-64"])
def test_sixteen_environments_in_one_launch(dtype, shape):
    """the automatic choice for a batch of 16: 4 x 4 workgroups per environment, two environments per XCD, all in ONE launch
    (block -> (environment, tile) map over rows of XCD slots); per-environment kappa; first, middle and last environment
    against the oracle"""
    nx, ny = shape
    dom = std_domain(P, nx, ny)
    rng = np.random.default_rng(16)
    eq = P.CahnHilliard2DPeriodic(dom, 0.002, MU["regsol"], MOB["c1mc"])
    y0 = np.clip(0.5 + 0.05 * rng.standard_normal((16, nx, ny)), 0.05, 0.95).astype(dtype)
    kappas = [0.002 + 1e-5 * b for b in range(16)]
    got, kern = _advance(eq, y0, L.INT_RK4, 2e-7, 9, 0, kappas=kappas)
    assert kern.startswith("rk4_coop") and "4x4 workgroups" in kern, kern
    for b in (0, 7, 8, 15):
        ref = y0[b].astype(np.float64)
        for i in range(9):
            ref = O.rk4_step(lambda t, u: O.ch_rhs_fd(u, *dom.dx, kappas[b], MU["regsol"], MOB["c1mc"]), 0.0, ref, 2e-7)
        _check(got[b], ref, y0[b].astype(np.float64), dtype, kern)


def test_tiles_narrower_than_the_halo_wait_for_every_workgroup(monkeypatch):
    """tiles of 6 x 6 cells under an 8-cell halo: a ring reaches two tiles away, so the exchange waits for every workgroup
    of the environment instead of the 8 neighbours (PDEOPT_COOP_TILE forces the tile edge)"""
    monkeypatch.setenv("PDEOPT_COOP_TILE", "6")
    nx, ny = 48, 60
    dom = std_domain(P, nx, ny)
    rng = np.random.default_rng(9)
    eq = P.CahnHilliard2DPeriodic(dom, 0.002, MU["regsol"], MOB["c1mc"])
    y0 = np.clip(0.5 + 0.05 * rng.standard_normal((1, nx, ny)), 0.05, 0.95)
    got, kern = _advance(eq, y0, L.INT_RK4, 2e-7, 9, 2)
    assert kern.startswith("rk4_coop") and "8x10 workgroups" in kern, kern
    ref = y0[0]
    for i in range(9):
        ref = O.rk4_step(lambda t, u: O.ch_rhs_fd(u, *dom.dx, 0.002, MU["regsol"], MOB["c1mc"]), 0.0, ref, 2e-7)
    assert rel_l2(got[0] - y0[0], ref - y0[0]) < 1e-9


def test_auto_policy():
    """one mid-sized environment and enough substeps: several CUs per environment; a batch the tiled kernels sweep in one
    launch, a few substeps, a grid of the one-CU kernel's range or a caller-chosen tiled knob: the other paths"""
    dom = std_domain(P, 128, 128)
    eq = P.CahnHilliard2DPeriodic(dom, 0.002, MU["regsol"], MOB["c1mc"])
    rng = np.random.default_rng(0)

    def kernel(batch, n, shape=(128, 128), knob=None):
        d = std_domain(P, *shape)
        e = P.CahnHilliard2DPeriodic(d, 0.002, MU["regsol"], MOB["c1mc"])
        y = np.clip(0.5 + 0.05 * rng.standard_normal((batch,) + shape), 0.05, 0.95).astype(np.float32)
        eng = P.HipEngine()
        if knob:
            knob(eng)
        eng.configure(dtype=y.dtype, batch=batch, **e._engine_problem())
        eng.set_state(y)
        eng.advance(L.INT_RK4, 2e-7, n)
        k = eng.last_kernel
        assert np.all(np.isfinite(eng.get_state()))
        eng.close()
        return k

    assert kernel(1, 100).startswith("rk4_coop"), kernel(1, 100)
    assert kernel(2, 100).startswith("rk4_coop")
    assert not kernel(64, 100).startswith("rk4_coop")
    assert not kernel(1, 4).startswith("rk4_coop")
    assert kernel(1, 100, (64, 64)).startswith("small_persist")
    assert not kernel(1, 100, (256, 256)).startswith("rk4_coop")  # the tiled whole-substep kernel is as fast from ~200^2 on
    assert not kernel(1, 100, knob=lambda e: e.set_fuse_stages(1)).startswith("rk4_coop")


# ------------------------------------------------------------------------------------------------------------------------
# Substep counts at the edges of a round, the policy's own threshold, split calls, several launches, time tables.
#
# Substeps one halo load pays for: `const int S = H / (stages * R)` of the fixed-step loop in stencil_coop_adaptive.hpp with
# H = 8 halo cells, R the stencil radius of one right-hand side (2 for the Cahn-Hilliard forms, 1 for Allen-Cahn and
# advection-diffusion) and 4 stages for RK4, 1 for Euler.
_RADIUS = {"ch": 2, "ch_sbm": 2, "ac": 1, "ac_sbm": 1, "ad": 1}
_INTEG = {"rk4": (L.INT_RK4, O.rk4_step, 4), "euler": (L.INT_EULER, O.euler_step, 1)}


def _round(kind, integ):
    return 8 // (_INTEG[integ][2] * _RADIUS[kind])


def _edge_counts(S):
    """less than a round, one short of it, exactly one (no exchange at all), one more (a round + a partial one), two full
    rounds, two and a partial one"""
    return sorted({n for n in (1, S - 1, S, S + 1, 2 * S, 2 * S + 1) if n > 0})


def _ad_velocity(t, x, y):
    g = np.exp(-((x - 0.9) ** 2 + (y - 1.2) ** 2) / (2 * 0.05))
    return -0.1 * (x - 0.9) / 0.05 * g, -0.1 * (y - 1.2) / 0.05 * g


def _problem(kind, shape, dtype, batch=2):
    """equation object, initial states, per-environment control values, dt, t0 and rhs(b) -> f(t, u) of the fp64 oracle"""
    nx, ny = shape
    rng = np.random.default_rng(nx * 1000 + ny)
    t0 = 0.0
    if kind == "ch":
        dom = std_domain(P, nx, ny)
        eq = P.CahnHilliard2DPeriodic(dom, 0.002, MU["regsol"], MOB["c1mc"])
        y0 = np.clip(0.5 + 0.05 * rng.standard_normal((2, nx, ny)), 0.05, 0.95)
        kappas, dt = [0.002, 0.0026], 2e-7
        rhs = lambda b: (lambda t, u: O.ch_rhs_fd(u, *dom.dx, kappas[b], MU["regsol"], MOB["c1mc"]))
    elif kind == "ac":
        dom = std_domain(P, nx, ny)
        eq = P.AllenCahn2DPeriodic(dom, 0.002, MU["cubic"], MOB["one"])
        y0 = 0.1 * rng.standard_normal((2, nx, ny))
        kappas, dt = [0.002, 0.0026], 5e-5
        rhs = lambda b: (lambda t, u: O.ac_rhs_fd(u, *dom.dx, kappas[b], MU["cubic"], MOB["one"]))
    elif kind == "ad":
        dom = P.Domain((nx, ny), ((0.0, 0.02 * nx), (0.0, 0.02 * ny)), "dimensionless")
        eq = P.AdvectionDiffusion2D(dom, _ad_velocity, 0.1, time_dependent=False)
        y0 = 0.5 + 0.01 * rng.standard_normal((2, nx, ny))
        kappas, dt = [0.1, 0.13], 2e-4  # (the per-environment control value of this equation is its diffusivity)
        vx, vy = eq.face_velocities(0.0)
        rhs = lambda b: (lambda t, u: O.ad_rhs_fd(u, *dom.dx, vx, vy, kappas[b]))
    else:
        psi = sbm_psi(nx, ny)
        dom = sbm_domain(P, psi)
        y0 = np.clip(0.5 + 0.1 * rng.standard_normal((2, nx, ny)), 0.1, 0.9)
        kappas, t0 = [1.5, 1.8], 0.03
        if kind == "ac_sbm":
            eq = P.AllenCahn2DSmoothedBoundary(dom, 1.5, SBM_F, MU["regsol"], MOB["c1mc"], SBM_THETA)
            dt = 2e-2
            rhs = lambda b: (lambda t, u: O.ac_sbm_rhs(u, psi, 1.0, 1.0, kappas[b], SBM_F, MU["regsol"], MOB["c1mc"], SBM_THETA(t), eq.left_half))
        else:
            eq = P.CahnHilliard2DSmoothedBoundary(dom, 1.5, SBM_F, MU["regsol"], MOB["c1mc"], SBM_THETA, SBM_FLUX)
            dt = 2e-3
            rhs = lambda b: (lambda t, u: O.ch_sbm_rhs(u, psi, 1.0, 1.0, kappas[b], SBM_F, MU["regsol"], MOB["c1mc"], SBM_THETA(t), SBM_FLUX(t),
                                                       eq.left_half))
    return eq, y0[:batch].astype(dtype), kappas[:batch], dt, t0, rhs


def _oracle(rhs_b, step, y0_b, dt, n, t0, dtype=np.float64):
    """n substeps of the numpy oracle from t0.  dtype float32: the same steps with the state, dt and every stage's slope
    rounded to fp32 (times stay double, as in the kernel) -- what fp32 arithmetic itself leaves of the fp64 result"""
    if dtype is np.float64:
        f, ref, h = rhs_b, y0_b.astype(np.float64), dt
    else:
        f = lambda t, u: np.asarray(rhs_b(t, u.astype(np.float32)), dtype=np.float32)
        ref, h = y0_b.astype(np.float32), np.float32(dt)
    for i in range(n):
        ref = np.asarray(step(f, np.float64(t0 + i * dt), ref, h), dtype=dtype)
    return ref


def _check_sbm(got, ref, y0, dtype, kern):
    """the gates of test_smoothed_boundary_fixed_step_with_time_dependent_contact_angle"""
    y0 = y0.astype(np.float64)
    if dtype is np.float64:
        assert rel_l2(got - y0, ref - y0) < 1e-9, (kern, rel_l2(got - y0, ref - y0))
    else:
        assert np.max(np.abs(got - ref)) < 5e-6 and rel_l2(got.astype(np.float64) - y0, ref - y0) < 2e-3, (
            kern, float(np.max(np.abs(got - ref))), rel_l2(got.astype(np.float64) - y0, ref - y0))


def _check_case(kind, integ, dtype, eq, y0, kappas, dt, t0, rhs, n, opt):
    """advance n substeps on the multi-workgroup kernel; gates: the oracle, and (periodic forms) the tiled path"""
    code, step, _ = _INTEG[integ]
    got, kern = _advance(eq, y0, code, dt, n, opt, t0=t0, kappas=kappas)
    # (a change of policy must not turn the case into a test of another kernel)
    assert kern.startswith(integ + "_coop") and "workgroups" in kern, (kern, n)
    for b in range(y0.shape[0]):
        ref = _oracle(rhs(b), step, y0[b], dt, n, t0)
        if kind.endswith("_sbm"):
            _check_sbm(got[b], ref, y0[b], dtype, (kern, n, b))
        else:
            _check(got[b], ref, y0[b].astype(np.float64), dtype, (kern, n, b))
    if not kind.endswith("_sbm"):
        tiled, kern_t = _advance(eq, y0, code, dt, n, -1, t0=t0, kappas=kappas)
        assert "coop" not in kern_t, kern_t
        if dtype is np.float64:
            assert rel_l2(got - y0, tiled - y0) < 1e-11, (kern, kern_t, n, rel_l2(got - y0, tiled - y0))
        else:
            assert np.max(np.abs(got - tiled)) < 5e-7, (kern, kern_t, n, float(np.max(np.abs(got - tiled))))
    return kern


# tiles at least 8 cells wide (the exchange waits for the 8 neighbours only) and a ragged split
_SWEEP_SHAPES = {"ch": [(128, 128), (100, 100)], "ac": [(128, 128), (72, 120)], "ad": [(128, 128), (100, 100)],
                 "ch_sbm": [(128, 128), (100, 100)], "ac_sbm": [(128, 128), (72, 120)]}
_SWEEP = [(kind, integ, shape, n) for kind in _SWEEP_SHAPES for integ in ("rk4", "euler") for shape in _SWEEP_SHAPES[kind]
          for n in _edge_counts(_round(kind, integ))]


def test_fp32_arithmetic_itself_stays_inside_the_fp32_gates_at_one_substep():
    """No device needed.  The fp32 gates (state rounding: inc_tol_f32; the smoothed-boundary test's 5e-6 / 2e-3) were written
    for 9 - 17 substeps; at n = 1 the increment is smallest against the state's rounding.  The oracle stepped in fp32 (state,
    dt and every stage's slope rounded to fp32) must itself pass them against the fp64 oracle, with a factor 2 to spare,
    for every case of the sweep below -- otherwise a case's dt would have to change (none had to)."""
    for kind, shapes in _SWEEP_SHAPES.items():
        for shape in shapes:
            for integ in ("rk4", "euler"):
                eq, y0, kappas, dt, t0, rhs = _problem(kind, shape, np.float32)
                step = _INTEG[integ][1]
                for b in range(2):
                    ref = _oracle(rhs(b), step, y0[b], dt, 1, t0)
                    f32 = _oracle(rhs(b), step, y0[b], dt, 1, t0, np.float32)
                    y0b = y0[b].astype(np.float64)
                    err, inc = float(np.max(np.abs(f32 - ref))), rel_l2(f32.astype(np.float64) - y0b, ref - y0b)
                    if kind.endswith("_sbm"):
                        assert err < 2.5e-6 and inc < 1e-3, (kind, shape, integ, b, err, inc)
                    else:
                        assert err < 1e-6 and inc < 0.5 * inc_tol_f32(ref, y0b), (kind, shape, integ, b, err, inc, inc_tol_f32(ref, y0b))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,integ,shape,n", _SWEEP, ids=lambda v: str(v).replace(" ", ""))
def test_substep_counts_around_a_round(kind, integ, shape, n, dtype):
    """n = 1, S - 1, S, S + 1, 2 S, 2 S + 1 for the S substeps one halo load pays for: solves that end before the first
    exchange (n <= S: the write-back into the state waits for the partners' initial loads, nothing else orders it), that end
    exactly on a round, and partial last rounds (m substeps, m * stages time-term slots, halo budget e = 8 - m * stages * R
    left over).  Two environments with their own kappa (diffusivity for advection-diffusion).  theta(t), flux(t) of the
    smoothed-boundary forms from t0 = 0.03.  What a passing run does NOT show is the absence of the n <= S race itself:
    that depends on scheduling; it is closed by the ordering argument in the kernel and DESIGN 4.7."""
    _check_case(kind, integ, dtype, *_problem(kind, shape, dtype), n, 2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("integ,n", [("rk4", 1), ("euler", 4)])
def test_short_solves_on_tiles_narrower_than_the_halo(monkeypatch, integ, n, dtype):
    """6 x 6 tiles on 48 x 60 (every workgroup waits for every other): one RK4 substep / four Euler substeps = one round"""
    monkeypatch.setenv("PDEOPT_COOP_TILE", "6")
    kern = _check_case("ch", integ, dtype, *_problem("ch", (48, 60), dtype), n, 2)
    assert "8x10 workgroups" in kern, kern


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind,integ", [("ac", "euler"), ("ad", "euler"), ("ch", "euler"), ("ac", "rk4"), ("ch", "rk4")])
def test_eight_substeps_at_the_automatic_policys_threshold(kind, integ, dtype):
    """no knob set, one 128^2 environment, n = 8 = the fewest substeps the policy hands to this kernel: Euler Allen-Cahn /
    advection-diffusion one round and no exchange at all, Euler Cahn-Hilliard two full rounds, RK4 Allen-Cahn four, RK4
    Cahn-Hilliard eight"""
    _check_case(kind, integ, dtype, *_problem(kind, (128, 128), dtype, batch=1), 8, 0)


def _advance_in_calls(eq, y0, code, dt, calls, kappas, tag):
    eng = P.HipEngine()
    eng.set_small_persist(2)
    eng.configure(dtype=y0.dtype, batch=y0.shape[0], **eq._engine_problem())
    eq._engine_upload(eng, 0.0, dt * sum(calls))
    eng.set_env_params(0, kappa=kappas)
    eng.set_state(y0)
    done = 0
    for n in calls:
        eng.advance(code, dt, n, done * dt)
        assert eng.last_kernel.startswith(tag), eng.last_kernel
        done += n
    out = eng.get_state()
    eng.close()
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(128, 128), (100, 100)], ids=str)
@pytest.mark.parametrize("integ", ["rk4", "euler"])
@pytest.mark.parametrize("kind", ["ch", "ac", "ad"])
def test_split_calls_equal_one_call_bitwise(kind, integ, shape, dtype):
    """A cell of a tile is only ever written by its owner, and the halo cells are recomputed by the same code from the same
    inputs, so for the autonomous equations the state after n = 2 S substeps does not depend on where rounds or calls end:
    one call, n calls of one substep, two calls of one round each -- the same bits.  A stale halo cell would show here
    without any tolerance."""
    eq, y0, kappas, dt, _, _ = _problem(kind, shape, dtype)
    code, S = _INTEG[integ][0], _round(kind, integ)
    n = 2 * S
    whole = _advance_in_calls(eq, y0, code, dt, [n], kappas, integ + "_coop")
    np.testing.assert_array_equal(_advance_in_calls(eq, y0, code, dt, [1] * n, kappas, integ + "_coop"), whole)
    np.testing.assert_array_equal(_advance_in_calls(eq, y0, code, dt, [S] * 2, kappas, integ + "_coop"), whole)


def test_more_environments_than_one_launch_holds():
    """70 environments of 128^2 fp32 under the forced knob.  One launch holds (compute units per XCD // workgroups of an
    environment per XCD) x (8 // XCDs per environment) environments (coop_launch_shape), every workgroup being resident
    at once.  The fewest workgroups whose arrays fit the LDS for this problem are 2 x 2 tiles of 64^2 (5 arrays of 80 x 81
    floats = 130 KB; 3 x 1 and 2 x 1 need more than 160 KB): 32 // 4 x 8 = 64 environments on the 8 x 32 compute units of
    an MI355X -- so whatever split the planner picks for 70, there are at least two launches, with their own offsets into
    the states, the control values and the published round numbers, and one shared abort word.  The split is read from the
    kernel's name, the launch count from the engine's counter; the environments either side of every launch boundary, the
    first and the last are held to the oracle."""
    batch, n, dt = 70, 3, 2e-7
    dom = std_domain(P, 128, 128)
    rng = np.random.default_rng(70)
    eq = P.CahnHilliard2DPeriodic(dom, 0.002, MU["regsol"], MOB["c1mc"])
    y0 = np.clip(0.5 + 0.05 * rng.standard_normal((batch, 128, 128)), 0.05, 0.95).astype(np.float32)
    kappas = [0.002 + 1e-5 * b for b in range(batch)]
    eng = P.HipEngine()
    eng.set_small_persist(2)
    eng.configure(dtype=y0.dtype, batch=batch, **eq._engine_problem())
    eng.set_env_params(0, kappa=kappas)
    eng.set_state(y0)
    before = eng.stage_launches()
    eng.advance(L.INT_RK4, dt, n, 0.0)
    launches, kern, got = eng.stage_launches() - before, eng.last_kernel, eng.get_state()
    eng.close()
    assert kern.startswith("rk4_coop"), kern
    px, py = (int(v) for v in kern.rsplit(",", 1)[1].split(" ")[0].split("x"))
    nwg, xs = px * py, 1
    while xs < 8 and -(-nwg // xs) > 32:
        xs *= 2
    per_launch = (32 // -(-nwg // xs)) * (8 // xs)
    assert per_launch < batch and launches == -(-batch // per_launch) >= 2, (kern, per_launch, launches)
    edges = {0, batch - 1}
    for e0 in range(per_launch, batch, per_launch):
        edges |= {e0 - 1, e0}
    for b in sorted(edges):
        ref = _oracle(lambda t, u: O.ch_rhs_fd(u, *dom.dx, kappas[b], MU["regsol"], MOB["c1mc"]), O.rk4_step, y0[b], dt, n, 0.0)
        _check(got[b], ref, y0[b].astype(np.float64), np.float32, (kern, b))


def _table_engine(eq, y0, opt, t0):
    """the smoothed-boundary fields as _engine_upload sends them, but NO callback: constant terms (theta, flux frozen at t0)"""
    eng = P.HipEngine()
    eng.set_small_persist(opt)
    eng.configure(dtype=y0.dtype, batch=1, **eq._engine_problem())
    eng.set_aux(L.AUX_SBM_PSI, eq.psi)
    eng.set_aux(L.AUX_SBM_NORM_GRAD, eq.norm_grad_psi)
    eng.set_aux(L.AUX_SBM_MASK, eq.left_half)
    eng.set_time_terms(None, constant=eq._time_terms(t0))
    eng.set_state(y0)
    return eng


def _set_time_table(eng, ts, terms):
    ts = np.ascontiguousarray(ts, dtype=np.float64)
    terms = np.ascontiguousarray(terms, dtype=np.float64).reshape(-1, 3)
    eng._check(eng._lib.pdeopt_set_time_table(eng._h, len(ts), ts.ctypes.data_as(L.C.c_void_p), terms.ctypes.data_as(L.C.c_void_p)))


def _stage_times(integ, t0, dt, n):
    ts = float(t0) + np.arange(n, dtype=np.float64) * float(dt)  # t0 + (double) step * dt, as HipEngine._upload_time_table
    return np.unique(np.concatenate([ts, ts + float(dt) / 2, ts + float(dt)])) if integ == "rk4" else ts


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("opt", [0, 2], ids=["auto", "forced"])
@pytest.mark.parametrize("integ", ["rk4", "euler"])
@pytest.mark.parametrize("kind,shape", [("ch_sbm", (100, 100)), ("ac_sbm", (72, 120))])
def test_time_table_without_a_callback(kind, shape, integ, opt, dtype):
    """theta(t), flux(t) sampled at the call's stage times (pdeopt_set_time_table) and no callback registered -- the
    documented way to run without one.  The multi-workgroup kernel knows constants and polynomials only, so the library
    must not route this call to it (it did: theta and the flux stayed frozen at the constants and the call returned OK);
    the tiled smoothed-boundary kernel serves the table, whatever the knob.  A table that lacks one stage time of the call
    is still reported.  Before the routing was fixed these 16 cases ran on rk4_coop / euler_coop and reproduced the solve
    with theta, flux frozen at t0 to rounding (1e-15 in fp64): rel_l2 of the increment against the oracle 8.9e-4 (RK4) /
    7.9e-4 (Euler) for Cahn-Hilliard, 6.1e-2 / 5.6e-2 for Allen-Cahn, in both precisions and under both knobs."""
    eq, y0, _, dt, t0, rhs = _problem(kind, shape, dtype, batch=1)
    code, step, _ = _INTEG[integ]
    n = 9
    ts = _stage_times(integ, t0, dt, n)
    terms = [eq._time_terms(float(t)) for t in ts]
    eng = _table_engine(eq, y0, opt, t0)
    _set_time_table(eng, ts, terms)
    eng.advance(code, dt, n, t0)
    got, kern = eng.get_state(), eng.last_kernel
    ref = _oracle(rhs(0), step, y0[0], dt, n, t0)
    frozen = _oracle(lambda t, u: rhs(0)(t0, u), step, y0[0], dt, n, t0)  # what the ignored table gave
    y0d = y0[0].astype(np.float64)
    print(f"{kind} {integ} {np.dtype(dtype).name} opt {opt}: {kern}, rel_l2 of the increment against the oracle "
          f"{rel_l2(got[0].astype(np.float64) - y0d, ref - y0d):.3e}, against theta, flux frozen at t0 {rel_l2(got[0].astype(np.float64) - y0d, frozen - y0d):.3e}")
    assert kern.startswith("sbm_tiled<"), kern
    _check_sbm(got[0], ref, y0[0], dtype, kern)
    # (the fp32 gate on the increment, 2e-3, is wider than what freezing theta and the flux changes in the Cahn-Hilliard form,
    # 8.9e-4: nearer to the oracle than to the frozen solve, in every precision)
    inc_g = got[0].astype(np.float64) - y0d
    assert np.linalg.norm(inc_g - (ref - y0d)) < 0.5 * np.linalg.norm(frozen - ref), kern
    # a table without one of the call's stage times (here the middle one): refused, not served with the constants
    eng.set_state(y0)
    _set_time_table(eng, np.delete(ts, len(ts) // 2), np.delete(np.asarray(terms, dtype=np.float64).reshape(-1, 3), len(ts) // 2, axis=0))
    with pytest.raises(ValueError, match="not in the table"):
        eng.advance(code, dt, n, t0)
    eng.close()
