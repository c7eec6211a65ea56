"""The 2-D sensitivity kernels (csrc/sens.hip: sens_tangent_rhs_kernel, sens_gn_partial_kernel) off the square,
whole-tile, whole-block grids of tests/test_gpu_sens.py: ragged grids, grids smaller than one 16 x 32 tile (the
division in wrap_idx), hx != hy, every closure class of the in-kernel family with the first and the last coefficient
of each closure (Legendre up to index 15), tangent trajectories on those grids through Euler, rocFFT IMEX and the
hand-written FFT passes with an anisotropic spacing and an odd batch, and the Gauss-Newton sums on grids whose last
block of 2048 cells is partial.  Everything is held to the fp64 numpy reference tests/sens_ref.py or to fp64 numpy
sums over the fetched fields."""
import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from pde_opt_amd import fit
from pde_opt_amd.numerics.closures import EXP_WRAP, LEGENDRE, LOGIT_PRIOR, ClosureDesc
import sens_ref as S
from test_gpu_sens import KAPPA, _rel, _sens_engine
from test_gpu_sens3d import CLOSURES as CLOSURES3D

pytestmark = pytest.mark.gpu

MU, MOB = S.MU_ROLE, S.MOB_ROLE


def _legendre16_mu():
    """16 Legendre coefficients: (0.1, -3, 0.4, 0.2) plus seeded values of at most 0.05, so |a_k| <= 0.1 for k >= 4"""
    a = 0.05 * np.random.default_rng(16).uniform(-1.0, 1.0, 16)
    a[:4] += (0.1, -3.0, 0.4, 0.2)
    return ClosureDesc(LEGENDRE, LOGIT_PRIOR, tuple(float(v) for v in a))


# (mu, D, parameters): the first and the highest coefficient of each closure are among the parameters
CLOSURES = {
    "legendre16": (_legendre16_mu(), ClosureDesc(LEGENDRE, EXP_WRAP, (-0.3, 0.2, 0.1)),
                   [(MU, 0), (MU, 7), (MU, 15), (MOB, 0), (MOB, 2)]),
    "poly": CLOSURES3D["poly"][:2] + ([(MU, 2), (MOB, 2), (MU, 0), (MU, 3), (MOB, 0)],),
    "mix_entropy_exp_poly": CLOSURES3D["mix_entropy_exp_poly"][:2] + ([(MU, 1), (MOB, 1), (MOB, 0), (MU, 0), (MU, 2)],),
}

# (shape, hx, hy); the output tile of sens_tangent_rhs_kernel is 16 x 32
SHAPES = [
    ((40, 72), 1 / 64, 1 / 128),    # ragged on both axes
    ((17, 33), 1 / 64, 1 / 128),    # one cell past a tile on each axis
    ((16, 32), 1 / 64, 1 / 128),    # exactly one tile
    ((6, 10), 1 / 64, 1 / 128),     # smaller than a tile: the ring wraps more than once
    ((3, 70), 1 / 64, 1 / 128),
    ((64, 128), 1 / 128, 1 / 64),   # whole tiles, the anisotropy the other way round
]


def _domain(shape, h):
    return P.Domain(shape, tuple((0.0, n * hh) for n, hh in zip(shape, h)), "dimensionless")


def _state(shape, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return np.clip(0.5 + 0.1 * rng.standard_normal(shape), 0.1, 0.9).astype(dtype)


def _smooth_state(shape, seed):
    """a few Fourier modes around 0.5 and 1 % of noise, so every wavenumber of the grid is present"""
    rng = np.random.default_rng(seed)
    x, y = (np.arange(n) / n for n in shape)
    u = 0.5 + 0.01 * rng.standard_normal(shape)
    for _ in range(6):
        kx, ky = rng.integers(1, 4, 2)
        u += 0.03 * rng.standard_normal() * np.cos(2 * np.pi * (kx * x[:, None] + ky * y[None, :]) + rng.uniform(0, 6))
    return u


# ---- 1. the tangent-linear right-hand side over shapes x closures x dtypes ----------------------------------------


@pytest.mark.parametrize("closures", sorted(CLOSURES))
@pytest.mark.parametrize("shape,hx,hy", SHAPES, ids=["%dx%d" % s[0] for s in SHAPES])
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-11), (np.float32, 1e-4)], ids=["fp64", "fp32"])
def test_tangent_rhs_shapes_and_closures(closures, shape, hx, hy, dtype, tol):
    mu, mob, params = CLOSURES[closures]
    dom = _domain(shape, (hx, hy))
    assert tuple(dom.dx) == (hx, hy)
    eq = P.CahnHilliard2DPeriodic(dom, KAPPA, mu, mob)
    B, Pn = 2, len(params)
    base = np.stack([_state(shape, 1 + b, dtype) for b in range(B)])
    rng = np.random.default_rng(7)
    random_tang = (0.05 * rng.standard_normal((Pn * B,) + shape)).astype(dtype)
    # the second pass has all tangents zero: the slope is df/dp_j alone, so the Jacobian term cannot hide a wrong
    # basis function
    errs = []
    for name, tang in (("random", random_tang), ("zero", np.zeros_like(random_tang))):
        eng = _sens_engine(eq, None, base, tang, params)
        k = eng.sens_rhs()
        for b in range(B):
            u = base[b].astype(np.float64)
            errs.append(((name, b, "base"), _rel(k[b], S.ch_rhs(u, hx, hy, KAPPA, mu, mob)), max(tol, 1e-12)))
            for j, (role, kc) in enumerate(params):
                du = tang[j * B + b].astype(np.float64)
                want = S.tangent_rhs(u, du, hx, hy, KAPPA, mu, mob, role, kc)
                got = k[B + j * B + b]
                if not np.any(want):
                    # mu's constant coefficient with zero tangents: the gradient of a constant, 0 in every arithmetic
                    assert (role, kc, name) == (MU, 0, "zero")
                    errs.append(((name, b, role, kc), float(np.max(np.abs(got))), 0.0))
                else:
                    errs.append(((name, b, role, kc), _rel(got, want), tol))
    print("\n[tangent_rhs %s %dx%d %s] worst rel err %.3e (gate %.0e)" % (
        closures, shape[0], shape[1], np.dtype(dtype).name, max(e for _, e, _ in errs), tol))
    for what, err, gate in errs:
        assert err <= gate, (what, err)


# ---- 2. trajectories off the happy path (fp64, 50 substeps) --------------------------------------------------------


def _moving(closures):
    """the closure set's parameters without mu's constant coefficient: only grad mu enters the right-hand side, so a
    tangent that starts from zero stays zero and has no relative error"""
    return [p for p in CLOSURES[closures][2] if p != (MU, 0)]


def _run_trajectories(shape, h, closures, params, integrator, dt, B):
    mu, mob, _ = CLOSURES[closures]
    dom = _domain(shape, h)
    eq = P.CahnHilliard2DPeriodic(dom, KAPPA, mu, mob)
    imex = integrator == "imex"
    solver = P.SemiImplicitFourierSpectral(A=0.5, fourier_symbol=eq.fourier_symbol) if imex else None
    u0 = np.stack([_smooth_state(shape, 3 + b) for b in range(B)])
    Pn, n = len(params), 50
    eng = _sens_engine(eq, solver, u0, np.zeros((Pn * B,) + shape), params)
    eng.sens_advance(L.INT_IMEX if imex else L.INT_EULER, dt, n)
    got = eng.get_state()
    worst_u = worst_du = 0.0
    for b in range(B):
        u_ref, dus = S.trajectory(u0[b], params, dt, n, h[0], h[1], KAPPA, mu, mob, integrator, 0.5, eq.fourier_symbol)
        assert np.linalg.norm(u_ref - u0[b]) > 0 and all(np.linalg.norm(d) > 0 for d in dus)
        worst_u = max(worst_u, _rel(got[b], u_ref))
        worst_du = max([worst_du] + [_rel(got[B + j * B + b], dus[j]) for j in range(Pn)])
    print("\n[trajectory %s %dx%d %s B=%d P=%d] base %.3e tangents %.3e" % (
        closures, shape[0], shape[1], integrator, B, Pn, worst_u, worst_du))
    assert worst_u <= 1e-12
    assert worst_du <= 1e-10
    return eng


def test_trajectory_ragged_poly_euler():
    # explicit Euler: dt is well under 2 / (kappa D (4 / hx^2 + 4 / hy^2)^2) = 1.0e-7
    eng = _run_trajectories((40, 72), (1 / 64, 1 / 128), "poly", _moving("poly"), "euler", 2e-8, 1)
    assert "sens_tangent_rhs" in eng.last_kernel and "euler" in eng.last_kernel


def test_trajectory_ragged_mix_entropy_imex_rocfft():
    eng = _run_trajectories((40, 72), (1 / 64, 1 / 128), "mix_entropy_exp_poly", _moving("mix_entropy_exp_poly"),
                            "imex", 2e-6, 1)
    assert "imex_rocfft" in eng.last_kernel


@pytest.mark.parametrize("B,params", [(3, [(MU, 7), (MU, 15), (MOB, 2)]), (1, [(MU, 15), (MOB, 0)])],
                         ids=["batch12", "batch3"])
@pytest.mark.parametrize("shape,h", [((64, 128), (1 / 128, 1 / 64)), ((128, 64), (1 / 64, 1 / 128))],
                         ids=["64x128", "128x64"])
def test_trajectory_fused_imex_anisotropic(shape, h, B, params):
    # the fused passes transform two real environments as one complex field: (1 + 3) 3 = 12 environments are six full
    # pairs, (1 + 2) 1 = 3 leave the last complex field with one environment
    eng = _run_trajectories(shape, h, "legendre16", params, "imex", 2e-6, B)
    assert "imex_fused_lds_fft" in eng.last_kernel


# ---- 3. the Gauss-Newton sums with partial blocks -------------------------------------------------------------------
# sens_gn_partial_kernel gives 2048 cells to a block of 256 threads: 40 x 72 = 2880 cells are two blocks with a tail of
# 832, 6 x 10 = 60 cells one block with fewer cells than threads, 96 x 80 leaves a tail of 1536 and 10 x 12 x 9 = 1080.
# The polynomial closures are defined for every real c, so state, tangents and frames are all plain random fields of
# order 1.

GN_GRIDS = [(40, 72), (6, 10), (96, 80), (10, 12, 9)]
GN_PARAMS = {1: [(MU, 2)], 5: [(MU, 0), (MU, 1), (MU, 3), (MOB, 0), (MOB, 2)]}
THETA = 0.37


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("interp", [0, 1], ids=["state", "lerp"])
@pytest.mark.parametrize("Pn", [1, 5])
@pytest.mark.parametrize("shape", GN_GRIDS, ids=["x".join(map(str, s)) for s in GN_GRIDS])
def test_gauss_newton_sums_partial_blocks(shape, Pn, interp, dtype):
    mu, mob, _ = CLOSURES["poly"]
    params = GN_PARAMS[Pn]
    h = (1 / 64, 1 / 128, 1 / 64)[:len(shape)]
    eq_type = P.CahnHilliard2DPeriodic if len(shape) == 2 else P.CahnHilliard3DPeriodic
    eq = eq_type(_domain(shape, h), KAPPA, mu, mob)
    B = 2
    rng = np.random.default_rng(100 + Pn)
    snap = rng.standard_normal(((1 + Pn) * B,) + shape).astype(dtype)
    frames = rng.standard_normal((2, B) + shape).astype(dtype)
    eng = _sens_engine(eq, None, snap[:B], snap[B:], params)
    eng.sens_set_data(frames)
    if interp:
        eng.snapshot()
        eng.sens_advance(L.INT_EULER, 5e-9, 4)  # a few stable explicit substeps, so that y != snap
    y = eng.get_state()
    got = eng.sens_accumulate(1, THETA if interp else 1.0, bool(interp))
    assert got.shape == (B, 1 + Pn + Pn * (Pn + 1) // 2)
    assert eng.sens_accumulate(1, THETA if interp else 1.0, bool(interp)).tobytes() == got.tobytes()

    s64, y64 = snap.astype(np.float64), y.astype(np.float64)
    assert np.all(np.isfinite(y64))
    if interp:
        assert all(np.linalg.norm(y64[e] - s64[e]) > 1e-3 * np.linalg.norm(s64[e]) for e in range(len(y64)))
    pred = s64 + THETA * (y64 - s64) if interp else y64
    mag = np.abs(s64) + np.abs(y64)
    # rows of the products: 0 = the residual of the B trajectories, 1 + j = tangent j; mags: |snap| + |y| of the
    # predicted field each row is made of
    rows = [frames[1].astype(np.float64) - pred[:B]] + [pred[B + j * B: B + (j + 1) * B] for j in range(Pn)]
    mags = [mag[:B]] + [mag[B + j * B: B + (j + 1) * B] for j in range(Pn)]

    def gate(i, j):
        # fp64, and fp32 without the lerp (the kernel multiplies exact fp32 values in double): only the order of the
        # summation differs.  fp32 with the lerp: snap + theta (y - snap) is formed in fp32, at most 4 roundings of
        # 2^-24 relative to |snap| + |y| per predicted value (derived, not measured).
        g = 1e-10 * np.sqrt(np.sum(rows[i] ** 2) * np.sum(rows[j] ** 2))
        if interp and dtype == np.float32:
            g += 4 * 2.0 ** -24 * np.sqrt(np.sum(mags[i] ** 2) * np.sum(rows[j] ** 2))
        return g

    ssr, rdp, G = fit.unpack_sums(got, Pn)
    checks = [(("ssr",), ssr, np.sum(rows[0] ** 2), gate(0, 0))]
    for i in range(Pn):
        checks.append((("rdp", i), rdp[i], np.sum(rows[0] * rows[1 + i]), gate(0, 1 + i)))
        for j in range(i, Pn):
            checks.append((("G", i, j), G[i, j], np.sum(rows[1 + i] * rows[1 + j]), gate(1 + i, 1 + j)))
            assert G[j, i] == G[i, j]
    print("\n[gn %s P=%d interp=%d %s] worst |got - want| / gate %.3e" % (
        "x".join(map(str, shape)), Pn, interp, np.dtype(dtype).name, max(abs(g - w) / t for _, g, w, t in checks)))
    for what, g, w, t in checks:
        assert abs(g - w) <= t, (what, g, w, t)
