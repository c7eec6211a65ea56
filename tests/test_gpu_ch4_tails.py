"""The ragged trips of the single-pass Cahn-Hilliard RK4 kernel (csrc/stencil_fused_ch4.hpp): what the helpers' full trips
of whole vectors leave of a stage's ring is evaluated cell by cell (flux_divergence_cell), and the chemical-potential
passes take their first trip from an offset formed once per row length.  The arithmetic per cell is the vector
path's, so the result stays BITWISE that of the stage-pair kernels.  Shapes: the smallest at which a tail can go
wrong -- one tile (every halo cell a wrap of the tile itself), 2 x 2 tiles with a non-zero environment offset, an odd
tile count along the rows, the 64 x 64 geometry (other ragged counts), and the halo-8 instantiation on virtual ranks.
Three substeps: every stage's tail and the in-place w3 overwrite run more than once."""
import numpy as np
import pytest

import pde_opt_amd as P
from oracle import c_oracle as CO
from pde_opt_amd import _lib as L
from pde_opt_amd.decomp import CartesianGrid, DecomposedSolver, HipTileBackend, LocalGroupComm, advance_group
from util import MOB, MU, inc_tol_f32, rel_l2, std_domain, white_noise_state

pytestmark = pytest.mark.gpu

NSUB = 3
# (mu, mobility, dt, the C oracle's closures): logit + linear mu with c (1 - c) takes the folded mu line, the cubic
# the general one (eval_mu - kappa lap)
CLOSURES = {
    "regsol": ("regsol", "c1mc", 2e-7, lambda: (CO.closure(0, 1, (3.0, -6.0)), CO.closure(0, 0, (0.0, 1.0, -1.0)))),
    "cubic": ("cubic", "one_plus_sq", 2e-8, lambda: (CO.closure(0, 0, (0.0, -1.0, 0.0, 1.0)), CO.closure(0, 0, (1.0, 0.0, 1.0)))),
}


def _solve(eq, u, dt, kappas, fuse, rows):
    eng = P.HipEngine()
    eng.set_fuse_stages(fuse)
    eng.set_small_persist(-1)
    eng.set_graph(-1)
    if rows:
        eng.set_tile_rows(rows)
    eng.configure(dtype=np.float32, batch=u.shape[0], **eq._engine_problem())
    eng.set_env_params(0, kappa=kappas)
    eng.set_state(u)
    eng.advance(L.INT_RK4, dt, NSUB)
    out, kern = eng.get_state(), eng.last_kernel
    eng.close()
    return out, kern


@pytest.mark.parametrize("closures", sorted(CLOSURES))
@pytest.mark.parametrize("shape,batch,rows", [((32, 128), 1, 0), ((64, 256), 3, 0), ((96, 128), 1, 0), ((64, 64), 1, 64),
                                              ((128, 64), 1, 64)])
def test_single_pass_tails_equal_stage_pairs_and_oracle(shape, batch, rows, closures):
    mu, mob, dt, oracle_closures = CLOSURES[closures]
    nx, ny = shape
    rng = np.random.default_rng(53)
    dom = std_domain(P, nx, ny)
    eq = P.CahnHilliard2DPeriodic(dom, 0.002, MU[mu], MOB[mob])
    u = white_noise_state(rng, (batch, nx, ny), np.float32, "c")
    kappas = 0.002 * (1.0 + 0.1 * np.arange(batch))
    got, kern = _solve(eq, u, dt, kappas, 0, rows)
    assert "rk4_quad" in kern and ("rows64" if rows == 64 else "rows32") in kern, kern
    pairs, kern1 = _solve(eq, u, dt, kappas, 1, 0)
    assert "stage_pair" in kern1, kern1
    assert np.isfinite(got).all() and np.any(got != u)
    assert np.array_equal(got, pairs)
    hx, hy = dom.dx
    cmu, cmob = oracle_closures()
    for b in sorted({0, batch - 1}):
        y0 = u[b].astype(np.float64)
        ref = CO.rk4(0, y0, hx, hy, kappas[b], cmu, cmob, dt, NSUB)
        err, tol = rel_l2(got[b].astype(np.float64) - y0, ref - y0), inc_tol_f32(ref, y0)
        print(f"{shape} b={b} {closures}: increment error {err:.3e} (tolerance {tol:.3e})")
        assert err < tol, (b, err, tol)


def test_halo8_tails_on_virtual_ranks_equal_monolithic():
    """2 x 1 ranks of 64 x 128 cells in the halo-8 layout: the HALO instantiation's tails, edge tiles fed from the
    neighbours' strips -- bitwise the monolithic periodic solve"""
    px, py, tx, ty = 2, 1, 64, 128
    nx, ny = px * tx, py * ty
    rng = np.random.default_rng(59)
    dom = std_domain(P, nx, ny)
    eq = P.CahnHilliard2DPeriodic(dom, 0.002, MU["regsol"], MOB["c1mc"])
    y0 = white_noise_state(rng, (nx, ny), np.float32, "c")
    want, kern = _solve(eq, y0[None], 2e-7, np.array([0.002]), 0, 0)
    assert "rk4_quad" in kern, kern
    comms = LocalGroupComm.create(px * py)
    solvers = []
    for r in range(px * py):
        be = HipTileBackend(eq, (tx, ty), np.float32, halo=8)
        be.engine.set_fuse_stages(0)
        s = DecomposedSolver(eq, CartesianGrid(px, py, r), comm=comms[r], dtype=np.float32, backend=be)
        s.set_global_state(y0)
        solvers.append(s)
    advance_group(solvers, 2e-7, 2)
    advance_group(solvers, 2e-7, NSUB - 2)
    got = np.empty_like(y0)
    for s in solvers:
        assert "rk4_quad<f32,CH,halo8" in s.backend.engine.last_kernel, s.backend.engine.last_kernel
        si, sj = s.grid.tile_slices(nx, ny)
        got[si, sj] = s.local_state()
        s.backend.engine.close()
    comms[0].group.close()
    assert np.array_equal(got, want[0])
