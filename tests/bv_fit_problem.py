"""The synthetic fit of tests/test_gpu_bv_fit.py -- recover mu and j0 of a constant-current Butler-Volmer run from frames,
with and without the voltage curve -- and the same fit on the CPU: fp64 numpy tangents (tests/bv_sens_ref.py) under the
library's own Levenberg-Marquardt (``cpu_fit``).  ``python tests/bv_fit_problem.py`` prints the figures the GPU test is
gated against (10 x them, the convention of tests/test_gpu_sens_ac.py).

32 x 64 cells, B = 2 trajectories, 200 RK4 steps of 1e-6 with save points after 60, 130 and 200 steps.  The states are the
notebook's noise relaxed for a short time only (``T_RELAX``), so that the fields still move by several per cent in 2e-4.

At constant current mu's constant coefficient cannot be seen in the frames: a shift of mu is absorbed by the voltage
(v -> v - c, eta = mu + v stands still).  The frames-only fit leaves it where it started (its Gauss-Newton column is zero)
and is judged on the other entries; the voltage curve (dv/dmu_0 = -1) is what pins it down."""
import numpy as np

import bv_ref as R
import bv_sens_ref as S
from pde_opt_amd import fit

NX, NY = 32, 64
H, KAPPA, ALPHA, CRATE = S.H, S.KAPPA, S.ALPHA, 0.02
MU_TRUE, J0_TRUE = [0.1, -3.0, 0.2], [-0.9, 0.15]
MU_INIT, J0_INIT = [0.3, -2.7, 0.3], [-0.7, 0.1]
DT = 1e-6
SAVE_STEPS = (60, 130, 200)
TS = np.array([0.0] + [k * DT for k in SAVE_STEPS])
T_RELAX = 1e-3
SEEDS = (1, 2)
VOLTAGE_WEIGHT = 1.0
PARAMS = S.PARAMS


def logit(c):
    return np.log(c / (1.0 - c))


def y0s():
    u = np.stack([R.relaxed_state(s, NX, NY, t_relax=T_RELAX) for s in SEEDS])
    assert 0.05 < u.min() and u.max() < 0.95
    return u


def closures(p):
    return S.Closure(S.MU_DESC.with_coef(p[:3])), S.Closure(S.J0_DESC.with_coef(p[3:]))


def reference_solve(p, u0s, tangents=True, save_steps=SAVE_STEPS):
    """frames, voltages and their tangents at the save points from the numpy reference: ``(ys (T-1, B, nx, ny),
    V (T-1, B), dys (T-1, B, P, nx, ny), dV (T-1, B, P))`` (the last two None without tangents)"""
    mu, j0 = closures(p)
    Pn = len(PARAMS)
    ys, V, dys, dV = [], [], [], []
    for u0 in u0s:
        rows = []
        if tangents:
            f = S.current_rhs(PARAMS, H, H, KAPPA, ALPHA, CRATE, mu, j0)

            def visit(i, u, dus):
                if i in save_steps:
                    v, dvs, _, _ = S.voltage_tangents(u, dus, PARAMS, H, H, KAPPA, CRATE, mu, j0)
                    rows.append((u, v, np.stack(dus), np.array(dvs)))

            S.trajectory(f, u0, Pn, DT, save_steps[-1], "rk4", visit)
        else:
            rhs, u, done = (lambda t, y: R.rhs_current(y, H, H, KAPPA, ALPHA, CRATE, mu, j0)), u0, 0
            for k in save_steps:
                u = R.steps(rhs, u, DT, k - done, "rk4")
                done = k
                rows.append((u, R.voltage(u, H, H, KAPPA, CRATE, mu, j0), None, None))
        ys.append([r[0] for r in rows])
        V.append([r[1] for r in rows])
        dys.append([r[2] for r in rows])
        dV.append([r[3] for r in rows])
    sw = lambda a: np.swapaxes(np.array(a), 0, 1)  # noqa: E731
    return sw(ys), sw(V), (sw(dys) if tangents else None), (sw(dV) if tangents else None)


def cpu_fit(voltage_weight=0.0, max_steps=100):
    """the fit with the numpy reference in place of the GPU: ``(p, parameter error over the identifiable entries, final
    loss mean(r^2) + voltage_weight mean(r_V^2), solves)``"""
    u0s = y0s()
    p_true = np.array(MU_TRUE + J0_TRUE)
    data, v_obs, _, _ = reference_solve(p_true, u0s, tangents=False)
    M = data.size
    w_v = voltage_weight * M / v_obs.size
    n = [0]

    def sums(p):
        n[0] += 1
        ys, V, dys, dV = reference_solve(p, u0s)
        r = (data - ys).reshape(-1)
        J = np.moveaxis(dys, 2, -1).reshape(-1, len(PARAMS))
        out = float(r @ r), J.T @ r, J.T @ J
        if voltage_weight:
            out = fit.add_voltage_sums(*out, v_obs - V, dV, w_v)
        return out

    def ssr(p):
        ys, V, _, _ = reference_solve(p, u0s, tangents=False)
        return float(np.sum((data - ys) ** 2)) + (w_v * float(np.sum((v_obs - V) ** 2)) if voltage_weight else 0.0)

    obj = fit.Objective(sums=sums, ssr=ssr, M=M)
    p, _ = fit.levenberg_marquardt(obj, np.array(MU_INIT + J0_INIT), max_steps=max_steps)
    return p, param_error(p, bool(voltage_weight)), ssr(p) / M, n[0]


def param_error(p, with_voltage):
    """max |p - p_true| over the entries the data can see: all of them with the voltage curve, all but mu's constant
    coefficient without"""
    d = np.abs(np.asarray(p) - np.array(MU_TRUE + J0_TRUE))
    return float(np.max(d if with_voltage else d[1:]))


if __name__ == "__main__":
    for w in (0.0, VOLTAGE_WEIGHT):
        p, err, loss, n = cpu_fit(w)
        print(f"voltage_weight = {w}: p = {np.array2string(p, precision=12)}, error = {err:.3e}, loss = {loss:.3e}   ({n} solves)")
