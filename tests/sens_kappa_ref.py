"""fp64 numpy tangent-linear reference with kappa, the gradient-energy coefficient, among the parameters: the
Cahn-Hilliard (2-D, 3-D) and Allen-Cahn (2-D) FD right-hand sides and their Euler / RK4 / IMEX steps, built on the
oracle's primitives (oracle/np_oracle.py) and the closure derivatives of tests/sens_ref.py.  Test infrastructure only:
the GPU tangents (csrc/sens.hip, the KAPPA instantiations; csrc/spectral.hip, sens_imex_mul_kappa_kernel) and the finite
differences of the oracle are both checked against it.

``eq`` is ``"ch2d"``, ``"ac2d"`` or ``"ch3d"``; ``h`` the spacings ``(hx, hy)`` or ``(hx, hy, hz)``; ``params`` a list of
``(role, k)`` with role ``MU_ROLE``, ``MOB_ROLE`` (D, or Allen-Cahn's R) or ``KAPPA_ROLE`` (k = 0).

The kappa tangent's direct term is ``d m / d kappa = -lap(u)`` with ``m = mu_h(u) - kappa lap(u)``.  Under IMEX kappa also
moves the implicit operator ``L = 1 + A dt symbol``, ``symbol = kappa K2^2`` (linear in kappa):

    du1 = du0 + dt Re ifftn( fftn(df) / L ) - dt Re ifftn( A dt (symbol / kappa) fftn(f) / L^2 )

The functions keep the dtype of the state they are given (python scalars, complex64 transforms of float32 fields), so
running them on float32 inputs measures the reference's own float32-versus-float64 distance."""
import numpy as np

from oracle import np_oracle as O
from sens_ref import MOB_ROLE, MU_ROLE, closure_dc, closure_dcoef, perturbed  # noqa: F401  (re-exported)

KAPPA_ROLE = 2


def lap(u, h):
    """5- or 7-point Laplacian, in the oracle's order (x, y[, z] terms)"""
    return sum((O.nb(u, 1, ax) - 2 * u + O.nb(u, -1, ax)) / h[ax] ** 2 for ax in range(u.ndim))


def _cl(f, u):
    """a closure (or its derivative) in the dtype of u"""
    return np.asarray(f(u)).astype(u.dtype)


def rhs(eq, u, h, kappa, mu, mob):
    m = _cl(mu, u) - kappa * lap(u, h)
    if eq == "ac2d":
        return -_cl(mob, u) * m
    D = _cl(mob, u)
    out = 0.0
    for ax in range(u.ndim):
        out = out + O.div_face(O.avg_face(D, ax) * O.grad_face(m, h[ax], ax), h[ax], ax)
    return out


def tangent_rhs(eq, u, du, h, kappa, mu, mob, role, k):
    """J_f(u) du + d f / d p for the parameter (role, k)"""
    m = _cl(mu, u) - kappa * lap(u, h)
    D = _cl(mob, u)
    dmu = _cl(lambda c: closure_dc(mu, c), u) * du - kappa * lap(du, h)
    dD = _cl(lambda c: closure_dc(mob, c), u) * du
    if role == MU_ROLE:
        dmu = dmu + _cl(lambda c: closure_dcoef(mu, k, c), u)
    elif role == MOB_ROLE:
        dD = dD + _cl(lambda c: closure_dcoef(mob, k, c), u)
    else:
        assert role == KAPPA_ROLE and k == 0, (role, k)
        dmu = dmu - lap(u, h)
    if eq == "ac2d":
        return -dD * m - D * dmu
    out = 0.0
    for ax in range(u.ndim):
        F = O.avg_face(dD, ax) * O.grad_face(m, h[ax], ax) + O.avg_face(D, ax) * O.grad_face(dmu, h[ax], ax)
        out = out + O.div_face(F, h[ax], ax)
    return out


def slopes(eq, u, dus, params, h, kappa, mu, mob):
    return rhs(eq, u, h, kappa, mu, mob), [tangent_rhs(eq, u, du, h, kappa, mu, mob, r, k) for du, (r, k) in zip(dus, params)]


def symbol_of(shape, h, kappa):
    """kappa K2^2 on the grid, K2 = sum (2 pi i k_ax)^2 (cahn_hilliard.py:68-74, and its 3-D form)"""
    ks = np.meshgrid(*[np.fft.fftfreq(n, d) for n, d in zip(shape, h)], indexing="ij")
    k2 = sum((2j * np.pi * k) ** 2 for k in ks)
    return kappa * k2 ** 2


def step(eq, u, dus, params, dt, h, kappa, mu, mob, integrator, A=0.5, symbol=None):
    """one Euler, classical RK4 or IMEX step of the state and its tangents (the derivative of the discrete step)"""
    f = lambda v, dvs: slopes(eq, v, dvs, params, h, kappa, mu, mob)
    axpy = lambda a, k, dks: (u + a * k, [du + a * dk for du, dk in zip(dus, dks)])
    k1, d1 = f(u, dus)
    if integrator == "euler":
        return axpy(dt, k1, d1)
    if integrator == "imex":
        ctype = np.complex64 if u.dtype == np.float32 else np.complex128
        sym = np.asarray(symbol).astype(ctype)
        L = 1.0 + (A * dt) * sym
        fk = np.fft.fftn(k1)
        solve = lambda g: np.fft.ifftn(np.fft.fftn(g) / L).real.astype(u.dtype)
        out = []
        for du, dk, (role, _) in zip(dus, d1, params):
            new = du + dt * solve(dk)
            if role == KAPPA_ROLE:  # the operator's own derivative: dL/dkappa = A dt symbol / kappa
                new = new - dt * np.fft.ifftn((A * dt) * (sym / kappa) * fk / (L * L)).real.astype(u.dtype)
            out.append(new)
        return u + dt * solve(k1), out
    assert integrator == "rk4", integrator
    k2, d2 = f(*axpy(dt / 2, k1, d1))
    k3, d3 = f(*axpy(dt / 2, k2, d2))
    k4, d4 = f(*axpy(dt, k3, d3))
    comb = lambda a, b, c, d: (a + 2 * b + 2 * c + d) * (dt / 6)
    return u + comb(k1, k2, k3, k4), [du + comb(a, b, c, d) for du, a, b, c, d in zip(dus, d1, d2, d3, d4)]


def trajectory(eq, u0, params, dt, n, h, kappa, mu, mob, integrator, A=0.5, symbol=None):
    u, dus = u0, [np.zeros_like(u0) for _ in params]
    for _ in range(n):
        u, dus = step(eq, u, dus, params, dt, h, kappa, mu, mob, integrator, A, symbol)
    return u, dus


def end_state(eq, u0, dt, n, h, kappa, mu, mob, integrator, A=0.5):
    """the ORACLE's trajectory (np_oracle right-hand sides and steps) at one kappa: what central differences perturb"""
    if eq == "ch3d":
        f = lambda t, v: O.ch3d_rhs_fd(v, h[0], h[1], h[2], kappa, mu, mob)
    else:
        f = lambda t, v: (O.ch_rhs_fd if eq == "ch2d" else O.ac_rhs_fd)(v, h[0], h[1], kappa, mu, mob)
    sym = symbol_of(u0.shape, h, kappa) if integrator == "imex" else None
    u = u0
    for _ in range(n):
        if integrator == "imex":
            u = O.imex_step(f, 0.0, u, dt, A, sym)
        else:
            u = (O.euler_step if integrator == "euler" else O.rk4_step)(f, 0.0, u, dt)
    return u
