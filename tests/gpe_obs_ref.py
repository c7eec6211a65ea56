"""numpy reference of the GPE observables, written from the table of definitions: complex128,
or complex64 with the field, the potential and the transforms held in single precision and every sum in fp64 (like
``gpe_rot_ref.RotCase(double=False)``).

    norm  = h^2 sum |psi|^2            e_pot = h^2 sum V |psi|^2            e_int = h^2 sum k/2 |psi|^4
    e_kin = h^2 [sum 1/2 (2 pi kx)^2 Px + sum 1/2 (2 pi ky)^2 Py],   Px = |fft(psi, axis 0)|^2 / nx,  Py alike
    l_z   = h^2 [sum x (2 pi ky) Py - sum y (2 pi kx) Px]             x2, y2 = h^2 sum x^2 |psi|^2, h^2 sum y^2 |psi|^2
    energy = (kappa e_kin + e_pot + e_int - omega l_z) / norm,        mu = (kappa e_kin + e_pot + 2 e_int - omega l_z) / norm
"""
import numpy as np

NAMES = ("norm", "e_kin", "e_pot", "e_int", "l_z", "x2", "y2")


def trap(domain, e, trap_factor=1.0):
    x, y = domain.mesh()
    return 0.5 * trap_factor * ((1 + e) * x**2 + (1 - e) * y**2)


def observables(domain, psi, V, k, double=True):
    """``(values, scales)``: two dicts over ``NAMES`` for one complex (nx, ny) field; the scale of an observable is the
    sum of the absolute values of its terms (what an error of it is measured against: ``l_z`` cancels)"""
    c, r = (np.complex128, np.float64) if double else (np.complex64, np.float32)
    psi = np.asarray(psi).astype(c)
    nx, ny = psi.shape
    x, y = domain.mesh()
    kx, ky = domain.fft_mesh()
    h2 = domain.dx[0] * domain.dx[1]
    f64 = lambda a: np.asarray(a).astype(np.float64)
    d = f64(psi.real) ** 2 + f64(psi.imag) ** 2
    px = np.fft.fft(psi, axis=0).astype(c)
    py = np.fft.fft(psi, axis=1).astype(c)
    Px = (f64(px.real) ** 2 + f64(px.imag) ** 2) / nx
    Py = (f64(py.real) ** 2 + f64(py.imag) ** 2) / ny
    wx, wy = 2 * np.pi * kx, 2 * np.pi * ky
    Vr = f64(np.broadcast_to(np.asarray(V), psi.shape).astype(r))
    terms = {
        "norm": [d],
        "e_kin": [0.5 * wx**2 * Px, 0.5 * wy**2 * Py],
        "e_pot": [Vr * d],
        "e_int": [0.5 * float(r(k)) * d * d],
        "l_z": [x * wy * Py, -y * wx * Px],
        "x2": [x**2 * d],
        "y2": [y**2 * d],
    }
    vals = {n: h2 * float(sum(np.sum(t) for t in ts)) for n, ts in terms.items()}
    scales = {n: h2 * float(sum(np.sum(np.abs(t)) for t in ts)) for n, ts in terms.items()}
    return vals, scales


def derived(vals, omega=0.0, kappa=1.0):
    """``(energy, mu)`` per particle"""
    common = kappa * vals["e_kin"] + vals["e_pot"] - omega * vals["l_z"]
    return (common + vals["e_int"]) / vals["norm"], (common + 2 * vals["e_int"]) / vals["norm"]


def ground_state_loop(case, domain, psi0, k, omega, dt, tol=1e-8, check_every=25, max_steps=100_000):
    """``PDEModel.ground_state``'s loop on ``gpe_rot_ref.RotCase(..., time_scale=-1j)``: blocks of ``check_every`` steps,
    converged when ``|energy_now - energy_prev| / (check_every dt) <= tol``.  Returns ``(psi, steps, converged,
    history)``, history = [(energy, mu)] per check"""
    psi, prev, done, hist = np.asarray(psi0).astype(case.c), None, 0, []
    while done < max_steps:
        n = min(check_every, max_steps - done)
        psi = case.advance(psi, dt, n)
        done += n
        e, mu = derived(observables(domain, psi, case.V, k)[0], omega)
        hist.append((e, mu))
        if prev is not None and abs(e - prev) / (n * dt) <= tol:
            return psi, done, True, hist
        prev = e
    return psi, done, False, hist
