"""numpy reference of the stirred, ramped rotating-frame split step, on top of
``gpe_rot_ref.RotCase``: the step that starts at local time t0 uses

    Omega(t0) = omega + omega_rate t0   in all four line operators,    V(t0) = trap + lights(t0, X, Y)   in b,

complex128, or complex64 with every array held single (the rotation operators, the potential and the light field are
formed in double and rounded once, as ``RotCase`` rounds its constant arrays).
"""
import numpy as np

import gpe_rot_ref as R


class StirCase(R.RotCase):
    """``RotCase`` plus ``lights`` (a callable ``lights(t, X, Y)`` or None) and ``omega_rate``"""

    def __init__(self, domain, k, e, omega, time_scale=1.0, double=True, lights=None, omega_rate=0.0):
        super().__init__(domain, k, e, omega, time_scale, double)
        self.omega, self.omega_rate, self.lights = float(omega), float(omega_rate), lights
        self.x, self.y = domain.mesh()
        kx, ky = domain.fft_mesh()
        self.ikx, self.iky = 2j * np.pi * kx, 2j * np.pi * ky

    def omega_at(self, t0):
        return self.omega + self.omega_rate * float(t0)

    def potential(self, t0):
        if self.lights is None:
            return self.V
        light = np.broadcast_to(np.asarray(self.lights(float(t0), self.x, self.y), dtype=np.float64), self.V.shape)
        return (self.V + light.astype(self.r)).astype(self.r)

    def half_ops_at(self, dt, t0):
        """the half operators rebuilt from Omega(t0)"""
        om = self.omega_at(t0)
        ax = (0.5j * self.ikx**2 - om * self.y * self.ikx).astype(self.c)
        ay = (0.5j * self.iky**2 + om * self.x * self.iky).astype(self.c)
        s = self.c(0.5 * dt * self.time_scale)
        return np.exp(s * ax).astype(self.c), np.exp(s * ay).astype(self.c)

    def step(self, psi, dt, t0=0.0):
        """one step of a complex (nx, ny) field from local time t0"""
        psi = np.asarray(psi).astype(self.c)
        ex, ey = self.half_ops_at(dt, t0)
        tau = self.c(dt * self.time_scale)
        lx = lambda v: self.ifft(self.fft(v, 0) * ex, 0)
        ly = lambda v: self.ifft(self.fft(v, 1) * ey, 1)
        b = (-1j * (self.potential(t0) + self.k * np.abs(psi) ** 2)).astype(self.c)
        v = ly(lx(psi))
        v = (v * np.exp(b * tau)).astype(self.c)
        v = (v / np.sqrt(np.sum(np.abs(v) ** 2) * self.h2)).astype(self.c)
        return lx(ly(v))

    def advance(self, psi, dt, n, t0=0.0):
        """n steps; step s starts at t0 + s dt (the local time ``pdeopt_advance`` hands its substep s)"""
        for s in range(n):
            psi = self.step(psi, dt, t0 + s * dt)
        return psi


def solve(case, psi0, ts, dt0):
    """``gpe_rot_ref.solve``'s save semantics on the new step: step i starts at ts[0] + i dt0"""

    class Timed:
        c = case.c

        def __init__(self):
            self.i = 0

        def step(self, psi, dt):
            t = float(ts[0]) + self.i * dt0
            self.i += 1
            return case.step(psi, dt, t)

    return R.solve(Timed(), psi0, ts, dt0)
