"""numpy reference of the rotating-frame alternating-direction split step, written from the
formulas: complex128, or complex64 with every array and transform held in single precision.

    Lx(s) v = ifft_x[exp(s Ax) fft_x v],   Ax(kx, y) = 0.5j (2 pi i kx)^2 - Omega y (2 pi i kx)
    Ly(s) v = ifft_y[exp(s Ay) fft_y v],   Ay(x, ky) = 0.5j (2 pi i ky)^2 + Omega x (2 pi i ky)
    psi1 = Ly(tau/2) Lx(tau/2) psi0;  b = -i (V + k |psi0|^2);  psi2 = psi1 exp(b tau)
    psi3 = psi2 / sqrt(h^2 sum |psi2|^2);  psi4 = Lx(tau/2) Ly(tau/2) psi3
"""
import math

import numpy as np


class RotCase:
    """the constant arrays of one (domain, k, e, omega, dx, time_scale) in the precision of the run"""

    def __init__(self, domain, k, e, omega, time_scale=1.0, double=True):
        self.c = np.complex128 if double else np.complex64
        self.r = np.float64 if double else np.float32
        x, y = domain.mesh()
        kx, ky = domain.fft_mesh()
        ikx, iky = 2j * np.pi * kx, 2j * np.pi * ky
        self.Ax = (0.5j * ikx**2 - omega * y * ikx).astype(self.c)
        self.Ay = (0.5j * iky**2 + omega * x * iky).astype(self.c)
        self.V = (0.5 * ((1 + e) * x**2 + (1 - e) * y**2)).astype(self.r)
        self.k = self.r(k)
        self.h2 = self.r(domain.dx[0] ** 2)
        self.time_scale = complex(time_scale)
        self._half = {}

    def fft(self, v, axis):
        return np.fft.fft(v, axis=axis).astype(self.c)

    def ifft(self, v, axis):
        return np.fft.ifft(v, axis=axis).astype(self.c)

    def half_ops(self, dt):
        if dt not in self._half:
            s = self.c(0.5 * dt * self.time_scale)
            self._half[dt] = (np.exp(s * self.Ax).astype(self.c), np.exp(s * self.Ay).astype(self.c))
        return self._half[dt]

    def step(self, psi, dt):
        """one step of a complex (nx, ny) field"""
        psi = np.asarray(psi).astype(self.c)
        ex, ey = self.half_ops(dt)
        tau = self.c(dt * self.time_scale)
        lx = lambda v: self.ifft(self.fft(v, 0) * ex, 0)
        ly = lambda v: self.ifft(self.fft(v, 1) * ey, 1)
        b = (-1j * (self.V + self.k * np.abs(psi) ** 2)).astype(self.c)
        v = ly(lx(psi))
        v = (v * np.exp(b * tau)).astype(self.c)
        v = (v / np.sqrt(np.sum(np.abs(v) ** 2) * self.h2)).astype(self.c)
        return lx(ly(v))

    def advance(self, psi, dt, n):
        for _ in range(n):
            psi = self.step(psi, dt)
        return psi


def to_pairs(psi):
    return np.stack([psi.real, psi.imag], axis=-1)


def from_pairs(y):
    return y[..., 0] + 1j * y[..., 1]


def solve(case, psi0, ts, dt0):
    """``PDEModel.solve``'s save semantics on the reference: steps of dt0 from ts[0], the last one clipped to ts[-1],
    save points inside a step interpolated linearly between the step's ends"""
    t0, t1 = float(ts[0]), float(ts[-1])
    span = t1 - t0
    n_full = int(math.floor(span / dt0 + 1e-9))
    rem = span - n_full * dt0
    if rem <= 1e-9 * dt0:
        rem = 0.0
    edges = [t0 + i * dt0 for i in range(n_full + 1)] + ([t1] if rem > 0 else [])
    states = [np.asarray(psi0).astype(case.c)]
    for i in range(len(edges) - 1):
        states.append(case.step(states[-1], dt0 if i < n_full else rem))
    out = []
    for tq in (float(t) for t in ts):
        i = int(np.searchsorted(edges, tq - 1e-12 * max(1.0, abs(tq))))
        if i == 0 or abs(edges[i] - tq) <= 1e-12 * max(1.0, abs(tq)):
            out.append(states[min(i, len(states) - 1)])
        else:
            th = (tq - edges[i - 1]) / (edges[i] - edges[i - 1])
            out.append(states[i - 1] + th * (states[i] - states[i - 1]))
    return np.stack(out)


def smooth_state(domain, seed, batch=1):
    """a smooth, seeded, normalised, non-symmetric wavefunction per environment: a few off-centre Gaussians with
    plane-wave phases"""
    rng = np.random.default_rng(seed)
    x, y = domain.mesh()
    (x0, x1), (y0, y1) = domain.box
    lx, ly = x1 - x0, y1 - y0
    out = []
    for _ in range(batch):
        psi = np.zeros(x.shape, dtype=np.complex128)
        for _ in range(3):
            cx, cy = x0 + lx * rng.uniform(0.35, 0.65), y0 + ly * rng.uniform(0.35, 0.65)
            w = rng.uniform(0.08, 0.14) * min(lx, ly)
            px, py = rng.uniform(-2, 2, 2) * 2 * np.pi / np.array([lx, ly])
            psi += rng.uniform(0.5, 1.0) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * w**2) + 1j * (px * x + py * y))
        psi /= np.sqrt(np.sum(np.abs(psi) ** 2) * domain.dx[0] ** 2)
        out.append(psi)
    return np.stack(out)
