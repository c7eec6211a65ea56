"""Inputs and references for the spectral steps on broadband states with multiplier tables that have no symmetry
(tests/test_spectral_ref_cpu.py, tests/test_gpu_spectral_broadband.py).  A helper, not a test.

The Strang and the IMEX step at complex128 are ``oracle/np_oracle.py::strang_step`` and ``imex_step``: they take any table
and stay the definition.  ``strang_step_single`` / ``imex_step_single`` are the same steps with every transform (and all
arithmetic) in single precision, through ``torch.fft`` on the CPU -- this numpy's ``np.fft`` computes in complex128 whatever
it is given.  Their distance from the complex128 reference on a case is what the fp32 gates of the GPU tests are made of.

Tables (one independent complex value per bin, so any permutation of a table changes the result):
    Strang:  A = eq.A_term + R,  R complex, uniform per bin, |R tau / 2| <= 0.5 with tau = dt time_scale
    IMEX:    symbol = s0 (1 + r) + i s0 r',  s0 the equation's fourier_symbol, r and r' uniform in [-0.5, 0.5] per bin:
             Re symbol >= 0, so |1 + A dt symbol| >= 1
States: complex standard normal per cell, normalised with the reference's dx[0]^2 cell area (Strang);
clip(0.5 + 0.05 N(0, 1), 0.05, 0.95) (IMEX, as tests/test_gpu_fuzz.py)."""
import numpy as np
import torch

from oracle import np_oracle as O
from util import MOB, MU, rel_l2

# ---- the cases of the GPU tests (the CPU test checks that every one of them discriminates) -----------------------------

FFT_SIZES = (64, 128, 256, 512, 1024)  # PDEOPT_FFT_SIZES of csrc/strang_fused.hip
TIME_SCALES = (1.0, -1j, 0.3 - 1j)
STRANG_DT, STRANG_STEPS, STRANG_BATCH = 1e-3, 3, 3
# every transform size once as nx and once as ny with nx != ny, the square one for the transposed table, rocFFT sizes
STRANG_FUSED_SHAPES = ((64, 128), (128, 64), (256, 64), (64, 512), (512, 256), (1024, 64), (64, 1024), (128, 128))
STRANG_ROCFFT_SHAPES = ((48, 40), (96, 80))
STRANG_GENERIC_SHAPE = (128, 64)  # rocFFT forced on a size the fused kernels cover

IMEX_A, IMEX_DT, IMEX_STEPS, KAPPA = 0.5, 1e-6, 3, 0.002
IMEX_FUSED_SHAPES = ((64, 256), (256, 64), (128, 1024), (1024, 128), (512, 64))
IMEX_PER_ENV_SHAPE, IMEX_PER_ENV_SCALES = (128, 256), (1.0, 1.25, 1.5)
IMEX_ROCFFT_SHAPES = ((48, 40), (96, 80), (256, 1), (1, 96))
IMEX_GENERIC_SHAPE = (128, 64)
IMEX_3D_SHAPES = ((16, 12, 20), (8, 6, 10))

# (shape, path): "fused" = the hand-written transforms, "rocfft" = sizes they do not cover, "generic" = rocFFT forced
STRANG_CASES = ([(s, "fused") for s in STRANG_FUSED_SHAPES] + [(s, "rocfft") for s in STRANG_ROCFFT_SHAPES]
                + [(STRANG_GENERIC_SHAPE, "generic")])
# (shape, batch, path): "per_env" = one environment per complex field (unequal set_env_imex_scale)
IMEX_CASES = ([(s, b, "fused") for s in IMEX_FUSED_SHAPES for b in (2, 3)] + [(IMEX_PER_ENV_SHAPE, 3, "per_env")]
              + [(s, 2, "rocfft") for s in IMEX_ROCFFT_SHAPES] + [(IMEX_GENERIC_SHAPE, 3, "generic")]
              + [(s, 2, "rocfft") for s in IMEX_3D_SHAPES])


def imex_case(P, shape, batch, path):
    return ImexCase(P, shape, batch, scales=IMEX_PER_ENV_SCALES if path == "per_env" else None)


# the project's gates: fp64 relative L2 (tests/test_gpu_fuzz.py: Strang states; tests/test_gpu_fft.py: IMEX increments)
# and the fp32 ceilings that stay on top of the computed fp32 gate
STRANG_GATE64, STRANG_CEIL32 = 1e-10, 2e-5
IMEX_GATE64, IMEX_CEIL32 = 1e-9, 5e-4
F32_MARGIN = 8.0  # x the single-precision reference's own distance: the device rounds in another order


def gate32(ref_distance, ceiling):
    return min(F32_MARGIN * ref_distance, ceiling)


# ---- tables ---------------------------------------------------------------------------------------------------------


def mirrored(table):
    """table(-k): index (n - i) % n along every axis"""
    return table[np.ix_(*[(-np.arange(n)) % n for n in table.shape])]


def strang_table(A_even, dt, time_scale, seed):
    rng = np.random.default_rng(seed)
    A_even = np.asarray(A_even, dtype=np.complex128)
    scale = 0.5 / (np.sqrt(2.0) * abs(dt * time_scale) / 2.0)
    R = scale * (rng.uniform(-1.0, 1.0, A_even.shape) + 1j * rng.uniform(-1.0, 1.0, A_even.shape))
    assert np.abs(R * dt * time_scale / 2.0).max() <= 0.5
    return A_even + R


def imex_table(s0, seed):
    rng = np.random.default_rng(seed)
    s0 = np.real(np.asarray(s0)).astype(np.float64)
    return s0 * (1.0 + rng.uniform(-0.5, 0.5, s0.shape)) + 1j * s0 * rng.uniform(-0.5, 0.5, s0.shape)


def symmetrised(M):
    """M_h(k) = (M(k) + conj M(-k)) / 2: Re ifftn(M fftn f) = ifftn(M_h fftn f) for a real f"""
    return 0.5 * (M + np.conj(mirrored(M)))


# ---- Strang --------------------------------------------------------------------------------------------------------

GPE_K, GPE_E = 500.0, 0.2
GPE_LIGHTS = lambda t, x, y: 0.05 * x - 0.02 * y  # noqa: E731


class StrangCase:
    """the GPE of tests/test_gpu_fft.py on the box (-12, 12) x (-9, 9), kinetic A_term + R, white noise, one interaction
    strength per environment"""

    def __init__(self, P, shape, time_scale, batch=STRANG_BATCH, seed=0):
        nx, ny = shape
        self.shape, self.time_scale, self.dt, self.steps = tuple(shape), time_scale, STRANG_DT, STRANG_STEPS
        self.dom = P.Domain((nx, ny), ((-12.0, 12.0), (-9.0, 9.0)), "dimensionless")
        self.eq = P.GPE2DTSControl(self.dom, GPE_K, GPE_E, GPE_LIGHTS, trap_factor=1.0, kinetic=True)
        self.X, self.Y = self.dom.mesh()
        self.dx = float(self.eq.dx)
        self.A_even = np.asarray(self.eq.A_term, dtype=np.complex128)
        self.A = strang_table(self.A_even, self.dt, time_scale, seed + 1)
        self.ks = GPE_K * (1.0 + 0.1 * np.arange(batch))
        rng = np.random.default_rng(seed)
        psi = (rng.standard_normal((batch, nx, ny)) + 1j * rng.standard_normal((batch, nx, ny))) / np.sqrt(2.0)
        psi /= np.sqrt(np.sum(np.abs(psi) ** 2, axis=(1, 2), keepdims=True) * self.dx**2)
        self.y0 = np.stack([psi.real, psi.imag], axis=-1)

    def solver(self, P, table=None):
        return P.StrangSplitting(self.A if table is None else table, self.eq.dx, self.eq.fft, self.eq.ifft, self.time_scale)

    def reference(self, y0, table=None):
        """complex128 (np_oracle.strang_step) from the state y0 (batch, nx, ny, 2) of any real dtype"""
        table = self.A if table is None else table
        lights = GPE_LIGHTS(0.0, self.X, self.Y)
        out = []
        for b, y in enumerate(np.asarray(y0, dtype=np.float64)):
            bt = lambda t, yy, k=self.ks[b]: O.gpe_b_terms(yy, self.X, self.Y, k, GPE_E, 1.0, lights)
            for i in range(self.steps):
                y = O.strang_step(bt, i * self.dt, y, self.dt, table, self.dx, self.time_scale)
            out.append(y)
        return np.stack(out)

    def reference_single(self, y0, table=None, double=False):
        """the same steps with every transform and all arithmetic at complex64 (``double``: complex128, to hold this
        restatement against np_oracle)"""
        table = self.A if table is None else table
        real, cplx = (torch.float64, torch.complex128) if double else (torch.float32, torch.complex64)
        A = torch.as_tensor(table).to(cplx)
        V = torch.as_tensor(0.5 * ((1 + GPE_E) * self.X**2 + (1 - GPE_E) * self.Y**2) + GPE_LIGHTS(0.0, self.X, self.Y)).to(real)
        out = []
        for b, y in enumerate(np.asarray(y0)):
            y = torch.as_tensor(np.ascontiguousarray(y)).to(real)
            for _ in range(self.steps):
                y = strang_step_single(y, V, float(self.ks[b]), self.dt, A, self.dx, self.time_scale)
            assert y.dtype == real
            out.append(y.double().numpy())
        return np.stack(out)


def strang_step_single(y, V, k, dt, A, dx, time_scale):
    """np_oracle.strang_step (solvers.py:99-115 of the reference) in the precision of its torch arguments"""
    cplx = A.dtype
    psi = torch.view_as_complex(y.contiguous())
    tau = torch.tensor(dt * complex(time_scale), dtype=cplx)
    e_half = torch.exp(A * (0.5 * tau))
    b = (-1j * (V + k * (psi.real**2 + psi.imag**2)).to(cplx))
    psi = torch.fft.ifftn(torch.fft.fftn(psi) * e_half)
    psi = psi * torch.exp(b * tau)
    psi = psi / torch.sqrt(torch.sum(psi.real**2 + psi.imag**2) * dx**2)
    psi = torch.fft.ifftn(torch.fft.fftn(psi) * e_half)
    assert psi.dtype == cplx, psi.dtype  # no transform upcast on the way
    return torch.view_as_real(psi)


# ---- IMEX ----------------------------------------------------------------------------------------------------------


class ImexCase:
    """Cahn-Hilliard (regular solution, D = c (1 - c)) on a grid of spacing 0.01 in 1, 2 or 3 dimensions with the
    asymmetric complex symbol; ``scales``: environment b integrates with scales[b] x kappa and scales[b] x the symbol"""

    def __init__(self, P, shape, batch, scales=None, seed=0):
        self.shape, self.batch, self.dt, self.steps, self.A = tuple(shape), batch, IMEX_DT, IMEX_STEPS, IMEX_A
        h = 0.01
        self.dom = P.Domain(self.shape, tuple((-h * n / 2, h * n / 2) for n in self.shape), "dimensionless")
        cls = P.CahnHilliard3DPeriodic if len(self.shape) == 3 else P.CahnHilliard2DPeriodic
        self.eq = cls(self.dom, KAPPA, MU["regsol"], MOB["c1mc"])
        self.s0 = np.real(np.asarray(self.eq.fourier_symbol)).astype(np.float64)
        self.symbol = imex_table(self.s0, seed + 1)
        self.scales = np.ones(batch) if scales is None else np.asarray(scales, dtype=np.float64)
        rng = np.random.default_rng(seed)
        self.y0 = np.clip(0.5 + 0.05 * rng.standard_normal((batch,) + self.shape), 0.05, 0.95)

    def solver(self, P, table=None):
        return P.SemiImplicitFourierSpectral(self.A, self.symbol if table is None else table, self.eq.fft, self.eq.ifft)

    def rhs(self, b):
        # Python floats: a numpy float64 scalar would lift a float32 state to float64
        h, kap = [float(v) for v in self.dom.dx], float(KAPPA * self.scales[b])
        if len(self.shape) == 3:
            return lambda t, u: O.ch3d_rhs_fd(u, h[0], h[1], h[2], kap, MU["regsol"], MOB["c1mc"])
        return lambda t, u: O.ch_rhs_fd(u, h[0], h[1], kap, MU["regsol"], MOB["c1mc"])

    def reference(self, y0, table=None):
        """complex128 (np_oracle.imex_step) from the states y0 (batch, *shape) of any real dtype"""
        table = self.symbol if table is None else table
        out = []
        for b, y in enumerate(np.asarray(y0, dtype=np.float64)):
            f = self.rhs(b)
            for i in range(self.steps):
                y = O.imex_step(f, i * self.dt, y, self.dt, self.A, self.scales[b] * table)
            out.append(y)
        return np.stack(out)

    def reference_single(self, y0, table=None, double=False):
        """the same steps with the right-hand side in float32 and every transform at complex64"""
        table = self.symbol if table is None else table
        real, cplx = (np.float64, torch.complex128) if double else (np.float32, torch.complex64)
        out = []
        for b, y in enumerate(np.asarray(y0)):
            f = self.rhs(b)
            denom = 1.0 + self.A * self.dt * torch.as_tensor(self.scales[b] * table).to(cplx)
            y = y.astype(real)
            for i in range(self.steps):
                y = imex_step_single(f, i * self.dt, y, self.dt, denom)
            assert y.dtype == real
            out.append(y.astype(np.float64))
        return np.stack(out)


def imex_step_single(rhs, t0, y0, dt, denom):
    """np_oracle.imex_step (solvers.py:56-63 of the reference) in the precision of y0 / denom"""
    f0 = torch.as_tensor(np.ascontiguousarray(rhs(t0, y0)))
    assert f0.dtype == torch.as_tensor(y0).dtype
    inc = torch.fft.ifftn(torch.fft.fftn(f0) / denom)
    assert inc.dtype == denom.dtype, inc.dtype  # no transform upcast on the way
    return y0 + y0.dtype.type(dt) * inc.real.numpy()


def increments_distance(got, want, y0):
    """largest relative L2 distance of the increments over the environments"""
    y0 = np.asarray(y0, dtype=np.float64)
    return max(rel_l2(np.asarray(g, np.float64) - y, w - y) for g, w, y in zip(got, want, y0))


def states_distance(got, want):
    return max(rel_l2(g, w) for g, w in zip(got, want))
