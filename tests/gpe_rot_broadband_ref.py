"""Inputs, references, gates and mutants for the rotating-frame split step on white noise
(tests/test_gpe_rot_broadband_cpu.py, tests/test_gpu_gpe_rot_broadband.py).  A helper, not a test.

The smooth states of tests/gpe_rot_ref.py leave the upper bins of the longer lines at rounding level, so a wrong frequency
slot, digit reversal, late-stage twiddle or Nyquist sign in the line operator moves the result by 1e-15 there.  Here every
cell holds an independent complex normal number, so every bin of every line carries weight.

Domain: one cell size H for every shape, the box (-n H / 2, n H / 2) per axis, so hx = hy (the solver's norm weight is
unambiguous) and the largest coordinate grows with the line length.  With DT the real part of (tau / 2) Ax and (tau / 2) Ay
stays below DAMPING_BOUND over every bin, line, environment, time scale and step of every case (``damping`` measures it,
``make_case`` asserts it): no bin is damped away or overflows in imaginary time.

References: ``gpe_rot_ref.RotCase`` / ``gpe_rot_stir_ref.StirCase`` at complex128 stay the definition.  The
single-precision reference is the same class with ``TorchTransforms`` mixed in: this numpy's ``np.fft`` computes in
complex128 whatever it is given, so ``RotCase(double=False)`` rounds only between transforms, which is kinder than any
device transform on white noise at N = 1024.  Through ``torch.fft`` on the CPU the transforms themselves run at complex64,
and the distance of that run from the complex128 one on a case is what the case's fp32 gate is made of.

Mutants: the complex128 reference with one fault of the kind a line kernel can have (``MUTANTS``).  The CPU test holds every
applicable one at 10 x the fp32 gate or more on every GPU case, so a device result inside the gate excludes them all."""
import functools

import numpy as np
import torch

import pde_opt_amd as P
from pde_opt_amd.numerics.functions.lights import GaussianSpot, GaussianSpots

import gpe_rot_ref as R
import gpe_rot_stir_ref as S

# ---- the cases of the GPU tests (the CPU test checks that every one of them discriminates) -----------------------------

ROT_SIZES = (64, 128, 256, 512, 1024)  # PDEOPT_ROT_SIZES of csrc/gpe_rot_step.hpp
H, DT, STEPS, BATCH = 0.1875, 2e-3, 3, 3
TIME_SCALES = (1.0, -1j, 0.3 - 1j)
E = 0.1
KS = (50.0, 55.0, 60.0)  # 50 (1, 1.1, 1.2): one interaction strength and one Omega per environment (EnvParams)
OMEGAS = (0.7, -0.45, 0.0)
# every line length as nx and as ny with nx != ny, a square one, sizes only rocFFT covers
FUSED_SHAPES = ((64, 128), (128, 64), (256, 64), (64, 256), (512, 256), (64, 512), (1024, 64), (64, 1024), (256, 256))
ROCFFT_SHAPES = ((48, 40), (96, 80))
GENERIC_SHAPE = (128, 64)  # rocFFT forced on a size the fused passes cover
# (shape, path): "fused" = the hand-written line transforms, "rocfft" = sizes they do not cover, "generic" = rocFFT forced
FROZEN_CASES = tuple([(s, "fused") for s in FUSED_SHAPES] + [(s, "rocfft") for s in ROCFFT_SHAPES] + [(GENERIC_SHAPE, "generic")])

# the stirred variant: two moving spots and a rotation ramp per environment, the trap's anisotropy per environment too (a
# per-environment potential), steps from the local time T0
T0 = 0.3
STIR_ES = (0.1, 0.15, 0.2)
STIR_RATES = (0.9, 0.2, -0.5)
STIR_CASES = tuple([(s, "fused") for s in ((256, 64), (64, 256), (64, 1024), (1024, 64), (512, 256))] + [((48, 40), "rocfft")])

# shape, precision of the bitwise tests: a wave-local column pass in fp32, a 256-point row pass in fp64, and the fp64
# 1024-point column pass whose JOIN runs as LAST + FIRST
BITWISE_CASES = (((256, 64), np.float32), ((64, 256), np.float64), ((1024, 64), np.float64))

GATE64 = 1e-10  # tests/test_gpu_gpe_rot.py
F32_MARGIN = 8.0  # x the single-precision reference's own distance (tests/test_gpu_gpe_adjoint.py, spectral_ref.gate32)
CEIL32 = 2e-5  # the project's Strang ceiling
MUTANT_MARGIN = 10.0  # x the fp32 gate: what every applicable mutant moves every case by, at least
DAMPING_BOUND = 3.0


def gate32(ref_distance):
    return min(F32_MARGIN * ref_distance, CEIL32)


def dist(a, b):
    """max-abs distance relative to max-abs, over the whole batch"""
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def domain(shape):
    return P.Domain(tuple(shape), tuple((-n * H / 2, n * H / 2) for n in shape), "dimensionless")


@functools.lru_cache(maxsize=None)
def white_noise(shape, batch=BATCH, seed=0):
    """complex standard normal per cell, normalised with H^2, rounded to single precision so that both precisions of the
    device and every reference start from the same numbers; (batch, nx, ny) complex128, read-only"""
    rng = np.random.default_rng(seed)
    psi = (rng.standard_normal((batch,) + tuple(shape)) + 1j * rng.standard_normal((batch,) + tuple(shape))) / np.sqrt(2.0)
    psi /= np.sqrt(np.sum(np.abs(psi) ** 2, axis=(1, 2), keepdims=True) * H**2)
    psi = psi.astype(np.complex64).astype(np.complex128)
    psi.flags.writeable = False
    return psi


def spots_of(b):
    """two moving spots of environment b, off-centre, placed and moving differently in x and y (as
    tests/test_gpu_gpe_rot_stir.py)"""
    return GaussianSpots([GaussianSpot(3.0 + b, 0.5, -0.6 + 0.1 * b, 0.8, 0.3 - 0.07 * b, -0.4, 0.35),
                          GaussianSpot(-2.0, 1.0 + b, 0.7, -0.5 - 0.2 * b, -0.45, 0.6 + 0.1 * b, 0.25 + 0.05 * b)])


def params_of(b, stirred):
    """the fields of ``GPE2DTSRot`` of environment b"""
    if stirred:
        return dict(k=KS[b], e=STIR_ES[b], omega=OMEGAS[b], lights=spots_of(b), omega_rate=STIR_RATES[b])
    return dict(k=KS[b], e=E, omega=OMEGAS[b])


# ---- references -----------------------------------------------------------------------------------------------------


class TorchTransforms:
    """mixin over ``RotCase`` / ``StirCase``: every transform through ``torch.fft`` on the CPU in the precision of the
    case, complex64 for ``double=False``"""

    def _transform(self, f, v, axis):
        out = f(torch.from_numpy(np.ascontiguousarray(v, dtype=self.c)), dim=axis)
        assert out.dtype == (torch.complex128 if self.c is np.complex128 else torch.complex64), out.dtype  # no upcast
        return out.numpy()

    def fft(self, v, axis):
        return self._transform(torch.fft.fft, v, axis)

    def ifft(self, v, axis):
        return self._transform(torch.fft.ifft, v, axis)


class TorchRotCase(TorchTransforms, R.RotCase):
    pass


class TorchStirCase(TorchTransforms, S.StirCase):
    pass


PRECISIONS = ("double", "single", "torch_double")  # numpy complex128; torch complex64; torch complex128


def damping(shape, stirred):
    """max |Re (tau / 2) A| over both line operators, every bin and line, environment, time scale and step"""
    dom = domain(shape)
    x, y = dom.mesh()
    kx, ky = dom.fft_mesh()
    ikx, iky = 2j * np.pi * kx, 2j * np.pi * ky
    worst = 0.0
    for b in range(BATCH):
        times = [T0 + s * DT for s in range(STEPS)] if stirred else [0.0]
        for t in times:
            om = OMEGAS[b] + (STIR_RATES[b] * t if stirred else 0.0)
            for ts in TIME_SCALES:
                s = 0.5 * DT * complex(ts)
                worst = max(worst, float(np.abs((s * (0.5j * ikx**2 - om * y * ikx)).real).max()),
                            float(np.abs((s * (0.5j * iky**2 + om * x * iky)).real).max()))
    return worst


@functools.lru_cache(maxsize=None)
def _damping_checked(shape, stirred):
    d = damping(shape, stirred)
    assert d <= DAMPING_BOUND, (shape, stirred, d)
    return d


def make_case(shape, b, time_scale, stirred, precision="double", mutant=None):
    """the reference of environment b of a case; ``mutant``: one of MUTANTS, the reference with that fault"""
    _damping_checked(tuple(shape), bool(stirred))
    dom = domain(shape)
    p = params_of(b, stirred)
    double = precision != "single"
    torch_fft = precision != "double"
    if stirred:
        cls = TorchStirCase if torch_fft else S.StirCase
        case = cls(dom, p["k"], p["e"], p["omega"], time_scale, double, p["lights"], p["omega_rate"])
    else:
        cls = TorchRotCase if torch_fft else R.RotCase
        case = cls(dom, p["k"], p["e"], p["omega"], time_scale, double)
    if mutant is not None:
        _mutate(case, dom, p, mutant)
    return case


def run(case, psi, stirred):
    """the states after 1 step and after STEPS steps (step s of the stirred case starts at T0 + s DT)"""
    out = []
    for s in range(STEPS):
        psi = case.step(psi, DT, T0 + s * DT) if stirred else case.step(psi, DT)
        if s in (0, STEPS - 1):
            out.append(np.asarray(psi).astype(np.complex128))
    return out


def mutant_reference(shape, time_scale, stirred, mutant, precision="double", envs=range(BATCH)):
    """(after 1 step, after STEPS steps), each (len(envs), nx, ny) complex128 and read-only, from ``white_noise(shape)``"""
    per_env = [run(make_case(shape, b, time_scale, stirred, precision, mutant), white_noise(tuple(shape))[b], stirred)
               for b in envs]
    out = tuple(np.stack([e[i] for e in per_env]) for i in range(2))
    for a in out:
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=16)  # the tests that share a case's references stand next to each other
def reference(shape, time_scale, stirred, precision="double"):
    """the reference without a fault, computed once per case and shared"""
    return mutant_reference(shape, time_scale, stirred, None, precision)


def gates32(shape, time_scale, stirred):
    """(the single-precision reference's distance, the fp32 gate) after 1 step and after STEPS steps"""
    want = reference(shape, time_scale, stirred)
    own = reference(shape, time_scale, stirred, "single")
    return tuple((dist(o, w), gate32(dist(o, w))) for o, w in zip(own, want))


# ---- mutants --------------------------------------------------------------------------------------------------------

# per axis: the Nyquist bin taken as +N/2, neighbouring upper bins exchanged, the bins in bit-reversed order, the line's coordinate
# off by one cell, the line's coordinate taken along the other axis's mesh; then the sign of Omega and a conjugated multiplier
MUTANTS = ("nyquist_x", "nyquist_y", "exchange_x", "exchange_y", "bitrev_x", "bitrev_y", "shift_x", "shift_y",
           "other_coord_x", "other_coord_y", "omega_sign", "conjugate")


def applicable(mutant, shape, time_scale):
    n = shape[1] if mutant.endswith("_y") else shape[0]
    if mutant.startswith("bitrev"):
        return n & (n - 1) == 0  # the digit reversal of the hand-written transforms; the rocFFT sizes have none
    if mutant.startswith("other_coord"):
        return shape[0] != shape[1]  # the two meshes of a square grid are equal
    if mutant == "conjugate":
        return complex(time_scale).real != 0.0  # in pure imaginary time the multiplier is real
    return True


def _bit_reversed(n):
    bits = n.bit_length() - 1
    return np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])


def exchanged_bins(n):
    """the pairs of upper bins the exchange mutants swap, two bins apart: (n/2 - 3, n/2 - 5), then every four bins down,
    one pair per 128 points -- a bin of white noise holds 1 / n of a line's weight, so one pair alone moves a 1024-point
    line by 5.6e-5 in one step, under 10 x its fp32 gate"""
    return [(n // 2 - 3 - 4 * q, n // 2 - 5 - 4 * q) for q in range(max(1, n // 128))]


def _mutate(case, dom, p, mutant):
    """rebuild the line operators of ``case`` (Ax, Ay; for a StirCase the meshes its ``half_ops_at`` builds them from) with
    one fault; the potential and the lights keep the true meshes"""
    nx, ny = dom.points
    x, y = dom.mesh()
    kx, ky = dom.fft_mesh()
    ikx, iky = 2j * np.pi * kx, 2j * np.pi * ky
    y_of_ax, x_of_ay = y, x  # the line coordinates of the two operators
    sign = 1.0
    kind, _, axis = mutant.rpartition("_")
    if mutant == "omega_sign":
        sign = -1.0
    elif mutant == "conjugate":
        for name in ("half_ops", "half_ops_at"):
            if hasattr(case, name):
                setattr(case, name, lambda *a, _f=getattr(case, name): tuple(np.conj(m) for m in _f(*a)))
        return
    elif kind == "nyquist":  # fftfreq has -N/2 there; the kinetic part is even and does not see it
        if axis == "x":
            ikx = ikx.copy()
            ikx[nx // 2, :] *= -1
        else:
            iky = iky.copy()
            iky[:, ny // 2] *= -1
    elif kind in ("exchange", "bitrev"):
        n = nx if axis == "x" else ny
        perm = np.arange(n)
        if kind == "exchange":
            for a, b in exchanged_bins(n):
                perm[[a, b]] = perm[[b, a]]
        else:
            perm = _bit_reversed(n)
        if axis == "x":
            ikx = ikx[perm, :]
        else:
            iky = iky[:, perm]
    elif kind == "shift":
        if axis == "x":
            y_of_ax = np.roll(y, 1, axis=1)
        else:
            x_of_ay = np.roll(x, 1, axis=0)
    elif kind == "other_coord":  # first coordinate and spacing of the other axis (the spacings are equal here)
        ax_x, ax_y = dom.axes()
        if axis == "x":
            y_of_ax = np.broadcast_to(ax_x[0] + dom.dx[0] * np.arange(ny), (nx, ny))
        else:
            x_of_ay = np.broadcast_to((ax_y[0] + dom.dx[1] * np.arange(nx))[:, None], (nx, ny))
    else:
        raise ValueError(mutant)
    om = sign * p["omega"]
    case.Ax = (0.5j * ikx**2 - om * y_of_ax * ikx).astype(case.c)
    case.Ay = (0.5j * iky**2 + om * x_of_ay * iky).astype(case.c)
    case._half = {}
    if isinstance(case, S.StirCase):
        if case.lights is not None:
            case.lights = lambda t, X, Y, _f=case.lights: _f(t, x, y)
        case.omega, case.omega_rate = sign * case.omega, sign * case.omega_rate
        case.ikx, case.iky, case.y, case.x = ikx, iky, y_of_ax, x_of_ay
