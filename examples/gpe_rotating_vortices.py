"""Vortices in a rotating trap: imaginary time (``time_scale=-1j``) of the rotating-frame GPE (``GPE2DTSRot`` +
``RotatingStrangSplitting``, the alternating-direction split step of DESIGN.md section 4.10) from a seeded, noisy
Thomas-Fermi profile at 128^2 with one imprinted phase singularity, then the vortex census on the device.  Above the critical rotation the ground state
carries vortices; the relaxation lets them in from the edge of the cloud.  Runs in a few seconds."""
import time

import numpy as np

import pde_opt_amd as P

N, BOX = 128, 8.0
K, E, OMEGA = 100.0, 0.0, 0.9
DT, STEPS, SEED = 2e-3, 400, 0
AMP_THRESH = 1e-3  # plaquettes whose |psi| is below this are not counted (a core itself is a zero of psi)

dom = P.Domain((N, N), ((-BOX, BOX), (-BOX, BOX)), "dimensionless")


def initial_state():
    """Thomas-Fermi profile of the non-rotating trap, sqrt(max(mu - V, 0) / k), times seeded complex noise"""
    x, y = dom.mesh()
    v = 0.5 * ((1 + E) * x**2 + (1 - E) * y**2)
    mu = np.sqrt(K / np.pi)  # 2-D harmonic trap: the profile integrates to one
    rng = np.random.default_rng(SEED)
    psi = np.sqrt(np.maximum(mu - v, 0.0) / K) + 0.02 * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))
    psi = psi * (1 + 0.1 * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)))
    # relaxation from a vortex-free state sits on the symmetric saddle for a long time: imprint one off-centre phase
    # singularity, which the rotating trap pulls in and keeps
    psi = psi * np.exp(1j * np.angle((x - 1.3) + 1j * (y + 0.4)))
    psi /= np.sqrt(np.sum(np.abs(psi) ** 2) * dom.dx[0] ** 2)
    return np.stack([psi.real, psi.imag], axis=-1).astype(np.float32)


def main():
    model = P.PDEModel(P.GPE2DTSRot, dom, P.RotatingStrangSplitting)
    t0 = time.perf_counter()
    ys = model.solve(dict(k=K, e=E, omega=OMEGA), initial_state(), [0.0, STEPS * DT], {"time_scale": -1j}, dt0=DT)
    el = time.perf_counter() - t0
    eng = model._engine  # the final state is still resident: count on the device
    counts, _ = eng.detect_vortices(AMP_THRESH, 0.5, want_winding=False)
    state = ys[-1]
    norm = float(np.sum(state.astype(np.float64) ** 2) * dom.dx[0] ** 2)
    print(f"{STEPS} imaginary-time steps of {N}^2 at Omega = {OMEGA} in {el:.2f} s ({eng.last_kernel}); norm {norm:.6f}; "
          f"vortices {int(counts[0, 0])}, total charge {int(counts[0, 1])}")
    # the step renormalises BETWEEN its half steps (as StrangSplitting does); in imaginary time the two line operators
    # after that are not unitary, so the norm at a step's end is 1 + O(dt): 1.00086 here, on the device and in numpy
    assert np.isfinite(state).all() and abs(norm - 1.0) < 5e-3
    return state, int(counts[0, 0])


if __name__ == "__main__":
    main()
    print("ok")
