"""The rotating-frame GPE without a GPU: the class surface of ``GPE2DTSRot`` against the reference's recorded outputs,
the numpy reference of the alternating-direction split step (tests/gpe_rot_ref.py) against the oracle's Strang step at
Omega = 0 and against an analytic eigenstate, the refusals, and the new ABI symbols."""
import os
import re

import numpy as np
import pytest

import pde_opt_amd as P
from pde_opt_amd import _lib as L
from oracle import np_oracle as O

import gpe_rot_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "gpe_rot_terms.npz"))


def gold_equation():
    dom = P.Domain(tuple(int(v) for v in GOLD["points"]), tuple(tuple(float(v) for v in b) for b in GOLD["box"]), "dimensionless")
    return P.GPE2DTSRot(dom, float(GOLD["k"]), float(GOLD["e"]), float(GOLD["omega"]))


# ---- class surface and golden ------------------------------------------------------------------------------------------

def test_exported_where_the_reference_exports_it():
    import pde_opt_amd.numerics as N
    import pde_opt_amd.numerics.equations as E

    assert P.GPE2DTSRot is N.GPE2DTSRot is E.GPE2DTSRot
    assert P.RotatingStrangSplitting is N.RotatingStrangSplitting


@pytest.mark.parametrize("name", ["kx", "ky", "two_pi_i_kx", "two_pi_i_ky", "two_pi_i_kx_2", "two_pi_i_ky_2", "two_pi_i_k_2",
                                  "xmesh", "ymesh"])
def test_published_attributes_equal_the_reference_class(name):
    np.testing.assert_allclose(getattr(gold_equation(), name), GOLD[name], rtol=1e-15, atol=0)


def test_a_terms_and_b_terms_equal_the_reference_class():
    eq = gold_equation()
    ax, ay = eq.A_terms(None, 0.0)
    np.testing.assert_allclose(ax, GOLD["A_x"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(ay, GOLD["A_y"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(eq.B_terms(GOLD["state"], 0.0), GOLD["B"], rtol=1e-14, atol=0)
    assert eq.fft is np.fft.fftn and eq.ifft is np.fft.ifftn
    assert eq.dx == eq.domain.dx[0] and eq._state_trailing == (2,)


# ---- the numpy reference ------------------------------------------------------------------------------------------------

def test_omega_zero_is_the_oracles_strang_step_with_the_kinetic_a_term():
    dom = P.Domain((32, 32), ((-5.0, 5.0), (-5.0, 5.0)), "dimensionless")
    k, e = 50.0, 0.1
    psi = R.smooth_state(dom, 3)[0]
    x, y = dom.mesh()
    kx, ky = dom.fft_mesh()
    a_term = 0.5j * ((2j * np.pi * kx) ** 2 + (2j * np.pi * ky) ** 2)
    b_terms = lambda t, s: O.gpe_b_terms(s, x, y, k, e, 1.0, 0.0)
    for ts in (1.0, -1j, 0.3 - 1j):
        case = R.RotCase(dom, k, e, 0.0, ts)
        got, want = psi, R.to_pairs(psi)
        for _ in range(3):
            got = case.step(got, 0.01)
            want = O.strang_step(b_terms, 0.0, want, 0.01, a_term, dom.dx[0], ts)
        err = np.max(np.abs(got - R.from_pairs(want))) / np.max(np.abs(want))
        assert err <= 1e-13, (ts, err)


@pytest.mark.parametrize("omega", [0.6, -0.4])
def test_analytic_eigenstate_second_order(omega):
    """psi ~ (x + i y) exp(-r^2 / 2) has energy 2 and L_z = 1: after T it is psi exp(-i (2 - Omega) T)"""
    dom = P.Domain((64, 64), ((-8.0, 8.0), (-8.0, 8.0)), "dimensionless")
    x, y = dom.mesh()
    psi0 = (x + 1j * y) * np.exp(-(x**2 + y**2) / 2)
    psi0 /= np.sqrt(np.sum(np.abs(psi0) ** 2) * dom.dx[0] ** 2)
    T = 0.5
    exact = psi0 * np.exp(-1j * (2 - omega) * T)
    case = R.RotCase(dom, 0.0, 0.0, omega)
    errs = []
    for dt in (1e-2, 5e-3):
        got = case.advance(psi0, dt, int(round(T / dt)))
        errs.append(np.max(np.abs(got - exact)) / np.max(np.abs(exact)))
    print(f"omega {omega}: errors {errs[0]:.3e} {errs[1]:.3e} ratio {errs[0] / errs[1]:.3f}")
    assert errs[0] <= 5e-5
    assert 3.5 <= errs[0] / errs[1] <= 4.5


# ---- refusals -----------------------------------------------------------------------------------------------------------

DOM = P.Domain((16, 16), ((-2.0, 2.0), (-2.0, 2.0)), "dimensionless")


def test_strang_splitting_on_the_rotating_equation_names_the_solver():
    with pytest.raises(ValueError, match="RotatingStrangSplitting"):
        P.PDEModel(P.GPE2DTSRot, DOM, P.StrangSplitting)


def test_rotating_solver_on_the_control_equation_names_the_solver():
    with pytest.raises(ValueError, match="StrangSplitting"):
        P.PDEModel(P.GPE2DTSControl, DOM, P.RotatingStrangSplitting)
    with pytest.raises(ValueError, match="GPE2DTSRot"):
        P.PDEModel(P.CahnHilliard2DPeriodic, DOM, P.RotatingStrangSplitting)


def test_the_matching_pair_is_accepted():
    from pde_opt_amd.utils import check_equation_solver_compatibility, prepare_solver_params

    check_equation_solver_compatibility(P.RotatingStrangSplitting, P.GPE2DTSRot)
    assert P.RotatingStrangSplitting.required_equation_attrs == ["A_terms", "dx"]
    eq = P.GPE2DTSRot(DOM, 1.0, 0.0, 0.3)
    s = P.RotatingStrangSplitting(**prepare_solver_params(P.RotatingStrangSplitting, {"time_scale": -1j}, eq))
    assert s.dx == eq.dx and s.time_scale == -1j and s.integrator == L.INT_STRANG_ROT
    assert P.RotatingStrangSplitting(0.25).time_scale == 1.0


def test_gradients_of_the_rotating_equation_are_refused():
    m = P.PDEModel(P.GPE2DTSRot, DOM, P.RotatingStrangSplitting)
    y0 = np.zeros((16, 16, 2))
    params = dict(k=1.0, e=0.0, omega=0.3)
    with pytest.raises(NotImplementedError, match="rotating"):
        m.control_gradient(lambda ys: ys.sum(), y0, [0.0, 0.1], params)
    with pytest.raises(NotImplementedError, match="rotating"):
        m.optimize(lambda ys: ys.sum(), y0, [0.0, 0.1], {"omega": 0.3}, {"k": 1.0, "e": 0.0})
    with pytest.raises(NotImplementedError, match="rotating"):
        m.train({"ys": [y0, y0], "ts": [0.0, 0.1]}, [[0, 1]], {"omega": 0.3}, {"k": 1.0, "e": 0.0}, {}, {}, 0.0)


# ---- ABI ----------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(os.path.dirname(HERE), "include", "pdeopt_hip.h")).read()
    assert re.search(r"PDEOPT_INT_STRANG_ROT\s*=\s*5\b", header) and L.INT_STRANG_ROT == 5
    for name, nargs in (("pdeopt_set_gpe_rotation", 4), ("pdeopt_set_env_gpe_omega", 4)):
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl and len(decl.group(1).split(",")) == nargs
        assert name in L._SIGNATURES and len(L._SIGNATURES[name][1]) == nargs
    # Omega travels by its own call: pdeopt_problem (whose size tests/test_abi.py pins) has no field for it
    assert not any(n for n, _ in L.Problem._fields_ if "omega" in n)


def test_both_gpe_classes_share_a_grid():
    """the two classes cache their meshes in one per-grid table: either order of construction works"""
    for first, second in ((0, 1), (1, 0)):
        dom = P.Domain((8, 10 + first), ((-1.0, 1.0), (-1.0, 1.0)), "dimensionless")
        make = [lambda: P.GPE2DTSRot(dom, 1.0, 0.0, 0.3), lambda: P.GPE2DTSControl(dom, 1.0, 0.0, lambda t, x, y: 0.0 * x, kinetic=True)]
        a, b = make[first](), make[second]()
        assert np.array_equal(a.xmesh, b.xmesh) and np.array_equal(a.ymesh, b.ymesh)
