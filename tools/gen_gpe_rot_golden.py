"""Generate tests/golden/gpe_rot_terms.npz: ``A_terms`` / ``B_terms`` of the reference's ``GPE2DTSRot`` on a 16 x 12
domain (arrays only).  The reference's files are loaded by path under the stub recipe of SURVEY.md Appendix B (jax.numpy
-> numpy); nothing of theirs is copied.  No-op where the reference tree is absent.

Run:  python tools/gen_gpe_rot_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = os.environ.get("PDE_OPT_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "gpe_rot_terms.npz")

POINTS, BOX = (16, 12), ((-4.0, 4.0), (-3.0, 3.0))
K, E, OMEGA, SEED = 37.5, 0.15, 0.7, 11


def _shell(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _load(name, relpath):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def main():
    if not os.path.isdir(REF):
        print("reference tree absent; nothing to do")
        return
    _shell("jax", numpy=np, jit=lambda f, **k: f, Array=np.ndarray)
    sys.modules["jax.numpy"] = np
    for pkg in ("pde_opt", "pde_opt.numerics", "pde_opt.numerics.equations"):
        _shell(pkg)
    _shell("pde_opt.numerics.shapes", Shape=object)
    dom = _load("pde_opt.numerics.domains", "pde_opt/numerics/domains.py")
    _load("pde_opt.numerics.equations.base_eq", "pde_opt/numerics/equations/base_eq.py")
    gp = _load("pde_opt.numerics.equations.gross_pitaevskii", "pde_opt/numerics/equations/gross_pitaevskii.py")
    # the reference class leaves the abstract ``rhs`` open (it cannot be instantiated as written): close it in a subclass
    rot = type("GPE2DTSRot", (gp.GPE2DTSRot,), {"rhs": lambda self, state, t: self.B_terms(state, t)})
    eq = rot(dom.Domain(POINTS, BOX, "dimensionless"), K, E, OMEGA)
    rng = np.random.default_rng(SEED)
    state = rng.standard_normal(POINTS) + 1j * rng.standard_normal(POINTS)
    ax, ay = eq.A_terms(None, 0.0)
    np.savez_compressed(OUT, points=np.array(POINTS), box=np.array(BOX), k=K, e=E, omega=OMEGA, state=state,
             A_x=np.asarray(ax), A_y=np.asarray(ay), B=np.asarray(eq.B_terms(state, 0.0)),
             **{n: np.asarray(getattr(eq, n)) for n in ("kx", "ky", "two_pi_i_kx", "two_pi_i_ky", "two_pi_i_kx_2",
                                                        "two_pi_i_ky_2", "two_pi_i_k_2", "xmesh", "ymesh")})
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
