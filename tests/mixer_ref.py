"""A numpy restatement of the reference's Mixer2d (pde_opt/numerics/functions/mixer_mlp.py:13-86), written from its
definition and independent of torch: one field (H, W) in, one out, parameters taken from the flat vector in the order
pde_opt_amd/numerics/functions/mixer.py documents."""
import numpy as np

EPS = 1e-5

ACTS = {
    "relu": lambda z: np.maximum(z, 0.0),
    "tanh": np.tanh,
    "gelu_tanh": lambda z: 0.5 * z * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (z + 0.044715 * z**3))),
}


def split(flat, grid, p, C, mp, mh, blocks):
    """the flat vector as a dict of arrays"""
    P = (grid[0] // p) * (grid[1] // p)
    o = 0

    def take(*shape):
        nonlocal o
        n = int(np.prod(shape))
        a = np.asarray(flat[o:o + n], dtype=np.float64).reshape(shape)
        o += n
        return a

    out = {"win": take(C, p, p), "bin": take(C), "wout": take(C, p, p), "bout": take(1), "blocks": []}
    for _ in range(blocks):
        out["blocks"].append({"w1": take(mp, P), "b1": take(mp), "w2": take(P, mp), "b2": take(P),
                              "w3": take(mh, C), "b3": take(mh), "w4": take(C, mh), "b4": take(C),
                              "g1": take(C, P), "be1": take(C, P), "g2": take(P, C), "be2": take(P, C)})
    out["gf"], out["bef"] = take(C, P), take(C, P)
    assert o == len(flat), (o, len(flat))
    return out


def layer_norm(y, g, b):
    """over the whole array: one mean, one biased variance"""
    return (y - y.mean()) / np.sqrt(y.var() + EPS) * g + b


def forward(flat, u, p, C, mp, mh, blocks, act="relu"):
    H, W = u.shape
    h, w = H // p, W // p
    q = split(flat, (H, W), p, C, mp, mh, blocks)
    f = ACTS[act]
    y = np.zeros((C, h * w))
    for i in range(h):
        for j in range(w):
            patch = u[i * p:(i + 1) * p, j * p:(j + 1) * p]
            y[:, i * w + j] = (q["win"] * patch).sum(axis=(1, 2)) + q["bin"]
    for b in q["blocks"]:
        n = layer_norm(y, b["g1"], b["be1"])
        y = y + f(n @ b["w1"].T + b["b1"]) @ b["w2"].T + b["b2"]      # every channel row: P -> mp -> P
        y = y.T
        n = layer_norm(y, b["g2"], b["be2"])
        y = y + f(n @ b["w3"].T + b["b3"]) @ b["w4"].T + b["b4"]      # every patch row: C -> mh -> C
        y = y.T
    y = layer_norm(y, q["gf"], q["bef"])
    out = np.zeros((H, W))
    for i in range(h):
        for j in range(w):
            out[i * p:(i + 1) * p, j * p:(j + 1) * p] = np.tensordot(y[:, i * w + j], q["wout"], axes=(0, 0)) + q["bout"][0]
    return out
