"""What the coefficient gradient of D costs in PDEModel.mse_backward: a 128 x 128 grid, B = 3, 200 IMEX substeps, the
notebook's PeriodicCNN(1, (32, 64, 64), 1) with native_cnn on, timed with closure_grads and without on the same build.

    python tools/fieldmu_joint_bench.py [--out profiles/fieldmu_joint.json] [--repeats 7] [--warmup 2]

Each timing is host wall time of one whole call (it ends with a host read of the loss, so the device is idle when the clock
stops); the two variants alternate, so drift hits both; median, minimum and maximum over the repeats are reported."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import pde_opt_amd as P
from pde_opt_amd.numerics.functions.cnn import PeriodicCNN
from pde_opt_amd.numerics.functions.legendre import DiffusionLegendrePolynomials

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--grid", type=int, default=128)
ap.add_argument("--substeps", type=int, default=200)
args = ap.parse_args()

N, B = args.grid, 3
dom = P.Domain((N, N), ((0.0, 0.01 * N), (0.0, 0.01 * N)), "dimensionless")
model = P.PDEModel(P.CahnHilliard2DPeriodic, dom, P.SemiImplicitFourierSpectral)
model.fieldmu_solver().native_cnn = True
rng = np.random.default_rng(0)
y0s = np.clip(0.5 + 0.05 * rng.standard_normal((B, N, N)), 0.05, 0.95)
values = np.clip(y0s[:, None] + 0.01 * rng.standard_normal((B, 1, N, N)), 0.05, 0.95)
ts = np.array([0.0, args.substeps * 1e-6])
torch.manual_seed(0)
cnn = PeriodicCNN(1, (32, 64, 64), 1).double().to("cuda")
with torch.no_grad():
    for p in cnn.parameters():
        p.mul_(0.3)
params = {"kappa": 0.002, "mu": cnn, "D": DiffusionLegendrePolynomials(np.array([-0.3, 0.2]))}


def once(joint):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.mse_backward(params, (y0s, values), {"A": 0.5}, ts, {}, 0.0, closure_grads={} if joint else None)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


for _ in range(args.warmup):
    once(False), once(True)
t = {False: [], True: []}
for _ in range(args.repeats):
    for joint in (False, True):
        t[joint].append(once(joint))
stat = lambda v: {"median_s": statistics.median(v), "min_s": min(v), "max_s": max(v), "all_s": v}
res = {"grid": [N, N], "batch": B, "substeps": args.substeps, "network": "PeriodicCNN(1, (32, 64, 64), 1), native_cnn, fp64",
       "repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
       "mse_backward": stat(t[False]), "mse_backward_closure_grads": stat(t[True]),
       "ratio_of_medians": statistics.median(t[True]) / statistics.median(t[False])}
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
