"""Times of the WoE scorecard fit (models/scorecard.py, csrc/scorecard.hip) on one GPU at ``--rows`` x 20 synthetic
LendingClub-shaped rows: one Newton pass and the whole Newton fit through the kernel path, against a torch
composition on the same device in the same run (gather the fp64 WoE matrix ``Z [N, F + 1]``, ``Z.T @ (s[:, None]
* Z)`` and the residual product), the two alternating; also the encode and score kernels and the whole
``Scorecard.fit``. The composition is timed twice: gathering ``Z`` in every pass, and with ``Z`` kept (1.7 GB at
10M rows). Every figure is (median, min, max) in ms of ``torch.cuda.Event`` pairs around warmed calls that end in
a synchronise. One JSON line on stdout.

    python scripts/bench_scorecard.py [--rows 10000000] [--out scorecard_perf.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch

from cobalt_smart_lender_ai_amd.dataio import synth
from cobalt_smart_lender_ai_amd.models import scorecard as S
from cobalt_smart_lender_ai_amd.ops import scorecard_ops as ops

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_scorecard.py measures on a GPU; none is visible")
N = args.rows
dev = torch.device("cuda:0")
X, y = synth.make_lendingclub(N, seed=0, device=dev)
F = X.shape[1]
P = F + 1


def timed(fns, reps=args.repeats, warm=2):
    """(median, min, max) ms per function; the functions alternate inside every repeat."""
    for _ in range(warm):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


res = {"rows": N, "features": F}
t0 = time.perf_counter()
sc = S.Scorecard().fit(X, y, feature_names=list(synth.FEATURES))
torch.cuda.synchronize()
res["fit_first_call_s"] = time.perf_counter() - t0
res["fit_passes"] = sc.fit_info["passes"]
res["kept"] = sc.n_kept
res["cells"] = int(sc.cell_ptr[-1])

codes = ops.scorecard_encode(X, sc.edges)
tab = np.concatenate(sc.woe)
kernel_pass = ops.newton_pass(codes, sc.cell_ptr, tab, y, None)
tab_d = torch.from_numpy(tab).to(dev)
ptr_d = torch.from_numpy(sc.cell_ptr[:-1].copy()).to(dev)
pos = y > 0.5
ones = torch.ones((N, 1), dtype=torch.float64, device=dev)


def gather():
    return torch.cat([ones, tab_d[codes.to(torch.int64) + ptr_d]], dim=1)


def compose(Z, beta_d):
    eta = Z @ beta_d
    e = torch.exp(-eta.abs())
    inv = 1.0 / (1.0 + e)
    big, small = inv, e * inv
    p = torch.where(eta >= 0, big, small)
    q = torch.where(eta >= 0, small, big)
    r = torch.where(pos, -q, p)
    loss = (torch.log1p(e) + eta.clamp_min(0.0) - torch.where(pos, eta, torch.zeros_like(eta))).sum()
    return torch.cat([loss.reshape(1), Z.T @ r, (Z.T @ ((p * q)[:, None] * Z)).reshape(-1)])


def composition_pass(Z=None):
    def run(beta):
        o = compose(gather() if Z is None else Z, torch.from_numpy(np.asarray(beta, dtype=np.float64)).to(dev))
        o = o.cpu().numpy()
        return float(o[0]), o[1:1 + P].copy(), o[1 + P:].reshape(P, P).copy()
    return run


Zkept = gather()
beta = sc.beta
k_out = kernel_pass(beta)
c_out = composition_pass(Zkept)(beta)
res["hess_max_rel_diff"] = float(np.max(np.abs(k_out[2] - c_out[2])) / np.max(np.abs(c_out[2])))
res["grad_max_abs_diff"] = float(np.max(np.abs(k_out[1] - c_out[1])))

names = ["pass_kernel_ms", "pass_composition_gather_ms", "pass_composition_kept_ms"]
for n, t in zip(names, timed([lambda: kernel_pass(beta), lambda: composition_pass()(beta),
                              lambda: composition_pass(Zkept)(beta)])):
    res[n] = t
keep = [0] + [f + 1 for f in range(F) if not sc.dropped[f]]
info = {}


def fit_with(newton, key):
    def run():
        info[key] = S.fit_newton(newton, P, keep, float(N))[1]["passes"]
    return run


for n, t in zip(["fit_kernel_ms", "fit_composition_gather_ms", "fit_composition_kept_ms"],
                timed([fit_with(kernel_pass, "k"), fit_with(composition_pass(), "g"),
                       fit_with(composition_pass(Zkept), "z")], reps=3, warm=1)):
    res[n] = t
res["fit_passes_by_path"] = info
del Zkept
res["encode_ms"], res["score_top4_ms"] = timed([
    lambda: ops.scorecard_encode(X, sc.edges),
    lambda: ops.scorecard_score(X, sc.edges, float(sc.beta[0]), sc.contrib, np.concatenate(sc.int_points),
                                sc.shortfall, 4)])
# the whole fit once more, warm: the fine edges are quantiles taken on the host, which is most of it
t0 = time.perf_counter()
S.Scorecard().fit(X, y)
torch.cuda.synchronize()
res["fit_second_call_s"] = time.perf_counter() - t0
# bytes a pass reads per row, from the shapes: the kernel reads the codes and the label (weights: + 8); the
# composition reads Z for eta, reads it and writes s Z, reads both in the GEMM and Z again for the gradient,
# and with the gather also reads the codes, writes their int64 indices, reads them and writes Z
res["bytes_per_row"] = {"kernel": F + 4, "composition_kept": 6 * 8 * P,
                        "composition_gather": 6 * 8 * P + F + 2 * 8 * F + 2 * 8 * P}
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
