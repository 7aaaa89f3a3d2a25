"""Times of the fair-lending sums (fairness/, csrc/fairness.hip) on one GPU at ``--rows`` x ``--reps`` with
``--groups`` groups and labels, for 1 and 16 cutoffs: ``fairness_sums_gpu`` on device-resident inputs (packing the
records, the kernels), the two kernels alone on packed records (``cobalt_fairness`` with the whole run in one
call), ``fair_lending_audit`` end to end with one cutoff (sums, per-group AUC, the report), and for scale the NumPy
host path ``fairness_sums_host`` at ``--host-rows`` x ``--host-reps`` on the same machine. GPU figures are (median,
min, max) in ms of a host clock around warmed calls that end in a synchronise; draws per second are rows x
replicates over the median. The device sums are compared with the host's on the host-sized slice. One JSON line
on stdout.

    python scripts/bench_fairness.py [--rows 1000000] [--reps 2000] [--groups 8] [--out fair_perf.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch

from cobalt_smart_lender_ai_amd import _native, fairness
from cobalt_smart_lender_ai_amd.fairness import sums as S
from cobalt_smart_lender_ai_amd.ops import fairness_ops

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=2000)
ap.add_argument("--groups", type=int, default=8)
ap.add_argument("--host-rows", type=int, default=20_000)
ap.add_argument("--host-reps", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_fairness.py measures on a GPU; none is visible")
n, R, G = args.rows, args.reps, args.groups
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
group = rng.integers(0, G, size=n)
score = np.clip(rng.beta(2.0, 5.0, size=n) + 0.02 * (group % 3), 0.0, 1.0).astype(np.float32)
y = (rng.random(n) < score).astype(np.int64)
seed = 7
cuts = {1: [0.5], 16: [float(c) for c in np.linspace(0.05, 0.8, 16)]}


def timed(fn, reps=args.repeats, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


res = {"rows": n, "reps": R, "groups": G, "draws": float(n) * R}
s_d, g_d, y_d = (torch.from_numpy(v).to(dev) for v in (score, group, y))
idx_d = torch.arange(n, device=dev)
lib, tile = _native.lib(), fairness_ops.fairness_tile_rows()
for K, cut in cuts.items():
    res[f"fairness_sums_gpu_ms_k{K}"] = timed(lambda: fairness_ops.fairness_sums_gpu(s_d, g_d, y_d, cut, R, seed,
                                                                                      n_groups=G))
    res[f"fairness_sums_gpu_draws_per_s_k{K}"] = res["draws"] / (res[f"fairness_sums_gpu_ms_k{K}"][0] * 1e-3)
    recs, tile_group = fairness_ops.pack_rows(idx_d, s_d, y_d, torch.from_numpy(S.check_cutoffs(cut)).to(dev), g_d, G,
                                              tile)
    total = int(recs.shape[0])
    need = fairness_ops.fairness_workspace_bytes(total, R, K)
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.zeros((4 + 2 * K, G, R), dtype=torch.int64, device=dev)

    def kernels():
        rc = lib.cobalt_fairness(recs.data_ptr(), total, K, tile_group.data_ptr(), G, 0, R, seed, 1, work.data_ptr(),
                                 need, out.data_ptr(), R, _native.stream_handle())
        assert rc == 0

    res[f"kernels_ms_k{K}"] = timed(kernels)
    res[f"kernels_draws_per_s_k{K}"] = res["draws"] / (res[f"kernels_ms_k{K}"][0] * 1e-3)
    res[f"workspace_mib_k{K}"] = need / 2 ** 20
    hn, hr = min(args.host_rows, n), min(args.host_reps, R)
    t0 = time.perf_counter()
    want = S.fairness_sums_host(score[:hn], group[:hn], y[:hn], cut, seed, hr, n_groups=G)
    res[f"host_s_k{K}"] = time.perf_counter() - t0
    res[f"host_draws_per_s_k{K}"] = float(hn) * hr / res[f"host_s_k{K}"]
    got = fairness_ops.fairness_sums_gpu(s_d[:hn], g_d[:hn], y_d[:hn], cut, hr, seed, n_groups=G)
    res[f"equal_to_host_k{K}"] = bool(np.array_equal(got.cpu().numpy(), want))
    del work, out, recs
res["host_rows"], res["host_reps"] = min(args.host_rows, n), min(args.host_reps, R)
res["fair_lending_audit_ms"] = timed(lambda: fairness.fair_lending_audit(s_d, g_d, y_d, n_boot=R, seed=seed),
                                     reps=max(1, args.repeats // 2))
rep = fairness.fair_lending_audit(s_d, g_d, y_d, n_boot=R, seed=seed)
res["air"] = {k: [v["air"].point, v["air"].low, v["air"].high, v.verdict] for k, v in rep["group"].groups.items()}
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
