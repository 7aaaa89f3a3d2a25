"""Times of the portfolio loss simulation (portfolio/, csrc/portfolio.hip) on one GPU: ``simulate_losses`` end to
end on ``--loans`` x ``--scenarios`` with one sector and ``--segments`` segments (host preparation, upload, the
kernels, the report), ``portfolio_sums_gpu`` alone on device-resident prepared inputs, and for scale the NumPy
host path ``portfolio_sums_host`` at ``--host-loans`` x ``--host-scenarios`` on the same machine. GPU figures are
(median, min, max) in ms of a host clock around warmed calls that end in a synchronise; draws per second are
loans x scenarios over the median. The device sums are compared with the host's on the host-sized slice, and the
full run's expected loss is printed next to ``sum PD L`` and its standard error. One JSON line on stdout.

    python scripts/bench_portfolio.py [--loans 1000000] [--scenarios 10000] [--segments 8] [--out pf_perf.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch

from cobalt_smart_lender_ai_amd import portfolio
from cobalt_smart_lender_ai_amd.ops import portfolio_ops
from cobalt_smart_lender_ai_amd.portfolio import loss as P

ap = argparse.ArgumentParser()
ap.add_argument("--loans", type=int, default=1_000_000)
ap.add_argument("--scenarios", type=int, default=10_000)
ap.add_argument("--segments", type=int, default=8)
ap.add_argument("--host-loans", type=int, default=20_000)
ap.add_argument("--host-scenarios", type=int, default=1_000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_portfolio.py measures on a GPU; none is visible")
n, S, G = args.loans, args.scenarios, args.segments
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
pd = np.clip(rng.beta(1.2, 14.0, size=n), 1e-4, 0.9)
ead = np.round(rng.lognormal(9.3, 0.7, size=n), 2)
seg = rng.integers(0, G, size=n)
rho, lgd, seed = 0.15, 0.6, 7


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


res = {"loans": n, "scenarios": S, "segments": G, "sectors": 1, "draws": float(n) * S}
pd_d, ead_d, seg_d = (torch.from_numpy(v).to(dev) for v in (pd, ead, seg))
res["simulate_losses_ms"] = timed(lambda: portfolio.simulate_losses(pd_d, ead_d, lgd, rho=rho, segment=seg_d,
                                                                    n_scenarios=S, seed=seed))
res["simulate_losses_draws_per_s"] = res["draws"] / (res["simulate_losses_ms"][0] * 1e-3)
rep = portfolio.simulate_losses(pd_d, ead_d, lgd, rho=rho, segment=seg_d, n_scenarios=S, seed=seed)
res["expected_loss"], res["expected_loss_analytic"] = rep.expected_loss, rep.expected_loss_analytic
res["expected_loss_standard_error"] = rep.std / S ** 0.5
res["var_es_asrf_0.999"] = [rep.var["0.999"], rep.es["0.999"], rep.asrf_var["0.999"]]
Q, L = P.probit_points(pd, rho), P.loss_amounts(ead, lgd)
A = P.scenario_offsets(rho, S, seed)
idx = np.arange(n, dtype=np.int64)
dargs = [torch.from_numpy(v).to(dev) for v in (idx, Q, L.astype(np.int64), np.zeros(n, dtype=np.int64), A)]
table = torch.from_numpy(np.array(P.threshold_table())).to(dev)
res["portfolio_sums_gpu_ms"] = timed(lambda: portfolio_ops.portfolio_sums_gpu(*dargs, seed, segment=seg_d,
                                                                              n_segments=G, table=table))
res["portfolio_sums_gpu_draws_per_s"] = res["draws"] / (res["portfolio_sums_gpu_ms"][0] * 1e-3)
hn, hs = min(args.host_loans, n), min(args.host_scenarios, S)
t0 = time.perf_counter()
want = P.portfolio_sums_host(idx[:hn], Q[:hn], L[:hn], None, A[:hs], seed, segment=seg[:hn], n_segments=G)
res["host_s"] = time.perf_counter() - t0
res["host_loans"], res["host_scenarios"] = hn, hs
res["host_draws_per_s"] = float(hn) * hs / res["host_s"]
got = portfolio_ops.portfolio_sums_gpu(*(t[:hn] for t in dargs[:4]), dargs[4][:hs], seed, segment=seg_d[:hn],
                                       n_segments=G, table=table)
res["equal_to_host"] = bool(np.array_equal(got.cpu().numpy(), want))
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
