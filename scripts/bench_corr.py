"""Times of the correlation matrix (select/collinearity.py, csrc/corr.hip) on one GPU: one Pearson
``correlation_matrix`` on a device-resident ``--rows`` x ``--features`` float32 matrix with the tree dataset's
missing pattern (the 20 synthetic LendingClub-shaped columns, repeated with noise up to the width), the moments
kernel and the column-sum kernel alone, and for scale ``pandas.DataFrame.corr()`` on the same frame on the host.
GPU figures are (median, min, max) in ms of ``torch.cuda.Event`` pairs around warmed calls that end in a
synchronise; the read rate is the matrix's bytes over the kernel's time. One JSON line on stdout.

    python scripts/bench_corr.py [--rows 2320000] [--features 106] [--pandas-rows 2320000] [--out corr_perf.json]
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
from cobalt_smart_lender_ai_amd.ops import corr_ops as ops
from cobalt_smart_lender_ai_amd.select import correlation_matrix

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=2_320_000)
ap.add_argument("--features", type=int, default=106)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--pandas-rows", type=int, default=None, help="rows of the pandas run (default: all; 0 skips it)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_corr.py measures on a GPU; none is visible")
N, F = args.rows, args.features
dev = torch.device("cuda:0")
X20, _ = synth.make_lendingclub(N, seed=0, device=dev)
g = torch.Generator(device=dev).manual_seed(1)
X = torch.empty((N, F), dtype=torch.float32, device=dev)
for f in range(F):  # copy k of a column: the column plus k tenths of its spread in noise (NaN stays NaN)
    src = X20[:, f % X20.shape[1]].to(torch.float32)
    k = f // X20.shape[1]
    sd = float(torch.nan_to_num(src).std())
    X[:, f] = src + 0.1 * k * sd * torch.randn(N, device=dev, generator=g) if k else src
del X20


def timed(fn, reps=args.repeats, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


res = {"rows": N, "features": F, "missing_share": float(torch.isnan(X).float().mean())}
mu = ops.column_centre(X)
res["correlation_matrix_ms"] = timed(lambda: correlation_matrix(X))
res["moments_kernel_ms"] = timed(lambda: ops.pair_moments(X, mu))
res["column_centre_ms"] = timed(lambda: ops.column_centre(X))
nbytes = 4.0 * N * F
res["matrix_bytes"] = nbytes
res["moments_read_GBps"] = nbytes / (res["moments_kernel_ms"][0] * 1e-3) / 1e9
res["column_sums_read_GBps"] = nbytes / (res["column_centre_ms"][0] * 1e-3) / 1e9
# fp64 MFMA work of the moments kernel: 3 FT^2 + FT tiles of 16 x 16 x 4 per 4 rows, 2 flop per multiply-add
FT = (F + 15) // 16
res["mfma_tiles_per_step"] = 3 * FT * FT + FT
res["moments_fp64_TFLOPs"] = (-(-N // 4)) * res["mfma_tiles_per_step"] * 2048.0 / (res["moments_kernel_ms"][0] * 1e-3) / 1e12
rep = correlation_matrix(X)
pr = args.rows if args.pandas_rows is None else args.pandas_rows
if pr:
    import pandas as pd

    df = pd.DataFrame(X[:pr].cpu().numpy())
    t0 = time.perf_counter()
    want = df.corr().to_numpy()
    res["pandas_corr_s"] = time.perf_counter() - t0
    res["pandas_rows"] = pr
    if pr == N:  # pandas accumulates float32 columns in float64, as the kernel does
        res["max_abs_diff_to_pandas"] = float(np.nanmax(np.abs(rep.r - want)))
        res["nan_pattern_equal"] = bool(np.array_equal(np.isnan(rep.r), np.isnan(want)))
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
