"""Times of the calibration kernels (csrc/calib.hip) on one GPU: the isotonic fit at ``--rows`` rows split into
sort, grouping + cumsum, hull and knots, ``calib_apply`` and ``reliability_sums``, the hull when no tile sheds a
point, and the same isotonic fit by sklearn on the host at 1M rows as the yardstick. Every GPU figure is
(median, min, max) in ms of ``torch.cuda.Event`` pairs around warmed calls. One JSON line on stdout.

    python scripts/bench_calibration.py [--rows 10000000] [--out calib_perf.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import numpy as np
import torch

from cobalt_smart_lender_ai_amd.metrics import calibration as C
from cobalt_smart_lender_ai_amd.models import calibration as MC
from cobalt_smart_lender_ai_amd.ops import calib_ops

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
N = args.rows
g = torch.Generator(device="cuda").manual_seed(0)
m = torch.randn(N, device="cuda", generator=g) * 1.5 - 1.0
y = (torch.rand(N, device="cuda", generator=g) < torch.sigmoid(0.8 * m - 0.5)).to(torch.float32)


def timed(fn, reps=7, warm=2):
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


res = {"rows": N}
res["sort_ms"] = timed(lambda: torch.sort(m, stable=True))
res["groups_incl_sort_ms"] = timed(lambda: calib_ops.iso_groups_gpu(m, y))
ux, cw, cs, total = calib_ops.iso_groups_gpu(m, y)
res["groups"] = int(ux.shape[0])
res["hull_ms"] = timed(lambda: calib_ops.iso_hull(cw, cs, total))
hull, rounds = calib_ops.iso_hull(cw, cs, total, return_rounds=True)
res["hull_vertices"] = int(hull.shape[0])
res["survivors_per_round"] = rounds
res["fit_total_ms"] = timed(lambda: calib_ops.iso_fit_gpu(m, y))
cal = MC.IsotonicCalibrator().fit(m, y)
res["knots"] = int(cal.x_thresholds_.shape[0])
xk = torch.from_numpy(cal.x_thresholds_).cuda()
vk = torch.from_numpy(cal.y_thresholds_).cuda()
res["apply_ms"] = timed(lambda: calib_ops.calib_apply(m, xk, vk))
p = calib_ops.calib_apply(m, xk, vk)
for B in (10, 100):
    e = torch.from_numpy(C.edges_for("uniform", B)).cuda()
    res[f"reliability_B{B}_ms"] = timed(lambda: calib_ops.reliability_sums(p, y, None, e, check=False))
wq = torch.randint(1, 200, (N,), device="cuda", dtype=torch.int32)
e = torch.from_numpy(C.edges_for("uniform", 10)).cuda()
res["reliability_B10_weighted_ms"] = timed(lambda: calib_ops.reliability_sums(p, y, wq, e, check=False))
res["reliability_report_ms"] = timed(lambda: C.reliability_report(y, p), reps=3, warm=1)

# adversarial: no tile sheds a point (46340 groups is the most the weight bound allows)
k = torch.arange(46340, dtype=torch.int64, device="cuda")
cwa = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(torch.full_like(k, 46340), 0)])
csa = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(k, 0)])
res["hull_convex_46341_ms"] = timed(lambda: calib_ops.iso_hull(cwa, csa, int(cwa[-1])), reps=3, warm=1)

# yardstick: sklearn on the host at 1M rows
M1 = min(N, 1_000_000)
from sklearn.isotonic import IsotonicRegression
mh = m[:M1].cpu().numpy().astype(np.float64)
yh = y[:M1].cpu().numpy().astype(np.float64)
t0 = time.perf_counter()
IsotonicRegression(out_of_bounds="clip").fit(mh, yh)
res["sklearn_1M_ms"] = (time.perf_counter() - t0) * 1e3
res["gpu_fit_1M_ms"] = timed(lambda: calib_ops.iso_fit_gpu(m[:M1], y[:M1]))
t0 = time.perf_counter()
C.iso_fit_host(mh.astype(np.float32), yh)
res["host_fit_1M_ms"] = (time.perf_counter() - t0) * 1e3
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
