#!/usr/bin/env python
"""Timings of the drift count table (``ops.monitor_ops.bin_counts_gpu``, ``csrc/bincount.hip``) on a
device-resident float32 matrix, against the obvious composition from library ops.

(K) ``bin_counts_gpu``: one pass over the row-major ``X``, all features, into an int64 ``[1, cells]`` table
    (the upload of the edges and the zeroing of the table included);
(T) the composition: per column ``torch.bucketize(X[:, f], edges_f)`` (``right=False``: the same side), the
    NaN mask into the missing cell, ``torch.bincount(cells, minlength=K + 2)``; the column reads are strided, F
    passes over ``X``.

Shapes: 1M x 20 and 10M x 20 with 9 and 255 edges per feature, 2.3M x 106 with 9. Normal columns with 2 % NaN;
edges are the quantile edges (``monitor.drift_edges``) of the first 100k rows, built outside the timed region
and shared by both sides. The sides alternate inside one process, ``--repeats`` rounds after one warm-up
round; every round's time is kept and medians are compared. Both sides give the same integers (asserted once
per shape, outside the timed region). ``x_read_gb_s`` is N * F * 4 bytes over the kernel's median time: the
rate of the single read of ``X``. Writes one JSON document (``--out``) and prints it as one line.

usage: bench_drift.py [--repeats 7] [--out profiles/drift/bench_drift.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from cobalt_smart_lender_ai_amd.monitor import drift_edges  # noqa: E402
from cobalt_smart_lender_ai_amd.ops import monitor_ops  # noqa: E402

SHAPES = [(1_000_000, 20, 9), (1_000_000, 20, 255), (10_000_000, 20, 9), (10_000_000, 20, 255),
          (2_300_000, 106, 9)]
T0 = time.time()


def note(what: str) -> None:
    print(f"[bench_drift +{time.time() - T0:7.1f}s] {what}", file=sys.stderr, flush=True)


def once(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def composition(X: torch.Tensor, edges_dev: list[torch.Tensor]) -> torch.Tensor:
    out = []
    for f, z in enumerate(edges_dev):
        col = X[:, f]
        cell = torch.bucketize(col, z, right=False)
        cell = torch.where(torch.isnan(col), z.numel() + 1, cell)
        out.append(torch.bincount(cell, minlength=z.numel() + 2))
    return torch.cat(out)[None, :]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "drift" / "bench_drift.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "shapes": []}
    for N, F, K in SHAPES:
        g = torch.Generator(device=dev).manual_seed(N + F + K)
        X = torch.randn((N, F), device=dev, generator=g)
        X[torch.rand((N, F), device=dev, generator=g) < 0.02] = float("nan")
        head = X[:100_000].cpu().numpy()
        edges = [drift_edges(head[:, f], K + 1) for f in range(F)]
        edges_dev = [torch.from_numpy(z).to(dev) for z in edges]
        sides = {"kernel": lambda: monitor_ops.bin_counts_gpu(X, edges),
                 "torch_bucketize_bincount": lambda: composition(X, edges_dev)}
        assert torch.equal(sides["kernel"](), sides["torch_bucketize_bincount"]()), (N, F, K)
        torch.cuda.synchronize()
        ms = {k: [] for k in sides}
        for _ in range(a.repeats):
            for k, fn in sides.items():
                ms[k].append(round(once(fn), 3))
        med = {k: statistics.median(v) for k, v in ms.items()}
        row = {"rows": N, "features": F, "edges_per_feature": K,
               "groups": len(monitor_ops.bin_counts_plan(edges, 1)) - 1,
               "kernel_median_ms": round(med["kernel"], 3),
               "torch_median_ms": round(med["torch_bucketize_bincount"], 3),
               "speedup": round(med["torch_bucketize_bincount"] / med["kernel"], 2),
               "x_read_gb_s": round(N * F * 4 / (med["kernel"] * 1e-3) / 1e9, 1), "rounds_ms": ms}
        note(json.dumps({k: v for k, v in row.items() if k != "rounds_ms"}))
        res["shapes"].append(row)
        del X
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
