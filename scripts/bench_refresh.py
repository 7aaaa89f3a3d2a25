#!/usr/bin/env python
"""Leaf-index and leaf-refresh timings on the reference model (300 trees, depth 7, 20 features) over a
device-resident batch, next to one ``predict_margin`` of the same rows for scale:

* ``predict_leaf``: the walk that writes tree-major uint16 indices, plus the op's transpose to int32 [N, T];
* ``refresh``: the launches of ``csrc/refresh.hip`` (one forest walk per tree group, then per tree one
  streaming pass over the rows and one finalize block), and the whole call with the host's share (labels and
  weights checked and uploaded, statistics fetched, the new booster assembled).

The structure's floor is one forest walk plus T streaming passes (per row and tree: 2 B index, 2 B previous
index, 4 B margin read + 4 B written, 4 B label, 4 B weight). Median device time (events; one warm-up first,
synchronise outside the timed region). One JSON line per row count.

usage: bench_refresh.py [--rows 1000000 10000000] [--repeats 5]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from cobalt_smart_lender_ai_amd.dataio import synth  # noqa: E402
from cobalt_smart_lender_ai_amd.models.booster import (load_pickle_bytes, refresh_params,  # noqa: E402
                                                       refresh_row_weights)
from cobalt_smart_lender_ai_amd.models.gbdt_host import quant_scales  # noqa: E402
from cobalt_smart_lender_ai_amd.ops import predict_ops  # noqa: E402


def timed(fn, repeats: int) -> float:
    """Median milliseconds of ``repeats`` runs after one warm-up."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    b = load_pickle_bytes((ROOT / "src" / "api" / "models" / "xgb_model_tree.pkl").read_bytes())[1]
    dev = torch.device("cuda", 0)
    for rows in a.rows:
        X, y = synth.make_lendingclub(rows, seed=5, device=dev)
        X = X[:, : b.num_feature].contiguous()
        y = y.to(torch.float32).contiguous()
        T, N = b.num_trees, X.shape[0]
        p = refresh_params(b, {})
        y_host = y.cpu().numpy()
        wt_host = refresh_row_weights(y_host, None, p["scale_pos_weight"])
        gscale, hscale = quant_scales(float(wt_host.max()), p["grad_bits"])
        wt = torch.as_tensor(wt_host, device=dev)

        t_predict = timed(lambda: b.predict_margin(X), a.repeats)
        t_leaf = timed(lambda: predict_ops.predict_leaf_gpu(b, X), a.repeats)
        t_launch = timed(lambda: predict_ops.refresh_gpu(b, X, y, wt, p, gscale, hscale, True), a.repeats)
        t_keep = timed(lambda: predict_ops.refresh_gpu(b, X, y, wt, p, gscale, hscale, False), a.repeats)
        t_e2e = timed(lambda: b.refresh(X, y), max(2, a.repeats // 2))
        new, m = b.refresh(X, y, return_margin=True)
        ok = bool(torch.equal(m, new.predict_margin(X)))
        stream_bytes = 20 * N * T  # the accumulate passes' traffic (see the module docstring)
        print(json.dumps({
            "rows": N, "trees": T, "group_trees": predict_ops._group_trees(N, T, None),
            "predict_margin_ms": round(t_predict, 3), "predict_leaf_ms": round(t_leaf, 3),
            "refresh_launches_ms": round(t_launch, 3), "refresh_keep_leaves_launches_ms": round(t_keep, 3),
            "refresh_end_to_end_ms": round(t_e2e, 3), "refresh_over_predict": round(t_launch / t_predict, 2),
            "refresh_us_per_tree": round(t_launch / T * 1e3, 2),
            "stream_floor_ms_at_4TBps": round(stream_bytes / 4e12 * 1e3, 3), "margins_consistent": ok}), flush=True)
        del X, y, wt, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
