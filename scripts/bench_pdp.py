#!/usr/bin/env python
"""Partial-dependence timings at the reference model's shape (the shipped checkpoint: 300 trees, depth 7,
20 features) on a device-resident batch: a 100-point 1-D grid and a 20 x 20 2-D grid.

(a) baseline -- what a user could do before ``Booster.partial_dependence``: per grid point clone ``X``,
    overwrite the column(s), ``predict_proba`` on the GPU, ``torch.mean`` (the forest is packed and
    uploaded before the timed region);
(b) the kernel path (``csrc/pdp.hip``) for ``kind="average"`` and ``kind="both"``: launches only
    (``predict_ops.partial_dependence_gpu``, results left on the device) and end to end through
    ``Booster.partial_dependence`` (grid construction and the copies to the host included).

Median of ``--repeats`` runs after one warm-up; device events around work that ends in a synchronise.
Writes one JSON document (``--out``) and prints it as one line.

usage: bench_pdp.py [--rows 100000] [--repeats 5] [--out profiles/pdp/bench_pdp.json]"""
import argparse
import json
import lzma
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from cobalt_smart_lender_ai_amd.dataio import synth  # noqa: E402
from cobalt_smart_lender_ai_amd.models.booster import load_pickle_bytes  # noqa: E402
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
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pdp" / "bench_pdp.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pdp.py needs a GPU"
    b = load_pickle_bytes(lzma.decompress((ROOT / "tests" / "golden" / "xgb_model_tree.pkl.xz").read_bytes()))[1]
    dev = torch.device("cuda", 0)
    X, _ = synth.make_lendingclub(a.rows, seed=5, device=dev)
    X = X[:, : b.num_feature].to(torch.float32).contiguous()
    N = X.shape[0]
    predict_ops.gpu_forest(b, dev)
    Xh = X.cpu().numpy()
    # the two features with the most splits: the curves a user would look at first
    used = np.zeros(b.num_feature, np.int64)
    for t in b.trees:
        np.add.at(used, t.split_indices[~t.is_leaf], 1)
    f1, f2 = (int(f) for f in np.argsort(-used, kind="stable")[:2])

    def axis(f, n):  # n points between the 5th and 95th percentile, whatever the column's number of unique values
        col = Xh[:, f][~np.isnan(Xh[:, f])]
        return np.linspace(np.quantile(col, 0.05), np.quantile(col, 0.95), n).astype(np.float32)

    cases = {"1d_100": ((f1,), [axis(f1, 100)]), "2d_20x20": ((f1, f2), [axis(f1, 20), axis(f2, 20)])}
    res = {"rows": N, "trees": b.num_trees, "features": b.num_feature, "max_depth": b.max_depth(),
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, (feats, grids) in cases.items():
        G = int(np.prod([len(g) for g in grids]))
        gd = [torch.from_numpy(g).to(dev) for g in grids]

        def baseline():
            out = torch.empty(G, dtype=torch.float32, device=dev)
            k = 0
            for i1 in range(len(grids[0])):
                for i2 in range(len(grids[1]) if len(feats) == 2 else 1):
                    Xs = X.clone()
                    Xs[:, feats[0]] = gd[0][i1]
                    if len(feats) == 2:
                        Xs[:, feats[1]] = gd[1][i2]
                    out[k] = torch.mean(b.predict_proba(Xs))
                    k += 1
            return out

        def kernel(want_ice):
            return predict_ops.partial_dependence_gpu(b, X, feats, grids, want_ice=want_ice, want_avg=True)

        grid_arg = grids[0] if len(feats) == 1 else grids
        t_base = timed(baseline, a.repeats)
        t_avg = timed(lambda: kernel(False), a.repeats)
        t_both = timed(lambda: kernel(True), a.repeats)
        t_avg_api = timed(lambda: b.partial_dependence(X, feats, grid=grid_arg, kind="average"), a.repeats)
        t_both_api = timed(lambda: b.partial_dependence(X, feats, grid=grid_arg, kind="both"), a.repeats)
        # the two paths compute the same curve (fp32 mean of device probabilities against the fp64 mean)
        base = baseline().double().cpu().numpy()
        new = b.partial_dependence(X, feats, grid=grid_arg, kind="average")["average"].reshape(-1)
        res["cases"][name] = {
            "features": list(feats), "grid_points": G,
            "baseline_clone_predict_mean_ms": round(t_base, 3),
            "kernel_average_ms": round(t_avg, 3), "kernel_both_ms": round(t_both, 3),
            "api_average_ms": round(t_avg_api, 3), "api_both_ms": round(t_both_api, 3),
            "baseline_over_kernel_average": round(t_base / t_avg, 2),
            "baseline_over_kernel_both": round(t_base / t_both, 2),
            "baseline_over_api_average": round(t_base / t_avg_api, 2),
            "baseline_over_api_both": round(t_base / t_both_api, 2),
            "row_trees_per_second_kernel_average": round(N * G * b.num_trees / (t_avg * 1e-3), 0),
            "max_abs_curve_difference": float(np.abs(base - new).max()),
        }
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
