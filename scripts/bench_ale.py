#!/usr/bin/env python
"""Accumulated-local-effects timings at the reference model's shape (the shipped checkpoint: 300 trees, depth 7,
20 features) on a device-resident batch: the 1-D ALE sums of all 20 features, ``grid_resolution`` 20 and 100.

(A) the path ``csrc/ale.hip`` replaces: per feature the row's lo / hi edge (``torch.bucketize``) written into a
    scratch copy of ``X`` and scored through ``permutation_scores_gpu(want_margins=True)`` with an identity
    permutation (that launch walks its baseline job too), the effects and the per-interval sums as tensor ops
    (a sort by interval, a float64 ``cumsum`` and its differences at the interval bounds -- not ``index_add_``:
    nine of the features are binary, one interval, and with ``index_add_`` this side was still running after
    five minutes, presumably in a million float64 atomic adds to one address; results left on the device);
(P) the same with the plain predictor (``predict_margin`` on the substituted copy: two walks per feature);
(B) ``predict_ops.accumulated_local_effects``: cells, the per-chunk stable sorts, one ``k_ale`` launch per 2^17
    rows for all 20 jobs, ``k_ale_reduce``, and the copy of the sums to the host.

The edges are built once, outside the timed region, and are the same for every side; so is the packed forest.
The sides alternate inside one session, ``--repeats`` rounds after one warm-up round; every round's time is
kept. All sides give the same sums (asserted once, outside the timed region). Writes one JSON document
(``--out``) and prints it as one line.

usage: bench_ale.py [--rows 1000000] [--repeats 4] [--out profiles/ale/bench_ale.json]"""
import argparse
import json
import lzma
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from cobalt_smart_lender_ai_amd.dataio import synth  # noqa: E402
from cobalt_smart_lender_ai_amd.models.booster import ale_edges, load_pickle_bytes  # noqa: E402
from cobalt_smart_lender_ai_amd.ops import predict_ops  # noqa: E402


T0 = time.time()


def note(what: str) -> None:
    print(f"[bench_ale +{time.time() - T0:7.1f}s] {what}", file=sys.stderr, flush=True)


def once(fn) -> float:
    """Milliseconds of one run (device events around work that ends in a synchronise)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(sides: dict, repeats: int) -> dict:
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(repeats):
        for k, fn in sides.items():
            ms[k].append(round(once(fn), 3))
    return ms


def summary(ms: dict) -> dict:
    return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": min(v), "max_ms": max(v), "rounds_ms": v}
            for k, v in ms.items()}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ale" / "bench_ale.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ale.py needs a GPU"
    b = load_pickle_bytes(lzma.decompress((ROOT / "tests" / "golden" / "xgb_model_tree.pkl.xz").read_bytes()))[1]
    dev = torch.device("cuda", 0)
    X, _ = synth.make_lendingclub(a.rows, seed=5, device=dev)
    X = X[:, : b.num_feature].to(torch.float32).contiguous()
    N = X.shape[0]
    Xh = X.cpu().numpy()
    predict_ops.gpu_forest(b, dev)
    ident = torch.arange(N, dtype=torch.int32, device=dev).reshape(1, N)

    res = {"rows": N, "trees": b.num_trees, "features": b.num_feature, "max_depth": b.max_depth(),
           "rounds": a.repeats, "device": torch.cuda.get_device_name(0), "cases": {}}
    for resolution in (20, 100):
        edges = [ale_edges(Xh[:, f], resolution) for f in range(b.num_feature)]
        feats = [f for f in range(b.num_feature) if len(edges[f]) >= 2]
        zs = {f: torch.from_numpy(edges[f]).to(dev) for f in feats}
        kmax = max(len(edges[f]) - 1 for f in feats)

        def substituted(score) -> torch.Tensor:
            """[jobs, kmax, 3] float64 on the device from a scorer of a substituted copy of X."""
            out = torch.zeros((len(feats), kmax, 3), dtype=torch.float64, device=dev)
            Xs = X.clone()
            for j, f in enumerate(feats):
                z, x = zs[f], X[:, f]
                live = ~torch.isnan(x)
                k = torch.bucketize(torch.nan_to_num(x, nan=0.0), z).clamp(1, len(z) - 1)
                Xs[:, f] = z[k - 1]
                lo = score(Xs, f).double()
                Xs[:, f] = z[k]
                hi = score(Xs, f).double()
                Xs[:, f] = x
                wv = live.double()
                srt, idx = torch.sort(k - 1)
                bounds = torch.searchsorted(srt, torch.arange(kmax + 1, device=dev))
                for q, v in enumerate((wv * (hi - lo), wv * (torch.sigmoid(hi) - torch.sigmoid(lo)), wv)):
                    c = torch.cat([v.new_zeros(1), torch.cumsum(v[idx], 0)])
                    out[j, :, q] = c[bounds[1:]] - c[bounds[:-1]]
            return out

        def via_perm(Xs, f):
            m, _ = predict_ops.permutation_scores_gpu(b, Xs, None, [f], ident, want_margins=True, want_sums=False)
            return m[1]

        def via_predict(Xs, f):
            return b.predict_margin(Xs)

        def fused():
            return predict_ops.accumulated_local_effects(b, X, [(f,) for f in feats], [[edges[f]] for f in feats])

        # the sides agree (outside the timed region)
        note(f"grid_resolution={resolution}: {len(feats)} jobs")
        Bs = fused()
        torch.cuda.synchronize()
        note("B done")
        A = substituted(via_perm).cpu().numpy()
        note("A done")
        P = substituted(via_predict).cpu().numpy()
        note("P done")
        diff = 0.0
        for j, f in enumerate(feats):
            K = len(edges[f]) - 1
            for q, key in enumerate(("sum_margin", "sum_prob", "weight")):
                scale = max(1.0, float(np.abs(Bs[j][key]).max()))
                diff = max(diff, float(np.abs(A[j, :K, q] - Bs[j][key]).max()) / scale,
                           float(np.abs(P[j, :K, q] - Bs[j][key]).max()) / scale)
        assert diff <= 1e-9, diff
        ms = alternate({"A_substitute_permutation_scores": lambda: substituted(via_perm),
                        "P_substitute_predict_margin": lambda: substituted(via_predict),
                        "B_ale_kernel": fused}, a.repeats)
        note("timed rounds done")
        s = summary(ms)
        med = {k: v["median_ms"] for k, v in s.items()}
        res["cases"][f"grid_resolution={resolution}"] = {
            "jobs": len(feats), "intervals": [len(edges[f]) - 1 for f in feats], "sides": s,
            "max_relative_sum_difference": diff,
            "A_over_B": round(med["A_substitute_permutation_scores"] / med["B_ale_kernel"], 3),
            "P_over_B": round(med["P_substitute_predict_margin"] / med["B_ale_kernel"], 3),
            "row_corner_trees_per_second_B": round(N * 2 * len(feats) * b.num_trees / (med["B_ale_kernel"] * 1e-3), 0)}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
