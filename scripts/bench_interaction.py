#!/usr/bin/env python
"""Cost of interaction constraints at bench.py's headline shape (10M rows, 20 features, 300 depth-7 trees).

One process, one GPU: after warm-up fits of both kinds, unconstrained and constrained fits (five groups of
four features) are timed ALTERNATELY, each fit between device synchronisations, so clock and thermal drift
hit both kinds alike. Prints every fit's time and one JSON line with the medians, the spreads and the
ratio. The constrained fit runs the separate evaluation + partition kernels (no fused pass), so the ratio
includes that; it also grows other (more additive) trees than the free fit.

    python scripts/bench_interaction.py [--rows N] [--trees T] [--depth D] [--steps K] [--warmup W]
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from cobalt_smart_lender_ai_amd.dataio import synth  # noqa: E402
from cobalt_smart_lender_ai_amd.models import gbdt  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--trees", type=int, default=300)
    ap.add_argument("--depth", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    X, y = synth.make_lendingclub(a.rows, seed=a.seed, device=dev)
    pos = float(y.sum())
    F = X.shape[1]
    free = gbdt.GBDTParams(n_estimators=a.trees, max_depth=a.depth, learning_rate=0.05, gamma=5.0, reg_lambda=1.0,
                           min_child_weight=1.0, max_bin=256, scale_pos_weight=(a.rows - pos) / pos, random_state=78,
                           sketch_rows=None)
    cons = [list(range(f, min(f + 4, F))) for f in range(0, F, 4)]  # 20 features: five groups of four
    inter = dataclasses.replace(free, interaction_constraints=cons)

    def fit(p) -> tuple[float, int]:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        b = gbdt.train(X, y, p, device=dev, feature_names=synth.FEATURES, feature_types=synth.FEATURE_TYPES)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, sum(int((t.left_children != -1).sum()) for t in b.trees)

    for _ in range(a.warmup):
        fit(free)
        fit(inter)
    times: dict[str, list[float]] = {"unconstrained": [], "constrained": []}
    splits = {}
    for i in range(a.steps):
        for name, p in (("unconstrained", free), ("constrained", inter)):
            ms, splits[name] = fit(p)
            times[name].append(ms)
            print(f"[bench_interaction] step {i} {name}: {ms:.1f} ms", file=sys.stderr)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"rows": a.rows, "features": F, "trees": a.trees, "depth": a.depth, "steps": a.steps,
                      "constraints": cons, "fit_ms_median": med,
                      "fit_ms_min_max": {k: [min(v), max(v)] for k, v in times.items()},
                      "fit_ms_all": times, "splits": splits,
                      "constrained_over_unconstrained": med["constrained"] / med["unconstrained"]}))


if __name__ == "__main__":
    main()
