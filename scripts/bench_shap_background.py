#!/usr/bin/env python
"""Interventional TreeSHAP timings at the reference model's shape (the shipped checkpoint: 300 trees, depth 7,
20 features) on device-resident rows: ``--rows`` explained rows against backgrounds of ``--backgrounds`` rows, in
margin ("raw") and in probability mode (``csrc/shapbg.hip`` through ``predict_ops.treeshap_interventional_gpu``:
the mask kernel of every background tile and the launches of the values included; paths packed and uploaded
before the timed region), next to the path-dependent ``predict_ops.treeshap_gpu`` on the same rows for scale.

The sides alternate inside one session, ``--repeats`` rounds after one warm-up round; every round's time is kept.
Per case the rate is given in (row, background row) pairs per second and in (row, background row, path) triples
per second. The host oracle (``treeshap_interventional_host``, NumPy) is timed once on a ``--host-rows`` x
``--host-rows`` subsample, which is also compared with the GPU values. Writes one JSON document (``--out``) and
prints it as one line.

usage: bench_shap_background.py [--rows 4096] [--backgrounds 100 1000] [--repeats 5]
                                [--out profiles/shapbg/bench_shap_background.json]"""
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
from cobalt_smart_lender_ai_amd.models.booster import load_pickle_bytes, treeshap_interventional_host  # noqa: E402
from cobalt_smart_lender_ai_amd.ops import predict_ops  # noqa: E402


def once(fn) -> float:
    """Milliseconds of one run (device events around work that ends in a synchronise)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(sides: dict, repeats: int) -> dict:
    """``{name: [ms per round]}``: one warm-up round, then ``repeats`` rounds that run the sides in turn."""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(repeats):
        for k, fn in sides.items():
            ms[k].append(round(once(fn), 3))
    return ms


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--backgrounds", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shapbg" / "bench_shap_background.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_shap_background.py needs a GPU"
    b = load_pickle_bytes(lzma.decompress((ROOT / "tests" / "golden" / "xgb_model_tree.pkl.xz").read_bytes()))[1]
    dev = torch.device("cuda", 0)
    nbmax = max(a.backgrounds)
    X, _ = synth.make_lendingclub(a.rows + nbmax, seed=5, device=dev)
    X = X[:, : b.num_feature].to(torch.float32).contiguous()
    X, Z = X[: a.rows], X[a.rows:]
    N, F = X.shape
    gf = predict_ops.gpu_forest(b, dev, None, with_shap=True)
    phi = torch.empty((N, F), dtype=torch.float64, device=dev)
    phi_pd = torch.zeros((N, F), dtype=torch.float64, device=dev)

    sides = {"path_dependent_treeshap_gpu": lambda: predict_ops.treeshap_gpu(b, X, phi_pd)}
    for nb in a.backgrounds:
        for mode in ("raw", "probability"):
            sides[f"interventional_B{nb}_{mode}"] = (
                lambda nb=nb, mode=mode: predict_ops.treeshap_interventional_gpu(b, X, Z[:nb], phi,
                                                                                 probability=(mode == "probability")))
    ms = alternate(sides, a.repeats)
    res = {"rows": N, "trees": b.num_trees, "features": b.num_feature, "max_depth": b.max_depth(),
           "paths": gf.n_paths, "longest_path": gf.max_len, "rounds": a.repeats,
           "background_tile": predict_ops._background_tile(gf.n_paths), "device": torch.cuda.get_device_name(0),
           "cases": {}}
    for k, v in ms.items():
        c = {"median_ms": round(statistics.median(v), 3), "min_ms": min(v), "max_ms": max(v), "rounds_ms": v}
        if k.startswith("interventional"):
            nb = int(k.split("_")[1][1:])
            c["pairs_per_second"] = round(N * nb / (c["median_ms"] * 1e-3), 0)
            c["path_triples_per_second"] = round(N * nb * gf.n_paths / (c["median_ms"] * 1e-3), 0)
        else:
            c["rows_per_second"] = round(N / (c["median_ms"] * 1e-3), 0)
        res["cases"][k] = c

    # the host oracle on a subsample, and the GPU values against it
    h = a.host_rows
    Xh, Zh = X[:h].cpu().numpy(), Z[:h].cpu().numpy()
    host = {}
    for mode in ("raw", "probability"):
        treeshap_interventional_host(b, Xh[:1], Zh[:1], mode)  # (builds the cached path arrays)
        t0 = time.perf_counter()
        want = treeshap_interventional_host(b, Xh, Zh, mode)
        dt = time.perf_counter() - t0
        got = torch.empty((h, F), dtype=torch.float64, device=dev)
        predict_ops.treeshap_interventional_gpu(b, X[:h], Z[:h], got, probability=(mode == "probability"))
        diff = float(np.abs(got.cpu().numpy() - want).max())
        assert diff <= 1e-9, (mode, diff)
        host[mode] = {"rows": h, "background": h, "seconds": round(dt, 3), "pairs_per_second": round(h * h / dt, 1),
                      "max_abs_gpu_minus_host": diff}
    res["host_oracle"] = host
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
