#!/usr/bin/env python
"""Counterfactual-recourse timings at the shipped model's shape (300 trees, depth 7, 20 features) on
device-resident synthetic rows that the model declines, under the default policy (config.RECOURSE_POLICY),
``max_changes=1``.

(a) composition -- what a user could build before ``csrc/recourse.hip``: per actionable feature one
    ``partial_dependence_gpu(want_ice=True)`` on the same candidate table (a ``[G, N]`` float32 matrix), then
    torch reductions over it for the three slots;
(b) the scan kernel: one ``recourse_scan_gpu`` call for all features (launches only, results left on the
    device);
(c) ``explain.counterfactuals`` end to end (margins, scan, selection, report on the host).

(a) and (b) are checked to give the same indices and margin bits. One warm-up on the first 4096 rows, then
``--repeats`` alternating runs of (a) and (b); device events around work that ends in a synchronise; every run
is listed, so the spread is visible. Both walk (row, candidate, tree) the same number of times; the count is
computed from the shapes. Writes one JSON document (``--out``) and prints it as one line.

usage: bench_recourse.py [--rows 1000000] [--repeats 2] [--out profiles/configs/recourse-1m.json]"""
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
from cobalt_smart_lender_ai_amd import _native, explain  # noqa: E402
from cobalt_smart_lender_ai_amd.dataio import synth  # noqa: E402
from cobalt_smart_lender_ai_amd.explain import recourse as R  # noqa: E402
from cobalt_smart_lender_ai_amd.models.booster import load_pickle_bytes  # noqa: E402
from cobalt_smart_lender_ai_amd.ops import predict_ops  # noqa: E402


def event_ms(fn) -> tuple[float, object]:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def declined_rows(b, rows: int, cutoff: float, dev) -> torch.Tensor:
    """``rows`` synthetic rows with a probability of default above ``cutoff``."""
    keep, have, seed = [], 0, 5
    while have < rows:
        X, _ = synth.make_lendingclub(max(rows, 65536), seed=seed, device=dev)
        X = X[:, : b.num_feature].to(torch.float32).contiguous()
        X = X[b.predict_proba(X) > cutoff]
        keep.append(X)
        have += X.shape[0]
        seed += 1
        if seed > 200:
            raise RuntimeError("the generator yields too few declined rows")
    return torch.cat(keep)[:rows].contiguous()


def composition(b, X, p, target: float):
    """The three slots per feature from ICE matrices: (idx [N, A, 3] int32, margin [N, A, 3] float32)."""
    N, A = X.shape[0], len(p.feats)
    idx = torch.empty((N, A, 3), dtype=torch.int32, device=X.device)
    mg = torch.empty((N, A, 3), dtype=torch.float32, device=X.device)
    empty = torch.tensor(0x7FC00000, dtype=torch.int32, device=X.device).view(torch.float32)
    for a, f in enumerate(p.feats):
        jlo, jhi = int(p.win[a, 0]), int(p.win[a, 1])
        cv = torch.from_numpy(p.cands[a]).to(X.device)
        G = jhi - jlo + 1
        x = X[:, f]
        c = torch.searchsorted(cv, x.contiguous(), right=True) - 1
        if G <= 0:
            idx[:, a] = -1
            mg[:, a] = empty
            continue
        ice, _ = predict_ops.partial_dependence_gpu(b, X, (f,), [p.cands[a][jlo:jhi + 1]], want_ice=True,
                                                    want_avg=False)
        j = torch.arange(jlo, jhi + 1, device=X.device)[:, None]
        below = j < c[None, :]
        d = int(p.dirs[a])
        ok = (j != c[None, :]) & ~torch.isnan(x)[None, :] & (~below if d == 1 else below if d == -1 else True)
        hit = ok & (ice <= target)
        dn = torch.where(hit & below, j, -1).max(dim=0).values
        up = torch.where(hit & ~below, j, jhi + 1).min(dim=0).values
        up = torch.where(up > jhi, -1, up)
        m = torch.where(ok, ice, torch.full_like(ice, float("inf")))
        tie = ok & (ice == m.min(dim=0).values[None, :])
        dist = torch.where(tie, (j - c[None, :]).abs(), 1 << 40)
        be = torch.where(tie & (dist == dist.min(dim=0).values[None, :]), j, jhi + 1).min(dim=0).values
        be = torch.where(be > jhi, -1, be)
        for s, sel in enumerate((dn, up, be)):
            idx[:, a, s] = sel.to(torch.int32)
            got = ice.gather(0, (sel.clamp(min=jlo) - jlo)[None, :])[0]
            mg[:, a, s] = torch.where(sel >= 0, got, empty)
    return idx, mg


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--cutoff", type=float, default=0.5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "configs" / "recourse-1m.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_recourse.py needs a GPU"
    b = load_pickle_bytes(lzma.decompress((ROOT / "tests" / "golden" / "xgb_model_tree.pkl.xz").read_bytes()))[1]
    dev = torch.device("cuda", 0)
    predict_ops.gpu_forest(b, dev)
    X = declined_rows(b, a.rows, a.cutoff, dev)
    N = X.shape[0]
    policy = R.default_policy(b)
    p = R._build_policy(b, None, policy["immutable"], policy["increase_only"], policy["decrease_only"], None,
                        policy["grids"], None, None, None)
    target = R.target_margin(a.cutoff)
    chunk = int(_native.lib().cobalt_recourse_chunk())
    points = sum(-(-(int(hi) - int(lo) + 1) // chunk) * chunk for lo, hi in p.win if hi >= lo)
    walks = N * points * b.num_trees

    def scan(Xs):
        return predict_ops.recourse_scan_gpu(b, Xs, p.feats, p.cands, win=p.win, dirs=p.dirs, target_margin=target)

    scan(X[:4096]), composition(b, X[:4096], p, target)   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t_comp, t_scan = [], []
    for _ in range(a.repeats):
        ms, (ci, cm) = event_ms(lambda: composition(b, X, p, target))
        t_comp.append(ms)
        ms, (si, sm) = event_ms(lambda: scan(X))
        t_scan.append(ms)
        print(f"[recourse] composition {t_comp[-1]:.0f} ms, scan {ms:.0f} ms", file=sys.stderr, flush=True)
    same = bool(torch.equal(ci, si)) and bool(torch.equal(cm.view(torch.int32), sm.view(torch.int32)))
    del ci, cm
    t_api, rep = event_ms(lambda: explain.counterfactuals(b, X, cutoff=a.cutoff, max_changes=1, **policy))
    s = rep.summary()
    res = {"config": "recourse-1m", "metric": "ms per call, device-resident rows", "rows": N, "trees": b.num_trees,
           "features": b.num_feature, "actionable": len(p.feats), "candidates": int(p.cand_ptr[-1]),
           "scored_points_per_row": points, "cutoff": a.cutoff, "max_changes": 1,
           "device": torch.cuda.get_device_name(0),
           "composition_pdp_ice_plus_torch_ms": [round(t, 1) for t in t_comp],
           "scan_kernel_ms": [round(t, 1) for t in t_scan],
           "composition_over_scan": round(statistics.median(t_comp) / statistics.median(t_scan), 3),
           "counterfactuals_end_to_end_ms": round(t_api, 1),
           "walks_per_second_scan": round(walks / (statistics.median(t_scan) * 1e-3), 0),
           "composition_equals_scan": same, "status_share": s["status_share"], "median_cost": s["median_cost"]}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
