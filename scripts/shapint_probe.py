#!/usr/bin/env python
"""TreeSHAP interaction-value timings on the reference model (300 trees, depth 7, 20 features), with
``shap_values`` on the same device-resident batches in the same process as the yardstick. Per batch
size one JSON line: median device time (events; warm-up first, synchronise outside the timed region)
of the interaction kernel alone (SHAP values precomputed), of ``shap_interaction_values`` end to end
(SHAP values + kernel + output allocation) and of ``shap_values``.

usage: shapint_probe.py [batch ...]   (default 4096 65535)"""
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from cobalt_smart_lender_ai_amd import _native  # noqa: E402
from cobalt_smart_lender_ai_amd.dataio import synth  # noqa: E402
from cobalt_smart_lender_ai_amd.models.booster import load_pickle_bytes  # noqa: E402
from cobalt_smart_lender_ai_amd.ops import predict_ops  # noqa: E402

REPEATS = 7


def timed(fn) -> float:
    """Median milliseconds of REPEATS runs after one warm-up."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main() -> None:
    sizes = [int(a) for a in sys.argv[1:]] or [4096, 65535]
    b = load_pickle_bytes((ROOT / "src" / "api" / "models" / "xgb_model_tree.pkl").read_bytes())[1]
    dev = torch.device("cuda", 0)
    F = b.num_feature
    X, _ = synth.make_lendingclub(max(sizes), seed=5, device=dev)
    X = X[:, :F].contiguous()
    gf = predict_ops.gpu_forest(b, dev, None, with_shap=True)
    lib = _native.lib()
    lds = int(lib.cobalt_treeshap_interactions_lds(F, gf.max_len))
    print(json.dumps({"paths": int(gf.n_paths), "max_len": int(gf.max_len), "features": F, "lds_bytes_per_block": lds,
                      "blocks_per_cu_by_lds": (160 * 1024) // lds}), flush=True)
    for n in sizes:
        Xn = X[:n].contiguous()
        phi = b.shap_values(Xn)
        out = torch.empty((n, F, F), dtype=torch.float64, device=dev)

        def kernel_only():
            for s in range(0, n, predict_ops.SHAP_INT_ROWS):
                e = min(n, s + predict_ops.SHAP_INT_ROWS)
                rc = lib.cobalt_treeshap_interactions(Xn[s:e].data_ptr(), e - s, F, Xn.stride(0), gf.elems.data_ptr(),
                                                      gf.path_ptr.data_ptr(), gf.path_val.data_ptr(), gf.n_paths,
                                                      gf.max_len, phi[s:e].data_ptr(), out[s:e].data_ptr(),
                                                      _native.stream_handle())
                _native.check(rc, "cobalt_treeshap_interactions")

        t_kernel = timed(kernel_only)
        t_e2e = timed(lambda: b.shap_interaction_values(Xn))
        t_shap = timed(lambda: b.shap_values(Xn))
        full = b.shap_interaction_values(Xn)
        ok = bool(torch.equal(full, out)) and bool((full.sum(2) - phi).abs().max() < 1e-9)
        print(json.dumps({"rows": n, "interactions_kernel_ms": round(t_kernel, 3),
                          "interactions_end_to_end_ms": round(t_e2e, 3), "shap_values_ms": round(t_shap, 3),
                          "ratio_end_to_end": round(t_e2e / t_shap, 1), "ratio_kernel": round(t_kernel / t_shap, 1),
                          "rows_per_s_end_to_end": round(n / t_e2e * 1e3), "consistent": ok}), flush=True)


if __name__ == "__main__":
    main()
