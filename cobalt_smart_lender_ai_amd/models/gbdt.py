"""Gradient-boosted decision trees for binary credit-default classification.

Public API:

* :func:`train` — fit a :class:`~.booster.Booster` on a feature matrix (GPU: hand-written gfx950
  kernels, optionally data-parallel across ranks; CPU: the NumPy reference trainer).
* :class:`GBDTClassifier` — an sklearn-compatible estimator with the constructor arguments and
  attributes of ``xgboost.XGBClassifier`` used by the reference (``n_estimators``, ``max_depth``,
  ``learning_rate``, ``gamma``, ``subsample``, ``colsample_bytree``, ``scale_pos_weight``,
  ``random_state``, ``eval_metric``, ``feature_importances_``, ``get_booster()``, ``predict_proba``),
  so it drops into sklearn's RFE / RandomizedSearchCV exactly where the reference used XGBClassifier
  (src/model_train_test/model_tree_train_test.py:111-164).

A fit = quantile sketch (K12) + binning (K13) + ``n_estimators`` boosting rounds of depthwise
histogram trees (K14-K20). See ``csrc/gbdt.hip`` for the device design.
"""
from __future__ import annotations

import ctypes
import json
import logging
import math
import os
import time
from dataclasses import asdict, dataclass, field
from typing import Any, Sequence

import numpy as np
import torch

from . import gbdt_host, sketch
from .booster import Booster, dump_pickle_bytes, sigmoid32, trees_from_heap_nodes
from ..config import knob

log = logging.getLogger(__name__)

XGB_DEFAULTS = dict(n_estimators=100, max_depth=6, learning_rate=0.3, gamma=0.0, min_child_weight=1.0,
                    reg_lambda=1.0, reg_alpha=0.0, subsample=1.0, colsample_bytree=1.0, max_bin=256,
                    scale_pos_weight=1.0, random_state=0, base_score=None)


@dataclass
class GBDTParams:
    n_estimators: int = 100
    max_depth: int = 6
    learning_rate: float = 0.3
    gamma: float = 0.0
    min_child_weight: float = 1.0
    reg_lambda: float = 1.0
    reg_alpha: float = 0.0
    subsample: float = 1.0
    colsample_bytree: float = 1.0
    max_bin: int = 256
    scale_pos_weight: float = 1.0
    random_state: int = 0
    base_score: float | None = None
    # rows of the strided global sample the quantile sketch uses; None / 0 = every row (exact weighted
    # quantiles; on the GPU the device sketch of csrc/sketch.hip, exact under data parallelism too);
    # SKETCH_AUTO (default) = every row on a GPU (XGBoost hist's semantics: the device sketch, ~4 ms at
    # 10M rows; up to 2^18 rows the full sort), a 2^18-row strided sample on the CPU; streams / external
    # memory: see models/stream.stream_cuts
    sketch_rows: int | None = -1
    # quantile-sketch weights: "sample" = the sample weights (XGBoost hist semantics, the reference's
    # tree_method), "hessian" = first-round hessians (sample weight x scale_pos_weight for positives,
    # XGBoost approx semantics); sketch_mode "summary" merges per-rank QuantileSummary objects
    # instead of all-gathering the global sample (see models/sketch.py)
    sketch_weight: str = "sample"
    sketch_mode: str = "sample"
    # fixed-point gradient precision: 17 bits (default; one packed u64 LDS atomic per cell) or 25 bits
    # ("wide": g and h summed in separate int64 cells, 256x finer steps; 32-byte records, <= 24 features
    # on the GPU; the CPU trainer implements both exactly -- docs/PERF.md "Gradient precision")
    grad_bits: int = 17
    # monotone constraints (XGBoost's ``monotone_constraints``): a sequence of {-1, 0, +1} per feature, the
    # string form "(1,0,-1)", or {feature_name: +-1} (resolved against the fit's feature names; unnamed
    # features get 0). None / () / "()" / all zeros: the unconstrained fit. See :func:`resolve_monotone`.
    monotone_constraints: Any = None
    # interaction constraints (XGBoost's ``interaction_constraints``): a list of feature groups, as lists of
    # indices, lists of feature names (resolved against the fit's feature names) or the string / JSON form
    # "[[0, 1], [2, 3]]". Features may share a root-to-leaf path only when one group holds them all.
    # None / [] / "" / "[]": the unconstrained fit. See :func:`resolve_interaction`.
    interaction_constraints: Any = None
    # trees after which the GPU trainer regroups the training rows by the leaf they reached (the model and
    # the returned margins do not depend on it; see :func:`resolve_row_reorder`): a list of tree indices, an
    # int period, the string forms "0,8,32" / "every:16" / "off". None: COBALT_ROW_REORDER
    row_reorder: Any = None

    @classmethod
    def from_kwargs(cls, **kw) -> "GBDTParams":
        names = {f for f in cls.__dataclass_fields__}
        alias = {"eta": "learning_rate", "lambda": "reg_lambda", "alpha": "reg_alpha", "min_split_loss": "gamma",
                 "seed": "random_state"}
        out = {}
        for k, v in kw.items():
            k = alias.get(k, k)
            if k in names and v is not None:
                out[k] = v
        return cls(**out)


@dataclass
class FitReport:
    """Timings and sizes of one fit (for logs / bench)."""
    n_rows: int = 0
    n_rows_global: int = 0
    n_features: int = 0
    n_trees: int = 0
    device: str = "cpu"
    world: int = 1
    t_sketch: float = 0.0
    t_bin: float = 0.0
    t_boost: float = 0.0
    t_total: float = 0.0
    phases: dict[str, float] = field(default_factory=dict)   # filled when ``sync_phases`` is set
    sync_phases: bool = False
    extra: dict[str, Any] = field(default_factory=dict)

    def mark(self, name: str, t_prev: float, dev: torch.device) -> float:
        """Record the wall time since ``t_prev`` under ``name`` (device-synchronised when profiling)."""
        if not self.sync_phases:
            return t_prev
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        now = time.perf_counter()
        self.phases[name] = self.phases.get(name, 0.0) + (now - t_prev)
        return now


def _to_tensor(X, device, dtype=torch.float32) -> torch.Tensor:
    if isinstance(X, torch.Tensor):
        return X.to(device=device, dtype=dtype).contiguous()
    if hasattr(X, "to_numpy"):
        X = X.to_numpy(dtype=np.float32, na_value=np.nan) if hasattr(X, "columns") else X.to_numpy()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(X, dtype=np.float32)), device=device).to(dtype).contiguous()


def _resolve_device(device: str | torch.device | None, X) -> torch.device:
    if device is None:
        if isinstance(X, torch.Tensor):
            return X.device
        return torch.device("cuda" if torch.cuda.is_available() else "cpu")
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def feature_masks(n_trees: int, n_feat: int, colsample: float, seed: int) -> np.ndarray:
    """Per-tree column masks for ``colsample_bytree`` (all ones when 1.0)."""
    m = np.ones((n_trees, n_feat), dtype=np.uint8)
    if colsample >= 1.0:
        return m
    k = max(1, int(math.floor(colsample * n_feat)))
    rng = np.random.default_rng(seed + 0x5EED)
    for t in range(n_trees):
        m[t] = 0
        m[t, rng.choice(n_feat, size=k, replace=False)] = 1
    return m


@dataclass
class BinnedData:
    """A quantised training matrix: cuts + bins, reusable across fits on the same rows (RFE steps,
    search candidates). GPU: row records [N, stride] + feature-major bins [F, N]; host: uint8 [N, F]."""
    device: torch.device
    n_rows: int
    n_rows_global: int
    n_features: int
    row_offset: int
    cuts: torch.Tensor
    nbins: torch.Tensor
    records: torch.Tensor | None = None
    binsT: torch.Tensor | None = None
    bins_host: np.ndarray | None = None
    t_sketch: float = 0.0
    t_bin: float = 0.0


def _allreduce_max_flags(flags: torch.Tensor, dist, dev) -> torch.Tensor:
    t = flags.to(torch.float32).to(dist._coll_device(dev))
    dist.allreduce(t, "max")
    return t.to(dev) > 0


def _summary_cuts(samp: torch.Tensor, wsamp: torch.Tensor | None, max_bin: int, has_missing: torch.Tensor,
                  dist, dev, on_device: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """sketch_mode="summary": every rank summarises its own sample, the summaries are all-gathered
    (a few KB per feature instead of the raw rows) and merged identically on every rank. Integer
    weights are scaled by the GLOBAL max weight, so one unit means the same weight on every rank.
    ``on_device``: the summary is built where the sample lives (:func:`sketch.device_summary`; the
    full-data sketch), else by the host :class:`sketch.QuantileSummary`."""
    w_max = None
    if wsamp is not None:
        w_max = float(wsamp.max()) if wsamp.numel() else 0.0
        if dist is not None and dist.world > 1:
            w_max = dist.allreduce_scalar(w_max, "max", dev)
        w_max = w_max if w_max > 0 else 1.0
    if on_device:
        off, vals, wts = sketch.device_summary(samp, wsamp, w_max=w_max)
    else:
        summ = sketch.QuantileSummary.build(samp.cpu().numpy(), None if wsamp is None else wsamp.cpu().numpy(),
                                            w_max=w_max)
        off, vals, wts, _ = summ.to_arrays()
    if dist is not None and dist.world > 1:
        per = int(dist.allreduce_scalar(float(len(vals)), "max", dev))  # common padded length
        ent = torch.full((per, 2), float("nan"), dtype=torch.float64)
        ent[: len(vals), 0] = torch.from_numpy(vals.astype(np.float64))
        ent[: len(vals), 1] = torch.from_numpy(wts.astype(np.float64))
        offs = torch.from_numpy(off.astype(np.float64))[:, None]
        all_ent = dist.allgather_rows(ent.to(dist._coll_device(dev))).cpu().numpy()
        all_off = dist.allgather_rows(offs.to(dist._coll_device(dev))).cpu().numpy()[:, 0].astype(np.int64)
        F1 = len(off)
        parts = []
        for r in range(dist.world):
            o = all_off[r * F1:(r + 1) * F1]
            e = all_ent[r * per:r * per + int(o[-1])]
            parts.append(sketch.QuantileSummary.from_arrays(o, e[:, 0].astype(np.float32), e[:, 1].astype(np.int64),
                                                            np.zeros(F1 - 1, dtype=bool)))
        summ = sketch.QuantileSummary.merge(parts)
    else:
        summ = sketch.QuantileSummary.from_arrays(off, vals, wts, np.zeros(len(off) - 1, dtype=bool))
    summ.has_missing = has_missing.cpu().numpy().astype(bool)
    c, nb = summ.cuts(max_bin)
    return torch.from_numpy(c).to(dev), torch.from_numpy(nb).to(dev)


SKETCH_AUTO = -1
SKETCH_SAMPLE_ROWS = 1 << 18


def resolve_sketch_rows(sketch_rows: int | None, dev, n_rows_global: int | None = None) -> int | None:
    """SKETCH_AUTO -> None (every row, the device sketch) on a CUDA device above 2^18 rows; the
    2^18-row sample elsewhere (up to 2^18 rows that sample IS every row, by the cheaper full sort)."""
    if sketch_rows is not None and sketch_rows < 0:
        big = n_rows_global is None or n_rows_global > SKETCH_SAMPLE_ROWS
        return None if (torch.device(dev).type == "cuda" and big) else SKETCH_SAMPLE_ROWS
    return sketch_rows


def bin_dataset(X, *, max_bin: int = 256, sketch_rows: int | None = SKETCH_AUTO, device=None, dist=None,
                n_rows_global: int | None = None, row_offset: int = 0, sketch_weights=None,
                sketch_mode: str = "sample") -> BinnedData:
    """Weighted quantile sketch (K12) on a global strided sample + binning (K13).

    ``sketch_rows`` None / 0: every row (XGBoost ``hist`` sketches all rows), exact weighted quantiles.
    On a GPU this is the bucketed device sketch (``sketch.device_exact_cuts``): under data parallelism
    its bucket histograms are all-reduced and the target buckets' candidates all-gathered, so every rank
    gets the full data's cuts without gathering the raw rows. On the CPU under data parallelism each
    rank summarises its shard and the summaries are merged (``sketch_mode="summary"``).
    ``sketch_weights`` ([N_local], optional): per-row sketch weights (see models/sketch.py).
    A feature gets 256 bins only if it has no missing value in the FULL data (all ranks).
    ``SKETCH_AUTO``: every row on a GPU, the 2^18-row sample on the CPU."""
    dev = _resolve_device(device, X)
    world = dist.world if dist is not None else 1
    Xt = _to_tensor(X, dev)
    N, F = Xt.shape
    n_glob = n_rows_global if n_rows_global is not None else (
        int(dist.allreduce_scalar(N, "sum", dev)) if world > 1 else N)
    sketch_rows = resolve_sketch_rows(sketch_rows, dev, n_glob)
    ts = time.perf_counter()
    has_missing = torch.isnan(Xt).any(0) if N else torch.zeros(F, dtype=torch.bool, device=dev)
    full = not sketch_rows
    if full and dev.type == "cuda" and sketch_mode != "summary":
        # every row, exactly (csrc/sketch.hip: bucket histograms + per-bucket selection, no row sort;
        # under data parallelism four device all-reduces -- the missing flags ride in the first -- so
        # the cuts are the full data's)
        sw = _to_tensor(sketch_weights, dev).reshape(-1) if sketch_weights is not None else None
        cuts, nbins = sketch.device_exact_cuts(Xt, max_bin, sw, has_missing if world == 1 else None,
                                               dist=dist if world > 1 else None, row_offset=row_offset,
                                               n_rows_global=n_glob)
        torch.cuda.synchronize(dev)
        t_sketch = time.perf_counter() - ts
        tb = time.perf_counter()
        bd = BinnedData(dev, N, n_glob, F, row_offset, cuts, nbins, t_sketch=t_sketch)
        _bin_device(bd, Xt, cuts, nbins)
        torch.cuda.synchronize(dev)
        bd.t_bin = time.perf_counter() - tb
        return bd
    if world > 1:
        has_missing = _allreduce_max_flags(has_missing, dist, dev)
    stride = 1 if full else sketch.sample_stride(n_glob, sketch_rows)
    samp = sketch.local_sample(Xt, row_offset, stride)
    wsamp = None
    if sketch_weights is not None:
        wsamp = sketch.local_sample(_to_tensor(sketch_weights, dev).reshape(-1, 1), row_offset, stride)[:, 0]
    if sketch_mode == "summary" or (full and world > 1):
        cuts, nbins = _summary_cuts(samp, wsamp, max_bin, has_missing, dist, dev, on_device=full)
    else:
        if world > 1:
            samp = dist.allgather_rows(samp)
            if wsamp is not None:
                wsamp = dist.allgather_rows(wsamp.reshape(-1, 1), pad_value=0.0)[:, 0]
        cuts, nbins = sketch.compute_cuts(samp, max_bin, wsamp, has_missing)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t_sketch = time.perf_counter() - ts
    tb = time.perf_counter()
    bd = BinnedData(dev, N, n_glob, F, row_offset, cuts, nbins, t_sketch=t_sketch)
    if dev.type == "cuda":
        _bin_device(bd, Xt, cuts, nbins)
        torch.cuda.synchronize(dev)
    else:
        bd.bins_host = sketch.bin_matrix_host(Xt.cpu().numpy(), cuts.cpu().numpy(), nbins.cpu().numpy())
    bd.t_bin = time.perf_counter() - tb
    return bd


def _bin_device(bd: BinnedData, Xt: torch.Tensor, cuts: torch.Tensor, nbins: torch.Tensor) -> None:
    """Binning on the GPU: row records (32 bytes for <= 24 features) + feature-major bins.
    (Packed 16-byte records were measured slower in round 5 -- the per-feature bit-field extracts cost
    the histogram gathers more than the halved bytes saved: profiles/round5/packed_vs_32byte.txt.)"""
    from ..ops import gbdt_ops

    bd.records, bd.binsT = gbdt_ops.bin_matrix(Xt, cuts, nbins)


def sketch_weights_for(params: "GBDTParams", y, sample_weight=None, device=None):
    """Per-row sketch weights for ``params.sketch_weight`` (None = unweighted)."""
    mode = getattr(params, "sketch_weight", "sample")
    if mode == "sample":
        return sample_weight
    if mode != "hessian":
        raise ValueError(f"sketch_weight must be 'sample' or 'hessian', got {mode!r}")
    yt = _to_tensor(y, device).reshape(-1)
    w = _to_tensor(sample_weight, device).reshape(-1) if sample_weight is not None else torch.ones_like(yt)
    spw = float(params.scale_pos_weight if params.scale_pos_weight is not None else 1.0)
    return w * torch.where(yt == 1.0, torch.tensor(spw, device=yt.device), torch.tensor(1.0, device=yt.device))


def subset_rows(bd: BinnedData, rows: np.ndarray) -> BinnedData:
    """Rows ``rows`` of a binned matrix with the same cuts (CV folds re-use one binning)."""
    idx = torch.as_tensor(np.asarray(rows, dtype=np.int64), device=bd.device)
    out = BinnedData(bd.device, len(rows), len(rows), bd.n_features, 0, bd.cuts, bd.nbins)
    if bd.records is not None:
        out.records = bd.records.index_select(0, idx).contiguous()
        out.binsT = bd.binsT.index_select(1, idx).contiguous()
    else:
        out.bins_host = bd.bins_host[np.asarray(rows)]
    return out


def subset_features(bd: BinnedData, feats) -> BinnedData:
    """The binned matrix restricted to the feature columns ``feats`` (ascending indices), repacked:
    row records of the narrower width (32 bytes for <= 24 features: the fused fast path) and the
    matching feature-major rows -- a device gather of ``N x len(feats)`` bytes, no re-sketch (cuts
    are per feature). A fit on it grows exactly the trees of a ``feature_mask`` fit on ``bd``
    (same bins, same colsample draws, same tie order), at the cost of the narrower matrix."""
    f = np.asarray(feats, dtype=np.int64)
    idx = torch.as_tensor(f, device=bd.device)
    out = BinnedData(bd.device, bd.n_rows, bd.n_rows_global, len(f), bd.row_offset,
                     bd.cuts.index_select(0, idx).contiguous(), bd.nbins.index_select(0, idx).contiguous())
    if bd.records is not None:
        from ..ops import gbdt_ops

        rec = torch.zeros((bd.n_rows, gbdt_ops.row_stride(len(f))), dtype=torch.uint8, device=bd.device)
        rec[:, : len(f)] = bd.records.index_select(1, idx)
        out.records = rec
        out.binsT = bd.binsT.index_select(0, idx).contiguous()
    else:
        out.bins_host = np.ascontiguousarray(bd.bins_host[:, f])
    return out


def expand_features(bst: Booster, feats, n_features: int, feature_names: Sequence[str] | None = None,
                    feature_types: Sequence[str] | None = None, monotone_constraints=None,
                    interaction_constraints=None) -> Booster:
    """A booster fitted on :func:`subset_features` columns, re-expressed over the full feature space
    (split indices mapped back; leaves keep index 0 as XGBoost writes them). Its monotone constraints go
    back to full width: ``monotone_constraints`` (the full vector) when given, else the subset's entries
    at ``feats`` and 0 elsewhere. Likewise its interaction constraints: ``interaction_constraints`` (the
    full-width groups) when given, else the subset's groups with their indices mapped back."""
    from .booster import Tree

    f = np.asarray(feats, dtype=np.int32)
    trees = []
    for t in bst.trees:
        si = np.where(t.left_children != -1, f[t.split_indices], 0).astype(np.int32)
        trees.append(Tree(t.left_children, t.right_children, t.parents, si, t.split_conditions, t.default_left,
                          t.base_weights, t.loss_changes, t.sum_hessian))
    tparams = dict(bst.train_params)
    if monotone_constraints is not None:
        tparams["monotone_constraints"] = tuple(int(c) for c in monotone_constraints)
    elif bst.monotone_constraints is not None:
        full = np.zeros(int(n_features), dtype=np.int8)
        full[f] = bst.monotone_constraints
        tparams["monotone_constraints"] = tuple(int(c) for c in full)
    if interaction_constraints is not None:
        tparams["interaction_constraints"] = [[int(i) for i in g] for g in interaction_constraints]
    elif bst.interaction_constraints is not None:
        tparams["interaction_constraints"] = [[int(f[i]) for i in g] for g in bst.interaction_constraints]
    return Booster(trees, list(feature_names) if feature_names is not None else None,
                   list(feature_types) if feature_types is not None else None, bst.base_score, int(n_features),
                   bst.objective, tparams, dict(bst.attributes))


def resolve_monotone(mc, n_features: int, feature_names: Sequence[str] | None = None) -> np.ndarray | None:
    """``monotone_constraints`` in any accepted form -> int8 [n_features] in {-1, 0, +1}, or None for an
    unconstrained fit (None, an empty form, all zeros). ``ValueError``: a length other than the feature
    count, a value outside {-1, 0, 1}, a dict without feature names or with an unknown name."""
    if mc is None:
        return None
    if isinstance(mc, dict):
        if not mc:
            return None
        if feature_names is None:
            raise ValueError("monotone_constraints given by feature name needs feature_names")
        names = [str(n) for n in feature_names]
        unknown = [k for k in mc if str(k) not in names]
        if unknown:
            raise ValueError(f"monotone_constraints names unknown features: {unknown}")
        vals = [0] * len(names)
        for k, v in mc.items():
            vals[names.index(str(k))] = v
    else:
        vals = _mono_plain(mc)
        if not vals:
            return None
    if len(vals) != n_features:
        raise ValueError(f"monotone_constraints has {len(vals)} entries, the data has {n_features} features")
    bad = [v for v in vals if isinstance(v, bool) or v not in (-1, 0, 1)]
    if bad:
        raise ValueError(f"monotone_constraints values must be -1, 0 or 1 (got {bad[0]!r})")
    vec = np.asarray([int(v) for v in vals], dtype=np.int8)
    return vec if vec.any() else None


def _refuse_monotone(params: "GBDTParams", what: str) -> None:
    """Constrained fits run on one device, in core: every other trainer refuses the argument by name."""
    mc = getattr(params, "monotone_constraints", None)
    if mc is None:
        return
    plain = _mono_plain(mc)
    if any(mc.values()) if plain is None else any(plain):
        raise ValueError(f"monotone_constraints is not supported {what}")


def _mono_plain(mc) -> list | None:
    """The sequence / string forms as a plain list (None for a dict)."""
    from .booster import parse_monotone_string

    if isinstance(mc, dict):
        return None
    if isinstance(mc, str):
        return list(parse_monotone_string(mc))
    return list(np.asarray(mc).reshape(-1).tolist())


GPU_MAX_INTERACTION_GROUPS = 64  # one bit per group in the device's 64-bit group words (csrc/gbdt.hip InterDev)


def _inter_plain(ic) -> list:
    """``interaction_constraints`` as a list of lists of raw entries (the string form parsed as JSON)."""
    if ic is None:
        return []
    if isinstance(ic, str):
        if not ic.strip():
            return []
        try:
            ic = json.loads(ic)
        except ValueError:
            raise ValueError(f"interaction_constraints: cannot parse {ic!r} (expected a form like "
                             "'[[0, 1], [2, 3]]')") from None
    if isinstance(ic, (dict, str, bytes)) or not hasattr(ic, "__iter__"):
        raise ValueError("interaction_constraints must be a list of lists of feature indices or names")
    groups = []
    for g in ic:
        if isinstance(g, (dict, str, bytes)) or not hasattr(g, "__iter__"):
            raise ValueError(f"interaction_constraints: every group is a list of features (got {g!r})")
        groups.append(list(g))
    return groups


def resolve_interaction(ic, n_features: int, feature_names: Sequence[str] | None = None, *,
                        max_groups: int | None = None) -> list[list[int]] | None:
    """``interaction_constraints`` in any accepted form (a list of lists of feature indices or of feature
    names, XGBoost's string / JSON form ``"[[0, 1], [2, 3]]"``) -> the canonical groups: index lists, each
    sorted and without duplicates, empty groups dropped; None for an unconstrained fit (None, ``[]``, ``""``,
    ``"[]"``, only empty groups). A non-empty constraint is never simplified away: one group holding every
    feature stays a constraint. ``ValueError``: an index out of range, an entry that is neither an integer
    nor a name (bools and floats included), a name without feature names or an unknown one, more than
    ``max_groups`` groups (the GPU trainer's 64)."""
    names = [str(n) for n in feature_names] if feature_names is not None else None
    out = []
    for g in _inter_plain(ic):
        idx = set()
        for e in g:
            if isinstance(e, str):
                if names is None:
                    raise ValueError(f"interaction_constraints given by feature name ({e!r}) needs feature_names")
                if e not in names:
                    raise ValueError(f"interaction_constraints names an unknown feature: {e!r}")
                idx.add(names.index(e))
            elif isinstance(e, (bool, np.bool_)) or not isinstance(e, (int, np.integer)):
                raise ValueError(f"interaction_constraints entries must be feature indices or names (got {e!r})")
            elif not 0 <= int(e) < n_features:
                raise ValueError(f"interaction_constraints index {int(e)} is out of range for {n_features} features")
            else:
                idx.add(int(e))
        if idx:
            out.append(sorted(idx))
    if not out:
        return None
    if max_groups is not None and len(out) > max_groups:
        raise ValueError(f"interaction_constraints has {len(out)} groups; the GPU trainer supports at most "
                         f"{max_groups} (fit on the CPU for more)")
    return out


def _refuse_interaction(params: "GBDTParams", what: str) -> None:
    """As :func:`_refuse_monotone`: every trainer but the in-core, one-device one refuses the argument by name."""
    if any(len(g) for g in _inter_plain(getattr(params, "interaction_constraints", None))):
        raise ValueError(f"interaction_constraints is not supported {what}")


def subset_interaction(groups: list[list[int]] | None, feats) -> list[list[int]] | None:
    """Full-width groups restricted to the surviving features ``feats`` (ascending full-width indices) and
    renumbered to their positions. Groups that become empty are dropped; a group that shrinks to one
    feature stays (a singleton is not the same as ungrouped). None when no group survives."""
    if groups is None:
        return None
    pos = {int(f): i for i, f in enumerate(np.asarray(feats).reshape(-1).tolist())}
    out = [sorted(pos[f] for f in g if f in pos) for g in groups]
    return [g for g in out if g] or None


def interaction_words(groups: list[list[int]], n_features: int) -> np.ndarray:
    """The device's form of the groups: uint64 [n_features], bit k of word f set iff f is in group k."""
    w = np.zeros(int(n_features), dtype=np.uint64)
    for k, g in enumerate(groups):
        w[np.asarray(g, dtype=np.int64)] |= np.uint64(1) << np.uint64(k)
    return w


# COBALT_ROW_REORDER=auto: the schedule by local row count (docs/PERF.md "Row reorder")
# (same-box A/B against the parent, profiles/round7/ab_row_reorder.txt: 10M rows 222.8 -> 206.0 ms per fit,
# 5M 142.6 -> 136.7, 2.5M 99.6 -> 95.6, 1.25M 73.4 -> 71.5; below 1M rows not measured: off)
ROW_REORDER_AUTO: list[tuple[int, str]] = [(1_000_000, "0"), (8_000_000, "0,8,32,128")]  # (min rows, schedule)


def resolve_row_reorder(spec, n_trees: int, n_rows: int) -> list[int]:
    """Tree indices after which the rows are regrouped (sorted, < n_trees - 1: a reorder after the last
    tree serves nothing). ``spec``: None (the COBALT_ROW_REORDER knob), a sequence of tree indices, an int
    period (0: off) or "0,8,32" / "every:16" / "off" / "" / "auto"."""
    if spec is None:
        spec = knob("COBALT_ROW_REORDER", "auto")
    if isinstance(spec, str):
        s = spec.strip().lower()
        if s == "auto":
            s = "off"
            for min_rows, sched in ROW_REORDER_AUTO:
                if n_rows >= min_rows:
                    s = sched
        if s in ("", "off"):
            return []
        spec = int(s[6:]) if s.startswith("every:") else [int(t) for t in s.split(",") if t.strip()]
    if isinstance(spec, (int, np.integer)):
        spec = range(0, n_trees, int(spec)) if int(spec) > 0 else []
    out = sorted({int(t) for t in spec})
    if out and out[0] < 0:
        raise ValueError("row_reorder: tree indices must be >= 0")
    return [t for t in out if t < n_trees - 1]


def check_grad_bits(grad_bits: int, n_features: int, device_type: str) -> None:
    """``grad_bits`` is 17 or 25; the GPU's wide (25-bit) cells need the 32-byte row records of <= 24
    features (csrc/gbdt.hip cobalt_gbdt_create refuses the rest with -6)."""
    if grad_bits not in gbdt_host.GRAD_BITS:
        raise ValueError(f"grad_bits must be one of {gbdt_host.GRAD_BITS}")
    if grad_bits > 17 and device_type == "cuda" and n_features > 24:
        raise ValueError(f"grad_bits={grad_bits} on the GPU supports <= 24 features (32-byte row records); "
                         f"got {n_features}: use grad_bits=17")


def check_gpu_shape(max_depth: int, n_rows: int) -> None:
    """The GPU trainer's limits (csrc/gbdt.hip cobalt_gbdt_create: -1 / -5), named before any device work."""
    if not 1 <= max_depth <= 10:
        raise ValueError(f"the GPU trainer supports max_depth 1-10 (got {max_depth}); use the host trainer "
                         "(device='cpu') for deeper trees")
    if n_rows >= (1 << 31) - 1:
        raise ValueError(f"{n_rows} rows exceed one GPU fit's int32 row ids: shard them over ranks "
                         "(data parallel) or stream them (models.external.train_external)")


class EvalMonitor:
    """The validation sets of one fit: their per-round metric curves and XGBoost's early-stopping rule.

    ``evals`` = ``[(X_val, y_val[, w_val]), ...]`` (raw float32 features; never binned). The trainer hands
    over the new trees segment by segment (:meth:`add_trees`); every set's margins are carried forward,
    so each tree is walked once per validation row (``Booster.eval_curve``). The LAST set and the LAST
    metric drive early stopping: the best round moves on a strict improvement ("logloss" / "error"
    minimised, "auc" maximised) and the fit stops at the first round ``r`` with ``r - best >=
    early_stopping_rounds``. ``scale_pos_weight`` does not enter the metrics."""

    def __init__(self, evals, eval_metric=None, early_stopping_rounds: int | None = None, device=None,
                 n_features: int | None = None, verbose: bool = False):
        from .booster import check_eval_inputs

        if early_stopping_rounds is not None and int(early_stopping_rounds) < 1:
            raise ValueError("early_stopping_rounds must be >= 1")
        self.rounds = int(early_stopping_rounds) if early_stopping_rounds is not None else None
        if eval_metric is None:
            eval_metric = ["logloss"]
        self.metrics = [eval_metric] if isinstance(eval_metric, str) else list(eval_metric)
        if not self.metrics:
            raise ValueError("eval_metric is empty")
        self.dev = torch.device(device) if device is not None else torch.device("cpu")
        self.verbose = bool(verbose)
        self.sets = []
        for i, ev in enumerate(evals):
            if not isinstance(ev, (tuple, list)) or len(ev) not in (2, 3):
                raise ValueError(f"evals[{i}] must be (X, y) or (X, y, sample_weight)")
            Xv = _to_tensor(ev[0], self.dev)
            if Xv.ndim != 2 or (n_features is not None and Xv.shape[1] != n_features):
                raise ValueError(f"evals[{i}]: X has shape {tuple(Xv.shape)}, the training data has "
                                 f"{n_features} features")
            yv = _to_tensor(ev[1], "cpu").reshape(-1).numpy()
            wv = _to_tensor(ev[2], "cpu").reshape(-1).numpy() if len(ev) == 3 and ev[2] is not None else None
            check_eval_inputs(int(Xv.shape[0]), yv, wv, self.metrics)
            self.sets.append((Xv if self.dev.type == "cuda" else Xv.numpy(), yv, wv))
        self.margins: list = [None] * len(self.sets)
        self.curves = [{m: [] for m in self.metrics} for _ in self.sets]
        self.best: int | None = None
        self.best_score: float | None = None
        self.stopped: int | None = None   # global index of the round at which the rule fired

    def start_from(self, init_booster: Booster) -> None:
        """The sets' margins under the model that boosting continues from (one pass over its trees)."""
        self.margins = [init_booster.predict_margin(Xv, device=self.dev) for Xv, _, _ in self.sets]

    def add_trees(self, segment: Booster, first_round: int) -> int | None:
        """Score the trees of ``segment`` (global rounds ``first_round ...``) on every set and apply the
        rule round by round; returns the round at which the fit stops (it keeps trees 0..that round)."""
        from .booster import EVAL_MAXIMIZE

        got = []
        for i, (Xv, yv, wv) in enumerate(self.sets):
            curve, self.margins[i] = segment.eval_curve(Xv, yv, wv, self.metrics, device=self.dev,
                                                        margin=self.margins[i])
            got.append(curve)
        keep = segment.num_trees
        if self.rounds is not None:
            drive, bigger = got[-1][self.metrics[-1]], EVAL_MAXIMIZE[self.metrics[-1]]
            for j in range(segment.num_trees):
                r, s = first_round + j, float(drive[j])
                if self.best is None or (s > self.best_score if bigger else s < self.best_score):
                    self.best, self.best_score = r, s
                elif r - self.best >= self.rounds:
                    self.stopped, keep = r, j + 1
                    break
        for i, curve in enumerate(got):
            for m in self.metrics:
                self.curves[i][m].extend(float(v) for v in curve[m][:keep])
            if self.verbose:
                for j in range(keep):
                    print(f"[{first_round + j}]\t" + "\t".join(
                        f"validation_{k}-{m}:{got[k][m][j]:.5f}" for k in range(len(got)) for m in self.metrics))
        return self.stopped

    def result(self) -> dict[str, dict[str, list[float]]]:
        return {f"validation_{i}": {m: list(v) for m, v in c.items()} for i, c in enumerate(self.curves)}


def _eval_monitor(evals, eval_metric, early_stopping_rounds, dev, n_features, dist, checkpointing: bool,
                  verbose: bool = False) -> EvalMonitor | None:
    """The fit's :class:`EvalMonitor` (None without ``evals``); everything unsupported is refused here,
    before any device work or collective."""
    if isinstance(evals, EvalMonitor):
        return evals
    if not evals:
        if early_stopping_rounds is not None:
            raise ValueError("early_stopping_rounds needs at least one validation set (evals / eval_set)")
        return None
    if dist is not None and dist.world > 1:
        raise ValueError("evals are not supported in data-parallel fits (dist.world > 1)")
    if early_stopping_rounds is not None and checkpointing:
        raise ValueError("early_stopping_rounds cannot be combined with checkpoint_path")
    return EvalMonitor(evals, eval_metric, early_stopping_rounds, dev, n_features, verbose)


def train(X, y, params: GBDTParams | dict | None = None, *, sample_weight=None, device=None,
          feature_names: Sequence[str] | None = None, feature_types: Sequence[str] | None = None,
          dist=None, n_rows_global: int | None = None, row_offset: int = 0,
          report: FitReport | None = None, init_booster: Booster | None = None,
          checkpoint_path: str | None = None, checkpoint_every: int = 0, resume: bool = True,
          exact_fp64: bool = False, evals=None, eval_metric=None, early_stopping_rounds: int | None = None,
          evals_result: dict | None = None, es_segment: int | None = None, verbose_eval: bool = False) -> Booster:
    """Fit a binary:logistic GBDT. With ``dist`` (a :class:`~..parallel.dist.DistContext`) each rank
    passes its local row shard (``row_offset`` = global index of its first row).

    ``init_booster`` continues boosting from an existing model for ``n_estimators`` MORE trees
    (XGBoost's ``xgb_model=``). ``checkpoint_path`` + ``checkpoint_every`` write the model every that
    many trees (atomic replace, rank 0); with ``resume`` an existing checkpoint there is loaded and
    training continues to ``n_estimators`` trees in total -- bit-identical to an uninterrupted fit,
    because sampling is keyed by the global tree index and the margins are re-predicted in tree order.

    ``exact_fp64`` (CPU only): unquantised fp64 gradients and histograms -- the accuracy reference of
    the fixed-point trainer (tests/test_quantization.py).

    ``evals`` = ``[(X_val, y_val[, w_val]), ...]`` + ``eval_metric`` ("logloss" (default), "error", "auc", or
    a list) record the metrics after every new round into ``evals_result`` (``{"validation_0": {metric:
    [...]}, ...}``); ``early_stopping_rounds`` stops the fit by XGBoost's rule on the last set's last metric
    (:class:`EvalMonitor`) and stores ``best_iteration`` / ``best_score`` in the model's attributes. The
    early-stopped model is a byte-identical prefix of the full fit; a fit without ``evals`` is untouched.
    ``es_segment``: trees grown between two looks at the curve (default ``early_stopping_rounds``: the rule
    cannot fire sooner than that many rounds after the best one, so at most that many trees minus one are
    grown in vain); it does not change the result. Not supported (``ValueError``): data-parallel fits,
    ``early_stopping_rounds`` with ``checkpoint_path``."""
    if params is None:
        params = GBDTParams()
    elif isinstance(params, dict):
        params = GBDTParams.from_kwargs(**params)
    t0 = time.perf_counter()
    if dist is not None:
        _refuse_monotone(params, "in data-parallel fits (dist)")
        _refuse_interaction(params, "in data-parallel fits (dist)")
    evals = _eval_monitor(evals, eval_metric, early_stopping_rounds, _resolve_device(device, X), int(X.shape[1]),
                          dist, checkpoint_path is not None, verbose_eval)
    ckpt = Checkpointer(checkpoint_path, checkpoint_every, params, dist) if checkpoint_path else None
    total = None
    if ckpt is not None and resume and init_booster is None:
        init_booster = ckpt.load()
        if init_booster is not None:
            total = int(params.n_estimators)
            log.info("resuming from %s at tree %d of %d", checkpoint_path, init_booster.num_trees, total)
    dev = _resolve_device(device, X)
    # the trainer's shape limits, before the sketch (and its data-parallel collectives) and the binning;
    # train_binned checks them again for pre-binned inputs
    check_grad_bits(int(params.grad_bits), int(X.shape[1]), dev.type)
    if dev.type == "cuda":
        check_gpu_shape(int(params.max_depth), int(X.shape[0]))
    # (the constraint's form and the GPU's group limit too: a refusal comes before any device work)
    resolve_interaction(params.interaction_constraints, int(X.shape[1]), feature_names if feature_names is not None
                        else (init_booster.feature_names if init_booster is not None else None),
                        max_groups=GPU_MAX_INTERACTION_GROUPS if dev.type == "cuda" else None)
    init_margin = None
    if init_booster is not None:
        from ..ops import predict_ops

        Xt = _to_tensor(X, dev)
        init_margin = predict_ops.predict_margin(init_booster, Xt, dev)
        if not isinstance(init_margin, torch.Tensor):
            init_margin = torch.as_tensor(init_margin)
        init_margin = init_margin.to(dev, torch.float32).contiguous()
    bd = bin_dataset(X, max_bin=params.max_bin, sketch_rows=params.sketch_rows, device=device, dist=dist,
                     n_rows_global=n_rows_global, row_offset=row_offset,
                     sketch_weights=sketch_weights_for(params, y, sample_weight, dev),
                     sketch_mode=params.sketch_mode)
    bst = train_binned(bd, y, params, sample_weight=sample_weight, feature_names=feature_names,
                       feature_types=feature_types, dist=dist, report=report, init_booster=init_booster,
                       init_margin=init_margin, total_trees=total, checkpoint=ckpt, exact_fp64=exact_fp64,
                       evals=evals, evals_result=evals_result, es_segment=es_segment)
    if report is not None:
        report.t_total = time.perf_counter() - t0
    return bst


def train_binned(bd: BinnedData, y, params: GBDTParams | dict | None = None, *, sample_weight=None,
                 feature_names: Sequence[str] | None = None, feature_types: Sequence[str] | None = None,
                 feature_mask: np.ndarray | None = None, dist=None, report: FitReport | None = None,
                 init_booster: Booster | None = None, init_margin: torch.Tensor | None = None,
                 total_trees: int | None = None, checkpoint: "Checkpointer | None" = None,
                 exact_fp64: bool = False, evals=None, eval_metric=None, early_stopping_rounds: int | None = None,
                 evals_result: dict | None = None, es_segment: int | None = None) -> Booster:
    """Boost on pre-binned data. ``feature_mask`` (bool [F]) restricts the fit to a feature subset
    (the trees still index the full feature space, so a subset fit costs no re-binning).
    ``init_booster`` + ``init_margin`` (its margins on these rows) continue an existing model: grow
    ``total_trees - init_booster.num_trees`` trees (default ``n_estimators`` more).
    ``evals`` / ``eval_metric`` / ``early_stopping_rounds`` / ``evals_result`` / ``es_segment``: see
    :func:`train` (with ``init_booster`` the curves cover the new rounds; ``best_iteration`` is a global
    tree index)."""
    if params is None:
        params = GBDTParams()
    elif isinstance(params, dict):
        params = GBDTParams.from_kwargs(**params)
    dev = bd.device
    world = dist.world if dist is not None else 1
    mon = _eval_monitor(evals, eval_metric, early_stopping_rounds, dev, bd.n_features, dist, checkpoint is not None)
    early = mon is not None and mon.rounds is not None
    if es_segment is not None and int(es_segment) < 1:
        raise ValueError("es_segment must be >= 1")
    grad_bits = int(params.grad_bits)
    N, F = bd.n_rows, bd.n_features
    if dist is not None:
        _refuse_monotone(params, "in data-parallel fits (dist)")
        _refuse_interaction(params, "in data-parallel fits (dist)")
    mono = resolve_monotone(params.monotone_constraints, F, feature_names if feature_names is not None else (
        init_booster.feature_names if init_booster is not None else None))
    inter = resolve_interaction(params.interaction_constraints, F, feature_names if feature_names is not None else (
        init_booster.feature_names if init_booster is not None else None),
        max_groups=GPU_MAX_INTERACTION_GROUPS if dev.type == "cuda" else None)
    check_grad_bits(grad_bits, F, dev.type)
    if dev.type == "cuda":
        check_gpu_shape(int(params.max_depth), N)
    rep = report if report is not None else FitReport()
    tp = rep.mark("pre", time.perf_counter(), dev)
    yt = _to_tensor(y, dev).reshape(-1)
    if yt.shape[0] != N:
        raise ValueError("X and y row counts differ")
    spw = float(params.scale_pos_weight if params.scale_pos_weight is not None else 1.0)
    # (python scalars, not device tensors: no host-to-device copies; the same float32 values)
    pw = torch.where(yt == 1.0, spw, 1.0).to(torch.float32)
    wt = (_to_tensor(sample_weight, dev).reshape(-1) * pw) if sample_weight is not None else pw
    wt = wt.to(torch.float32).contiguous()

    T0 = init_booster.num_trees if init_booster is not None else 0
    if init_booster is not None and init_margin is None:
        raise ValueError("init_booster needs init_margin (its margins on the training rows)")
    if mon is not None and T0:
        mon.start_from(init_booster)
    # base score = weighted label mean (XGBoost boost_from_average for binary:logistic) and the largest
    # weight (the fixed-point scales); under data parallelism both in ONE collective: [sum w, sum w y,
    # every rank's max weight in its own slot] summed on the device
    need_bs = init_booster is None and params.base_score is None
    labels_binary = None  # known after the one-rank read below
    if world > 1:
        buf = torch.zeros(2 + world, dtype=torch.float64, device=dev)
        if need_bs:
            buf[0] = wt.double().sum()
            buf[1] = (wt.double() * yt.double()).sum()
        if N:
            buf[2 + dist.rank] = wt.max().double()
        if hasattr(dist, "device_allreduce") and dev.type == "cuda":
            dist.device_allreduce(buf, "sum")
        else:
            t = buf.to(dist._coll_device(dev))
            dist.allreduce(t, "sum")
            buf = t.to(dev)
        sw, swy, wmax = (float(v) for v in (buf[0], buf[1], buf[2:].max()))
    else:  # one device -> host read for the three (and whether the labels are 0 / 1, for the trainer)
        wd = wt.double()
        z = torch.zeros((), dtype=torch.float64, device=dev)
        sw, swy, wmax, y01 = torch.stack([wd.sum() if need_bs else z, (wd * yt.double()).sum() if need_bs else z,
                                          wd.max() if N else z + 1.0,
                                          ((yt == 0) | (yt == 1)).all().double()]).tolist()
        labels_binary = y01 != 0.0
    if init_booster is not None:
        base_score = float(init_booster.base_score)
    elif params.base_score is None:
        base_score = min(max(swy / sw if sw > 0 else 0.5, 1e-6), 1 - 1e-6)
    else:
        base_score = float(params.base_score)
    base_score = float(np.float32(base_score))
    base_margin = Booster([], base_score=base_score, num_feature=F).base_margin
    gscale, hscale = gbdt_host.quant_scales(wmax, grad_bits)

    T_new = (int(total_trees) - T0) if total_trees is not None else int(params.n_estimators)
    if T_new < 0:
        raise ValueError("the initial model already has more trees than requested")
    T = T0 + T_new  # global tree indices [T0, T) are grown; masks/RNG are keyed by the global index
    fmask_np = feature_masks(T, F, float(params.colsample_bytree), int(params.random_state))
    if feature_mask is not None:
        fm_sub = np.asarray(feature_mask, dtype=bool)
        active = np.nonzero(fm_sub)[0]
        fmask_np = np.zeros((T, F), dtype=np.uint8)
        sub = feature_masks(T, len(active), float(params.colsample_bytree), int(params.random_state))
        fmask_np[:, active] = sub
    seg = checkpoint.every if checkpoint is not None and checkpoint.every > 0 else max(T_new, 1)
    if early:  # grow a segment, look at the validation curve, stop or go on
        seg = int(es_segment) if es_segment is not None else mon.rounds
    trees_so_far = list(init_booster.trees) if init_booster is not None else []
    names = list(feature_names) if feature_names is not None else (
        list(init_booster.feature_names) if init_booster is not None and init_booster.feature_names else None)
    ftypes = list(feature_types) if feature_types is not None else (
        list(init_booster.feature_types) if init_booster is not None and init_booster.feature_types else None)

    def make_booster(trees):
        return Booster(trees=list(trees), feature_names=names, feature_types=ftypes, base_score=base_score,
                       num_feature=F,
                       train_params=dict(eta=hp.eta, gamma=hp.gamma, max_depth=hp.max_depth,
                                         min_child_weight=hp.min_child_weight, reg_lambda=hp.reg_lambda,
                                         reg_alpha=hp.reg_alpha, subsample=hp.subsample,
                                         colsample_bytree=float(params.colsample_bytree),
                                         max_bin=int(params.max_bin), scale_pos_weight=spw, seed=hp.seed,
                                         **({"monotone_constraints": tuple(int(c) for c in mono)}
                                            if mono is not None else {}),
                                         **({"interaction_constraints": [list(g) for g in inter]}
                                            if inter is not None else {})))

    def early_stop(s0: int) -> bool:
        """Early stopping: score the segment's trees (rounds s0 ...); on a stop keep trees 0..that round."""
        if not early:
            return False
        stop = mon.add_trees(make_booster(trees_so_far[s0:]), s0)
        if stop is not None:
            del trees_so_far[stop + 1:]
        return stop is not None

    def segment_done(new_nodes: np.ndarray, end: int) -> None:
        trees_so_far.extend(trees_from_heap_nodes(new_nodes, hp.max_depth))
        if checkpoint is not None:
            checkpoint.save(make_booster(trees_so_far))
        fault_after = int(knob("COBALT_FAULT_AFTER_TREES", "0") or 0)
        fault_rank = int(knob("COBALT_FAULT_RANK", "-1") or -1)
        if fault_after and end >= fault_after and end < T and (fault_rank < 0 or fault_rank == (dist.rank if dist else 0)):
            stall = float(knob("COBALT_FAULT_STALL_S", "0") or 0)
            if stall > 0:  # a slow (not dead) rank: once, then it carries on
                if not getattr(segment_done, "stalled", False):
                    segment_done.stalled = True
                    time.sleep(stall)
            else:
                raise InjectedFault(f"injected fault after tree {end}")
    hp = gbdt_host.HostGbdtParams(max_depth=int(params.max_depth), eta=float(params.learning_rate),
                                  reg_lambda=float(params.reg_lambda), reg_alpha=float(params.reg_alpha),
                                  gamma=float(params.gamma), min_child_weight=float(params.min_child_weight),
                                  subsample=float(params.subsample), seed=int(params.random_state),
                                  gscale=1.0 if exact_fp64 else gscale, hscale=1.0 if exact_fp64 else hscale,
                                  quant=not exact_fp64, qbits=grad_bits, monotone=mono,
                                  interaction=inter)
    if exact_fp64 and dev.type != "cpu":
        raise ValueError("exact_fp64 is the host (CPU) reference trainer")
    tp = rep.mark("labels_weights", tp, dev)
    tb = time.perf_counter()
    if dev.type == "cuda":
        from ..ops import gbdt_ops

        margin = (init_margin.to(dev, torch.float32).clone().contiguous() if init_margin is not None
                  else torch.full((N,), base_margin, dtype=torch.float32, device=dev))
        comm = dist.native_comm if dist is not None else None
        if world > 1 and comm is None:
            raise RuntimeError("data-parallel GPU training needs the native RCCL communicator")
        tr = gbdt_ops.GpuGbdtTrainer(n_rows=N, n_feat=F, max_depth=hp.max_depth, max_trees=T, eta=hp.eta,
                                     reg_lambda=hp.reg_lambda, reg_alpha=hp.reg_alpha, gamma=hp.gamma,
                                     min_child_weight=hp.min_child_weight, subsample=hp.subsample,
                                     gscale=gscale, hscale=hscale, base_margin=base_margin,
                                     seed=hp.seed, row_offset=bd.row_offset, world_size=world, comm=comm,
                                     grad_bits=grad_bits)
        fm = torch.as_tensor(fmask_np, device=dev).contiguous()
        tr.set_data(bd.records, bd.binsT, bd.cuts.contiguous(), bd.nbins.to(torch.int32).contiguous(),
                    yt.contiguous(), wt, margin, fm)
        # 0/1 labels and no sample weights: the labels ride in the row records' padding and the weights
        # follow from them (8 fewer bytes per row in every gradient pass); COBALT_LABEL_IN_RECORD=0 off
        if (sample_weight is None and knob("COBALT_LABEL_IN_RECORD", "1") != "0"
                and bd.records.shape[1] == 32 and F <= 23
                and (labels_binary if labels_binary is not None else bool(((yt == 0) | (yt == 1)).all()))):
            tr.set_binary_labels(float(np.float32(spw)))
        if mono is not None:  # (a reused context starts every fit unconstrained: cobalt_gbdt_reuse)
            tr.set_monotone(mono)
        if inter is not None:
            tr.set_interaction(interaction_words(inter, F), len(inter))
        # row reorder: one process, in core, 32-byte records, 17-bit gradients, a fresh model, no checkpoints
        ro_sched = resolve_row_reorder(params.row_reorder, T, N)
        ro_off = ("data parallel" if world > 1 else "init_booster" if init_booster is not None or T0
                  else "checkpointing" if checkpoint is not None
                  else "generic records" if bd.records.shape[1] != 32 or F > 24
                  else "wide gradients" if grad_bits != 17 else None) if ro_sched else "no schedule"
        ro_done: list[int] = []

        def grow(a: int, n: int) -> None:
            """``tr.grow(a, n)``, split at the scheduled reorders (a reorder runs between two grow calls)."""
            nonlocal ro_off
            b = a + n
            for r in ([] if ro_off else [r for r in ro_sched if a <= r < b]):
                tr.grow(a, r + 1 - a)
                a = r + 1
                if tr.reorder(r):
                    ro_done.append(r)
                else:
                    ro_off = "not supported for this fit by the native trainer"
                    break
            if b > a:
                tr.grow(a, b - a)
        tp = rep.mark("trainer_setup", tp, dev)
        completed = False
        try:
            if T0:
                tr.set_start(T0)
            if world > 1:
                # COBALT_FAULT_CORRUPT_RANK=r [COBALT_FAULT_CORRUPT_TREE=t]: rank r grows a different tree t
                # (its root totals perturbed), which the in-flight replica check must catch on every rank
                cr = int(knob("COBALT_FAULT_CORRUPT_RANK", "-1") or -1)
                if cr == dist.rank:
                    tr.set_fault(int(knob("COBALT_FAULT_CORRUPT_TREE", "1") or 1))
            head = None
            if checkpoint is None and not early and T - T0 >= 64 and _own_device(world):
                # Two grow calls: the first part's trees are fetched (on a side stream) and converted on
                # the host while the GPU grows the last ones -- the host's ~1 ms per 300 trees of
                # fetch + conversion leaves the fit's critical path.
                tail = min(32, (T - T0) // 4)
                head = T - tail
                grow(T0, head - T0)
                ev = torch.cuda.Event()
                ev.record()
                grow(head, T - head)
                rep.extra["plan"] = tr.plan()
                if world > 1:
                    _watch_segment(dist, dev, T0, head, tr, ev)
                else:
                    ev.synchronize()
                trees_so_far.extend(trees_from_heap_nodes(tr.fetch(T0, head - T0, _side_stream(dev)), hp.max_depth))
            for s0 in ([head] if head is not None else range(T0, T, seg)):
                s1 = min(T, s0 + seg)
                if head is None:
                    grow(s0, s1 - s0)
                    rep.extra["plan"] = tr.plan()
                if world > 1:  # fail fast (abort the communicator) if a peer rank dies mid-segment
                    _watch_segment(dist, dev, s0, s1, tr)
                tp = rep.mark("grow", tp, dev)
                seg_nodes = tr.fetch(s0, s1 - s0)
                if world > 1 and tr.replica_error():
                    raise ReplicaDivergence(f"data-parallel replicas diverged before tree {s1} (rank {dist.rank}): "
                                            "the ranks' split decisions differ (in-flight digest check)")
                tp = rep.mark("fetch", tp, dev)
                segment_done(seg_nodes, s1)
                tp = rep.mark("convert", tp, dev)
                if early_stop(s0):  # (every grown tree was fetched: the context can be parked)
                    break
            tr.unpermute()  # (reordered rows: the margins back in the caller's row order)
            rep.extra["row_reorder"] = {"trees": ro_done, "off": ro_off}
            completed = True
        finally:
            tr.close(park=completed)  # a completed fit's context is kept for the next fit of these shapes
        tp = rep.mark("close", tp, dev)
        rep.extra["margin"] = margin  # training margins incl. every tree (device tensor)
    else:
        cuts_np = bd.cuts.cpu().numpy()
        nb_np = bd.nbins.cpu().numpy()
        margin_np = (init_margin.cpu().numpy().astype(np.float32).copy() if init_margin is not None
                     else np.full(N, np.float32(base_margin), dtype=np.float32))
        y_np = yt.cpu().numpy()
        w_np = wt.cpu().numpy()
        allreduce = None
        if world > 1:
            def allreduce(a: np.ndarray) -> np.ndarray:
                t = torch.from_numpy(np.ascontiguousarray(a))
                dist.allreduce(t, "sum")
                return t.numpy()
        for s0 in range(T0, T, seg):
            s1 = min(T, s0 + seg)
            recs = []
            for t in range(s0, s1):
                gq, hq = gbdt_host.gradients_host(margin_np, y_np, w_np, hp, t, bd.row_offset)
                recs.append(gbdt_host.grow_tree_host(bd.bins_host, cuts_np, nb_np, gq, hq, margin_np, hp,
                                                     fmask_np[t], allreduce))
            segment_done(np.stack(recs), s1)
            if early_stop(s0):
                break
        rep.extra["margin"] = margin_np
    t_boost = time.perf_counter() - tb
    tp = rep.mark("to_trees", tp, dev)
    bst = make_booster(trees_so_far)
    if mon is not None:
        if not early and len(trees_so_far) > T0:  # the whole curve of the new trees in one pass per set
            mon.add_trees(make_booster(trees_so_far[T0:]), T0)
        if early and mon.best is not None:
            bst.attributes["best_iteration"] = str(mon.best)
            bst.attributes["best_score"] = repr(mon.best_score)
        if evals_result is not None:
            evals_result.clear()
            evals_result.update(mon.result())
    if report is not None:
        report.n_rows, report.n_rows_global, report.n_features = N, bd.n_rows_global, F
        report.n_trees = len(trees_so_far)
        report.device, report.world = str(dev), world
        report.t_sketch, report.t_bin, report.t_boost = bd.t_sketch, bd.t_bin, t_boost
        report.extra["cuts"] = bd.cuts
        report.extra["nbins"] = bd.nbins
    return bst


_side_streams: dict = {}


def _own_device(world: int) -> bool:
    """Whether the fit may take a second stream of its own (the fetch overlap): one process only. Ranks
    that share a device (the one-GPU rehearsals) are time-sliced or CU-partitioned, and their exchange
    kernels wait on each other inside the GPU: an extra stream per process deadlocked unmasked ranks for
    the 120 s exchange deadline (tests/test_00gpu_dp_ipc.py, a CU budget without masks) and slowed
    CU-masked ranks 9x (2 ranks, 2M rows: 945.6 vs 102.7 ms per fit,
    profiles/round6/ab_sketch_side_stream.txt). Data-parallel fits on separate GPUs would not share
    queues, but that configuration cannot be rehearsed on one GPU, so they keep one stream too."""
    return world <= 1


def _side_stream(dev) -> torch.cuda.Stream:
    """A second stream of ``dev`` (created once) for copies that must not wait on the trainer's stream."""
    key = torch.device(dev).index or 0
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(torch.device("cuda", key))
    return _side_streams[key]


def _watch_segment(dist, dev, s0: int, s1: int, tr=None, ev=None) -> None:
    """Wait for trees [s0, s1) -- the work before ``ev`` (default: everything enqueued so far) -- with
    the data-parallel watchdog (a dead or failed peer aborts the communicator instead of hanging)."""
    from .. import _native
    from ..parallel import dist as pdist

    if ev is None:
        ev = torch.cuda.Event()
        ev.record()
    comm = dist.native_comm
    lib = _native.lib()

    def comm_error():
        e = lib.cobalt_comm_async_error(ctypes.c_void_p(comm)) if comm else 0
        return e
    # a replica divergence does not stop the stream (every rank keeps exchanging in step): the segment
    # finishes and the caller raises ReplicaDivergence after it, on every rank
    pdist.wait_with_watchdog(ev.query, timeout_s=pdist.collective_timeout_s(), comm_error=comm_error if comm else None,
                             abort=lambda: pdist.abort_native_comm(dist), what=f"trees {s0}..{s1 - 1}")


class InjectedFault(RuntimeError):
    """Raised by the fault-injection hook (``COBALT_FAULT_AFTER_TREES`` [+ ``COBALT_FAULT_RANK``])."""


class ReplicaDivergence(RuntimeError):
    """Data-parallel ranks grew different trees (a stale or corrupted exchange on some rank). Raised on
    every rank of the fit: each one's digest check compares the ranks' summed digests with its own."""


class Checkpointer:
    """Periodic model checkpoints of a fit (checkpoint-per-N-trees + resume).

    The checkpoint is the XGBoost UBJSON model of the trees grown so far (loadable by any consumer
    of the format) plus a JSON sidecar with the fit parameters; both are replaced atomically
    (write + ``os.replace``). Only rank 0 writes under data parallelism; every rank reads on resume."""

    def __init__(self, path: str, every: int, params: GBDTParams, dist=None):
        self.path = str(path)
        self.every = int(every)
        self.params = params
        self.rank = dist.rank if dist is not None else 0

    def _meta(self, n_trees: int) -> dict:
        keys = ("max_depth", "learning_rate", "gamma", "min_child_weight", "reg_lambda", "reg_alpha", "subsample",
                "colsample_bytree", "max_bin", "scale_pos_weight", "random_state", "n_estimators")
        meta = {"n_trees": n_trees, "params": {k: getattr(self.params, k) for k in keys}}
        # (None without constraints, whatever the form: a checkpoint from before the parameter resumes)
        mc = self.params.monotone_constraints
        if isinstance(mc, dict):
            mc = {str(k): int(v) for k, v in sorted(mc.items()) if int(v)} or None
        elif mc is not None:
            plain = _mono_plain(mc)
            mc = [int(v) for v in plain] if any(plain) else None
        meta["params"]["monotone_constraints"] = mc
        # (likewise: the groups as given -- indices or names --, None without constraints)
        ic = [[e if isinstance(e, str) else int(e) for e in g] for g in _inter_plain(self.params.interaction_constraints)]
        meta["params"]["interaction_constraints"] = [g for g in ic if g] or None
        return meta

    def save(self, booster: Booster) -> None:
        if self.rank != 0:
            return
        tmp = self.path + ".tmp"
        with open(tmp, "wb") as fh:
            fh.write(booster.save_raw("ubj"))
        os.replace(tmp, self.path)
        with open(tmp + ".json", "w") as fh:
            json.dump(self._meta(booster.num_trees), fh)
        os.replace(tmp + ".json", self.path + ".json")

    def load(self) -> Booster | None:
        if not os.path.exists(self.path):
            return None
        meta_p = self.path + ".json"
        if os.path.exists(meta_p):
            with open(meta_p) as fh:
                meta = json.load(fh)
            want = self._meta(meta["n_trees"])["params"]
            diff = {k: (meta["params"].get(k), v) for k, v in want.items()
                    if k != "n_estimators" and meta["params"].get(k) != v}
            if diff:
                raise ValueError(f"checkpoint {self.path} was written with different parameters: {diff}")
        with open(self.path, "rb") as fh:
            return Booster.load_raw(fh.read())


def _feature_info(X) -> tuple[list[str] | None, list[str] | None]:
    if hasattr(X, "columns"):
        names = [str(c) for c in X.columns]
        types = []
        for c in X.columns:
            dt = X[c].dtype
            if dt == bool or str(dt) == "bool":
                types.append("i")
            elif np.issubdtype(dt, np.integer):
                types.append("int")
            else:
                types.append("float")
        return names, types
    return None, None


class GBDTClassifier:
    """sklearn-compatible drop-in for ``xgboost.XGBClassifier`` backed by this framework's trainer."""

    _param_names = ["n_estimators", "max_depth", "learning_rate", "gamma", "min_child_weight", "reg_lambda",
                    "reg_alpha", "subsample", "colsample_bytree", "max_bin", "scale_pos_weight", "random_state",
                    "base_score", "eval_metric", "use_label_encoder", "device", "importance_type", "n_jobs",
                    "sketch_rows", "sketch_weight", "early_stopping_rounds", "monotone_constraints",
                    "interaction_constraints"]

    def __init__(self, n_estimators=None, max_depth=None, learning_rate=None, gamma=None, min_child_weight=None,
                 reg_lambda=None, reg_alpha=None, subsample=None, colsample_bytree=None, max_bin=None,
                 scale_pos_weight=None, random_state=None, base_score=None, eval_metric=None,
                 use_label_encoder=None, device=None, importance_type=None, n_jobs=None, sketch_rows=None,
                 sketch_weight=None, early_stopping_rounds=None, monotone_constraints=None,
                 interaction_constraints=None):
        self.n_estimators = n_estimators
        self.max_depth = max_depth
        self.learning_rate = learning_rate
        self.gamma = gamma
        self.min_child_weight = min_child_weight
        self.reg_lambda = reg_lambda
        self.reg_alpha = reg_alpha
        self.subsample = subsample
        self.colsample_bytree = colsample_bytree
        self.max_bin = max_bin
        self.scale_pos_weight = scale_pos_weight
        self.random_state = random_state
        self.base_score = base_score
        self.eval_metric = eval_metric
        self.use_label_encoder = use_label_encoder
        self.device = device
        self.importance_type = importance_type
        self.n_jobs = n_jobs
        self.sketch_rows = sketch_rows
        self.sketch_weight = sketch_weight
        self.early_stopping_rounds = early_stopping_rounds
        self.monotone_constraints = monotone_constraints
        self.interaction_constraints = interaction_constraints

    # sklearn protocol
    def get_params(self, deep: bool = True) -> dict[str, Any]:
        # ``monotone_constraints`` / ``interaction_constraints`` are listed when set (``clone`` / ``set_params``
        # carry them); an estimator without constraints reports exactly the parameters it reported before the
        # arguments existed
        return {k: getattr(self, k) for k in self._param_names
                if k not in ("monotone_constraints", "interaction_constraints") or getattr(self, k) is not None}

    def set_params(self, **params) -> "GBDTClassifier":
        for k, v in params.items():
            if k not in self._param_names:
                raise ValueError(f"invalid parameter {k!r}")
            setattr(self, k, v)
        return self

    def __sklearn_tags__(self):
        from sklearn.utils import Tags, ClassifierTags, TargetTags, InputTags
        return Tags(estimator_type="classifier", target_tags=TargetTags(required=True),
                    classifier_tags=ClassifierTags(), input_tags=InputTags(allow_nan=True))

    _estimator_type = "classifier"

    def _train_params(self) -> GBDTParams:
        kw = {k: v for k, v in self.get_params().items() if v is not None}
        return GBDTParams.from_kwargs(**{k: v for k, v in {**XGB_DEFAULTS, **kw}.items()})

    def fit(self, X, y, sample_weight=None, xgb_model=None, eval_set=None, sample_weight_eval_set=None,
            verbose=None, **_):
        """``xgb_model`` (a Booster, a fitted classifier or a model/pickle path) continues boosting
        from that model for ``n_estimators`` more trees, as XGBoost's ``fit(xgb_model=...)``.

        ``eval_set`` = ``[(X_val, y_val), ...]`` (+ ``sample_weight_eval_set``, one weight vector or None
        per set): the constructor's ``eval_metric`` (default "logloss") is recorded after every round
        (:meth:`evals_result`), and with ``early_stopping_rounds`` the fit stops by XGBoost's rule on
        the last set's last metric (:func:`train`); ``verbose`` prints the rounds."""
        names, types = _feature_info(X)
        init = None
        if xgb_model is not None:
            if isinstance(xgb_model, Booster):
                init = xgb_model
            elif hasattr(xgb_model, "get_booster"):
                init = xgb_model.get_booster()
            else:
                from pathlib import Path

                raw = Path(xgb_model).read_bytes()
                if raw[:1] == b"\x80":
                    from .booster import load_pickle_bytes

                    init = load_pickle_bytes(raw)[1]
                else:
                    init = Booster.load_raw(raw)
        y_np = np.asarray(y.to_numpy() if hasattr(y, "to_numpy") else y).reshape(-1)
        self.classes_ = np.unique(y_np)
        if len(self.classes_) > 2:
            raise ValueError("GBDTClassifier supports binary targets")
        self.n_classes_ = 2
        yb = (y_np == self.classes_[-1]).astype(np.float32) if len(self.classes_) == 2 else y_np.astype(np.float32)
        evals = None
        if eval_set:
            wts = list(sample_weight_eval_set) if sample_weight_eval_set is not None else [None] * len(eval_set)
            if len(wts) != len(eval_set):
                raise ValueError("sample_weight_eval_set needs one entry per eval_set entry")
            evals = []
            for (Xv, yv), wv in zip(eval_set, wts):
                yv = np.asarray(yv.to_numpy() if hasattr(yv, "to_numpy") else yv).reshape(-1)
                if not np.isin(yv, self.classes_).all():
                    raise ValueError("eval_set labels must be among the training classes")
                yvb = (yv == self.classes_[-1]).astype(np.float32) if len(self.classes_) == 2 else yv.astype(np.float32)
                evals.append((self._matrix_named(Xv, names), yvb, wv))
        rep = FitReport()
        history: dict = {}
        self._Booster = train(X, yb, self._train_params(), sample_weight=sample_weight, device=self.device,
                              feature_names=names, feature_types=types, report=rep, init_booster=init,
                              evals=evals, eval_metric=self.eval_metric,
                              early_stopping_rounds=self.early_stopping_rounds, evals_result=history,
                              verbose_eval=bool(verbose))
        if evals is not None:
            self.evals_result_ = history
        elif hasattr(self, "evals_result_"):
            del self.evals_result_
        self.fit_report_ = rep
        self.n_features_in_ = self._Booster.num_feature
        if names is not None:
            self.feature_names_in_ = np.array(names, dtype=object)
        return self

    def get_booster(self) -> Booster:
        if not hasattr(self, "_Booster"):
            raise ValueError("need to call fit or load_model beforehand")
        return self._Booster

    @staticmethod
    def _matrix_named(X, names) -> np.ndarray | torch.Tensor:
        if isinstance(X, torch.Tensor):
            return X
        if hasattr(X, "columns") and names is not None:
            X = X[list(names)]
        return np.asarray(X.to_numpy(dtype=np.float32, na_value=np.nan) if hasattr(X, "to_numpy") else X,
                          dtype=np.float32)

    def _matrix(self, X) -> np.ndarray | torch.Tensor:
        return self._matrix_named(X, getattr(self, "feature_names_in_", None))

    def evals_result(self) -> dict[str, dict[str, list[float]]]:
        """``{"validation_0": {metric: [value per round]}, ...}`` of the last ``fit(eval_set=...)``."""
        if not hasattr(self, "evals_result_"):
            raise ValueError("no evaluation results: call fit with eval_set")
        return self.evals_result_

    @property
    def best_iteration(self) -> int:
        """Best round of an early-stopped fit (a global tree index)."""
        v = self.get_booster().best_iteration
        if v is None:
            raise AttributeError("best_iteration is only defined after a fit with early_stopping_rounds")
        return v

    @property
    def best_score(self) -> float:
        v = self.get_booster().best_score
        if v is None:
            raise AttributeError("best_score is only defined after a fit with early_stopping_rounds")
        return v

    def _n_trees(self, iteration_range) -> int | None:
        """Trees to score: the prefix ``iteration_range = (0, n)`` (``(0, 0)``: all); by default the first
        ``best_iteration + 1`` trees of an early-stopped model, else all (None)."""
        b = self.get_booster()
        if iteration_range is None:
            n = b.best_iteration + 1 if b.best_iteration is not None else b.num_trees
        else:
            lo, hi = (int(v) for v in iteration_range)
            if lo != 0 or hi < 0 or hi > b.num_trees:
                raise ValueError(f"iteration_range must be (0, n) with n <= {b.num_trees} trees, got {iteration_range}")
            n = hi if hi > 0 else b.num_trees
        return None if n >= b.num_trees else n

    def predict_proba(self, X, iteration_range=None) -> np.ndarray:
        p = self.get_booster().predict_proba(self._matrix(X), device=self.device,
                                             n_trees=self._n_trees(iteration_range))
        p = p.cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
        return np.stack([1.0 - p, p], axis=1)

    def predict(self, X, iteration_range=None) -> np.ndarray:
        p = self.predict_proba(X, iteration_range)[:, 1]
        pred = (p > 0.5).astype(np.int64)
        return self.classes_[pred] if getattr(self, "classes_", None) is not None and len(self.classes_) == 2 else pred

    def apply(self, X, iteration_range=None) -> np.ndarray:
        """The leaf every row lands in, per tree (``XGBClassifier.apply``): int32 [N, trees] node ids in the
        booster's numbering, over the trees :meth:`predict_proba` would score (``iteration_range``, else up to
        ``best_iteration``)."""
        n = self._n_trees(iteration_range)
        leaf = self.get_booster().predict_leaf(self._matrix(X), device=self.device, n_trees=n)
        return leaf.cpu().numpy() if isinstance(leaf, torch.Tensor) else np.asarray(leaf)

    def counterfactuals(self, X, **kw):
        """The nearest change that brings each declined row to the cutoff
        (:func:`~..explain.recourse.counterfactuals`), over the trees :meth:`predict_proba` scores, on this
        estimator's device."""
        from ..explain.recourse import counterfactuals

        return counterfactuals(self, X, **kw)

    def refresh(self, X, y, sample_weight=None, refresh_leaf: bool = True) -> "GBDTClassifier":
        """A NEW estimator whose trees keep this model's structure and whose node statistics (and, with
        ``refresh_leaf``, leaf values) are re-estimated on ``(X, y)`` with this estimator's hyper-parameters:
        XGBoost's ``process_type="update", updater="refresh"`` (:meth:`Booster.refresh`). This estimator is
        not modified; the result saves and loads like a fitted one."""
        b = self.get_booster()
        y_np = np.asarray(y.to_numpy() if hasattr(y, "to_numpy") else y).reshape(-1)
        classes = getattr(self, "classes_", None)
        if classes is not None and len(classes) == 2:
            if not np.isin(y_np, classes).all():
                raise ValueError("refresh labels must be among the training classes")
            yb = (y_np == classes[-1]).astype(np.float32)
        else:
            yb = y_np.astype(np.float32)
        p = self._train_params()
        new = type(self)(**self.get_params())
        new._Booster = b.refresh(self._matrix(X), yb, sample_weight, refresh_leaf=refresh_leaf, device=self.device,
                                 learning_rate=float(p.learning_rate), reg_lambda=float(p.reg_lambda),
                                 reg_alpha=float(p.reg_alpha), min_child_weight=float(p.min_child_weight),
                                 scale_pos_weight=float(p.scale_pos_weight), random_state=int(p.random_state),
                                 grad_bits=int(p.grad_bits))
        for k in ("classes_", "n_classes_", "n_features_in_", "feature_names_in_"):
            if hasattr(self, k):
                setattr(new, k, getattr(self, k))
        return new

    def _binary_labels(self, y):
        if isinstance(y, torch.Tensor):
            return y
        y_np = np.asarray(y.to_numpy() if hasattr(y, "to_numpy") else y).reshape(-1)
        classes = getattr(self, "classes_", None)
        if classes is not None and len(classes) == 2 and not np.isin(y_np, (0, 1)).all():
            if not np.isin(y_np, classes).all():
                raise ValueError("labels must be among the training classes")
            return (y_np == classes[-1]).astype(np.int64)
        return y_np

    def calibrate(self, X=None, y=None, method: str = "isotonic", sample_weight=None):
        """A :class:`models.calibration.CalibratedModel`: this classifier with a calibrator fitted on its margin
        over the held-out rows ``(X, y)``. ``method``: "isotonic", "sigmoid" (Platt) or "prior" (the analytic
        inverse of ``scale_pos_weight``; ``X`` and ``y`` may be None). CUDA tensors are fitted on their device.
        This estimator and its ``predict_proba`` are unchanged."""
        from .calibration import CalibratedModel, make_calibrator

        b = self.get_booster()
        cal = make_calibrator(method, float(self._train_params().scale_pos_weight))
        if method != "prior":
            if X is None or y is None:
                raise ValueError(f"method {method!r} needs held-out rows X and labels y")
            margin = b.predict_margin(self._matrix(X), device=self.device, n_trees=self._n_trees(None))
            cal.fit(margin, self._binary_labels(y), sample_weight)
        return CalibratedModel(self, cal)

    def reliability(self, X, y, **kw):
        """``metrics.calibration.reliability_report`` of this model's ``prob_default`` on ``(X, y)``."""
        from ..metrics.calibration import reliability_report

        p = self.get_booster().predict_proba(self._matrix(X), device=self.device, n_trees=self._n_trees(None))
        return reliability_report(self._binary_labels(y), p, **kw)

    def score(self, X, y) -> float:
        from ..metrics.classification import accuracy_score

        return accuracy_score(np.asarray(y), self.predict(X))

    @property
    def feature_importances_(self) -> np.ndarray:
        return self.get_booster().feature_importances(self.importance_type or "gain")

    # checkpoint I/O (reference: joblib.dump(best_model_tree) -> xgb_model_tree.pkl)
    def sklearn_state_params(self) -> dict[str, Any]:
        p = {k: getattr(self, k) for k in ["n_estimators", "max_depth", "learning_rate", "gamma", "min_child_weight",
                                           "reg_alpha", "reg_lambda", "subsample", "colsample_bytree",
                                           "scale_pos_weight", "base_score", "random_state", "max_bin", "device",
                                           "importance_type", "n_jobs", "eval_metric", "early_stopping_rounds",
                                           "monotone_constraints", "interaction_constraints"]}
        ic = p["interaction_constraints"]
        if ic is not None and not isinstance(ic, str):  # lists are written in XGBoost's string (JSON) form
            p["interaction_constraints"] = json.dumps(
                [[e if isinstance(e, str) else int(e) for e in g] for g in _inter_plain(ic)])
        mc = p["monotone_constraints"]
        if mc is not None and not isinstance(mc, (str, dict)):  # a sequence is written in XGBoost's string form
            from .booster import monotone_string

            p["monotone_constraints"] = monotone_string(_mono_plain(mc))
        p["kwargs"] = {"use_label_encoder": self.use_label_encoder} if self.use_label_encoder is not None else {}
        return p

    def save_pickle(self, path) -> None:
        from pathlib import Path

        Path(path).write_bytes(dump_pickle_bytes(self.get_booster(), self.sklearn_state_params()))

    @classmethod
    def load_pickle(cls, path) -> "GBDTClassifier":
        from pathlib import Path
        from .booster import load_pickle_bytes

        st, bst = load_pickle_bytes(Path(path).read_bytes())
        kw = {k: st.get(k) for k in cls._param_names if k in st and k not in ("use_label_encoder",)}
        if isinstance(kw.get("scale_pos_weight"), np.floating):
            kw["scale_pos_weight"] = float(kw["scale_pos_weight"])
        m = cls(**kw)
        m._Booster = bst
        m.classes_ = np.array([0, 1])
        m.n_classes_ = 2
        m.n_features_in_ = bst.num_feature
        if bst.feature_names:
            m.feature_names_in_ = np.array(bst.feature_names, dtype=object)
        return m

    def save_model(self, path) -> None:
        self.get_booster().save_model(path)

    def load_model(self, path) -> None:
        self._Booster = Booster.load_model(path)
        self.classes_ = np.array([0, 1])
        self.n_classes_ = 2


# XGBoost-compatible alias used by the reference-shaped CLIs
XGBClassifier = GBDTClassifier
