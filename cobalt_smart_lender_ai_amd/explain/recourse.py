"""Counterfactual recourse: the nearest change to an applicant's features that brings the model's probability
of default to a cutoff ("what would have to be different for this loan to be approved").

The model is a forest: along one feature, the others fixed, its margin is piecewise constant and changes
only at that feature's split thresholds ``t_0 < ... < t_{K-1}``. One candidate per interval,
``[-inf, t_0, ..., t_{K-1}]``, therefore covers every value the feature can take, and the scan of
``csrc/recourse.hip`` (definition: :func:`~..models.booster.recourse_scan_host`) scores each row at each of them
and keeps, per row and feature, the nearest interval below and above the row's own whose margin is at or below
the target, and the interval with the lowest margin. This module turns those into changes with a cost, picks the
cheapest per row, and reports.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Sequence

import numpy as np
import torch

from ..models.booster import Booster, sigmoid32

STATUSES = ("already_approved", "resolved", "no_recourse")
_APPROVED, _RESOLVED, _NONE = 0, 1, 2


# ------------------------------------------------------------------------------------- report
@dataclass
class RecourseReport:
    """Per-row result of :func:`counterfactuals` (NumPy arrays over the N rows):

    ``status``: "already_approved" (the margin was at or below the target; not scanned), "resolved" (the changes
    reach the target) or "no_recourse" (no allowed change does; such a row reports no changes);
    ``changes``: per row the ``(feature, from, to, cost)`` tuples in applied order; ``total_cost``: their summed
    cost (0 for approved rows, NaN for "no_recourse"); ``margin_before`` / ``margin_after`` (float32; equal unless
    resolved) and ``prob_before`` / ``prob_after``, their sigmoids. ``margin_after`` has the bits of
    ``predict_margin`` on the row with ``changes`` applied."""

    feature_names: list[str]
    cutoff: float
    target_margin: float
    status_code: np.ndarray        # int8 [N]: index into STATUSES
    change_feature: np.ndarray     # int32 [N, max_changes]: model feature index, -1 = no change in this place
    change_from: np.ndarray        # float32 [N, max_changes]
    change_to: np.ndarray          # float32 [N, max_changes]
    change_cost: np.ndarray        # float64 [N, max_changes]
    total_cost: np.ndarray         # float64 [N]
    margin_before: np.ndarray      # float32 [N]
    margin_after: np.ndarray       # float32 [N]

    def __len__(self) -> int:
        return int(self.status_code.shape[0])

    @property
    def status(self) -> np.ndarray:
        return np.asarray(STATUSES, dtype=object)[self.status_code]

    @property
    def prob_before(self) -> np.ndarray:
        return sigmoid32(self.margin_before)

    @property
    def prob_after(self) -> np.ndarray:
        return sigmoid32(self.margin_after)

    def row_changes(self, r: int) -> list[tuple[str, float, float, float]]:
        return [(self.feature_names[int(f)], float(self.change_from[r, k]), float(self.change_to[r, k]),
                 float(self.change_cost[r, k])) for k, f in enumerate(self.change_feature[r]) if f >= 0]

    @property
    def changes(self) -> list[list[tuple[str, float, float, float]]]:
        return [self.row_changes(r) for r in range(len(self))]

    def to_records(self) -> list[dict[str, Any]]:
        """One JSON-ready dict per row (``total_cost`` is None for "no_recourse")."""
        pb, pa = self.prob_before, self.prob_after
        out = []
        for r in range(len(self)):
            cost = float(self.total_cost[r])
            out.append({"status": STATUSES[int(self.status_code[r])],
                        "changes": [{"feature": f, "from": a, "to": b, "cost": c} for f, a, b, c in self.row_changes(r)],
                        "total_cost": None if math.isnan(cost) else cost,
                        "margin_before": float(self.margin_before[r]), "margin_after": float(self.margin_after[r]),
                        "prob_before": float(pb[r]), "prob_after": float(pa[r])})
        return out

    def to_dict(self) -> dict[str, Any]:
        return {"cutoff": self.cutoff, "target_margin": self.target_margin, "summary": self.summary(),
                "rows": self.to_records()}

    def summary(self) -> dict[str, Any]:
        """``{"n_rows", "status_share": {status: share of rows}, "changed_feature_share": {feature: share of the
        resolved rows that changed it}, "median_cost": median total cost of the resolved rows or None}``."""
        n = len(self)
        share = {s: (float(np.mean(self.status_code == k)) if n else 0.0) for k, s in enumerate(STATUSES)}
        res = self.status_code == _RESOLVED
        n_res = int(res.sum())
        feats: dict[str, float] = {}
        if n_res:
            f = self.change_feature[res]
            cnt = np.bincount(f[f >= 0].astype(np.int64), minlength=len(self.feature_names))
            feats = {self.feature_names[i]: float(cnt[i]) / n_res for i in np.argsort(-cnt, kind="stable") if cnt[i]}
        return {"n_rows": n, "status_share": share, "changed_feature_share": feats,
                "median_cost": float(np.median(self.total_cost[res])) if n_res else None}


# ------------------------------------------------------------------------------------- policy
@dataclass
class _Policy:
    feats: list[int]               # actionable features that have candidates, in position order
    cands: list[np.ndarray]        # the values that are scored
    up_val: np.ndarray             # float32 [sum K]: the value reported for an up move to candidate j
    dn_val: np.ndarray             # ... and for a down move
    cand_ptr: np.ndarray           # int64 [A + 1]
    win: np.ndarray                # int32 [A, 2]
    dirs: np.ndarray               # int32 [A]
    scale: np.ndarray              # float64 [A]


def _index_set(b: Booster, names) -> set[int]:
    if names is None or isinstance(names, (str, int, np.integer)):
        names = [] if names is None else [names]
    return {b._feature_index(f) for f in names}


def _keyed(b: Booster, d, what: str) -> dict[int, Any]:
    out = {}
    for k, v in (d or {}).items():
        f = b._feature_index(k)
        if f in out:
            raise ValueError(f"{what} names feature {k!r} twice")
        out[f] = v
    return out


def _host_matrix(Z) -> np.ndarray:
    if isinstance(Z, torch.Tensor):
        return Z.detach().cpu().numpy().astype(np.float32, copy=False)
    return np.asarray(Z.to_numpy(dtype=np.float32, na_value=np.nan) if hasattr(Z, "to_numpy") else Z, dtype=np.float32)


def _build_policy(b: Booster, actionable, immutable, increase_only, decrease_only, bounds, grids, scale, reference,
                  n_trees) -> _Policy:
    fixed, inc, dec = _index_set(b, immutable), _index_set(b, increase_only), _index_set(b, decrease_only)
    if inc & dec:
        raise ValueError("a feature cannot be both increase_only and decrease_only")
    bounds, grids, scale = _keyed(b, bounds, "bounds"), _keyed(b, grids, "grids"), _keyed(b, scale, "scale")
    order = list(range(b.num_feature)) if actionable is None else [b._feature_index(f) for f in actionable]
    if len(set(order)) != len(order):
        raise ValueError("actionable names a feature twice")
    ref = None if reference is None else _host_matrix(reference)
    if ref is not None and (ref.ndim != 2 or ref.shape[1] < b.num_feature):
        raise ValueError(f"reference must be [rows, >= {b.num_feature}], got shape {ref.shape}")
    p = _Policy([], [], None, None, None, None, None, None)
    ups, dns, wins, dirs, scales = [], [], [], [], []
    for f in order:
        if f in fixed:
            continue
        if f in grids:
            cv = np.unique(np.asarray(grids[f], dtype=np.float32).reshape(-1))
            if cv.size == 0 or not np.isfinite(cv).all():
                raise ValueError(f"the grid of feature {f} must hold finite values")
            up = dn = cv
        else:
            t = b.split_values(f, n_trees)
            if t.size == 0:
                continue  # no split and no grid: nothing to offer
            cv = np.concatenate([np.array([-np.inf], np.float32), t])
            up = cv                                                      # the smallest value of interval j
            dn = np.concatenate([np.nextafter(t, np.float32(-np.inf)),   # the largest value still inside it
                                 np.array([np.inf], np.float32)]).astype(np.float32)
        lo, hi = (np.float32(v) for v in bounds.get(f, (-np.inf, np.inf)))
        if np.isnan(lo) or np.isnan(hi):
            raise ValueError(f"the bounds of feature {f} must not be NaN")
        # the candidates whose interval meets [lo, hi]; the value reported is the nearest one inside both
        inside = np.flatnonzero((dn >= lo) & (up <= hi))
        wins.append((int(inside[0]), int(inside[-1])) if inside.size else (0, -1))
        ups.append(np.maximum(up, lo))
        dns.append(np.minimum(dn, hi))
        dirs.append(1 if f in inc else (-1 if f in dec else 0))
        if f in scale:
            s = float(scale[f])
            if not s > 0:
                raise ValueError(f"the scale of feature {f} must be positive, got {s}")
        else:
            s = 0.0
            if ref is not None:
                col = ref[:, f].astype(np.float64)
                col = col[~np.isnan(col)]
                s = float(np.quantile(col, 0.95) - np.quantile(col, 0.05)) if col.size else 0.0
            if not s > 0:
                fin = cv[np.isfinite(cv)]
                s = float(fin[-1]) - float(fin[0]) if fin.size else 0.0
            if not s > 0 or not math.isfinite(s):
                s = 1.0
        scales.append(s)
        p.feats.append(f)
        p.cands.append(cv)
    if p.feats:
        p.up_val = np.concatenate(ups).astype(np.float32)
        p.dn_val = np.concatenate(dns).astype(np.float32)
        p.cand_ptr = np.zeros(len(p.feats) + 1, np.int64)
        np.cumsum([len(c) for c in p.cands], out=p.cand_ptr[1:])
        p.win = np.asarray(wins, np.int32).reshape(-1, 2)
        p.dirs = np.asarray(dirs, np.int32)
        p.scale = np.asarray(scales, np.float64)
    return p


# ------------------------------------------------------------------------------------ selection
def _first_true(mask: torch.Tensor) -> torch.Tensor:
    """Per row the lowest column where ``mask`` holds (the number of columns where none does)."""
    n = mask.shape[1]
    pos = torch.arange(n, device=mask.device).expand_as(mask)
    return torch.where(mask, pos, torch.full_like(pos, n)).min(dim=1).values


def _cheapest(has: torch.Tensor, cost: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Among the columns where ``has`` holds, per row the lowest column of minimal cost, and that cost."""
    inf = torch.full_like(cost, math.inf)
    cmin = torch.where(has, cost, inf).min(dim=1).values
    return _first_true(has & (cost == cmin[:, None])), cmin


def target_margin(cutoff: float) -> float:
    """The largest float32 margin ``m`` with ``m <= logit(cutoff)``: a row is approved when its float32 margin is
    at or below it."""
    if not 0.0 < float(cutoff) < 1.0:
        raise ValueError(f"cutoff must lie inside (0, 1), got {cutoff}")
    L = math.log(float(cutoff) / (1.0 - float(cutoff)))
    t = np.float32(L)
    if float(t) > L:
        t = np.nextafter(t, np.float32(-np.inf))
    return float(t)


def _margins(b: Booster, X: torch.Tensor, n_trees) -> torch.Tensor:
    from ..ops import predict_ops

    return torch.as_tensor(predict_ops.predict_margin(b, X, device=X.device, n_trees=n_trees), device=X.device)


def _scan(b: Booster, X: torch.Tensor, p: _Policy, target: float, n_trees) -> tuple[torch.Tensor, torch.Tensor]:
    from ..ops import predict_ops

    idx, mg = predict_ops.recourse_scan(b, X, p.feats, p.cands, win=p.win, dirs=p.dirs, target_margin=target,
                                        n_trees=n_trees, device=X.device)
    return torch.as_tensor(idx, device=X.device), torch.as_tensor(mg, device=X.device)


def default_policy(b: Booster) -> dict[str, Any]:
    """``config.RECOURSE_POLICY`` (the deployed features) as keyword arguments of :func:`counterfactuals`,
    restricted to the features ``b`` has."""
    from ..config import RECOURSE_POLICY

    names = set(b.feature_names or [])
    return {k: ({f: g for f, g in v.items() if f in names} if isinstance(v, dict)
                else tuple(f for f in v if f in names)) for k, v in RECOURSE_POLICY.items()}


def _resolve_model(model, kw: dict) -> tuple[Booster, Any]:
    """(booster, X converter); a classifier's trees and device become defaults in ``kw``."""
    from .shap import TreeExplainer

    if isinstance(model, TreeExplainer):
        if kw.get("device") is None:
            kw["device"] = model.device
        return model.booster, None
    if isinstance(model, Booster):
        return model, None
    if hasattr(model, "get_booster") and hasattr(model, "_n_trees"):
        if kw.get("n_trees") is None:
            kw["n_trees"] = model._n_trees(None)
        if kw.get("device") is None:
            kw["device"] = model.device
        return model.get_booster(), model._matrix
    raise TypeError("expected a GBDTClassifier, a Booster or a TreeExplainer")


def counterfactuals(model, X, *, cutoff: float = 0.5, actionable=None, immutable=(), increase_only=(),
                    decrease_only=(), bounds=None, grids=None, scale=None, reference=None, max_changes: int = 1,
                    n_trees: int | None = None, device=None) -> RecourseReport:
    """For every row of ``X`` whose probability of default is above ``cutoff``, the cheapest change of one
    feature that brings it to the cutoff or below (a :class:`RecourseReport`). ``model``: a ``GBDTClassifier``
    (its scored trees and device), a ``Booster`` or a ``TreeExplainer``. A row is approved when its float32 margin
    is ``<= logit(cutoff)``; approved rows are reported "already_approved" and are not scanned.

    **What may change.** ``actionable``: the features (names or indices) that may change, in the order that
    breaks ties (default: all, in model order); ``immutable`` ones never do; ``increase_only`` /
    ``decrease_only`` restrict the direction; ``bounds={feature: (lo, hi)}`` keeps the new value inside
    ``[lo, hi]``. A NaN cell is never changed.

    **Candidates.** With ``t_0 < ... < t_{K-1}`` the feature's split values (:meth:`Booster.split_values`), the
    margin is constant on each of the K + 1 intervals they cut, so one candidate per interval is every value the
    feature can take. An up move to an interval reports its smallest value ``t_{j-1}`` (the smallest change that
    gets there), a down move its largest, ``nextafter(t_j, -inf)`` in float32 (or the bound, where a bound cuts the
    interval); -inf is never reported. ``grids={feature: values}`` replaces the intervals by explicit values
    for features that live on a grid (dummies, ``term`` in {36, 60}); the value reported is the grid value. A row
    value off its grid takes the nearest grid value below it as its own position (and that one is never
    proposed). A feature without split values and without a grid has nothing to offer.

    **Cost** of a change is ``|x_new - x| / scale[feature]`` in float64. ``scale`` defaults to the q95 - q05
    spread of the feature's non-NaN values in ``reference`` (rows like the training set) when given, else to the
    spread of its candidates ``t_{K-1} - t_0``, else (not positive) to 1.

    **Search.** Rounds of one scan each, at most ``max_changes``. A row with a move that reaches the target takes
    the cheapest (ties: the earlier feature, then down before up) and is "resolved". Otherwise, if a round is
    left, it takes the move with the lowest margin among the features it has not changed yet (ties: the lower
    cost, then the earlier feature) provided that lowers its margin, and goes on from there; else it is
    "no_recourse". With ``max_changes=1`` the answer is the exact minimum-cost single-feature change over every
    value the features can take. With more it is greedy: a cheaper pair of changes may exist, and a pair may
    exist where none is found.

    The same selection code runs on either device (torch ops; on a CUDA device nothing but the final report
    leaves it, on the CPU the scan is the NumPy definition), so both give the same report."""
    from ..ops import predict_ops

    kw = {"n_trees": n_trees, "device": device}
    b, conv = _resolve_model(model, kw)
    n_trees, device = kw["n_trees"], kw["device"]
    if conv is not None:
        X = conv(X)
    elif not isinstance(X, torch.Tensor):
        if hasattr(X, "columns") and b.feature_names:
            X = X[b.feature_names]
        X = _host_matrix(X)
    if X.ndim != 2 or X.shape[1] < b.num_feature:
        raise ValueError(f"X has shape {tuple(X.shape)}, model needs [rows, >= {b.num_feature}]")
    if int(max_changes) < 1:
        raise ValueError(f"max_changes must be at least 1, got {max_changes}")
    R = int(max_changes)
    target = target_margin(cutoff)
    p = _build_policy(b, actionable, immutable, increase_only, decrease_only, bounds, grids, scale, reference, n_trees)
    dev = predict_ops._device_of(X, device)
    Xt = predict_ops._as_f32(X, dev)
    N = Xt.shape[0]
    names = list(b.feature_names or [f"f{i}" for i in range(b.num_feature)])

    m0 = _margins(b, Xt, n_trees) if N else torch.empty(0, dtype=torch.float32, device=dev)
    status = torch.where(m0 <= target, _APPROVED, _NONE).to(torch.int8)
    ch_feat = torch.full((N, R), -1, dtype=torch.int32, device=dev)
    ch_from = torch.zeros((N, R), dtype=torch.float32, device=dev)
    ch_to = torch.zeros((N, R), dtype=torch.float32, device=dev)
    ch_cost = torch.zeros((N, R), dtype=torch.float64, device=dev)
    m_after = m0.clone()

    rows = torch.nonzero(status == _NONE).reshape(-1)   # the rows still searched, ...
    if p.feats and rows.numel():
        A = len(p.feats)
        fcol = torch.as_tensor(p.feats, dtype=torch.int64, device=dev)
        off = torch.as_tensor(p.cand_ptr[:-1], device=dev)[None, :, None]
        cand = torch.as_tensor(np.concatenate(p.cands), device=dev)
        up_val, dn_val = torch.as_tensor(p.up_val, device=dev), torch.as_tensor(p.dn_val, device=dev)
        sc = torch.as_tensor(p.scale, device=dev)[None, :]
        Xw = Xt[rows].clone()                            # ... at their current values
        cur = m0[rows]
        changed = torch.zeros((rows.numel(), A), dtype=torch.bool, device=dev)
        for k in range(R):
            idx, mg = _scan(b, Xw, p, target, n_trees)
            x = Xw[:, fcol]
            xd = x.double()
            at = off + idx.clamp(min=0).long()           # [n, A, 3] -> positions in the flat tables
            # 1. a move that reaches the target: the cheapest of (feature, down / up)
            val = torch.stack([dn_val[at[..., 0]], up_val[at[..., 1]]], dim=2)           # [n, A, 2]
            cost = (val.double() - xd[..., None]).abs() / sc[..., None]
            has = idx[..., :2] >= 0
            pick, cmin = _cheapest(has.reshape(-1, 2 * A), cost.reshape(-1, 2 * A))
            done = pick < 2 * A
            d = torch.nonzero(done).reshape(-1)
            a, s = pick[d] // 2, pick[d] % 2
            g = rows[d]
            ch_feat[g, k] = fcol[a].to(torch.int32)
            ch_from[g, k] = x[d, a]
            ch_to[g, k] = val[d, a, s]
            ch_cost[g, k] = cmin[d]
            m_after[g] = mg[d, a, s]
            status[g] = _RESOLVED
            if k == R - 1:
                break
            # 2. otherwise the move with the lowest margin among the features not changed yet
            j2 = idx[..., 2]
            below = cand[at[..., 2]] <= x                # candidates up to the row's own position are <= x
            v2 = torch.where(below, dn_val[at[..., 2]], up_val[at[..., 2]])
            c2 = (v2.double() - xd).abs() / sc
            m2 = mg[..., 2]
            has2 = (j2 >= 0) & ~changed & ~done[:, None]
            mmin = torch.where(has2, m2, torch.full_like(m2, math.inf)).min(dim=1).values
            pick2, cmin2 = _cheapest(has2 & (m2 == mmin[:, None]), c2)
            go = (pick2 < A) & (mmin < cur)
            d = torch.nonzero(go).reshape(-1)
            if d.numel() == 0:
                break
            a = pick2[d]
            g = rows[d]
            ch_feat[g, k] = fcol[a].to(torch.int32)
            ch_from[g, k] = x[d, a]
            ch_to[g, k] = v2[d, a]
            ch_cost[g, k] = cmin2[d]
            Xw = Xw[d]
            Xw[torch.arange(d.numel(), device=dev), fcol[a]] = v2[d, a]
            changed = changed[d]
            changed[torch.arange(d.numel(), device=dev), a] = True
            cur = mmin[d]
            rows = g
    # a row without recourse reports no changes
    none = status == _NONE
    ch_feat[none] = -1
    ch_from[none] = 0
    ch_to[none] = 0
    ch_cost[none] = 0
    total = ch_cost[:, 0].clone()
    for k in range(1, R):  # in applied order: the same float64 sum on either device
        total += ch_cost[:, k]
    total[none] = math.nan
    host = [t.cpu().numpy() for t in (status, ch_feat, ch_from, ch_to, ch_cost, total, m0, m_after)]
    return RecourseReport(names, float(cutoff), target, *host)
