"""A weight-of-evidence points scorecard: the transparent challenger of the GBDT champion.

Coarse-classed characteristics, weight of evidence (WoE) per class, a logistic regression on the WoE values,
a points table scaled by "points to double the odds" and reason codes read off the table. This module holds the
definitions in NumPy (they are the oracles of ``csrc/scorecard.hip`` and the CPU path) and the model; on a GPU
the counts come from ``csrc/bincount.hip`` and the three passes over the rows (encode, Newton pass, score) from
``csrc/scorecard.hip`` through ``ops.scorecard_ops``. Class 0 (``y <= 0.5``) is "good", class 1 "bad"; the
margin is the log-odds of bad, so a coefficient on a WoE value is about -1.

Classing (:func:`coarse_classing`) runs on the host from integer counts, so a CPU fit and a GPU fit of the same
data have the same bins. Fine edges come from ``monitor.drift.drift_edges(col, n_fine)``, the ``[2, cells]``
counts (row 0 good, row 1 bad, weights quantised as in ``monitor.drift``) from ``bin_counts_host`` /
``bin_counts_gpu``. A coarse bin is a run of adjacent fine *value* cells; the missing (NaN) cell is handled apart.
Bad rates are compared on integers (cross-multiplied), so no tie depends on rounding.

 1. Share and classes. While there is more than one bin and some bin holds less than ``min_bin_share`` of the
    total weight (all cells, the missing one included) or lacks a class: the LEFTMOST such bin is merged with
    its neighbour of smaller weight; equal weights, the LEFT neighbour; an end bin has one neighbour.
 2. Monotone bad rate, by pool-adjacent-violators from the left: a bin whose bad rate does not strictly
    continue the direction (an equal rate violates too) is pooled with its left neighbour, and the pooled bin is
    compared again with the one before it. Direction ``+1``: the bad rate rises with the value, ``-1``: it falls,
    ``0``: the step is skipped. ``"auto"``: both directions are pooled and the one with the larger information
    value (of the value bins, ``woe_iv``) is kept; equal IVs, the decreasing one.
 3. While there are more than ``max_bins`` value bins, the adjacent pair with the smallest ``|WoE difference|``
    (``woe_iv`` of the current value bins, with the missing bin when it stands alone) is merged; equal
    differences, the LEFTMOST pair.

The missing cell is a bin of its own when it holds at least ``min_bin_share`` of the weight and both classes;
otherwise it is left out of the WoE computation and gets WoE 0 (neutral). The coarse edges are the fine edges
between the surviving bins (float32). A characteristic left with a single bin is dropped: coefficient 0, 0 points.
"""
from __future__ import annotations

import json
import math
import os
from typing import Any, Sequence

import numpy as np
import torch

from ..monitor.drift import (_labels, _matrix, _on_gpu, _quantized, bin_counts_host, cell_pointer, check_drift_edges,
                             drift_cell, drift_edges, woe_iv)

MAX_FEATURE_CELLS = 256   # codes are uint8
MAX_TOP = 8
GPU_MAX_FEATURES = 63     # csrc/scorecard.hip kScMaxFeatures
GPU_MAX_CELLS = 8192      # csrc/scorecard.hip kScMaxCells


# --------------------------------------------------------------------------------------------------- classing
def _pava(bins: list[list[int]], direction: int) -> list[list[int]]:
    """Pool-adjacent-violators on ``[first cell, last cell, good, bad]`` bins (module docstring, step 2)."""
    out: list[list[int]] = []
    for b in bins:
        out.append(list(b))
        while len(out) > 1:
            a, c = out[-2], out[-1]
            # bad rate of c against a, as integers: bad_c tot_a - bad_a tot_c
            d = c[3] * (a[2] + a[3]) - a[3] * (c[2] + c[3])
            if d * direction > 0:
                break
            out[-2:] = [[a[0], c[1], a[2] + c[2], a[3] + c[3]]]
    return out


def _value_counts(bins: list[list[int]]) -> np.ndarray:
    return np.array([[b[2] for b in bins], [b[3] for b in bins]], dtype=np.int64)


def coarse_classing(counts2, fine_edges, *, max_bins: int = 6, min_bin_share: float = 0.05,
                    monotone: int | str = "auto") -> dict[str, Any]:
    """The coarse classes of one characteristic from its fine ``[2, K + 2]`` counts and ``K`` fine edges (module
    docstring). Returns ``edges`` (float32, a subset of ``fine_edges``), ``counts`` (int64 ``[2, K' + 2]``),
    ``woe`` (float64 ``[K' + 2]``), ``iv``, ``direction`` (+1 / -1 / 0 as applied), ``missing_own_bin`` and
    ``dropped``."""
    z = check_drift_edges(fine_edges)
    c = np.asarray(counts2, dtype=np.int64)
    if c.shape != (2, len(z) + 2):
        raise ValueError(f"{len(z)} edges need [2, {len(z) + 2}] counts, got shape {c.shape}")
    if len(z) + 2 > MAX_FEATURE_CELLS:
        raise ValueError(f"at most {MAX_FEATURE_CELLS} cells per feature")
    if int(max_bins) < 1 or not 0.0 <= float(min_bin_share) < 1.0:
        raise ValueError("max_bins must be at least 1 and min_bin_share in [0, 1)")
    if monotone not in ("auto", 1, -1, 0):
        raise ValueError(f'monotone must be "auto", +1, -1 or 0, got {monotone!r}')
    good, bad = int(c[0].sum()), int(c[1].sum())
    if good <= 0 or bad <= 0:
        raise ValueError("a scorecard needs both classes")
    total = good + bad

    def thin(g: int, b: int) -> bool:
        return (g + b) < min_bin_share * total or g == 0 or b == 0

    bins = [[k, k, int(c[0, k]), int(c[1, k])] for k in range(len(z) + 1)]
    while len(bins) > 1:
        k = next((i for i, b in enumerate(bins) if thin(b[2], b[3])), None)
        if k is None:
            break
        if k == 0:
            j = 1
        elif k == len(bins) - 1:
            j = k - 1
        else:
            lw, rw = bins[k - 1][2] + bins[k - 1][3], bins[k + 1][2] + bins[k + 1][3]
            j = k + 1 if rw < lw else k - 1
        lo, hi = min(j, k), max(j, k)
        bins[lo:hi + 1] = [[bins[lo][0], bins[hi][1], bins[lo][2] + bins[hi][2], bins[lo][3] + bins[hi][3]]]

    mg, mb = int(c[0, -1]), int(c[1, -1])
    own = not thin(mg, mb)
    vgood, vbad = sum(b[2] for b in bins), sum(b[3] for b in bins)
    has_values = vgood > 0 and vbad > 0

    direction = 0
    if has_values and monotone != 0:
        if monotone == "auto":
            up, down = _pava(bins, 1), _pava(bins, -1)
            direction = 1 if woe_iv(_value_counts(up))[1] > woe_iv(_value_counts(down))[1] else -1
            bins = up if direction == 1 else down
        else:
            direction = int(monotone)
            bins = _pava(bins, direction)

    def table(bs):
        cc = np.concatenate([_value_counts(bs), [[mg if own else 0], [mb if own else 0]]], axis=1)
        return woe_iv(cc)

    while has_values and len(bins) > max_bins:
        w = table(bins)[0]
        k = int(np.argmin(np.abs(np.diff(w[:len(bins)]))))   # argmin returns the leftmost minimum
        bins[k:k + 2] = [[bins[k][0], bins[k + 1][1], bins[k][2] + bins[k + 1][2], bins[k][3] + bins[k + 1][3]]]

    edges = np.array([z[b[1]] for b in bins[:-1]], dtype=np.float32)
    counts = np.concatenate([_value_counts(bins), [[mg], [mb]]], axis=1)
    if has_values or own:
        woe, iv = table(bins)
        woe = woe.copy()
    else:   # one class has all its weight in a thin missing cell: nothing to class
        woe, iv = np.zeros(len(bins) + 1), 0.0
    if not own:
        woe[-1] = 0.0
    dropped = len(bins) + (1 if own else 0) < 2
    if dropped:
        woe[:] = 0.0
        iv = 0.0
    return {"edges": edges, "counts": counts, "woe": woe, "iv": float(iv), "direction": direction,
            "missing_own_bin": bool(own), "dropped": bool(dropped)}


# ------------------------------------------------------------------------------------------------ definitions
def scorecard_encode_host(X, edges_list: Sequence[np.ndarray]) -> np.ndarray:
    """uint8 ``[N, F]``: ``codes[i, f] = drift_cell(edges_f, X[i, f])``. A value equal to an edge falls in the
    lower cell, +-inf in the end cells, NaN in cell ``K + 1``. The definition of ``k_sc_encode``."""
    X = np.asarray(X, dtype=np.float32)
    if X.ndim != 2 or X.shape[1] != len(edges_list):
        raise ValueError(f"X must be [rows, {len(edges_list)}], got shape {X.shape}")
    out = np.empty(X.shape, dtype=np.uint8)
    for f, z in enumerate(edges_list):
        z = check_drift_edges(z)
        if len(z) + 2 > MAX_FEATURE_CELLS:
            raise ValueError(f"at most {MAX_FEATURE_CELLS} cells per feature")
        out[:, f] = drift_cell(z, X[:, f])
    return out


def _row_terms(codes, cell_ptr, tab, y, w, beta):
    """Per row: ``Z [N, P]`` (1, then the WoE values), eta, p, q, e, labels and weights (float64)."""
    codes = np.asarray(codes)
    N, F = codes.shape
    ptr = np.asarray(cell_ptr, dtype=np.int64)
    tab = np.asarray(tab, dtype=np.float64)
    beta = np.asarray(beta, dtype=np.float64)
    if ptr.shape[0] != F + 1 or beta.shape[0] != F + 1 or tab.shape[0] != int(ptr[-1]):
        raise ValueError("codes, cell_ptr, tab and beta do not describe one table")
    Z = np.ones((N, F + 1), dtype=np.float64)
    eta = np.full(N, beta[0], dtype=np.float64)
    for f in range(F):
        cells = int(ptr[f + 1] - ptr[f])
        Z[:, f + 1] = tab[ptr[f] + np.minimum(codes[:, f].astype(np.int64), cells - 1)]
        eta = eta + beta[f + 1] * Z[:, f + 1]
    e = np.exp(-np.abs(eta))
    inv = 1.0 / (1.0 + e)
    big, small = inv, e * inv
    pos_eta = eta >= 0.0
    p = np.where(pos_eta, big, small)
    q = np.where(pos_eta, small, big)
    yb = np.asarray(y, dtype=np.float32).reshape(-1) > np.float32(0.5)
    wv = np.ones(N, dtype=np.float64) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
    if yb.shape[0] != N or wv.shape[0] != N:
        raise ValueError(f"{N} rows need {N} labels and weights")
    return Z, eta, e, p, q, yb, wv


def scorecard_newton_host(codes, cell_ptr, tab, y, w, beta) -> tuple[float, np.ndarray, np.ndarray]:
    """One Newton pass of the logistic regression on the WoE values: ``(loss, grad [F + 1], hess [F + 1, F + 1])``
    in float64. ``z~_i = (1, tab_f[codes[i, f]])``, ``eta = sum_j beta_j z~_ij`` in index order; with ``e =
    exp(-|eta|)``, ``p = sigma(eta)`` and ``q = sigma(-eta)`` are both formed from ``e`` (``1 - p`` is never
    computed); the residual is ``p`` for y = 0 and ``-q`` for y = 1, the curvature ``p q``, the loss term
    ``log1p(e) + max(eta, 0) - y eta``; labels are ``y > 0.5``. ``grad = sum w r z~``, ``hess = sum w p q z~ z~^T``
    with one triangle computed and mirrored. A code past a feature's cells reads its last cell. The definition
    of ``k_sc_newton``."""
    Z, eta, e, p, q, yb, wv = _row_terms(codes, cell_ptr, tab, y, w, beta)
    r = np.where(yb, -q, p)
    loss = float(np.sum(wv * (np.log1p(e) + np.maximum(eta, 0.0) - np.where(yb, eta, 0.0))))
    grad = Z.T @ (wv * r)
    H = np.triu(Z.T @ (Z * (wv * (p * q))[:, None]))
    return loss, grad, H + np.triu(H, 1).T


def scorecard_newton_abs_host(codes, cell_ptr, tab, y, w, beta) -> tuple[float, np.ndarray, np.ndarray]:
    """The sums of the absolute values of the terms of :func:`scorecard_newton_host`: what a summation error
    bound is relative to."""
    Z, eta, e, p, q, yb, wv = _row_terms(codes, cell_ptr, tab, y, w, beta)
    r = np.where(yb, -q, p)
    A = np.abs(Z)
    loss = float(np.sum(np.abs(wv * (np.log1p(e) + np.maximum(eta, 0.0) - np.where(yb, eta, 0.0)))))
    return loss, A.T @ np.abs(wv * r), A.T @ (A * np.abs(wv * (p * q))[:, None])


def reason_codes_host(shortfall_rows: np.ndarray, top: int) -> np.ndarray:
    """int32 ``[N, top]``: per row the features with the largest shortfall, largest first, ties to the lower
    feature index, -1 once the shortfall is 0 (``shortfall_rows``: float64 ``[N, F]``, >= 0)."""
    if not 0 <= int(top) <= MAX_TOP:
        raise ValueError(f"top must lie in 0 .. {MAX_TOP}, got {top}")
    s = np.asarray(shortfall_rows, dtype=np.float64)
    N, F = s.shape
    out = np.full((N, int(top)), -1, dtype=np.int32)
    order = np.argsort(-s, axis=1, kind="stable")[:, :top]
    val = np.take_along_axis(s, order, axis=1)
    k = order.shape[1]
    out[:, :k] = np.where(val > 0.0, order, -1)
    return out


def scorecard_score_host(X, edges_list, beta0: float, contrib, ipoints, shortfall, top: int):
    """``(margin float64 [N], integer score int32 [N], reasons int32 [N, top])`` of the rows of ``X``: the margin
    is ``beta0`` plus the per-cell contributions (``contrib``, float64 ``[cells]``) added in feature order, the
    integer score the sum of the row's ``ipoints`` cells, the reasons :func:`reason_codes_host` of its
    ``shortfall`` cells. The definition of ``k_sc_score``."""
    codes = scorecard_encode_host(X, edges_list).astype(np.int64)
    ptr = cell_pointer([check_drift_edges(z) for z in edges_list])
    contrib = np.asarray(contrib, dtype=np.float64)
    ipoints = np.asarray(ipoints, dtype=np.int32)
    shortfall = np.asarray(shortfall, dtype=np.float64)
    N, F = codes.shape
    m = np.full(N, float(beta0), dtype=np.float64)
    pts = np.zeros(N, dtype=np.int32)
    sf = np.empty((N, F), dtype=np.float64)
    for f in range(F):
        cell = ptr[f] + codes[:, f]
        m = m + contrib[cell]
        pts = pts + ipoints[cell]
        sf[:, f] = shortfall[cell]
    return m, pts, reason_codes_host(sf, top)


# ------------------------------------------------------------------------------------------------------ the fit
def fit_newton(newton_pass, n_coef: int, keep: Sequence[int], sum_w: float, *, l2: float = 0.0, gtol: float = 1e-9,
               max_iter: int = 50) -> tuple[np.ndarray, dict[str, Any]]:
    """Newton's method on ``newton_pass(beta) -> (loss, grad, hess)`` (NumPy float64), one driver for the host
    and the device pass. Only the coefficients ``keep`` (0 is the intercept) move; ``l2`` is added on the host
    to the non-intercept diagonal; the system is solved by Cholesky; the step is halved while the loss rises;
    the fit stops when ``max |grad| <= gtol sum_w`` or after ``max_iter`` passes. Returns ``(beta, info)``."""
    keep = np.asarray(sorted(set(int(k) for k in keep) | {0}), dtype=np.int64)
    pen = np.where(keep > 0, float(l2), 0.0)
    beta = np.zeros(n_coef, dtype=np.float64)

    def evaluate(b):
        loss, g, H = newton_pass(b)
        g, H = np.asarray(g, dtype=np.float64), np.asarray(H, dtype=np.float64)
        bk = b[keep]
        return (float(loss) + 0.5 * float(np.sum(pen * bk * bk)), g[keep] + pen * bk,
                H[np.ix_(keep, keep)] + np.diag(pen))

    loss, g, H = evaluate(beta)
    passes, converged = 1, False
    while True:
        if float(np.max(np.abs(g))) <= gtol * sum_w:
            converged = True
            break
        if passes >= max_iter:
            break
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError as e:
            raise ValueError("the Hessian of the scorecard fit is not positive definite (two characteristics "
                             "carry the same information, or the classes separate): set l2 > 0") from e
        step = np.linalg.solve(L.T, np.linalg.solve(L, g))
        t, moved = 1.0, False
        while passes < max_iter and t >= 2.0 ** -40:
            cand = beta.copy()
            cand[keep] = beta[keep] - t * step
            l2_, g2, H2 = evaluate(cand)
            passes += 1
            if l2_ <= loss:
                beta, loss, g, H, moved = cand, l2_, g2, H2, True
                break
            t *= 0.5
        if not moved:
            break
    return beta, {"passes": passes, "converged": converged, "loss": loss, "max_grad": float(np.max(np.abs(g)))}


def _f64_hex(v) -> list[str]:
    return [float(x).hex() for x in np.asarray(v, dtype=np.float64).reshape(-1)]


def _f32_hex(v) -> list[str]:
    return [float(x).hex() for x in np.asarray(v, dtype=np.float32).reshape(-1)]


class Scorecard:
    """The WoE points scorecard (module docstring). ``fit`` on NumPy / CPU input runs on the host, on CUDA tensors
    on their device; both give the same bins and WoE and coefficients that agree to the solver's tolerance. All
    public results are NumPy arrays.

    ``monotone``: ``"auto"``, ``+1``, ``-1``, ``0``, or a ``{feature name: direction}`` dict (features it does
    not name are ``"auto"``). ``pdo``: points that double the odds good:bad; a score of ``base_points`` means odds
    of ``base_odds`` : 1."""

    def __init__(self, n_fine: int = 20, max_bins: int = 6, min_bin_share: float = 0.05, monotone="auto",
                 l2: float = 0.0, pdo: float = 20.0, base_points: float = 600.0, base_odds: float = 50.0,
                 round_points: bool = True, gtol: float = 1e-9, max_iter: int = 50):
        if not 1 <= int(n_fine) <= MAX_FEATURE_CELLS - 2:
            raise ValueError(f"n_fine must lie in 1 .. {MAX_FEATURE_CELLS - 2} (at most {MAX_FEATURE_CELLS} cells "
                             f"per feature, so that codes fit in uint8)")
        if not pdo > 0 or not base_odds > 0 or l2 < 0:
            raise ValueError("pdo and base_odds must be positive, l2 non-negative")
        self.n_fine, self.max_bins, self.min_bin_share = int(n_fine), int(max_bins), float(min_bin_share)
        self.monotone, self.l2 = monotone, float(l2)
        self.pdo, self.base_points, self.base_odds = float(pdo), float(base_points), float(base_odds)
        self.round_points, self.gtol, self.max_iter = bool(round_points), float(gtol), int(max_iter)
        self.feature_names: list[str] | None = None

    # ---- fit
    def _direction(self, name: str):
        if isinstance(self.monotone, dict):
            return self.monotone.get(name, "auto")
        return self.monotone

    def fit(self, X, y, sample_weight=None, feature_names: Sequence[str] | None = None) -> "Scorecard":
        names = list(feature_names) if feature_names is not None else None
        if names is None and hasattr(X, "columns"):
            names = [str(c) for c in X.columns]
        X = _matrix(X, names)
        if X.ndim != 2 or X.shape[0] == 0 or X.shape[1] == 0:
            raise ValueError(f"X must be [rows, features] with rows, got shape {tuple(X.shape)}")
        n, F = X.shape
        names = names if names is not None else [f"f{i}" for i in range(F)]
        if len(names) != F:
            raise ValueError(f"{F} columns but {len(names)} feature names")
        gpu = _on_gpu(X)
        if gpu and F > GPU_MAX_FEATURES:
            raise ValueError(f"the GPU scorecard takes at most {GPU_MAX_FEATURES} features, got {F}")
        yv = _labels(y, n, X)
        wq = _quantized(sample_weight, n, X, None)
        Xh = X.cpu().numpy() if gpu else X
        fine = [drift_edges(Xh[:, f], self.n_fine) for f in range(F)]
        if gpu:
            from ..ops import monitor_ops

            counts = monitor_ops.bin_counts_gpu(X, fine, y=yv, wq=wq, wq_in_range=True).cpu().numpy()
            fptr = cell_pointer(fine)
        else:
            counts, fptr = bin_counts_host(X, fine, yv, wq)
        classes = [coarse_classing(counts[:, int(fptr[f]):int(fptr[f + 1])], fine[f], max_bins=self.max_bins,
                                   min_bin_share=self.min_bin_share, monotone=self._direction(names[f]))
                   for f in range(F)]
        self.feature_names = names
        self.edges = [c["edges"] for c in classes]
        self.counts = [c["counts"] for c in classes]
        self.woe = [c["woe"] for c in classes]
        self.iv = [c["iv"] for c in classes]
        self.direction = [c["direction"] for c in classes]
        self.missing_own_bin = [c["missing_own_bin"] for c in classes]
        self.dropped = [c["dropped"] for c in classes]
        if all(self.dropped):
            raise ValueError("no characteristic is left with more than one bin")

        from ..ops import scorecard_ops as ops

        codes = ops.scorecard_encode(X, self.edges)
        ptr = cell_pointer(self.edges)
        tab = np.concatenate(self.woe)
        if sample_weight is None:
            w, sum_w = None, float(n)
        elif gpu:
            w = torch.as_tensor(sample_weight).reshape(-1).to(device=X.device, dtype=torch.float64)
            sum_w = float(w.sum())
        else:
            w = np.asarray(sample_weight.detach().cpu().numpy() if isinstance(sample_weight, torch.Tensor)
                           else sample_weight, dtype=np.float64).reshape(-1)
            sum_w = float(w.sum())
        newton = ops.newton_pass(codes, ptr, tab, yv, w)   # beta -> (loss, grad, hess) as NumPy
        keep = [0] + [f + 1 for f in range(F) if not self.dropped[f]]
        self.beta, self.fit_info = fit_newton(newton, F + 1, keep, sum_w, l2=self.l2, gtol=self.gtol,
                                              max_iter=self.max_iter)
        self._finish()
        return self

    # ---- points
    def _finish(self) -> None:
        """Everything derived from the bins, the WoE values and the coefficients: the per-cell tables the scoring
        reads. Deterministic float64 arithmetic, so a loaded model scores with the same bits."""
        F = len(self.edges)
        self.cell_ptr = cell_pointer(self.edges)
        kept = [f for f in range(F) if not self.dropped[f]]
        self.n_kept = len(kept)
        self.factor = self.pdo / math.log(2.0)
        self.offset = self.base_points - self.factor * math.log(self.base_odds)
        b0 = float(self.beta[0])
        self.contrib = np.concatenate([float(self.beta[f + 1]) * self.woe[f] for f in range(F)])
        self.points = [self.offset / self.n_kept - self.factor * (float(self.beta[f + 1]) * self.woe[f] + b0 / self.n_kept)
                       if not self.dropped[f] else np.zeros_like(self.woe[f]) for f in range(F)]
        self.int_points = [np.rint(p).astype(np.int32) for p in self.points] if self.round_points \
            else [np.zeros(len(p), dtype=np.int32) for p in self.points]
        self.shortfall = np.concatenate([p.max() - p for p in self.points])

    def _check_fitted(self) -> None:
        if getattr(self, "beta", None) is None:
            raise ValueError("this Scorecard is not fitted")

    def _score_all(self, X, top: int):
        self._check_fitted()
        from ..ops import scorecard_ops as ops

        X = _matrix(X, self.feature_names)
        if X.ndim != 2 or X.shape[1] != len(self.edges):
            raise ValueError(f"X must be [rows, {len(self.edges)}], got shape {tuple(X.shape)}")
        m, pts, rs = ops.scorecard_score(X, self.edges, float(self.beta[0]), self.contrib,
                                         np.concatenate(self.int_points), self.shortfall, top)
        if isinstance(m, torch.Tensor):
            m, pts, rs = m.cpu().numpy(), pts.cpu().numpy(), rs.cpu().numpy()
        return m, pts, rs

    def encode(self, X) -> np.ndarray:
        """uint8 ``[N, F]``: the bin of every value (the row's line in :meth:`table` per characteristic)."""
        self._check_fitted()
        from ..ops import scorecard_ops as ops

        codes = ops.scorecard_encode(_matrix(X, self.feature_names), self.edges)
        return codes.cpu().numpy() if isinstance(codes, torch.Tensor) else codes

    def decision_function(self, X) -> np.ndarray:
        """float64 ``[N]``: the unrounded margin, the log-odds of bad."""
        return self._score_all(X, 0)[0]

    def predict_proba(self, X) -> np.ndarray:
        """float64 ``[N, 2]`` (good, bad), from the unrounded margin."""
        m = self.decision_function(X)
        e = np.exp(-np.abs(m))
        inv = 1.0 / (1.0 + e)
        p = np.where(m >= 0.0, inv, e * inv)
        q = np.where(m >= 0.0, e * inv, inv)
        return np.stack([q, p], axis=1)

    def predict(self, X) -> np.ndarray:
        return (self.decision_function(X) > 0.0).astype(np.int64)

    def score(self, X, rounded: bool | None = None) -> np.ndarray:
        """The points score of every row: the sum of the integer table (int32) with ``round_points`` (or
        ``rounded=True``), else ``offset - factor margin`` (float64)."""
        rounded = self.round_points if rounded is None else bool(rounded)
        if rounded and not self.round_points:
            raise ValueError("this scorecard has no integer table (round_points=False)")
        m, pts, _ = self._score_all(X, 0)
        return pts if rounded else self.offset - self.factor * m

    def reasons(self, X, top: int = 4) -> np.ndarray:
        """int32 ``[N, top]``: per row the characteristics furthest below their maximum points ("points below
        maximum"), largest shortfall first, ties to the lower feature index, -1 where none is left."""
        if not 1 <= int(top) <= MAX_TOP:
            raise ValueError(f"top must lie in 1 .. {MAX_TOP}, got {top}")
        return self._score_all(X, int(top))[2]

    # ---- the table
    def bin_labels(self, f: int) -> list[str]:
        z = self.edges[f]
        lo = ["-inf"] + [f"{float(v):g}" for v in z]
        hi = [f"{float(v):g}" for v in z] + ["+inf"]
        return [f"({a}, {b}]" if b != "+inf" else f"({a}, +inf)" for a, b in zip(lo, hi)] + ["missing"]

    def table(self) -> list[dict[str, Any]]:
        """One row per characteristic and bin: ``feature, bin, label, count, bad_rate, woe, iv`` (of the
        characteristic), ``coefficient, points`` (and ``int_points``), ``note`` ("dropped", "neutral: thin missing
        cell" or "")."""
        self._check_fitted()
        rows = []
        for f, name in enumerate(self.feature_names):
            c, labels = self.counts[f], self.bin_labels(f)
            for a in range(c.shape[1]):
                tot = int(c[0, a] + c[1, a])
                note = "dropped" if self.dropped[f] else \
                    "neutral: thin missing cell" if a == c.shape[1] - 1 and not self.missing_own_bin[f] else ""
                row = {"feature": name, "bin": a, "label": labels[a], "count": tot,
                       "bad_rate": float(c[1, a] / tot) if tot else float("nan"), "woe": float(self.woe[f][a]),
                       "iv": float(self.iv[f]), "coefficient": float(self.beta[f + 1]),
                       "points": float(self.points[f][a]), "note": note}
                if self.round_points:
                    row["int_points"] = int(self.int_points[f][a])
                rows.append(row)
        return rows

    # ---- persistence: float64 as float.hex, which round-trips exactly
    def to_dict(self) -> dict[str, Any]:
        self._check_fitted()
        params = {k: getattr(self, k) for k in ("n_fine", "max_bins", "min_bin_share", "monotone", "l2", "pdo",
                                                "base_points", "base_odds", "round_points", "gtol", "max_iter")}
        return {"version": 1, "kind": "woe_scorecard", "params": params, "feature_names": self.feature_names,
                "edges": [_f32_hex(z) for z in self.edges], "counts": [c.tolist() for c in self.counts],
                "woe": [_f64_hex(w) for w in self.woe], "iv": _f64_hex(self.iv), "direction": self.direction,
                "missing_own_bin": self.missing_own_bin, "dropped": self.dropped, "beta": _f64_hex(self.beta),
                "fit_info": self.fit_info}

    @classmethod
    def from_dict(cls, d: dict[str, Any]) -> "Scorecard":
        if d.get("version") != 1 or d.get("kind") != "woe_scorecard":
            raise ValueError(f"not a scorecard (version {d.get('version')!r}, kind {d.get('kind')!r})")
        sc = cls(**d["params"])
        sc.feature_names = list(d["feature_names"])
        sc.edges = [np.array([float.fromhex(v) for v in z], dtype=np.float32) for z in d["edges"]]
        sc.counts = [np.asarray(c, dtype=np.int64).reshape(2, -1) for c in d["counts"]]
        sc.woe = [np.array([float.fromhex(v) for v in w], dtype=np.float64) for w in d["woe"]]
        sc.iv = [float.fromhex(v) for v in d["iv"]]
        sc.direction = [int(v) for v in d["direction"]]
        sc.missing_own_bin = [bool(v) for v in d["missing_own_bin"]]
        sc.dropped = [bool(v) for v in d["dropped"]]
        sc.beta = np.array([float.fromhex(v) for v in d["beta"]], dtype=np.float64)
        sc.fit_info = dict(d.get("fit_info", {}))
        if not (len(sc.edges) == len(sc.woe) == len(sc.counts) == len(sc.feature_names) == len(sc.beta) - 1) or any(
                len(w) != len(z) + 2 or c.shape[1] != len(z) + 2 for z, w, c in zip(sc.edges, sc.woe, sc.counts)):
            raise ValueError("names, edges, counts, WoE values and coefficients do not describe one table")
        sc._finish()
        return sc

    def save(self, directory) -> str:
        """Writes ``scorecard.json`` into ``directory`` (created when missing); returns its path."""
        os.makedirs(directory, exist_ok=True)
        path = os.path.join(str(directory), "scorecard.json")
        with open(path, "w") as fh:
            json.dump(self.to_dict(), fh)
        return path

    @classmethod
    def load(cls, path) -> "Scorecard":
        """From ``scorecard.json`` or the directory that holds it."""
        path = str(path)
        if os.path.isdir(path):
            path = os.path.join(path, "scorecard.json")
        with open(path) as fh:
            return cls.from_dict(json.load(fh))

    def points_frame(self):
        """:meth:`table` as a pandas frame (what the command line writes to ``scorecard_points.csv``)."""
        import pandas as pd

        return pd.DataFrame(self.table())
