"""Score calibration: the isotonic fit, the piecewise-linear apply and the reliability table behind the
calibration report (ECE / MCE, the Murphy decomposition of the Brier score, calibration-in-the-large,
Hosmer-Lemeshow).

This module is the definition and the CPU path; ``csrc/calib.hip`` (through ``ops.calib_ops``) computes the same
integers, and from them the same floats, on the GPU. The calibrators built on it are in ``models.calibration``.

**Weights.** Every row has an integer weight: 1 without ``sample_weight``, else :func:`quantize_weights`
(``round(w * scale / max(w))`` with ``scale`` the largest power of two ``<= models.sketch.WEIGHT_SCALE`` that
keeps the total ``<= 2^31 - 1``). Rows of integer weight 0 are dropped. The bound on the total is what makes
every cross product of the hull test fit int64: each factor is below 2^31, and products are compared, never
subtracted.

**Isotonic regression** is the greatest convex minorant of the cumulative-sum diagram: stable-sort the rows by
float32 score, merge equal scores into groups (:func:`iso_groups`), take the strict lower convex hull of the
points ``(cw[k], cs[k])`` (:func:`iso_hull_host`); the groups between two consecutive hull vertices form one
block of PAV and its value is one fp64 division of two exact integers. :func:`iso_hull_tiled_host` is the
kernel's decomposition (tile hulls by log-step merges, two rounds, a final chain) and returns the same list.

**Reliability table** (:func:`reliability_sums_host`): int64 ``[3, B]``, per bin the weight ``W``, the weighted
positives ``S`` and ``Pq = sum wq * rint(p * 2^30)``. A bin is the number of interior edges ``<= p`` (intervals
are right-open, the last one closed). Interior edges are float32; an fp64 edge is rounded UP to float32
(:func:`edges_to_f32`), which leaves ``edge <= p`` unchanged for every float32 ``p``. Every figure of
:func:`reliability_report` is derived from this table, so the host and the device give the same report.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from ..models.sketch import WEIGHT_SCALE

MAX_ROWS = 1 << 28
MAX_TOTAL_WEIGHT = (1 << 31) - 1
MAX_BINS = 4096
P_SCALE = 1 << 30            # fixed point of the predicted probability in Pq
TABLE_FIELDS = ("W", "S", "Pq")
HULL_ROUNDS = 2              # tile rounds of the decomposition when the points do not fit one tile


# ------------------------------------------------------------------------------------------------ inputs
def _np(x) -> np.ndarray:
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _is_cuda(x) -> bool:
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


def quantize_weights(sample_weight, n: int):
    """Integer weights of ``n`` rows: None (every row 1) without ``sample_weight``, else int64
    ``round(w * (scale / max(w)))`` with ``scale = WEIGHT_SCALE / 2^k`` for the smallest ``k >= 0`` whose total is
    ``<= 2^31 - 1``. ``ValueError`` for negative or non-finite weights, a wrong length, or weights that are all 0."""
    if sample_weight is None:
        return None
    w = _np(sample_weight).astype(np.float64).reshape(-1)
    if w.shape[0] != n:
        raise ValueError(f"{w.shape[0]} weights, {n} rows")
    if n and (not np.isfinite(w).all() or (w < 0).any()):
        raise ValueError("sample_weight must be finite and >= 0")
    m = float(w.max()) if n else 0.0
    if m <= 0:
        raise ValueError("sample_weight has no positive entry")
    scale = float(WEIGHT_SCALE)
    est = float(w.sum()) / m
    while est * scale - 0.5 * n - 1.0 > MAX_TOTAL_WEIGHT:   # certainly too large: no need to round the rows
        scale *= 0.5
    while True:
        wq = np.round(w * (scale / m)).astype(np.int64)
        if int(wq.sum()) <= MAX_TOTAL_WEIGHT:
            return wq
        scale *= 0.5


def check_inputs(score, y, wq=None):
    """float32 scores, bool labels and int64 weights (or None) of the rows with a non-zero weight, after the
    refusals: labels outside {0, 1}, NaN scores, ``n < 1``, ``n > 2^28``, total weight ``> 2^31 - 1``."""
    s = _np(score).reshape(-1)
    yv = _np(y).reshape(-1)
    n = s.shape[0]
    if yv.shape[0] != n:
        raise ValueError(f"{yv.shape[0]} labels, {n} scores")
    if n < 1:
        raise ValueError("empty input")
    if n > MAX_ROWS:
        raise ValueError(f"at most 2^28 rows ({n} given)")
    if not np.all((yv == 0) | (yv == 1)):
        raise ValueError("labels must be 0 or 1")
    s = s.astype(np.float32)
    if np.isnan(s).any():
        raise ValueError("NaN scores")
    yb = yv.astype(bool)
    if wq is None:
        return s, yb, None
    wq = _np(wq).reshape(-1)
    if wq.shape[0] != n:
        raise ValueError(f"{wq.shape[0]} weights, {n} rows")
    if not np.issubdtype(wq.dtype, np.integer):
        raise ValueError("integer weights expected (quantize_weights)")
    wq = wq.astype(np.int64)
    if (wq < 0).any():
        raise ValueError("negative weight")
    if int(wq.max()) > MAX_TOTAL_WEIGHT or int(wq.sum()) > MAX_TOTAL_WEIGHT:   # n * max < 2^59: the sum is exact
        raise ValueError("total integer weight above 2^31 - 1")
    keep = wq > 0
    if not keep.all():
        s, yb, wq = s[keep], yb[keep], wq[keep]
        if s.shape[0] < 1:
            raise ValueError("every row has weight 0")
    return s, yb, wq


# ------------------------------------------------------------------------------------------------ isotonic
def iso_groups(score, y, wq=None):
    """``(ux float32 [G], cw int64 [G + 1], cs int64 [G + 1])``: the distinct scores in ascending order (a stable
    sort, runs of equal scores merged) and the cumulative weight / weighted positives before each group, with
    ``cw[0] = cs[0] = 0`` and ``cw`` strictly increasing."""
    s, yb, wq = check_inputs(score, y, wq)
    order = np.argsort(s, kind="stable")
    ss = s[order]
    w = np.ones(ss.shape[0], dtype=np.int64) if wq is None else wq[order]
    start = np.ones(ss.shape[0], dtype=bool)
    start[1:] = ss[1:] != ss[:-1]
    firsts = np.flatnonzero(start)
    cw = np.concatenate([[0], np.cumsum(w)])
    cs = np.concatenate([[0], np.cumsum(w * yb[order])])
    ends = np.concatenate([firsts[1:], [ss.shape[0]]])
    sel = np.concatenate([[0], ends])
    return ss[firsts], cw[sel].astype(np.int64), cs[sel].astype(np.int64)


def _check_cum(cw, cs):
    cw = np.asarray(cw, dtype=np.int64).reshape(-1)
    cs = np.asarray(cs, dtype=np.int64).reshape(-1)
    if cw.shape != cs.shape or cw.shape[0] < 2:
        raise ValueError("cw and cs must be two vectors of G + 1 >= 2 entries")
    if cw.shape[0] - 1 > MAX_ROWS:
        raise ValueError("more than 2^28 groups")
    if int(cw[-1]) > MAX_TOTAL_WEIGHT:
        raise ValueError("total integer weight above 2^31 - 1")
    return cw, cs


def _pop(cw, cs, a: int, b: int, k: int) -> bool:
    """Vertex ``b`` (above ``a`` on the stack) goes when ``k`` arrives: slope(a, b) >= slope(b, k), as a
    comparison of two products of factors below 2^31."""
    return (int(cs[b]) - int(cs[a])) * (int(cw[k]) - int(cw[b])) >= (int(cs[k]) - int(cs[b])) * (int(cw[b]) - int(cw[a]))


def _chain(cw, cs, idx) -> list[int]:
    st: list[int] = []
    for k in idx:
        k = int(k)
        while len(st) >= 2 and _pop(cw, cs, st[-2], st[-1], k):
            st.pop()
        st.append(k)
    return st


def iso_hull_host(cw, cs) -> np.ndarray:
    """int32 ascending indices of the strict lower convex hull of ``(cw[k], cs[k])``, 0 and G included; collinear
    interior points are dropped (adjacent blocks of equal mean are pooled). The monotone chain in exact integers."""
    cw, cs = _check_cum(cw, cs)
    return np.asarray(_chain(cw, cs, range(cw.shape[0])), dtype=np.int32)


def _tile_hull(cw, cs, idx: np.ndarray) -> np.ndarray:
    """The hull of the points ``idx`` (ascending) as a block of the tile kernel builds it: every point starts as
    a run of one, runs are merged pairwise in log steps. A merge pushes the right run's hull onto the left run's
    stack (a doubly linked list, so nothing moves) and stops at the first push after the right run's first that
    pops nothing: from there on the right hull's own links are already right."""
    n = idx.shape[0]
    nxt = np.zeros(n, dtype=np.int64)
    prv = np.zeros(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    h = 1
    while h < n:
        for a in range(0, n, 2 * h):
            m = a + h
            if m >= n:
                continue
            b = min(a + 2 * h, n)
            top, r, j = m - 1, m, 0
            while True:
                rn = -1 if r == b - 1 else int(nxt[r])
                popped = False
                while top != a:
                    p = int(prv[top])
                    if not _pop(cw, cs, int(idx[p]), int(idx[top]), int(idx[r])):
                        break
                    alive[top] = False
                    top = p
                    popped = True
                nxt[top] = r
                prv[r] = top
                if rn < 0 or (not popped and j >= 1):
                    break
                top, r, j = r, rn, j + 1
        h *= 2
    return idx[alive]


def iso_hull_tiled_host(cw, cs, tile_rows: int) -> np.ndarray:
    """The kernel's decomposition on the host, for any tile length ``>= 2``. A vertex of the whole set's hull is
    a vertex of the hull of any contiguous tile that holds it, so the hull of the union of tile hulls is the
    hull. Up to ``tile_rows`` points: one tile. Beyond: :data:`HULL_ROUNDS` rounds of tile hulls over the
    survivors (a fixed number, whatever they shed), then one tile when the survivors fit it, else the plain
    chain. Returns exactly :func:`iso_hull_host`'s list."""
    tile_rows = int(tile_rows)
    if tile_rows < 2:
        raise ValueError("tile_rows must be at least 2")
    cw, cs = _check_cum(cw, cs)
    idx = np.arange(cw.shape[0], dtype=np.int64)
    if idx.shape[0] > tile_rows:
        for _ in range(HULL_ROUNDS):
            idx = np.concatenate([_tile_hull(cw, cs, idx[a:a + tile_rows]) for a in range(0, idx.shape[0], tile_rows)])
    if idx.shape[0] <= tile_rows:
        return _tile_hull(cw, cs, idx).astype(np.int32)
    return np.asarray(_chain(cw, cs, idx), dtype=np.int32)


def block_values(hull, cw, cs) -> np.ndarray:
    """float64 value of every block ``[hull[i], hull[i + 1])``: one division of two exact integers."""
    hull = np.asarray(hull, dtype=np.int64)
    cw, cs = np.asarray(cw, dtype=np.int64), np.asarray(cs, dtype=np.int64)
    return (cs[hull[1:]] - cs[hull[:-1]]).astype(np.float64) / (cw[hull[1:]] - cw[hull[:-1]]).astype(np.float64)


def knots_from_blocks(x_first, x_last, first, last, values):
    """The knots from the blocks' first / last group (scores ``x_first`` / ``x_last``, group indices ``first`` /
    ``last``) and fp64 ``values``: both ends of every block (one point when the block is one group), then, as
    ``IsotonicRegression`` does, without the points whose value equals both neighbours'."""
    first, last = np.asarray(first, dtype=np.int64), np.asarray(last, dtype=np.int64)
    two = last > first
    nb = first.shape[0]
    pos = np.stack([np.ones(nb, dtype=bool), two], axis=1).reshape(-1)
    xs = np.stack([np.asarray(x_first, dtype=np.float32), np.asarray(x_last, dtype=np.float32)], axis=1).reshape(-1)[pos]
    vs = np.repeat(np.asarray(values, dtype=np.float64), 2)[pos]
    keep = np.ones(xs.shape[0], dtype=bool)
    if xs.shape[0] > 2:
        keep[1:-1] = (vs[1:-1] != vs[:-2]) | (vs[1:-1] != vs[2:])
    return xs[keep], vs[keep]


def iso_knots(ux, hull, cw, cs):
    """``(xk float32 [K], vk float64 [K])``: the fitted step function as ``sklearn.isotonic.IsotonicRegression``
    keeps it (``X_thresholds_``, ``y_thresholds_``): the per-group values without the interior points of
    constant runs."""
    ux = np.asarray(ux, dtype=np.float32)
    hull = np.asarray(hull, dtype=np.int64)
    first, last = hull[:-1], hull[1:] - 1
    return knots_from_blocks(ux[first], ux[last], first, last, block_values(hull, cw, cs))


def iso_fit_host(score, y, wq=None):
    """Knots of the isotonic fit of the 0/1 labels on the scores, on the host."""
    ux, cw, cs = iso_groups(score, y, wq)
    return iso_knots(ux, iso_hull_host(cw, cs), cw, cs)


def check_knots(xk, vk):
    xk = np.ascontiguousarray(_np(xk), dtype=np.float32).reshape(-1)
    vk = np.ascontiguousarray(_np(vk), dtype=np.float64).reshape(-1)
    if xk.shape[0] < 1 or xk.shape != vk.shape:
        raise ValueError("xk and vk must be two vectors of K >= 1 knots")
    if np.isnan(xk).any() or (xk.shape[0] > 1 and not np.all(xk[1:] > xk[:-1])):
        raise ValueError("knot positions must be strictly increasing")
    return xk, vk


def calib_apply_host(x, xk, vk, *, fp64: bool = False) -> np.ndarray:
    """float32 ``[N]``: the piecewise-linear function through the knots at ``x`` (float32), clipped to the knots'
    range. With ``xk[j] <= x < xk[j + 1]``: ``vk[j] + (vk[j+1] - vk[j]) * ((double)x - xk[j]) /
    ((double)xk[j+1] - xk[j])`` in fp64, in this order, rounded to float32. One knot: the constant. NaN gives NaN.
    ``fp64`` returns the fp64 values before that last rounding."""
    xk, vk = check_knots(xk, vk)
    x = np.asarray(_np(x), dtype=np.float32).reshape(-1)
    K = xk.shape[0]
    nan = np.isnan(x)
    if K == 1:
        r = np.full(x.shape[0], vk[0], dtype=np.float64)
    else:
        xc = np.clip(np.where(nan, xk[0], x), xk[0], xk[-1]).astype(np.float32)
        j = np.clip(np.searchsorted(xk, xc, side="right") - 1, 0, K - 2)
        x0, x1 = xk[j].astype(np.float64), xk[j + 1].astype(np.float64)
        v0, v1 = vk[j], vk[j + 1]
        with np.errstate(over="ignore", invalid="ignore"):
            r = v0 + (v1 - v0) * (xc.astype(np.float64) - x0) / (x1 - x0)
    r[nan] = np.nan
    return r if fp64 else r.astype(np.float32)


# ------------------------------------------------------------------------------------------------ reliability
def edges_to_f32(edges64) -> np.ndarray:
    """float32 interior edges from fp64 ones, each rounded UP (the smallest float32 ``>= e``): for a float32 ``p``,
    ``e32 <= p`` exactly when ``e <= p``."""
    e = np.asarray(edges64, dtype=np.float64).reshape(-1)
    e32 = e.astype(np.float32)
    low = e32.astype(np.float64) < e
    e32[low] = np.nextafter(e32[low], np.float32(np.inf))
    return e32


def check_edges(edges) -> np.ndarray:
    e = np.ascontiguousarray(_np(edges), dtype=np.float32).reshape(-1)
    if e.shape[0] + 1 > MAX_BINS:
        raise ValueError(f"at most {MAX_BINS} bins")
    if np.isnan(e).any() or (e.shape[0] > 1 and np.any(e[1:] < e[:-1])):
        raise ValueError("edges must be ascending and not NaN")
    return e


def reliability_sums_host(p, y, wq, edges) -> np.ndarray:
    """int64 ``[3, B]`` (``W``, ``S``, ``Pq``) of the float32 probabilities ``p`` in [0, 1], the 0/1 labels and the
    integer weights (None: 1 per row) over the ``B - 1`` float32 interior ``edges``: a row's bin is the number of
    edges ``<= p``."""
    e = check_edges(edges)
    p = np.asarray(_np(p), dtype=np.float32).reshape(-1)
    yv = _np(y).reshape(-1)
    if yv.shape[0] != p.shape[0]:
        raise ValueError(f"{yv.shape[0]} labels, {p.shape[0]} probabilities")
    if np.isnan(p).any():
        raise ValueError("NaN probabilities")
    if p.shape[0] and (p.min() < 0 or p.max() > 1):
        raise ValueError("probabilities must lie in [0, 1]")
    if not np.all((yv == 0) | (yv == 1)):
        raise ValueError("labels must be 0 or 1")
    w = np.ones(p.shape[0], dtype=np.int64) if wq is None else np.asarray(_np(wq)).reshape(-1).astype(np.int64)
    if w.shape[0] != p.shape[0]:
        raise ValueError(f"{w.shape[0]} weights, {p.shape[0]} rows")
    if (w < 0).any() or (w > WEIGHT_SCALE).any():
        raise ValueError("integer weights must lie in [0, 2^20]")
    B = e.shape[0] + 1
    b = np.searchsorted(e, p, side="right")
    q = np.rint(p.astype(np.float64) * float(P_SCALE)).astype(np.int64)
    out = np.zeros((3, B), dtype=np.int64)
    np.add.at(out[0], b, w)
    np.add.at(out[1], b, w * (yv != 0))
    np.add.at(out[2], b, w * q)
    return out


def _plain(x):
    x = float(x)
    return None if math.isnan(x) else x


@dataclass
class ReliabilityReport:
    """What :func:`reliability_report` returns. Per bin (arrays of ``n_bins``; NaN in an empty bin): ``count`` (the
    weight in units of the mean row weight), ``mean_predicted``, ``observed`` and ``gap = mean_predicted -
    observed``. ``brier`` is ``reliability - resolution + uncertainty`` over the bins: the Brier score of the
    scores replaced by their bin means (equal to the Brier score when scores are constant within bins).
    ``hl`` is the Hosmer-Lemeshow statistic over the non-empty bins and ``hl_pvalue`` its chi-square tail with
    ``hl_dof = non-empty bins - 2`` degrees of freedom (NaN when that is below 1)."""
    n: int
    n_bins: int
    strategy: str
    edges: np.ndarray
    count: np.ndarray
    mean_predicted: np.ndarray
    observed: np.ndarray
    gap: np.ndarray
    ece: float
    mce: float
    brier: float
    reliability: float
    resolution: float
    uncertainty: float
    calibration_in_the_large: float
    mean_predicted_all: float
    base_rate: float
    hl: float
    hl_dof: int
    hl_pvalue: float
    table: np.ndarray = field(repr=False, default=None)   # int64 [3, B]

    def to_dict(self) -> dict:
        d = {"n": int(self.n), "n_bins": int(self.n_bins), "strategy": self.strategy,
             "edges": [float(v) for v in self.edges],
             "bins": [{"count": _plain(c), "mean_predicted": _plain(m), "observed": _plain(o), "gap": _plain(g)}
                      for c, m, o, g in zip(self.count, self.mean_predicted, self.observed, self.gap)]}
        for k in ("ece", "mce", "brier", "reliability", "resolution", "uncertainty", "calibration_in_the_large",
                  "mean_predicted_all", "base_rate", "hl", "hl_pvalue"):
            d[k] = _plain(getattr(self, k))
        d["hl_dof"] = int(self.hl_dof)
        return d


def report_from_table(table, edges, n: int, strategy: str = "custom") -> ReliabilityReport:
    """The finishing arithmetic, one function for both paths: equal integers give equal floats."""
    from scipy.stats import chi2

    table = np.asarray(table, dtype=np.int64)
    W, S, Pq = (table[k].astype(np.float64) for k in range(3))
    B = table.shape[1]
    tot = float(table[0].sum())
    if tot <= 0:
        raise ValueError("no weight in the table")
    live = table[0] > 0
    Ws = np.where(live, W, 1.0)
    nan = np.full(B, np.nan)
    mp = np.where(live, Pq / (Ws * float(P_SCALE)), nan)
    ob = np.where(live, S / Ws, nan)
    gap = mp - ob
    share = W / tot
    g0 = np.where(live, gap, 0.0)
    base = float(table[1].sum()) / tot
    mean_all = float(table[2].sum()) / (tot * float(P_SCALE))
    rel = float(np.sum(share * g0 * g0))
    res = float(np.sum(share * np.where(live, ob - base, 0.0) ** 2))
    unc = base * (1.0 - base)
    # Hosmer-Lemeshow in units of rows: the table scaled by n / total weight
    unit = float(n) / tot
    num = (S - W * np.where(live, mp, 0.0)) ** 2
    den = W * np.where(live, mp * (1.0 - mp), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))
    hl = unit * float(np.sum(np.where(live, terms, 0.0)))
    dof = int(live.sum()) - 2
    pval = float(chi2.sf(hl, dof)) if dof >= 1 else math.nan
    return ReliabilityReport(n=int(n), n_bins=B, strategy=strategy, edges=np.asarray(edges, dtype=np.float32),
                             count=W * unit, mean_predicted=mp, observed=ob, gap=gap,
                             ece=float(np.sum(share * np.abs(g0))), mce=float(np.max(np.abs(g0))),
                             brier=rel - res + unc, reliability=rel, resolution=res, uncertainty=unc,
                             calibration_in_the_large=mean_all - base, mean_predicted_all=mean_all, base_rate=base,
                             hl=hl, hl_dof=dof, hl_pvalue=pval, table=table)


def quantile_positions(n: int, n_bins: int):
    """Where the ``n_bins - 1`` interior quantile edges sit in the sorted probabilities: ``(lo, hi, frac)`` with
    the edge ``s[lo] + (s[hi] - s[lo]) * frac`` in fp64 (linear interpolation at ``q * (n - 1)``)."""
    q = np.arange(1, n_bins, dtype=np.float64) / float(n_bins)
    pos = q * float(n - 1)
    lo = np.floor(pos).astype(np.int64)
    hi = np.minimum(lo + 1, n - 1)
    return lo, hi, pos - lo


def edges_for(strategy: str, n_bins: int, sorted_at=None, n: int = 0) -> np.ndarray:
    """float32 interior edges: ``uniform`` cuts [0, 1] into equal widths; ``quantile`` takes the unweighted
    quantiles of the probabilities, read through ``sorted_at(indices) -> values of the sorted vector``."""
    n_bins = int(n_bins)
    if n_bins < 1 or n_bins > MAX_BINS:
        raise ValueError(f"n_bins must lie in 1 .. {MAX_BINS}")
    if strategy == "uniform":
        return edges_to_f32(np.linspace(0.0, 1.0, n_bins + 1)[1:-1])
    if strategy != "quantile":
        raise ValueError("strategy must be 'quantile' or 'uniform'")
    lo, hi, frac = quantile_positions(n, n_bins)
    a = np.asarray(sorted_at(lo), dtype=np.float64)
    b = np.asarray(sorted_at(hi), dtype=np.float64)
    return edges_to_f32(a + (b - a) * frac)


def reliability_report(y, p, *, n_bins: int = 10, strategy: str = "quantile", sample_weight=None,
                       edges=None) -> ReliabilityReport:
    """The calibration report of the probabilities ``p`` (float32, in [0, 1]) against the 0/1 labels ``y``.
    ``strategy``: "quantile" (equal-count bins of ``p``, unweighted) or "uniform" (equal widths); ``edges``
    (ascending interior edges) overrides both. ``sample_weight`` is quantised as for the isotonic fit, capped at
    2^20 per row. CUDA tensors go to ``csrc/calib.hip``; everything else takes the host path; both give the same
    table and so the same report. ``ValueError`` for labels other than 0/1, NaN or out-of-range probabilities,
    no rows, more than 2^28 rows, more than 4096 bins."""
    on_gpu = _is_cuda(p) or _is_cuda(y)
    n = int(np.prod(tuple(p.shape))) if hasattr(p, "shape") else len(p)
    if n < 1:
        raise ValueError("empty input")
    if n > MAX_ROWS:
        raise ValueError(f"at most 2^28 rows ({n} given)")
    wq = quantize_weights(sample_weight, n)
    if on_gpu:
        from ..ops import calib_ops

        return calib_ops.reliability_report_gpu(y, p, wq, n_bins, strategy, edges)
    pv = np.asarray(_np(p), dtype=np.float32).reshape(-1)
    if edges is not None:
        e, strategy = check_edges(edges_to_f32(_np(edges))), "custom"
    else:
        srt = np.sort(pv) if strategy == "quantile" else None
        e = edges_for(strategy, n_bins, (lambda i: srt[i]) if srt is not None else None, n)
    return report_from_table(reliability_sums_host(pv, y, wq, e), e, n, strategy)
