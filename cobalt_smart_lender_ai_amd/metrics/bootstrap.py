"""Bootstrap confidence intervals for the discrimination metrics (AUC, Gini, KS), the operating point (error,
precision, recall, F1), optional logloss / Brier, and a paired champion / challenger comparison.

This module is the definition and the CPU path; ``csrc/bootstrap.hip`` (through ``ops.metrics_ops``) computes
the same integers on the GPU.

**Resampling.** The Poisson bootstrap: replicate ``b`` gives original row ``i`` a Poisson(1) count ``c[b, i]``.
A replicate's size ``sum_i c[b, i]`` is therefore close to ``n`` but not exactly ``n`` (mean ``n``, standard
deviation ``sqrt(n)``), unlike the multinomial bootstrap. The counts come from the counter-based generator
Philox4x32-10 with key ``(seed & 0xffffffff, seed >> 32)``, counter ``(i, b >> 2, 0, 0)`` and output word
``b & 3`` (one call serves four replicates of one row); the count is ``#{k : u >= T[k]}`` with ``T`` the
Poisson(1) CDF scaled to 2^32 (:data:`POISSON1_THRESHOLDS`; at most 12). They depend on the ORIGINAL row index,
never on the sorted position: two models scored on the same rows see the same resample, which makes the
comparison paired.

**Rank structure**, once per score vector: a stable sort of the float32 scores, a flag on the first row of every
run of equal scores, the original row of every sorted row (:func:`rank_structure`).

**Per-replicate integer sums** (:data:`FIELDS`), with ``pos_g`` / ``neg_g`` the count-weighted positives and
negatives of tie group ``g`` in ascending score order: ``P``, ``N``; ``U2 = sum_g pos_g (2 negbelow_g + neg_g)``
(``auc = U2 / (2 P N)``, ``gini = 2 auc - 1``); ``KSn = max_g |cumpos_g N - cumneg_g P|`` (``ks = KSn / (P N)``);
``TP`` / ``FP``, the counts of the rows with ``score > threshold``. Everything is an exact int64 (``n <= 2^28``
rows of at most 12 copies keep ``2 P N < 2^63``), so host and device agree exactly. The optional fp64 sums
``sum_i c_i t_i`` (logloss and Brier terms) are floating point and agree to rounding only.

A replicate with ``P = 0`` or ``N = 0`` has no rank metrics: its AUC, Gini and KS are NaN, it is counted in
``n_degenerate`` and left out of the percentiles. The operating-point metrics follow ``classification_report``
(0 for an empty denominator); logloss / Brier are NaN for an empty replicate.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
# floor(2^32 * PoissonCDF(k; 1)), k = 0 .. 11
POISSON1_THRESHOLDS = np.array([0x5e2d58d8, 0xbc5ab1b1, 0xeb715e1d, 0xfb239797, 0xff1025f5, 0xffd90f3b, 0xfffa8b71,
                                0xffff540c, 0xffffed1f, 0xfffffe21, 0xffffffd4, 0xfffffffc], dtype=np.uint64)
MAX_COUNT = len(POISSON1_THRESHOLDS)
MAX_ROWS = 1 << 28

FIELDS = ("P", "N", "U2", "KSn", "TP", "FP")
FLOAT_FIELDS = ("logloss_sum", "brier_sum")
RANK_METRICS = ("auc", "gini", "ks")
POINT_METRICS = ("error", "precision", "recall", "f1")
TERM_METRICS = ("logloss", "brier")
METRICS = RANK_METRICS + POINT_METRICS + TERM_METRICS

IDX_BITS = 28
LABEL_BIT, START_BIT, PRED_BIT = 1 << 28, 1 << 29, 1 << 30
_U32 = np.uint64(0xffffffff)
_HOST_CHUNK = 1 << 22  # count-matrix entries per chunk of replicates on the host


# ---------------------------------------------------------------------------------------------- the generator
def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10 on ``counter`` ``[..., 4]`` and ``key`` ``[..., 2]`` (broadcast against each other), as
    uint32 ``[..., 4]``. Vectorised in uint64 arithmetic: the 32 x 32 -> 64 products are exact."""
    c = np.asarray(counter, dtype=np.uint64) & _U32
    k = np.asarray(key, dtype=np.uint64) & _U32
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    x = [np.broadcast_to(c[..., j], shape) for j in range(4)]
    k0, k1 = np.broadcast_to(k[..., 0], shape), np.broadcast_to(k[..., 1], shape)
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * x[0], m1 * x[2]
        x = [(p1 >> s32) ^ x[1] ^ k0, p1 & _U32, (p0 >> s32) ^ x[3] ^ k1, p0 & _U32]
        k0 = (k0 + np.uint64(PHILOX_W0)) & _U32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _U32
    return np.stack(x, axis=-1).astype(np.uint32)


def poisson1_count(u) -> np.ndarray:
    """``#{k : u >= T[k]}`` for uint32 ``u``: a Poisson(1) count in 0 .. 12."""
    return np.searchsorted(POISSON1_THRESHOLDS, np.asarray(u, dtype=np.uint64), side="right").astype(np.uint8)


def bootstrap_counts_host(seed: int, rows, reps: int, rep0: int = 0) -> np.ndarray:
    """uint8 ``[reps, len(rows)]``: the count of original row ``rows[i]`` in replicate ``rep0 + b``. ``rows`` is
    a number of rows (``0 .. rows - 1``) or a vector of original row indices."""
    seed = int(seed) & 0xffffffffffffffff
    idx = np.arange(rows, dtype=np.uint64) if np.isscalar(rows) else np.asarray(rows, dtype=np.uint64).reshape(-1)
    reps, rep0 = int(reps), int(rep0)
    out = np.empty((reps, idx.shape[0]), dtype=np.uint8)
    key = np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64)
    ctr = np.zeros((idx.shape[0], 4), dtype=np.uint64)
    ctr[:, 0] = idx
    for q in range(rep0 >> 2, (rep0 + reps + 3) >> 2):
        ctr[:, 1] = q
        cnt = poisson1_count(philox4x32_10(ctr, key))            # [rows, 4]
        lo, hi = max(4 * q, rep0), min(4 * q + 4, rep0 + reps)
        out[lo - rep0:hi - rep0] = cnt[:, lo - 4 * q:hi - 4 * q].T
    return out


# ------------------------------------------------------------------------------------------- the rank structure
@dataclass
class RankStructure:
    """One score vector, sorted: ``order`` (original row of every sorted row), ``label`` / ``start`` / ``pred``
    (bool, in sorted order) and the packed ``words`` the kernel reads."""
    order: np.ndarray
    label: np.ndarray
    start: np.ndarray
    pred: np.ndarray

    @property
    def n(self) -> int:
        return int(self.order.shape[0])

    @property
    def words(self) -> np.ndarray:
        return pack_words(self.order, self.label, self.start, self.pred)


def pack_words(order, label, start, pred) -> np.ndarray:
    """uint32 per sorted row: original row index (28 bits), label bit, group-start bit, predicted-positive bit."""
    w = np.asarray(order, dtype=np.uint32)
    return (w | (np.asarray(label, bool).astype(np.uint32) << np.uint32(28))
            | (np.asarray(start, bool).astype(np.uint32) << np.uint32(29))
            | (np.asarray(pred, bool).astype(np.uint32) << np.uint32(30)))


def _check_inputs(y_true, y_score) -> tuple[np.ndarray, np.ndarray]:
    y = np.asarray(y_true).reshape(-1)
    s = np.asarray(y_score).reshape(-1)
    if s.shape[0] != y.shape[0]:
        raise ValueError(f"{y.shape[0]} labels, {s.shape[0]} scores")
    if y.shape[0] < 1:
        raise ValueError("empty input")
    if y.shape[0] > MAX_ROWS:
        raise ValueError(f"at most 2^28 rows ({y.shape[0]} given): beyond it 2 P N can pass 2^63")
    if not np.all((y == 0) | (y == 1)):
        raise ValueError("labels must be 0 or 1")
    s = s.astype(np.float32)
    if np.isnan(s).any():
        raise ValueError("NaN scores")
    return y.astype(bool), s


def rank_structure(y_true, y_score, threshold: float = 0.5) -> RankStructure:
    """Stable ascending sort of the float32 scores with the tie-group starts; ``pred`` is ``score > threshold``
    (the threshold rounded to float32, as the scores are)."""
    y, s = _check_inputs(y_true, y_score)
    order = np.argsort(s, kind="stable")
    ss = s[order]
    start = np.ones(ss.shape[0], dtype=bool)
    start[1:] = ss[1:] != ss[:-1]
    return RankStructure(order=order.astype(np.int64), label=y[order], start=start, pred=ss > np.float32(threshold))


def loss_terms(y_true, y_score, eps: float = 1e-15) -> np.ndarray:
    """float64 ``[2, n]`` in ORIGINAL row order: the logloss term of every row (scores clamped to
    ``[eps, 1 - eps]`` in fp64, as ``metrics.classification.log_loss`` does) and its Brier term."""
    y = np.asarray(y_true).reshape(-1).astype(np.float64)
    p = np.asarray(y_score).reshape(-1).astype(np.float32).astype(np.float64)
    q = np.clip(p, eps, 1 - eps)
    return np.stack([-(y * np.log(q) + (1 - y) * np.log1p(-q)), (p - y) ** 2])


# ------------------------------------------------------------------------------------------------ the sums, host
def _as_counts(counts, n: int) -> np.ndarray:
    c = np.asarray(counts)
    if c.ndim == 1:
        c = c[None, :]
    if c.ndim != 2 or c.shape[1] != n:
        raise ValueError(f"counts must be [replicates, {n}], got {c.shape}")
    return c


def _group_sums(c: np.ndarray, rs: RankStructure):
    """Count-weighted positives and negatives of every tie group: int64 ``[B, G]`` each."""
    firsts = np.flatnonzero(rs.start)
    pos = np.add.reduceat(c * rs.label[None, :], firsts, axis=1)
    neg = np.add.reduceat(c * ~rs.label[None, :], firsts, axis=1)
    return pos, neg


def bootstrap_sums_host(rs: RankStructure, counts, terms=None):
    """The direct form. ``counts``: integers ``[B, n]`` indexed by ORIGINAL row; ``terms``: float64 ``[2, n]`` in
    original row order or None. Returns int64 ``[6, B]`` (:data:`FIELDS`) and float64 ``[2, B]`` (zeros without
    terms; the float sums add the rows in sorted order)."""
    counts = _as_counts(counts, rs.n)
    B = counts.shape[0]
    ints = np.zeros((len(FIELDS), B), dtype=np.int64)
    fl = np.zeros((2, B), dtype=np.float64)
    step = max(1, _HOST_CHUNK // rs.n)
    for b0 in range(0, B, step):
        c = counts[b0:b0 + step][:, rs.order].astype(np.int64)
        pos, neg = _group_sums(c, rs)
        cpos, cneg = np.cumsum(pos, axis=1), np.cumsum(neg, axis=1)
        P, N = cpos[:, -1], cneg[:, -1]
        sl = slice(b0, b0 + c.shape[0])
        ints[0, sl], ints[1, sl] = P, N
        ints[2, sl] = (pos * (2 * (cneg - neg) + neg)).sum(axis=1)
        ints[3, sl] = np.abs(cpos * N[:, None] - cneg * P[:, None]).max(axis=1)
        ints[4, sl] = (c * (rs.pred & rs.label)[None, :]).sum(axis=1)
        ints[5, sl] = (c * (rs.pred & ~rs.label)[None, :]).sum(axis=1)
        if terms is not None:
            t = np.asarray(terms, dtype=np.float64)[:, rs.order]
            for k in range(2):
                fl[k, sl] = np.cumsum(c * t[k][None, :], axis=1)[:, -1]   # sequential, in sorted order
    return ints, fl


def bootstrap_sums_tiled_host(rs: RankStructure, counts, tile_rows: int, terms=None):
    """The kernel's decomposition on the host, for any tile length: per tile of ``tile_rows`` sorted rows a record
    (head ``Ph Nh``: the rows before the tile's first group start, the whole tile when it has none; middle
    ``Pm Nm Lm``: the complete groups between the first and the last start; tail ``Pt Nt``: from the last start
    on; ``TP FP``; the fp64 sums), then the two stitch recurrences over the tiles. Same returns as
    :func:`bootstrap_sums_host`, and the same integers."""
    tile_rows = int(tile_rows)
    if tile_rows < 1:
        raise ValueError("tile_rows must be positive")
    counts = _as_counts(counts, rs.n)
    n, B = rs.n, counts.shape[0]
    c = counts[:, rs.order].astype(np.int64)
    lab = rs.label
    t = None if terms is None else np.asarray(terms, dtype=np.float64)[:, rs.order]
    recs, ksrecs = [], []
    for a in range(0, n, tile_rows):
        b = min(a + tile_rows, n)
        ct, lt = c[:, a:b], lab[a:b]
        st = np.flatnonzero(rs.start[a:b])
        z = np.zeros(B, dtype=np.int64)
        rec = {"flag": len(st) > 0, "Pm": z, "Nm": z, "Lm": z, "Pt": z, "Nt": z, "st": st, "a": a, "b": b,
               "TP": (ct * (rs.pred[a:b] & lt)[None, :]).sum(axis=1),
               "FP": (ct * (rs.pred[a:b] & ~lt)[None, :]).sum(axis=1)}
        head = slice(0, st[0]) if len(st) else slice(0, b - a)
        rec["Ph"] = (ct[:, head] * lt[head][None, :]).sum(axis=1)
        rec["Nh"] = (ct[:, head] * ~lt[head][None, :]).sum(axis=1)
        if len(st):
            tail = slice(st[-1], b - a)
            rec["Pt"] = (ct[:, tail] * lt[tail][None, :]).sum(axis=1)
            rec["Nt"] = (ct[:, tail] * ~lt[tail][None, :]).sum(axis=1)
        if len(st) > 1:
            mid = slice(st[0], st[-1])
            firsts = st[:-1] - st[0]
            pos = np.add.reduceat(ct[:, mid] * lt[mid][None, :], firsts, axis=1)
            neg = np.add.reduceat(ct[:, mid] * ~lt[mid][None, :], firsts, axis=1)
            cneg = np.cumsum(neg, axis=1)
            rec["Pm"], rec["Nm"] = pos.sum(axis=1), neg.sum(axis=1)
            rec["Lm"] = (pos * (2 * (cneg - neg) + neg)).sum(axis=1)
            rec["mid"] = (np.cumsum(pos, axis=1), cneg)
        if t is not None:
            rec["fs"] = [np.cumsum(ct * t[k, a:b][None, :], axis=1)[:, -1] for k in range(2)]
        recs.append(rec)
    # stitch 1: AUC, the totals and the float sums
    ints = np.zeros((len(FIELDS), B), dtype=np.int64)
    fl = np.zeros((2, B), dtype=np.float64)
    Ncl, op, on, U2 = (np.zeros(B, dtype=np.int64) for _ in range(4))
    for rec in recs:
        op, on = op + rec["Ph"], on + rec["Nh"]
        if rec["flag"]:
            U2 = U2 + op * (2 * Ncl + on)
            Ncl = Ncl + on
            U2 = U2 + rec["Lm"] + 2 * rec["Pm"] * Ncl
            Ncl = Ncl + rec["Nm"]
            op, on = rec["Pt"], rec["Nt"]
        ints[0] += rec["Ph"] + rec["Pm"] + rec["Pt"]
        ints[1] += rec["Nh"] + rec["Nm"] + rec["Nt"]
        ints[4] += rec["TP"]
        ints[5] += rec["FP"]
        if t is not None:
            fl[0] = fl[0] + rec["fs"][0]
            fl[1] = fl[1] + rec["fs"][1]
    ints[2] = U2 + op * (2 * Ncl + on)
    # the second pass (it needs P and N) and its stitch: KS
    P, N = ints[0], ints[1]
    cp, cn, best = (np.zeros(B, dtype=np.int64) for _ in range(3))
    for rec in recs:
        cp, cn = cp + rec["Ph"], cn + rec["Nh"]
        if rec["flag"]:
            mx = mn = np.zeros(B, dtype=np.int64)
            if "mid" in rec:
                d = rec["mid"][0] * N[:, None] - rec["mid"][1] * P[:, None]
                mx, mn = np.maximum(d.max(axis=1), 0), np.minimum(d.min(axis=1), 0)
            off = cp * N - cn * P
            best = np.maximum(best, np.maximum(off + mx, -(off + mn)))
            cp, cn = cp + rec["Pm"] + rec["Pt"], cn + rec["Nm"] + rec["Nt"]
    ints[3] = best
    return ints, fl


# -------------------------------------------------------------------------------- from the sums to the metrics
def _ratio(num, den) -> np.ndarray:
    """``num / den`` in float64, 0 where the denominator is empty (``classification_report``'s convention)."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def metrics_from_sums(ints, fl, metrics) -> dict[str, np.ndarray]:
    """The finishing arithmetic, one function for both paths: equal integers give equal floats. ``ints``: int64
    ``[6, B]``; ``fl``: float64 ``[2, B]``. Returns ``{metric: float64 [B]}``, NaN where the metric does not
    exist (rank metrics with ``P = 0`` or ``N = 0``; logloss / Brier of an empty replicate)."""
    ints = np.asarray(ints, dtype=np.int64)
    P, N, U2, KSn, TP, FP = (ints[k] for k in range(6))
    Pf, Nf = P.astype(np.float64), N.astype(np.float64)
    ok = (P > 0) & (N > 0)
    pn = np.where(ok, Pf * Nf, 1.0)
    out = {}
    for m in metrics:
        if m == "auc":
            v = np.where(ok, U2.astype(np.float64) / (2.0 * pn), np.nan)
        elif m == "gini":
            v = np.where(ok, 2.0 * (U2.astype(np.float64) / (2.0 * pn)) - 1.0, np.nan)
        elif m == "ks":
            v = np.where(ok, KSn.astype(np.float64) / pn, np.nan)
        elif m == "error":
            v = _ratio(FP + (P - TP), P + N)
        elif m == "precision":
            v = _ratio(TP, TP + FP)
        elif m == "recall":
            v = _ratio(TP, P)
        elif m == "f1":
            p, r = _ratio(TP, TP + FP), _ratio(TP, P)
            v = _ratio(2.0 * p * r, p + r)
        elif m in TERM_METRICS:
            tot = Pf + Nf
            v = np.where(tot > 0, np.asarray(fl, dtype=np.float64)[TERM_METRICS.index(m)] / np.where(tot > 0, tot, 1.0),
                         np.nan)
        else:
            raise ValueError(f"unknown metric {m!r}; known: {', '.join(METRICS)}")
        out[m] = v.astype(np.float64)
    return out


def _interval(values: np.ndarray, alpha: float) -> tuple[float, float]:
    v = values[~np.isnan(values)]
    if v.size == 0:
        return (math.nan, math.nan)
    lo, hi = np.quantile(v, [alpha / 2, 1 - alpha / 2])
    return (float(lo), float(hi))


def _std(values: np.ndarray) -> float:
    v = values[~np.isnan(values)]
    return float(np.std(v, ddof=1)) if v.size > 1 else math.nan


def _plain(x):
    """Plain floats for ``json.dumps``: NaN becomes None (strict JSON has no NaN)."""
    x = float(x)
    return None if math.isnan(x) else x


@dataclass
class MetricInterval:
    """One metric: the point estimate (all counts 1), the replicate values (NaN where degenerate), their
    standard deviation (``ddof = 1``) and percentile interval over the non-NaN replicates."""
    point: float
    values: np.ndarray
    std: float
    low: float
    high: float
    n_degenerate: int

    def to_dict(self) -> dict:
        return {"point": _plain(self.point), "std": _plain(self.std), "low": _plain(self.low),
                "high": _plain(self.high), "n_degenerate": int(self.n_degenerate),
                "values": [_plain(v) for v in self.values]}


@dataclass
class MetricDelta:
    """The replicate-wise difference ``a - b`` of one metric: point difference, interval, and the share of the
    non-NaN replicates with a difference ``<= 0``."""
    point: float
    values: np.ndarray
    low: float
    high: float
    share_le_zero: float
    n_degenerate: int

    def to_dict(self) -> dict:
        return {"point": _plain(self.point), "low": _plain(self.low), "high": _plain(self.high),
                "share_le_zero": _plain(self.share_le_zero), "n_degenerate": int(self.n_degenerate),
                "values": [_plain(v) for v in self.values]}


@dataclass
class BootstrapReport:
    """What :func:`bootstrap_ci` returns: ``metrics[name]`` for model a, and with a second score vector
    ``metrics_b[name]`` and ``delta[name]`` (a - b on the same resamples)."""
    n: int
    n_boot: int
    alpha: float
    seed: int
    threshold: float
    metrics: dict[str, MetricInterval]
    metrics_b: dict[str, MetricInterval] | None = None
    delta: dict[str, MetricDelta] | None = None
    sums: dict = field(default_factory=dict, repr=False)   # "a" / "b": (int64 [6, B], float64 [2, B])

    def __getitem__(self, name: str) -> MetricInterval:
        return self.metrics[name]

    def to_dict(self) -> dict:
        d = {"n": int(self.n), "n_boot": int(self.n_boot), "alpha": float(self.alpha), "seed": int(self.seed),
             "threshold": float(self.threshold), "metrics": {k: v.to_dict() for k, v in self.metrics.items()}}
        if self.metrics_b is not None:
            d["metrics_b"] = {k: v.to_dict() for k, v in self.metrics_b.items()}
            d["delta"] = {k: v.to_dict() for k, v in self.delta.items()}
        return d


def _intervals(point_sums, rep_sums, metrics, alpha) -> dict[str, MetricInterval]:
    point = metrics_from_sums(*point_sums, metrics)
    reps = metrics_from_sums(*rep_sums, metrics)
    out = {}
    for m in metrics:
        v = reps[m]
        lo, hi = _interval(v, alpha)
        out[m] = MetricInterval(point=float(point[m][0]), values=v, std=_std(v), low=lo, high=hi,
                                n_degenerate=int(np.isnan(v).sum()))
    return out


def _is_cuda(x) -> bool:
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


def _to_numpy(x) -> np.ndarray:
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _sums_host(y, score, n_boot, seed, threshold, want_terms):
    rs = rank_structure(y, score, threshold)
    terms = loss_terms(y, score) if want_terms else None
    point = bootstrap_sums_host(rs, np.ones((1, rs.n), dtype=np.uint8), terms)
    ints = np.zeros((len(FIELDS), n_boot), dtype=np.int64)
    fl = np.zeros((2, n_boot), dtype=np.float64)
    step = max(4, (_HOST_CHUNK // rs.n) // 4 * 4)
    for b0 in range(0, n_boot, step):
        b1 = min(b0 + step, n_boot)
        ints[:, b0:b1], fl[:, b0:b1] = bootstrap_sums_host(rs, bootstrap_counts_host(seed, rs.n, b1 - b0, b0), terms)
    return point, (ints, fl)


def bootstrap_ci(y_true, y_score, y_score_b=None, *, metrics=("auc", "ks"), n_boot: int = 1000, alpha: float = 0.05,
                 seed: int = 0, threshold: float = 0.5, device=None, sample_weight=None) -> BootstrapReport:
    """Poisson-bootstrap percentile intervals of ``metrics`` (any of :data:`METRICS`) for the scores ``y_score``
    against the 0/1 labels ``y_true``, and, with ``y_score_b``, for a second model on the same rows and for the
    replicate-wise difference a - b (paired: both models see the same resamples).

    Inputs are NumPy arrays or tensors. CUDA tensors, or ``device="cuda"``, take the GPU path
    (``csrc/bootstrap.hip``); otherwise the host path runs. Both give the same integers and so the same report
    for the rank and operating-point metrics. ``threshold`` is in score units. Each replicate's size is close
    to ``n`` but not exactly ``n`` (Poisson bootstrap). ``ValueError`` for ``sample_weight`` (not supported),
    labels other than 0/1, NaN scores, ``n_boot < 1``, more than 2^28 rows, an unknown metric."""
    if sample_weight is not None:
        raise ValueError("sample_weight is not supported by bootstrap_ci")
    n_boot = int(n_boot)
    if n_boot < 1:
        raise ValueError("n_boot must be at least 1")
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError("alpha must lie in (0, 1)")
    metrics = tuple(metrics)
    for m in metrics:
        if m not in METRICS:
            raise ValueError(f"unknown metric {m!r}; known: {', '.join(METRICS)}")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits")
    want_terms = any(m in TERM_METRICS for m in metrics)
    on_gpu = (str(device).startswith("cuda") if device is not None
              else any(_is_cuda(x) for x in (y_true, y_score, y_score_b)))
    n = int(np.prod(tuple(y_true.shape))) if hasattr(y_true, "shape") else len(y_true)
    if n > MAX_ROWS:
        raise ValueError(f"at most 2^28 rows ({n} given): beyond it 2 P N can pass 2^63")
    if on_gpu:
        from ..ops import metrics_ops

        def sums(score):
            return metrics_ops.bootstrap_sums_for_ci(y_true, score, n_boot, seed, threshold, want_terms,
                                                     "ks" in metrics, device)
    else:
        y_np = _to_numpy(y_true)

        def sums(score):
            return _sums_host(y_np, _to_numpy(score), n_boot, seed, threshold, want_terms)

    point_a, reps_a = sums(y_score)
    rep = BootstrapReport(n=n, n_boot=n_boot, alpha=float(alpha), seed=seed, threshold=float(threshold),
                          metrics=_intervals(point_a, reps_a, metrics, alpha), sums={"a": reps_a})
    if y_score_b is not None:
        point_b, reps_b = sums(y_score_b)
        rep.metrics_b = _intervals(point_b, reps_b, metrics, alpha)
        rep.sums["b"] = reps_b
        rep.delta = {}
        for m in metrics:
            d = rep.metrics[m].values - rep.metrics_b[m].values
            live = d[~np.isnan(d)]
            lo, hi = _interval(d, alpha)
            rep.delta[m] = MetricDelta(point=rep.metrics[m].point - rep.metrics_b[m].point, values=d, low=lo, high=hi,
                                       share_le_zero=float((live <= 0).mean()) if live.size else math.nan,
                                       n_degenerate=int(np.isnan(d).sum()))
    return rep
