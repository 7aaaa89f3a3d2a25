"""Fair-lending audit of a credit model at its cutoff: does it treat protected groups differently?
:func:`fair_lending_audit` reports, per group against a reference group, the adverse impact ratio (with the
four-fifths rule), the statistical parity difference, the standardised mean difference of the score and, with
outcomes, the error-rate gaps, the calibration gap and the per-group AUC, each with a Poisson-bootstrap percentile
interval. The resamples are those of ``metrics.bootstrap_ci`` with the same seed, so the fairness report and the
accuracy report of one model are paired.

Every number is a ratio of the exact integer sums of ``fairness.sums`` (``csrc/fairness.hip`` on the GPU,
``fairness_sums_host`` on the host: the same integers), finished by one host function, so both paths give the
same report.

**The score grid.** Means and variances of the score (``smd``, ``calibration_gap``) are taken of
``q / 65536`` with ``q = min(floor(score * 65536), 65535)``: the score rounded down to a 16-bit grid, at most
``2^-16`` below the score itself. Variances are population variances (``ddof = 0``) under the replicate's counts.

**Decisions.** A row is declined when ``score > cutoff`` (both as float32) and approved otherwise, as
``explain.recourse`` approves at ``score <= cutoff``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from ..metrics import bootstrap as B
from ..metrics.bootstrap import MetricInterval, _interval, _plain, _std
from . import sums as S
from .sums import fairness_sums_host, fairness_sums_tiled_host, field_names

__all__ = ["fair_lending_audit", "FairnessReport", "AttributeAudit", "GroupAudit", "metrics_from_sums",
           "fairness_sums_host", "fairness_sums_tiled_host", "field_names", "verdict"]

BASE_METRICS = ("share", "approval_rate", "air", "parity_diff", "smd")
LABEL_METRICS = ("bad_rate", "declined_given_bad", "equal_opportunity_gap", "declined_given_good",
                 "false_positive_gap", "calibration_gap")
VERDICTS = ("adverse", "inconclusive", "pass")


def _is_cuda(x) -> bool:
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


def _to_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else (None if x is None else np.asarray(x))


def _div(num, den) -> np.ndarray:
    """``num / den`` in float64, NaN where the denominator is zero or NaN."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    ok = den > 0
    return np.where(ok, num / np.where(ok, den, 1.0), np.nan)


def metrics_from_sums(sums, ref: int, k: int = 0, labels: bool = False) -> dict[str, np.ndarray]:
    """The finishing arithmetic, one function for both paths: equal integers give equal floats. ``sums``: int64
    ``[4 + 2 K, G, B]``; ``ref``: the reference group's code; ``k``: the cutoff audited. Returns
    ``{metric: float64 [G, B]}``, NaN where a denominator is zero: a group that is empty in the replicate, a
    reference that approves nobody, a group with no bads (or no goods), a pooled variance of zero."""
    sums = np.asarray(sums, dtype=np.int64)
    K = (sums.shape[0] - len(S.FIXED_FIELDS)) // 2
    n, Bd, S1, S2 = sums[0], sums[1], sums[2], sums[3]
    D, DB = sums[4 + k], sums[4 + K + k]
    appr = _div(n - D, n)
    mean = _div(S1, n) / S.Q_SCALE
    var = np.maximum(_div(S2, n) / (S.Q_SCALE * S.Q_SCALE) - mean * mean, 0.0)
    pooled = (var + var[ref][None, :]) / 2.0
    with np.errstate(invalid="ignore"):
        out = {"share": _div(n, n.sum(axis=0)[None, :]),
               "approval_rate": appr,
               "air": _div(appr, appr[ref][None, :]),
               "parity_diff": appr - appr[ref][None, :],
               "smd": _div(mean - mean[ref][None, :], np.sqrt(pooled))}
        if labels:
            bad = _div(Bd, n)
            dgb, dgg = _div(DB, Bd), _div(D - DB, n - Bd)
            out.update({"bad_rate": bad, "declined_given_bad": dgb,
                        "equal_opportunity_gap": dgb - dgb[ref][None, :], "declined_given_good": dgg,
                        "false_positive_gap": dgg - dgg[ref][None, :], "calibration_gap": mean - bad})
    return out


def verdict(low: float, high: float, air_floor: float = 0.8) -> str:
    """The four-fifths rule on an interval of the adverse impact ratio: ``"adverse"`` when the upper end is below
    the floor, ``"pass"`` when the lower end is at or above it, ``"inconclusive"`` otherwise (the floor lies inside
    the interval, or there is no interval)."""
    if high < air_floor:
        return "adverse"
    if low >= air_floor:
        return "pass"
    return "inconclusive"


def _mi(point: float, values: np.ndarray, alpha: float) -> MetricInterval:
    values = np.asarray(values, dtype=np.float64)
    lo, hi = _interval(values, alpha)
    return MetricInterval(point=float(point), values=values, std=_std(values), low=lo, high=hi,
                          n_degenerate=int(np.isnan(values).sum()))


def _mi_dict(m: MetricInterval, values: bool) -> dict:
    d = m.to_dict()
    if not values:
        d.pop("values")
    return d


@dataclass
class GroupAudit:
    """One group of one attribute: its size, whether it is the reference, the four-fifths ``verdict`` and
    ``metrics[name]`` (point value, replicate values, standard error, percentile interval, degenerate
    replicates)."""
    name: str
    n: int
    is_reference: bool
    verdict: str
    metrics: dict[str, MetricInterval]

    def __getitem__(self, name: str) -> MetricInterval:
        return self.metrics[name]

    def to_dict(self, values: bool = False) -> dict:
        return {"name": self.name, "n": int(self.n), "is_reference": bool(self.is_reference),
                "verdict": self.verdict, "metrics": {k: _mi_dict(v, values) for k, v in self.metrics.items()}}


@dataclass
class AttributeAudit:
    """One protected attribute: ``groups[name]`` in the order of the codes, the ``reference`` group, and for
    every cutoff of the grid the adverse impact ratio of every group (``curve[name][j]`` at ``cutoffs[j]``)."""
    name: str
    reference: str
    groups: dict[str, GroupAudit]
    cutoffs: list
    curve: dict[str, list]
    sums: dict = field(default_factory=dict, repr=False)   # "point" / "reps": int64 [4 + 2 K, G, .]

    def __getitem__(self, name: str) -> GroupAudit:
        return self.groups[name]

    def to_dict(self, values: bool = False) -> dict:
        return {"name": self.name, "reference": self.reference,
                "groups": {k: v.to_dict(values) for k, v in self.groups.items()},
                "cutoffs": [float(c) for c in self.cutoffs],
                "curve": {k: [_mi_dict(m, values) for m in v] for k, v in self.curve.items()}}


@dataclass
class FairnessReport:
    """What :func:`fair_lending_audit` returns: ``attributes[name]`` (a single group vector is the attribute
    ``"group"``)."""
    n: int
    n_boot: int
    alpha: float
    seed: int
    cutoff: float
    air_floor: float
    has_labels: bool
    attributes: dict[str, AttributeAudit]

    def __getitem__(self, name: str) -> AttributeAudit:
        return self.attributes[name]

    def table(self) -> list[dict]:
        """One row per attribute and group: ``attribute``, ``group``, ``n``, ``is_reference``, ``verdict`` and for
        every metric its point value and ``<metric>_low`` / ``<metric>_high`` / ``<metric>_std`` /
        ``<metric>_n_degenerate``."""
        rows = []
        for a in self.attributes.values():
            for g in a.groups.values():
                row = {"attribute": a.name, "group": g.name, "n": int(g.n), "is_reference": g.is_reference,
                       "verdict": g.verdict}
                for k, m in g.metrics.items():
                    row[k] = _plain(m.point)
                    row[k + "_low"], row[k + "_high"] = _plain(m.low), _plain(m.high)
                    row[k + "_std"], row[k + "_n_degenerate"] = _plain(m.std), int(m.n_degenerate)
                rows.append(row)
        return rows

    def air_curve(self) -> list[dict]:
        """The adverse impact ratio with its band at every cutoff of the grid (empty without ``cutoffs``): rows
        of ``attribute``, ``group``, ``cutoff``, ``air``, ``low``, ``high``, ``std``, ``n_degenerate``."""
        rows = []
        for a in self.attributes.values():
            for gname, curve in a.curve.items():
                for c, m in zip(a.cutoffs, curve):
                    rows.append({"attribute": a.name, "group": gname, "cutoff": float(c), "air": _plain(m.point),
                                 "low": _plain(m.low), "high": _plain(m.high), "std": _plain(m.std),
                                 "n_degenerate": int(m.n_degenerate)})
        return rows

    def to_dict(self, values: bool = False) -> dict:
        return {"n": int(self.n), "n_boot": int(self.n_boot), "alpha": float(self.alpha), "seed": int(self.seed),
                "cutoff": float(self.cutoff), "air_floor": float(self.air_floor), "has_labels": self.has_labels,
                "attributes": {k: v.to_dict(values) for k, v in self.attributes.items()}}

    def summary(self) -> str:
        pct = 100.0 * (1.0 - self.alpha)
        lines = [f"fair-lending audit: {self.n} rows, cutoff {self.cutoff:g} (declined above it), {self.n_boot} "
                 f"bootstrap replicates, {pct:g}% intervals, floor {self.air_floor:g}"]
        for a in self.attributes.values():
            lines.append(f"{a.name} (reference: {a.reference})")
            for g in a.groups.values():
                air, ap, smd = g["air"], g["approval_rate"], g["smd"]
                line = (f"  {g.name:<16} n={g.n:<9d} approved {ap.point:7.4f}  AIR {air.point:6.3f} "
                        f"[{air.low:6.3f}, {air.high:6.3f}]  SMD {smd.point:+6.3f}  {g.verdict}")
                if self.has_labels:
                    line += (f"  EO gap {g['equal_opportunity_gap'].point:+6.3f}  FP gap "
                             f"{g['false_positive_gap'].point:+6.3f}  AUC {g['auc'].point:5.3f}")
                lines.append(line)
        return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ the inputs
def _group_codes(v, names, n: int):
    """Codes (a NumPy int64 vector, or a CUDA int64 tensor when ``v`` is one) and the groups' names. Strings
    become sorted-unique codes; integers index ``names`` when it is given and otherwise become sorted-unique
    codes named by their value."""
    if _is_cuda(v):
        import torch

        t = v.reshape(-1)
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError("group must hold integer codes or strings")
        t = t.to(torch.int64)
        if t.shape[0] != n:
            raise ValueError(f"{n} scores, {t.shape[0]} group entries")
        if names is not None:
            lo, hi = (int(x) for x in torch.stack([t.min(), t.max()]).cpu())
            if lo < 0 or hi >= len(names):
                raise ValueError(f"group codes must lie in 0 .. {len(names) - 1}")
            return t, [str(x) for x in names]
        uniq = torch.unique(t)
        if uniq.shape[0] > S.MAX_GROUPS:
            raise ValueError(f"at most {S.MAX_GROUPS} groups, got {uniq.shape[0]}")
        return torch.searchsorted(uniq, t), [str(int(x)) for x in uniq.cpu()]
    a = _to_numpy(v).reshape(-1)
    if a.shape[0] != n:
        raise ValueError(f"{n} scores, {a.shape[0]} group entries")
    if a.dtype.kind in "iu":
        a = a.astype(np.int64)
        if names is not None:
            if a.min() < 0 or a.max() >= len(names):
                raise ValueError(f"group codes must lie in 0 .. {len(names) - 1}")
            return a, [str(x) for x in names]
        uniq, inv = np.unique(a, return_inverse=True)
        out = [str(int(x)) for x in uniq]
    elif a.dtype.kind in "USO":
        if names is not None:
            raise ValueError("group_names go with integer codes; strings name themselves")
        uniq, inv = np.unique(a.astype(str), return_inverse=True)
        out = [str(x) for x in uniq]
    else:
        raise ValueError("group must hold integer codes or strings")
    if len(out) > S.MAX_GROUPS:
        raise ValueError(f"at most {S.MAX_GROUPS} groups, got {len(out)}")
    return inv.reshape(-1).astype(np.int64), out


def _auc_sums(on_gpu, score, y, codes, g: int, cutoff: float, n_boot: int, seed: int):
    """The bootstrap sums (``metrics.bootstrap.FIELDS``) of group ``g``'s rows, point and replicates: the rank
    structure of the group alone, the counts of its ORIGINAL rows, so the resample is the audit's."""
    if on_gpu:
        import torch

        from ..ops import metrics_ops

        rows = torch.nonzero(codes == g).reshape(-1)
        if rows.shape[0] == 0:
            return None
        words, order = metrics_ops.rank_words_gpu(y[rows], score[rows], cutoff)
        words = ((words.to(torch.int64) & ~((1 << B.IDX_BITS) - 1)) | rows[order]).to(torch.int32).contiguous()
        point, _ = metrics_ops.bootstrap_sums_gpu(words, 1, seed, ks=False, unit=True)
        reps, _ = metrics_ops.bootstrap_sums_gpu(words, n_boot, seed, ks=False)
        return point.cpu().numpy(), reps.cpu().numpy()
    rows = np.flatnonzero(codes == g)
    if rows.shape[0] == 0:
        return None
    rs = B.rank_structure(y[rows], score[rows], cutoff)
    point, _ = B.bootstrap_sums_host(rs, np.ones((1, rs.n), dtype=np.uint8))
    reps = np.zeros((len(B.FIELDS), n_boot), dtype=np.int64)
    step = max(4, (B._HOST_CHUNK // rs.n) // 4 * 4)
    for b0 in range(0, n_boot, step):
        b1 = min(b0 + step, n_boot)
        reps[:, b0:b1], _ = B.bootstrap_sums_host(rs, B.bootstrap_counts_host(seed, rows, b1 - b0, b0))
    return point, reps


def _audit(name, score, codes, names, y, cuts, n_boot, alpha, seed, air_floor, reference, on_gpu) -> AttributeAudit:
    G = len(names)
    if on_gpu:
        from ..ops import fairness_ops

        point = fairness_ops.fairness_sums_gpu(score, codes, y, cuts, 1, seed, n_groups=G, unit=True).cpu().numpy()
        reps = np.concatenate([fairness_ops.fairness_sums_gpu(score, codes, y, cuts, min(S.MAX_REPS, n_boot - b),
                                                              seed, b, n_groups=G).cpu().numpy()
                               for b in range(0, n_boot, S.MAX_REPS)], axis=2)
    else:
        point = fairness_sums_host(score, codes, y, cuts, seed, 1, n_groups=G, unit=True)
        reps = np.concatenate([fairness_sums_host(score, codes, y, cuts, seed, min(S.MAX_REPS, n_boot - b), b,
                                                  n_groups=G) for b in range(0, n_boot, S.MAX_REPS)], axis=2)
    if reference is None:
        ref = int(np.argmax(np.nan_to_num(_div(point[0, :, 0] - point[4, :, 0], point[0, :, 0]), nan=-1.0)))
    else:
        if str(reference) not in names:
            raise ValueError(f"unknown reference {reference!r} for {name}; groups: {', '.join(names)}")
        ref = names.index(str(reference))
    labels = y is not None
    pm, rm = metrics_from_sums(point, ref, 0, labels), metrics_from_sums(reps, ref, 0, labels)
    groups = {}
    for g, gname in enumerate(names):
        metrics = {m: _mi(pm[m][g, 0], rm[m][g], alpha) for m in pm}
        if labels:
            auc = _auc_sums(on_gpu, score, y, codes, g, float(cuts[0]), n_boot, seed)
            if auc is None:
                metrics["auc"] = _mi(math.nan, np.full(n_boot, np.nan), alpha)
            else:
                zeros = np.zeros((2, 1))
                metrics["auc"] = _mi(B.metrics_from_sums(auc[0], zeros, ("auc",))["auc"][0],
                                     B.metrics_from_sums(auc[1], zeros, ("auc",))["auc"], alpha)
        air = metrics["air"]
        groups[gname] = GroupAudit(name=gname, n=int(point[0, g, 0]), is_reference=g == ref,
                                   verdict=verdict(air.low, air.high, air_floor), metrics=metrics)
    curve = {gname: [] for gname in names} if len(cuts) > 1 else {}
    for k in range(1, len(cuts)):
        pk, rk = metrics_from_sums(point, ref, k)["air"], metrics_from_sums(reps, ref, k)["air"]
        for g, gname in enumerate(names):
            curve[gname].append(_mi(pk[g, 0], rk[g], alpha))
    return AttributeAudit(name=name, reference=names[ref], groups=groups, cutoffs=[float(c) for c in cuts[1:]],
                          curve=curve, sums={"point": point, "reps": reps})


def fair_lending_audit(p_default, group, y=None, *, cutoff: float = 0.5, reference=None, group_names=None,
                       cutoffs=None, n_boot: int = 1000, alpha: float = 0.05, seed: int = 0,
                       air_floor: float = 0.8) -> FairnessReport:
    """Audit the scores ``p_default`` (probabilities of default in ``[0, 1]``; a row is declined when its score
    is above ``cutoff``) for different treatment of the groups of ``group``.

    ``group``: a vector of integer codes, a vector of strings, or a dict ``{attribute: vector}`` (one audit per
    attribute, all on the same resamples). Strings become sorted-unique codes; integers are named by
    ``group_names`` (a list indexed by code, or a dict of lists for a dict of attributes) or else by their value.
    ``reference``: the comparison group's name (or a dict per attribute); by default the group with the highest
    approval rate. ``y``: 0/1 outcomes (1 = bad), which add the error-rate gaps, the calibration gap and the
    per-group AUC. ``cutoffs``: up to 15 further cutoffs for :meth:`FairnessReport.air_curve`.

    Per group the report holds ``n``, ``share``, ``approval_rate``, ``air`` (approval rate over the reference's),
    ``parity_diff``, ``smd`` (``(mean_g - mean_ref) / sqrt((var_g + var_ref) / 2)`` of the score on its 16-bit
    grid) and a four-fifths ``verdict`` (:func:`verdict`); with ``y`` also ``bad_rate``, ``declined_given_bad`` and
    its ``equal_opportunity_gap`` to the reference, ``declined_given_good`` and its ``false_positive_gap``,
    ``calibration_gap`` (mean score minus bad rate) and ``auc``. Every entry is a ``MetricInterval``; a replicate in
    which an entry's denominator is zero is NaN there, left out of its percentiles and counted in
    ``n_degenerate``.

    CUDA tensors are audited on their device (``csrc/fairness.hip``), NumPy arrays on the host; both give the
    same report. ``ValueError`` for NaN scores or scores outside ``[0, 1]``, labels other than 0/1, more than 64
    groups, more than 16 cutoffs in all, more than 2^27 rows, length mismatches, an unknown ``reference``."""
    n_boot = int(n_boot)
    if n_boot < 1:
        raise ValueError("n_boot must be at least 1")
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError("alpha must lie in (0, 1)")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits")
    cuts = S.check_cutoffs([float(cutoff)] + ([] if cutoffs is None else [float(c) for c in _to_numpy(cutoffs)]))
    attrs = group if isinstance(group, dict) else {"group": group}
    if not attrs:
        raise ValueError("no attribute to audit")
    as_dict = isinstance(group, dict)
    on_gpu = _is_cuda(p_default) or _is_cuda(y) or any(_is_cuda(v) for v in attrs.values())
    n = int(np.prod(tuple(p_default.shape))) if hasattr(p_default, "shape") else len(p_default)
    if n < 1:
        raise ValueError("empty input")
    if n > S.MAX_ROWS:
        raise ValueError(f"at most 2^27 rows ({n} given)")
    if on_gpu:
        import torch

        dev = next(x.device for x in [p_default, y, *attrs.values()] if _is_cuda(x))

        def up(x):
            return None if x is None else (x if isinstance(x, torch.Tensor) else torch.from_numpy(
                np.ascontiguousarray(x))).to(dev).reshape(-1)
        score, yy = up(p_default), up(y)
        if not score.dtype.is_floating_point:
            score = score.to(torch.float32)
    else:
        up = None
        score = _to_numpy(p_default).reshape(-1)
        yy = None if y is None else _to_numpy(y).reshape(-1)
        S.score_grid(score)
    if yy is not None and yy.shape[0] != n:
        raise ValueError(f"{n} scores, {yy.shape[0]} labels")
    audits = {}
    for name, v in attrs.items():
        names = group_names.get(name) if as_dict and isinstance(group_names, dict) else group_names
        ref = reference.get(name) if as_dict and isinstance(reference, dict) else reference
        codes, names = _group_codes(v, names, n)
        if on_gpu and not _is_cuda(codes):
            codes = up(codes)
        audits[str(name)] = _audit(str(name), score, codes, names, yy, cuts, n_boot, float(alpha), seed,
                                   float(air_floor), ref, on_gpu)
    return FairnessReport(n=n, n_boot=n_boot, alpha=float(alpha), seed=seed, cutoff=float(cutoff),
                          air_floor=float(air_floor), has_labels=y is not None, attributes=audits)
