"""Portfolio credit risk: what a book of calibrated PDs means for the lender. :func:`simulate_losses` runs the
Gaussian-copula factor model over the book (``csrc/portfolio.hip`` on the GPU, ``portfolio.loss`` on the host:
the same integers) and reports the loss distribution: expected loss, value-at-risk, expected shortfall and which
segment drives the tail."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from . import loss as L
from .loss import (portfolio_sums_host, portfolio_sums_tiled_host, probit_points, loss_amounts, scenario_offsets,
                   threshold_table)

__all__ = ["simulate_losses", "LossReport", "portfolio_sums_host", "portfolio_sums_tiled_host", "probit_points",
           "loss_amounts", "scenario_offsets", "threshold_table"]


def _is_cuda(x) -> bool:
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


def _to_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else (None if x is None else np.asarray(x))


def order_statistic(q: float, n: int) -> int:
    """The 1-based rank ``ceil(q n)`` (at least 1), with ``q`` read as the decimal it was written as."""
    return max(1, min(n, math.ceil(Fraction(str(float(q))) * n)))


def _qkey(q: float) -> str:
    return repr(float(q))


@dataclass
class LossReport:
    """What :func:`simulate_losses` returns. Money is in currency (the integer sums divided by ``unit``);
    ``var`` / ``es`` / ``unexpected_loss`` / ``asrf_var`` are keyed by the quantile. ``var[q]`` is the order
    statistic ``ceil(q S)`` of the sorted scenario losses, ``es[q]`` the mean of the losses at or above it.
    ``by_segment[name]`` holds the segment's ``expected_loss``, ``expected_loss_analytic``, ``default_rate`` and
    ``es_contribution[q]``: the mean of the segment's loss over the tail scenarios of ``es[q]`` (the Euler
    allocation). ``tail_units`` / ``by_segment[name]["tail_units"]`` keep the integer tail sums, in units: the
    segments' add up to the book's exactly."""
    n_loans: int
    n_scenarios: int
    n_sectors: int
    seed: int
    unit: int
    quantiles: tuple
    expected_loss: float
    expected_loss_analytic: float
    std: float
    var: dict
    es: dict
    unexpected_loss: dict
    default_rate: dict
    by_segment: dict
    tail_units: dict
    tail_count: dict
    asrf_var: dict | None
    losses: np.ndarray = field(repr=False)
    sums: np.ndarray = field(repr=False)        # int64 [2, G, S], in units

    def to_dict(self) -> dict:
        return {"n_loans": self.n_loans, "n_scenarios": self.n_scenarios, "n_sectors": self.n_sectors,
                "seed": self.seed, "unit": self.unit, "quantiles": [float(q) for q in self.quantiles],
                "expected_loss": self.expected_loss, "expected_loss_analytic": self.expected_loss_analytic,
                "std": self.std, "var": dict(self.var), "es": dict(self.es),
                "unexpected_loss": dict(self.unexpected_loss), "default_rate": dict(self.default_rate),
                "by_segment": {k: {kk: (dict(vv) if isinstance(vv, dict) else vv) for kk, vv in v.items()}
                               for k, v in self.by_segment.items()},
                "tail_units": dict(self.tail_units), "tail_count": dict(self.tail_count),
                "asrf_var": None if self.asrf_var is None else dict(self.asrf_var),
                "losses": [float(v) for v in self.losses]}

    def to_frame(self):
        """One row per segment: EL, analytic EL, default rate and the ES contribution at every quantile."""
        import pandas as pd

        rows = []
        for name, seg in self.by_segment.items():
            row = {"segment": name, "n_loans": seg["n_loans"], "expected_loss": seg["expected_loss"],
                   "expected_loss_analytic": seg["expected_loss_analytic"], "default_rate": seg["default_rate"]}
            for q in self.quantiles:
                row[f"es_contribution_{_qkey(q)}"] = seg["es_contribution"][_qkey(q)]
            rows.append(row)
        return pd.DataFrame(rows)

    def summary(self) -> str:
        lines = [f"portfolio loss: {self.n_loans} loans, {self.n_scenarios} scenarios, {self.n_sectors} sector(s), "
                 f"seed {self.seed}",
                 f"  expected loss {self.expected_loss:,.2f} (analytic {self.expected_loss_analytic:,.2f}), "
                 f"std {self.std:,.2f}, default rate {self.default_rate['mean']:.4%}"]
        for q in self.quantiles:
            k = _qkey(q)
            asrf = "" if self.asrf_var is None else f"  ASRF {self.asrf_var[k]:,.2f}"
            lines.append(f"  q={k}: VaR {self.var[k]:,.2f}  ES {self.es[k]:,.2f}  UL {self.unexpected_loss[k]:,.2f}"
                         + asrf)
        if len(self.by_segment) > 1:
            k = _qkey(self.quantiles[-1])
            lines.append(f"  by segment (EL; share of ES at q={k}):")
            for name, seg in self.by_segment.items():
                share = seg["es_contribution"][k] / self.es[k] if self.es[k] > 0 else 0.0
                lines.append(f"    {name}: {seg['expected_loss']:,.2f}; {share:.1%}")
        return "\n".join(lines)


def _segment_codes(segment, n: int):
    if segment is None:
        return np.zeros(n, dtype=np.int64), ["all"]
    s = _to_numpy(segment).reshape(-1)
    if s.shape[0] != n:
        raise ValueError(f"{n} loans, {s.shape[0]} segment labels")
    if np.issubdtype(s.dtype, np.integer):
        if n and (s.min() < 0 or s.max() >= L.MAX_SEGMENTS):
            raise ValueError(f"segment codes must lie in 0 .. {L.MAX_SEGMENTS - 1}")
        return s.astype(np.int64), [str(g) for g in range(int(s.max()) + 1 if n else 1)]
    names, codes = np.unique(s.astype(str), return_inverse=True)
    if len(names) > L.MAX_SEGMENTS:
        raise ValueError(f"at most {L.MAX_SEGMENTS} segments, got {len(names)}")
    return codes.astype(np.int64).reshape(-1), [str(v) for v in names]


def report_from_sums(sums: np.ndarray, *, pd, amounts, segment, names, quantiles, unit, seed, n_sectors,
                     asrf=None) -> LossReport:
    """The finishing arithmetic, one function for both paths: equal integers give equal reports."""
    sums = np.asarray(sums, dtype=np.int64)
    G, S = sums.shape[1], sums.shape[2]
    n = int(pd.shape[0])
    u = float(unit)
    total, dflt = sums[0].sum(axis=0), sums[1].sum(axis=0)
    order = np.argsort(total, kind="stable")
    srt = total[order]
    el = float(total.sum()) / (S * u) if S * u else 0.0
    analytic_i = pd * amounts.astype(np.float64)
    var, es, ul, tail_units, tail_count = {}, {}, {}, {}, {}
    seg_tail = {}
    for q in quantiles:
        k = _qkey(q)
        v = int(srt[order_statistic(q, S) - 1])
        tail = total >= v
        cnt = int(tail.sum())
        var[k] = v / u
        tail_units[k], tail_count[k] = int(total[tail].sum()), cnt
        es[k] = tail_units[k] / (cnt * u)
        ul[k] = var[k] - el
        seg_tail[k] = sums[0][:, tail].sum(axis=1)
    rate = dflt.astype(np.float64) / n
    rsrt = np.sort(rate)
    default_rate = {"mean": float(dflt.sum()) / (S * n)}
    for q in quantiles:
        default_rate[_qkey(q)] = float(rsrt[order_statistic(q, S) - 1])
    counts = np.bincount(segment, minlength=G)
    by_segment = {}
    for g, name in enumerate(names):
        by_segment[name] = {
            "n_loans": int(counts[g]),
            "expected_loss": float(sums[0, g].sum()) / (S * u),
            "expected_loss_analytic": float(analytic_i[segment == g].sum()) / u,
            "default_rate": float(sums[1, g].sum()) / (S * counts[g]) if counts[g] else 0.0,
            "tail_units": {k: int(seg_tail[k][g]) for k in seg_tail},
            "es_contribution": {k: int(seg_tail[k][g]) / (tail_count[k] * u) for k in seg_tail}}
    return LossReport(n_loans=n, n_scenarios=S, n_sectors=int(n_sectors), seed=int(seed), unit=int(unit),
                      quantiles=tuple(float(q) for q in quantiles), expected_loss=el,
                      expected_loss_analytic=float(analytic_i.sum()) / u,
                      std=float(np.std(total.astype(np.float64), ddof=1)) / u if S > 1 else 0.0,
                      var=var, es=es, unexpected_loss=ul, default_rate=default_rate, by_segment=by_segment,
                      tail_units=tail_units, tail_count=tail_count, asrf_var=asrf,
                      losses=total.astype(np.float64) / u, sums=sums)


def simulate_losses(pd, exposure, lgd=1.0, *, rho=0.15, sector=None, segment=None, n_scenarios: int = 10000,
                    seed: int = 0, scenarios=None, quantiles=(0.95, 0.99, 0.999), unit: int = 100, device=None,
                    single_factor: bool = False) -> LossReport:
    """Monte-Carlo loss distribution of a loan book under the Gaussian-copula factor model.

    ``pd``: calibrated default probabilities; ``exposure``: exposure at default; ``lgd``: a scalar or one value
    per loan; ``rho``: asset correlation, a scalar or one value per sector; ``sector``: integer sector ids
    (at most 16 sectors, one factor each; ``single_factor`` shares one factor between them); ``segment``: integer
    codes or strings (at most 64 distinct), for the per-segment breakdown; ``scenarios``: the caller's factor
    values ``[S]`` or ``[S, K]`` in place of the seeded standard normals (a stress test is e.g.
    ``numpy.full(S, -2.33)``); ``unit``: integer units per currency unit (100: cents).

    CUDA tensors, or ``device="cuda"``, take the GPU path; otherwise the host path runs. Both give the same
    integers and so the same report. ``ValueError`` for NaN, PDs outside [0, 1], negative amounts, amounts of
    2^32 units or more, ``rho`` outside [0, 1), more than 2^28 loans, 16 sectors or 64 segments."""
    on_gpu = (str(device).startswith("cuda") if device is not None
              else any(_is_cuda(x) for x in (pd, exposure, lgd, sector, segment)))
    dev = device if device is not None else next((x.device for x in (pd, exposure, lgd, sector, segment)
                                                  if _is_cuda(x)), None)
    p = _to_numpy(pd).astype(np.float64).reshape(-1)
    n = p.shape[0]
    if n < 1:
        raise ValueError("empty portfolio")
    if n > L.MAX_LOANS:
        raise ValueError(f"at most 2^28 loans ({n} given)")
    quantiles = tuple(float(q) for q in quantiles)
    if not quantiles or any(not 0.0 < q < 1.0 for q in quantiles):
        raise ValueError("quantiles must lie in (0, 1)")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits")
    lgd_np = _to_numpy(lgd) if hasattr(lgd, "shape") else lgd
    sec_np = _to_numpy(sector)
    amounts = loss_amounts(_to_numpy(exposure), lgd_np, unit)
    if amounts.shape[0] != n:
        raise ValueError(f"{n} PDs, {amounts.shape[0]} exposures")
    rho_np = _to_numpy(rho) if hasattr(rho, "shape") else rho
    rho_k, sec = L.resolve_sectors(rho_np, sec_np, n)
    K = rho_k.shape[0]
    Q = probit_points(p, rho_k, sec if K > 1 else None)
    z = None if scenarios is None else _to_numpy(scenarios).astype(np.float64)
    A = scenario_offsets(rho_k, n_scenarios, seed, n_sectors=K, single_factor=single_factor, scenarios=z)
    S = A.shape[0]
    seg, names = _segment_codes(segment, n)
    G = len(names)
    idx = np.arange(n, dtype=np.int64)
    step = L.MAX_SCENARIOS
    if on_gpu:
        import torch

        from ..ops import portfolio_ops

        d = torch.device(dev if dev is not None else "cuda")
        args = [torch.from_numpy(v).to(d) for v in (idx, Q, amounts.astype(np.int64), sec.astype(np.int64))]
        seg_d, table = torch.from_numpy(seg).to(d), torch.from_numpy(np.array(threshold_table())).to(d)
        parts = [portfolio_ops.portfolio_sums_gpu(*args, torch.from_numpy(A[b:b + step]).to(d), seed, segment=seg_d,
                                                  n_segments=G, rep0=b, table=table) for b in range(0, S, step)]
        sums = torch.cat(parts, dim=2).cpu().numpy()
    else:
        sums = np.concatenate([portfolio_sums_host(idx, Q, amounts, sec, A[b:b + step], seed, segment=seg,
                                                   n_segments=G, rep0=b) for b in range(0, S, step)], axis=2)
    asrf = None
    one_factor = K == 1 or single_factor or (z is not None and (z.ndim == 1 or z.shape[1] == 1))
    if one_factor:
        from scipy.special import ndtr, ndtri

        w = np.sqrt(rho_k)[sec]
        with np.errstate(invalid="ignore"):
            t = ndtri(p)
            asrf = {}
            for q in quantiles:
                cond = np.where(p <= 0, 0.0, np.where(p >= 1, 1.0, ndtr((t + w * ndtri(q)) / np.sqrt(1.0 - w * w))))
                asrf[_qkey(q)] = float((cond * amounts.astype(np.float64)).sum()) / float(unit)
    return report_from_sums(sums, pd=p, amounts=amounts, segment=seg, names=names, quantiles=quantiles, unit=unit,
                            seed=seed, n_sectors=K, asrf=asrf)
