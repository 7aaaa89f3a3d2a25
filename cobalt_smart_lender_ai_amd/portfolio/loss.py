"""The portfolio credit-loss simulation, defined in integers: the definition and the CPU path.
``csrc/portfolio.hip`` (through ``ops.portfolio_ops``) computes the same integers on the GPU.

**Model.** The Gaussian-copula factor model with one factor per sector: loan ``i`` of sector ``k`` defaults in
scenario ``s`` when ``w_k Z_sk + sqrt(1 - w_k^2) eps_is < t_i`` with ``t_i = Phi^-1(PD_i)`` and
``w_k = sqrt(rho_k)``. Given ``Z`` that is a Bernoulli draw with probability
``Phi((t_i - w_k Z_sk) / sqrt(1 - w_k^2))``; the loss on default is ``EAD_i LGD_i``.

**Prepared once, in fp64 on the host** (both paths share this code):

* ``L_i = round(EAD_i LGD_i unit)`` as uint32 (:func:`loss_amounts`);
* ``Q_i = round(t_i / sqrt(1 - w_k^2) 2^20)`` as int32, clamped to +-2^30 (:func:`probit_points`);
* ``A_sk = round(w_k Z_sk / sqrt(1 - w_k^2) 2^20)`` as int32 ``[S, K]``, clamped to +-2^29
  (:func:`scenario_offsets`);
* ``T[j] = floor(Phi(-8 + j 2^-9) 2^32)``, ``j = 0 .. 8192``, int64, with ``T[0] = 0`` and ``T[8192] = 2^32`` by
  definition (:func:`threshold_table`).

**A draw**, integers only (:func:`draw_thresholds`, :func:`draw_uniforms`): with
``X = clamp(Q_i - A_sk + 8 2^20, 0, 16 2^20)``, ``j = X >> 11`` and ``f = X & 2047`` the threshold is
``thr = T[j] + (((T[min(j + 1, 8192)] - T[j]) f) >> 11)`` in 64 bits; the uniform ``u`` is word ``s & 3`` of
Philox4x32-10 (``metrics.bootstrap.philox4x32_10``) with counter ``(i, s >> 2, 0, DOMAIN)`` and key
``(seed lo, seed hi)``, ``i`` the ORIGINAL loan index; the loan defaults iff ``u < thr`` (64-bit compare: ``thr =
2^32`` always defaults, ``thr = 0`` never). ``DOMAIN`` is non-zero, so the streams never coincide with the
bootstrap's (its fourth counter word is 0). ``|Q| = 2^30`` is beyond the reach of any offset: PD = 0 never
defaults and PD = 1 always does.

**Sums.** ``loss[g, s]`` is the sum of ``L_i`` over the defaulted loans of segment ``g`` in scenario ``s`` and
``defaults[g, s]`` their number, both int64: :func:`portfolio_sums_host` returns int64 ``[2, G, S]``. Limits:
``n <= 2^28`` loans, ``K <= 16`` sectors, ``G <= 64`` segments, ``S <= 2^20`` scenarios per call.
"""
from __future__ import annotations

import functools

import numpy as np

from ..metrics.bootstrap import philox4x32_10

FRAC_BITS = 20
ONE = 1 << FRAC_BITS
Q_CLAMP = 1 << 30
A_CLAMP = 1 << 29
TABLE_STEPS = 8192                       # steps of 2^-9 over [-8, 8]
TABLE_SHIFT = FRAC_BITS - 9              # X >> 11 is the table index
TABLE_MASK = (1 << TABLE_SHIFT) - 1
X_OFFSET = 8 * ONE
X_MAX = 16 * ONE
DOMAIN = 0x504C4F53                      # "PLOS": fourth counter word of the portfolio's Philox streams
MAX_LOANS = 1 << 28
MAX_SECTORS = 16
MAX_SEGMENTS = 64
MAX_SCENARIOS = 1 << 20
FIELDS = ("loss", "defaults")
_HOST_CHUNK = 1 << 22                    # draws per chunk of scenarios on the host


# ------------------------------------------------------------------------------------------ the fp64 preparation
def loss_amounts(exposure, lgd=1.0, unit: int = 100) -> np.ndarray:
    """uint32 ``[n]``: ``round(EAD_i LGD_i unit)``. ``ValueError`` for NaN, negative values and amounts at or
    above 2^32 units."""
    ead = np.asarray(exposure, dtype=np.float64).reshape(-1)
    lg = np.broadcast_to(np.asarray(lgd, dtype=np.float64), ead.shape) if np.ndim(lgd) == 0 else \
        np.asarray(lgd, dtype=np.float64).reshape(-1)
    if lg.shape != ead.shape:
        raise ValueError(f"{ead.shape[0]} exposures, {lg.shape[0]} LGDs")
    if int(unit) < 1:
        raise ValueError("unit must be a positive integer")
    amount = ead * lg * float(int(unit))
    if np.isnan(amount).any():
        raise ValueError("NaN exposure or LGD")
    if (ead < 0).any() or (lg < 0).any():
        raise ValueError("negative exposure or LGD")
    amount = np.rint(amount)
    if (amount >= 2.0 ** 32).any():
        raise ValueError("a loss amount reaches 2^32 units: use a coarser unit")
    return amount.astype(np.uint32)


def _rho_vector(rho, n_sectors: int) -> np.ndarray:
    r = np.asarray(rho, dtype=np.float64).reshape(-1)
    if r.shape[0] == 1:
        r = np.repeat(r, n_sectors)
    if r.shape[0] != n_sectors:
        raise ValueError(f"rho must be a scalar or one value per sector ({n_sectors}), got {r.shape[0]}")
    if np.isnan(r).any() or (r < 0).any() or (r >= 1).any():
        raise ValueError("rho must lie in [0, 1)")
    return r


def sector_codes(sector, n: int) -> tuple[np.ndarray, int]:
    """uint8 ``[n]`` sector ids and the number of sectors ``K`` (None: one sector)."""
    if sector is None:
        return np.zeros(n, dtype=np.uint8), 1
    s = np.asarray(sector).reshape(-1)
    if s.shape[0] != n:
        raise ValueError(f"{n} loans, {s.shape[0]} sector ids")
    if not np.issubdtype(s.dtype, np.integer):
        raise ValueError("sector ids must be integers")
    if n and (s.min() < 0 or s.max() >= MAX_SECTORS):
        raise ValueError(f"sector ids must lie in 0 .. {MAX_SECTORS - 1}")
    return s.astype(np.uint8), int(s.max()) + 1 if n else 1


def resolve_sectors(rho, sector, n: int) -> tuple[np.ndarray, np.ndarray]:
    """``rho`` as float64 ``[K]`` and the sector ids as uint8 ``[n]``: ``K`` is the length of ``rho`` when it has
    one value per sector, else the largest sector id plus one (a scalar ``rho`` serves every sector)."""
    sec, k_seen = sector_codes(sector, n)
    k = k_seen if np.size(rho) == 1 else int(np.size(rho))
    if not 1 <= k <= MAX_SECTORS:
        raise ValueError(f"1 .. {MAX_SECTORS} sectors, got {k}")
    if k_seen > k:
        raise ValueError(f"sector id {k_seen - 1} with {k} values of rho")
    return _rho_vector(rho, k), sec


def probit_points(pd, rho, sector=None) -> np.ndarray:
    """int32 ``[n]``: ``Q_i = round(Phi^-1(PD_i) / sqrt(1 - rho_k) 2^20)`` clamped to +-2^30 (PD = 0 gives -2^30,
    PD = 1 gives 2^30). ``rho``: one value per sector (or a scalar). ``ValueError`` for NaN and PDs outside
    ``[0, 1]``."""
    from scipy.special import ndtri

    p = np.asarray(pd, dtype=np.float64).reshape(-1)
    if np.isnan(p).any():
        raise ValueError("NaN PD")
    if (p < 0).any() or (p > 1).any():
        raise ValueError("PDs must lie in [0, 1]")
    r, sec = resolve_sectors(rho, sector, p.shape[0])
    q = np.rint(ndtri(p) / np.sqrt(1.0 - r[sec]) * float(ONE))
    return np.clip(q, -float(Q_CLAMP), float(Q_CLAMP)).astype(np.int32)


def scenario_offsets(rho, n_scenarios: int | None = None, seed: int = 0, *, n_sectors: int | None = None,
                     single_factor: bool = False, scenarios=None) -> np.ndarray:
    """int32 ``[S, K]``: ``A_sk = round(w_k Z_sk / sqrt(1 - w_k^2) 2^20)`` clamped to +-2^29, ``w_k =
    sqrt(rho_k)``. ``Z`` is ``scenarios`` (``[S]``: one factor shared by all sectors, or ``[S, K]``) when given,
    else ``numpy.random.default_rng(seed).standard_normal((S, K))`` (``(S, 1)`` shared by all sectors with
    ``single_factor``)."""
    k = int(n_sectors) if n_sectors is not None else int(np.size(rho))
    if not 1 <= k <= MAX_SECTORS:
        raise ValueError(f"1 .. {MAX_SECTORS} sectors, got {k}")
    r = _rho_vector(rho, k)
    if scenarios is not None:
        z = np.asarray(scenarios, dtype=np.float64)
        if z.ndim == 1:
            z = z[:, None]
        if z.ndim != 2 or z.shape[1] not in (1, k):
            raise ValueError(f"scenarios must be [S] or [S, {k}], got {z.shape}")
        if np.isnan(z).any():
            raise ValueError("NaN scenario factor")
    else:
        if n_scenarios is None or int(n_scenarios) < 1:
            raise ValueError("at least one scenario")
        z = np.random.default_rng(int(seed)).standard_normal((int(n_scenarios), 1 if single_factor else k))
    if z.shape[0] < 1:
        raise ValueError("at least one scenario")
    z = np.broadcast_to(z, (z.shape[0], k))
    a = np.rint(np.sqrt(r)[None, :] * z / np.sqrt(1.0 - r)[None, :] * float(ONE))
    return np.ascontiguousarray(np.clip(a, -float(A_CLAMP), float(A_CLAMP)).astype(np.int32))


@functools.lru_cache(maxsize=1)
def _threshold_table() -> np.ndarray:
    from scipy.special import ndtr

    x = -8.0 + np.arange(TABLE_STEPS + 1, dtype=np.float64) * 2.0 ** -9
    t = np.floor(ndtr(x) * 2.0 ** 32).astype(np.int64)
    t[0], t[TABLE_STEPS] = 0, 1 << 32
    assert (np.diff(t) >= 0).all() and t[TABLE_STEPS - 1] < 1 << 32
    t.setflags(write=False)
    return t


def threshold_table() -> np.ndarray:
    """int64 ``[8193]``: ``T[j] = floor(Phi(-8 + j 2^-9) 2^32)``, ``T[0] = 0``, ``T[8192] = 2^32`` (read-only,
    built once)."""
    return _threshold_table()


# ---------------------------------------------------------------------------------------------------- one draw
def draw_thresholds(Q, A_col, table=None) -> np.ndarray:
    """int64 thresholds in ``0 .. 2^32`` of the probit points ``Q`` against the offsets ``A_col`` (broadcast)."""
    T = threshold_table() if table is None else np.asarray(table, dtype=np.int64)
    x = np.clip(np.asarray(Q, dtype=np.int64) - np.asarray(A_col, dtype=np.int64) + X_OFFSET, 0, X_MAX)
    j, f = x >> TABLE_SHIFT, x & TABLE_MASK
    t0 = T[j]
    return t0 + (((T[np.minimum(j + 1, TABLE_STEPS)] - t0) * f) >> TABLE_SHIFT)


def draw_uniforms(idx, quad: int, seed: int) -> np.ndarray:
    """uint32 ``[n, 4]``: the uniforms of the original loans ``idx`` in scenarios ``4 quad .. 4 quad + 3``."""
    idx = np.asarray(idx, dtype=np.uint64).reshape(-1)
    seed = int(seed) & 0xffffffffffffffff
    ctr = np.zeros((idx.shape[0], 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 3] = idx, int(quad), DOMAIN
    return philox4x32_10(ctr, np.array([seed & 0xffffffff, seed >> 32], dtype=np.uint64))


# ----------------------------------------------------------------------------------------------- the sums, host
def _check_sums_inputs(idx, Q, L, sector, A, seed, segment, n_segments, rep0):
    idx = np.asarray(idx).reshape(-1)
    n = idx.shape[0]
    if n < 1:
        raise ValueError("empty portfolio")
    if n > MAX_LOANS:
        raise ValueError(f"at most 2^28 loans ({n} given)")
    if idx.min() < 0 or idx.max() >= MAX_LOANS:
        raise ValueError("original loan indices must lie in 0 .. 2^28 - 1")
    Q, L = np.asarray(Q).reshape(-1), np.asarray(L).reshape(-1)
    sector = np.zeros(n, dtype=np.uint8) if sector is None else np.asarray(sector).reshape(-1)
    if not (Q.shape[0] == L.shape[0] == sector.shape[0] == n):
        raise ValueError("idx, Q, L and sector must have one entry per loan")
    if np.abs(Q.astype(np.int64)).max() > Q_CLAMP:
        raise ValueError("Q beyond +-2^30")
    if L.astype(np.int64).min() < 0 or L.astype(np.int64).max() >= 1 << 32:
        raise ValueError("loss amounts must fit 32 bits")
    A = np.asarray(A)
    if A.ndim != 2 or A.shape[0] < 1 or not 1 <= A.shape[1] <= MAX_SECTORS:
        raise ValueError(f"A must be [S, K] with 1 <= K <= {MAX_SECTORS}, got {A.shape}")
    if A.shape[0] > MAX_SCENARIOS:
        raise ValueError(f"at most 2^20 scenarios per call ({A.shape[0]} given)")
    if np.abs(A.astype(np.int64)).max() > A_CLAMP:
        raise ValueError("A beyond +-2^29")
    if sector.astype(np.int64).min() < 0 or sector.astype(np.int64).max() >= A.shape[1]:
        raise ValueError(f"sector ids must lie in 0 .. {A.shape[1] - 1}")
    G = int(n_segments)
    if not 1 <= G <= MAX_SEGMENTS:
        raise ValueError(f"1 .. {MAX_SEGMENTS} segments, got {G}")
    segment = np.zeros(n, dtype=np.int64) if segment is None else np.asarray(segment).reshape(-1).astype(np.int64)
    if segment.shape[0] != n or segment.min() < 0 or segment.max() >= G:
        raise ValueError(f"segment codes must be one per loan, in 0 .. {G - 1}")
    rep0, seed = int(rep0), int(seed)
    if rep0 < 0 or rep0 % 4 or rep0 + A.shape[0] > 1 << 32:
        raise ValueError("rep0 must be a non-negative multiple of 4")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits")
    return (idx.astype(np.int64), Q.astype(np.int64), L.astype(np.int64), sector.astype(np.int64),
            A.astype(np.int64), seed, segment, G, rep0)


def _range_sums(idx, Q, L, sector, A, seed, rep0, bounds, table) -> np.ndarray:
    """int64 ``[2, len(bounds) - 1, S]``: the sums of the loan ranges ``bounds[r] .. bounds[r + 1]`` (positions
    in the arrays given), scenario ``rep0 + s`` for row ``s`` of ``A``."""
    n, S = idx.shape[0], A.shape[0]
    out = np.zeros((2, len(bounds) - 1, S), dtype=np.int64)
    quads = max(1, _HOST_CHUNK // (4 * n))
    lo, hi = bounds[:-1], bounds[1:]
    q0, q1 = rep0 >> 2, (rep0 + S + 3) >> 2
    for qa in range(q0, q1, quads):
        qb = min(qa + quads, q1)
        u = np.concatenate([draw_uniforms(idx, q, seed) for q in range(qa, qb)], axis=1)        # [n, 4 (qb - qa)]
        s0, s1 = max(4 * qa, rep0), min(4 * qb, rep0 + S)
        u = u[:, s0 - 4 * qa:s1 - 4 * qa].astype(np.int64)
        thr = draw_thresholds(Q[:, None], A[s0 - rep0:s1 - rep0][:, sector].T, table)
        d = u < thr
        for f, v in enumerate((d * L[:, None], d.astype(np.int64))):
            cs = np.concatenate([np.zeros((1, v.shape[1]), dtype=np.int64), np.cumsum(v, axis=0)])
            out[f, :, s0 - rep0:s1 - rep0] = cs[hi] - cs[lo]
    return out


def portfolio_sums_host(idx, Q, L, sector, A, seed: int = 0, *, segment=None, n_segments: int = 1, rep0: int = 0,
                        table=None) -> np.ndarray:
    """The direct form: int64 ``[2, G, S]`` (:data:`FIELDS`). ``idx``: original loan indices; ``Q`` / ``L`` /
    ``sector``: per loan; ``A``: int32 ``[S, K]``, row ``s`` being scenario ``rep0 + s`` (``rep0`` a multiple of
    4); ``segment``: codes in ``0 .. n_segments - 1`` or None (one segment)."""
    idx, Q, L, sector, A, seed, segment, G, rep0 = _check_sums_inputs(idx, Q, L, sector, A, seed, segment,
                                                                      n_segments, rep0)
    order = np.argsort(segment, kind="stable")
    bounds = np.searchsorted(segment[order], np.arange(G + 1))
    return _range_sums(idx[order], Q[order], L[order], sector[order], A, seed, rep0, bounds, table)


def tile_layout(segment, n_segments: int, tile_rows: int):
    """How the kernel lays the loans out: sorted by segment (stably), every segment padded to a whole number of
    tiles. Returns ``src`` (int64 ``[tiles * tile_rows]``: the position of the loan that stands there, -1 for
    padding) and ``tile_seg`` (int64 ``[G + 1]``: segment ``g`` owns tiles ``tile_seg[g] .. tile_seg[g + 1]``)."""
    segment = np.asarray(segment, dtype=np.int64).reshape(-1)
    G, tile_rows = int(n_segments), int(tile_rows)
    if tile_rows < 1:
        raise ValueError("tile_rows must be positive")
    counts = np.bincount(segment, minlength=G)
    tile_seg = np.concatenate([[0], np.cumsum((counts + tile_rows - 1) // tile_rows)]).astype(np.int64)
    order = np.argsort(segment, kind="stable")
    seg_sorted = segment[order]
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    src = np.full(int(tile_seg[-1]) * tile_rows, -1, dtype=np.int64)
    src[tile_seg[seg_sorted] * tile_rows + np.arange(segment.shape[0]) - first[seg_sorted]] = order
    return src, tile_seg


def portfolio_sums_tiled_host(idx, Q, L, sector, A, seed: int = 0, *, tile_rows: int, segment=None,
                              n_segments: int = 1, rep0: int = 0, table=None) -> np.ndarray:
    """The kernel's decomposition on the host, for any tile length: the loans in :func:`tile_layout` order with
    padding records (``Q = -2^30``, ``L = 0``: they never default), per tile the loss in 64 bits and the defaults
    in 32, then per segment the sum of its tiles in order. Same return as :func:`portfolio_sums_host`, and the
    same integers."""
    idx, Q, L, sector, A, seed, segment, G, rep0 = _check_sums_inputs(idx, Q, L, sector, A, seed, segment,
                                                                      n_segments, rep0)
    src, tile_seg = tile_layout(segment, G, tile_rows)
    pad = src < 0
    take = np.where(pad, 0, src)
    idx_t, sec_t = np.where(pad, 0, idx[take]), np.where(pad, 0, sector[take])
    Q_t, L_t = np.where(pad, -Q_CLAMP, Q[take]), np.where(pad, 0, L[take])
    tiles = int(tile_seg[-1])
    recs = _range_sums(idx_t, Q_t, L_t, sec_t, A, seed, rep0, np.arange(tiles + 1) * int(tile_rows), table)
    assert recs[1].max(initial=0) < 1 << 32
    out = np.zeros((2, G, A.shape[0]), dtype=np.int64)
    for g in range(G):
        for t in range(int(tile_seg[g]), int(tile_seg[g + 1])):
            out[:, g] += recs[:, t]
    return out
