"""The portfolio loss sums on the GPU: ``csrc/portfolio.hip`` (per scenario and segment the summed loss and the
number of defaults under the Gaussian-copula factor model). The definition and the CPU path are
``portfolio.loss.portfolio_sums_host``; the integers are the same.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _native
from ..portfolio import loss as P

_V, _I, _I64, _U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
# (loans, n, A, K, sector_max, table, tile_seg (host), G, rep0, scenarios, seed, workspace, workspace_bytes, out,
#  ld, stream)
_native.register("cobalt_portfolio", _I, [_V, _I64, _V, _I, _I, _V, _V, _I, _I64, _I, _U64, _V, _I64, _V, _I64, _V])
_native.register("cobalt_portfolio_workspace_bytes", _I64, [_I64, _I])
_native.register("cobalt_portfolio_tile_rows", _I, [])
_native.register("cobalt_portfolio_block_scenarios", _I, [])
_native.register("cobalt_portfolio_max_rows", _I64, [])

WORKSPACE_TARGET = 1 << 30   # bytes: scenarios are split into calls whose tile records stay under it


def portfolio_tile_rows() -> int:
    return int(_native.lib().cobalt_portfolio_tile_rows())


def portfolio_block_scenarios() -> int:
    return int(_native.lib().cobalt_portfolio_block_scenarios())


def portfolio_workspace_bytes(n: int, scenarios: int) -> int:
    """Bytes of scratch one call needs, or the kernel's negative refusal for these shapes."""
    return int(_native.lib().cobalt_portfolio_workspace_bytes(int(n), int(scenarios)))


def _vector(name: str, t, dtype, n: int | None, dev) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"portfolio_sums_gpu takes CUDA tensors ({name} is not one)")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name} is on {t.device}, the loans on {dev}")
    if t.dim() != 1 or t.dtype != dtype or (n is not None and t.shape[0] != n):
        raise ValueError(f"{name} must be a {dtype} vector" + (f" of {n}" if n is not None else "")
                         + f", got {t.dtype} {tuple(t.shape)}")
    return t


def pack_loans(idx: torch.Tensor, Q: torch.Tensor, L: torch.Tensor, sector: torch.Tensor, segment: torch.Tensor,
               n_segments: int, tile_rows: int):
    """The kernel's records (int32 ``[rows, 4]``: original index, Q, the bits of L, sector) in
    ``portfolio.loss.tile_layout`` order: sorted by segment, every segment padded to whole tiles with records
    that never default (``Q = -2^30``, ``L = 0``). Also the host table ``tile_seg`` (int32 ``[G + 1]``)."""
    n, dev = idx.shape[0], idx.device
    counts = torch.bincount(segment, minlength=n_segments)
    tiles_of = (counts + tile_rows - 1) // tile_rows
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    tile_first = torch.cat([zero, torch.cumsum(tiles_of, 0)])
    first = torch.cat([zero, torch.cumsum(counts, 0)])
    seg_sorted, order = torch.sort(segment, stable=True)
    dest = tile_first[seg_sorted] * tile_rows + torch.arange(n, device=dev) - first[seg_sorted]
    tile_seg = tile_first.cpu()
    rows = int(tile_seg[-1]) * tile_rows
    recs = torch.zeros((rows, 4), dtype=torch.int32, device=dev)
    recs[:, 1] = -P.Q_CLAMP
    bits = torch.where(L >= 1 << 31, L - (1 << 32), L).to(torch.int32)
    recs[dest] = torch.stack([idx.to(torch.int32), Q, bits, sector.to(torch.int32)], dim=1)[order]
    return recs, tile_seg.to(torch.int32).contiguous()


def portfolio_sums_gpu(idx: torch.Tensor, Q: torch.Tensor, L: torch.Tensor, sector: torch.Tensor | None,
                       A: torch.Tensor, seed: int = 0, *, segment: torch.Tensor | None = None, n_segments: int = 1,
                       rep0: int = 0, table: torch.Tensor | None = None) -> torch.Tensor:
    """int64 ``[2, G, S]`` (``portfolio.loss.FIELDS``) on the device of the inputs, on the current stream.

    ``idx`` (int64, original loan indices), ``Q`` (int32), ``L`` (int64, ``0 .. 2^32 - 1``), ``sector`` (int64 or
    None) and ``segment`` (int64 codes in ``0 .. n_segments - 1`` or None) have one entry per loan; ``A`` is int32
    ``[S, K]``, row ``s`` being scenario ``rep0 + s`` (``rep0`` a multiple of 4); ``table`` is int64 ``[8193]``
    (``portfolio.loss.threshold_table``, uploaded when None). Scenarios are split into calls that keep the
    scratch near 1 GiB. ``ValueError`` / ``RuntimeError`` before any launch (the range checks cost one
    synchronisation)."""
    idx = _vector("idx", idx, torch.int64, None, None)
    n, dev = int(idx.shape[0]), idx.device
    Q = _vector("Q", Q, torch.int32, n, dev)
    L = _vector("L", L, torch.int64, n, dev)
    if n < 1 or n > P.MAX_LOANS:
        raise ValueError(f"1 .. 2^28 loans, got {n}")
    if not isinstance(A, torch.Tensor) or A.device != dev or A.dim() != 2 or A.dtype != torch.int32:
        raise ValueError(f"A must be an int32 [S, K] tensor on {dev}")
    S, K = int(A.shape[0]), int(A.shape[1])
    if not 1 <= K <= P.MAX_SECTORS:
        raise ValueError(f"1 .. {P.MAX_SECTORS} sectors, got {K}")
    if S < 1:
        raise ValueError("at least one scenario")
    G, rep0, seed = int(n_segments), int(rep0), int(seed)
    if not 1 <= G <= P.MAX_SEGMENTS:
        raise ValueError(f"1 .. {P.MAX_SEGMENTS} segments, got {G}")
    if rep0 < 0 or rep0 % 4 or rep0 + S > 1 << 32:
        raise ValueError("rep0 must be a non-negative multiple of 4")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits")
    sector = torch.zeros(n, dtype=torch.int64, device=dev) if sector is None else \
        _vector("sector", sector, torch.int64, n, dev)
    segment = torch.zeros(n, dtype=torch.int64, device=dev) if segment is None else \
        _vector("segment", segment, torch.int64, n, dev)
    if table is None:
        table = torch.from_numpy(np.array(P.threshold_table())).to(dev)
    if table.device != dev or table.dtype != torch.int64 or tuple(table.shape) != (P.TABLE_STEPS + 1,):
        raise ValueError(f"table must be int64 [{P.TABLE_STEPS + 1}] on {dev}")
    A, table = A.contiguous(), table.contiguous()
    with torch.cuda.device(dev):
        lim = torch.stack([idx.min(), idx.max(), Q.to(torch.int64).abs().max(), L.min(), L.max(), sector.min(),
                           sector.max(), segment.min(), segment.max(), A.to(torch.int64).abs().max()]).cpu().tolist()
        if lim[0] < 0 or lim[1] >= P.MAX_LOANS:
            raise ValueError("original loan indices must lie in 0 .. 2^28 - 1")
        if lim[2] > P.Q_CLAMP:
            raise ValueError("Q beyond +-2^30")
        if lim[3] < 0 or lim[4] >= 1 << 32:
            raise ValueError("loss amounts must fit 32 bits")
        if lim[5] < 0 or lim[6] >= K:
            raise ValueError(f"sector ids must lie in 0 .. {K - 1}")
        if lim[7] < 0 or lim[8] >= G:
            raise ValueError(f"segment codes must lie in 0 .. {G - 1}")
        if lim[9] > P.A_CLAMP:
            raise ValueError("A beyond +-2^29")
        recs, tile_seg = pack_loans(idx, Q, L, sector, segment, G, portfolio_tile_rows())
        rows = int(recs.shape[0])
        if rows > P.MAX_LOANS:
            raise ValueError(f"{rows} records after padding the segments to whole tiles: at most 2^28")
        out = torch.zeros((2, G, S), dtype=torch.int64, device=dev)
        per4 = portfolio_workspace_bytes(rows, 4)
        _native.check(min(per4, 0), "cobalt_portfolio_workspace_bytes")
        step = min(S, P.MAX_SCENARIOS, max(4, WORKSPACE_TARGET // per4 * 4))
        need = portfolio_workspace_bytes(rows, step)
        _native.check(min(need, 0), "cobalt_portfolio_workspace_bytes")
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        for b0 in range(0, S, step):
            rc = _native.lib().cobalt_portfolio(recs.data_ptr(), rows, A[b0:].data_ptr(), K, int(lim[6]),
                                                table.data_ptr(), tile_seg.data_ptr(), G, rep0 + b0,
                                                min(step, S - b0), seed, work.data_ptr(), need,
                                                out[:, :, b0:].data_ptr(), S, _native.stream_handle())
            _native.check(rc, "cobalt_portfolio")
    return out
