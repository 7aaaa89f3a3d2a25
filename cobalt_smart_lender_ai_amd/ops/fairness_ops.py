"""The fair-lending sums on the GPU: ``csrc/fairness.hip`` (per bootstrap replicate, protected group and cutoff
the exact integers ``n B S1 S2 D_k DB_k``). The definition and the CPU path are
``fairness.sums.fairness_sums_host``; the integers are the same.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _native
from ..fairness import sums as F

_V, _I, _I64, _U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
# (rows, n, K, tile_group (host), G, rep0, reps, seed, flags, workspace, workspace_bytes, out, ld, stream)
_native.register("cobalt_fairness", _I, [_V, _I64, _I, _V, _I, _I64, _I, _U64, _I, _V, _I64, _V, _I64, _V])
_native.register("cobalt_fairness_workspace_bytes", _I64, [_I64, _I, _I])
_native.register("cobalt_fairness_tile_rows", _I, [])
_native.register("cobalt_fairness_block_reps", _I, [])
_native.register("cobalt_fairness_max_rows", _I64, [])

FLAG_LABELS, FLAG_UNIT = 1, 2
WORKSPACE_TARGET = 1 << 30   # bytes: replicates are split into calls whose tile records stay under it


def fairness_tile_rows() -> int:
    return int(_native.lib().cobalt_fairness_tile_rows())


def fairness_block_reps() -> int:
    return int(_native.lib().cobalt_fairness_block_reps())


def fairness_workspace_bytes(n: int, reps: int, K: int) -> int:
    """Bytes of scratch one call needs, or the kernel's negative refusal for these shapes."""
    return int(_native.lib().cobalt_fairness_workspace_bytes(int(n), int(reps), int(K)))


def _vector(name: str, t, n: int | None, dev) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"fairness_sums_gpu takes CUDA tensors ({name} is not one)")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name} is on {t.device}, the scores on {dev}")
    if t.dim() != 1 or (n is not None and t.shape[0] != n):
        raise ValueError(f"{name} must be a vector" + (f" of {n}" if n is not None else "")
                         + f", got {tuple(t.shape)}")
    return t


def pack_rows(rows: torch.Tensor, score: torch.Tensor, y: torch.Tensor | None, cutoffs: torch.Tensor,
              group: torch.Tensor, n_groups: int, tile_rows: int):
    """The kernel's records (int32 ``[rows, 2]``: the word of original index and label bit; the decline mask in
    the low and ``q`` in the high 16 bits) in ``portfolio.loss.tile_layout`` order: sorted by group (stably), every
    group padded to whole tiles with records that carry the padding bit. Also the host table ``tile_group``
    (int32 ``[G + 1]``). ``score`` is float32, ``cutoffs`` float32 ``[K]`` on the same device; the rest int64."""
    n, dev = score.shape[0], score.device
    K = int(cutoffs.shape[0])
    q = torch.floor(score * float(F.Q_SCALE)).clamp(max=float(F.Q_MAX)).to(torch.int64)
    mask = ((score[:, None] > cutoffs[None, :]).to(torch.int64) << torch.arange(K, device=dev)[None, :]).sum(dim=1)
    word = rows if y is None else rows | (y << F.IDX_BITS)
    hi = mask | (q << 16)
    hi = torch.where(hi >= 1 << 31, hi - (1 << 32), hi)
    counts = torch.bincount(group, minlength=n_groups)
    tiles_of = (counts + tile_rows - 1) // tile_rows
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    tile_first = torch.cat([zero, torch.cumsum(tiles_of, 0)])
    first = torch.cat([zero, torch.cumsum(counts, 0)])
    g_sorted, order = torch.sort(group, stable=True)
    dest = tile_first[g_sorted] * tile_rows + torch.arange(n, device=dev) - first[g_sorted]
    tile_group = tile_first.cpu()
    total = int(tile_group[-1]) * tile_rows
    recs = torch.zeros((total, 2), dtype=torch.int32, device=dev)
    recs[:, 0] = F.PAD_BIT
    recs[dest] = torch.stack([word, hi], dim=1)[order].to(torch.int32)
    return recs, tile_group.to(torch.int32).contiguous()


def fairness_sums_gpu(score: torch.Tensor, group: torch.Tensor, y: torch.Tensor | None, cutoffs, reps: int,
                      seed: int = 0, rep0: int = 0, *, n_groups: int | None = None, rows: torch.Tensor | None = None,
                      unit: bool = False) -> torch.Tensor:
    """int64 ``[4 + 2 K, G, reps]`` (``fairness.sums.field_names``) on the device of the inputs, on the current
    stream: replicates ``rep0 .. rep0 + reps - 1`` (``rep0`` a multiple of 4). ``score`` (floating point, PDs in
    ``[0, 1]``), ``group`` (integer codes ``0 .. G - 1``), ``y`` (0/1 or None) and ``rows`` (the original row
    indices, ``0 .. n - 1`` when None) are CUDA vectors with one entry per row; ``cutoffs`` is a host sequence of
    ``K`` values. The records are packed on the device; replicates are split into calls that keep the scratch
    near 1 GiB. ``ValueError`` / ``RuntimeError`` before any launch of the kernel (the range checks cost one
    synchronisation)."""
    score = _vector("score", score, None, None)
    n, dev = int(score.shape[0]), score.device
    if not score.dtype.is_floating_point:
        raise ValueError(f"score must be floating point, got {score.dtype}")
    group = _vector("group", group, n, dev)
    if group.dtype.is_floating_point or group.dtype == torch.bool:
        raise ValueError("group codes must be integers")
    if y is not None:
        y = _vector("y", y, n, dev)
    if rows is not None:
        rows = _vector("rows", rows, n, dev)
    if n < 1 or n > F.MAX_ROWS:
        raise ValueError(f"1 .. 2^27 rows, got {n}")
    cut = F.check_cutoffs(cutoffs)
    K = int(cut.shape[0])
    reps, rep0, seed = int(reps), int(rep0), int(seed)
    if reps < 1:
        raise ValueError("at least one replicate")
    if rep0 < 0 or rep0 % 4 or rep0 + reps > 1 << 32:
        raise ValueError("rep0 must be a non-negative multiple of 4")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits")
    with torch.cuda.device(dev):
        s = score.to(torch.float32)
        g = group.to(torch.int64)
        yy = None if y is None else y.to(torch.int64)
        idx = torch.arange(n, device=dev) if rows is None else rows.to(torch.int64)
        bad_y = torch.zeros((), dtype=torch.bool, device=dev) if y is None else ((y != 0) & (y != 1)).any()
        lim = torch.stack([torch.isnan(s).any().to(torch.int64), (s < 0).any().to(torch.int64),
                           (s > 1).any().to(torch.int64), bad_y.to(torch.int64), g.min(), g.max(), idx.min(),
                           idx.max()]).cpu().tolist()
        if lim[0]:
            raise ValueError("NaN scores")
        if lim[1] or lim[2]:
            raise ValueError("scores must lie in [0, 1]")
        if lim[3]:
            raise ValueError("labels must be 0 or 1")
        G = int(lim[5]) + 1 if n_groups is None else int(n_groups)
        if not 1 <= G <= F.MAX_GROUPS:
            raise ValueError(f"1 .. {F.MAX_GROUPS} groups, got {G}")
        if lim[4] < 0 or lim[5] >= G:
            raise ValueError(f"group codes must lie in 0 .. {G - 1}")
        if lim[6] < 0 or lim[7] >= 1 << F.IDX_BITS:
            raise ValueError("original row indices must lie in 0 .. 2^28 - 1")
        recs, tile_group = pack_rows(idx, s, yy, torch.from_numpy(cut).to(dev), g, G, fairness_tile_rows())
        total = int(recs.shape[0])
        if total > F.MAX_ROWS:
            raise ValueError(f"{total} records after padding the groups to whole tiles: at most 2^27")
        flags = (FLAG_LABELS if y is not None else 0) | (FLAG_UNIT if unit else 0)
        out = torch.zeros((len(F.FIXED_FIELDS) + 2 * K, G, reps), dtype=torch.int64, device=dev)
        per4 = fairness_workspace_bytes(total, 4, K)
        _native.check(min(per4, 0), "cobalt_fairness_workspace_bytes")
        step = min(reps, F.MAX_REPS, max(4, WORKSPACE_TARGET // per4 * 4))
        need = fairness_workspace_bytes(total, step, K)
        _native.check(min(need, 0), "cobalt_fairness_workspace_bytes")
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        for b0 in range(0, reps, step):
            rc = _native.lib().cobalt_fairness(recs.data_ptr(), total, K, tile_group.data_ptr(), G, rep0 + b0,
                                               min(step, reps - b0), seed, flags, work.data_ptr(), need,
                                               out[:, :, b0:].data_ptr(), reps, _native.stream_handle())
            _native.check(rc, "cobalt_fairness")
    return out
