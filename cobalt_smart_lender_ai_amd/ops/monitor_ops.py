"""The count table under the drift reports on the GPU: ``csrc/bincount.hip`` (exact per-feature, per-bin,
per-class weighted counts of a device-resident ``[N, F]`` matrix in one pass). The definition and the CPU path
are ``monitor.drift.bin_counts_host``; the integers are the same.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _native
from ..monitor.drift import cell_pointer, check_drift_edges

_V, _I, _I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
# (X, n, F, ldx, edges, cell_ptr_host, cell_ptr, y, wq, counts, stream)
_native.register("cobalt_bin_counts", _I, [_V, _I64, _I, _I64, _V, _V, _V, _V, _V, _V, _V])
_native.register("cobalt_bin_counts_groups", _I, [_V, _I, _I, _V])
_native.register("cobalt_bin_counts_tile_rows", _I, [])
_native.register("cobalt_bin_counts_max_edges", _I, [])
_native.register("cobalt_bin_counts_max_blocks", _I, [])

BIN_MAX_EDGES = 4096      # per feature (csrc/bincount.hip kBinMaxEdges)
BIN_MAX_WEIGHT = 1 << 20  # models.sketch.WEIGHT_SCALE: what a 32-bit LDS counter is sized for


def _cell_ptr32(edges_list) -> np.ndarray:
    """``cell_pointer`` as the int32 vector the kernel reads; ``ValueError`` when the table has 2^31 cells or more."""
    ptr = cell_pointer(edges_list)
    if int(ptr[-1]) >= 1 << 31:
        raise ValueError(f"{int(ptr[-1])} cells do not fit the kernel's int32 cell index")
    return ptr.astype(np.int32)


def bin_counts_plan(edges_list, classes: int) -> list[int]:
    """The kernel's feature groups for these edges and ``classes`` (1 or 2) count rows: the first feature of
    every group, then F. One group is one ``blockIdx.y``: its edges and counters share the LDS."""
    ptr = _cell_ptr32(edges_list)
    first = np.zeros(len(edges_list) + 1, dtype=np.int32)
    g = int(_native.lib().cobalt_bin_counts_groups(ptr.ctypes.data, len(edges_list), int(classes), first.ctypes.data))
    _native.check(min(g, 0), "cobalt_bin_counts_groups")
    return [int(v) for v in first[:g + 1]]


def bin_counts_gpu(X: torch.Tensor, edges_list, y: torch.Tensor | None = None, wq: torch.Tensor | None = None,
                   out: torch.Tensor | None = None, *, wq_in_range: bool = False) -> torch.Tensor:
    """int64 ``[C, cells]`` on the device of ``X``: the count table of ``monitor.drift.bin_counts_host``, on the
    current stream. ``X``: float32 [N, F] with unit column stride; rows may be strided (a column slice of a
    wider matrix is read in place). ``y``: [N] labels (class ``y > 0.5``) or None (``C = 1``); ``wq``: [N]
    integer weights in ``[0, 2^20]`` or None; the range is checked here (one reduction and one synchronisation)
    unless the caller vouches for it with ``wq_in_range`` (``monitor.drift`` quantises them itself and does,
    so a stream of chunks never waits for the device). ``out`` is added to (a chunked caller passes it again); without it
    a zeroed table is made. Edges are checked on the host (:func:`~..monitor.drift.check_drift_edges`);
    ``ValueError`` / ``RuntimeError`` before any launch."""
    if not isinstance(X, torch.Tensor) or X.device.type != "cuda":
        raise ValueError("bin_counts_gpu takes a CUDA tensor")
    if X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError(f"X must be float32 [rows, features], got {X.dtype} {tuple(X.shape)}")
    N, F = X.shape
    if F < 1 or len(edges_list) != F:
        raise ValueError(f"{F} columns need {F} edge vectors, got {len(edges_list)}")
    if F > 1 and X.stride(1) != 1:
        raise ValueError(f"X must have unit column stride, got stride {X.stride(1)}")
    ldx = X.stride(0) if N > 1 else F
    if ldx < F:
        raise ValueError(f"rows of X overlap (row stride {ldx} < {F} columns)")
    edges = [check_drift_edges(z) for z in edges_list]
    if any(len(z) > BIN_MAX_EDGES for z in edges):
        raise ValueError(f"at most {BIN_MAX_EDGES} edges per feature")
    dev = X.device
    C = 1 if y is None else 2
    ptr = _cell_ptr32(edges)
    cells = int(ptr[-1])
    if y is not None:
        y = y.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if y.shape[0] != N:
            raise ValueError(f"X has {N} rows, y has {y.shape[0]}")
    if wq is not None:
        wq = wq.to(device=dev).reshape(-1)
        if wq.shape[0] != N or wq.dtype.is_floating_point:
            raise ValueError(f"wq must be {N} integers")
        if N and not wq_in_range:
            lo, hi = (int(v) for v in torch.stack(torch.aminmax(wq)).cpu())
            if lo < 0 or hi > BIN_MAX_WEIGHT:
                raise ValueError(f"integer weights must lie in [0, {BIN_MAX_WEIGHT}]")
        wq = wq.to(torch.int32).contiguous()
    if out is None:
        out = torch.zeros((C, cells), dtype=torch.int64, device=dev)
    elif out.shape != (C, cells) or out.dtype != torch.int64 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int64 [{C}, {cells}] tensor on {dev}")
    flat = np.concatenate(edges) if cells > 2 * F else np.zeros(0, np.float32)
    ed = torch.from_numpy(flat).to(dev) if flat.size else None
    pd = torch.from_numpy(ptr).to(dev)
    rc = _native.lib().cobalt_bin_counts(X.data_ptr(), N, F, ldx, _native.ptr(ed), ptr.ctypes.data, pd.data_ptr(),
                                         _native.ptr(y), _native.ptr(wq), out.data_ptr(), _native.stream_handle())
    _native.check(rc, "cobalt_bin_counts")
    return out
