"""The three passes of the WoE scorecard over the rows: ``csrc/scorecard.hip`` for CUDA tensors, the definitions of
``models.scorecard`` (``scorecard_encode_host``, ``scorecard_newton_host``, ``scorecard_score_host``) otherwise.
The codes, the margins, the integer scores and the reason indices are the same bits on both paths; the Newton sums
agree to the summation error. Arguments are checked before any launch (``ValueError``).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _native
from ..models import scorecard as S
from ..monitor.drift import cell_pointer, check_drift_edges

_V, _I, _I64, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
# (X, n, F, ldx, edges, cell_ptr_host, cell_ptr, codes, stream)
_native.register("cobalt_sc_encode", _I, [_V, _I64, _I, _I64, _V, _V, _V, _V, _V])
# (codes, n, F, cell_ptr_host, cell_ptr, tab, y, w, beta, workspace, workspace_bytes, out, stream)
_native.register("cobalt_sc_newton", _I, [_V, _I64, _I, _V, _V, _V, _V, _V, _V, _V, _I64, _V, _V])
_native.register("cobalt_sc_newton_workspace_bytes", _I64, [_I64, _I])
# (X, n, F, ldx, edges, cell_ptr_host, cell_ptr, beta0, contrib, ipoints, shortfall, top, margin, iscore, reasons,
#  stream)
_native.register("cobalt_sc_score", _I, [_V, _I64, _I, _I64, _V, _V, _V, _D, _V, _V, _V, _I, _V, _V, _V, _V])
for _name in ("cobalt_sc_max_features", "cobalt_sc_max_cells", "cobalt_sc_max_top", "cobalt_sc_encode_tile_rows",
              "cobalt_sc_newton_block_rows"):
    _native.register(_name, _I, [])

GPU_MAX_FEATURES = S.GPU_MAX_FEATURES
GPU_MAX_CELLS = S.GPU_MAX_CELLS


def encode_tile_rows() -> int:
    """Rows of one block of the encode kernel."""
    return int(_native.lib().cobalt_sc_encode_tile_rows())


def newton_block_rows() -> int:
    """Rows of one block of the Newton kernel (until the grid is full)."""
    return int(_native.lib().cobalt_sc_newton_block_rows())


def _check_table(ptr: np.ndarray, F: int) -> None:
    """The limits of the kernels, named: raised before any launch."""
    if F < 1 or F > GPU_MAX_FEATURES:
        raise ValueError(f"the GPU scorecard kernels take 1 .. {GPU_MAX_FEATURES} features, got {F}")
    if int(np.max(np.diff(ptr))) > S.MAX_FEATURE_CELLS:
        raise ValueError(f"at most {S.MAX_FEATURE_CELLS} cells per feature (codes are uint8)")
    if int(ptr[-1]) > GPU_MAX_CELLS:
        raise ValueError(f"the GPU scorecard kernels take at most {GPU_MAX_CELLS} cells in all, got {int(ptr[-1])}")


def _rows(X: torch.Tensor, F_expected: int | None = None):
    if X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError(f"X must be float32 [rows, features], got {X.dtype} {tuple(X.shape)}")
    N, F = X.shape
    if F_expected is not None and F != F_expected:
        raise ValueError(f"{F} columns need {F} edge vectors, got {F_expected}")
    if F > 1 and X.stride(1) != 1:
        raise ValueError(f"X must have unit column stride, got stride {X.stride(1)}")
    ldx = X.stride(0) if N > 1 else F
    if ldx < F:
        raise ValueError(f"rows of X overlap (row stride {ldx} < {F} columns)")
    return N, F, ldx


def _edge_tables(edges_list, dev):
    edges = [check_drift_edges(z) for z in edges_list]
    ptr = cell_pointer(edges)
    _check_table(ptr, len(edges))
    ptr32 = ptr.astype(np.int32)
    flat = np.concatenate(edges) if int(ptr[-1]) > 2 * len(edges) else np.zeros(0, np.float32)
    ed = torch.from_numpy(flat).to(dev) if flat.size else None
    return ptr32, ed, torch.from_numpy(ptr32).to(dev)


def scorecard_encode(X, edges_list):
    """uint8 ``[N, F]`` codes of ``X`` among the coarse edges (``models.scorecard.scorecard_encode_host``): a CUDA
    tensor (float32, unit column stride, rows may be strided) is encoded on its device and a CUDA tensor comes
    back; anything else goes through the host definition and a NumPy array comes back."""
    if not (isinstance(X, torch.Tensor) and X.device.type == "cuda"):
        return S.scorecard_encode_host(X.detach().numpy() if isinstance(X, torch.Tensor) else X, edges_list)
    N, F, ldx = _rows(X, len(edges_list))
    ptr32, ed, pd = _edge_tables(edges_list, X.device)
    codes = torch.empty((N, F), dtype=torch.uint8, device=X.device)
    with torch.cuda.device(X.device):
        rc = _native.lib().cobalt_sc_encode(X.data_ptr(), N, F, ldx, _native.ptr(ed), ptr32.ctypes.data, pd.data_ptr(),
                                            codes.data_ptr(), _native.stream_handle())
    _native.check(rc, "cobalt_sc_encode")
    return codes


class _DeviceNewton:
    """The device buffers of the passes of one fit (codes, tables, labels, weights, workspace): a pass uploads
    beta, launches, and reads ``1 + P + P P`` doubles back."""

    def __init__(self, codes: torch.Tensor, cell_ptr, tab, y, w):
        if codes.dim() != 2 or codes.dtype != torch.uint8:
            raise ValueError(f"codes must be uint8 [rows, features], got {codes.dtype} {tuple(codes.shape)}")
        N, F = codes.shape
        ptr = np.asarray(cell_ptr, dtype=np.int64).reshape(-1)
        if ptr.shape[0] != F + 1 or ptr[0] != 0 or bool((np.diff(ptr) < 2).any()):
            raise ValueError(f"cell_ptr must hold {F + 1} ascending entries from 0, at least 2 cells per feature")
        _check_table(ptr, F)
        tab = np.ascontiguousarray(tab, dtype=np.float64).reshape(-1)
        if tab.shape[0] != int(ptr[-1]) or not bool(np.isfinite(tab).all()):
            raise ValueError(f"tab must hold {int(ptr[-1])} finite values")
        dev = codes.device
        self.dev, self.N, self.F = dev, N, F
        self.codes = codes.contiguous()
        if self.codes.data_ptr() % 4:
            self.codes = self.codes.clone()
        self.ptr32 = ptr.astype(np.int32)
        self.ptr_d = torch.from_numpy(self.ptr32).to(dev)
        self.tab_d = torch.from_numpy(tab).to(dev)
        yt = y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y, dtype=np.float32))
        self.y = yt.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        self.w = None
        if w is not None:
            wt = w if isinstance(w, torch.Tensor) else torch.as_tensor(np.asarray(w, dtype=np.float64))
            self.w = wt.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
        if self.y.shape[0] != N or (self.w is not None and self.w.shape[0] != N):
            raise ValueError(f"{N} rows need {N} labels and weights")
        need = int(_native.lib().cobalt_sc_newton_workspace_bytes(N, F))
        _native.check(min(need, 0), "cobalt_sc_newton_workspace_bytes")
        self.work = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=dev)
        self.need = need

    def launch(self, beta) -> torch.Tensor:
        """float64 ``[1 + P + P P]`` on the device: loss, grad, hess (on the current stream)."""
        P = self.F + 1
        b = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
        if b.shape[0] != P or not bool(np.isfinite(b).all()):
            raise ValueError(f"beta must hold {P} finite values")
        out = torch.zeros(1 + P + P * P, dtype=torch.float64, device=self.dev)
        bd = torch.from_numpy(b).to(self.dev)
        with torch.cuda.device(self.dev):
            rc = _native.lib().cobalt_sc_newton(self.codes.data_ptr(), self.N, self.F, self.ptr32.ctypes.data,
                                                self.ptr_d.data_ptr(), self.tab_d.data_ptr(), self.y.data_ptr(),
                                                _native.ptr(self.w), bd.data_ptr(), self.work.data_ptr(), self.need,
                                                out.data_ptr(), _native.stream_handle())
        _native.check(rc, "cobalt_sc_newton")
        return out

    def __call__(self, beta):
        P = self.F + 1
        o = self.launch(beta).cpu().numpy()
        return float(o[0]), o[1:1 + P].copy(), o[1 + P:].reshape(P, P).copy()


def newton_pass(codes, cell_ptr, tab, y, w):
    """``beta -> (loss, grad, hess)`` as NumPy float64 for these rows: the kernel when ``codes`` is a CUDA tensor
    (the buffers are set up once), ``models.scorecard.scorecard_newton_host`` otherwise."""
    if isinstance(codes, torch.Tensor) and codes.device.type == "cuda":
        return _DeviceNewton(codes, cell_ptr, tab, y, w)
    ch = codes.numpy() if isinstance(codes, torch.Tensor) else np.asarray(codes)
    yh = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y
    wh = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w
    return lambda beta: S.scorecard_newton_host(ch, cell_ptr, tab, yh, wh, beta)


def scorecard_newton(codes, cell_ptr, tab, y, w, beta):
    """One Newton pass, ``(loss, grad [F + 1], hess [F + 1, F + 1])`` as NumPy float64
    (``models.scorecard.scorecard_newton_host`` is the definition): on the device of ``codes`` when it is a CUDA
    tensor, where the same input gives the same bits on every call."""
    return newton_pass(codes, cell_ptr, tab, y, w)(beta)


def scorecard_score(X, edges_list, beta0: float, contrib, ipoints, shortfall, top: int = 0):
    """``(margin float64 [N], integer score int32 [N], reasons int32 [N, top])``
    (``models.scorecard.scorecard_score_host`` is the definition): CUDA tensors for a CUDA ``X``, NumPy arrays
    otherwise; the same bits either way."""
    if not 0 <= int(top) <= S.MAX_TOP:
        raise ValueError(f"top must lie in 0 .. {S.MAX_TOP}, got {top}")
    top = int(top)
    if not (isinstance(X, torch.Tensor) and X.device.type == "cuda"):
        return S.scorecard_score_host(X.detach().numpy() if isinstance(X, torch.Tensor) else X, edges_list, beta0,
                                      contrib, ipoints, shortfall, top)
    N, F, ldx = _rows(X, len(edges_list))
    dev = X.device
    ptr32, ed, pd = _edge_tables(edges_list, dev)
    cells = int(ptr32[-1])
    c = np.ascontiguousarray(contrib, dtype=np.float64).reshape(-1)
    ip = np.ascontiguousarray(ipoints, dtype=np.int32).reshape(-1)
    sf = np.ascontiguousarray(shortfall, dtype=np.float64).reshape(-1)
    if c.shape[0] != cells or ip.shape[0] != cells or sf.shape[0] != cells:
        raise ValueError(f"contrib, ipoints and shortfall must hold {cells} cells each")
    if not math_isfinite(beta0):
        raise ValueError("beta0 must be finite")
    cd, ipd, sfd = (torch.from_numpy(a).to(dev) for a in (c, ip, sf))
    margin = torch.empty(N, dtype=torch.float64, device=dev)
    iscore = torch.empty(N, dtype=torch.int32, device=dev)
    reasons = torch.empty((N, top), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _native.lib().cobalt_sc_score(X.data_ptr(), N, F, ldx, _native.ptr(ed), ptr32.ctypes.data, pd.data_ptr(),
                                           float(beta0), cd.data_ptr(), ipd.data_ptr(), sfd.data_ptr(), top,
                                           margin.data_ptr(), iscore.data_ptr(),
                                           reasons.data_ptr() if top and N else None, _native.stream_handle())
    _native.check(rc, "cobalt_sc_score")
    return margin, iscore, reasons


def math_isfinite(v) -> bool:
    return bool(np.isfinite(float(v)))
