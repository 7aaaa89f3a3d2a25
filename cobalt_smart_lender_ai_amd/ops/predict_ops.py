"""Inference entry points: margins, probabilities, TreeSHAP and per-tree learning curves for a
:class:`Booster`.

GPU path: gfx950 kernels in ``csrc/predict.hip`` (forest packed once per booster and device, cached),
``csrc/shapint.hip``, ``csrc/shapbg.hip``, ``csrc/evalcurve.hip``, ``csrc/pdp.hip``, ``csrc/permimp.hip``,
``csrc/ale.hip``, ``csrc/recourse.hip`` and ``csrc/refresh.hip`` (leaf indices, leaf refresh).
CPU path: the NumPy reference implementations in ``models/booster.py``.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np
import torch

from .. import _native
from ..models.booster import (Booster, Tree, _refreshed_booster, ale_host, check_ale_edges, check_background,
                              check_eval_inputs,
                              check_model_output, check_perm_inputs, check_recourse_args, check_refresh_inputs,
                              eval_curve_host, partial_dependence_host, permutation_scores_host, predict_leaf_host,
                              predict_margin_host, recourse_scan_host, refresh_host, refresh_params,
                              refresh_row_weights,
                              refreshed_tree, sigmoid32, staged_margins_host, treeshap_host,
                              treeshap_interactions_host, treeshap_interventional_host)
from ..models.gbdt_host import quant_scales
from ..config import knob

# LDS tile capacity in nodes: a model's tile is max(this, its largest tree), at most MAX_TILE_NODES
# (csrc/predict.hip kMaxTileNodes). 2048 measured best on MI355X (125M-row scoring, 300 depth-7
# trees: 1024 -> 793M, 2048 -> 810M, 3072 -> 683M, 6144 -> 490M, 8192 -> 261M rows/s) -- smaller
# tiles mean more resident blocks per CU. COBALT_PRED_TILE overrides it for sweeps.
TILE_NODES = int(knob("COBALT_PRED_TILE", "2048"))
MAX_TILE_NODES = 8192
MAX_PATH = 15

_native.register("cobalt_predict", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p])
_native.register("cobalt_treeshap", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                  ctypes.c_void_p])
_native.register("cobalt_treeshap_chunks", ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int])
_native.register("cobalt_predict_small_rows", ctypes.c_int64, [])
_native.register("cobalt_predict_small", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
_SMALL_ROWS = 131072
_native.register("cobalt_shap_table_build", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p])
_native.register("cobalt_treeshap_tab", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_int, ctypes.c_void_p])
SHAP_ROWS_MIN = 256  # batches from this size use the row-parallel table kernel
SHAP_ROWS_MAX_F = 48
SHAP_TABLE_MAX_K = 10             # longest path (unique features) that gets a pattern table
SHAP_TABLE_MAX_BYTES = 2 << 30    # per-model table budget on the device

_native.register("cobalt_treeshap_interactions", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
_native.register("cobalt_treeshap_interactions_max_f", ctypes.c_int, [])
_native.register("cobalt_treeshap_interactions_lds", ctypes.c_int64, [ctypes.c_int, ctypes.c_int])
SHAP_INT_MAX_F = 48            # widest model of the interaction kernel (csrc/shapint.hip kShapIntMaxF)
# Rows per launch of the interaction values: bounds the scratch of the SHAP values they start from
# (phi [rows, F] plus treeshap_gpu's [rows, chunks, F] slab: 16384 x 117 x 20 doubles = 307 MB for the
# shipped model); the interaction kernel itself keeps its accumulators in LDS and has no global scratch.
SHAP_INT_ROWS = 16384

# csrc/shapbg.hip: masks (X, n, F, ldx, elems, path_ptr, path_val, n_paths, max_len, base_margin, masks, margins,
# stream); values (X, n, F, ldx, elems, path_ptr, path_val, n_paths, max_len, zmask, zmargin, nb, xmargin, first,
# last, n_background, phi, stream)
_native.register("cobalt_shapbg_masks", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p])
_native.register("cobalt_treeshap_interventional", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p])
_native.register("cobalt_shapbg_max_f", ctypes.c_int, [])
_native.register("cobalt_shapbg_max_tile", ctypes.c_int, [])
SHAP_BG_MAX_F = 256            # widest X of the interventional kernel (csrc/shapbg.hip kBgMaxF)
SHAP_BG_MAX_TILE = 1024        # background rows per launch (csrc/shapbg.hip kBgMaxTile)
SHAP_BG_MASK_BYTES = 64 << 20  # mask workspace: the background tile is this many bytes of [tile, n_paths] uint16
SHAP_BG_ROWS = 16384           # rows of X per launch (bounds the margins of probability mode)

# csrc/evalcurve.hip: (X, n, F, ldx, y, w, nodes, tree_ptr, tile_ptr, n_tiles, tile_cap, n_trees, base_margin,
# margin_in, margin_out, stage_margins, workspace, sums, stream)
_native.register("cobalt_eval_curve", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                  ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p])
_native.register("cobalt_eval_curve_workspace", ctypes.c_int64, [ctypes.c_int64, ctypes.c_int])

# csrc/pdp.hip: (X, n, F, ldx, nodes, tree_ptr, tile_ptr, n_tiles, tile_cap, base_margin, f1, f2, g1, G1, g2, G2,
# w, ice, workspace, sums, stream)
_native.register("cobalt_pdp", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
_native.register("cobalt_pdp_workspace", ctypes.c_int64, [ctypes.c_int64, ctypes.c_int])
_native.register("cobalt_pdp_grid_chunk", ctypes.c_int, [])
_native.register("cobalt_pdp_chunk_rows", ctypes.c_int64, [])
_native.register("cobalt_pdp_max_grid", ctypes.c_int, [])
PDP_MAX_GRID = 1 << 16         # grid points per call (csrc/pdp.hip kPdpMaxGrid)

# csrc/recourse.hip: (X, n, F, ldx, nodes, tree_ptr, tile_ptr, n_tiles, tile_cap, base_margin, feats_host,
# cand_ptr_host, win_host, dir_host, feats, cand_ptr, cand_val, n_cand, win, dir, A, target, idx, margin, stream)
_native.register("cobalt_recourse_scan", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p])
_native.register("cobalt_recourse_chunk", ctypes.c_int, [])
_native.register("cobalt_recourse_chunk_rows", ctypes.c_int64, [])

# csrc/permimp.hip: (X, n, F, ldx, nodes, tree_ptr, tile_ptr, n_tiles, tile_cap, base_margin, feats, nf, cols, perm,
# R, y, w, margins, workspace, sums, rep_chunk, stream)
_native.register("cobalt_perm_importance", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
_native.register("cobalt_perm_workspace", ctypes.c_int64, [ctypes.c_int64, ctypes.c_int])
_native.register("cobalt_perm_rep_chunk", ctypes.c_int, [])
_native.register("cobalt_perm_chunk_rows", ctypes.c_int64, [])
PERM_REP_CHUNK = 0             # repeats per block of csrc/permimp.hip: 0 = its default, 8 or 16 (sweeps)

# csrc/ale.hip: cells (X, n, F, ldx, jobs_host, jobs, J, dims, edges, n_edges, cells, stream); ale (X, n, F, ldx,
# nodes, tree_ptr, tile_ptr, n_tiles, tile_cap, base_margin, jobs_host, jobs, J, dims, edges, n_edges, w, order,
# seg_ptr, max_cells, rows, workspace, sums, stream)
_native.register("cobalt_ale_cells", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p])
_native.register("cobalt_ale", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
_native.register("cobalt_ale_workspace", ctypes.c_int64, [ctypes.c_int64, ctypes.c_int, ctypes.c_int])
_native.register("cobalt_ale_chunk_rows", ctypes.c_int64, [])
_native.register("cobalt_ale_max_intervals", ctypes.c_int, [])
_native.register("cobalt_ale_max_cells", ctypes.c_int, [])
_native.register("cobalt_ale_max_jobs", ctypes.c_int, [])
_native.register("cobalt_ale_no_cell", ctypes.c_int, [])
ALE_MAX_INTERVALS = 4096       # intervals per axis (csrc/ale.hip kAleMaxIntervals)
ALE_MAX_CELLS = 1 << 16        # K1 * K2 of a pair (kAleMaxCells)
ALE_MAX_JOBS = 65535           # features / pairs per launch (kAleMaxJobs); more are split over launches

PATH_ELEM = np.dtype([("lo", "<f4"), ("hi", "<f4"), ("feat", "<i4"), ("nan_ok", "<i4"), ("zero", "<f8")])


def _bfs_order(t: Tree) -> list[int]:
    order, q = [], [0]
    while q:
        nxt = []
        for j in q:
            order.append(j)
            if t.left_children[j] != -1:
                nxt += [int(t.left_children[j]), int(t.right_children[j])]
        q = nxt
    return order


def tile_capacity(b: Booster, n_trees: int | None = None) -> int:
    """LDS tile capacity (nodes) for this forest: TILE_NODES, grown to fit the largest tree."""
    trees = b.trees[: (n_trees if n_trees is not None else b.num_trees)]
    biggest = max((len(t.left_children) for t in trees), default=0)
    cap = max(TILE_NODES, -(-biggest // 64) * 64)
    if cap > MAX_TILE_NODES:
        raise ValueError(f"tree with {biggest} nodes exceeds the LDS tile ({MAX_TILE_NODES} nodes)")
    return cap


def _pack_tree(t: Tree) -> tuple[np.ndarray, np.ndarray]:
    """(meta uint32 [n], val float32 [n]) of one tree in BFS order (csrc/forest_walk.h)."""
    order = _bfs_order(t)
    if len(order) > 0xFFFE:
        raise ValueError("tree too large for the packed predictor")
    nid = {j: i for i, j in enumerate(order)}
    meta = np.zeros(len(order), dtype=np.uint32)
    val = np.zeros(len(order), dtype=np.float32)
    for j, i in nid.items():
        if t.left_children[j] == -1:
            meta[i] = 0xFFFF
        else:
            l, r = nid[int(t.left_children[j])], nid[int(t.right_children[j])]
            assert r == l + 1
            f = int(t.split_indices[j])
            if f > 0x7FFF:
                raise ValueError("feature index too large for the packed predictor")
            meta[i] = (l & 0xFFFF) | (f << 16) | (int(t.default_left[j]) << 31)
        val[i] = t.split_conditions[j]
    return meta, val


def pack_forest(b: Booster, n_trees: int | None = None,
                tile_nodes: int | None = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(nodes uint32 [M, 2], tree_ptr int32 [T+1], tile_ptr int32 [n_tiles+1]); trees are grouped into
    tiles of at most ``tile_nodes`` (default ``tile_capacity``) nodes."""
    tile_nodes = tile_capacity(b, n_trees) if tile_nodes is None else tile_nodes
    trees = b.trees[: (n_trees if n_trees is not None else b.num_trees)]
    metas, vals, tree_ptr = [], [], [0]
    # a tree's packed nodes do not depend on its neighbours: kept per tree, so that packing the prefixes
    # of one model (predict_margin(n_trees=t) for many t) packs every tree once
    packed = b.__dict__.setdefault("_packed_trees", {})
    for t in trees:
        ent = packed.get(id(t))
        if ent is None or ent[0] is not t:
            ent = packed[id(t)] = (t, *_pack_tree(t))
        metas.append(ent[1])
        vals.append(ent[2])
        tree_ptr.append(tree_ptr[-1] + len(ent[1]))
    M = tree_ptr[-1]
    nodes = np.zeros((M, 2), dtype=np.uint32)
    if M:
        nodes[:, 0] = np.concatenate(metas)
        nodes[:, 1] = np.concatenate(vals).view(np.uint32)
    tiles = [0]
    acc = 0
    for i in range(len(trees)):
        sz = tree_ptr[i + 1] - tree_ptr[i]
        if sz > tile_nodes:
            raise ValueError("tree exceeds the LDS tile")
        if acc + sz > tile_nodes:
            tiles.append(i)
            acc = 0
        acc += sz
    tiles.append(len(trees))
    return nodes, np.asarray(tree_ptr, dtype=np.int32), np.asarray(tiles, dtype=np.int32)


def extract_paths(b: Booster) -> tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """Leaf paths with repeated features merged (elements, path_ptr, leaf values, max unique len)."""
    elems: list[tuple] = []
    ptr = [0]
    vals: list[float] = []
    max_len = 0
    for t in b.trees:
        cov = t.sum_hessian.astype(np.float64)
        stack = [(0, [])]
        while stack:
            j, path = stack.pop()
            if t.left_children[j] == -1:
                merged: dict[int, list] = {}
                order: list[int] = []
                for (parent, f, went_left, child) in path:
                    if f not in merged:
                        merged[f] = [-np.inf, np.nan, True, 1.0]  # hi = NaN: no upper bound (x = +inf follows)
                        order.append(f)
                    m = merged[f]
                    thr = float(t.split_conditions[parent])
                    if went_left:
                        m[1] = thr if m[1] != m[1] else min(m[1], thr)
                    else:
                        m[0] = max(m[0], thr)
                    m[2] = m[2] and (bool(t.default_left[parent]) == went_left)
                    m[3] *= cov[child] / cov[parent]
                for f in order:
                    lo, hi, nan_ok, z = merged[f]
                    elems.append((np.float32(lo), np.float32(hi), f, int(nan_ok), z))
                max_len = max(max_len, len(order))
                ptr.append(len(elems))
                vals.append(float(t.split_conditions[j]))
                continue
            f = int(t.split_indices[j])
            l, r = int(t.left_children[j]), int(t.right_children[j])
            stack.append((r, path + [(j, f, False, r)]))
            stack.append((l, path + [(j, f, True, l)]))
    arr = np.array(elems, dtype=PATH_ELEM) if elems else np.zeros(0, dtype=PATH_ELEM)
    return arr, np.asarray(ptr, dtype=np.int32), np.asarray(vals, dtype=np.float64), max_len


@dataclass
class _GpuForest:
    nodes: torch.Tensor
    tree_ptr: torch.Tensor
    tile_ptr: torch.Tensor
    n_tiles: int
    n_trees: int
    tile_cap: int
    elems: torch.Tensor | None = None
    path_ptr: torch.Tensor | None = None
    path_val: torch.Tensor | None = None
    n_paths: int = 0
    max_len: int = 0
    tab_ptr: torch.Tensor | None = None   # Fast-TreeSHAP pattern tables (None: direct kernel)
    table: torch.Tensor | None = None
    unpack: torch.Tensor | None = None    # packed node -> booster node id (None once known: the identity)
    unpack_known: bool = False


def gpu_forest(b: Booster, device: torch.device, n_trees: int | None = None, with_shap: bool = False) -> _GpuForest:
    cache = b.__dict__.setdefault("_gpu_cache", {})
    key = (str(device), n_trees if n_trees is not None else b.num_trees)
    gf = cache.get(key)
    if gf is None:
        cap = tile_capacity(b, n_trees)
        nodes, tptr, tiles = pack_forest(b, n_trees, cap)
        gf = _GpuForest(torch.from_numpy(nodes).to(device), torch.from_numpy(tptr).to(device),
                        torch.from_numpy(tiles).to(device), len(tiles) - 1, len(tptr) - 1, cap)
        cache[key] = gf
    if with_shap and gf.elems is None:
        el, pp, pv, ml = extract_paths(b)
        if ml > MAX_PATH:
            raise ValueError(f"path with {ml} unique features exceeds the GPU TreeSHAP limit {MAX_PATH}")
        gf.elems = torch.from_numpy(el.view(np.uint8).copy()).to(device)
        gf.path_ptr = torch.from_numpy(pp).to(device)
        gf.path_val = torch.from_numpy(pv).to(device)
        gf.n_paths = len(pv)
        gf.max_len = ml
        k = np.diff(pp).astype(np.int64)
        sizes = (np.left_shift(1, k) * k) if len(k) else np.zeros(0, np.int64)
        if len(k) and ml <= SHAP_TABLE_MAX_K and int(sizes.sum()) * 8 <= SHAP_TABLE_MAX_BYTES:
            tp = np.zeros(len(k) + 1, dtype=np.int64)
            np.cumsum(sizes, out=tp[1:])
            gf.tab_ptr = torch.from_numpy(tp).to(device)
            gf.table = torch.empty(int(tp[-1]), dtype=torch.float64, device=device)
            rc = _native.lib().cobalt_shap_table_build(gf.elems.data_ptr(), gf.path_ptr.data_ptr(),
                                                       gf.path_val.data_ptr(), gf.n_paths, ml, gf.tab_ptr.data_ptr(),
                                                       gf.table.data_ptr(), _native.stream_handle())
            _native.check(rc, "cobalt_shap_table_build")
    return gf


def _device_of(X, device) -> torch.device:
    if device is not None:
        d = torch.device(device)
    elif isinstance(X, torch.Tensor):
        d = X.device
    else:
        d = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def _as_f32(X, device: torch.device) -> torch.Tensor:
    if isinstance(X, torch.Tensor):
        return X.to(device=device, dtype=torch.float32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(X, dtype=np.float32)), device=device)


def _check_kernel_rows(b: Booster, X: torch.Tensor) -> None:
    """What the kernels assume of ``X`` and never look at themselves: float32 rows ``stride(0)`` apart with
    unit column stride, at least as wide as the model (a tree reads ``x[feature]``). Raised before any
    launch; :func:`_as_f32` brings any input into this form."""
    if X.dim() != 2:
        raise ValueError(f"X must be [rows, features], got shape {tuple(X.shape)}")
    if X.dtype != torch.float32:
        raise ValueError(f"X must be float32, got {X.dtype}")
    if X.shape[1] > 1 and X.stride(1) != 1:
        raise ValueError(f"X must have unit column stride, got stride {X.stride(1)}")
    if X.shape[1] < b.num_feature:
        raise ValueError(f"X has {X.shape[1]} features, model needs {b.num_feature}")


def predict_gpu(b: Booster, X: torch.Tensor, n_trees: int | None = None, out_margin: torch.Tensor | None = None,
                out_prob: torch.Tensor | None = None) -> None:
    """Launch the predictor on the current stream (graph-capturable: no host sync; small batches use a
    scratch buffer from the caching allocator, which a graph capture takes from its private pool).
    ``X``: float32 with unit column stride (rows may be strided), else ``ValueError``."""
    _check_kernel_rows(b, X)
    gf = gpu_forest(b, X.device, n_trees)
    N, F = X.shape
    lib = _native.lib()
    om = out_margin.data_ptr() if out_margin is not None else None
    op = out_prob.data_ptr() if out_prob is not None else None
    if N < _SMALL_ROWS and N * gf.n_trees <= (1 << 24):
        # tile-parallel path (see csrc/predict.hip): grid = row blocks x tree tiles
        leaves = torch.empty(N * gf.n_trees, dtype=torch.float32, device=X.device)
        rc = lib.cobalt_predict_small(X.data_ptr(), N, F, X.stride(0), gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(),
                                      gf.tile_ptr.data_ptr(), gf.n_tiles, gf.tile_cap, gf.n_trees, b.base_margin,
                                      leaves.data_ptr(), om, op, _native.stream_handle())
        _native.check(rc, "cobalt_predict_small")
        return
    rc = lib.cobalt_predict(X.data_ptr(), N, F, X.stride(0), gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(),
                            gf.tile_ptr.data_ptr(), gf.n_tiles, gf.tile_cap, b.base_margin, om, op,
                            _native.stream_handle())
    _native.check(rc, "cobalt_predict")


_FORCE_DIRECT_SHAP = False  # tests compare the row-parallel table kernel against the direct kernel


def treeshap_gpu(b: Booster, X: torch.Tensor, phi: torch.Tensor) -> None:
    """Write TreeSHAP values into ``phi`` [N, F] float64 on the current stream (deterministic: no
    floating-point atomics; partial sums are combined in a fixed order). ``X`` as for :func:`predict_gpu`."""
    _check_kernel_rows(b, X)
    N, F = X.shape
    gf = gpu_forest(b, X.device, None, with_shap=True)
    lib = _native.lib()
    for s in range(0, N, 65535):
        e = min(N, s + 65535)
        nch = int(lib.cobalt_treeshap_chunks(e - s, F, gf.n_paths))
        work = torch.empty((e - s) * nch * F, dtype=torch.float64, device=X.device) if nch > 1 else None
        wp = work.data_ptr() if work is not None else None
        if gf.table is not None and not _FORCE_DIRECT_SHAP and e - s >= SHAP_ROWS_MIN and F <= SHAP_ROWS_MAX_F:
            rc = lib.cobalt_treeshap_tab(X[s:e].data_ptr(), e - s, F, X.stride(0), gf.elems.data_ptr(),
                                         gf.path_ptr.data_ptr(), gf.n_paths, gf.max_len, gf.tab_ptr.data_ptr(),
                                         gf.table.data_ptr(), phi[s:e].data_ptr(), wp, nch, _native.stream_handle())
            _native.check(rc, "cobalt_treeshap_tab")
        else:
            rc = lib.cobalt_treeshap(X[s:e].data_ptr(), e - s, F, X.stride(0), gf.elems.data_ptr(),
                                     gf.path_ptr.data_ptr(), gf.path_val.data_ptr(), gf.n_paths, gf.max_len,
                                     phi[s:e].data_ptr(), wp, nch, _native.stream_handle())
            _native.check(rc, "cobalt_treeshap")


def predict_margin(b: Booster, X, device=None, n_trees: int | None = None):
    d = _device_of(X, device)
    if d.type == "cuda":
        Xt = _as_f32(X, d)
        out = torch.empty(Xt.shape[0], dtype=torch.float32, device=d)
        predict_gpu(b, Xt, n_trees, out_margin=out)
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()
    Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
    return predict_margin_host(b, Xn, n_trees)


def predict_proba(b: Booster, X, device=None, n_trees: int | None = None):
    d = _device_of(X, device)
    if d.type == "cuda":
        Xt = _as_f32(X, d)
        out = torch.empty(Xt.shape[0], dtype=torch.float32, device=d)
        predict_gpu(b, Xt, n_trees, out_prob=out)
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()
    return sigmoid32(predict_margin(b, X, "cpu", n_trees=n_trees))


# ------------------------------------------------------------------------------- learning curves
# Stage margins held at once by the AUC curve (the forest is scored in tree chunks of this many bytes)
AUC_STAGE_BYTES = 256 << 20


def _eval_curve_launch(b: Booster, Xt: torch.Tensor, yt: torch.Tensor | None, wt: torch.Tensor | None,
                       margin_in: torch.Tensor | None, margin_out: torch.Tensor | None,
                       stages: torch.Tensor | None) -> torch.Tensor | None:
    """One ``cobalt_eval_curve`` call over all trees of ``b`` on the current stream; returns the [T, 3]
    float64 sums (sum w loss, sum w err, sum w) when ``yt`` is given."""
    gf = gpu_forest(b, Xt.device)
    N, F = Xt.shape
    if F < b.num_feature:
        raise ValueError(f"X has {F} features, model needs {b.num_feature}")
    lib = _native.lib()
    sums = work = None
    if yt is not None:
        sums = torch.empty((gf.n_trees, 3), dtype=torch.float64, device=Xt.device)
        work = torch.empty(int(lib.cobalt_eval_curve_workspace(N, gf.n_trees)), dtype=torch.uint8, device=Xt.device)
    rc = lib.cobalt_eval_curve(Xt.data_ptr(), N, F, Xt.stride(0), _native.ptr(yt), _native.ptr(wt),
                               gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(), gf.tile_ptr.data_ptr(), gf.n_tiles,
                               gf.tile_cap, gf.n_trees, b.base_margin, _native.ptr(margin_in),
                               _native.ptr(margin_out), _native.ptr(stages), _native.ptr(work), _native.ptr(sums),
                               _native.stream_handle())
    _native.check(rc, "cobalt_eval_curve")
    return sums


def _tree_range(b: Booster, t0: int, t1: int) -> Booster:
    return Booster(b.trees[t0:t1], b.feature_names, b.feature_types, b.base_score, b.num_feature, b.objective)


def _host_vec(v, dtype=np.float32) -> np.ndarray:
    return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(dtype).reshape(-1)


def eval_curve(b: Booster, X, y, sample_weight=None, metrics=("logloss",), device=None, margin=None):
    """``({metric: float64 [num_trees]}, final margins [N] float32)``: the metrics of ``(X, y)`` after every
    tree. GPU: one pass of ``csrc/evalcurve.hip`` over the forest for "logloss" / "error" (deterministic:
    the same input gives the same bits); "auc" scores :func:`staged_margins` in bounded tree chunks with
    :func:`~..metrics.auc.roc_auc` (unweighted). CPU: :func:`~..models.booster.eval_curve_host`.
    ``margin``: start from these margins instead of the base margin. Raises ``ValueError`` before any
    launch for labels outside [0, 1], weights that sum to <= 0, row-count mismatches, an unknown metric and
    "auc" with one class."""
    d = _device_of(X, device)
    if d.type != "cuda":
        Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
        return eval_curve_host(b, Xn, _host_vec(y), None if sample_weight is None else _host_vec(sample_weight),
                               metrics, None if margin is None else _host_vec(margin))
    Xt = _as_f32(X, d)
    N = Xt.shape[0]
    # labels and weights are a few bytes per row: they are checked on the host
    y32 = _host_vec(y)
    w32 = None if sample_weight is None else _host_vec(sample_weight)
    m_rows = None if margin is None else int(torch.as_tensor(margin).reshape(-1).shape[0])
    metrics = check_eval_inputs(N, y32, w32, metrics, m_rows)
    yt = torch.as_tensor(y32, device=d)
    wt = None if w32 is None else torch.as_tensor(w32, device=d)
    m_in = None if margin is None else torch.as_tensor(margin).to(device=d, dtype=torch.float32).reshape(-1).contiguous()
    T = b.num_trees
    out: dict[str, np.ndarray] = {}
    m_out = torch.empty(N, dtype=torch.float32, device=d)
    if T == 0:
        m_out = m_in.clone() if m_in is not None else torch.full((N,), b.base_margin, dtype=torch.float32, device=d)
        out = {m: np.empty(0, dtype=np.float64) for m in metrics}
    elif "logloss" in metrics or "error" in metrics:
        s = _eval_curve_launch(b, Xt, yt, wt, m_in, m_out, None).cpu().numpy()
        if "logloss" in metrics:
            out["logloss"] = s[:, 0] / s[:, 2]
        if "error" in metrics:
            out["error"] = s[:, 1] / s[:, 2]
    if "auc" in metrics and T:
        from ..metrics.auc import roc_auc

        auc = np.empty(T, dtype=np.float64)
        ypos = (yt > 0.5).to(torch.float64)
        per = max(1, AUC_STAGE_BYTES // max(4 * N, 1))
        cur = m_in
        for t0 in range(0, T, per):
            t1 = min(T, t0 + per)
            stages = torch.empty((t1 - t0, N), dtype=torch.float32, device=d)
            nxt = torch.empty(N, dtype=torch.float32, device=d)
            _eval_curve_launch(b if (t0, t1) == (0, T) else _tree_range(b, t0, t1), Xt, None, None, cur, nxt, stages)
            for t in range(t0, t1):
                auc[t] = roc_auc(ypos, stages[t - t0])
            cur = nxt
        m_out = cur
        out["auc"] = auc
    out = {m: out[m] for m in metrics}
    return out, (m_out if isinstance(X, torch.Tensor) else m_out.cpu().numpy())


def staged_margins(b: Booster, X, device=None):
    """Margins after every tree, [num_trees, N] float32 (stage ``t`` has the bits of
    ``predict_margin(n_trees=t + 1)``); one forest pass on the GPU."""
    d = _device_of(X, device)
    if d.type != "cuda":
        Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
        return staged_margins_host(b, Xn)
    Xt = _as_f32(X, d)
    stages = torch.empty((b.num_trees, Xt.shape[0]), dtype=torch.float32, device=d)
    if b.num_trees and Xt.shape[0]:
        _eval_curve_launch(b, Xt, None, None, None, None, stages)
    return stages if isinstance(X, torch.Tensor) else stages.cpu().numpy()


# --------------------------------------------------------------------------- partial dependence
def _check_pd_args(b: Booster, feats, grids) -> tuple[tuple[int, ...], list[np.ndarray]]:
    """Features as a tuple of one or two distinct indices inside the model, grids as non-empty float32
    vectors (one per feature; NaN = the feature is missing). ``ValueError`` otherwise."""
    feats = tuple(int(f) for f in feats)
    if len(feats) not in (1, 2):
        raise ValueError(f"partial dependence takes one or two features, got {len(feats)}")
    for f in feats:
        if not 0 <= f < b.num_feature:
            raise ValueError(f"feature index {f} outside [0, {b.num_feature})")
    if len(feats) == 2 and feats[0] == feats[1]:
        raise ValueError(f"the two features must differ, got {feats}")
    if len(grids) != len(feats):
        raise ValueError(f"{len(feats)} features need {len(feats)} grids, got {len(grids)}")
    out = []
    for g in grids:
        g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        g = np.ascontiguousarray(g, dtype=np.float32)
        if g.ndim != 1 or g.shape[0] == 0:
            raise ValueError(f"a grid axis must be a non-empty vector, got shape {g.shape}")
        out.append(g)
    return feats, out


def partial_dependence_gpu(b: Booster, X: torch.Tensor, feats, grids, *, n_trees: int | None = None,
                           weights: torch.Tensor | None = None, want_ice: bool,
                           want_avg: bool) -> tuple[torch.Tensor | None, torch.Tensor | None]:
    """Launch ``csrc/pdp.hip`` on the current stream (no host sync). Grid point ``k = i1 * G2 + i2`` scores
    every row with ``x[feats[0]] = grids[0][i1]`` (and ``x[feats[1]] = grids[1][i2]``); ``X`` is not written.
    Returns ``(ice, sums)``: ``ice`` [G, N] float32 margins with the bits of ``predict_margin`` on the
    substituted rows (``want_ice``), ``sums`` [2 G + 1] float64 = (sum w m, sum w p) per grid point, then
    sum w (``want_avg``; deterministic: fixed reduction order, no floating-point atomics). ``X`` as for
    :func:`predict_gpu`; ``weights``: float32 [N] on the device of ``X``. ``ValueError`` / ``RuntimeError``
    (a model outside the kernel's LDS limits) before anything is launched."""
    _check_kernel_rows(b, X)
    feats, grids = _check_pd_args(b, feats, grids)
    N, F = X.shape
    G1 = len(grids[0])
    G2 = len(grids[1]) if len(feats) == 2 else 1
    G = G1 * G2
    if G > PDP_MAX_GRID:
        raise ValueError(f"{G} grid points exceed the limit of {PDP_MAX_GRID} per call")
    if weights is not None and (weights.dtype != torch.float32 or weights.dim() != 1 or weights.shape[0] != N
                                or weights.device != X.device or not weights.is_contiguous()):
        raise ValueError(f"weights must be a contiguous float32 [{N}] tensor on {X.device}")
    gf = gpu_forest(b, X.device, n_trees)
    lib = _native.lib()
    g1 = torch.from_numpy(grids[0]).to(X.device)
    g2 = torch.from_numpy(grids[1]).to(X.device) if len(feats) == 2 else None
    ice = torch.empty((G, N), dtype=torch.float32, device=X.device) if want_ice else None
    sums = work = None
    if want_avg:
        sums = torch.zeros(2 * G + 1, dtype=torch.float64, device=X.device)
        work = torch.empty(int(lib.cobalt_pdp_workspace(N, G)), dtype=torch.uint8, device=X.device)
    rc = lib.cobalt_pdp(X.data_ptr(), N, F, X.stride(0), gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(),
                        gf.tile_ptr.data_ptr(), gf.n_tiles, gf.tile_cap, b.base_margin, feats[0],
                        feats[1] if len(feats) == 2 else -1, g1.data_ptr(), G1, _native.ptr(g2), G2,
                        _native.ptr(weights), _native.ptr(ice), _native.ptr(work), _native.ptr(sums),
                        _native.stream_handle())
    _native.check(rc, "cobalt_pdp")
    return ice, sums


def partial_dependence(b: Booster, X, feats, grids, *, n_trees: int | None = None, weights=None,
                       want_ice: bool = True, want_avg: bool = True, device=None):
    """``(ice, avg_margin, avg_prob)`` as NumPy: ICE margins [G, N] float32 (None without ``want_ice``) and
    the weighted means over the rows of the margin and of the probability, float64 [G] (None without
    ``want_avg``), at the grid points ``k = i1 * G2 + i2``. A CUDA device runs ``csrc/pdp.hip``, the CPU runs
    :func:`~..models.booster.partial_dependence_host` (the definition)."""
    d = _device_of(X, device)
    w32 = None if weights is None else _host_vec(weights)
    if d.type != "cuda":
        Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
        feats, grids = _check_pd_args(b, feats, grids)
        ice, am, ap = partial_dependence_host(b, Xn, feats, grids, n_trees, w32)
        return (ice if want_ice else None), (am if want_avg else None), (ap if want_avg else None)
    Xt = _as_f32(X, d)
    wt = None if w32 is None else torch.as_tensor(w32, device=d)
    ice, sums = partial_dependence_gpu(b, Xt, feats, grids, n_trees=n_trees, weights=wt, want_ice=want_ice,
                                       want_avg=want_avg)
    am = ap = None
    if sums is not None:
        s = sums.cpu().numpy()
        am, ap = s[0:-1:2] / s[-1], s[1:-1:2] / s[-1]
    return (None if ice is None else ice.cpu().numpy()), am, ap


# ---------------------------------------------------------------------- counterfactual recourse
def recourse_scan_gpu(b: Booster, X: torch.Tensor, feats, cands, *, win=None, dirs=None, target_margin: float,
                      n_trees: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Launch ``csrc/recourse.hip`` on the current stream (no host sync): for every row and every actionable
    feature the nearest candidate below (slot 0) and above (slot 1) the row's own position whose substituted
    margin is ``<= target_margin``, and the candidate with the lowest margin (slot 2); the definition is
    :func:`~..models.booster.recourse_scan_host`. Returns ``(idx, margin)``, int32 and float32 ``[N, A, 3]`` on the
    device of ``X``; margins have the bits of ``predict_margin`` on the substituted rows and ``X`` is not
    written. ``X`` as for :func:`predict_gpu`. ``ValueError`` / ``RuntimeError`` (a model outside the kernel's LDS
    limits) before anything is launched."""
    _check_kernel_rows(b, X)
    feats, cands, win, dirs = check_recourse_args(b, feats, cands, win, dirs)
    N, F = X.shape
    A = len(feats)
    cand_ptr = np.zeros(A + 1, dtype=np.int64)
    np.cumsum([len(cv) for cv in cands], out=cand_ptr[1:])
    if cand_ptr[-1] >= 2 ** 31:
        raise ValueError("too many candidates for one call")
    # one int32 table on the host (checked by the entry point) and its copy on the device (read by the kernel)
    table = np.concatenate([np.asarray(feats, np.int32), cand_ptr.astype(np.int32), win.reshape(-1), dirs])
    table = np.ascontiguousarray(table, dtype=np.int32)
    off = np.cumsum([0, A, A + 1, 2 * A]) * 4
    table_d = torch.from_numpy(table).to(X.device)
    vals = np.concatenate(cands) if cand_ptr[-1] else np.zeros(1, np.float32)
    vals_d = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32)).to(X.device)
    gf = gpu_forest(b, X.device, n_trees)
    idx = torch.empty((N, A, 3), dtype=torch.int32, device=X.device)
    margin = torch.empty((N, A, 3), dtype=torch.float32, device=X.device)
    hp, dp = table.ctypes.data, table_d.data_ptr()
    rc = _native.lib().cobalt_recourse_scan(
        X.data_ptr(), N, F, X.stride(0), gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(), gf.tile_ptr.data_ptr(),
        gf.n_tiles, gf.tile_cap, b.base_margin, *(hp + int(o) for o in off), *(dp + int(o) for o in off[:2]),
        vals_d.data_ptr(), int(cand_ptr[-1]), dp + int(off[2]), dp + int(off[3]), A, float(np.float32(target_margin)),
        idx.data_ptr(), margin.data_ptr(), _native.stream_handle())
    _native.check(rc, "cobalt_recourse_scan")
    return idx, margin


def recourse_scan(b: Booster, X, feats, cands, *, win=None, dirs=None, target_margin: float,
                  n_trees: int | None = None, device=None):
    """``(idx, margin)`` of a recourse scan, [N, A, 3]: tensors on the device for a CUDA tensor ``X``, NumPy
    otherwise. A CUDA device runs ``csrc/recourse.hip``, the CPU runs
    :func:`~..models.booster.recourse_scan_host` (the definition)."""
    d = _device_of(X, device)
    if d.type != "cuda":
        Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
        return recourse_scan_host(b, Xn, feats, cands, win, dirs, target_margin, n_trees)
    idx, margin = recourse_scan_gpu(b, _as_f32(X, d), feats, cands, win=win, dirs=dirs, target_margin=target_margin,
                                    n_trees=n_trees)
    return (idx, margin) if isinstance(X, torch.Tensor) else (idx.cpu().numpy(), margin.cpu().numpy())


# ------------------------------------------------------------------------ permutation importance
def permutation_scores_gpu(b: Booster, X: torch.Tensor, y: torch.Tensor | None, feats, perm: torch.Tensor, *,
                           n_trees: int | None = None, weights: torch.Tensor | None = None, want_margins: bool,
                           want_sums: bool) -> tuple[torch.Tensor | None, torch.Tensor | None]:
    """Launch ``csrc/permimp.hip`` on the current stream. Job 0 scores ``X`` (the baseline), job
    ``1 + i * R + r`` scores every row ``n`` with ``x[feats[i]] = X[perm[r][n], feats[i]]``; ``X`` is not written.
    Returns ``(margins, sums)``: ``margins`` [1 + nf R, N] float32 with the bits of ``predict_margin`` on the
    substituted matrix (``want_margins``), ``sums`` [2 (1 + nf R) + 1] float64 = (sum w loss, sum w err) per
    job, then sum w (``want_sums``; deterministic: fixed reduction order, no floating-point atomics).
    ``X`` as for :func:`predict_gpu`; ``y`` (needed for the sums) and ``weights``: contiguous float32 [N] on the
    device of ``X``; ``perm``: contiguous int32 [R, N] on that device. The kernel reads
    ``cols[i][perm[r][n]]`` unchecked, so the range of ``perm`` is checked here, on the device (two
    reductions and the one host read of this function). ``ValueError`` / ``RuntimeError`` (a model outside
    the kernel's LDS limits) before anything of the kernel is launched."""
    _check_kernel_rows(b, X)
    N, F = X.shape
    feats = [int(f) for f in feats]
    for f in feats:
        if not 0 <= f < b.num_feature:
            raise ValueError(f"feature index {f} outside [0, {b.num_feature})")
    nf = len(feats)
    if (not isinstance(perm, torch.Tensor) or perm.dtype != torch.int32 or perm.dim() != 2 or perm.shape[0] < 1
            or perm.shape[1] != N or perm.device != X.device or not perm.is_contiguous()):
        raise ValueError(f"perm must be a contiguous int32 [R >= 1, {N}] tensor on {X.device}")
    R = int(perm.shape[0])
    for name, v in (("y", y), ("weights", weights)):
        if v is not None and (v.dtype != torch.float32 or v.dim() != 1 or v.shape[0] != N or v.device != X.device
                              or not v.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 [{N}] tensor on {X.device}")
    if want_sums and y is None:
        raise ValueError("the sums need y")
    if N == 0:
        raise ValueError("X has no rows")
    lo, hi = (int(v) for v in torch.stack([perm.min(), perm.max()]).tolist())
    if lo < 0 or hi >= N:
        raise ValueError(f"perm must hold row indices in [0, {N}), got [{lo}, {hi}]")
    J = 1 + nf * R
    gf = gpu_forest(b, X.device, n_trees)
    lib = _native.lib()
    ft = torch.tensor(feats, dtype=torch.int32, device=X.device) if nf else None
    cols = X[:, feats].t().contiguous() if nf else None   # [nf, N]: the gather reads 4 N contiguous bytes
    margins = torch.empty((J, N), dtype=torch.float32, device=X.device) if want_margins else None
    sums = work = None
    if want_sums:
        sums = torch.zeros(2 * J + 1, dtype=torch.float64, device=X.device)
        work = torch.empty(int(lib.cobalt_perm_workspace(N, J)), dtype=torch.uint8, device=X.device)
    rc = lib.cobalt_perm_importance(X.data_ptr(), N, F, X.stride(0), gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(),
                                    gf.tile_ptr.data_ptr(), gf.n_tiles, gf.tile_cap, b.base_margin, _native.ptr(ft),
                                    nf, _native.ptr(cols), perm.data_ptr(), R, _native.ptr(y) if want_sums else None,
                                    _native.ptr(weights), _native.ptr(margins), _native.ptr(work),
                                    _native.ptr(sums), PERM_REP_CHUNK, _native.stream_handle())
    _native.check(rc, "cobalt_perm_importance")
    return margins, sums


def permutation_scores(b: Booster, X, y, feats, perm, *, n_trees: int | None = None, weights=None,
                       metrics=("logloss",), device=None) -> tuple[dict[str, float], dict[str, np.ndarray]]:
    """``(baseline, scores)``: ``{metric: float}`` of ``(X, y)`` and ``{metric: float64 [len(feats), R]}`` of
    the jobs (feature ``feats[i]`` shuffled by ``perm[r]``). A CUDA device runs ``csrc/permimp.hip``: "logloss"
    and "error" come from one launch that never materialises margins; "auc" stages the margins of at most
    ``AUC_STAGE_BYTES`` of jobs at a time and scores each with :func:`~..metrics.auc.roc_auc`, as
    :func:`eval_curve` does. The CPU runs :func:`~..models.booster.permutation_scores_host` (the definition).
    ``ValueError`` as there, before any launch."""
    d = _device_of(X, device)
    y32 = _host_vec(y)
    w32 = None if weights is None else _host_vec(weights)
    if d.type != "cuda":
        Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
        pn = perm.cpu().numpy() if isinstance(perm, torch.Tensor) else np.asarray(perm)
        return permutation_scores_host(b, Xn, y32, feats, pn, n_trees, w32, metrics)
    Xt = _as_f32(X, d)
    N = Xt.shape[0]
    pshape = tuple(perm.shape) if hasattr(perm, "shape") else np.asarray(perm).shape
    metrics = check_perm_inputs(N, y32, w32, metrics, pshape)
    if isinstance(perm, torch.Tensor):
        if perm.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise ValueError("perm must hold integer row indices")
        if perm.dtype != torch.int32 and (int(perm.min()) < 0 or int(perm.max()) >= N):
            raise ValueError(f"perm must hold row indices in [0, {N})")
        pt = perm.to(device=d, dtype=torch.int32).contiguous()
    else:
        pn = np.asarray(perm)
        if pn.dtype.kind not in "iu" or int(pn.min()) < 0 or int(pn.max()) >= N:
            raise ValueError(f"perm must hold integer row indices in [0, {N})")
        pt = torch.as_tensor(np.ascontiguousarray(pn, dtype=np.int32), device=d)
    feats = [int(f) for f in feats]
    nf, R = len(feats), int(pt.shape[0])
    yt = torch.as_tensor(y32, device=d)
    wt = None if w32 is None else torch.as_tensor(w32, device=d)
    base: dict[str, float] = {}
    scores: dict[str, np.ndarray] = {}
    if "logloss" in metrics or "error" in metrics:
        _, sums = permutation_scores_gpu(b, Xt, yt, feats, pt, n_trees=n_trees, weights=wt, want_margins=False,
                                         want_sums=True)
        s = sums.cpu().numpy()
        for k, name in enumerate(("logloss", "error")):
            if name in metrics:
                v = s[k:-1:2] / s[-1]
                base[name] = float(v[0])
                scores[name] = v[1:].reshape(nf, R).copy()
    if "auc" in metrics:
        from ..metrics.auc import roc_auc

        ypos = (yt > 0.5).to(torch.float64)
        auc = np.empty((nf, R), dtype=np.float64)
        per = max(1, AUC_STAGE_BYTES // max(4 * N, 1) - 1)  # jobs per launch next to its baseline
        have_base = False
        if per >= R:  # whole features: per // R of them at a time
            groups = [(feats[i:i + per // R], i, 0, R) for i in range(0, nf, per // R)]
        else:         # one feature at a time, `per` of its repeats
            groups = [([feats[i]], i, r0, min(R, r0 + per)) for i in range(nf) for r0 in range(0, R, per)]
        for fs, i0, r0, r1 in groups or [([], 0, 0, R)]:
            m, _ = permutation_scores_gpu(b, Xt, None, fs, pt[r0:r1], n_trees=n_trees, want_margins=True,
                                          want_sums=False)
            if not have_base:
                base["auc"] = float(roc_auc(ypos, m[0]))
                have_base = True
            for i in range(len(fs)):
                for r in range(r1 - r0):
                    auc[i0 + i, r0 + r] = roc_auc(ypos, m[1 + i * (r1 - r0) + r])
        scores["auc"] = auc
    return {m: base[m] for m in metrics}, {m: scores[m] for m in metrics}


# ------------------------------------------------------------------- accumulated local effects
# Entries of the [jobs, N] int32 cell and order matrices of one launch series (4 + 4 bytes each: 1 GiB): more
# jobs are split over several series, each of which stages the rows again. Results do not depend on it.
ALE_JOB_ENTRIES = 1 << 27


def _check_ale_args(b: Booster, jobs, edges) -> tuple[list[tuple[int, ...]], list[list[np.ndarray]]]:
    """Jobs as tuples of one or two distinct feature indices inside the model (all of one kind), with one
    finite, strictly increasing float32 edge vector per feature, within the kernel's limits. ``ValueError``
    otherwise."""
    jobs = [tuple(int(f) for f in (j if isinstance(j, (tuple, list)) else (j,))) for j in jobs]
    if not jobs:
        raise ValueError("no ALE job")
    dims = len(jobs[0])
    if len(edges) != len(jobs):
        raise ValueError(f"{len(jobs)} jobs need {len(jobs)} edge lists, got {len(edges)}")
    out = []
    for feats, ez in zip(jobs, edges):
        if len(feats) not in (1, 2) or len(feats) != dims:
            raise ValueError(f"the jobs of one call take one feature each or two each, got {feats} next to {jobs[0]}")
        for f in feats:
            if not 0 <= f < b.num_feature:
                raise ValueError(f"feature index {f} outside [0, {b.num_feature})")
        if dims == 2 and feats[0] == feats[1]:
            raise ValueError(f"the two features must differ, got {feats}")
        ez = [ez] if dims == 1 and not isinstance(ez, (tuple, list)) else list(ez)
        if len(ez) != dims:
            raise ValueError(f"{dims} features need {dims} edge vectors, got {len(ez)}")
        ez = [check_ale_edges(z) for z in ez]
        if any(len(z) - 1 > ALE_MAX_INTERVALS for z in ez) or int(np.prod([len(z) - 1 for z in ez])) > ALE_MAX_CELLS:
            raise ValueError(f"at most {ALE_MAX_INTERVALS} intervals per feature and {ALE_MAX_CELLS} cells per pair")
        out.append(ez)
    return jobs, out


def accumulated_local_effects_gpu(b: Booster, X: torch.Tensor, jobs, edges, *, n_trees: int | None = None,
                                  weights: torch.Tensor | None = None, want_rows: bool,
                                  want_sums: bool) -> tuple[torch.Tensor | None, torch.Tensor | None]:
    """Launch ``csrc/ale.hip`` on the current stream (no host sync). ``jobs``: tuples of one feature index each,
    or of two each; ``edges``: per job one edge vector per feature (K + 1 increasing values = K intervals). Job
    ``j`` scores every row at the corners of the interval / cell it lies in (``models.booster.ale_host``: corner
    ``c = i1 + 2 i2``); ``X`` is not written. Returns ``(rows, sums)``: ``rows`` [J, C, N] float32 corner
    margins, C = 2 or 4, with the bits of ``predict_margin`` on the substituted rows (``want_rows``); ``sums``
    [J, max cells, 3] float64 = (sum w d_margin, sum w d_prob, sum w) per interval ``k - 1`` / cell
    ``(k - 1) * K2 + (l - 1)`` (``want_sums``; rows with NaN in a feature of the job enter no sum). The sums
    are grouped without atomics: the rows' cells are sorted stably per row chunk (``torch.sort``) and one block
    per cell adds its segment in a fixed order, so the same input gives the same bits. ``X`` as for
    :func:`predict_gpu`; ``weights``: float32 [N] on the device of ``X``. ``ValueError`` / ``RuntimeError`` (a
    model outside the kernel's LDS limits) before anything of the walk is launched."""
    _check_kernel_rows(b, X)
    jobs, edges = _check_ale_args(b, jobs, edges)
    N, F = X.shape
    if N == 0:
        raise ValueError("X has no rows")
    J, dims = len(jobs), len(jobs[0])
    if J > ALE_MAX_JOBS:
        raise ValueError(f"{J} jobs exceed the limit of {ALE_MAX_JOBS} per call")
    if weights is not None and (weights.dtype != torch.float32 or weights.dim() != 1 or weights.shape[0] != N
                                or weights.device != X.device or not weights.is_contiguous()):
        raise ValueError(f"weights must be a contiguous float32 [{N}] tensor on {X.device}")
    desc = np.zeros((J, 6), dtype=np.int32)   # {f1, f2, off1, K1, off2, K2}
    flat, off = [], 0
    for j, (feats, ez) in enumerate(zip(jobs, edges)):
        desc[j] = (feats[0], -1, off, len(ez[0]) - 1, 0, 1)
        flat.append(ez[0])
        off += len(ez[0])
        if dims == 2:
            desc[j, 1], desc[j, 4], desc[j, 5] = feats[1], off, len(ez[1]) - 1
            flat.append(ez[1])
            off += len(ez[1])
    max_cells = int((desc[:, 3].astype(np.int64) * desc[:, 5]).max())
    gf = gpu_forest(b, X.device, n_trees)
    lib = _native.lib()
    dev = X.device
    jd = torch.from_numpy(desc).to(dev)
    ed = torch.from_numpy(np.concatenate(flat)).to(dev)
    stream = _native.stream_handle()
    order = seg = sums = work = None
    if want_sums:
        cells = torch.empty((J, N), dtype=torch.int32, device=dev)
        rc = lib.cobalt_ale_cells(X.data_ptr(), N, F, X.stride(0), desc.ctypes.data, jd.data_ptr(), J, dims,
                                  ed.data_ptr(), off, cells.data_ptr(), stream)
        _native.check(rc, "cobalt_ale_cells")
        chunk = int(lib.cobalt_ale_chunk_rows())
        starts = range(0, N, chunk)
        order = torch.empty((J, N), dtype=torch.int32, device=dev)
        seg = torch.empty((len(starts), J, max_cells + 1), dtype=torch.int32, device=dev)
        bounds = torch.arange(max_cells + 1, dtype=torch.int32, device=dev).expand(J, -1).contiguous()
        for ci, r0 in enumerate(starts):
            srt, idx = torch.sort(cells[:, r0:r0 + chunk], dim=1, stable=True)
            order[:, r0:r0 + chunk] = idx   # chunk-local row indices, cell by cell, ascending inside a cell
            seg[ci] = torch.searchsorted(srt.contiguous(), bounds, out_int32=True)
        sums = torch.zeros((J, max_cells, 3), dtype=torch.float64, device=dev)
        if not want_rows:
            work = torch.empty(int(lib.cobalt_ale_workspace(N, J, dims)), dtype=torch.uint8, device=dev)
    rows = torch.empty((J, 1 << dims, N), dtype=torch.float32, device=dev) if want_rows else None
    rc = lib.cobalt_ale(X.data_ptr(), N, F, X.stride(0), gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(),
                        gf.tile_ptr.data_ptr(), gf.n_tiles, gf.tile_cap, b.base_margin, desc.ctypes.data,
                        jd.data_ptr(), J, dims, ed.data_ptr(), off, _native.ptr(weights), _native.ptr(order),
                        _native.ptr(seg), max_cells, _native.ptr(rows), _native.ptr(work), _native.ptr(sums), stream)
    _native.check(rc, "cobalt_ale")
    return rows, sums


def accumulated_local_effects(b: Booster, X, jobs, edges, *, n_trees: int | None = None, weights=None,
                              device=None) -> list[dict]:
    """The ALE sums of every job (a tuple of one or two feature indices, with one edge vector per feature; one-
    and two-feature jobs may be mixed), as NumPy: per job ``{"sum_margin", "sum_prob", "weight": float64 [K1] or
    [K1, K2], "n_missing": int}`` (``models.booster.ale_curve`` turns them into curves). A CUDA device runs
    ``csrc/ale.hip``, all jobs of a kind in one launch series; the CPU runs
    :func:`~..models.booster.ale_host` (the definition) job by job."""
    d = _device_of(X, device)
    w32 = None if weights is None else _host_vec(weights)
    jobs = [tuple(int(f) for f in (j if isinstance(j, (tuple, list)) else (j,))) for j in jobs]
    out: list[dict | None] = [None] * len(jobs)
    if d.type != "cuda":
        Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
        for i, (feats, ez) in enumerate(zip(jobs, edges)):
            ez = [ez] if len(feats) == 1 and not isinstance(ez, (tuple, list)) else list(ez)
            r = ale_host(b, Xn, feats, ez, n_trees, w32)
            out[i] = {k: r[k] for k in ("sum_margin", "sum_prob", "weight", "n_missing")}
        return out
    Xt = _as_f32(X, d)
    N = Xt.shape[0]
    if w32 is not None and w32.shape[0] != N:
        raise ValueError(f"X has {N} rows, weights has {w32.shape[0]}")
    wt = None if w32 is None else torch.as_tensor(w32, device=d)
    per = max(1, min(ALE_MAX_JOBS, ALE_JOB_ENTRIES // max(N, 1)))
    for dims in (1, 2):
        ids = [i for i, feats in enumerate(jobs) if len(feats) == dims]
        for g0 in range(0, len(ids), per):
            grp = ids[g0:g0 + per]
            gj, ge = _check_ale_args(b, [jobs[i] for i in grp], [edges[i] for i in grp])
            _, sums = accumulated_local_effects_gpu(b, Xt, gj, ge, n_trees=n_trees, weights=wt, want_rows=False,
                                                    want_sums=True)
            nan = torch.isnan(Xt)
            miss = torch.stack([nan[:, list(feats)].any(dim=1).sum() for feats in gj]).cpu().numpy()
            s = sums.cpu().numpy()
            for q, i in enumerate(grp):
                shape = tuple(len(z) - 1 for z in ge[q])
                c = s[q, :int(np.prod(shape))]
                out[i] = {"sum_margin": c[:, 0].reshape(shape).copy(), "sum_prob": c[:, 1].reshape(shape).copy(),
                          "weight": c[:, 2].reshape(shape).copy(), "n_missing": int(miss[q])}
    if any(o is None for o in out):
        raise ValueError("an ALE job takes one or two features")
    return out


# ------------------------------------------------------------------- leaf indices and leaf refresh
# Bytes of the tree-major uint16 [trees, N] leaf-index buffer of csrc/refresh.hip (2 N bytes per tree): the
# forest is processed in groups of trees whose buffer fits. 1 GiB holds the 300-tree model's indices of 1.7M
# rows in one group and still takes 53 trees at a time at 10M rows (a group costs one extra launch and a
# re-staging of the rows); results do not depend on it.
LEAF_INDEX_BYTES = 1 << 30
REFRESH_MAX_NODES = 6301       # largest tree of the refresh kernels (csrc/refresh.hip cobalt_refresh_max_nodes)


def _unpack_table(b: Booster, gf: _GpuForest) -> torch.Tensor | None:
    """int32 [M] on the forest's device: booster node id of every packed node (the inverse of pack_forest's
    BFS renumbering), or None when the booster's numbering already is the packed one (the trainer's is)."""
    if gf.unpack_known:
        return gf.unpack
    orders = [np.asarray(_bfs_order(t), dtype=np.int32) for t in b.trees[:gf.n_trees]]
    if any((o != np.arange(len(o), dtype=np.int32)).any() for o in orders):
        gf.unpack = torch.from_numpy(np.concatenate(orders)).to(gf.nodes.device)
    gf.unpack_known = True
    return gf.unpack


def _group_trees(n_rows: int, n_trees: int, leaf_index_bytes: int | None) -> int:
    nbytes = LEAF_INDEX_BYTES if leaf_index_bytes is None else int(leaf_index_bytes)
    if nbytes < 1:
        raise ValueError(f"leaf_index_bytes must be positive, got {leaf_index_bytes}")
    return max(1, min(n_trees, nbytes // max(2 * n_rows, 1)))


def predict_leaf_gpu(b: Booster, X: torch.Tensor, n_trees: int | None = None,
                     leaf_index_bytes: int | None = None) -> torch.Tensor:
    """int32 [N, T] on the device of ``X``: the booster node id of every row's leaf in every tree
    (``csrc/refresh.hip`` k_leaf_index on the current stream, then a gather through the per-tree table that
    undoes the packer's renumbering). ``X`` as for :func:`predict_gpu`. The device buffer of packed indices
    is tree-major uint16 and bounded by ``leaf_index_bytes`` (default ``LEAF_INDEX_BYTES``): the trees are
    taken in groups."""
    _check_kernel_rows(b, X)
    gf = gpu_forest(b, X.device, n_trees)
    N, F = X.shape
    T = gf.n_trees
    out = torch.empty((N, T), dtype=torch.int32, device=X.device)
    if N == 0 or T == 0:
        return out
    lib = _native.lib()
    table = _unpack_table(b, gf)
    per = _group_trees(N, T, leaf_index_bytes)
    idx = torch.empty((per, N), dtype=torch.int16, device=X.device)  # (uint16 bits)
    for t0 in range(0, T, per):
        t1 = min(T, t0 + per)
        rc = lib.cobalt_leaf_index(X.data_ptr(), N, F, X.stride(0), gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(),
                                   gf.tile_ptr.data_ptr(), gf.n_tiles, gf.tile_cap, T, t0, t1, idx.data_ptr(),
                                   _native.stream_handle())
        _native.check(rc, "cobalt_leaf_index")
        packed = idx[: t1 - t0].to(torch.int32) & 0xFFFF
        if table is not None:
            packed = table[(packed + gf.tree_ptr[t0:t1, None]).long()]
        out[:, t0:t1] = packed.t()
    return out


def predict_leaf(b: Booster, X, device=None, n_trees: int | None = None):
    d = _device_of(X, device)
    if n_trees is not None and not 0 <= n_trees <= b.num_trees:
        raise ValueError(f"n_trees must be in [0, {b.num_trees}], got {n_trees}")
    if d.type == "cuda":
        out = predict_leaf_gpu(b, _as_f32(X, d), n_trees)
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()
    Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
    out = predict_leaf_host(b, Xn, n_trees)
    return torch.from_numpy(out) if isinstance(X, torch.Tensor) else out


def refresh_gpu(b: Booster, X: torch.Tensor, y: torch.Tensor, w: torch.Tensor, p: dict, gscale: float,
                hscale: float, refresh_leaf: bool, leaf_index_bytes: int | None = None):
    """Launch ``csrc/refresh.hip`` over all trees of ``b`` on the current stream (2 T + a few launches, no host
    synchronisation in between). ``X`` as for :func:`predict_gpu`; ``y`` / ``w``: contiguous float32 [N] on its
    device (``w`` = the row weights of :func:`~..models.booster.refresh_row_weights`); ``p``:
    :func:`~..models.booster.refresh_params`. Returns device tensors in PACKED node order (``pack_forest``):
    ``(sums int64 [M, 2], stats float32 [3, M] = base weight / cover / loss change, leaf values float32 [M],
    margins float32 [N])``. ``RuntimeError`` for a tree outside the kernels' LDS tables, before any launch."""
    _check_kernel_rows(b, X)
    N, F = X.shape
    for name, v in (("y", y), ("w", w)):
        if v.dtype != torch.float32 or v.dim() != 1 or v.shape[0] != N or v.device != X.device or not v.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 [{N}] tensor on {X.device}")
    gf = gpu_forest(b, X.device)
    T = gf.n_trees
    tptr = np.ascontiguousarray(pack_forest(b, None, gf.tile_cap)[1], dtype=np.int32)
    M = int(tptr[-1])
    biggest = int(np.diff(tptr).max()) if T else 0
    if biggest > REFRESH_MAX_NODES:
        raise RuntimeError(f"a tree with {biggest} nodes exceeds the refresh kernels' LDS tables "
                           f"({REFRESH_MAX_NODES} nodes)")
    per = _group_trees(N, T, leaf_index_bytes)
    idx = torch.empty((per, N), dtype=torch.int16, device=X.device)
    sums = torch.empty((M, 2), dtype=torch.int64, device=X.device)
    stats = torch.empty((3, M), dtype=torch.float32, device=X.device)
    leaf_val = torch.empty(M, dtype=torch.float32, device=X.device)
    margin = torch.full((N,), b.base_margin, dtype=torch.float32, device=X.device)
    rc = _native.lib().cobalt_refresh(X.data_ptr(), N, F, X.stride(0), y.data_ptr(), w.data_ptr(), gf.nodes.data_ptr(),
                                      gf.tree_ptr.data_ptr(), gf.tile_ptr.data_ptr(), gf.n_tiles, gf.tile_cap, T,
                                      tptr.ctypes.data, p["eta"], p["reg_lambda"], p["reg_alpha"],
                                      p["min_child_weight"], gscale, hscale, int(p["seed"]) & ((1 << 64) - 1),
                                      p["grad_bits"], int(bool(refresh_leaf)), per, idx.data_ptr(), sums.data_ptr(),
                                      stats.data_ptr(), leaf_val.data_ptr(), margin.data_ptr(),
                                      _native.stream_handle())
    _native.check(rc, "cobalt_refresh")
    return sums, stats, leaf_val, margin


def refresh(b: Booster, X, y, sample_weight=None, *, refresh_leaf: bool = True, device=None,
            leaf_index_bytes: int | None = None, dist=None, node_sums: list | None = None, **overrides):
    """``(new booster, its margins on X)``: :meth:`Booster.refresh`. A CUDA device runs ``csrc/refresh.hip``
    (byte-identical to the CPU path, :func:`~..models.booster.refresh_host`, the definition). The margins are a
    tensor on the device for a tensor ``X``, else NumPy. ``leaf_index_bytes``: bound of the device buffer of
    leaf indices (default ``LEAF_INDEX_BYTES``; the trees are processed in groups that fit, and the result
    does not depend on the grouping). ``node_sums``: a list that receives every tree's int64 [n, 2] node sums
    in the booster's numbering. ``ValueError`` (:func:`~..models.booster.check_refresh_inputs`) before any
    launch."""
    d = _device_of(X, device)
    y32 = _host_vec(y)
    w32 = None if sample_weight is None else _host_vec(sample_weight)
    if d.type != "cuda":
        Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
        new, margin = refresh_host(b, Xn, y32, w32, refresh_leaf=refresh_leaf, dist=dist, node_sums=node_sums,
                                   **overrides)
        return new, (torch.from_numpy(margin) if isinstance(X, torch.Tensor) else margin)
    # labels and weights are a few bytes per row: they are checked, and the row weights formed, on the host
    check_refresh_inputs(b, tuple(X.shape), y32, w32, dist)
    p = refresh_params(b, overrides)
    wt = refresh_row_weights(y32, w32, p["scale_pos_weight"])
    gscale, hscale = quant_scales(float(wt.max()), p["grad_bits"])
    Xt = _as_f32(X, d)
    sums, stats, leaf_val, margin = refresh_gpu(b, Xt, torch.as_tensor(y32, device=d), torch.as_tensor(wt, device=d),
                                                p, gscale, hscale, refresh_leaf, leaf_index_bytes)
    sums_h, stats_h, leaf_h = sums.cpu().numpy(), stats.cpu().numpy(), leaf_val.cpu().numpy()
    trees, n0 = [], 0
    for t in b.trees:
        order = np.asarray(_bfs_order(t), dtype=np.int64)  # packed index -> booster node id
        n1 = n0 + len(order)
        cols = []
        for src in (stats_h[0, n0:n1], stats_h[1, n0:n1], stats_h[2, n0:n1], leaf_h[n0:n1]):
            a = np.empty(len(order), dtype=np.float32)
            a[order] = src
            cols.append(a)
        if node_sums is not None:
            s = np.empty((len(order), 2), dtype=np.int64)
            s[order] = sums_h[n0:n1]
            node_sums.append(s)
        trees.append(refreshed_tree(t, *cols, refresh_leaf))
        n0 = n1
    new = _refreshed_booster(b, trees, p)
    return new, (margin if isinstance(X, torch.Tensor) else margin.cpu().numpy())


def shap_values(b: Booster, X, device=None):
    d = _device_of(X, device)
    if d.type == "cuda":
        Xt = _as_f32(X, d)
        _check_kernel_rows(b, Xt)  # (a narrower X than the model: ValueError before anything is launched)
        phi = torch.zeros((Xt.shape[0], Xt.shape[1]), dtype=torch.float64, device=d)
        treeshap_gpu(b, Xt, phi)
        return phi if isinstance(X, torch.Tensor) else phi.cpu().numpy()
    Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
    if Xn.ndim != 2 or Xn.shape[1] < b.num_feature:
        raise ValueError(f"X has shape {Xn.shape}, model needs [rows, >= {b.num_feature}]")
    return treeshap_host(b, Xn)


# tests run the long-path kernel variant on models whose paths would take the short-path one
_FORCE_LONG_PATH_INTERACTIONS = False


def treeshap_interactions_gpu(b: Booster, X: torch.Tensor, out: torch.Tensor) -> None:
    """Write TreeSHAP interaction values into ``out`` [N, F, F] float64 on the current stream
    (deterministic like :func:`treeshap_gpu`: a row's values do not depend on the batch). Raises
    ``ValueError`` before anything is launched when the model is outside the kernel's limits."""
    N, F = X.shape
    if F < b.num_feature:
        raise ValueError(f"X has {F} features, model needs {b.num_feature}")
    if F > SHAP_INT_MAX_F:
        raise ValueError(f"{F} features exceed the GPU TreeSHAP interaction limit of {SHAP_INT_MAX_F} features")
    if tuple(out.shape) != (N, F, F) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float64 [{N}, {F}, {F}] tensor")
    if N == 0:
        return
    gf = gpu_forest(b, X.device, None, with_shap=True)  # (raises ValueError past MAX_PATH features per path)
    lib = _native.lib()
    max_len = MAX_PATH if _FORCE_LONG_PATH_INTERACTIONS else gf.max_len
    for s in range(0, N, SHAP_INT_ROWS):
        e = min(N, s + SHAP_INT_ROWS)
        phi = torch.zeros((e - s, F), dtype=torch.float64, device=X.device)
        treeshap_gpu(b, X[s:e], phi)
        rc = lib.cobalt_treeshap_interactions(X[s:e].data_ptr(), e - s, F, X.stride(0), gf.elems.data_ptr(),
                                              gf.path_ptr.data_ptr(), gf.path_val.data_ptr(), gf.n_paths,
                                              max_len, phi.data_ptr(), out[s:e].data_ptr(),
                                              _native.stream_handle())
        _native.check(rc, "cobalt_treeshap_interactions")


def shap_interaction_values(b: Booster, X, device=None):
    d = _device_of(X, device)
    if d.type == "cuda":
        Xt = _as_f32(X, d)
        out = torch.empty((Xt.shape[0], Xt.shape[1], Xt.shape[1]), dtype=torch.float64, device=d)
        treeshap_interactions_gpu(b, Xt, out)
        return out if isinstance(X, torch.Tensor) else out.cpu().numpy()
    Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
    return treeshap_interactions_host(b, Xn)


# ------------------------------------------------------------------------ interventional TreeSHAP
_FORCE_BG_TILE = 0  # tests: background rows per tile (0 = from the model), so small sets span several tiles


def _background_tile(n_paths: int) -> int:
    """Background rows per launch: a function of the model alone, so a row's values do not depend on N."""
    if _FORCE_BG_TILE:
        return max(1, min(int(_FORCE_BG_TILE), SHAP_BG_MAX_TILE))
    return max(1, min(SHAP_BG_MAX_TILE, SHAP_BG_MASK_BYTES // max(2 * n_paths, 1)))


def _sliced(b: Booster, n_trees: int | None) -> Booster:
    """The first ``n_trees`` trees as a booster, kept with ``b`` (its packed paths live on the object)."""
    if n_trees is None or n_trees == b.num_trees:
        return b
    if not 0 <= n_trees <= b.num_trees:
        raise ValueError(f"n_trees must be in [0, {b.num_trees}], got {n_trees}")
    cache = b.__dict__.setdefault("_slice_cache", {})
    ent = cache.get(n_trees)
    if ent is None or len(ent.trees) != n_trees or any(x is not y for x, y in zip(ent.trees, b.trees)):
        ent = cache[n_trees] = b.slice(n_trees)
    return ent


def treeshap_interventional_gpu(b: Booster, X: torch.Tensor, Z: torch.Tensor, phi: torch.Tensor, *,
                                probability: bool = False) -> None:
    """Write the interventional TreeSHAP values of the rows ``X`` against the background rows ``Z`` into
    ``phi`` [N, F] float64 on the current stream (``csrc/shapbg.hip``; margin space, or ``shap``'s per-pair
    rescaling to probability space). Deterministic: no floating-point atomics, and a row's values do not
    depend on the batch. ``X`` and ``Z`` as for :func:`predict_gpu` (rows may be strided). The workspace is a
    background tile of masks (``SHAP_BG_MASK_BYTES``) whatever N and B are. ``ValueError`` before anything is
    launched for an empty background, more than ``MAX_PATH`` unique features on a path and more than
    ``SHAP_BG_MAX_F`` columns."""
    _check_kernel_rows(b, X)
    _check_kernel_rows(b, Z)
    N, F = X.shape
    B, Fz = Z.shape
    if B == 0:
        raise ValueError("the background set has no rows")
    if Z.device != X.device:
        raise ValueError(f"X is on {X.device}, the background on {Z.device}")
    if max(F, Fz) > SHAP_BG_MAX_F:
        raise ValueError(f"{max(F, Fz)} columns exceed the GPU interventional TreeSHAP limit of {SHAP_BG_MAX_F}")
    if tuple(phi.shape) != (N, F) or phi.dtype != torch.float64 or not phi.is_contiguous() or phi.device != X.device:
        raise ValueError(f"phi must be a contiguous float64 [{N}, {F}] tensor on {X.device}")
    gf = gpu_forest(b, X.device, None, with_shap=True)  # (raises ValueError past MAX_PATH features per path)
    if N == 0:
        return
    lib = _native.lib()
    stream = _native.stream_handle()
    tile = _background_tile(gf.n_paths)
    zmask = torch.empty(max(min(tile, B) * gf.n_paths, 1), dtype=torch.int16, device=X.device)
    zmargin = torch.empty(min(tile, B), dtype=torch.float64, device=X.device)
    paths = (_native.ptr(gf.elems), gf.path_ptr.data_ptr(), gf.path_val.data_ptr(), gf.n_paths, gf.max_len)
    for r0 in range(0, N, SHAP_BG_ROWS):
        Xr = X[r0:r0 + SHAP_BG_ROWS]
        n = Xr.shape[0]
        xmargin = None
        if probability:
            xmargin = torch.empty(n, dtype=torch.float64, device=X.device)
            rc = lib.cobalt_shapbg_masks(Xr.data_ptr(), n, F, X.stride(0), *paths, float(b.base_margin), None,
                                         xmargin.data_ptr(), stream)
            _native.check(rc, "cobalt_shapbg_masks")
        for t0 in range(0, B, tile):
            Zt = Z[t0:t0 + tile]
            nb = Zt.shape[0]
            rc = lib.cobalt_shapbg_masks(Zt.data_ptr(), nb, Fz, Z.stride(0), *paths, float(b.base_margin),
                                         zmask.data_ptr(), zmargin.data_ptr(), stream)
            _native.check(rc, "cobalt_shapbg_masks")
            rc = lib.cobalt_treeshap_interventional(Xr.data_ptr(), n, F, X.stride(0), *paths, zmask.data_ptr(),
                                                    zmargin.data_ptr(), nb, _native.ptr(xmargin), int(t0 == 0),
                                                    int(t0 + nb == B), B, phi[r0:r0 + n].data_ptr(), stream)
            _native.check(rc, "cobalt_treeshap_interventional")


def shap_values_interventional(b: Booster, X, Z, *, model_output: str = "raw", n_trees: int | None = None,
                               device=None):
    """Interventional TreeSHAP values [N, F] float64 of ``X`` against the background rows ``Z``: a tensor in
    gives a tensor on the device out, NumPy in gives NumPy out. A CUDA device runs ``csrc/shapbg.hip``, the
    CPU runs :func:`~..models.booster.treeshap_interventional_host` (the definition). ``n_trees``: the first
    trees only. ``ValueError`` for an empty background and for ``X`` or ``Z`` narrower than the model."""
    prob = check_model_output(model_output)
    b = _sliced(b, n_trees)
    d = _device_of(X, device)
    if d.type == "cuda":
        Xt, Zt = _as_f32(X, d), _as_f32(Z, d)
        _check_kernel_rows(b, Xt)
        _check_kernel_rows(b, Zt)
        phi = torch.empty((Xt.shape[0], Xt.shape[1]), dtype=torch.float64, device=d)
        treeshap_interventional_gpu(b, Xt, Zt, phi, probability=prob)
        return phi if isinstance(X, torch.Tensor) else phi.cpu().numpy()
    Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X, dtype=np.float32)
    Zn = Z.cpu().numpy() if isinstance(Z, torch.Tensor) else np.asarray(Z, dtype=np.float32)
    check_background(b, Xn, Zn)
    return treeshap_interventional_host(b, Xn, Zn, model_output)
