"""Hand-built forests and an independent SHAP oracle for the predictor / TreeSHAP tests
(test_scoring_oracle_cpu.py, test_gpu_scoring_edges.py). Plain functions, no fixtures, no training:
``Tree`` / ``Booster`` objects are assembled from arrays, so a test chooses the width, the tree sizes,
the path lengths, the thresholds and the covers exactly.

The oracle, :func:`shap_bruteforce`, computes path-dependent Shapley values from the definition (a sum
over feature subsets of cover-weighted expectations) on the raw trees: no leaf paths, no EXTEND / UNWIND,
nothing shared with ``treeshap_host`` or the kernels.
"""
from __future__ import annotations

import math

import numpy as np

from cobalt_smart_lender_ai_amd.models import booster as B
from cobalt_smart_lender_ai_amd.models.booster import ROOT_PARENT, Booster, Tree

# Largest |treeshap_host - shap_bruteforce| / max|phi| over the forests of test_scoring_oracle_cpu.py
# (measured there and asserted not to be exceeded); the GPU tolerance is derived from it.
EPS_REF = 3.7e-15
BRUTE_MAX_FEATURES = 12


# ------------------------------------------------------------------------------------ builders
class _Nodes:
    """A tree under construction: parallel lists, children appended in pairs."""

    def __init__(self):
        self.left, self.right, self.parent = [-1], [-1], [ROOT_PARENT]
        self.feat, self.thr, self.dl, self.depth = [0], [0.0], [0], [0]

    def split(self, j: int, feat: int, thr: float, default_left: int) -> tuple[int, int]:
        l = len(self.left)
        for _ in range(2):
            self.left.append(-1)
            self.right.append(-1)
            self.parent.append(j)
            self.feat.append(0)
            self.thr.append(0.0)
            self.dl.append(0)
            self.depth.append(self.depth[j] + 1)
        self.left[j], self.right[j] = l, l + 1
        self.feat[j], self.thr[j], self.dl[j] = int(feat), float(thr), int(default_left)
        return l, l + 1

    def path_features(self, j: int) -> set[int]:
        out = set()
        while self.parent[j] != ROOT_PARENT:
            j = self.parent[j]
            out.add(self.feat[j])
        return out

    def finish(self, rng, leaf_cover=None) -> Tree:
        """Leaf values ~ N(0, 0.1) float32; leaf covers integers in [1, 64] (or ``leaf_cover(node)``),
        every parent the exact float32 sum of its children."""
        n = len(self.left)
        left = np.asarray(self.left, np.int32)
        cond = np.asarray(self.thr, np.float32)
        cover = np.zeros(n, np.float64)
        for j in range(n - 1, -1, -1):  # children have larger indices than their parent
            if left[j] == -1:
                cond[j] = np.float32(rng.normal(0.0, 0.1))
                cover[j] = float(rng.integers(1, 65)) if leaf_cover is None else float(leaf_cover(j))
            else:
                cover[j] = cover[self.left[j]] + cover[self.right[j]]
        assert cover[0] > 0 and cover.max() < 2 ** 24
        return Tree(left_children=left, right_children=np.asarray(self.right, np.int32),
                    parents=np.asarray(self.parent, np.int32), split_indices=np.asarray(self.feat, np.int32),
                    split_conditions=cond, default_left=np.asarray(self.dl, np.uint8),
                    base_weights=np.zeros(n, np.float32), loss_changes=np.zeros(n, np.float32),
                    sum_hessian=cover.astype(np.float32))


def _pick_split(rng, nodes: _Nodes, j: int, cols, repeat: bool, grid, default_left):
    """(feature, threshold, default_left) for a split at node ``j``; None when no feature is left."""
    cand = list(cols) if repeat else [c for c in cols if c not in nodes.path_features(j)]
    if not cand:
        return None
    f = int(cand[int(rng.integers(len(cand)))])
    thr = float(grid[int(rng.integers(len(grid)))]) if grid is not None else float(np.float32(rng.normal()))
    dl = int(rng.integers(2)) if default_left is None else int(default_left)
    return f, thr, dl


def random_tree(rng, F: int, depth: int, p_leaf: float = 0.15, *, cols=None, repeat: bool = True, grid=None,
                default_left=None) -> Tree:
    """A random tree of at most ``depth`` levels of splits; below the root a node is a leaf with
    probability ``p_leaf``. ``cols``: the features splits may use (default all ``F``); ``repeat``: a feature
    may occur again on a path; ``grid``: thresholds are drawn from these values; ``default_left``: 0 / 1
    forces the missing-value direction, None mixes both."""
    cols = list(range(F)) if cols is None else list(cols)
    nodes = _Nodes()
    j = 0
    while j < len(nodes.left):
        if nodes.depth[j] < depth and (j == 0 or rng.random() >= p_leaf):
            s = _pick_split(rng, nodes, j, cols, repeat, grid, default_left)
            if s is not None:
                nodes.split(j, *s)
        j += 1
    return nodes.finish(rng)


def grown_tree(rng, F: int, n_leaves: int, max_depth: int = 12, *, cols=None, repeat: bool = True, grid=None,
               default_left=None) -> Tree:
    """A tree with exactly ``n_leaves`` leaves (2 n_leaves - 1 nodes): random leaves are split until the
    count is reached, none deeper than ``max_depth``."""
    cols = list(range(F)) if cols is None else list(cols)
    nodes = _Nodes()
    leaves = [0]
    while len(leaves) < n_leaves:
        open_ = [j for j in leaves if nodes.depth[j] < max_depth
                 and (repeat or len(nodes.path_features(j)) < len(cols))]
        assert open_, "cannot reach the requested number of leaves"
        j = open_[int(rng.integers(len(open_)))]
        l, r = nodes.split(j, *_pick_split(rng, nodes, j, cols, repeat, grid, default_left))
        leaves.remove(j)
        leaves += [l, r]
    return nodes.finish(rng)


def stump(value: float = 0.25, cover: float = 7.0) -> Tree:
    """A single-leaf tree: one leaf path with no element."""
    return Tree(left_children=np.array([-1], np.int32), right_children=np.array([-1], np.int32),
                parents=np.array([ROOT_PARENT], np.int32), split_indices=np.zeros(1, np.int32),
                split_conditions=np.array([value], np.float32), default_left=np.zeros(1, np.uint8),
                base_weights=np.zeros(1, np.float32), loss_changes=np.zeros(1, np.float32),
                sum_hessian=np.array([cover], np.float32))


def caterpillar(rng, k: int, cols, *, grid=None, default_left=None) -> Tree:
    """A chain of ``k`` splits on ``k`` distinct features (the first ``k`` of a shuffle of ``cols``): every
    split has one leaf child and the chain goes on at the other, on a random side. The longest path has
    exactly ``k`` distinct features; ``k == 0`` is a stump."""
    if k == 0:
        return stump(float(np.float32(rng.normal(0.0, 0.1))), float(rng.integers(1, 65)))
    feats = [int(c) for c in rng.permutation(list(cols))[:k]]
    assert len(feats) == k, "not enough features for the chain"
    nodes = _Nodes()
    j = 0
    for f in feats:
        thr = float(grid[int(rng.integers(len(grid)))]) if grid is not None else float(np.float32(rng.normal(0.0, 0.5)))
        dl = int(rng.integers(2)) if default_left is None else int(default_left)
        l, r = nodes.split(j, f, thr, dl)
        j = l if rng.random() < 0.5 else r
    return nodes.finish(rng)


def zero_cover_tree(rng, f_root: int = 0, f_inner: int = 1, zero_side: str = "left") -> Tree:
    """Root split on ``f_root`` at 0; its left child splits on ``f_inner`` at 0 into one leaf of cover 0 and
    one of positive cover (a loaded model, or ``min_child_weight=0`` with zero-weight rows); the root's right
    child is a leaf. Rows with x[f_root] < 0 and x[f_inner] < 0 (``zero_side="left"``) enter the zero-cover
    leaf."""
    nodes = _Nodes()
    l, _ = nodes.split(0, f_root, 0.0, int(rng.integers(2)))
    zl, zr = nodes.split(l, f_inner, 0.0, int(rng.integers(2)))
    z = zl if zero_side == "left" else zr
    return nodes.finish(rng, leaf_cover=lambda j: 0.0 if j == z else float(rng.integers(1, 65)))


def make_booster(trees, F: int, base_score: float = 0.3) -> Booster:
    """A fresh ``Booster`` (the GPU forest cache lives on the object)."""
    return Booster(list(trees), num_feature=F, base_score=base_score)


def random_forest(rng, F: int, n_trees: int, depth: int, p_leaf: float = 0.15, **kw) -> Booster:
    return make_booster([random_tree(rng, F, depth, p_leaf, **kw) for _ in range(n_trees)], F)


def forest_with_paths(rng, F: int, n_paths: int, leaves_per_tree: int = 8, max_depth: int = 4, **kw) -> Booster:
    """A forest with exactly ``n_paths`` leaf paths: trees of ``leaves_per_tree`` leaves and one smaller
    last tree (a stump when one path is left over)."""
    trees, left = [], n_paths
    while left > 0:
        m = min(left, leaves_per_tree)
        trees.append(stump(float(np.float32(rng.normal(0.0, 0.1)))) if m == 1
                     else grown_tree(rng, F, m, max_depth, **kw))
        left -= m
    return make_booster(trees, F)


def n_leaf_paths(b: Booster) -> int:
    return int(sum(int(t.is_leaf.sum()) for t in b.trees))


def max_unique_path(b: Booster) -> int:
    """Largest number of distinct features on one root-to-leaf path."""
    best = 0
    for t in b.trees:
        for _, path in B.iter_leaf_paths(t):
            best = max(best, len({f for _, f, _ in path}))
    return best


# -------------------------------------------------------------------------------- query rows
THRESHOLD_GRID = np.array([-1.5, 0.0, 0.25, np.nextafter(np.float32(0.25), np.float32(1.0)), 1.0, 2.5],
                          dtype=np.float32)  # 0.25 and its upper neighbour: thresholds one ulp apart


def edge_values(grid=THRESHOLD_GRID) -> np.ndarray:
    """Every threshold, its two neighbouring floats, +-inf, NaN, +-0 and the float32 denormals around 0."""
    g = np.asarray(grid, np.float32)
    tiny = np.float32(1e-45)  # smallest denormal
    vals = np.concatenate([g, np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf)),
                           np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, tiny, -tiny, 1e-39], np.float32)])
    return vals.astype(np.float32)


def edge_rows(rng, n: int, F: int, grid=THRESHOLD_GRID) -> np.ndarray:
    """[n, F] float32 rows whose cells are drawn from :func:`edge_values`; the first rows hold every
    value once in every column."""
    vals = edge_values(grid)
    X = vals[rng.integers(len(vals), size=(n, F))]
    m = min(n, len(vals))
    X[:m, :] = vals[:m, None]
    return np.ascontiguousarray(X, dtype=np.float32)


def predict_rowwise(b: Booster, X: np.ndarray, n_trees: int | None = None) -> np.ndarray:
    """The obvious walk: one row at a time, ``x < threshold`` goes left, NaN takes the default
    direction, float32 sum in tree order from the base margin."""
    X = np.asarray(X, np.float32)
    out = np.empty(X.shape[0], np.float32)
    for r in range(X.shape[0]):
        acc = np.float32(b.base_margin)
        for t in b.trees[: (b.num_trees if n_trees is None else n_trees)]:
            j = 0
            while t.left_children[j] != -1:
                v = X[r, t.split_indices[j]]
                left = bool(t.default_left[j]) if np.isnan(v) else bool(v < t.split_conditions[j])
                j = int(t.left_children[j] if left else t.right_children[j])
            acc = np.float32(acc + t.split_conditions[j])
        out[r] = acc
    return out


# ------------------------------------------------------------------------------------ oracle
def tree_features(t: Tree) -> list[int]:
    return sorted({int(f) for f in t.split_indices[~t.is_leaf]})


def _subset_values(t: Tree, X: np.ndarray, feats: list[int]) -> np.ndarray:
    """f_S(x) for all rows and all subsets S of ``feats`` ([N, 2^M] float64, bit i of the column index =
    feats[i] in S): at a split on a feature of S follow x, otherwise average the children by
    cover(child) / cover(parent)."""
    M = len(feats)
    bit = {f: i for i, f in enumerate(feats)}
    masks = np.arange(1 << M)
    cov = t.sum_hessian.astype(np.float64)

    def value(j: int) -> np.ndarray:
        if t.left_children[j] == -1:
            return np.full((1, 1), float(t.split_conditions[j]), np.float64)
        f = int(t.split_indices[j])
        l, r = int(t.left_children[j]), int(t.right_children[j])
        vl, vr = value(l), value(r)
        x = X[:, f]
        go_left = np.where(np.isnan(x), bool(t.default_left[j]), x < t.split_conditions[j])[:, None]
        in_s = ((masks >> bit[f]) & 1).astype(bool)[None, :]
        mean = vl * (cov[l] / cov[j]) + vr * (cov[r] / cov[j])
        return np.where(in_s, np.where(go_left, vl, vr), mean)

    return np.broadcast_to(value(0), (X.shape[0], 1 << M))


def shap_bruteforce(b: Booster, X: np.ndarray, max_features: int = BRUTE_MAX_FEATURES) -> np.ndarray:
    """Exact path-dependent Shapley values [N, F] float64 from the definition: per tree, over the M
    features the tree uses, ``phi_i = sum_{S without i} |S|! (M - |S| - 1)! / M! (f_{S+i}(x) - f_S(x))``.
    A tree with more than ``max_features`` distinct features falls back to ``treeshap_host``."""
    X = np.asarray(X, np.float32)
    N, F = X.shape
    phi = np.zeros((N, F), np.float64)
    for t in b.trees:
        feats = tree_features(t)
        M = len(feats)
        if M == 0:
            continue
        if M > max_features:
            phi += B.treeshap_host(Booster([t], num_feature=b.num_feature), X)
            continue
        masks = np.arange(1 << M)
        size = np.zeros(1 << M, np.int64)
        for i in range(M):
            size += (masks >> i) & 1
        wgt = np.array([math.factorial(s) * math.factorial(M - s - 1) / math.factorial(M) if s < M else 0.0
                        for s in range(M + 1)], np.float64)
        step = max(1, (1 << 21) >> M)  # rows per block: [step, 2^M] doubles stay near 16 MB
        for r0 in range(0, N, step):
            v = _subset_values(t, X[r0:r0 + step], feats)
            for i, f in enumerate(feats):
                without = masks[((masks >> i) & 1) == 0]
                phi[r0:r0 + step, f] += ((v[:, without | (1 << i)] - v[:, without]) * wgt[size[without]]).sum(1)
    return phi
