"""The accumulated-local-effects kernels (csrc/ale.hip) on the hand-built forests of scoring_forests.py and on a
small fitted model.

Corner margins: bit for bit against ``scoring_forests.predict_rowwise`` (one row at a time, independent of the
kernel and of ``predict_margin_host``) on explicitly substituted copies of X, the row's interval found here by
counting the edges below its value (independent of ``searchsorted``).

Interval sums: the bound of test_gpu_pdp.py for its averages, ``(n + 8) * 2^-52 * sum w|t|`` with ``n`` the rows
of the interval and ``t`` the terms that enter the sum, against the ``math.fsum`` sums of ``ale_host`` (the
standard bound ``(n - 1) u sum|x_i|``, u = 2^-53, of a floating-point sum of n terms in any order, doubled, plus
a few ulp for ``exp``). In margin units t is the row's effect (a difference of float32 margins, exact in
float64). In probability units the effect is a difference of sigmoids, each of which carries the few ulp by which
the device's ``exp`` may differ from NumPy's, so t is the sum of the corner probabilities, not their
difference. Derived, not measured; the tests print the largest ratio to the bound as ``[ale] ...``.

Curves: ``ale_curve`` is the same code for both paths, so the curve's error is the propagated error of the
interval means. With ``d_k = bound_k / W_k + |e_k| (n_k + 8) 2^-52`` the error of mean k (numerator and
denominator) and ``D = sum_k d_k``: every A[k] is a sum of at most all means (error <= D); 1-D centring subtracts
one weighted average of A (<= D more); in 2-D g1, g2 and the final mean are such averages of A or of its
differences (<= 5 D more), and the weights inside each of the averages carry the relative error that D already
holds once per interval (<= 2 D per average). That is at most 12 D; the tests allow ``16 D + 64 K u max|A|``, the
last term for the roundings of the cumulative sums themselves.

Which test catches which mistake in the kernel:
  ``<=`` instead of ``<`` in the interval search .. test_corner_margins (rows and splits exactly on edges, one ulp above)
  a fork that trusts the row's own path ........... test_repeated_splits_inside_one_interval
  corners in the wrong order (i2 + 2 i1) .......... test_corner_margins 2-D (edges of the two axes differ)
  tail lanes or NaN rows contributing weight ...... test_interval_sums (N = 65, 257; NaN rows; all rows NaN)
  a segment off by one ............................ test_interval_sums (weights per interval are exact integers unweighted)
  chunk-local against global row indices .......... test_chunking
"""
import functools
import math

import numpy as np
import pytest
import torch

import scoring_forests as sf
from cobalt_smart_lender_ai_amd import _native, explain
from cobalt_smart_lender_ai_amd.models import booster as B
from cobalt_smart_lender_ai_amd.models import gbdt
from cobalt_smart_lender_ai_amd.ops import predict_ops

pytestmark = pytest.mark.gpu

ROWS = (1, 65, 257)   # 257: a second block with one live row
U52 = 2.0 ** -52


# ------------------------------------------------------------------------------------ helpers
def _interval(z, x):
    """k in [1, K]: the edges below x, clamped (NaN: no edge is below)."""
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore"):
        return np.clip((z[None, :] < np.asarray(x, np.float32)[:, None]).sum(1), 1, len(z) - 1)


def _substituted(X, feats, edges):
    """[C * N, F]: the copies of X at the corners c = i1 + 2 i2 of every row's own interval / cell."""
    ks = [_interval(z, X[:, f]) for f, z in zip(feats, edges)]
    out = []
    for c in range(1 << len(feats)):
        Xs = np.array(X, np.float32)
        for a, (f, z) in enumerate(zip(feats, edges)):
            Xs[:, f] = np.asarray(z, np.float32)[ks[a] - 1 + ((c >> a) & 1)]
        out.append(Xs)
    return np.concatenate(out)


def _want(b, X, feats, edges, n_trees=None):
    return sf.predict_rowwise(b, _substituted(X, feats, edges), n_trees).reshape(1 << len(feats), X.shape[0])


def _gpu(b, Xd, jobs, edges, n_trees=None, w=None, rows=True, sums=False):
    r, s = predict_ops.accumulated_local_effects_gpu(b, Xd, jobs, edges, n_trees=n_trees, weights=w, want_rows=rows,
                                                     want_sums=sums)
    return (None if r is None else r.cpu().numpy()), (None if s is None else s.cpu().numpy())


def _check_corners(b, X, jobs, edges, label, n_trees=None, want=None):
    """All jobs in one call; every job's corner margins against the row-wise walk."""
    X = np.ascontiguousarray(X, np.float32)
    Xd = torch.from_numpy(X).cuda()
    got, _ = _gpu(b, Xd, jobs, edges, n_trees)
    C = 1 << len(jobs[0])
    assert got.dtype == np.float32 and got.shape == (len(jobs), C, X.shape[0]), (label, got.shape)
    for j, (feats, ez) in enumerate(zip(jobs, edges)):
        w_j = _want(b, X, feats, ez, n_trees) if want is None else want[j]
        np.testing.assert_array_equal(got[j], w_j, err_msg=f"{label} job {feats}")
    assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True), label  # X is never written
    return got


def _normal_rows(rng, n, F, nan=0.05):
    X = rng.normal(size=(n, F)).astype(np.float32)
    X[rng.random(X.shape) < nan] = np.nan
    return X


def _check_sums(b, X, jobs, edges, w, n_trees=None):
    """GPU sums of all jobs in one call against ale_host, and the curves made of them; returns the largest
    |error| / bound."""
    X = np.ascontiguousarray(X, np.float32)
    Xd = torch.from_numpy(X).cuda()
    wd = None if w is None else torch.from_numpy(np.asarray(w, np.float32)).cuda()
    rows, sums = _gpu(b, Xd, jobs, edges, n_trees, w=wd, sums=True)
    _, alone = _gpu(b, Xd, jobs, edges, n_trees, w=wd, rows=False, sums=True)   # corner margins in the workspace
    np.testing.assert_array_equal(alone, sums)
    w64 = np.ones(X.shape[0]) if w is None else np.asarray(w, np.float32).astype(np.float64)
    worst = 0.0
    for j, (feats, ez) in enumerate(zip(jobs, edges)):
        h = B.ale_host(b, X, feats, ez, n_trees, w)
        np.testing.assert_array_equal(rows[j], h["corners"])
        shape = h["weight"].shape
        ncell = int(np.prod(shape))
        got = sums[j, :ncell]
        assert not sums[j, ncell:].any()          # cells past the job's own are never written
        m = h["corners"].astype(np.float64)
        p = 1.0 / (1.0 + np.exp(-m))
        dm = m[1] - m[0] if len(feats) == 1 else (m[3] - m[2]) - (m[1] - m[0])
        err_e = {0: np.zeros(ncell), 1: np.zeros(ncell)}
        for c in range(ncell):
            idx = np.flatnonzero(h["cell"] == c)
            n = len(idx)
            terms = (np.abs(dm[idx]), p[:, idx].sum(0), np.ones(n))
            exact = (h["sum_margin"].reshape(-1)[c], h["sum_prob"].reshape(-1)[c], h["weight"].reshape(-1)[c])
            for q in range(3):
                bound = (n + 8) * U52 * math.fsum(w64[idx] * terms[q])
                err = abs(got[c, q] - exact[q])
                assert err <= bound, (feats, c, q, err, bound)
                worst = max(worst, err / bound if bound > 0 else 0.0)
                if q < 2 and exact[2] > 0:
                    err_e[q][c] = bound / exact[2] + abs(exact[q] / exact[2]) * (n + 8) * U52
            if n == 0:
                assert not got[c].any()
        if w is None:  # unweighted: the interval weights are the row counts, exactly
            np.testing.assert_array_equal(got[:, 2], np.bincount(h["cell"][h["cell"] >= 0], minlength=ncell))
        for q, key in enumerate(("sum_margin", "sum_prob")):
            a_gpu, _ = B.ale_curve(got[:, q].reshape(shape), got[:, 2].reshape(shape))
            a_host, _ = B.ale_curve(h[key], h["weight"])
            raw, _ = B.ale_curve(h[key], h["weight"], centered=False)
            tol = 16 * err_e[q].sum() + 64 * ncell * 2.0 ** -53 * float(np.abs(raw).max())
            assert float(np.abs(a_gpu - a_host).max()) <= tol, (feats, key)
    return worst


def _chain(rng, specs):
    """A caterpillar given split by split: (feature, threshold, default_left, side on which the chain goes on)."""
    nodes = sf._Nodes()
    j = 0
    for f, thr, dl, side in specs:
        l, r = nodes.split(j, f, thr, dl)
        j = l if side == "l" else r
    return nodes.finish(rng)


# ------------------------------------------------------------------------- corner bit-identity
GRID = sf.THRESHOLD_GRID      # -1.5, 0, 0.25, 0.25 + 1 ulp, 1, 2.5: increasing, so it serves as the edges too
JOBS_1D = [(2,), (0,), (4,)]
EDGES_1D = [[GRID], [GRID[1:5]], [GRID[[0, 5]]]]             # K = 5, 3 and 1
JOBS_2D = [(0, 4), (3, 1)]
EDGES_2D = [[GRID, GRID[1:5]], [GRID[[0, 2, 5]], GRID]]       # 5 x 3 and 2 x 5: no square lattice


@functools.lru_cache(maxsize=None)
def _edge_case():
    """Splits on THRESHOLD_GRID, rows from edge_values() (every threshold, its neighbours, +-inf, NaN, +-0) and
    the same grid as the edges: splits sit exactly on edges and one ulp above. 257 rows and their references,
    shared by the row counts below (a row's corners depend on that row alone)."""
    rng = np.random.default_rng(11)
    F = 5
    b = sf.random_forest(rng, F, 8, 4, grid=GRID)
    X = sf.edge_rows(rng, 257, F)
    want1 = [_want(b, X, f, e) for f, e in zip(JOBS_1D, EDGES_1D)]
    want2 = [_want(b, X, f, e) for f, e in zip(JOBS_2D, EDGES_2D)]
    for wnt in want1 + want2:
        wnt.setflags(write=False)
    return b, X, want1, want2


@pytest.mark.parametrize("N", ROWS)
def test_corner_margins(N):
    b, X, want1, want2 = _edge_case()
    got = _check_corners(b, X[:N], JOBS_1D, EDGES_1D, f"1-D N={N}", want=[w[:, :N] for w in want1])
    if N > 1:
        assert (got[0][0] != got[0][1]).any()     # the feature matters: lo and hi differ somewhere
    _check_corners(b, X[:N], JOBS_2D, EDGES_2D, f"2-D N={N}", want=[w[:, :N] for w in want2])


def test_single_leaf_stumps():
    b = sf.make_booster([sf.stump(0.25), sf.stump(-0.5)], 3)
    X = _normal_rows(np.random.default_rng(12), 65, 3)
    z = np.array([-1.0, 0.0, 1.0], np.float32)
    got = _check_corners(b, X, [(1,)], [[z]], "stumps 1-D")
    assert len(np.unique(got)) == 1
    got = _check_corners(b, X, [(0, 2)], [[z, z]], "stumps 2-D")
    assert len(np.unique(got)) == 1


def test_feature_no_tree_uses():
    """lo = hi = the plain margin bits and every effect is exactly 0.0."""
    rng = np.random.default_rng(13)
    F = 5
    trees = [sf.random_tree(rng, F, 4, cols=[0, 2, 3, 4]) for _ in range(6)]
    assert all(1 not in sf.tree_features(t) for t in trees)
    b = sf.make_booster(trees, F)
    X = _normal_rows(rng, 257, F)
    z = np.array([-2.0, -0.3, 0.4, 2.0], np.float32)
    Xd = torch.from_numpy(X).cuda()
    plain = b.predict_margin(Xd).cpu().numpy()
    got = _check_corners(b, X, [(1,), (3,)], [[z], [z]], "unused 1-D")
    np.testing.assert_array_equal(got[0][0], plain)
    np.testing.assert_array_equal(got[0][1], plain)
    _, sums = _gpu(b, Xd, [(1,), (3,)], [[z], [z]], rows=False, sums=True)
    assert not sums[0, :, :2].any() and sums[0, :, 2].sum() == (~np.isnan(X[:, 1])).sum()
    assert sums[1, :, 0].any()
    got2 = _check_corners(b, X, [(1, 3)], [[z, z]], "unused x used")
    np.testing.assert_array_equal(got2[0][0], got2[0][1])    # moving the unused feature changes nothing
    np.testing.assert_array_equal(got2[0][2], got2[0][3])
    _, sums2 = _gpu(b, Xd, [(1, 3)], [[z, z]], rows=False, sums=True)
    assert not sums2[0, :, :2].any()


def test_repeated_splits_inside_one_interval():
    """Chains that split on feature 0 several times, with two (and three) thresholds inside the one interval
    (0, 0.5] and other features in between: lo = 0 and hi = 0.5 part at the first of them and part again, or
    meet again, at the next. A walk that forks at the first such node and then follows the row's own path on
    either branch gets these wrong."""
    rng = np.random.default_rng(14)
    F = 3
    trees = []
    for _ in range(6):
        sides = rng.choice(["l", "r"], size=5)
        thr = rng.uniform(0.05, 0.45, size=3)
        trees.append(_chain(rng, [(0, thr[0], 0, sides[0]), (1, 0.0, 1, sides[1]), (0, thr[1], 1, sides[2]),
                                  (2, 0.1, 0, sides[3]), (0, thr[2], 0, sides[4])]))
    trees.append(_chain(rng, [(0, 0.3, 0, "l"), (0, 0.1, 0, "r"), (0, 0.2, 0, "l")]))   # 0.1 <= x < 0.2 at the end
    b = sf.make_booster(trees, F)
    X = _normal_rows(rng, 257, F, nan=0.1)
    X[:128, 0] = rng.uniform(0.0, 0.5, size=128).astype(np.float32)     # many rows inside the interval
    z = np.array([-1.0, 0.0, 0.5, 1.0], np.float32)
    got = _check_corners(b, X, [(0,)], [[z]], "repeated splits 1-D")
    inside = (X[:, 0] > 0) & (X[:, 0] <= 0.5)
    assert (got[0][0][inside] != got[0][1][inside]).any()
    _check_corners(b, X, [(0, 1), (2, 0)], [[z, np.array([-0.5, 0.5], np.float32)], [z, z]], "repeated splits 2-D")


@pytest.mark.parametrize("default_left", [0, 1])
def test_default_directions_with_nan_in_other_features(default_left):
    rng = np.random.default_rng(15 + default_left)
    F = 6
    b = sf.random_forest(rng, F, 7, 4, default_left=default_left)
    X = _normal_rows(rng, 65, F, nan=0.3)
    z = np.array([-1.2, -0.4, 0.1, 0.9, 1.6], np.float32)
    _check_corners(b, X, [(f,) for f in range(F)], [[z]] * F, f"default_left={default_left} 1-D")
    _check_corners(b, X, [(0, 5), (3, 2)], [[z, z[1:]], [z[:3], z]], f"default_left={default_left} 2-D")


def test_forest_over_several_tiles(monkeypatch):
    monkeypatch.setattr(predict_ops, "TILE_NODES", 64)
    rng = np.random.default_rng(17)
    F = 7
    b = sf.make_booster([sf.grown_tree(rng, F, 5, 7) for _ in range(20)], F)     # 9 nodes a tree: 7 per tile
    tiles = np.diff(predict_ops.pack_forest(b)[2])
    assert predict_ops.tile_capacity(b) == 64 and len(tiles) >= 3, tiles
    X = _normal_rows(rng, 257, F)
    z = np.array([-1.0, -0.2, 0.5, 1.3], np.float32)
    _check_corners(b, X, [(4,), (0,)], [[z], [z[1:]]], "3 tiles 1-D")
    _check_corners(b, X, [(6, 2)], [[z, z[:3]]], "3 tiles 2-D")


def test_tree_prefixes():
    rng = np.random.default_rng(18)
    b = sf.random_forest(rng, 6, 7, 4)
    X = _normal_rows(rng, 65, 6)
    z = np.array([-1.0, 0.0, 1.0], np.float32)
    seen = [_check_corners(b, X, [(2,)], [[z]], f"n_trees={n}", n) for n in (1, 2, 5, 7, None)]
    np.testing.assert_array_equal(seen[-1], seen[-2])
    assert not np.array_equal(seen[0], seen[1])
    _check_corners(b, X, [(2, 4)], [[z, z]], "n_trees=3 2-D", 3)


# ---------------------------------------------------------------------------------- interval sums
@pytest.mark.parametrize("N", ROWS)
def test_interval_sums(N):
    """Margin and probability sums, weighted and not, several features with different K in one call (K = 1 among
    them), an interval no row lies in ((3, 50]) and a feature that is NaN in every row."""
    rng = np.random.default_rng(20 + N)
    F = 5
    b = sf.random_forest(rng, F, 6, 4)
    X = _normal_rows(rng, N, F, nan=0.1)
    X[:, 4] = np.nan
    X = np.clip(X, -2.9, 2.9)
    w = rng.uniform(0.0, 2.0, size=N).astype(np.float32)
    w[rng.random(N) < 0.1] = 0.0
    z = np.array([-1.5, -0.5, 0.0, 0.6, 3.0, 50.0], np.float32)
    jobs1 = [(0,), (2,), (4,), (1,)]
    edges1 = [[z], [z[[0, 5]]], [z], [z[1:4]]]
    jobs2 = [(0, 1), (3, 4), (2, 0)]
    edges2 = [[z, z[1:4]], [z[:3], z], [z[[0, 5]], z[[0, 5]]]]
    worst = 0.0
    for wt in (None, w):
        worst = max(worst, _check_sums(b, X, jobs1, edges1, wt), _check_sums(b, X, jobs2, edges2, wt))
    print(f"[ale] interval sums N={N}: largest |sum_gpu - sum_exact| / bound = {worst:.3g}")
    # the public sums: one- and two-feature jobs mixed, GPU against CPU, n_missing included
    g = predict_ops.accumulated_local_effects(b, X, jobs1 + jobs2, edges1 + edges2, weights=w, device="cuda")
    c = predict_ops.accumulated_local_effects(b, X, jobs1 + jobs2, edges1 + edges2, weights=w, device="cpu")
    for gj, cj in zip(g, c):
        assert gj["n_missing"] == cj["n_missing"] and gj["weight"].shape == cj["weight"].shape
        np.testing.assert_allclose(gj["weight"], cj["weight"], rtol=(N + 8) * U52, atol=0)
    assert g[2]["n_missing"] == N and not g[2]["weight"].any() and not g[2]["sum_prob"].any()


def test_determinism_and_untouched_input():
    rng = np.random.default_rng(30)
    F = 6
    b = sf.random_forest(rng, F, 9, 4)
    X = _normal_rows(rng, 1000, F)
    Xd = torch.from_numpy(X).cuda()
    w = torch.from_numpy(rng.uniform(0, 1, size=1000).astype(np.float32)).cuda()
    z = np.array([-1.0, -0.3, 0.2, 0.8, 1.5], np.float32)
    for jobs, edges in (([(5,), (2,)], [[z], [z[1:]]]), ([(5, 2)], [[z, z]])):
        a = _gpu(b, Xd, jobs, edges, w=w, sums=True)
        c = _gpu(b, Xd, jobs, edges, w=w, sums=True)
        assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()
    assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True)


def test_chunking():
    """One row chunk and 65 rows of the next: `order` holds chunk-local indices and the chunk sums are added in
    chunk order. The only larger shape; 3 small trees keep the host side in seconds."""
    N = int(_native.lib().cobalt_ale_chunk_rows()) + 65
    rng = np.random.default_rng(31)
    F = 3
    b = sf.random_forest(rng, F, 3, 3)
    X = _normal_rows(rng, N, F, nan=0.02)
    w = rng.uniform(0.0, 2.0, size=N).astype(np.float32)
    z = np.array([-1.0, -0.2, 0.3, 1.1], np.float32)
    worst = max(_check_sums(b, X, [(1,), (0,)], [[z], [z[1:]]], w), _check_sums(b, X, [(2, 0)], [[z, z[:3]]], None))
    print(f"[ale] chunking N={N}: largest |sum_gpu - sum_exact| / bound = {worst:.3g}")


def test_workspace_and_limits():
    lib = _native.lib()
    chunk = int(lib.cobalt_ale_chunk_rows())
    assert lib.cobalt_ale_workspace(65, 3, 1) == 3 * 2 * 65 * 4
    assert lib.cobalt_ale_workspace(1 << 24, 3, 2) == lib.cobalt_ale_workspace(chunk, 3, 2) == 3 * 4 * chunk * 4
    assert lib.cobalt_ale_max_intervals() == predict_ops.ALE_MAX_INTERVALS
    assert lib.cobalt_ale_max_cells() == predict_ops.ALE_MAX_CELLS
    assert lib.cobalt_ale_max_jobs() == predict_ops.ALE_MAX_JOBS


# ---------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch():
    rng = np.random.default_rng(40)
    b = sf.random_forest(rng, 6, 3, 3)
    z = np.array([0.0, 1.0, 2.0], np.float32)
    Xd = torch.zeros((8, 6), dtype=torch.float32, device="cuda")
    kw = dict(want_rows=True, want_sums=True)
    with pytest.raises(ValueError, match="features"):
        predict_ops.accumulated_local_effects_gpu(b, Xd[:, :5], [(0,)], [[z]], **kw)          # narrow X
    with pytest.raises(ValueError, match="float32"):
        predict_ops.accumulated_local_effects_gpu(b, Xd.double(), [(0,)], [[z]], **kw)
    with pytest.raises(ValueError, match="differ"):
        predict_ops.accumulated_local_effects_gpu(b, Xd, [(2, 2)], [[z, z]], **kw)
    with pytest.raises(ValueError, match="outside"):
        predict_ops.accumulated_local_effects_gpu(b, Xd, [(6,)], [[z]], **kw)
    for bad in (z[::-1].copy(), np.array([0.0, 0.0, 1.0], np.float32), np.array([0.0], np.float32),
                np.array([0.0, np.nan], np.float32), np.array([0.0, np.inf], np.float32)):
        with pytest.raises(ValueError, match="edges"):
            predict_ops.accumulated_local_effects_gpu(b, Xd, [(0,)], [[bad]], **kw)
    with pytest.raises(ValueError):
        predict_ops.accumulated_local_effects_gpu(b, Xd, [(0,), (1, 2)], [[z], [z, z]], **kw)  # kinds mixed in one launch
    with pytest.raises(ValueError, match="weights"):
        predict_ops.accumulated_local_effects_gpu(b, Xd, [(0,)], [[z]], weights=torch.ones(7, device="cuda"), **kw)
    with pytest.raises(ValueError):
        b.accumulated_local_effects(Xd, (1, 1))
    with pytest.raises(ValueError):
        b.accumulated_local_effects(Xd, 0, grid=[1.0, 0.5])
    # a footprint beyond the LDS limit: 2048 * 8 + 256 * (144 | 1) * 4 bytes > 160 KiB
    wide = sf.random_forest(rng, 144, 2, 3)
    with pytest.raises(RuntimeError, match="code -3"):
        predict_ops.accumulated_local_effects_gpu(wide, torch.zeros((4, 144), dtype=torch.float32, device="cuda"),
                                                  [(0,)], [[z]], **kw)
    # the entry point itself refuses what the wrapper checks first; nothing is launched
    lib = _native.lib()
    gf = predict_ops.gpu_forest(b, Xd.device)
    ed = torch.from_numpy(np.concatenate([z, z])).cuda()
    rows = torch.full((1, 4, 8), 7.0, dtype=torch.float32, device="cuda")
    sums = torch.full((1, 4, 3), 7.0, dtype=torch.float64, device="cuda")
    order = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    seg = torch.zeros((1, 1, 5), dtype=torch.int32, device="cuda")
    work = torch.empty(int(lib.cobalt_ale_workspace(8, 1, 2)), dtype=torch.uint8, device="cuda")

    def call(desc, dims, tile_cap=gf.tile_cap, F=6, rows_p=rows.data_ptr(), work_p=work.data_ptr(),
             sums_p=sums.data_ptr(), n_edges=6):
        d = np.asarray([desc], dtype=np.int32)
        jd = torch.from_numpy(d).cuda()
        return lib.cobalt_ale(Xd.data_ptr(), 8, F, F, gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(),
                              gf.tile_ptr.data_ptr(), gf.n_tiles, tile_cap, 0.0, d.ctypes.data, jd.data_ptr(), 1, dims,
                              ed.data_ptr(), n_edges, None, order.data_ptr(), seg.data_ptr(), 4, rows_p, work_p,
                              sums_p, _native.stream_handle())

    ok1, ok2 = (0, -1, 0, 2, 0, 1), (0, 1, 0, 2, 3, 2)
    assert call(ok1, 1, tile_cap=8193) == -2 and call(ok2, 2, tile_cap=0) == -2
    assert call(ok1, 1, F=20000) == -3
    assert call(ok1, 1, rows_p=None, work_p=None) == -7
    assert call((6, -1, 0, 2, 0, 1), 1) == -8            # feature out of range
    assert call((-1, -1, 0, 2, 0, 1), 1) == -8
    assert call((2, 2, 0, 2, 3, 2), 2) == -8             # f1 == f2
    assert call((0, 6, 0, 2, 3, 2), 2) == -8
    assert call((0, -1, 0, 0, 0, 1), 1) == -8            # an empty edge list: no interval
    assert call((0, 1, 0, 2, 3, 0), 2) == -8
    assert call((0, -1, 0, 4097, 0, 1), 1, n_edges=5000) == -8   # too many intervals
    assert call((0, -1, 4, 2, 0, 1), 1) == -8            # edges past the end of the array
    assert call(ok2, 1) == -8 and call(ok1, 2) == -8     # a pair in a one-feature call and the reverse
    assert call(ok1, 3) == -8
    torch.cuda.synchronize()
    assert bool((rows == 7.0).all()) and bool((sums == 7.0).all())  # nothing was launched


# ------------------------------------------------------------------------ fitted model, end to end
def test_public_path_on_an_early_stopped_classifier():
    import pandas as pd

    rng = np.random.default_rng(50)
    n, F = 1200, 4
    X = rng.normal(size=(n, F)).astype(np.float32)
    X[:, 1] = (0.9 * X[:, 0] + 0.1 * X[:, 1]).astype(np.float32)         # correlated, as the feature is for
    X[rng.random(X.shape) < 0.03] = np.nan
    Z = np.nan_to_num(X)
    y = (Z[:, 0] - 0.8 * Z[:, 2] + 0.6 * Z[:, 2] * Z[:, 3] + 0.5 * rng.normal(size=n) > 0).astype(np.float32)
    names = ["a", "b", "c", "d"]
    df = pd.DataFrame(X, columns=names)
    clf = gbdt.GBDTClassifier(n_estimators=40, max_depth=3, learning_rate=0.5, early_stopping_rounds=3,
                              eval_metric="logloss", device="cuda")
    clf.fit(df[:800], y[:800], eval_set=[(df[800:], y[800:])])
    b = clf.get_booster()
    used = b.best_iteration + 1
    assert used < b.num_trees, "the fit must stop early for this test to mean anything"
    shuffled = df[800:][["d", "b", "a", "c"]]                            # columns in another order
    res = explain.accumulated_local_effects(clf, shuffled)
    assert [r["feature_names"] for r in res] == [[nm] for nm in names]
    want = b.accumulated_local_effects(X[800:], n_trees=used, device="cpu")
    full = b.accumulated_local_effects(X[800:], device="cpu")
    assert any(not np.allclose(w_["ale"], f_["ale"], rtol=0, atol=1e-9) for w_, f_ in zip(want, full))
    for r, w_ in zip(res, want):
        np.testing.assert_array_equal(r["edges"][0], w_["edges"][0])
        np.testing.assert_array_equal(r["interval_weight"], w_["interval_weight"])   # unweighted: row counts
        assert r["n_missing"] == w_["n_missing"]
        # the module's curve bound with probabilities in [0, 1]: an interval sum errs by at most (n + 8) 2^-52 * 2 n,
        # its mean by that over n plus |e| (n + 8) 2^-52 with |e| <= 1: d_k <= 3 (n_k + 8) 2^-52
        tol = 16 * float((3 * (r["interval_weight"] + 8) * U52).sum()) + 64 * len(r["ale"]) * 2.0 ** -53
        assert float(np.abs(r["ale"] - w_["ale"]).max()) <= tol
    pair = explain.accumulated_local_effects(clf, shuffled, ("a", "c"), grid_resolution=5, response="margin",
                                             iteration_range=(0, 4))
    assert pair["feature_names"] == ["a", "c"] and pair["ale"].shape == (6, 6)
    pw = b.accumulated_local_effects(X[800:], (0, 2), grid_resolution=5, response="margin", n_trees=4, device="cpu")
    # the same bound in margin units: every row's effect is at most E, so d_k <= 2 (n_k + 8) 2^-52 E
    h = B.ale_host(b, X[800:], (0, 2), pw["edges"], 4)
    m = h["corners"].astype(np.float64)
    E = float(np.abs((m[3] - m[2]) - (m[1] - m[0])).max())
    tol = 16 * float((2 * (pw["interval_weight"] + 8) * U52 * E).sum()) + 64 * 36 * 2.0 ** -53 * 25 * E
    assert float(np.abs(pair["ale"] - pw["ale"]).max()) <= tol
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    for shown in (res[0], pair, res):
        fig = explain.ale_plot(shown)
        assert hasattr(fig, "savefig")
        plt.close(fig)
