"""The partial-dependence / ICE kernel (csrc/pdp.hip, walk of csrc/pdp_walk.h) on the hand-built forests of
scoring_forests.py and on small fitted models.

ICE margins: bit for bit against ``scoring_forests.predict_rowwise`` (one row at a time, independent of the
kernel and of ``predict_margin_host``) on explicitly substituted copies of X.

Averages: ``|avg_gpu - avg_exact| <= (N + 8) * 2^-52 * sum w|t| / sum w`` where ``avg_exact`` is the
``math.fsum`` mean of the GPU's own ICE margins (or of the float64 probabilities computed from them) and ``t``
the term being averaged: the standard bound ``(N - 1) u sum|x_i|`` (u = 2^-53) of a floating-point sum of N
terms in any order, once for the numerator and once for ``sum w``, plus a few ulp for ``exp``. Derived, not
measured; each test prints the largest ratio to the bound it saw as ``[pdp] ...``.

Which test catches which mistake in the kernel:
  ``<=`` instead of ``<`` in the walk ........ test_value_edges (grid and row values exactly on the thresholds)
  transposed ``i1 * G2 + i2`` ................ test_two_feature_grids (3 x 5, 3 x 7, 5 x 7: none is square)
  override at ``r * F + f`` (even F) ......... test_widths (F = 2, 8, 80 have F | 1 != F)
  a dropped grid-chunk tail .................. test_rows_and_grid_sizes (G = chunk +- 1, 2 chunk + 1), test_two_feature_grids
  tail lanes contributing weight ............. test_averages (N = 65, 257 unweighted), test_tail_lanes_have_no_weight
  sigmoid of the mean ........................ test_averages (the probability term is the mean of sigmoids)
  "tree ignores f" with the wrong feature .... the kernel has no such shortcut; test_feature_used_by_every_tree_and_by_none
                                               would catch one (a feature every tree uses next to one none uses)
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


# ------------------------------------------------------------------------------------ helpers
def _chunk() -> int:
    return int(_native.lib().cobalt_pdp_grid_chunk())


def _substituted(X, feats, grids):
    """[G * N, F]: the copies of X for the grid points k = i1 * G2 + i2, one after the other."""
    out = []
    pts = [(a, None) for a in grids[0]] if len(feats) == 1 else [(a, c) for a in grids[0] for c in grids[1]]
    for a, c in pts:
        Xs = np.array(X, np.float32)
        Xs[:, feats[0]] = a
        if c is not None:
            Xs[:, feats[1]] = c
        out.append(Xs)
    return np.concatenate(out), len(pts)


def _want(b, X, feats, grids, n_trees=None):
    Xs, G = _substituted(X, feats, grids)
    return sf.predict_rowwise(b, Xs, n_trees).reshape(G, X.shape[0])


def _gpu(b, Xd, feats, grids, n_trees=None, w=None, ice=True, avg=False):
    i, s = predict_ops.partial_dependence_gpu(b, Xd, feats, grids, n_trees=n_trees, weights=w, want_ice=ice,
                                              want_avg=avg)
    return (None if i is None else i.cpu().numpy()), (None if s is None else s.cpu().numpy())


def _check_ice(b, X, feats, grids, label, n_trees=None):
    X = np.ascontiguousarray(X, np.float32)
    Xd = torch.from_numpy(X).cuda()
    got, _ = _gpu(b, Xd, feats, grids, n_trees)
    want = _want(b, X, feats, grids, n_trees)
    assert got.dtype == np.float32 and got.shape == want.shape, (label, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=label)
    assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True), label  # X is never written
    return got


def _normal_rows(rng, n, F, nan=0.05):
    X = rng.normal(size=(n, F)).astype(np.float32)
    X[rng.random(X.shape) < nan] = np.nan
    return X


def _numeric_grid(rng, G):
    g = rng.normal(size=G).astype(np.float32)
    if G > 2:
        g[G // 2] = np.nan  # the "missing" point, inside the grid
    return g


def _avg_ratio(ice, sums, w):
    """Asserts the averaging bound for every grid point (margin and probability); returns the largest
    |error| / bound."""
    G, N = ice.shape
    wd = np.ones(N) if w is None else np.asarray(w, np.float32).astype(np.float64)
    sw = math.fsum(wd)
    assert abs(sums[-1] - sw) <= (N + 8) * 2.0 ** -52 * sw
    worst = 0.0
    for k in range(G):
        m = ice[k].astype(np.float64)
        p = 1.0 / (1.0 + np.exp(-m))
        for t, num in ((m, sums[2 * k]), (p, sums[2 * k + 1])):
            exact = math.fsum(wd * t) / sw
            bound = (N + 8) * 2.0 ** -52 * math.fsum(wd * np.abs(t)) / sw
            err = abs(num / sums[-1] - exact)
            assert err <= bound, (k, err, bound)
            worst = max(worst, err / bound if bound > 0 else 0.0)
    return worst


# ------------------------------------------------------------------------------ ICE bit-identity
@functools.lru_cache(maxsize=None)
def _rows_case():
    """One forest, 513 rows and a (2 chunk + 1)-point grid with their reference, shared by the row / grid
    sizes below (grid point k of a 1-D grid depends on grid[k] only: a shorter grid is a prefix)."""
    rng = np.random.default_rng(11)
    F = 7
    b = sf.random_forest(rng, F, 6, 3)
    X = _normal_rows(rng, 513, F)
    grid = _numeric_grid(rng, 2 * _chunk() + 1)
    want = _want(b, X, (3,), [grid])
    want.setflags(write=False)
    return b, X, grid, want


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 513])
def test_rows_and_grid_sizes(N):
    b, X, grid, want = _rows_case()
    c = _chunk()
    Xd = torch.from_numpy(X[:N].copy()).cuda()
    for G in (1, c - 1, c, c + 1, 2 * c + 1):
        got, _ = _gpu(b, Xd, (3,), [grid[:G]])
        assert got.shape == (G, N)
        np.testing.assert_array_equal(got, want[:G, :N], err_msg=f"N={N} G={G}")


@pytest.mark.parametrize("shape", [(3, 5), (3, 7), (5, 7)])
def test_two_feature_grids(shape):
    """3 x 5 fits one grid chunk, 3 x 7 = 21 crosses one chunk boundary and 5 x 7 = 35 two (chunk 16); no grid is
    square, so a transposed i1 * G2 + i2 moves values."""
    rng = np.random.default_rng(12 + shape[0] + shape[1])
    F = 6
    b = sf.random_forest(rng, F, 8, 4)
    X = _normal_rows(rng, 257, F)
    _check_ice(b, X, (4, 1), [_numeric_grid(rng, shape[0]), _numeric_grid(rng, shape[1])], f"2-D {shape}")


@pytest.mark.parametrize("F", [1, 2, 7, 8, 80])
def test_widths(F):
    """Even and odd F | 1 (the staged row stride); F = 80 needs more than 64 KiB of LDS (2048 * 8 + 256 * 81 * 4
    bytes). The overridden feature is the last one (for F = 1 the only one); with two features, the last and
    the first."""
    rng = np.random.default_rng(20 + F)
    b = sf.random_forest(rng, F, 10, 4)
    X = _normal_rows(rng, 65, F)
    _check_ice(b, X, (F - 1,), [_numeric_grid(rng, _chunk() + 1)], f"F={F} 1-D")
    if F > 1:
        _check_ice(b, X, (F - 1, 0), [_numeric_grid(rng, 3), _numeric_grid(rng, 5)], f"F={F} 2-D")
        _check_ice(b, X, (0,), [_numeric_grid(rng, 4)], f"F={F} first")


def test_stumps_only():
    b = sf.make_booster([sf.stump(0.25), sf.stump(-0.5), sf.stump(0.125)], 3)
    X = _normal_rows(np.random.default_rng(30), 70, 3)
    got = _check_ice(b, X, (1,), [np.array([0.0, np.nan, 1.0], np.float32)], "stumps")
    assert len(np.unique(got)) == 1


# leaves per tree -> trees per 64-node tile (2 * leaves - 1 nodes each), as test_gpu_scoring_edges.py
_TILE_CASES = {1: 32, 2: 16, 3: 11, 4: 8, 5: 6, 9: 4}


@pytest.mark.parametrize("per_tile", sorted(_TILE_CASES))
def test_tile_populations(per_tile, monkeypatch):
    """Tiles of 1, 2, 3, 4, 5 and 9 trees (64-node tiles), at least three tiles, a smaller last one."""
    monkeypatch.setattr(predict_ops, "TILE_NODES", 64)
    rng = np.random.default_rng(40 + per_tile)
    F = 9
    n_trees = 2 * per_tile + max(1, per_tile - 2)
    b = sf.make_booster([sf.grown_tree(rng, F, _TILE_CASES[per_tile], 7) for _ in range(n_trees)], F)
    tiles = np.diff(predict_ops.pack_forest(b)[2])
    assert predict_ops.tile_capacity(b) == 64 and list(tiles[:2]) == [per_tile, per_tile] and len(tiles) >= 3, tiles
    X = _normal_rows(rng, 130, F)
    _check_ice(b, X, (4,), [_numeric_grid(rng, _chunk() + 1)], f"{per_tile} trees per tile")
    _check_ice(b, X, (8, 2), [_numeric_grid(rng, 3), _numeric_grid(rng, 2)], f"{per_tile} trees per tile, 2-D")


def test_feature_used_by_every_tree_and_by_none():
    rng = np.random.default_rng(50)
    F = 5
    trees = [sf.random_tree(rng, F, 4, cols=[3]) for _ in range(4)]        # split on feature 3 only
    trees += [sf.caterpillar(rng, 4, [0, 2, 3, 4]) for _ in range(5)]      # a chain over 0, 2, 3, 4: never 1
    for t in trees:
        used = set(sf.tree_features(t))
        assert 3 in used and 1 not in used
    b = sf.make_booster(trees, F)
    X = _normal_rows(rng, 100, F)
    grid = _numeric_grid(rng, 9)
    every = _check_ice(b, X, (3,), [grid], "feature of every tree")
    assert len(np.unique(every, axis=0)) > 1
    none = _check_ice(b, X, (1,), [grid], "feature of no tree")
    plain = b.predict_margin(torch.from_numpy(X).cuda()).cpu().numpy()
    for k in range(len(grid)):
        np.testing.assert_array_equal(none[k], plain)
    both = _check_ice(b, X, (1, 3), [grid[:3], grid], "unused x used")
    np.testing.assert_array_equal(both.reshape(3, 9, -1)[0], every)
    _check_ice(b, X, (3, 1), [grid, grid[:3]], "used x unused")


def test_tree_prefixes():
    rng = np.random.default_rng(60)
    b = sf.random_forest(rng, 6, 7, 4)
    X = _normal_rows(rng, 90, 6)
    grid = _numeric_grid(rng, 5)
    seen = []
    for n_trees in (1, 2, 5, 7, None):
        seen.append(_check_ice(b, X, (2,), [grid], f"n_trees={n_trees}", n_trees))
    np.testing.assert_array_equal(seen[-1], seen[-2])
    assert not np.array_equal(seen[0], seen[1])


def test_row_strided_input():
    rng = np.random.default_rng(70)
    F = 7
    b = sf.random_forest(rng, F, 6, 4)
    wide = _normal_rows(rng, 300, F + 5)
    Xd = torch.from_numpy(wide).cuda()[:, :F]
    assert Xd.stride(0) == F + 5 and not Xd.is_contiguous()
    grid = _numeric_grid(rng, _chunk() + 2)
    got, sums = _gpu(b, Xd, (6,), [grid], avg=True)
    np.testing.assert_array_equal(got, _want(b, wide[:, :F], (6,), [grid]))
    _avg_ratio(got, sums, None)
    # a matrix wider than the model: the extra columns are ignored
    got2, _ = _gpu(b, torch.from_numpy(wide).cuda(), (6,), [grid])
    np.testing.assert_array_equal(got2, got)


def test_value_edges():
    """Rows drawn from edge_values() (every threshold, its neighbours, +-inf, NaN, +-0, denormals) in the
    columns that stay, and the same values (NaN among them) as the grid: a value equal to a threshold goes
    right, NaN takes the default direction."""
    rng = np.random.default_rng(80)
    F = 5
    b = sf.random_forest(rng, F, 10, 4, grid=sf.THRESHOLD_GRID)
    X = sf.edge_rows(rng, 70, F)
    grid = sf.edge_values()
    assert np.isnan(grid).any() and np.isinf(grid).any()
    got = _check_ice(b, X, (2,), [grid], "edge values 1-D")
    assert len(np.unique(got, axis=0)) > 3
    _check_ice(b, X, (0, 4), [grid[:9], np.array([np.nan, 0.25, -0.0, np.inf], np.float32)], "edge values 2-D")


# ---------------------------------------------------------------------------------- averages
def test_averages():
    chunk_rows = int(_native.lib().cobalt_pdp_chunk_rows())
    rng = np.random.default_rng(90)
    F = 4
    b = sf.random_forest(rng, F, 3, 3)
    worst = 0.0
    for N in (65, 257, 2 * chunk_rows + 3):
        X = _normal_rows(rng, N, F)
        Xd = torch.from_numpy(X).cuda()
        w = rng.uniform(0.0, 2.0, size=N).astype(np.float32)
        w[rng.random(N) < 0.1] = 0.0
        for feats, grids in (((1,), [np.array([-0.5, np.nan, 0.7], np.float32)]),
                             ((2, 0), [np.array([0.1, -1.0], np.float32), np.array([np.nan, 0.3], np.float32)])):
            for wt in (None, w):
                ice, sums = _gpu(b, Xd, feats, grids, w=None if wt is None else torch.from_numpy(wt).cuda(),
                                 avg=True)
                worst = max(worst, _avg_ratio(ice, sums, wt))
                only, _ = _gpu(b, Xd, feats, grids)
                np.testing.assert_array_equal(only, ice)  # the ICE-only kernel gives the same margins
                _, alone = _gpu(b, Xd, feats, grids, w=None if wt is None else torch.from_numpy(wt).cuda(),
                                ice=False, avg=True)
                np.testing.assert_array_equal(alone, sums)
        if N == 65:  # the margins behind the averages are the right ones
            np.testing.assert_array_equal(ice, _want(b, X, feats, grids))
    print(f"[pdp] averages: largest |avg_gpu - avg_exact| / bound = {worst:.3g}")


def test_tail_lanes_have_no_weight():
    """65 rows against the same 65 rows padded to 128 with zero weights: same sums, bit for bit (the last
    block's lanes past n enter the wave sums as 0.0, like a zero-weight row)."""
    rng = np.random.default_rng(91)
    F = 4
    b = sf.random_forest(rng, F, 5, 3)
    X = _normal_rows(rng, 128, F)
    w = rng.uniform(0.5, 2.0, size=128).astype(np.float32)
    w[65:] = 0.0
    grid = [np.array([-1.0, 0.0, np.nan, 1.0], np.float32)]
    Xd, wd = torch.from_numpy(X).cuda(), torch.from_numpy(w).cuda()
    _, short = _gpu(b, Xd[:65], (3,), grid, w=wd[:65].contiguous(), avg=True)
    _, padded = _gpu(b, Xd, (3,), grid, w=wd, avg=True)
    np.testing.assert_array_equal(short, padded)
    _, ones = _gpu(b, Xd[:65], (3,), grid, w=torch.ones(65, device="cuda"), avg=True)
    _, unweighted = _gpu(b, Xd[:65], (3,), grid, avg=True)
    np.testing.assert_array_equal(ones, unweighted)
    assert unweighted[-1] == 65.0


def test_determinism_and_untouched_input():
    rng = np.random.default_rng(92)
    F = 6
    b = sf.random_forest(rng, F, 9, 4)
    X = _normal_rows(rng, 1000, F)
    Xd = torch.from_numpy(X).cuda()
    w = torch.from_numpy(rng.uniform(0, 1, size=1000).astype(np.float32)).cuda()
    grids = [_numeric_grid(rng, 5), _numeric_grid(rng, 7)]
    a = _gpu(b, Xd, (5, 2), grids, w=w, avg=True)
    c = _gpu(b, Xd, (5, 2), grids, w=w, avg=True)
    assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()
    assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True)


def test_workspace_is_bounded():
    lib = _native.lib()
    chunk_rows = int(lib.cobalt_pdp_chunk_rows())
    assert lib.cobalt_pdp_workspace(1, 5) == (5 * 4 * 2 + 4) * 8
    assert lib.cobalt_pdp_workspace(1 << 24, 100) == lib.cobalt_pdp_workspace(chunk_rows, 100)
    assert lib.cobalt_pdp_workspace(chunk_rows, 100) == (100 * 2 + 1) * (chunk_rows // 64) * 8


# ------------------------------------------------------------------------ fitted models, end to end
def _data(seed=0, n=2000, F=4):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)).astype(np.float32)
    X[rng.random(X.shape) < 0.05] = np.nan
    Z = np.nan_to_num(X)
    y = (Z[:, 0] - 0.8 * Z[:, 1] + 0.6 * Z[:, 2] * Z[:, 3] + 0.4 * Z[:, 0] * Z[:, 1]
         + 0.5 * rng.normal(size=n) > 0).astype(np.float32)
    return X, y


def _fit(X, y, **extra):
    p = dict(n_estimators=20, max_depth=4, learning_rate=0.3, **extra)
    return gbdt.train(torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda(), p, device="cuda")


def test_gpu_dict_equals_cpu_dict():
    X, y = _data(1)
    b = _fit(X, y)
    assert b.num_trees == 20
    N = X.shape[0]
    w = np.random.default_rng(2).uniform(0.5, 1.5, size=N).astype(np.float32)
    worst = 0.0
    for features, kw in ((0, dict(grid_resolution=12, include_missing=True)),
                         ((2, 3), dict(grid_resolution=5, sample_weight=w)),
                         (1, dict(grid_resolution=9, n_trees=7))):
        for response in ("probability", "margin"):
            g = b.partial_dependence(torch.from_numpy(X).cuda(), features, kind="both", response=response, **kw)
            c = b.partial_dependence(X, features, kind="both", response=response, device="cpu", **kw)
            assert g["feature_names"] == c["feature_names"]
            for ga, ca in zip(g["grid_values"], c["grid_values"]):
                np.testing.assert_array_equal(ga, ca)
            np.testing.assert_array_equal(g["individual"], c["individual"])
            assert g["average"].shape == c["average"].shape and g["average"].dtype == np.float64
            # the CPU path's averages are math.fsum means of the same margins: the exact value of the bound
            gm = b.partial_dependence(X, features, kind="individual", response="margin", device="cpu", **kw)
            t = gm["individual"].astype(np.float64).reshape(N, -1)
            if response == "probability":
                t = 1.0 / (1.0 + np.exp(-t))
            wd = kw.get("sample_weight", np.ones(N, np.float32)).astype(np.float64)
            bound = (N + 8) * 2.0 ** -52 * (wd[:, None] * np.abs(t)).sum(0) / wd.sum()
            err = np.abs(g["average"].reshape(-1) - c["average"].reshape(-1))
            assert (err <= bound).all(), (features, response, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
    print(f"[pdp] GPU dict against CPU dict: largest |average difference| / bound = {worst:.3g}")
    # numpy in, numpy out on the GPU too; the classifier front end agrees
    r = b.partial_dependence(X, 0, grid_resolution=6, device="cuda")
    np.testing.assert_array_equal(
        r["average"], b.partial_dependence(torch.from_numpy(X).cuda(), 0, grid_resolution=6)["average"])


def test_monotone_fit_has_monotone_ice_curves():
    """monotone_constraints +1 / -1: every row's ICE margin curve over an increasing numeric grid is
    non-decreasing / non-increasing, exactly: each tree's leaf is monotone in the feature and fp32 addition is
    monotone, so the sums in tree order are. The NaN point is left out."""
    X, y = _data(3)
    b = _fit(X, y, monotone_constraints=(1, -1, 0, 0))
    Xd = torch.from_numpy(X).cuda()
    used = set()
    for t in b.trees:
        used |= set(sf.tree_features(t))
    assert {0, 1} <= used
    for f, sign in ((0, 1), (1, -1)):
        r = b.partial_dependence(Xd, f, grid_resolution=40, percentiles=(0.0, 1.0), include_missing=True,
                                 kind="both", response="margin")
        g = r["grid_values"][0]
        assert np.isnan(g[-1]) and (np.diff(g[:-1]) > 0).all()
        d = np.diff(r["individual"][:, :-1], axis=1) * sign
        assert (d >= 0).all(), (f, float(d.min()))
        assert (d > 0).any()
        assert (np.diff(r["average"][:-1]) * sign >= 0).all()
    free = b.partial_dependence(Xd, 2, grid_resolution=40, kind="individual", response="margin")["individual"]
    d = np.diff(free, axis=1)
    assert (d > 0).any() and (d < 0).any()  # an unconstrained feature goes both ways: the check above can fail


def test_interaction_constrained_fit_is_additive_across_groups():
    """interaction_constraints [[0, 1], [2, 3]]: PD02[a, b] - PD0[a] - PD2[b] + mean margin = 0 up to
    16 * (N + 8) * 2^-52 * mean|margin|.

    Checked on float64 sums of per-tree contributions: every tree is scored alone by the kernel (its margins
    are its leaf values, exact in fp32; base margin 0), the kernel averages them, and the trees' averages are
    added in float64. The fp32 margins of the whole forest are not exactly additive (each row's sum in tree
    order rounds ~20 times at 2^-24 relative, ~1e-7, against a tolerance of ~1e-11); their residual is printed
    next to the float64 one."""
    groups = [[0, 1], [2, 3]]
    X, y = _data(4)
    b = _fit(X, y, interaction_constraints=groups)
    N = X.shape[0]
    sides = set()
    for t in b.trees:
        used = set(sf.tree_features(t))
        assert used <= {0, 1} or used <= {2, 3}, used
        sides |= {0} if used & {0, 1} else ({1} if used else set())
    assert sides == {0, 1}  # both groups are in the model
    Xd = torch.from_numpy(X).cuda()
    ga = np.linspace(-1.5, 1.5, 6).astype(np.float32)
    gb = np.array([-1.0, 0.0, np.nan, 0.5, 1.2], np.float32)

    def avg_margin(model, feats, grids):
        _, s = _gpu(model, Xd, feats, grids, ice=False, avg=True)
        return s[0:-1:2] / s[-1]

    margins = b.predict_margin(Xd).cpu().numpy().astype(np.float64)
    tol = 16 * (N + 8) * 2.0 ** -52 * float(np.abs(margins).mean())
    pd02 = np.zeros((6, 5))
    pd0 = np.zeros(6)
    pd2 = np.zeros(5)
    mean = 0.0
    for t in b.trees:
        one = B.Booster([t], num_feature=b.num_feature, base_score=0.5)
        assert one.base_margin == 0.0
        pd02 += avg_margin(one, (0, 2), [ga, gb]).reshape(6, 5)
        pd0 += avg_margin(one, (0,), [ga])
        pd2 += avg_margin(one, (2,), [gb])
        mean += math.fsum(one.predict_margin(Xd).cpu().numpy().astype(np.float64)) / N
    resid64 = float(np.abs(pd02 - pd0[:, None] - pd2[None, :] + mean).max())
    whole = (avg_margin(b, (0, 2), [ga, gb]).reshape(6, 5) - avg_margin(b, (0,), [ga])[:, None]
             - avg_margin(b, (2,), [gb])[None, :] + math.fsum(margins) / N)
    print(f"[pdp] additivity residual: float64 per-tree sums {resid64:.3g} (tolerance {tol:.3g}); "
          f"fp32 forest margins {float(np.abs(whole).max()):.3g}")
    assert resid64 <= tol, (resid64, tol)
    # the same pair inside one group does interact
    inside = (avg_margin(b, (0, 1), [ga, ga]).reshape(6, 6) - avg_margin(b, (0,), [ga])[:, None]
              - avg_margin(b, (1,), [ga])[None, :] + math.fsum(margins) / N)
    assert float(np.abs(inside).max()) > 1e-3


def test_explain_front_end_on_the_gpu():
    X, y = _data(5, n=600)
    clf = gbdt.GBDTClassifier(n_estimators=8, max_depth=3, learning_rate=0.3, device="cuda").fit(X, y)
    r = explain.partial_dependence(clf, X, (0, 1), grid_resolution=4, kind="both", iteration_range=(0, 5))
    want = clf.get_booster().partial_dependence(X, (0, 1), grid_resolution=4, kind="both", n_trees=5, device="cpu")
    np.testing.assert_array_equal(r["individual"], want["individual"])
    Xs = X.copy()
    Xs[:, 0], Xs[:, 1] = r["grid_values"][0][1], r["grid_values"][1][3]
    np.testing.assert_allclose(r["individual"][:, 1, 3], clf.predict_proba(Xs, iteration_range=(0, 5))[:, 1],
                               rtol=0, atol=2e-7)


# ---------------------------------------------------------------------------------- refusals
def test_refusals_before_any_launch():
    rng = np.random.default_rng(100)
    b = sf.random_forest(rng, 6, 3, 3)
    grid = [np.array([0.0, 1.0], np.float32)]
    Xd = torch.zeros((8, 6), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="features"):
        predict_ops.partial_dependence_gpu(b, Xd[:, :5], (0,), grid, want_ice=True, want_avg=True)   # narrow X
    with pytest.raises(ValueError, match="float32"):
        predict_ops.partial_dependence_gpu(b, Xd.double(), (0,), grid, want_ice=True, want_avg=True)
    with pytest.raises(ValueError, match="differ"):
        predict_ops.partial_dependence_gpu(b, Xd, (2, 2), grid * 2, want_ice=True, want_avg=True)
    with pytest.raises(ValueError):
        predict_ops.partial_dependence_gpu(b, Xd, (6,), grid, want_ice=True, want_avg=True)
    with pytest.raises(ValueError):
        predict_ops.partial_dependence_gpu(b, Xd, (0,), [np.zeros(0, np.float32)], want_ice=True, want_avg=True)
    with pytest.raises(ValueError, match="weights"):
        predict_ops.partial_dependence_gpu(b, Xd, (0,), grid, weights=torch.ones(7, device="cuda"), want_ice=False,
                                           want_avg=True)
    # a footprint beyond the LDS limit: 2048 * 8 + 256 * (144 | 1) * 4 bytes > 160 KiB
    wide = sf.random_forest(rng, 144, 2, 3)
    with pytest.raises(RuntimeError, match="code -3"):
        predict_ops.partial_dependence_gpu(wide, torch.zeros((4, 144), dtype=torch.float32, device="cuda"), (0,), grid,
                                           want_ice=True, want_avg=True)
    # the entry point itself refuses what the wrapper checks first
    lib = _native.lib()
    gf = predict_ops.gpu_forest(b, Xd.device)
    g = torch.zeros(2, dtype=torch.float32, device="cuda")
    ice = torch.full((2, 8), 7.0, dtype=torch.float32, device="cuda")

    def call(f1, f2, G1, G2, g2, tile_cap=gf.tile_cap, F=6):
        return lib.cobalt_pdp(Xd.data_ptr(), 8, F, F, gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(),
                              gf.tile_ptr.data_ptr(), gf.n_tiles, tile_cap, 0.0, f1, f2, g.data_ptr(), G1, g2, G2,
                              None, ice.data_ptr(), None, None, _native.stream_handle())

    assert call(2, 2, 2, 1, g.data_ptr()) == -8
    assert call(6, -1, 2, 1, None) == -8
    assert call(0, 1, 2, 1, None) == -8          # two features without a second grid
    assert call(0, -1, 2, 2, None) == -8         # one feature with a second axis
    assert call(0, -1, 0, 1, None) == -8
    assert call(0, -1, 2, 1, None, tile_cap=8193) == -2
    torch.cuda.synchronize()
    assert bool((ice == 7.0).all())  # nothing was launched
