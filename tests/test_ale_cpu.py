"""The host definition of accumulated local effects (models/booster.py ale_host, ale_curve, ale_edges,
Booster.accumulated_local_effects on the CPU): the oracle of csrc/ale.hip, checked here against facts that hold
by construction on hand-built forests.

Where a test asks for 1e-12 on margins, the forest has base_score 0.5 (base margin 0) and leaf values that are
small multiples of 2^-6: every float32 sum in tree order is then exact, so a forest that is additive on paper is
additive in its float32 margins too, and what is left is float64 rounding of the means and cumulative sums.
"""
import numpy as np
import pytest

import scoring_forests as sf
from cobalt_smart_lender_ai_amd import explain
from cobalt_smart_lender_ai_amd.models import booster as B


def _split_tree(feat, thr, left, right, default_left=0):
    """One split on ``feat`` at ``thr`` with leaf values ``left`` / ``right``."""
    nodes = sf._Nodes()
    nodes.split(0, feat, thr, default_left)
    t = nodes.finish(np.random.default_rng(0))
    t.split_conditions[1], t.split_conditions[2] = np.float32(left), np.float32(right)
    return t


def _dyadic_tree(rng, F, feat, n_splits=3):
    """A random tree on ``feat`` alone whose leaves are multiples of 2^-6 in [-1, 1]."""
    t = sf.grown_tree(rng, F, n_splits + 1, 6, cols=[feat])
    leaf = t.is_leaf
    t.split_conditions[leaf] = (rng.integers(-64, 65, size=int(leaf.sum())) / 64.0).astype(np.float32)
    return t


def _booster(trees, F):
    b = sf.make_booster(trees, F, base_score=0.5)
    assert b.base_margin == 0.0
    return b


# ---------------------------------------------------------------------------------- one stump
@pytest.mark.parametrize("thr,step_at", [(0.3, 2), (0.5, 2), (0.0, None), (1.0, 3), (-1.0, None), (1.7, None)])
def test_one_stump_steps_in_the_interval_that_holds_its_threshold(thr, step_at):
    """Edges 0, 0.25, 0.5, 1 and one split "x < t goes left (a), else right (b)". lo = z[k-1] and hi = z[k] land
    in different leaves exactly when z[k-1] < t <= z[k]: the uncentred curve steps by b - a there and is flat
    elsewhere. A threshold at or below z[0], or above z[K], is straddled by no interval."""
    z = np.array([0.0, 0.25, 0.5, 1.0], np.float32)
    a, bb = -0.75, 0.5
    b = _booster([_split_tree(1, thr, a, bb)], 3)
    rng = np.random.default_rng(1)
    X = rng.uniform(-0.5, 1.5, size=(200, 3)).astype(np.float32)
    r = b.accumulated_local_effects(X, 1, grid=z, response="margin", centered=False, device="cpu")
    want = np.zeros(4)
    if step_at is not None:
        want[step_at:] = bb - a
    np.testing.assert_array_equal(r["ale"], want)
    assert r["interval_weight"].sum() == 200 and r["n_missing"] == 0


def test_threshold_equal_to_an_edge():
    """t = z[2]: z[1] goes left (z[1] < t) and z[2] goes right (x < t is false at x = t), so the step belongs to
    (z[1], z[2]], the interval that holds t; with t one ulp above z[2] it belongs to the next interval."""
    z = np.array([0.0, 0.25, 0.5, 1.0], np.float32)
    X = np.linspace(-0.2, 1.2, 57, dtype=np.float32)[:, None]
    for thr, k in ((np.float32(0.5), 2), (np.nextafter(np.float32(0.5), np.float32(1.0)), 3)):
        b = _booster([_split_tree(0, thr, 0.0, 1.0)], 1)
        A = b.accumulated_local_effects(X, 0, grid=z, response="margin", centered=False, device="cpu")["ale"]
        np.testing.assert_array_equal(np.diff(A), np.eye(3)[k - 1])


# ------------------------------------------------------------------------------ additive forest
def test_additive_forest():
    rng = np.random.default_rng(2)
    F = 4
    owner = [0, 1, 2, 0, 1, 2, 0, 2, 1, 0]          # feature 3 is used by no tree
    trees = [_dyadic_tree(rng, F, f) for f in owner]
    b = _booster(trees, F)
    X = rng.normal(size=(400, F)).astype(np.float32)
    X[:, 1] = (0.8 * X[:, 0] + 0.2 * X[:, 1]).astype(np.float32)  # correlated columns
    w = rng.uniform(0.5, 2.0, size=400).astype(np.float32)
    for j in range(F):
        r = b.accumulated_local_effects(X, j, grid_resolution=9, response="margin", sample_weight=w, device="cpu")
        z = r["edges"][0]
        # the sum of j's trees at the edges (other columns do not matter), centred as the definition centres
        probe = np.zeros((len(z), F), np.float32)
        probe[:, j] = z
        mine = B.Booster([t for t, f in zip(trees, owner) if f == j], num_feature=F, base_score=0.5)
        g = B.predict_margin_host(mine, probe).astype(np.float64) if mine.trees else np.zeros(len(z))
        W = r["interval_weight"]
        want = g - (W * (g[:-1] + g[1:]) / 2).sum() / W.sum()
        np.testing.assert_allclose(r["ale"], want, rtol=0, atol=1e-12)
        if j == 3:
            np.testing.assert_array_equal(r["ale"], np.zeros(len(z)))
    for pair in ((0, 1), (1, 2), (2, 0), (0, 3)):
        r = b.accumulated_local_effects(X, pair, grid_resolution=6, response="margin", sample_weight=w, device="cpu")
        assert r["ale"].shape == (len(r["edges"][0]), len(r["edges"][1]))
        assert float(np.abs(r["ale"]).max()) <= 1e-12
        assert float(np.abs(r["interval_effect"]).max()) <= 1e-12


def test_a_tree_that_uses_both_features_interacts():
    """The counterpart of the zeros above: x0 AND x1 on one path is an interaction and shows as one."""
    nodes = sf._Nodes()
    _, r = nodes.split(0, 0, 0.0, 0)
    nodes.split(r, 1, 0.0, 0)
    t = nodes.finish(np.random.default_rng(0))
    t.split_conditions[t.is_leaf] = np.array([0.0, 0.0, 1.0], np.float32)   # 1 only where x0 >= 0 and x1 >= 0
    b = _booster([t], 2)
    X = np.random.default_rng(3).normal(size=(500, 2)).astype(np.float32)
    z = np.array([-1.0, -0.5, 0.5, 1.0], np.float32)   # only the middle cell straddles both thresholds
    r = b.accumulated_local_effects(X, (0, 1), grid=(z, z), response="margin", device="cpu")
    np.testing.assert_array_equal(r["interval_effect"], [[0, 0, 0], [0, 1, 0], [0, 0, 0]])
    assert float(np.abs(r["ale"]).max()) > 0.1


# --------------------------------------------------------------------- out-of-interval evaluation
def test_ale_never_visits_a_leaf_that_no_row_neighbourhood_reaches_and_pd_does():
    """x1 = x0 exactly; a leaf of 1000 sits at x0 < -1 and x1 >= 1, far off the diagonal. PD on x0 scores the rows
    with x1 >= 1 at x0 = -2 and lands there; ALE moves a row only inside its own interval of x0, and no interval
    holds both x0 < -1 and a row with x1 = x0 >= 1."""
    nodes = sf._Nodes()
    l, r = nodes.split(0, 0, -1.0, 0)
    nodes.split(l, 1, 1.0, 0)
    t = nodes.finish(np.random.default_rng(0))
    # BFS: 1 = left child (split on x1), 2 = right leaf, 3 / 4 = children of node 1
    t.split_conditions[2], t.split_conditions[3], t.split_conditions[4] = 0.25, -0.25, 1000.0
    b = _booster([t], 2)
    x = np.linspace(-2.0, 2.0, 41, dtype=np.float32)
    X = np.stack([x, x], axis=1)
    assert float(np.abs(B.predict_margin_host(b, X)).max()) <= 0.25      # no row sees the leaf
    z = np.array([-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0], np.float32)
    ale = b.accumulated_local_effects(X, 0, grid=z, response="margin", device="cpu")
    assert float(np.abs(ale["ale"]).max()) <= 0.5 and float(np.abs(ale["interval_effect"]).max()) <= 0.5
    pd = b.partial_dependence(X, 0, grid=z, response="margin", device="cpu")
    assert float(pd["average"].max()) > 100.0


# ------------------------------------------------------------------------------------ edge rules
def test_interval_rule():
    z = np.array([0.0, 1.0, 2.0], np.float32)
    up = np.nextafter(np.float32(1.0), np.float32(2.0))
    x = np.array([-np.inf, -5.0, 0.0, 1e-30, 1.0, up, 2.0, 2.5, np.inf, np.nan], np.float32)
    np.testing.assert_array_equal(B.ale_interval_host(z, x), [1, 1, 1, 1, 1, 2, 2, 2, 2, 1])


def test_nan_rows_infinities_and_clamping():
    b = _booster([_split_tree(0, 0.5, -1.0, 1.0), _split_tree(1, 0.0, 0.25, -0.25, default_left=1)], 2)
    z = np.array([0.0, 1.0, 2.0], np.float32)
    X = np.array([[np.nan, 0.0], [-np.inf, 1.0], [-3.0, np.nan], [0.0, 0.0], [1.0, -1.0], [1.5, 0.0], [7.0, 2.0],
                  [np.inf, 0.0], [np.nan, np.nan]], np.float32)
    r = B.ale_host(b, X, [0], [z])
    assert r["n_missing"] == 2
    np.testing.assert_array_equal(r["cell"], [-1, 0, 0, 0, 0, 1, 1, 1, -1])
    np.testing.assert_array_equal(r["weight"], [4.0, 3.0])
    # interval 1 is (., 1]: lo = 0 goes left (-1), hi = 1 goes right (+1); interval 2: both right
    np.testing.assert_array_equal(r["sum_margin"], [8.0, 0.0])
    # corners are predict_margin_host on the substituted rows, NaN in the other column included
    for c, zc in enumerate((z[r["cell"].clip(0)], z[r["cell"].clip(0) + 1])):
        Xs = X.copy()
        Xs[:, 0] = zc
        np.testing.assert_array_equal(r["corners"][c], B.predict_margin_host(b, Xs))
    res = b.accumulated_local_effects(X, 0, grid=z, response="margin", centered=False, device="cpu")
    np.testing.assert_array_equal(res["ale"], [0.0, 2.0, 2.0])
    assert res["n_missing"] == 2


def test_single_interval_empty_intervals_and_constant_columns():
    rng = np.random.default_rng(4)
    b = _booster([_split_tree(0, 0.5, -1.0, 1.0)], 2)
    X = rng.uniform(0.0, 1.0, size=(50, 2)).astype(np.float32)
    one = b.accumulated_local_effects(X, 0, grid=[0.0, 1.0], response="margin", device="cpu")     # K = 1
    np.testing.assert_array_equal(one["interval_effect"], [2.0])
    np.testing.assert_array_equal(one["ale"], [-1.0, 1.0])
    # no row in (2, 3] and (3, 4]: effect 0, the curve is carried forward
    r = b.accumulated_local_effects(X, 0, grid=[0.0, 1.0, 2.0, 3.0, 4.0], response="margin", centered=False,
                                    device="cpu")
    np.testing.assert_array_equal(r["interval_weight"], [50.0, 0.0, 0.0, 0.0])
    np.testing.assert_array_equal(r["ale"], [0.0, 2.0, 2.0, 2.0, 2.0])
    Xc = X.copy()
    Xc[:, 1] = 3.0
    Xc[:5, 1] = np.nan
    c = b.accumulated_local_effects(Xc, 1, device="cpu")
    np.testing.assert_array_equal(c["ale"], [0.0])
    assert c["interval_effect"].shape == (0,) and c["n_missing"] == 5 and len(c["edges"][0]) == 1
    both = b.accumulated_local_effects(Xc, device="cpu")     # features=None: every feature, a list
    assert isinstance(both, list) and [len(q["ale"]) for q in both] == [21, 1]


def test_default_edges():
    rng = np.random.default_rng(5)
    few = np.array([3.0, 1.0, np.nan, 2.0, 1.0, 3.0], np.float32)
    np.testing.assert_array_equal(B.ale_edges(few, 20), [1.0, 2.0, 3.0])
    np.testing.assert_array_equal(B.ale_edges(few, 2), [1.0, 2.0, 3.0])      # 3 <= 2 + 1 distinct values
    col = rng.normal(size=1000).astype(np.float32)
    col[::50] = np.nan
    z = B.ale_edges(col, 10)
    vals = col[~np.isnan(col)]
    want = np.unique(np.quantile(vals.astype(np.float64), np.linspace(0, 1, 11)).astype(np.float32))
    np.testing.assert_array_equal(z, want)
    assert z.dtype == np.float32 and len(z) == 11 and z[0] == vals.min() and z[-1] == vals.max()
    heavy = np.concatenate([np.zeros(900, np.float32), rng.normal(size=100).astype(np.float32)])
    zh = B.ale_edges(heavy, 20)                                              # repeated quantiles collapse
    assert (np.diff(zh) > 0).all() and len(zh) < 21
    assert len(B.ale_edges(np.full(7, 2.5, np.float32), 20)) == 1
    assert len(B.ale_edges(np.full(7, np.nan, np.float32), 20)) == 0


def test_bad_grids_weights_and_features_raise():
    b = _booster([_split_tree(0, 0.5, -1.0, 1.0)], 2)
    X = np.zeros((6, 2), np.float32)
    for bad in ([0.0], [0.0, 0.0], [1.0, 0.0], [0.0, np.nan, 1.0], [0.0, np.inf], [[0.0, 1.0]]):
        with pytest.raises(ValueError):
            b.accumulated_local_effects(X, 0, grid=bad, device="cpu")
    with pytest.raises(ValueError):
        b.accumulated_local_effects(X, (0, 1), grid=[0.0, 1.0], device="cpu")         # a pair needs two vectors
    for w in (np.ones(5), -np.ones(6), np.zeros(6), np.full(6, np.nan)):
        with pytest.raises(ValueError, match="sample_weight"):
            b.accumulated_local_effects(X, 0, grid=[0.0, 1.0], sample_weight=w, device="cpu")
    for feats in (2, -1, "nope", (0, 0), (0, 1, 1), [(0,)], 1.5):
        with pytest.raises(ValueError):
            b.accumulated_local_effects(X, feats, grid=None, device="cpu")
    with pytest.raises(ValueError, match="response"):
        b.accumulated_local_effects(X, 0, response="odds", device="cpu")
    with pytest.raises(ValueError):
        b.accumulated_local_effects(np.zeros((0, 2), np.float32), 0, device="cpu")
    with pytest.raises(ValueError):
        b.accumulated_local_effects(np.zeros((3, 1), np.float32), 0, device="cpu")


# --------------------------------------------------------------------------------------- weights
def test_integer_weights_equal_row_duplication():
    rng = np.random.default_rng(6)
    F = 3
    b = sf.random_forest(rng, F, 6, 3)
    X = rng.normal(size=(120, F)).astype(np.float32)
    X[rng.random(X.shape) < 0.05] = np.nan
    w = rng.integers(0, 4, size=120)
    w[0] = 2
    Xd = np.repeat(X, w, axis=0)
    z = np.array([-1.5, -0.5, 0.0, 0.4, 1.5], np.float32)
    for response in ("margin", "probability"):
        for feats, grid in ((1, z), ((0, 2), (z, z[1:]))):
            a = b.accumulated_local_effects(X, feats, grid=grid, response=response, sample_weight=w, device="cpu")
            d = b.accumulated_local_effects(Xd, feats, grid=grid, response=response, device="cpu")
            np.testing.assert_allclose(a["ale"], d["ale"], rtol=0, atol=1e-12)
            np.testing.assert_allclose(a["interval_effect"], d["interval_effect"], rtol=0, atol=1e-12)
            np.testing.assert_array_equal(a["interval_weight"], d["interval_weight"])


def test_uncentred_curve_is_the_running_sum_and_centring_removes_the_weighted_mean():
    rng = np.random.default_rng(7)
    b = sf.random_forest(rng, 3, 5, 3)
    X = rng.normal(size=(90, 3)).astype(np.float32)
    raw = b.accumulated_local_effects(X, 2, grid_resolution=7, centered=False, device="cpu")
    cen = b.accumulated_local_effects(X, 2, grid_resolution=7, device="cpu")
    np.testing.assert_array_equal(raw["ale"], np.concatenate([[0.0], np.cumsum(raw["interval_effect"])]))
    W, A = cen["interval_weight"], cen["ale"]
    assert abs(float((W * (A[:-1] + A[1:]) / 2).sum())) <= 1e-12 * W.sum()
    np.testing.assert_allclose(np.diff(A), np.diff(raw["ale"]), rtol=0, atol=1e-15)
    raw2 = b.accumulated_local_effects(X, (0, 1), grid_resolution=4, centered=False, device="cpu")
    e = raw2["interval_effect"]
    np.testing.assert_array_equal(raw2["ale"][1:, 1:], np.cumsum(np.cumsum(e, axis=0), axis=1))
    assert not raw2["ale"][0].any() and not raw2["ale"][:, 0].any()


# --------------------------------------------------------------------------------- front end
def test_explain_front_end_and_plots():
    rng = np.random.default_rng(8)
    b = sf.random_forest(rng, 4, 6, 3)
    X = rng.normal(size=(150, 4)).astype(np.float32)
    one = explain.accumulated_local_effects(b, X, 1, device="cpu")
    same = explain.accumulated_local_effects(explain.TreeExplainer(b, device="cpu"), X, "f1")
    np.testing.assert_array_equal(one["ale"], same["ale"])
    assert one["feature_names"] == ["f1"]
    pair = explain.accumulated_local_effects(b, X, (0, 2), grid_resolution=5, device="cpu")
    many = explain.accumulated_local_effects(b, X, [0, (1, 3), "f2"], grid_resolution=5, device="cpu")
    assert [len(r["edges"]) for r in many] == [1, 2, 1]
    with pytest.raises(TypeError):
        explain.accumulated_local_effects(object(), X)
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    for res in (one, pair, many):
        fig = explain.ale_plot(res)
        assert hasattr(fig, "savefig")
        plt.close(fig)
