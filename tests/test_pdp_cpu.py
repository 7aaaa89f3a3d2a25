"""Partial dependence / ICE on the CPU path: ``partial_dependence_host`` (the definition, also the oracle of
csrc/pdp.hip) against ``scoring_forests.predict_rowwise`` on explicitly substituted copies of X, the grid
rule, the argument checks, the classifier path and the plots.

Averages: ``partial_dependence_host`` sums with ``math.fsum`` (correctly rounded) and divides two doubles,
the test does the same from its own margins, so they agree to an ulp; the bound asked for is 4 ulp relative.
"""
import math

import numpy as np
import pytest

import scoring_forests as sf
from cobalt_smart_lender_ai_amd import explain
from cobalt_smart_lender_ai_amd.models import booster as B
from cobalt_smart_lender_ai_amd.models import gbdt
from cobalt_smart_lender_ai_amd.utils import plots

ULP4 = 4 * 2.0 ** -52


def _substituted(X, feats, grids):
    """One substituted copy of X per grid point k = i1 * G2 + i2, written out the long way."""
    out = []
    if len(feats) == 1:
        for a in grids[0]:
            Xs = np.array(X, np.float32)
            Xs[:, feats[0]] = a
            out.append(Xs)
        return out
    for a in grids[0]:
        for c in grids[1]:
            Xs = np.array(X, np.float32)
            Xs[:, feats[0]] = a
            Xs[:, feats[1]] = c
            out.append(Xs)
    return out


def _forest_and_rows(seed=0, F=6, n=37):
    rng = np.random.default_rng(seed)
    b = sf.random_forest(rng, F, 9, 4, grid=sf.THRESHOLD_GRID)
    return b, sf.edge_rows(rng, n, F)


# values the walk has to get right: missing, both infinities, the signed zero, a value exactly on a threshold
# (0.25 is one of THRESHOLD_GRID: x < 0.25 is false there) and its two neighbours
EDGE_GRID = np.array([np.nan, np.inf, -np.inf, -0.0, 0.25, np.nextafter(np.float32(0.25), np.float32(0)),
                      np.nextafter(np.float32(0.25), np.float32(1)), -1.5, 3.0], np.float32)


@pytest.mark.parametrize("case", ["1d", "2d-3x5"])
def test_host_ice_equals_rowwise_on_substituted_copies(case):
    b, X = _forest_and_rows(1)
    if case == "1d":
        feats, grids = (2,), [EDGE_GRID]
    else:  # non-square: a transposed i1 * G2 + i2 fails
        feats, grids = (4, 1), [EDGE_GRID[[0, 4, 7]], EDGE_GRID[[1, 0, 3, 4, 8]]]
    X0 = X.copy()
    ice, avg_m, avg_p = B.partial_dependence_host(b, X, feats, grids)
    assert np.array_equal(X, X0, equal_nan=True)
    want = np.stack([sf.predict_rowwise(b, Xs) for Xs in _substituted(X, feats, grids)])
    assert ice.dtype == np.float32 and ice.shape == want.shape
    np.testing.assert_array_equal(ice, want)
    for k in range(len(want)):
        m = want[k].astype(np.float64)
        em = math.fsum(m) / len(m)
        ep = math.fsum(1.0 / (1.0 + np.exp(-m))) / len(m)
        assert abs(avg_m[k] - em) <= ULP4 * abs(em)
        assert abs(avg_p[k] - ep) <= ULP4 * abs(ep)


def test_weighted_means_ignore_zero_weight_rows():
    b, X = _forest_and_rows(2, n=20)
    w = np.linspace(0.5, 2.0, 20).astype(np.float32)
    w[[3, 11]] = 0.0
    grid = np.array([-1.0, 0.25, np.nan], np.float32)
    ice, avg_m, avg_p = B.partial_dependence_host(b, X, (0,), [grid], None, w)
    keep = w > 0
    ice_k, avg_mk, avg_pk = B.partial_dependence_host(b, X[keep], (0,), [grid], None, w[keep])
    np.testing.assert_array_equal(ice[:, keep], ice_k)
    np.testing.assert_array_equal(avg_m, avg_mk)
    np.testing.assert_array_equal(avg_p, avg_pk)
    wd = w.astype(np.float64)
    for k in range(3):
        m = sf.predict_rowwise(b, _substituted(X, (0,), [grid])[k]).astype(np.float64)
        em = math.fsum(wd * m) / math.fsum(wd)
        ep = math.fsum(wd * (1.0 / (1.0 + np.exp(-m)))) / math.fsum(wd)
        assert abs(avg_m[k] - em) <= ULP4 * abs(em) and abs(avg_p[k] - ep) <= ULP4 * abs(ep)
    # and through the public interface
    r = b.partial_dependence(X, 0, grid=grid, sample_weight=w, response="margin", device="cpu")
    np.testing.assert_array_equal(r["average"], avg_m)


def test_probability_is_mean_of_sigmoids_not_sigmoid_of_mean():
    b, X = _forest_and_rows(3, n=50)
    r = b.partial_dependence(X, 1, grid=[-2.0, 0.0, 2.0], kind="both", device="cpu")
    rm = b.partial_dependence(X, 1, grid=[-2.0, 0.0, 2.0], kind="both", response="margin", device="cpu")
    assert r["individual"].dtype == np.float32 and r["individual"].shape == (50, 3)
    np.testing.assert_array_equal(r["individual"], B.sigmoid32(rm["individual"]))
    m = rm["individual"].astype(np.float64)
    want = np.array([math.fsum(1.0 / (1.0 + np.exp(-m[:, k]))) / 50 for k in range(3)])
    np.testing.assert_allclose(r["average"], want, rtol=ULP4, atol=0)
    sig_of_mean = 1.0 / (1.0 + np.exp(-rm["average"]))
    assert np.abs(sig_of_mean - want).max() > 1e-6  # the two differ on this forest: the check can tell them apart


def test_grid_construction():
    rng = np.random.default_rng(4)
    b = sf.random_forest(rng, 3, 4, 3)
    X = rng.normal(size=(200, 3)).astype(np.float32)
    X[:, 0] = rng.integers(0, 7, size=200).astype(np.float32) * 0.5  # 7 unique values
    X[rng.random(200) < 0.2, 0] = np.nan
    X[rng.random(200) < 0.2, 1] = np.nan
    r = b.partial_dependence(X, 0, grid_resolution=10, device="cpu")
    col0 = X[:, 0][~np.isnan(X[:, 0])]
    assert len(np.unique(col0)) == 7
    np.testing.assert_array_equal(r["grid_values"][0], np.unique(col0))
    assert r["grid_values"][0].dtype == np.float32 and r["average"].shape == (7,)
    col1 = X[:, 1][~np.isnan(X[:, 1])]
    want = np.linspace(np.percentile(col1, 5), np.percentile(col1, 95), 10).astype(np.float32)
    r = b.partial_dependence(X, 1, grid_resolution=10, device="cpu")
    np.testing.assert_array_equal(r["grid_values"][0], want)
    r = b.partial_dependence(X, (1, 0), grid_resolution=10, include_missing=True, device="cpu")
    np.testing.assert_array_equal(r["grid_values"][0][:-1], want)
    np.testing.assert_array_equal(r["grid_values"][1][:-1], np.unique(col0))
    assert np.isnan(r["grid_values"][0][-1]) and np.isnan(r["grid_values"][1][-1])
    assert r["average"].shape == (11, 8)
    r = b.partial_dependence(X, 2, percentiles=(0.25, 0.75), grid_resolution=5, device="cpu")
    np.testing.assert_array_equal(
        r["grid_values"][0], np.linspace(np.percentile(X[:, 2], 25), np.percentile(X[:, 2], 75), 5).astype(np.float32))


def test_argument_errors():
    rng = np.random.default_rng(5)
    b = sf.random_forest(rng, 4, 3, 3)
    b.feature_names = ["fico", "dti", "loan_amnt", "term"]
    X = rng.normal(size=(30, 4)).astype(np.float32)
    bad = [dict(features="income"), dict(features=4), dict(features=-1), dict(features=(1, 1)),
           dict(features=("dti", 1)), dict(features=(0, 1, 2)), dict(features=()), dict(features=0, grid=[]),
           dict(features=(0, 1), grid=[[0.0], []]), dict(features=0, kind="mean"), dict(features=0, response="odds"),
           dict(features=0, sample_weight=np.zeros(30)), dict(features=0, sample_weight=-np.ones(30)),
           dict(features=0, sample_weight=np.ones(29)), dict(features=0, percentiles=(0.9, 0.1)),
           dict(features=0, grid_resolution=1)]
    for kw in bad:
        with pytest.raises(ValueError):
            b.partial_dependence(X, device="cpu", **kw)
    Xn = X.copy()
    Xn[:, 2] = np.nan
    with pytest.raises(ValueError):
        b.partial_dependence(Xn, 2, device="cpu")  # all NaN, no explicit grid
    assert b.partial_dependence(Xn, 2, grid=[0.0, 1.0], device="cpu")["average"].shape == (2,)
    with pytest.raises(ValueError):
        b.partial_dependence(X[:, :3], 0, device="cpu")  # narrower than the model


def test_names_resolve_and_X_is_unchanged():
    rng = np.random.default_rng(6)
    b = sf.random_forest(rng, 4, 5, 3)
    b.feature_names = ["fico", "dti", "loan_amnt", "term"]
    X = rng.normal(size=(40, 4)).astype(np.float32)
    X[3, 1] = np.nan
    X0 = X.copy()
    by_name = b.partial_dependence(X, ("loan_amnt", "fico"), grid_resolution=4, kind="both", device="cpu")
    by_index = b.partial_dependence(X, (2, 0), grid_resolution=4, kind="both", device="cpu")
    assert np.array_equal(X, X0, equal_nan=True)
    assert by_name["feature_names"] == ["loan_amnt", "fico"] == by_index["feature_names"]
    for k in ("average", "individual"):
        np.testing.assert_array_equal(by_name[k], by_index[k])
    assert by_name["individual"].shape == (40, 4, 4) and by_name["average"].shape == (4, 4)
    one = b.partial_dependence(X, "dti", grid_resolution=4, device="cpu")
    assert one["feature_names"] == ["dti"] and "individual" not in one
    # individual[r, i1, i2] is row r at (grid 0 [i1], grid 1 [i2])
    g0, g1 = by_name["grid_values"]
    Xs = X.copy()
    Xs[:, 2], Xs[:, 0] = g0[1], g1[3]
    np.testing.assert_array_equal(by_name["individual"][:, 1, 3], B.sigmoid32(sf.predict_rowwise(b, Xs)))


def test_unused_feature_has_flat_ice():
    rng = np.random.default_rng(7)
    b = sf.random_forest(rng, 5, 6, 4, cols=[0, 1, 3, 4])  # no tree splits on feature 2
    X = sf.edge_rows(rng, 25, 5)
    r = b.partial_dependence(X, 2, grid=EDGE_GRID, kind="individual", response="margin", device="cpu")
    plain = sf.predict_rowwise(b, X)
    for k in range(len(EDGE_GRID)):
        np.testing.assert_array_equal(r["individual"][:, k], plain)


def _small_fit(**kw):
    rng = np.random.default_rng(8)
    X = rng.normal(size=(600, 4)).astype(np.float32)
    y = (X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.3 * rng.normal(size=600) > 0).astype(np.int64)
    clf = gbdt.GBDTClassifier(n_estimators=12, max_depth=3, learning_rate=0.3, device="cpu", **kw)
    return clf, X, y


def test_classifier_honours_best_iteration_and_iteration_range():
    clf, X, y = _small_fit()
    clf.fit(X, y)
    bst = clf.get_booster()
    grid = np.array([-1.0, 0.0, 1.0], np.float32)
    full = explain.partial_dependence(clf, X[:50], 0, grid=grid, kind="both")
    np.testing.assert_array_equal(full["average"], bst.partial_dependence(X[:50], 0, grid=grid, device="cpu")["average"])
    part = explain.partial_dependence(clf, X[:50], 0, grid=grid, kind="both", iteration_range=(0, 5))
    want = bst.partial_dependence(X[:50], 0, grid=grid, kind="both", n_trees=5, device="cpu")
    np.testing.assert_array_equal(part["average"], want["average"])
    np.testing.assert_array_equal(part["individual"], want["individual"])
    assert not np.array_equal(part["average"], full["average"])
    # ICE probabilities at the rows' own values are predict_proba's
    Xs = X[:50].copy()
    Xs[:, 0] = grid[2]
    np.testing.assert_array_equal(part["individual"][:, 2], clf.predict_proba(Xs, iteration_range=(0, 5))[:, 1]
                                  .astype(np.float32))
    # an early-stopped model scores best_iteration + 1 trees by default, as predict_proba does
    bst.attributes["best_iteration"] = "3"
    early = explain.partial_dependence(clf, X[:50], 0, grid=grid)
    np.testing.assert_array_equal(early["average"],
                                  bst.partial_dependence(X[:50], 0, grid=grid, n_trees=4, device="cpu")["average"])
    # a Booster and a TreeExplainer are accepted too
    np.testing.assert_array_equal(explain.partial_dependence(bst, X[:50], 0, grid=grid, device="cpu")["average"],
                                  full["average"])
    ex = explain.TreeExplainer(clf, device="cpu")
    np.testing.assert_array_equal(explain.partial_dependence(ex, X[:50], 0, grid=grid)["average"], full["average"])
    with pytest.raises(TypeError):
        explain.partial_dependence(object(), X, 0)


def test_pd_plot_figures():
    b, X = _forest_and_rows(9, n=30)
    one = b.partial_dependence(X, 1, grid=[-1.5, 0.0, 0.25, 1.0], include_missing=True, kind="both", device="cpu")
    fig = explain.pd_plot(one, max_ice=10)
    ax = fig.axes[0]
    assert ax.get_xlabel() == "f1" and "missing" in [t.get_text() for t in ax.get_xticklabels()]
    thick = [ln for ln in ax.get_lines() if ln.get_linewidth() > 2 and len(ln.get_xdata()) == 4]
    assert len(thick) == 1  # the average over the 4 numeric points; the missing point is drawn apart
    np.testing.assert_allclose(thick[0].get_ydata(), one["average"][:4])
    assert sum(len(ln.get_xdata()) == 4 for ln in ax.get_lines()) == 1 + 10
    plots.close(fig)
    fig = explain.pd_plot(one, ice=False, centered=True)
    thick = [ln for ln in fig.axes[0].get_lines() if len(ln.get_xdata()) == 4]
    assert len(thick) == 1 and thick[0].get_ydata()[0] == 0.0
    plots.close(fig)
    two = b.partial_dependence(X, (0, 3), grid=[[-1.0, 0.0, 1.0], [-2.0, 0.5, 1.0, 2.0]], device="cpu")
    fig = explain.pd_plot(two)
    assert fig.axes[0].get_xlabel() == "f0" and fig.axes[0].get_ylabel() == "f3"
    plots.close(fig)
