"""The oracles under the GPU scoring tests, checked against each other on a CPU host.

``treeshap_host`` (Lundberg's EXTEND / UNWIND, the algorithm of the kernels) must equal
``scoring_forests.shap_bruteforce`` (Shapley values from the definition, no paths) on the hand-built
forests of scoring_forests.py, and ``predict_margin_host`` must equal an obvious per-row float32 walk bit
for bit.

eps_ref -- the largest ``|treeshap_host - shap_bruteforce| / max|phi|`` over every forest of this module --
measured 3.7e-15 (the 11-feature caterpillars, 2^11 subsets per tree; every other forest 1e-16 .. 7e-16).
It is recorded as ``scoring_forests.EPS_REF = 3.7e-15`` and asserted here not to be exceeded; test_gpu_scoring_edges.py derives
its GPU-versus-oracle tolerance from it.
"""
import numpy as np
import pytest

import scoring_forests as sf
from cobalt_smart_lender_ai_amd.models import booster as B
from cobalt_smart_lender_ai_amd.ops import predict_ops


def _forests():
    """name -> (booster, query rows)."""
    out = {}
    rng = np.random.default_rng(11)
    grid = sf.THRESHOLD_GRID
    b = sf.random_forest(rng, 6, 6, 5, grid=grid)
    out["grid-edges"] = (b, sf.edge_rows(rng, 64, 6))
    b = sf.random_forest(rng, 20, 5, 5, cols=range(10))
    X = rng.normal(size=(24, 20)).astype(np.float32)
    X[rng.random(X.shape) < 0.1] = np.nan
    out["random-F20"] = (b, X)
    out["no-repeat-default-left"] = (sf.random_forest(rng, 7, 4, 5, repeat=False, default_left=1), X[:, :7].copy())
    out["no-repeat-default-right"] = (sf.random_forest(rng, 7, 4, 5, repeat=False, default_left=0), X[:, :7].copy())
    out["stumps"] = (sf.make_booster([sf.stump(0.25), sf.stump(-0.5, 3.0)], 3), X[:5, :3].copy())
    b = sf.make_booster([sf.zero_cover_tree(rng, 0, 1, "left"), sf.zero_cover_tree(rng, 1, 2, "right"),
                         sf.zero_cover_tree(rng, 2, 2, "left"), sf.stump(0.1),
                         sf.random_tree(rng, 3, 3, grid=grid)], 3)
    out["zero-cover"] = (b, sf.edge_rows(rng, 48, 3))
    for k in (1, 7, 8, 11):
        b = sf.make_booster([sf.caterpillar(rng, k, range(12)) for _ in range(3)] + [sf.stump(0.2)], 12)
        out[f"caterpillar-{k}"] = (b, rng.normal(0.0, 0.7, size=(12, 12)).astype(np.float32))
    out["paths-257"] = (sf.forest_with_paths(rng, 6, 257), rng.normal(size=(8, 6)).astype(np.float32))
    return out


FORESTS = _forests()


@pytest.mark.parametrize("name", list(FORESTS))
def test_treeshap_host_equals_bruteforce(name):
    b, X = FORESTS[name]
    with np.errstate(divide="raise", invalid="raise"):  # a zero-cover branch must not divide by its zero fraction
        phi_h = B.treeshap_host(b, X)
    phi_b = sf.shap_bruteforce(b, X)
    assert np.isfinite(phi_h).all() and np.isfinite(phi_b).all()
    scale = max(float(np.abs(phi_b).max()), 1e-300)
    eps = float(np.abs(phi_h - phi_b).max()) / scale
    print(f"[scoring-oracle] {name}: max|phi| {scale:.4g}, |treeshap_host - bruteforce| / max|phi| = {eps:.3g}")
    assert eps <= sf.EPS_REF, (name, eps)
    # local accuracy of the oracle itself: the values add up to the margin
    m = B.predict_margin_host(b, X).astype(np.float64)
    np.testing.assert_allclose(phi_b.sum(1) + b.expected_value(), m, rtol=0, atol=2e-6)


def test_eps_ref_is_a_rounding_error():
    assert sf.EPS_REF <= 1e-10  # above that the brute-force oracle would be wrong, not imprecise


@pytest.mark.parametrize("name", list(FORESTS))
def test_predict_margin_host_equals_rowwise_walk(name):
    b, X = FORESTS[name]
    want = sf.predict_rowwise(b, X)
    assert np.array_equal(B.predict_margin_host(b, X), want)
    for t in (1, min(3, b.num_trees)):
        assert np.array_equal(B.predict_margin_host(b, X, n_trees=t), sf.predict_rowwise(b, X, n_trees=t))
    assert np.array_equal(B.staged_margins_host(b, X)[-1], want)


def test_zero_cover_rows_on_both_sides():
    b, X = FORESTS["zero-cover"]
    t = b.trees[0]
    enters = (X[:, 0] < 0) & (X[:, 1] < 0)
    assert enters.any() and (~enters & ~np.isnan(X[:, :2]).any(1)).any()
    assert (t.sum_hessian[t.is_leaf] == 0).sum() == 1 and t.sum_hessian[0] > 0


def test_interactions_host_follows_the_trees_at_the_value_edges():
    """The merged-path interval test (``x >= lo and not x >= hi``, ``hi`` NaN without an upper bound) sends
    +-inf, the thresholds and their neighbours the way the tree walk does: the interaction rows sum to
    the SHAP values of the raw-tree oracle."""
    b, X = FORESTS["grid-edges"]
    inter = B.treeshap_interactions_host(b, X)
    phi = sf.shap_bruteforce(b, X)
    np.testing.assert_allclose(inter.sum(2), phi, rtol=1e-9, atol=1e-9)


def test_builders_build_what_they_say():
    rng = np.random.default_rng(5)
    for k in (0, 1, 7, 15):
        b = sf.make_booster([sf.caterpillar(rng, k, range(16))], 16)
        assert sf.max_unique_path(b) == k and sf.n_leaf_paths(b) == k + 1
        assert predict_ops.extract_paths(b)[3] == k
    for n in (1, 2, 255, 256, 257, 513):
        b = sf.forest_with_paths(rng, 6, n)
        assert sf.n_leaf_paths(b) == n == len(predict_ops.extract_paths(b)[2])
    for n in (4, 6, 8, 11, 16, 32):
        assert sf.grown_tree(rng, 5, n, 6).num_nodes == 2 * n - 1
    t = sf.random_tree(rng, 9, 5, repeat=False)
    for _, path in B.iter_leaf_paths(t):
        assert len({f for _, f, _ in path}) == len(path)
    for t in sf.random_forest(rng, 9, 3, 5).trees:  # covers: every parent is the sum of its children
        s = ~t.is_leaf
        assert np.array_equal(t.sum_hessian[s], t.sum_hessian[t.left_children[s]] + t.sum_hessian[t.right_children[s]])
    g = sf.random_tree(rng, 4, 5, grid=sf.THRESHOLD_GRID)
    assert np.isin(g.split_conditions[~g.is_leaf], sf.THRESHOLD_GRID).all()


def test_shap_values_refuses_a_narrow_matrix():
    b, X = FORESTS["random-F20"]
    with pytest.raises(ValueError):
        predict_ops.shap_values(b, X[:, :19], device="cpu")
