"""Interventional TreeSHAP against a background set on a CPU host: the closed form per merged leaf path
(``treeshap_interventional_host``) against the definition by subset enumeration on hybrid rows
(``shapley_interventional_bruteforce``), the identities the values must satisfy, and the argument rules of
``TreeExplainer(model, data=..., feature_perturbation=..., model_output=...)``.

Tolerance of closed form versus enumeration: ``BRUTE_TOL = 1e-10`` absolute, the bound the existing
oracle-versus-enumeration SHAP test uses (``_check_against_bruteforce`` in test_shap_interactions_cpu.py).
"""
import dataclasses

import numpy as np
import pytest
import torch

import scoring_forests as sf
from cobalt_smart_lender_ai_amd.explain import TreeExplainer
from cobalt_smart_lender_ai_amd.models import booster as B
from cobalt_smart_lender_ai_amd.ops import predict_ops

BRUTE_TOL = 1e-10  # test_shap_interactions_cpu._check_against_bruteforce: max |host - brute force| <= 1e-10
MODES = ("raw", "probability")


def _literal_rescale(fx, fz):
    """The issue's s(x, z) as written: the quotient, and the derivative where the margins are equal."""
    fx, fz = np.broadcast_arrays(fx, fz)
    sx, sz = 1.0 / (1.0 + np.exp(-fx)), 1.0 / (1.0 + np.exp(-fz))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(fx == fz, sx * (1.0 - sx), (sx - sz) / (fx - fz))


def _forests():
    """name -> (booster, X, Z): F <= 8, repeated features on paths, thresholds on the grid, NaN and +-inf in
    both matrices, both default directions."""
    out = {}
    rng = np.random.default_rng(23)
    grid = sf.THRESHOLD_GRID
    b = sf.random_forest(rng, 6, 6, 5, grid=grid)
    out["grid-edges-mixed-defaults"] = (b, sf.edge_rows(rng, 34, 6), sf.edge_rows(rng, 9, 6))
    for dl in (0, 1):
        b = sf.random_forest(rng, 5, 4, 5, grid=grid, default_left=dl)
        X, Z = sf.edge_rows(rng, 30, 5), sf.edge_rows(rng, 7, 5)
        Z[:3] = [np.nan, np.inf, -np.inf, 0.25, np.nan]
        out[f"default-left-{dl}"] = (b, X, Z)
    b = sf.random_forest(rng, 8, 5, 6, p_leaf=0.1)
    X = rng.normal(size=(8, 8)).astype(np.float32)
    Z = rng.normal(size=(4, 8)).astype(np.float32)
    X[rng.random(X.shape) < 0.15] = np.nan
    Z[rng.random(Z.shape) < 0.15] = np.nan
    X[0, 3], Z[1, 5] = np.inf, -np.inf
    out["random-F8"] = (b, X, Z)
    b = sf.make_booster([sf.caterpillar(rng, k, range(7), grid=grid) for k in (7, 5, 1)] + [sf.stump(0.2)], 7)
    out["caterpillars"] = (b, sf.edge_rows(rng, 12, 7), sf.edge_rows(rng, 5, 7))
    return out


FORESTS = _forests()


@pytest.fixture(scope="module")
def pair_values():
    """name -> the brute-force Shapley values of every (x, z) pair, [N, B, F]: computed once."""
    return {name: B.shapley_interventional_bruteforce(b, X, Z) for name, (b, X, Z) in FORESTS.items()}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(FORESTS))
def test_closed_form_equals_subset_enumeration(name, mode, pair_values):
    b, X, Z = FORESTS[name]
    assert sf.max_unique_path(b) < sf.n_leaf_paths(b)  # (a forest, not a stump)
    pairs = pair_values[name]
    if mode == "raw":
        want = pairs.mean(1)
    else:
        fx, fz = B.predict_margin64_host(b, X), B.predict_margin64_host(b, Z)
        want = (_literal_rescale(fx[:, None], fz[None, :])[:, :, None] * pairs).mean(1)
    got = B.treeshap_interventional_host(b, X, Z, mode)
    assert got.shape == X.shape and got.dtype == np.float64 and np.isfinite(got).all()
    diff = float(np.abs(got - want).max())
    print(f"[shap-background] {name} {mode}: max |closed form - enumeration| = {diff:.3e}, max |phi| = "
          f"{np.abs(want).max():.3g}")
    assert np.abs(want).max() > 1e-3
    assert diff <= BRUTE_TOL


def test_repeated_features_occur_on_paths():
    b = FORESTS["grid-edges-mixed-defaults"][0]
    assert any(len({f for _, f, _ in path}) < len(path) for t in b.trees for _, path in B.iter_leaf_paths(t))


@pytest.mark.parametrize("name", list(FORESTS))
def test_local_accuracy_both_modes(name):
    b, X, Z = FORESTS[name]
    fx = B.predict_margin64_host(b, X)
    # the float64 margin is the predictor's margin up to float32 rounding of the running sum
    np.testing.assert_allclose(fx, sf.predict_rowwise(b, X).astype(np.float64), rtol=0, atol=2e-6)
    phi = b.shap_values_interventional(X, Z, device="cpu")
    ev = b.expected_value_interventional(Z)
    assert ev == float(np.mean(B.predict_margin64_host(b, Z)))
    np.testing.assert_allclose(phi.sum(1) + ev, fx, rtol=0, atol=1e-12)
    phi = b.shap_values_interventional(X, Z, model_output="probability", device="cpu")
    ev = b.expected_value_interventional(Z, "probability")
    assert 0.0 < ev < 1.0
    np.testing.assert_allclose(phi.sum(1) + ev, 1.0 / (1.0 + np.exp(-fx)), rtol=0, atol=1e-12)


@pytest.mark.parametrize("mode", MODES)
def test_unused_feature_gets_exactly_zero(mode):
    rng = np.random.default_rng(5)
    b = sf.random_forest(rng, 9, 5, 4, cols=[0, 2, 3, 7])
    X = rng.normal(size=(6, 11)).astype(np.float32)   # wider than the model, too
    Z = rng.normal(size=(4, 9)).astype(np.float32)
    phi = b.shap_values_interventional(X, Z, model_output=mode, device="cpu")
    assert phi.shape == (6, 11)
    unused = [1, 4, 5, 6, 8, 9, 10]
    assert (phi[:, unused] == 0.0).all() and not np.signbit(phi[:, unused]).any()
    assert np.abs(phi[:, [0, 2, 3, 7]]).max() > 1e-3


@pytest.mark.parametrize("mode", MODES)
def test_row_equal_to_the_only_background_row_gives_zeros(mode):
    b, X, _ = FORESTS["grid-edges-mixed-defaults"]
    for r in (0, 5, 20):  # rows with NaN / inf cells among them
        phi = B.treeshap_interventional_host(b, X[r:r + 1], X[r:r + 1], mode)
        assert (phi == 0.0).all()


@pytest.mark.parametrize("mode", MODES)
def test_covers_do_not_matter(mode):
    b, X, Z = FORESTS["random-F8"]
    scaled = sf.make_booster([dataclasses.replace(t, sum_hessian=(t.sum_hessian * np.float32(3.5)).astype(np.float32))
                              for t in b.trees], 8)
    assert not np.array_equal(B.treeshap_host(b, X), B.treeshap_host(scaled, X))  # the path-dependent values do
    a, c = (B.treeshap_interventional_host(m, X, Z, mode) for m in (b, scaled))
    assert a.tobytes() == c.tobytes()
    assert b.expected_value_interventional(Z, mode) == scaled.expected_value_interventional(Z, mode)


@pytest.mark.parametrize("mode", MODES)
def test_stump_only_forest(mode):
    b = sf.make_booster([sf.stump(0.25), sf.stump(-0.5, 3.0)], 3)
    X = np.random.default_rng(1).normal(size=(4, 3)).astype(np.float32)
    phi = B.treeshap_interventional_host(b, X, X[:2], mode)
    assert phi.shape == (4, 3) and (phi == 0.0).all()
    f = np.float64(b.base_margin) + np.float64(np.float32(0.25)) + np.float64(np.float32(-0.5))
    want = f if mode == "raw" else 1.0 / (1.0 + np.exp(-f))
    assert b.expected_value_interventional(X[:2], mode) == pytest.approx(want, rel=1e-15)


def test_equal_margins_take_the_derivative_branch():
    b, X, Z = FORESTS["random-F8"]
    # a background that holds the explained row itself, a copy that differs inside the same leaves, and others
    x = X[2:3].copy()
    twin = x.copy()
    twin[0, np.isfinite(twin[0])] += np.float32(1e-6)
    Zb = np.concatenate([x, twin, Z])
    fx, fz = B.predict_margin64_host(b, x), B.predict_margin64_host(b, Zb)
    assert fz[0] == fx[0] and fz[1] == fx[0] and (fz[2:] != fx[0]).all()
    s = B.probability_rescale(fx[:, None], fz[None, :])
    p = 1.0 / (1.0 + np.exp(-fx[0]))
    assert np.isfinite(s).all() and s[0, 0] == pytest.approx(p * (1.0 - p), rel=1e-12)
    phi = B.treeshap_interventional_host(b, x, Zb, "probability")
    assert np.isfinite(phi).all()
    np.testing.assert_allclose(phi.sum(1) + b.expected_value_interventional(Zb, "probability"), [p], rtol=0, atol=1e-13)


def test_rescale_is_the_quotient_without_its_cancellation():
    rng = np.random.default_rng(3)
    fx, fz = rng.normal(0, 3, 2000), rng.normal(0, 3, 2000)
    fz[:50] = fx[:50]
    got = B.probability_rescale(fx, fz)
    far = np.abs(fx - fz) > 1e-3
    np.testing.assert_allclose(got[far], _literal_rescale(fx, fz)[far], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(got, B.probability_rescale(fz, fx))  # symmetric
    sx = 1.0 / (1.0 + np.exp(-fx))
    # (the derivative as sigmoid(f) sigmoid(-f): 1 - sigmoid(f) loses digits for large f)
    np.testing.assert_allclose(got[:50], (sx / (1.0 + np.exp(fx)))[:50], rtol=1e-15, atol=0)
    # margins one ulp apart: the quotient form is 0 or 2x off, this one is the derivative
    a = np.array([0.75])
    near = B.probability_rescale(a, np.nextafter(a, 2.0))
    np.testing.assert_allclose(near, B.probability_rescale(a, a), rtol=1e-15, atol=0)
    assert np.isfinite(B.probability_rescale(np.array([-800.0, 800.0, 800.0]), np.array([800.0, -800.0, 800.0]))).all()


def test_weight_table():
    W = B.interventional_weights()
    assert W.shape == (16, 16) and (W[0] == 0.0).all()
    assert W[1, 0] == 1.0 and W[1, 1] == 0.5 and W[2, 1] == pytest.approx(1 / 6) and W[15, 0] == pytest.approx(1 / 15)
    assert W[8, 8] == 0.0  # a + b beyond the longest path
    # the weights of a path's x-only and z-only features add up to the leaf swing: a W[a, b] - b W[b, a] = 1 or 0
    for a in range(1, 8):
        for c in range(1, 8):
            assert a * W[a, c] - c * W[c, a] == pytest.approx(0.0, abs=1e-15)
        assert a * W[a, 0] == pytest.approx(1.0)


def test_n_trees_scores_a_prefix():
    b, X, Z = FORESTS["random-F8"]
    got = b.shap_values_interventional(X, Z, n_trees=2, device="cpu")
    assert got.tobytes() == B.treeshap_interventional_host(b.slice(2), X, Z).tobytes()
    assert b.expected_value_interventional(Z, n_trees=2) == b.slice(2).expected_value_interventional(Z)
    assert predict_ops._sliced(b, 2) is predict_ops._sliced(b, 2) and predict_ops._sliced(b, None) is b
    with pytest.raises(ValueError, match="n_trees"):
        b.shap_values_interventional(X, Z, n_trees=99, device="cpu")


def test_inputs_and_outputs_of_the_entry_point():
    b, X, Z = FORESTS["random-F8"]
    want = B.treeshap_interventional_host(b, X, Z)
    got = predict_ops.shap_values_interventional(b, torch.from_numpy(X), torch.from_numpy(Z), device="cpu")
    assert np.asarray(got).tobytes() == want.tobytes()
    assert b.shap_values_interventional(X[:0], Z, device="cpu").shape == (0, 8)
    with pytest.raises(ValueError, match="no rows"):
        b.shap_values_interventional(X, Z[:0], device="cpu")
    with pytest.raises(ValueError, match="no rows"):
        b.expected_value_interventional(Z[:0])
    with pytest.raises(ValueError, match="model needs"):
        b.shap_values_interventional(X[:, :5], Z, device="cpu")
    with pytest.raises(ValueError, match="model needs"):
        b.shap_values_interventional(X, Z[:, :5], device="cpu")
    with pytest.raises(ValueError, match="model_output"):
        b.shap_values_interventional(X, Z, model_output="logit", device="cpu")


def test_long_path_is_refused():
    rng = np.random.default_rng(2)
    b = sf.make_booster([sf.caterpillar(rng, 16, range(16))], 16)
    X = rng.normal(size=(2, 16)).astype(np.float32)
    with pytest.raises(ValueError, match="16 unique features"):
        B.treeshap_interventional_host(b, X, X)


# ------------------------------------------------------------------------------- TreeExplainer
def test_explainer_argument_rules():
    b, X, Z = FORESTS["random-F8"]
    with pytest.raises(ValueError, match="needs a background set"):
        TreeExplainer(b, feature_perturbation="interventional")
    with pytest.raises(ValueError, match="needs a background set"):
        TreeExplainer(b, feature_perturbation="interventional", model_output="probability")
    for fp in ("auto", "tree_path_dependent"):
        with pytest.raises(ValueError, match="probability"):
            TreeExplainer(b, feature_perturbation=fp, model_output="probability")
    for mo in MODES:
        with pytest.raises(ValueError, match="cannot use data"):
            TreeExplainer(b, data=Z, feature_perturbation="tree_path_dependent", model_output=mo)
    with pytest.raises(ValueError, match="feature_perturbation must be"):
        TreeExplainer(b, data=Z, feature_perturbation="marginal")
    with pytest.raises(ValueError, match="model_output must be"):
        TreeExplainer(b, data=Z, model_output="log_loss")
    with pytest.raises(ValueError, match="no rows"):
        TreeExplainer(b, data=Z[:0])
    ex = TreeExplainer(b, data=Z, device="cpu")
    with pytest.raises(ValueError, match="path-dependent only"):
        ex.shap_interaction_values(X)


def test_explainer_without_data_is_unchanged():
    b, X, _ = FORESTS["random-F8"]
    for ex in (TreeExplainer(b, device="cpu"), TreeExplainer(b, None, "tree_path_dependent", "raw", device="cpu")):
        assert ex.feature_perturbation == "tree_path_dependent" and ex.data is None
        assert ex.shap_values(X).tobytes() == np.asarray(b.shap_values(X, device="cpu"), np.float64).tobytes()
        assert ex.expected_value == float(b.expected_value())
        assert ex.shap_interaction_values(X).tobytes() == b.shap_interaction_values(X, device="cpu").tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fp", ("auto", "interventional"))
def test_explainer_with_data(fp, mode):
    from cobalt_smart_lender_ai_amd.explain import force_data

    b, X, Z = FORESTS["random-F8"]
    ex = TreeExplainer(b, data=Z, feature_perturbation=fp, model_output=mode, device="cpu")
    assert ex.feature_perturbation == "interventional" and ex.model_output == mode
    want = B.treeshap_interventional_host(b, X, Z, mode)
    assert ex.shap_values(X).tobytes() == want.tobytes()
    assert ex.expected_value == b.expected_value_interventional(Z, mode)
    e = ex(X)
    assert e.values.tobytes() == want.tobytes() and (e.base_values == ex.expected_value).all()
    fd = force_data(e, 1)
    fx = B.predict_margin64_host(b, X[1:2])[0]
    assert fd["output"] == pytest.approx(fx if mode == "raw" else 1.0 / (1.0 + np.exp(-fx)), abs=1e-12)
    assert len(fd["contributions"]) == 8


def test_dataframe_background_is_reordered_by_name():
    import pandas as pd

    b0, X, Z = FORESTS["random-F8"]
    names = [f"col{i}" for i in range(8)]
    b = B.Booster(list(b0.trees), feature_names=names, num_feature=8, base_score=b0.base_score)
    want = B.treeshap_interventional_host(b, X, Z, "probability")
    shuffled = names[::-1]
    ex = TreeExplainer(b, data=pd.DataFrame(Z, columns=names)[shuffled], model_output="probability", device="cpu")
    assert ex.data.tobytes() == Z.tobytes()
    assert ex.shap_values(pd.DataFrame(X, columns=names)[shuffled]).tobytes() == want.tobytes()
