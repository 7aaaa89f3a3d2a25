"""TreeSHAP interaction values on the host: the path-based NumPy implementation against the literal
subset-enumeration definition, the three properties of the definition on the shipped model, the
explainer API and the ``/explain_interactions`` route (host path)."""
import numpy as np
import pytest
import torch

from cobalt_smart_lender_ai_amd.config import DEPLOYED_FEATURES, ServeConfig
from cobalt_smart_lender_ai_amd.dataio import synth
from cobalt_smart_lender_ai_amd.models import booster as B

UI_ROW = [10000, 36, 300, 660, 700, 1, 2, 2000, 10, 0, 3, 4000, 0, 0, 0, 0, 0, 0, 0, 0]
NAN = float("nan")


def _tree(nodes):
    """nodes: (left, right, feature, threshold or leaf value, default_left, cover) in node order."""
    n = len(nodes)
    parents = np.full(n, B.ROOT_PARENT, np.int32)
    for i, nd in enumerate(nodes):
        if nd[0] != -1:
            parents[nd[0]] = parents[nd[1]] = i
    col = lambda k, dt: np.array([nd[k] for nd in nodes], dtype=dt)  # noqa: E731
    return B.Tree(col(0, np.int32), col(1, np.int32), parents, col(2, np.int32), col(3, np.float32),
                  col(4, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.float32), col(5, np.float32))


def _leaf(v, cover):
    return (-1, -1, 0, v, 0, cover)


def hand_built_booster():
    """5 features, feature 4 never used: a stump (k = 0), a single split (k = 1, missing goes left), and
    a tree whose paths split twice on feature 1 (with both default directions, so NaN leaves every
    merged path) and reach 3 unique features."""
    stump = _tree([_leaf(0.3, 10.0)])
    single = _tree([(1, 2, 0, 0.5, 1, 10.0), _leaf(-0.4, 3.0), _leaf(0.7, 7.0)])
    deep = _tree([
        (1, 2, 1, 1.0, 1, 20.0),          # 0: f1 < 1.0, missing left
        (3, 4, 2, 0.0, 0, 12.0),          # 1: f2 < 0.0, missing right
        (5, 6, 3, 2.5, 1, 8.0),           # 2: f3 < 2.5, missing left
        (7, 8, 1, 0.2, 0, 5.0),           # 3: f1 < 0.2 again, missing right
        _leaf(0.25, 7.0),                 # 4
        _leaf(-0.6, 2.0),                 # 5
        (9, 10, 1, 3.0, 0, 6.0),          # 6: f1 < 3.0 again on the right branch, missing right
        (11, 12, 3, 1.5, 1, 1.5),         # 7: f3 < 1.5, missing left (4 splits, 3 unique features)
        _leaf(-0.9, 3.5),                 # 8
        _leaf(0.45, 4.0),                 # 9
        _leaf(-0.15, 2.0),                # 10
        _leaf(1.1, 0.5),                  # 11
        _leaf(0.8, 1.0),                  # 12
    ])
    return B.Booster([stump, single, deep], num_feature=5, base_score=0.4)


HAND_ROWS = np.array([
    [0.1, 0.1, -1.0, 1.0, 5.0],
    [0.9, 0.5, 1.0, 3.0, -2.0],
    [0.2, 2.0, -0.5, 3.0, 0.0],
    [0.7, 5.0, 0.5, 0.0, 1.0],
    [NAN, 0.1, -1.0, 1.0, 0.0],      # missing on the single split: default left
    [0.3, NAN, -1.0, 3.0, 0.0],      # missing on the twice-split feature: left at the root, right below
    [0.3, 0.1, NAN, NAN, NAN],       # missing right (f2) and, for the cold paths, left (f3)
    [NAN, NAN, NAN, NAN, NAN],
], dtype=np.float32)


@pytest.fixture(scope="module")
def trained_small():
    """A tiny fitted model on 6 features (depth 3: repeated features and unequal covers as they occur)."""
    from cobalt_smart_lender_ai_amd.models import gbdt

    X, y = synth.make_lendingclub(600, seed=5)
    X6 = X[:, [1, 3, 4, 5, 7, 10]].contiguous()
    X6[::7, 2] = NAN
    X6[::5, 0] = NAN
    b = gbdt.train(X6, y, gbdt.GBDTParams(n_estimators=4, max_depth=3, learning_rate=0.3), device="cpu")
    rows = X6[:6].numpy().copy()
    rows[5, :] = NAN
    return b, rows


def _check_against_bruteforce(b, X):
    got = B.treeshap_interactions_host(b, X)
    want = B.shapley_interactions_bruteforce(b, X)
    diff = float(np.abs(got - want).max())
    print(f"max |host - brute force| = {diff:.3e}")
    assert got.shape == (len(X), b.num_feature, b.num_feature) and got.dtype == np.float64
    assert diff <= 1e-10
    return got


def test_host_matches_bruteforce_hand_built():
    b = hand_built_booster()
    ks = sorted({len(e) for t in b.trees for _, e in B.merged_leaf_paths(t)})
    assert ks == [0, 1, 2, 3]                                    # stump, single split, merged paths
    raw = max(len(p) for _, p in B.iter_leaf_paths(b.trees[2]))
    assert raw == 4                                              # 4 splits, 3 unique features: f1 merged
    phi = _check_against_bruteforce(b, HAND_ROWS)
    assert not phi[:, 4, :].any() and not phi[:, :, 4].any()     # the unused feature: exactly zero
    # the rows really take both default directions
    m = B.predict_margin_host(b, HAND_ROWS)
    assert len(set(np.round(m, 6).tolist())) >= 5
    # the properties of the definition, on the same data
    np.testing.assert_allclose(phi.sum(2), B.treeshap_host(b, HAND_ROWS), rtol=0, atol=1e-12)
    np.testing.assert_allclose(phi.sum((1, 2)) + b.expected_value(), m, atol=1e-6)
    assert np.array_equal(phi, phi.transpose(0, 2, 1))


def test_host_matches_bruteforce_trained(trained_small):
    b, rows = trained_small
    assert b.num_feature == 6 and b.num_trees == 4
    _check_against_bruteforce(b, rows)


def test_single_tree_kinds_separately():
    """Each tree of the hand-built model on its own (a mistake that cancels between trees would hide)."""
    full = hand_built_booster()
    for t in full.trees:
        b = B.Booster([t], num_feature=5, base_score=0.5)
        phi = _check_against_bruteforce(b, HAND_ROWS)
        if t.num_nodes == 1:
            assert not phi.any()
        if t.num_nodes == 3:
            off = phi.copy()
            off[:, np.arange(5), np.arange(5)] = 0.0
            assert not off.any() and phi[:, 0, 0].any()          # k = 1: only a diagonal


@pytest.fixture(scope="module")
def shipped_rows():
    X, _ = synth.make_lendingclub(6, seed=9)
    X[0, 5] = NAN
    return torch.cat([X, torch.tensor([UI_ROW], dtype=torch.float32)]).numpy()


@pytest.fixture(scope="module")
def shipped_interactions(reference_booster, shipped_rows):
    return B.treeshap_interactions_host(reference_booster, shipped_rows)


def test_properties_on_shipped_model(reference_booster, shipped_rows, shipped_interactions):
    b, X, phi = reference_booster, shipped_rows, shipped_interactions
    assert phi.shape == (7, 20, 20)
    np.testing.assert_allclose(phi.sum(2), B.treeshap_host(b, X), rtol=1e-9, atol=1e-9)
    m = B.predict_margin_host(b, X).astype(np.float64)
    np.testing.assert_allclose(phi.sum((1, 2)) + b.expected_value(), m, atol=2e-5)
    assert float(np.abs(phi - phi.transpose(0, 2, 1)).max()) <= 1e-12
    off = phi.copy()
    off[:, np.arange(20), np.arange(20)] = 0.0
    assert np.abs(off).max() > 1e-3                              # the model does have interactions


def test_booster_and_ops_dispatch_to_host(reference_booster, shipped_rows, shipped_interactions):
    from cobalt_smart_lender_ai_amd.ops import predict_ops

    got = reference_booster.shap_interaction_values(shipped_rows[5:], device="cpu")
    assert isinstance(got, np.ndarray) and np.array_equal(got, shipped_interactions[5:])
    got = predict_ops.shap_interaction_values(reference_booster, torch.from_numpy(shipped_rows[6:]), device="cpu")
    assert np.array_equal(got, shipped_interactions[6:])


def test_top_interactions_ordering():
    from cobalt_smart_lender_ai_amd.explain import top_interactions

    names = ["a", "b", "c", "d"]
    v = np.zeros((2, 4, 4))
    v[0, 0, 1] = v[0, 1, 0] = 0.5       # (a, b): mean |sum| = (1.0 + 0.0) / 2 = 0.5
    v[1, 2, 3] = v[1, 3, 2] = -1.5      # (c, d): (0 + 3.0) / 2 = 1.5
    v[0, 0, 2] = v[0, 2, 0] = 0.25      # (a, c): 0.25 -- ties with (b, d) below, (a, c) comes first
    v[1, 1, 3] = v[1, 3, 1] = -0.25     # (b, d): 0.25
    v[:, 1, 1] = 9.0                    # the diagonal is no pair
    top = top_interactions(v, names, k=10)
    assert [(t["feature_a"], t["feature_b"]) for t in top] == [("c", "d"), ("a", "b"), ("a", "c"), ("b", "d"),
                                                               ("a", "d"), ("b", "c")]
    assert [t["strength"] for t in top] == [1.5, 0.5, 0.25, 0.25, 0.0, 0.0]
    assert set(top[0]) == {"feature_a", "feature_b", "strength"}
    assert len(top_interactions(v, names, k=2)) == 2
    one = top_interactions(v[1], names, k=1)                     # one matrix [F, F]
    assert one == [{"feature_a": "c", "feature_b": "d", "strength": 3.0}]


def test_tree_explainer_reorders_dataframe_columns(reference_booster, shipped_rows, shipped_interactions):
    import pandas as pd

    from cobalt_smart_lender_ai_amd.explain import TreeExplainer

    ex = TreeExplainer(reference_booster, device="cpu")
    df = pd.DataFrame(shipped_rows[4:], columns=DEPLOYED_FEATURES)
    got = ex.shap_interaction_values(df[DEPLOYED_FEATURES[::-1]])
    assert got.dtype == np.float64 and got.shape == (3, 20, 20)
    assert np.array_equal(got, shipped_interactions[4:])
    assert np.array_equal(ex.shap_interaction_values(shipped_rows[4:]), got)


def test_explain_interactions_route_host_path(reference_booster):
    from fastapi.testclient import TestClient

    from cobalt_smart_lender_ai_amd.serve.app import create_app

    body = dict(zip(DEPLOYED_FEATURES, [float(v) for v in UI_ROW]))
    app = create_app(ServeConfig(device="cpu"), booster=reference_booster)
    with TestClient(app) as c:
        before = c.post("/predict", json=body)
        r = c.post("/explain_interactions", json=body)
        after = c.post("/predict", json=body)
        metrics = c.get("/metrics").text
    assert r.status_code == 200, r.text
    j = r.json()
    assert set(j) == {"features", "base_value", "shap_values", "interaction_values", "top_pairs"}
    assert j["features"] == DEPLOYED_FEATURES
    inter = np.array(j["interaction_values"])
    assert inter.shape == (20, 20)
    np.testing.assert_allclose(inter.sum(1), j["shap_values"], rtol=0, atol=1e-12)
    assert np.array_equal(inter, inter.T)
    assert len(j["top_pairs"]) == 10 and set(j["top_pairs"][0]) == {"feature_a", "feature_b", "strength"}
    s = [t["strength"] for t in j["top_pairs"]]
    assert s == sorted(s, reverse=True) and s[0] > 0
    a, b_ = DEPLOYED_FEATURES.index(j["top_pairs"][0]["feature_a"]), DEPLOYED_FEATURES.index(j["top_pairs"][0]["feature_b"])
    assert a < b_ and abs(abs(2 * inter[a, b_]) - s[0]) < 1e-15
    # /predict is untouched: same response before and after, and the same attribution and base value
    assert before.status_code == 200 and before.json() == after.json()
    p = before.json()
    assert j["base_value"] == p["base_value"]
    np.testing.assert_allclose(j["shap_values"], p["shap_values"], rtol=1e-9, atol=1e-9)
    assert 'cobalt_requests_total{route="/explain_interactions",status="200"} 1.0' in metrics
    assert 'cobalt_scored_rows_total{route="/explain_interactions"} 1.0' in metrics
    # the same body rules as /predict: the two aliased fields are required under their aliases
    bad = dict(body)
    bad["application_type_Joint_App"] = bad.pop("application_type_Joint App")
    with TestClient(app) as c:
        assert c.post("/explain_interactions", json=bad).status_code == 422
