"""Interventional TreeSHAP on the GPU (csrc/shapbg.hip) against the host oracle
``treeshap_interventional_host`` (itself checked against subset enumeration in test_shap_background_cpu.py).

Tolerance: ``TOL`` = rtol = atol = 1e-9, the project's GPU-vs-oracle SHAP tolerance (``TOL`` in
test_gpu_shap_interactions.py), in margin and in probability mode.
"""
import numpy as np
import pytest
import torch

import scoring_forests as sf
from cobalt_smart_lender_ai_amd.dataio import synth
from cobalt_smart_lender_ai_amd.explain import TreeExplainer
from cobalt_smart_lender_ai_amd.models import booster as B
from cobalt_smart_lender_ai_amd.models import gbdt
from cobalt_smart_lender_ai_amd.ops import predict_ops

pytestmark = pytest.mark.gpu

UI_ROW = [10000, 36, 300, 660, 700, 1, 2, 2000, 10, 0, 3, 4000, 0, 0, 0, 0, 0, 0, 0, 0]
TOL = dict(rtol=1e-9, atol=1e-9)  # the project's GPU-vs-oracle SHAP tolerance
MODES = ("raw", "probability")
U32 = 2.0 ** -24                  # unit roundoff of float32


def _gpu(b, X, Z, mode="raw"):
    got = b.shap_values_interventional(torch.as_tensor(X).cuda(), torch.as_tensor(Z).cuda(), model_output=mode)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.is_cuda
    return got.cpu().numpy()


def _check(b, X, Z, mode, want=None):
    want = B.treeshap_interventional_host(b, X, Z, mode) if want is None else want
    got = _gpu(b, X, Z, mode)
    assert got.shape == want.shape
    print(f"[shap-background] {mode} N={len(X)} B={len(Z)}: max |gpu - host| = {np.abs(got - want).max():.3e}, "
          f"max |phi| = {np.abs(want).max():.3g}")
    np.testing.assert_allclose(got, want, **TOL)
    return got


def _margin32_bound(b):
    """Bound on |float32 running sum - float64 sum| of the base margin and one leaf per tree: (n - 1) u sum |x_i|
    for n terms, with the largest |leaf| of every tree."""
    s = abs(b.base_margin) + sum(float(np.abs(t.split_conditions[t.is_leaf]).max()) for t in b.trees)
    return b.num_trees * U32 * s


@pytest.mark.parametrize("mode", MODES)
def test_shipped_model_matches_host_oracle(reference_booster, mode):
    b = reference_booster
    X, _ = synth.make_lendingclub(11, seed=9)
    X[0, 5] = float("nan")
    X, Z = torch.cat([X[:6], torch.tensor([UI_ROW], dtype=torch.float32)]).numpy(), X[6:].numpy()
    assert X.shape == (7, 20) and Z.shape == (5, 20)
    got = _check(b, X, Z, mode)
    # local accuracy against the predictor's float32 margins
    m = sf.predict_rowwise(b, X).astype(np.float64)
    ev = b.expected_value_interventional(Z, mode)
    if mode == "raw":
        np.testing.assert_allclose(got.sum(1) + ev, m, rtol=0, atol=_margin32_bound(b) + 1e-9)
    else:
        np.testing.assert_allclose(got.sum(1) + ev, 1 / (1 + np.exp(-m)), rtol=0, atol=0.25 * _margin32_bound(b) + 1e-9)


@pytest.fixture(scope="module")
def many_paths():
    """A forest of 515 leaf paths (more than 256, not a multiple of 256), 300 rows, 65 background rows and the
    host values per (background size, mode), computed once."""
    rng = np.random.default_rng(41)
    b = sf.forest_with_paths(rng, 7, 515)
    assert sf.n_leaf_paths(b) == 515
    X = rng.normal(size=(300, 7)).astype(np.float32)
    Z = rng.normal(size=(65, 7)).astype(np.float32)
    X[rng.random(X.shape) < 0.05] = np.nan
    Z[rng.random(Z.shape) < 0.05] = np.nan
    ref = {(nb, mode): B.treeshap_interventional_host(b, X, Z[:nb], mode) for nb in (1, 2, 33, 65) for mode in MODES}
    return b, X, Z, ref


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nb", (1, 2, 33, 65))
@pytest.mark.parametrize("n", (1, 7, 300))
def test_batch_and_background_sizes(many_paths, n, nb, mode):
    b, X, Z, ref = many_paths
    _check(b, X[:n], Z[:nb], mode, ref[nb, mode][:n])


@pytest.mark.parametrize("mode", MODES)
def test_background_spans_several_tiles(many_paths, mode, monkeypatch):
    b, X, Z, ref = many_paths
    whole = _gpu(b, X[:40], Z, mode)
    monkeypatch.setattr(predict_ops, "_FORCE_BG_TILE", 16)   # 65 rows: four tiles and a last one of 1 row
    tiled = _check(b, X[:40], Z, mode, ref[65, mode][:40])
    monkeypatch.setattr(predict_ops, "_FORCE_BG_TILE", 4)    # 33 rows: eight tiles and a last one of 1 row
    _check(b, X[:40], Z[:33], mode, ref[33, mode][:40])
    np.testing.assert_allclose(tiled, whole, rtol=1e-12, atol=1e-13)  # (another summation order, the same values)


@pytest.mark.parametrize("mode", MODES)
def test_determinism_and_batch_independence(many_paths, mode):
    b, X, Z, _ = many_paths
    a = _gpu(b, X, Z, mode)
    c = _gpu(b, X, Z, mode)
    assert a.tobytes() == c.tobytes()
    alone = _gpu(b, X[:1], Z, mode)
    assert alone[0].tobytes() == a[0].tobytes()
    shifted = _gpu(b, np.concatenate([X[100:], X[:100]]), Z, mode)
    assert shifted[200].tobytes() == a[0].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_local_accuracy_on_the_gpu(many_paths, mode):
    b, X, Z, _ = many_paths
    got = _gpu(b, X, Z, mode)
    m = sf.predict_rowwise(b, X).astype(np.float64)
    ev = b.expected_value_interventional(Z, mode)
    bound = _margin32_bound(b)
    if mode == "raw":
        np.testing.assert_allclose(got.sum(1) + ev, m, rtol=0, atol=bound + 1e-9)
    else:
        np.testing.assert_allclose(got.sum(1) + ev, 1 / (1 + np.exp(-m)), rtol=0, atol=0.25 * bound + 1e-9)


@pytest.mark.parametrize("mode", MODES)
def test_fifteen_unique_features_on_a_path(mode):
    rng = np.random.default_rng(8)
    b = sf.make_booster([sf.caterpillar(rng, 15, range(16)), sf.caterpillar(rng, 15, range(16)),
                         sf.caterpillar(rng, 9, range(16)), sf.random_tree(rng, 16, 4), sf.stump(0.1)], 16)
    assert sf.max_unique_path(b) == 15
    X = rng.normal(0.0, 0.7, size=(19, 16)).astype(np.float32)
    Z = rng.normal(0.0, 0.7, size=(11, 16)).astype(np.float32)
    X[3, 2] = Z[1, 4] = np.nan
    _check(b, X, Z, mode)


@pytest.mark.parametrize("mode", MODES)
def test_edge_rows_on_the_threshold_grid(mode):
    rng = np.random.default_rng(13)
    b = sf.random_forest(rng, 6, 8, 5, grid=sf.THRESHOLD_GRID)
    _check(b, sf.edge_rows(rng, 70, 6), sf.edge_rows(rng, 33, 6), mode)


@pytest.mark.parametrize("mode", MODES)
def test_wider_x_and_strided_rows(mode):
    rng = np.random.default_rng(17)
    b = sf.random_forest(rng, 6, 5, 4)
    Xw = rng.normal(size=(37, 9)).astype(np.float32)   # three columns the model does not have
    Z = rng.normal(size=(10, 6)).astype(np.float32)
    got = _check(b, Xw, Z, mode)
    assert got.shape == (37, 9) and (got[:, 6:] == 0.0).all()
    # row-strided views of wider buffers, straight into the launcher
    Xbuf = torch.full((37, 13), 7.0, dtype=torch.float32, device="cuda")
    Zbuf = torch.full((10, 8), -3.0, dtype=torch.float32, device="cuda")
    Xbuf[:, :9] = torch.from_numpy(Xw).cuda()
    Zbuf[:, :6] = torch.from_numpy(Z).cuda()
    Xv, Zv = Xbuf[:, :9], Zbuf[:, :6]
    assert Xv.stride(0) == 13 and Zv.stride(0) == 8
    phi = torch.empty((37, 9), dtype=torch.float64, device="cuda")
    predict_ops.treeshap_interventional_gpu(b, Xv, Zv, phi, probability=(mode == "probability"))
    assert phi.cpu().numpy().tobytes() == got.tobytes()


def test_stumps_empty_batch_and_numpy_input():
    rng = np.random.default_rng(19)
    b = sf.make_booster([sf.stump(0.25), sf.stump(-0.5, 3.0)], 3)
    X = rng.normal(size=(5, 3)).astype(np.float32)
    for mode in MODES:
        assert (_gpu(b, X, X[:2], mode) == 0.0).all()
    b = sf.random_forest(rng, 5, 4, 4)
    X = rng.normal(size=(6, 5)).astype(np.float32)
    out = b.shap_values_interventional(X, X[:3], device="cuda")
    assert isinstance(out, np.ndarray) and out.dtype == np.float64
    np.testing.assert_allclose(out, B.treeshap_interventional_host(b, X, X[:3]), **TOL)
    empty = b.shap_values_interventional(torch.from_numpy(X[:0]).cuda(), torch.from_numpy(X).cuda())
    assert tuple(empty.shape) == (0, 5) and empty.dtype == torch.float64
    with pytest.raises(ValueError, match="no rows"):
        b.shap_values_interventional(torch.from_numpy(X).cuda(), torch.from_numpy(X[:0]).cuda())
    np.testing.assert_allclose(b.shap_values_interventional(X, X[:3], n_trees=2, device="cuda"),
                               B.treeshap_interventional_host(b.slice(2), X, X[:3]), **TOL)


def test_limits_are_refused_before_any_launch():
    rng = np.random.default_rng(29)
    b = sf.make_booster([sf.caterpillar(rng, 16, range(17))], 17)
    assert sf.max_unique_path(b) == 16
    X = torch.from_numpy(rng.normal(size=(4, 17)).astype(np.float32)).cuda()
    phi = torch.full((4, 17), 123.0, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="16 unique features"):
        predict_ops.treeshap_interventional_gpu(b, X, X, phi)
    assert (phi == 123.0).all()
    b = sf.random_forest(rng, 4, 2, 3)
    wide = torch.zeros((2, predict_ops.SHAP_BG_MAX_F + 1), dtype=torch.float32, device="cuda")
    assert predict_ops.SHAP_BG_MAX_F == predict_ops._native.lib().cobalt_shapbg_max_f()
    assert predict_ops.SHAP_BG_MAX_TILE == predict_ops._native.lib().cobalt_shapbg_max_tile()
    phi = torch.full(tuple(wide.shape), 123.0, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="columns exceed"):
        predict_ops.treeshap_interventional_gpu(b, wide, wide[:, :4], phi)
    assert (phi == 123.0).all()
    with pytest.raises(ValueError, match="model needs"):
        predict_ops.treeshap_interventional_gpu(b, wide[:, :3], wide[:, :4], phi[:, :3].contiguous())


def test_widest_x(many_paths):
    b, X, Z, ref = many_paths
    Xw = np.zeros((5, predict_ops.SHAP_BG_MAX_F), np.float32)
    Xw[:, :7] = X[:5]
    got = _gpu(b, Xw, Z[:33], "probability")
    np.testing.assert_allclose(got[:, :7], ref[33, "probability"][:5], **TOL)
    assert (got[:, 7:] == 0.0).all()


def test_explainer_probability_end_to_end():
    X, y = synth.make_lendingclub(1500, seed=5)
    X[::9, 2] = float("nan")
    clf = gbdt.GBDTClassifier(n_estimators=8, max_depth=4, learning_rate=0.3, device="cuda").fit(X.numpy(), y.numpy())
    b = clf.get_booster()
    Xe, Z = X[:50].numpy(), X[1000:1040].numpy()
    ex = TreeExplainer(clf, data=Z, model_output="probability", device="cuda")
    phi = ex.shap_values(Xe)
    assert phi.shape == Xe.shape and phi.dtype == np.float64
    np.testing.assert_allclose(phi, B.treeshap_interventional_host(b, Xe, Z, "probability"), **TOL)
    assert ex.expected_value == pytest.approx(float(np.mean(1 / (1 + np.exp(-B.predict_margin64_host(b, Z))))), rel=1e-14)
    # the values explain the float64 probability of the path margins exactly ...
    p64 = 1 / (1 + np.exp(-B.predict_margin64_host(b, Xe)))
    np.testing.assert_allclose(phi.sum(1) + ex.expected_value, p64, rtol=0, atol=1e-12)
    # ... and the classifier's float32 predict_proba up to the float32 rounding of its margin sum (sigmoid has
    # slope <= 1/4) and of the probability itself: the float32 exp, add, divide and the result, 4 roundings of
    # values <= 1
    proba = clf.predict_proba(Xe)[:, 1].astype(np.float64)
    gap = float(np.abs(phi.sum(1) + ex.expected_value - proba).max())
    bound = 0.25 * _margin32_bound(b) + 4 * U32
    print(f"[shap-background] max |sum phi + expected_value - predict_proba| = {gap:.3e} (bound {bound:.3e})")
    assert gap <= bound
    raw = TreeExplainer(clf, data=Z, device="cuda")
    m64 = B.predict_margin64_host(b, Xe)
    np.testing.assert_allclose(raw.shap_values(Xe).sum(1) + raw.expected_value, m64, rtol=0, atol=1e-12)
