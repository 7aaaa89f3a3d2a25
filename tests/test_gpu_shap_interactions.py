"""GPU (gfx950) TreeSHAP interaction values against the host oracle (``treeshap_interactions_host``, itself
checked against the subset-enumeration definition in test_shap_interactions_cpu.py)."""
import numpy as np
import pytest
import torch

from cobalt_smart_lender_ai_amd.dataio import synth
from cobalt_smart_lender_ai_amd.models import booster as B
from cobalt_smart_lender_ai_amd.models import gbdt
from cobalt_smart_lender_ai_amd.ops import predict_ops

pytestmark = pytest.mark.gpu

UI_ROW = [10000, 36, 300, 660, 700, 1, 2, 2000, 10, 0, 3, 4000, 0, 0, 0, 0, 0, 0, 0, 0]
TOL = dict(rtol=1e-9, atol=1e-9)  # the project's GPU-vs-oracle SHAP tolerance


def _fit(n_trees, depth, cols=None, seed=3, device="cuda"):
    X, y = synth.make_lendingclub(2000, seed=seed)
    if cols is not None:
        X = X[:, cols].contiguous()
    X[::11, 1] = float("nan")
    p = gbdt.GBDTParams(n_estimators=n_trees, max_depth=depth, learning_rate=0.3, gamma=0.0)
    return gbdt.train(X.to(device), y.to(device), p, device=device), X


@pytest.fixture(scope="module")
def small_model():
    return _fit(5, 4)


@pytest.fixture(scope="module")
def deep_model():
    """12 trees of depth 7: more paths than one chunk of 256 and not a multiple of it."""
    b, X = _fit(12, 7)
    n_paths = sum(int(t.is_leaf.sum()) for t in b.trees)
    assert n_paths > 256 and n_paths % 256 != 0
    return b, X


@pytest.fixture(scope="module")
def deep_reference(deep_model):
    b, X = deep_model
    return B.treeshap_interactions_host(b, X[:40].numpy())


def _gpu(b, X):
    return b.shap_interaction_values(X.cuda())


def test_shipped_model_matches_host_oracle(reference_booster):
    b = reference_booster
    X, _ = synth.make_lendingclub(6, seed=9)
    X[0, 5] = float("nan")
    X = torch.cat([X, torch.tensor([UI_ROW], dtype=torch.float32)])
    got = _gpu(b, X)
    assert got.dtype == torch.float64 and tuple(got.shape) == (7, 20, 20)
    want = B.treeshap_interactions_host(b, X.numpy())
    g = got.cpu().numpy()
    print(f"max |gpu - host| = {np.abs(g - want).max():.3e}")
    np.testing.assert_allclose(g, want, **TOL)
    phi = b.shap_values(X.cuda()).cpu().numpy()
    np.testing.assert_allclose(g.sum(2), phi, **TOL)
    assert np.array_equal(g, g.transpose(0, 2, 1))


def test_small_model_300_rows(small_model):
    """300 rows: past SHAP_ROWS_MIN (the SHAP values behind the diagonal come from the table kernel) and
    no multiple of a block size."""
    b, X = small_model
    assert 300 >= predict_ops.SHAP_ROWS_MIN
    got = _gpu(b, X[:300]).cpu().numpy()
    want = B.treeshap_interactions_host(b, X[:300].numpy())
    print(f"max |gpu - host| = {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, **TOL)
    assert np.array_equal(got, got.transpose(0, 2, 1))


def test_multi_chunk_model(deep_model, deep_reference):
    b, X = deep_model
    got = _gpu(b, X[:40]).cpu().numpy()
    print(f"max |gpu - host| = {np.abs(got - deep_reference).max():.3e}")
    np.testing.assert_allclose(got, deep_reference, **TOL)
    np.testing.assert_allclose(got.sum(2), b.shap_values(X[:40].cuda()).cpu().numpy(), **TOL)
    assert np.array_equal(got, got.transpose(0, 2, 1))


def test_row_is_bit_identical_across_batches_and_variants(deep_model, deep_reference, monkeypatch):
    b, X = deep_model
    Xg = X[:300].cuda()
    alone = _gpu(b, Xg[17:18])[0]
    results = {"rows 0..39": _gpu(b, Xg[:40])[17], "300 rows": _gpu(b, Xg)[17],
               "last of 18": _gpu(b, Xg[:18])[17]}
    monkeypatch.setattr(predict_ops, "_FORCE_LONG_PATH_INTERACTIONS", True)
    results["long-path variant, alone"] = _gpu(b, Xg[17:18])[0]
    results["long-path variant, rows 0..39"] = _gpu(b, Xg[:40])[17]
    for name, r in results.items():
        assert torch.equal(alone, r), name
    np.testing.assert_allclose(alone.cpu().numpy(), deep_reference[17], **TOL)


def test_one_row_and_no_rows(small_model):
    b, X = small_model
    one = _gpu(b, X[5:6])
    assert tuple(one.shape) == (1, 20, 20)
    np.testing.assert_allclose(one.cpu().numpy(), B.treeshap_interactions_host(b, X[5:6].numpy()), **TOL)
    none = _gpu(b, X[:0])
    assert tuple(none.shape) == (0, 20, 20) and none.dtype == torch.float64
    assert b.shap_interaction_values(np.zeros((0, 20), np.float32), device="cuda").shape == (0, 20, 20)


def test_four_features():
    b, X = _fit(4, 4, cols=[1, 3, 4, 7], device="cpu")  # (fitted on the host; explained on the GPU)
    got = _gpu(b, X[:33]).cpu().numpy()
    assert got.shape == (33, 4, 4)
    np.testing.assert_allclose(got, B.treeshap_interactions_host(b, X[:33].numpy()), **TOL)


def _widen(b, X, F):
    """The 20-feature model on F features: feature f moves to column F - 39 + 2 f (in order, the last
    column included), the other columns are noise the model never reads."""
    where = [F - 39 + 2 * f for f in range(b.num_feature)]
    trees = [B.Tree(t.left_children, t.right_children, t.parents,
                    np.where(t.is_leaf, 0, np.asarray(where, np.int32)[t.split_indices]).astype(np.int32),
                    t.split_conditions, t.default_left, t.base_weights, t.loss_changes, t.sum_hessian)
             for t in b.trees]
    Xw = torch.randn((X.shape[0], F), generator=torch.Generator().manual_seed(F))
    Xw[:, where] = X
    return B.Booster(trees, num_feature=F, base_score=b.base_score), Xw, where


def test_widest_model(small_model):
    b, X = small_model
    F = predict_ops.SHAP_INT_MAX_F
    assert F == 48 == predict_ops._native.lib().cobalt_treeshap_interactions_max_f()
    bw, Xw, where = _widen(b, X[:70], F)
    got = _gpu(bw, Xw).cpu().numpy()
    assert got.shape == (70, F, F)
    np.testing.assert_allclose(got, B.treeshap_interactions_host(bw, Xw.numpy()), **TOL)
    # the same numbers as the 20-feature model, moved; exact zeros everywhere else
    narrow = _gpu(b, X[:70]).cpu().numpy()
    assert np.array_equal(got[np.ix_(range(70), where, where)], narrow)
    unused = sorted(set(range(F)) - set(where))
    assert not got[:, unused, :].any() and not got[:, :, unused].any()


def test_too_wide_model_is_refused_before_any_launch(small_model):
    b, X = small_model
    F = predict_ops.SHAP_INT_MAX_F + 1
    bw, Xw, _ = _widen(b, X[:4], F)
    with pytest.raises(ValueError, match=f"limit of {predict_ops.SHAP_INT_MAX_F} features"):
        bw.shap_interaction_values(Xw.cuda())
    assert "_gpu_cache" not in bw.__dict__  # refused on the host: no forest was packed, nothing launched
    # the native entry point refuses it too, with an error code and no launch
    rc = predict_ops._native.lib().cobalt_treeshap_interactions(None, 4, F, F, None, None, None, 0, 3, None, None,
                                                               None)
    assert rc == -5


def _chain_tree(feats, seed):
    """A caterpillar tree: node i splits on feats[i], its left child is a leaf, its right child the next
    split -- the last leaf's path holds every feature once."""
    rng = np.random.default_rng(seed)
    k = len(feats)
    n = 2 * k + 1
    left = np.full(n, -1, np.int32)
    right = np.full(n, -1, np.int32)
    parents = np.full(n, B.ROOT_PARENT, np.int32)
    feat = np.zeros(n, np.int32)
    cond = rng.normal(size=n).astype(np.float32)      # leaf values, overwritten at the splits
    dleft = np.zeros(n, np.uint8)
    cover = np.zeros(n, np.float32)
    cover[0] = 1000.0
    for i in range(k):                                # split i = node 2 i, its leaf = node 2 i + 1
        s = 2 * i
        left[s], right[s] = s + 1, s + 2
        parents[s + 1] = parents[s + 2] = s
        feat[s] = feats[i]
        cond[s] = rng.normal() * 0.5
        dleft[s] = i % 2
        cover[s + 1] = np.float32(cover[s] * rng.uniform(0.2, 0.6))
        cover[s + 2] = cover[s] - cover[s + 1]
    z = np.zeros(n, np.float32)
    return B.Tree(left, right, parents, feat, cond, dleft, z, z, cover)


def test_long_paths_take_the_long_path_variant():
    """Paths of 8 to 11 unique features (more than the unrolled short-path variant holds)."""
    F = 12
    rng = np.random.default_rng(1)
    trees = [_chain_tree(rng.permutation(F)[:k].tolist(), seed=k) for k in (11, 9, 8, 3)]
    b = B.Booster(trees, num_feature=F, base_score=0.5)
    X = torch.randn((37, F), generator=torch.Generator().manual_seed(2))
    X[3, 4] = float("nan")
    X[9, :] = float("nan")
    got = _gpu(b, X).cpu().numpy()
    assert predict_ops.gpu_forest(b, torch.device("cuda", torch.cuda.current_device()), None, True).max_len == 11
    want = B.treeshap_interactions_host(b, X.numpy())
    print(f"max |gpu - host| = {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, **TOL)
    np.testing.assert_allclose(got.sum(2), b.shap_values(X.cuda()).cpu().numpy(), **TOL)
    assert np.array_equal(got, got.transpose(0, 2, 1))
