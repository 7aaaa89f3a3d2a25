"""Leaf-index prediction (``predict_leaf`` / ``apply``) and leaf refresh (``refresh``) on the host: the
definitions ``predict_leaf_host`` / ``refresh_host`` that the kernels of csrc/refresh.hip must match.

What is checked against what:
  leaf indices ........ a row-by-row walk written here; summing the leaf values through the indices in
                        float32 reproduces ``predict_margin_host`` bit for bit
  fixed point ......... a refresh of a host-trained model on its own training rows sees the integers the trainer
                        saw: leaf values and ``sum_hessian`` come back bit for bit
  exact arithmetic .... node sums against an unquantised float64 recomputation, within the quantiser's step
  refresh_leaf=False .. margins unchanged, covers of the new population
  edges, interface .... unreached leaves, one row, one class, zero weights, min_child_weight, reg_alpha, refusals
"""
import math

import numpy as np
import pytest

import scoring_forests as sf
from cobalt_smart_lender_ai_amd import explain
from cobalt_smart_lender_ai_amd.models import booster as B
from cobalt_smart_lender_ai_amd.models import gbdt, gbdt_host
from cobalt_smart_lender_ai_amd.models.booster import Booster


# ------------------------------------------------------------------------------------ helpers
def leaf_rowwise(b, X, n_trees=None):
    """The obvious walk, one row and one tree at a time: the node id where it ends."""
    X = np.asarray(X, np.float32)
    trees = b.trees[: (b.num_trees if n_trees is None else n_trees)]
    out = np.empty((X.shape[0], len(trees)), np.int32)
    for r in range(X.shape[0]):
        for i, t in enumerate(trees):
            j = 0
            while t.left_children[j] != -1:
                v = X[r, t.split_indices[j]]
                left = bool(t.default_left[j]) if np.isnan(v) else bool(v < t.split_conditions[j])
                j = int(t.left_children[j] if left else t.right_children[j])
            out[r, i] = j
    return out


def path_sums(t, leaf, a):
    """Per node, the sum of ``a`` over the rows whose root-to-leaf path holds the node (``a`` int64: exact;
    float64: ``math.fsum``)."""
    members = [[] for _ in range(t.num_nodes)]
    for r, j in enumerate(leaf):
        j = int(j)
        while True:
            members[j].append(r)
            if t.parents[j] == B.ROOT_PARENT:
                break
            j = int(t.parents[j])
    if a.dtype.kind == "i":
        return np.array([int(a[m].sum()) for m in members], np.int64), np.array([len(m) for m in members])
    return np.array([math.fsum(a[m]) for m in members], np.float64), np.array([len(m) for m in members])


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def labelled(rng, b, n, flip=0.3):
    X = rng.normal(size=(n, b.num_feature)).astype(np.float32)
    X[rng.random(X.shape) < 0.05] = np.nan
    p = B.sigmoid32(B.predict_margin_host(b, X))
    y = (rng.random(n) < np.where(rng.random(n) < flip, 0.5, p)).astype(np.float32)
    return X, y


def hand_forests():
    rng = np.random.default_rng(20260601)
    return {
        "random": sf.random_forest(rng, 8, 12, 5, grid=sf.THRESHOLD_GRID),
        "grown": sf.make_booster([sf.grown_tree(rng, 6, 9, 6, grid=sf.THRESHOLD_GRID) for _ in range(5)], 6),
        "caterpillar-12": sf.make_booster([sf.caterpillar(rng, 12, range(12), grid=sf.THRESHOLD_GRID)
                                           for _ in range(3)], 12),
        "stump": sf.make_booster([sf.stump(0.2), sf.stump(-0.1)], 3),
        "zero-cover": sf.make_booster([sf.zero_cover_tree(rng), sf.zero_cover_tree(rng, 1, 0, "right")], 2),
    }


FORESTS = hand_forests()


def trained():
    rng = np.random.default_rng(7)
    X = rng.normal(size=(4096, 8)).astype(np.float32)
    X[rng.random(X.shape) < 0.03] = np.nan
    z = np.nan_to_num(X)
    y = (z[:, 0] + 0.5 * z[:, 1] * z[:, 2] + rng.normal(size=4096) > 0.8).astype(np.float32)
    params = dict(n_estimators=10, max_depth=4, learning_rate=0.3, subsample=1.0, scale_pos_weight=3.0,
                  random_state=11)
    return gbdt.train(X, y, params, device="cpu"), X, y


TRAINED = trained()


# ------------------------------------------------------------------------------- 1 leaf index
@pytest.mark.parametrize("name", list(FORESTS))
def test_leaf_index_equals_rowwise_walk(name):
    b = FORESTS[name]
    X = sf.edge_rows(np.random.default_rng(1), 200, b.num_feature)
    got = B.predict_leaf_host(b, X)
    assert got.dtype == np.int32 and got.shape == (200, b.num_trees)
    np.testing.assert_array_equal(got, leaf_rowwise(b, X))
    for i, t in enumerate(b.trees):
        assert (t.left_children[got[:, i]] == -1).all()
    if name == "stump":
        assert (got == 0).all()  # the root is the leaf
    # the leaf values through the indices, summed in float32 in tree order: the margin, bit for bit
    acc = np.full(X.shape[0], np.float32(b.base_margin), np.float32)
    for i, t in enumerate(b.trees):
        acc = (acc + t.split_conditions[got[:, i]]).astype(np.float32)
    np.testing.assert_array_equal(bits(acc), bits(B.predict_margin_host(b, X)))
    # the public entry point and a prefix of the trees
    np.testing.assert_array_equal(b.predict_leaf(X, device="cpu"), got)
    k = b.num_trees // 2
    np.testing.assert_array_equal(b.predict_leaf(X, device="cpu", n_trees=k), got[:, :k])


# ------------------------------------------------------------------------------ 2 fixed point
def test_refresh_of_a_trained_model_on_its_rows_is_a_fixed_point():
    """The trainer's integers are the refresh's integers (same margins, same quantiser, same dither), so leaf
    values and ``sum_hessian`` are bit-identical. ``loss_changes``: the same quantity in another order of fp64
    operations (the trainer's ``calc_gain_pair`` has one division). ``base_weights`` is DEFINED differently: the
    trainer stores ``float32(weight * eta)`` (XGBoost's hist updater does), the refresh stores ``float32(weight)``
    (XGBoost's refresh updater does, and the definition of ``refresh_host``); it is checked against that
    definition from the node sums, and against the trained value through ``eta``."""
    bst, X, y = TRAINED
    sums = []
    new, margin = B.refresh_host(bst, X, y, node_sums=sums)
    p = B.refresh_params(bst, {})
    assert p["scale_pos_weight"] == 3.0 and p["eta"] == 0.3 and p["seed"] == 11
    gscale, hscale = gbdt_host.quant_scales(3.0, 17)
    lam, mcw = 1.0, 1.0
    for t, (old, ref) in enumerate(zip(bst.trees, new.trees)):
        np.testing.assert_array_equal(old.left_children, ref.left_children)
        np.testing.assert_array_equal(bits(old.split_conditions), bits(ref.split_conditions), err_msg=f"tree {t}")
        np.testing.assert_array_equal(bits(old.sum_hessian), bits(ref.sum_hessian), err_msg=f"tree {t}")
        G = sums[t][:, 0].astype(np.float64) * (1.0 / gscale)
        H = sums[t][:, 1].astype(np.float64) * (1.0 / hscale)
        w = np.array([gbdt_host._calc_weight(g, h, lam, 0.0, mcw) for g, h in zip(G, H)])
        np.testing.assert_array_equal(bits(ref.base_weights), bits(w.astype(np.float32)))
        np.testing.assert_array_equal(bits(old.base_weights), bits((w * 0.3).astype(np.float32)))
        gain = gbdt_host._calc_gain(G, H, lam, 0.0, mcw)
        for j in np.nonzero(~old.is_leaf)[0]:
            gl, gr = gain[old.left_children[j]], gain[old.right_children[j]]
            tol = np.spacing(np.abs(old.loss_changes[j])) + 4 * 2.0 ** -52 * (gl + gr + gain[j])
            assert abs(float(ref.loss_changes[j]) - float(old.loss_changes[j])) <= tol, (t, j)
        assert (ref.loss_changes[old.is_leaf] == 0).all()
    np.testing.assert_array_equal(bits(margin), bits(B.predict_margin_host(bst, X)))


# --------------------------------------------------------------------- 3 exact-arithmetic bound
@pytest.mark.parametrize("grad_bits", [17, 25])
def test_node_sums_are_within_the_quantiser_step_of_fp64(grad_bits):
    bst = TRAINED[0]
    rng = np.random.default_rng(3)
    X, y = labelled(rng, bst, 3000)
    sw = rng.uniform(0.25, 2.0, size=3000).astype(np.float32)
    sums = []
    new, _ = B.refresh_host(bst, X, y, sw, node_sums=sums, grad_bits=grad_bits)
    wt = B.refresh_row_weights(y, sw, 3.0)
    gscale, hscale = gbdt_host.quant_scales(float(wt.max()), grad_bits)
    stages = B.staged_margins_host(new, X)
    leaf = leaf_rowwise(new, X)
    for t, tree in enumerate(new.trees):
        m = (stages[t - 1] if t else np.full(len(y), np.float32(new.base_margin))).astype(np.float64)
        pr = 1.0 / (1.0 + np.exp(-m))
        g = (pr - y) * wt.astype(np.float64)
        h = np.maximum(pr * (1.0 - pr), 1e-16) * wt.astype(np.float64)
        Gx, cnt = path_sums(tree, leaf[:, t], g)
        Hx, _ = path_sums(tree, leaf[:, t], h)
        Hq = tree.sum_hessian.astype(np.float64)
        Gq = sums[t][:, 0] / gscale
        assert (np.abs(Hq - Hx) <= cnt / hscale + 2.0 ** -24 * Hx).all(), t
        assert (np.abs(Gq - Gx) <= cnt / gscale + 2.0 ** -24 * np.abs(Gx)).all(), t


# ------------------------------------------------------------------------ 4 refresh_leaf=False
def test_refresh_leaf_false_keeps_predictions_and_moves_covers():
    bst = TRAINED[0]
    rng = np.random.default_rng(4)
    X, y = labelled(rng, bst, 2500)
    X[:, 0] += np.float32(0.7)  # another population
    keep, m_keep = B.refresh_host(bst, X, y, refresh_leaf=False)
    full, _ = B.refresh_host(bst, X, y, refresh_leaf=True)
    np.testing.assert_array_equal(bits(m_keep), bits(B.predict_margin_host(bst, X)))
    np.testing.assert_array_equal(bits(B.predict_margin_host(keep, X)), bits(B.predict_margin_host(bst, X)))
    for old, ref in zip(bst.trees, keep.trees):
        np.testing.assert_array_equal(bits(old.split_conditions), bits(ref.split_conditions))
    # the first tree sees the base margin either way; later trees see the OLD leaf values in the margin
    np.testing.assert_array_equal(bits(keep.trees[0].sum_hessian), bits(full.trees[0].sum_hessian))
    assert any((bits(a.sum_hessian) != bits(c.sum_hessian)).any() for a, c in zip(keep.trees[1:], full.trees[1:]))
    wt = B.refresh_row_weights(y, None, 3.0)
    gscale, hscale = gbdt_host.quant_scales(3.0, 17)
    hp = gbdt_host.HostGbdtParams(0, 0.3, 1.0, 0.0, 0.0, 1.0, 1.0, 11, gscale, hscale)
    stages = B.staged_margins_host(bst, X)
    leaf = leaf_rowwise(bst, X)
    for t, tree in enumerate(keep.trees):
        m = stages[t - 1] if t else np.full(len(y), np.float32(bst.base_margin), np.float32)
        _, hq = gbdt_host.gradients_host(m, y, wt, hp, t)
        Hs, _ = path_sums(tree, leaf[:, t], hq)
        np.testing.assert_array_equal(bits(tree.sum_hessian), bits((Hs.astype(np.float64) * (1.0 / hscale))))
    # SHAP still adds up to the (unchanged) margin, around the new population's expected value
    # (a zero-cover LEAF is fine for TreeSHAP, a zero-cover split is not: none here)
    assert all((t.sum_hessian[~t.is_leaf] > 0).all() for t in keep.trees)
    ex = explain.TreeExplainer(keep, device="cpu")
    phi = ex.shap_values(X[:64])
    np.testing.assert_allclose(phi.sum(1) + ex.expected_value, B.predict_margin_host(bst, X[:64]).astype(np.float64),
                               rtol=0, atol=2e-6)
    assert keep.expected_value() != bst.expected_value()
    assert keep.get_score("cover") != bst.get_score("cover")


# --------------------------------------------------------------------------------- 5 edges
def test_unreached_leaf_has_value_zero_and_cover_zero():
    b = sf.make_booster([sf.zero_cover_tree(np.random.default_rng(5))], 2)
    rng = np.random.default_rng(6)
    X = np.abs(rng.normal(size=(300, 2))).astype(np.float32) + np.float32(0.1)  # x0 >= 0: all rows go right
    y = (rng.random(300) < 0.4).astype(np.float32)
    new, _ = B.refresh_host(b, X, y)
    t = new.trees[0]
    left = int(t.left_children[0])
    dead = [left, int(t.left_children[left]), int(t.right_children[left])]
    assert (t.sum_hessian[dead] == 0).all() and (t.base_weights[dead] == 0).all()
    assert (t.split_conditions[dead[1:]] == 0).all() and t.loss_changes[left] == 0
    right = int(t.right_children[0])
    assert t.sum_hessian[right] == t.sum_hessian[0] > 0 and t.split_conditions[right] != 0


def test_single_row_all_positive_and_zero_weights():
    b = FORESTS["random"]
    rng = np.random.default_rng(8)
    X = rng.normal(size=(400, 8)).astype(np.float32)
    one, m1 = B.refresh_host(b, X[:1], np.ones(1, np.float32))
    assert m1.shape == (1,) and np.isfinite(m1).all()
    leaf = leaf_rowwise(b, X[:1])
    for i, t in enumerate(one.trees):
        hit = np.zeros(t.num_nodes, bool)
        j = int(leaf[0, i])
        while True:
            hit[j] = True
            if t.parents[j] == B.ROOT_PARENT:
                break
            j = int(t.parents[j])
        assert (t.sum_hessian[~hit] == 0).all() and (t.split_conditions[~hit & t.is_leaf] == 0).all()
    pos, mp = B.refresh_host(b, X, np.ones(400, np.float32), reg_lambda=1.0)
    assert all((t.split_conditions[t.is_leaf & (t.sum_hessian >= 1)] > 0).all() for t in pos.trees)  # g < 0 everywhere
    np.testing.assert_array_equal(bits(mp), bits(B.predict_margin_host(pos, X)))
    # zero-weight rows contribute nothing: a leaf only they reach has cover 0 and value 0
    y = (rng.random(400) < 0.5).astype(np.float32)
    leaf = leaf_rowwise(b, X)
    w = np.where(leaf[:, 0] == leaf[0, 0], 0.0, 1.0).astype(np.float32)
    zw, _ = B.refresh_host(b, X, y, w)
    assert zw.trees[0].sum_hessian[leaf[0, 0]] == 0 and zw.trees[0].split_conditions[leaf[0, 0]] == 0
    assert zw.trees[0].sum_hessian[0] > 0


def test_min_child_weight_and_reg_alpha():
    bst, X, y = TRAINED
    big, _ = B.refresh_host(bst, X, y, min_child_weight=1e9)
    for t in big.trees:
        assert (t.base_weights == 0).all() and (t.split_conditions[t.is_leaf] == 0).all()
        assert (t.loss_changes == 0).all() and t.sum_hessian[0] > 0
    sums = []
    l1, _ = B.refresh_host(bst, X, y, reg_alpha=2.0, node_sums=sums)
    gscale, hscale = gbdt_host.quant_scales(3.0, 17)
    some_zero = some_shrunk = False
    for s, t in zip(sums, l1.trees):
        G, H = s[:, 0] * (1.0 / gscale), s[:, 1] * (1.0 / hscale)
        for j in range(t.num_nodes):
            if H[j] < 1.0:
                want = 0.0
            elif abs(G[j]) <= 2.0:
                want, some_zero = 0.0, True
            else:
                want, some_shrunk = -(G[j] - math.copysign(2.0, G[j])) / (H[j] + 1.0), True
            assert t.base_weights[j] == np.float32(want), j
            if t.left_children[j] == -1:
                assert t.split_conditions[j] == np.float32(want * 0.3), j
    assert some_zero and some_shrunk
    assert l1.train_params["reg_alpha"] == 2.0 and bst.train_params.get("reg_alpha") == 0.0


# ------------------------------------------------------------------------------ 6 interface
def test_input_booster_is_untouched_and_result_is_new():
    bst, X, y = TRAINED
    loaded = Booster.load_raw(bst.save_raw())
    assert loaded.source_config is not None
    raw = loaded.save_raw()
    new = loaded.refresh(X[:500], y[:500], device="cpu", learning_rate=0.1)
    assert loaded.save_raw() == raw
    assert new is not loaded and new.source_config is None
    assert new.feature_names == loaded.feature_names and new.base_score == loaded.base_score
    assert new.train_params["eta"] == 0.1 and loaded.train_params["eta"] == pytest.approx(0.3)
    assert all(a.split_conditions is not c.split_conditions for a, c in zip(loaded.trees, new.trees))
    b2, m2 = loaded.refresh(X[:500], y[:500], device="cpu", learning_rate=0.1, return_margin=True)
    assert b2.save_raw() == new.save_raw()
    np.testing.assert_array_equal(bits(m2), bits(new.predict_margin(X[:500], device="cpu")))
    with pytest.raises(TypeError):
        loaded.refresh(X[:10], y[:10], device="cpu", max_depth=3)


def test_classifier_apply_and_refresh(tmp_path):
    rng = np.random.default_rng(9)
    X = rng.normal(size=(1200, 6)).astype(np.float32)
    y = (X[:, 0] - X[:, 1] + rng.normal(size=1200) > 0).astype(np.int64)
    clf = gbdt.GBDTClassifier(n_estimators=30, max_depth=3, learning_rate=0.3, device="cpu", early_stopping_rounds=3,
                              random_state=2)
    clf.fit(X[:800], y[:800], eval_set=[(X[800:], y[800:])])
    b = clf.get_booster()
    assert b.best_iteration is not None and b.best_iteration + 1 <= b.num_trees
    leaf = clf.apply(X[:50])
    np.testing.assert_array_equal(leaf, leaf_rowwise(b, X[:50], b.best_iteration + 1))
    np.testing.assert_array_equal(clf.apply(X[:50], iteration_range=(0, 2)), leaf_rowwise(b, X[:50], 2))
    np.testing.assert_array_equal(clf.apply(X[:50], iteration_range=(0, 0)), leaf_rowwise(b, X[:50]))
    raw = b.save_raw()
    new = clf.refresh(X[800:], y[800:])
    assert isinstance(new, gbdt.GBDTClassifier) and new is not clf and new.get_booster() is not b
    assert b.save_raw() == raw
    assert new.get_params() == clf.get_params()
    assert new.predict_proba(X[:20]).shape == (20, 2)
    path = tmp_path / "refreshed.pkl"
    new.save_pickle(path)
    back = gbdt.GBDTClassifier.load_pickle(path)
    for a, c in zip(new.get_booster().trees, back.get_booster().trees):
        for f in ("left_children", "right_children", "parents", "split_indices", "default_left"):
            np.testing.assert_array_equal(getattr(a, f), getattr(c, f))
        for f in ("split_conditions", "base_weights", "loss_changes", "sum_hessian"):
            np.testing.assert_array_equal(bits(getattr(a, f)), bits(getattr(c, f)))
    np.testing.assert_array_equal(back.predict_proba(X[:20]), new.predict_proba(X[:20]))


def test_refusals():
    bst, X, y = TRAINED
    X, y = X[:200], y[:200]

    class World:
        world = 2

    mono = Booster(list(bst.trees), num_feature=8, base_score=bst.base_score,
                   train_params={**bst.train_params, "monotone_constraints": (1, 0, 0, 0, 0, 0, 0, 0)})
    bad_y = y.copy()
    bad_y[3] = 0.5
    neg = np.ones(200, np.float32)
    neg[0] = -1.0
    for fn in (lambda: mono.refresh(X, y, device="cpu"),
               lambda: bst.refresh(X, y, device="cpu", dist=World()),
               lambda: bst.refresh(X[:0], y[:0], device="cpu"),
               lambda: bst.refresh(X, bad_y, device="cpu"),
               lambda: bst.refresh(X, y * 2, device="cpu"),
               lambda: bst.refresh(X, y, neg, device="cpu"),
               lambda: bst.refresh(X, y, np.zeros(200, np.float32), device="cpu"),
               lambda: bst.refresh(X, y[:100], device="cpu"),
               lambda: bst.refresh(X[:, :4], y, device="cpu"),
               lambda: bst.refresh(X, y, device="cpu", grad_bits=20),
               lambda: B.refresh_host(bst, X, bad_y)):
        with pytest.raises(ValueError):
            fn()
