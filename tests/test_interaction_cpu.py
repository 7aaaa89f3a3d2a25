"""Interaction constraints on the host trainer (``models/gbdt_host.py``, the oracle of the GPU kernels):
the accepted forms, the path property of every tree, an independent re-derivation of every node's winning
split from the set-based rule, the byte-for-byte equivalences, monotone constraints on top, round trips,
RFE / feature subsets, the refused combinations and the SHAP interaction values of a constrained model.

The host trainer costs seconds per fit, so the fits are small and the 5 000-row ones are shared."""
import json

import numpy as np
import pytest

from cobalt_smart_lender_ai_amd.models import gbdt, gbdt_host
from cobalt_smart_lender_ai_amd.models.booster import Booster, treeshap_interactions_host
from cobalt_smart_lender_ai_amd.models.gbdt import GBDTClassifier, GBDTParams, resolve_interaction

from test_eval_curve_cpu import assert_same_trees
from test_monotone_cpu import check_structure, make_data

GROUPS = [[0, 1, 2], [2, 3], [4]]   # feature 5 is in no group
FIT = dict(n_estimators=10, max_depth=5, learning_rate=0.3)
NAMES = [f"x{i}" for i in range(6)]


def check_paths(b: Booster, groups) -> int:
    """Every split node below the root: some group holds its root-to-node feature set (its own split
    included), and no split lies below a split on an ungrouped feature. Returns the number of non-root
    splits checked."""
    sets = [set(g) for g in groups]
    grouped = set().union(*sets) if sets else set()
    seen = 0
    for ti, t in enumerate(b.trees):
        work = [(0, frozenset())]
        while work:
            i, above = work.pop()
            if t.left_children[i] == -1:
                continue
            f = int(t.split_indices[i])
            path = above | {f}
            if i != 0:
                assert not (above - grouped), f"tree {ti} node {i}: a split below the ungrouped {sorted(above - grouped)}"
                assert any(path <= s for s in sets), f"tree {ti} node {i}: no group holds {sorted(path)}"
                seen += 1
            work += [(int(t.left_children[i]), path), (int(t.right_children[i]), path)]
    return seen


def strip(b: Booster) -> bytes:
    """The model's bytes without the stored constraint (to compare with an unconstrained fit's)."""
    c = b.slice(b.num_trees)
    c.train_params.pop("interaction_constraints", None)
    return c.save_raw("ubj")


def shap_data(n=500, seed=12):
    """3 features with both products in the signal, so that a free model would interact on (1, 2) too."""
    r = np.random.default_rng(seed)
    X = r.uniform(-2, 2, (n, 3)).astype(np.float32)
    z = X[:, 0] * X[:, 1] + X[:, 0] * X[:, 2] + X[:, 1] * X[:, 2]
    y = (r.uniform(size=n) < 1 / (1 + np.exp(-2 * z))).astype(np.float32)
    return X, y


SHAP_GROUPS = [[0, 1], [0, 2]]
SHAP_FIT = dict(n_estimators=5, max_depth=3, learning_rate=0.5, interaction_constraints=SHAP_GROUPS)


@pytest.fixture(scope="module")
def data():
    return make_data(5000, 0)


@pytest.fixture(scope="module")
def fits(data):
    X, y = data
    free = gbdt.train(X, y, dict(FIT), device="cpu")
    cons = gbdt.train(X, y, dict(FIT, interaction_constraints=GROUPS), device="cpu")
    return free, cons


# ------------------------------------------------------------------------------- 1. the forms
def test_accepted_forms_resolve_to_the_canonical_groups():
    for form in (GROUPS, [(0, 1, 2), (2, 3), (4,)], [np.array([2, 1, 0]), [3, 2, 2], [4], []], "[[0, 1, 2], [2, 3], [4]]",
                 json.dumps(GROUPS), " [[2,1,0],[3,2],[4]] ", [["x0", "x1", "x2"], ["x2", "x3"], ["x4"]],
                 '[["x0", "x1", "x2"], ["x3", "x2"], ["x4"]]', [["x0", 1, 2], [np.int64(2), "x3"], [4]]):
        assert resolve_interaction(form, 6, NAMES) == GROUPS, form
    # sorted, without duplicates, empty groups dropped, group order kept; overlapping and repeated groups stay
    assert resolve_interaction([[3, 1, 3], [], [0], [1, 3]], 6) == [[1, 3], [0], [1, 3]]
    for form in (None, [], "", "  ", "[]", [[]], "[[], []]", ()):
        assert resolve_interaction(form, 6, NAMES) is None, form
    # one group with every feature is a constraint, not a shortcut
    assert resolve_interaction([list(range(6))], 6) == [list(range(6))]
    assert GBDTParams.from_kwargs(interaction_constraints="[[0, 1]]").interaction_constraints == "[[0, 1]]"
    # the host has no group limit; the GPU trainer's is given by the caller
    many = [[i % 6] for i in range(65)]
    assert len(resolve_interaction(many, 6)) == 65
    assert len(resolve_interaction(many[:64], 6, max_groups=64)) == 64
    with pytest.raises(ValueError, match="interaction_constraints.*64"):
        resolve_interaction(many, 6, max_groups=64)


@pytest.mark.parametrize("form, names", [
    ([[0, 6]], None),                     # an index out of range
    ([[0, -1]], None),
    ("[[0, 1], [2, 7]]", None),
    ([[0, 1.0]], None),                   # a non-integer
    ([[0, 1.5]], None),
    ("[[0, 1.5]]", None),
    ([[0, True]], None),                  # a bool
    ("[[0, true]]", None),
    ([[0, None]], None),
    ([["x0", "x1"]], None),               # a name without feature names
    ([["x0", "nope"]], NAMES),            # an unknown name
    ("[[0, 1], [2", None),                # not JSON
    ([0, 1], None),                       # not a list of lists
    ({"x0": [1]}, NAMES),
    ("{\"a\": [0]}", None),
    (3, None),
])
def test_invalid_constraints_raise(form, names):
    with pytest.raises(ValueError, match="interaction_constraints"):
        resolve_interaction(form, 6, names)
    X, y = make_data(64, 3)
    with pytest.raises(ValueError, match="interaction_constraints"):
        gbdt.train(X, y, dict(n_estimators=1, max_depth=2, interaction_constraints=form), device="cpu",
                   feature_names=names)


# ------------------------------------------------------------------------ 2. the host's trees
def test_host_structure(fits):
    free, cons = fits
    assert check_paths(cons, GROUPS) > 20
    assert cons.interaction_constraints == GROUPS
    assert strip(cons) != free.save_raw("ubj")
    with pytest.raises(AssertionError):  # (the check can fail: the free model breaks it)
        check_paths(free, GROUPS)


def allowed_by_sets(path: set, groups, F: int) -> np.ndarray:
    """The rule of the issue, by sets: below the root, the union of the groups that contain the path."""
    ok = np.zeros(F, dtype=bool)
    for g in groups:
        if path <= set(g):
            ok[list(g)] = True
    return ok


@pytest.mark.parametrize("extra", [{}, dict(reg_alpha=0.5, colsample_bytree=0.7)], ids=["base", "alpha_colsample"])
def test_every_winning_split_rederived_from_the_set_rule(extra):
    """The first two trees of a constrained fit, node by node: rows routed through the model's own splits,
    ``_node_hist`` + the UNCONSTRAINED ``_eval_node`` under ``fmask & allowed`` with ``allowed`` from the
    few lines above. Shares no constraint code with the trainer (the params carry no constraint)."""
    X, y = make_data(1500, 2)
    prm = dict(n_estimators=2, max_depth=4, learning_rate=0.3, max_bin=32, **extra)
    params = GBDTParams.from_kwargs(**prm)
    b = gbdt.train(X, y, dict(prm, interaction_constraints=GROUPS), device="cpu")
    bd = gbdt.bin_dataset(X, max_bin=32, device="cpu")
    bins, cuts, nbins = bd.bins_host, bd.cuts.numpy(), bd.nbins.numpy()
    N, F = bins.shape
    gs, hs = gbdt_host.quant_scales(1.0)
    p = gbdt_host.HostGbdtParams(max_depth=4, eta=0.3, reg_lambda=params.reg_lambda, reg_alpha=params.reg_alpha,
                                 gamma=params.gamma, min_child_weight=params.min_child_weight, subsample=1.0,
                                 seed=params.random_state, gscale=gs, hscale=hs)
    masks = gbdt.feature_masks(2, F, params.colsample_bytree, params.random_state)
    margin = np.full(N, np.float32(b.base_margin), dtype=np.float32)
    checked = 0
    for ti, t in enumerate(b.trees):
        fmask = np.asarray(masks[ti]).astype(bool)
        gq, hq = gbdt_host.gradients_host(margin, y, np.ones(N, np.float32), p, ti)
        work = [(0, np.arange(N), set(), 0)]
        while work:
            i, rows, path, level = work.pop()
            is_split = t.left_children[i] != -1
            if level == p.max_depth:
                assert not is_split
            else:
                allowed = np.ones(F, dtype=bool) if level == 0 else allowed_by_sets(path, GROUPS, F)
                hist = gbdt_host._node_hist(bins, rows, gq, hq, np.ones(F, np.uint8), nbins)
                G, H = hist[F, 0]
                best, _, _ = gbdt_host._eval_node(hist, G.item(), H.item(), nbins, fmask & allowed, p)
                ok = best is not None and np.float32(best[0]) > np.float32(1e-6) and np.float32(best[0]) >= np.float32(p.gamma)
                assert ok == bool(is_split), f"tree {ti} node {i}"
                checked += 1
            if not is_split:
                margin[rows] = (margin[rows] + t.split_conditions[i]).astype(np.float32)
                continue
            f, rr = best[1] >> 10, best[1] & 1023
            j, dl = (rr, 0) if rr < 512 else ((int(nbins[f]) - 1 - (rr - 512)) - 1, 1)
            assert (int(t.split_indices[i]), int(t.default_left[i])) == (f, dl), f"tree {ti} node {i}"
            assert t.split_conditions[i] == (cuts[f, j] if j >= 0 else -gbdt_host.FLT_MAX), f"tree {ti} node {i}"
            assert t.loss_changes[i] == np.float32(best[0])
            bf = bins[rows, f]
            left = np.where(bf == 255, dl == 1, bf.astype(np.int64) <= j) if int(nbins[f]) < 256 else bf.astype(np.int64) <= j
            work += [(int(t.left_children[i]), rows[left], path | {f}, level + 1),
                     (int(t.right_children[i]), rows[~left], path | {f}, level + 1)]
    assert checked > 20


# --------------------------------------------------------------------------- 3. equivalences
def test_one_group_of_all_features_equals_the_unconstrained_fit(fits, data):
    X, y = data
    free, _ = fits
    one = gbdt.train(X, y, dict(FIT, interaction_constraints=[list(range(6))]), device="cpu")
    assert one.interaction_constraints == [list(range(6))]
    assert strip(one) == free.save_raw("ubj")


def test_depth_one_equals_the_unconstrained_fit(data):
    X, y = data
    p = dict(n_estimators=4, max_depth=1, learning_rate=0.3)
    free = gbdt.train(X[:1500], y[:1500], dict(p), device="cpu")
    cons = gbdt.train(X[:1500], y[:1500], dict(p, interaction_constraints=GROUPS), device="cpu")
    assert strip(cons) == free.save_raw("ubj")
    assert_same_trees(cons.trees, free.trees)


def test_singleton_groups_give_single_feature_trees(data):
    X, y = data
    b = gbdt.train(X[:1500], y[:1500], dict(n_estimators=6, max_depth=4, learning_rate=0.3,
                                            interaction_constraints=[[f] for f in range(6)]), device="cpu")
    used = [set(t.split_indices[t.left_children != -1].tolist()) for t in b.trees]
    assert all(len(u) == 1 for u in used), used
    assert max(t.depth() for t in b.trees) > 1 and len(set().union(*used)) > 1


def test_exact_fp64_and_wide_gradients(data):
    X, y = data
    for kw, p in ((dict(exact_fp64=True), {}), ({}, dict(grad_bits=25))):
        b = gbdt.train(X[:1500], y[:1500], dict(n_estimators=4, max_depth=4, interaction_constraints=GROUPS, **p),
                       device="cpu", **kw)
        assert check_paths(b, GROUPS) > 8


# ------------------------------------------------------------------- 4. monotone on top
def test_monotone_and_interaction_constraints_compose(data):
    X, y = data
    mono = (1, -1, 0, 1, 0, -1)
    b = gbdt.train(X, y, dict(FIT, monotone_constraints=mono, interaction_constraints=GROUPS), device="cpu")
    assert check_structure(b, mono) > 20
    assert check_paths(b, GROUPS) > 20
    assert b.monotone_constraints == mono and b.interaction_constraints == GROUPS


# --------------------------------------------------------------------------- 5. round trips
def test_model_round_trips(fits):
    free, cons = fits
    raw = cons.save_raw("ubj")
    cfg = cons.to_doc()["Config"]["learner"]["gradient_booster"]["tree_train_param"]
    assert cfg["interaction_constraints"] == "[[0, 1, 2], [2, 3], [4]]"
    for fmt in ("ubj", "json"):
        back = Booster.load_raw(cons.save_raw(fmt))
        assert back.interaction_constraints == GROUPS and back.save_raw("ubj") == raw
    assert cons.slice(3).interaction_constraints == GROUPS
    assert free.to_doc()["Config"]["learner"]["gradient_booster"]["tree_train_param"]["interaction_constraints"] == ""
    assert Booster.load_raw(free.save_raw("ubj")).interaction_constraints is None


def test_classifier_params_clone_and_pickle(data, tmp_path):
    from sklearn.base import clone

    X, y = data
    X, y = X[:600], y[:600]
    clf = GBDTClassifier(n_estimators=3, max_depth=3, device="cpu", interaction_constraints=GROUPS)
    assert clf.get_params()["interaction_constraints"] == GROUPS
    assert "interaction_constraints" not in GBDTClassifier(n_estimators=3).get_params()
    assert clone(clf).interaction_constraints == GROUPS
    assert clone(clf).set_params(interaction_constraints=None).get_params() == GBDTClassifier(
        n_estimators=3, max_depth=3, device="cpu").get_params()
    clf.fit(X, y)
    want = gbdt.train(X, y, dict(n_estimators=3, max_depth=3, interaction_constraints=GROUPS), device="cpu")
    assert clf.get_booster().save_raw("ubj") == want.save_raw("ubj")
    path = tmp_path / "m.pkl"
    clf.save_pickle(path)
    back = GBDTClassifier.load_pickle(path)
    assert resolve_interaction(back.interaction_constraints, 6) == GROUPS
    assert back.get_booster().interaction_constraints == GROUPS
    assert back.get_booster().save_raw("ubj") == want.save_raw("ubj")


def test_checkpoint_resume_is_bit_identical(tmp_path):
    X, y = make_data(600, 5)
    p = dict(n_estimators=4, max_depth=3, interaction_constraints=GROUPS)
    whole = gbdt.train(X, y, dict(p), device="cpu").save_raw("ubj")
    path = str(tmp_path / "half.ubj")
    gbdt.train(X, y, dict(p, n_estimators=2), device="cpu", checkpoint_path=path, checkpoint_every=2)
    assert gbdt.train(X, y, dict(p), device="cpu", checkpoint_path=path, checkpoint_every=2).save_raw("ubj") == whole
    for other in ([[0, 1]], None):
        with pytest.raises(ValueError, match="different parameters"):
            gbdt.train(X, y, dict(p, interaction_constraints=other), device="cpu", checkpoint_path=path,
                       checkpoint_every=2)


# ------------------------------------------------------------------------- 6. RFE / subsets
def test_subset_then_expand_restores_the_groups():
    r = np.random.default_rng(31)   # (feature 3 carries signal of its own: the trees split on it, repeatedly)
    X = r.uniform(-2, 2, (1500, 6)).astype(np.float32)
    z = 2 * np.sin(3 * X[:, 3]) + X[:, 0] - X[:, 1] + 0.5 * X[:, 4]
    y = (r.uniform(size=1500) < 1 / (1 + np.exp(-z))).astype(np.float32)
    bd = gbdt.bin_dataset(X, device="cpu")
    full = resolve_interaction(GROUPS, 6)
    feats = np.array([0, 1, 3, 4, 5])   # feature 2 goes: [0,1,2] -> [0,1], [2,3] -> [3] (position 2), [4] -> [3]
    sub_groups = gbdt.subset_interaction(full, feats)
    assert sub_groups == [[0, 1], [2], [3]]
    assert gbdt.subset_interaction(full, [2, 5]) == [[0], [0]] and gbdt.subset_interaction(full, [5]) is None
    p = dict(n_estimators=6, max_depth=4, learning_rate=0.3)
    sub = gbdt.train_binned(gbdt.subset_features(bd, feats), y, dict(p, interaction_constraints=sub_groups))
    assert sub.interaction_constraints == sub_groups
    # without the full-width groups the subset's are mapped back; with them the booster carries them
    assert gbdt.expand_features(sub, feats, 6).interaction_constraints == [[0, 1], [3], [4]]
    wide = gbdt.expand_features(sub, feats, 6, interaction_constraints=full)
    assert wide.interaction_constraints == GROUPS
    # [2, 3] shrank to [3], which is still a group: below a split on 3 only 3 is used
    assert check_paths(wide, [[0, 1], [3], [4]]) > 8
    below3 = 0
    for t in wide.trees:
        for i in np.nonzero((t.left_children != -1) & (t.split_indices == 3))[0]:
            work = [int(t.left_children[i]), int(t.right_children[i])]
            while work:
                k = work.pop()
                if t.left_children[k] != -1:
                    assert t.split_indices[k] == 3
                    below3 += 1
                    work += [int(t.left_children[k]), int(t.right_children[k])]
    assert below3 > 0
    # the same trees as the masked full-width fit
    mask = np.zeros(6, dtype=bool)
    mask[feats] = True
    masked = gbdt.train_binned(bd, y, dict(p, interaction_constraints=GROUPS), feature_mask=mask)
    assert wide.save_raw("ubj") == masked.save_raw("ubj")


def test_rfe_repack_equals_masked():
    from cobalt_smart_lender_ai_amd.select.rfe import rfe

    r = np.random.default_rng(21)
    N = 800
    X = r.uniform(-2, 2, (N, 8)).astype(np.float32)
    z = 1.5 * X[:, 0] - X[:, 1] + 0.7 * X[:, 4] + 0.5 * X[:, 6] * X[:, 7] + np.sin(3 * X[:, 5])
    y = (r.uniform(size=N) < 1 / (1 + np.exp(-z))).astype(np.float32)
    names = [f"f{i}" for i in range(8)]
    groups = [[0, 1, 2], [2, 3], [4, 5], [6, 7]]
    p = GBDTParams(n_estimators=3, max_depth=3, interaction_constraints=[[names[i] for i in g] for g in groups])
    packed = rfe(X, y, p, n_features_to_select=5, device="cpu", feature_names=names, repack=True)
    masked = rfe(X, y, p, n_features_to_select=5, device="cpu", feature_names=names, repack=False)
    assert np.array_equal(packed.support_, masked.support_) and packed.n_features_ == 5
    assert packed.estimator_.save_raw("ubj") == masked.estimator_.save_raw("ubj")
    assert packed.estimator_.interaction_constraints == groups
    assert check_paths(packed.estimator_, groups) > 0


# ----------------------------------------------------------------------------- 7. refusals
def test_refused_combinations():
    from cobalt_smart_lender_ai_amd.models import external, stream
    from cobalt_smart_lender_ai_amd.parallel import loopback

    X, y = make_data(256, 6)
    p = dict(n_estimators=1, max_depth=2, interaction_constraints=GROUPS)
    src = stream.array_chunks(X, y, 128)
    with pytest.raises(ValueError, match="interaction_constraints"):
        stream.train_stream(src, dict(p), device="cpu")
    with pytest.raises(ValueError, match="interaction_constraints"):
        external.train_external(src, dict(p), device="cpu")

    def rank_fit(dist):
        with pytest.raises(ValueError, match="interaction_constraints"):
            gbdt.train(X, y, dict(p), device="cpu", dist=dist)
        with pytest.raises(ValueError, match="interaction_constraints"):
            gbdt.train_binned(gbdt.bin_dataset(X, device="cpu"), y, dict(p), dist=dist)
        return True
    assert loopback.run_ranks(1, rank_fit, device="cpu") == [True]
    # the empty forms are no constraints: nothing to refuse
    stream.train_stream(src, dict(p, interaction_constraints="[]"), device="cpu")


# --------------------------------------------------------------------------------- 8. SHAP
def test_shap_interactions_vanish_between_features_of_no_common_group():
    X, y = shap_data()
    b = gbdt.train(X, y, dict(SHAP_FIT), device="cpu")
    assert check_paths(b, SHAP_GROUPS) > 5
    phi2 = treeshap_interactions_host(b, X)
    assert np.abs(phi2[:, 1, 2]).max() <= 1e-9 and np.abs(phi2[:, 2, 1]).max() <= 1e-9
    assert np.abs(phi2[:, 0, 1]).max() > 1e-3
    free = gbdt.train(X, y, {k: v for k, v in SHAP_FIT.items() if k != "interaction_constraints"}, device="cpu")
    assert np.abs(treeshap_interactions_host(free, X)[:, 1, 2]).max() > 1e-3   # (the free model does interact)
