"""Every kernel built on csrc/forest_walk.h (ForestBlock + walk_trees, and the grid-point walks of
csrc/pdp_walk.h on the same staged tiles) takes the same path through the same forest: on one hand-built
forest and rows of edge values, the margins of the row-block predictor are reproduced bit for bit by the
tile-parallel predictor, the learning-curve kernel, the permutation-importance baseline, the ICE curve of a
feature no tree uses, and the leaf values that the leaf-index kernel points at. The entry points also agree
on what they refuse. Every assertion is an exact equality.
"""
import numpy as np
import pytest
import torch

import scoring_forests as sf
from cobalt_smart_lender_ai_amd import _native
from cobalt_smart_lender_ai_amd.ops import predict_ops

pytestmark = pytest.mark.gpu

F = 7
UNUSED = 6            # no tree splits on this feature
STUMPS = (19, 20)     # positions of the two single-leaf trees
ROWS = (1, 65, 257)   # 257: a second block with one live row, where the two row-staging variants differ


def _forest():
    rng = np.random.default_rng(2024)
    trees = [sf.random_tree(rng, F, 5, 0.15, cols=range(UNUSED), grid=sf.THRESHOLD_GRID) for _ in range(40)]
    trees[STUMPS[0]:STUMPS[0]] = [sf.stump(0.5), sf.stump(-0.25)]
    X = sf.edge_rows(rng, max(ROWS), F)
    y = (rng.random(max(ROWS)) < 0.5).astype(np.float32)
    return trees, X, y


def _tile_nodes(b):
    """The smallest tile size that cuts the forest into at least 3 tiles with a boundary between the stumps."""
    biggest = max(len(t.left_children) for t in b.trees)
    for cand in range(biggest, 8 * biggest):
        tiles = predict_ops.pack_forest(b, None, cand)[2]
        if len(tiles) - 1 >= 3 and STUMPS[1] in tiles[1:-1]:
            return cand
    raise AssertionError("no tile size separates the stumps")


@pytest.mark.parametrize("n", ROWS)
def test_every_forest_kernel_reproduces_the_predictor(n, monkeypatch):
    trees, X, y = _forest()
    b = sf.make_booster(trees, F)
    assert all(len(b.trees[s].left_children) == 1 for s in STUMPS)
    assert not any(UNUSED in sf.tree_features(t) for t in b.trees)
    monkeypatch.setattr(predict_ops, "TILE_NODES", _tile_nodes(b))
    tiles = predict_ops.pack_forest(b)[2]
    assert len(tiles) - 1 >= 3 and STUMPS[1] in tiles[1:-1], tiles
    Xd = torch.from_numpy(X[:n].copy()).cuda()
    assert torch.isnan(Xd).any() or n == 1

    m_t = torch.empty(n, dtype=torch.float32, device="cuda")
    with monkeypatch.context() as mp:
        mp.setattr(predict_ops, "_SMALL_ROWS", 0)          # the row-block kernel k_predict
        predict_ops.predict_gpu(b, Xd, None, out_margin=m_t)
    m = m_t.cpu().numpy()
    assert np.isfinite(m).all()

    small = torch.empty(n, dtype=torch.float32, device="cuda")
    predict_ops.predict_gpu(b, Xd, None, out_margin=small)  # k_predict_leaves + k_sum_leaves
    np.testing.assert_array_equal(small.cpu().numpy(), m)

    np.testing.assert_array_equal(predict_ops.staged_margins(b, Xd)[-1].cpu().numpy(), m)

    _, final = predict_ops.eval_curve(b, Xd, y[:n], metrics=("logloss", "error"))
    np.testing.assert_array_equal(final.cpu().numpy(), m)

    perm = torch.from_numpy(np.random.default_rng(n).permutation(n).astype(np.int32)[None, :]).cuda()
    jobs, _ = predict_ops.permutation_scores_gpu(b, Xd, None, (0,), perm, want_margins=True, want_sums=False)
    np.testing.assert_array_equal(jobs[0].cpu().numpy(), m)

    grid = np.array([np.nan, -1.5, 0.25, np.inf, 1e-45], np.float32)
    ice, _ = predict_ops.partial_dependence_gpu(b, Xd, (UNUSED,), [grid], want_ice=True, want_avg=False)
    np.testing.assert_array_equal(ice.cpu().numpy(), np.broadcast_to(m, (len(grid), n)))

    leaf = predict_ops.predict_leaf(b, Xd).cpu().numpy()
    acc = np.full(n, np.float32(b.base_margin), np.float32)
    for t, tree in enumerate(b.trees):
        assert (tree.left_children[leaf[:, t]] == -1).all()
        acc = (acc + tree.split_conditions[leaf[:, t]]).astype(np.float32)
    np.testing.assert_array_equal(acc, m)


def test_every_forest_entry_point_refuses_the_same_limits():
    """A tile above 8192 nodes is -2 and an LDS footprint above 160 KiB (2048 * 8 + 256 * (144 | 1) * 4 bytes)
    is -3 at all six entry points, before anything is launched."""
    rng = np.random.default_rng(5)
    b = sf.random_forest(rng, F, 3, 3)
    n, wide = 8, 144
    Xd = torch.zeros((n, wide), dtype=torch.float32, device="cuda")
    gf = predict_ops.gpu_forest(b, Xd.device)
    lib, st = _native.lib(), _native.stream_handle()
    forest = (gf.nodes.data_ptr(), gf.tree_ptr.data_ptr(), gf.tile_ptr.data_ptr(), gf.n_tiles)
    out = torch.full((4 * gf.n_trees, n), 7.0, dtype=torch.float32, device="cuda")
    idx = torch.full((gf.n_trees, n), 7, dtype=torch.int16, device="cuda")
    g1 = torch.zeros(1, dtype=torch.float32, device="cuda")
    ft = torch.zeros(1, dtype=torch.int32, device="cuda")
    cols = torch.zeros((1, n), dtype=torch.float32, device="cuda")
    perm = torch.zeros((1, n), dtype=torch.int32, device="cuda")
    o = out.data_ptr()

    def codes(width, tile_cap):
        x = (Xd.data_ptr(), n, width, wide)
        return {
            "cobalt_predict": lib.cobalt_predict(*x, *forest, tile_cap, 0.0, o, None, st),
            "cobalt_predict_small": lib.cobalt_predict_small(*x, *forest, tile_cap, gf.n_trees, 0.0, o, o, None, st),
            "cobalt_eval_curve": lib.cobalt_eval_curve(*x, None, None, *forest, tile_cap, gf.n_trees, 0.0, None, o,
                                                       None, None, None, st),
            "cobalt_pdp": lib.cobalt_pdp(*x, *forest, tile_cap, 0.0, 0, -1, g1.data_ptr(), 1, None, 1, None, o, None,
                                         None, st),
            "cobalt_perm_importance": lib.cobalt_perm_importance(*x, *forest, tile_cap, 0.0, ft.data_ptr(), 1,
                                                                 cols.data_ptr(), perm.data_ptr(), 1, None, None, o,
                                                                 None, None, 0, st),
            "cobalt_leaf_index": lib.cobalt_leaf_index(*x, *forest, tile_cap, gf.n_trees, 0, gf.n_trees,
                                                       idx.data_ptr(), st),
        }

    for width, tile_cap, want in ((F, 8193, -2), (F, 0, -2), (wide, 2048, -3)):
        got = codes(width, tile_cap)
        assert got == dict.fromkeys(got, want), (width, tile_cap, got)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((idx == 7).all())  # nothing was launched
