"""scripts/row_locality.py: the unit counting of the locality estimator on a hand-made 16-row example."""
import importlib.util
from pathlib import Path

import numpy as np

_spec = importlib.util.spec_from_file_location(
    "row_locality", Path(__file__).resolve().parents[1] / "scripts" / "row_locality.py")
rl = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rl)

NODE = [("status", "i4"), ("feat", "i4"), ("bin", "i4"), ("default_left", "i4"), ("build", "i4")]


def _example():
    """Depth 2. Root: feature 0 <= 0 (even rows left). Node 1 (built): feature 1 <= 0. Node 2: a leaf."""
    bins = np.zeros((16, 2), dtype=np.uint8)
    bins[:, 0] = np.arange(16) % 2
    bins[:, 1] = (np.arange(16) // 2) % 2
    nodes = np.zeros(7, dtype=NODE)
    nodes["status"][[0, 1]] = 2
    nodes["status"][[2, 3, 4]] = 3
    nodes["feat"][[0, 1]] = [0, 1]
    nodes["build"][[0, 1, 3]] = 1
    return bins, nodes


def test_walk_and_keys():
    bins, nodes = _example()
    at = rl.walk_levels(nodes, bins, 2)
    assert at[1].tolist() == [1, 2] * 8
    assert at[2].tolist() == [3, -1, 4, -1] * 4
    assert rl.leaf_keys(at, "heap").tolist() == [3, 2, 4, 2] * 4
    assert rl.leaf_keys(at, "dfs").tolist() == [0, 2, 1, 2] * 4  # node 2 (level 1) covers positions 2, 3


def test_unit_counting():
    assert rl.distinct_units(np.array([1, 1, 1, 1]), np.array([0, 31, 32, 95]), 32) == 3
    assert rl.distinct_units(np.array([1, 1, 2, 2]), np.array([0, 1, 0, 1]), 2) == 2  # per node, then summed
    assert rl.distinct_units(np.zeros(0, np.int64), np.zeros(0, np.int64), 2) == 0
    assert rl.packed_units(np.array([1, 1, 1, 4, 4]), 2) == 3


def test_level_counts_natural_and_reordered():
    bins, nodes = _example()
    at = rl.walk_levels(nodes, bins, 2)
    ident = np.arange(16, dtype=np.int64)
    # level 0: all 16 records = 8 units; level 1: the built node's 8 even rows, one unit each, 4 packed
    assert rl.level_counts(nodes, at, ident).tolist() == [[8, 8, 1, 1], [8, 4, 1, 1]]
    perm = rl.reorder(ident, rl.leaf_keys(at, "dfs"))
    assert perm.tolist() == [0, 4, 8, 12, 2, 6, 10, 14, 1, 3, 5, 7, 9, 11, 13, 15]  # stable within a leaf
    assert rl.level_counts(nodes, at, rl.positions(perm)).tolist() == [[8, 8, 1, 1], [4, 4, 1, 1]]
    # a second reorder keeps the earlier order inside every key: hierarchical
    again = rl.reorder(perm, (np.arange(16) >= 8).astype(np.int64))
    assert again.tolist() == [0, 4, 2, 6, 1, 3, 5, 7, 8, 12, 10, 14, 9, 11, 13, 15]


def test_schedules():
    assert rl.parse_schedule("", 10) == [] and rl.parse_schedule("off", 10) == []
    assert rl.parse_schedule("0,8,32", 20) == [0, 8]
    assert rl.parse_schedule("every:4", 10) == [0, 4, 8]
