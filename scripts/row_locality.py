#!/usr/bin/env python
"""How many memory units the trainer's per-level gathers touch, with the rows in their natural order
and with the rows regrouped by the leaf they reached in an earlier tree (CPU only, NumPy).

The GPU trainer's two gather kernels read through the row-id list of a node: ``k_hist`` one 32-byte
record per row of the BUILT child of every split (the smaller one; the sibling is a subtraction),
``k_part_pos`` one byte per row of every SPLIT node from the split feature's column of ``binsT``.
Memory moves in 64-byte units (records) and 32-byte sectors (byte columns), so what a node costs is
the number of distinct units / sectors its rows touch, not its row count.

This script trains the host oracle (models/gbdt_host.py) with the bench hyper-parameters on
``synth.make_lendingclub`` rows and, for every tree after the first and every level, counts

  rec64   distinct 64-byte units of the 32-byte records under the built children's rows
  col32   distinct 32-byte sectors of the split feature's byte column under the split nodes' rows

summed over the level's nodes, for each reorder schedule given with ``--schedule`` (repeatable) next
to the natural order. ``ideal`` is the count with every node's rows packed: ceil(rows / 2) and
ceil(rows / 32) per node. A reorder after tree t stably sorts the CURRENT order by the row's leaf in
tree t, so repeated reorders are hierarchical (latest tree primary, earlier ones secondary).

  --schedule 0          one reorder after tree 0
  --schedule 0,8,32     reorders after trees 0, 8 and 32
  --schedule every:16   after trees 0, 16, 32, ...
  --key dfs|heap        sort key: the leaf's left-most position on the bottom level (depth-first order:
                        every subtree's rows stay contiguous), or its heap index (level by level)
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

RECORD_BYTES, RECORD_UNIT = 32, 64  # a row record; the transfer it arrives in
COLUMN_SECTOR = 32                  # bytes (= rows) of a byte column per sector


def parse_schedule(text: str, n_trees: int) -> list[int]:
    """'' -> [], '0,8,32' -> those trees, 'every:16' -> 0, 16, 32, ... (all below n_trees)."""
    text = text.strip()
    if not text or text == "off":
        return []
    if text.startswith("every:"):
        return list(range(0, n_trees, int(text[6:])))
    return sorted({int(t) for t in text.split(",") if int(t) < n_trees})


def walk_levels(nodes: np.ndarray, bins: np.ndarray, depth: int) -> np.ndarray:
    """[depth + 1, N] heap node of every row at every level; -1 below the leaf the row stopped in."""
    n = bins.shape[0]
    at = np.full((depth + 1, n), -1, dtype=np.int32)
    at[0] = 0
    rows = np.arange(n)
    for level in range(depth):
        cur = at[level]
        live = cur >= 0
        q = np.where(live, cur, 0)
        split = live & (nodes["status"][q] == 2)
        f = np.where(split, nodes["feat"][q], 0)
        b = bins[rows, f]
        left = np.where(b == 255, nodes["default_left"][q] == 1, b.astype(np.int64) <= nodes["bin"][q])
        at[level + 1] = np.where(split, 2 * q + np.where(left, 1, 2), -1)
    return at


def leaf_keys(at: np.ndarray, order: str = "dfs") -> np.ndarray:
    """Sort key of every row: the leaf it stopped in (``at`` from walk_levels). 'heap': the heap index;
    'dfs': the left-most bottom-level position under that leaf, 0 .. 2^depth - 1."""
    depth = at.shape[0] - 1
    level = (at >= 0).sum(axis=0) - 1  # the leaf's level
    leaf = at[level, np.arange(at.shape[1])].astype(np.int64)
    if order == "heap":
        return leaf
    return ((leaf + 1) << (depth - level)) - (1 << depth)


def reorder(perm: np.ndarray, keys: np.ndarray) -> np.ndarray:
    """Stable sort of the current order ``perm`` (position -> original row) by the rows' keys."""
    return perm[np.argsort(keys[perm], kind="stable")]


def positions(perm: np.ndarray) -> np.ndarray:
    """original row -> position."""
    pos = np.empty_like(perm)
    pos[perm] = np.arange(len(perm), dtype=perm.dtype)
    return pos


def distinct_units(node: np.ndarray, pos: np.ndarray, rows_per_unit: int) -> int:
    """Sum over the nodes of the distinct units (``rows_per_unit`` consecutive positions) that the
    node's rows touch. ``node`` and ``pos`` are per selected row."""
    if len(node) == 0:
        return 0
    unit = pos.astype(np.int64) // rows_per_unit
    span = int(unit.max()) + 1
    return int(np.unique(node.astype(np.int64) * span + unit).size)


def packed_units(node: np.ndarray, rows_per_unit: int) -> int:
    """The same sum with every node's rows packed back to back from a unit boundary."""
    if len(node) == 0:
        return 0
    return int(((np.bincount(node) + rows_per_unit - 1) // rows_per_unit).sum())


def level_counts(nodes: np.ndarray, at: np.ndarray, pos: np.ndarray) -> np.ndarray:
    """[depth, 4] per level: rec64 of the built children (level 0: the root), its packed ideal, col32 of
    the split nodes, its packed ideal."""
    depth = at.shape[0] - 1
    out = np.zeros((depth, 4), dtype=np.int64)
    for level in range(depth):
        cur = at[level]
        q = np.where(cur >= 0, cur, 0)
        live = (cur >= 0) & (nodes["status"][q] >= 1)
        built = live & ((nodes["build"][q] == 1) | (level == 0))
        split = live & (nodes["status"][q] == 2)
        out[level, 0] = distinct_units(cur[built], pos[built], RECORD_UNIT // RECORD_BYTES)
        out[level, 1] = packed_units(cur[built], RECORD_UNIT // RECORD_BYTES)
        out[level, 2] = distinct_units(cur[split], pos[split], COLUMN_SECTOR)
        out[level, 3] = packed_units(cur[split], COLUMN_SECTOR)
    return out


def train_host(n_rows: int, n_trees: int, depth: int, seed: int):
    """The bench fit (eta 0.05, gamma 5, lambda 1, max_bin 256, scale_pos_weight neg/pos, seed 78) on
    the host oracle: yields (tree index, heap nodes) and returns through ``bins`` the binned rows."""
    import torch

    from cobalt_smart_lender_ai_amd.dataio import synth
    from cobalt_smart_lender_ai_amd.models import gbdt, gbdt_host
    from cobalt_smart_lender_ai_amd.models.booster import Booster

    X, y = synth.make_lendingclub(n_rows, seed=seed, device="cpu")
    bd = gbdt.bin_dataset(X, max_bin=256, device="cpu")
    y = y.numpy().astype(np.float32)
    pos = float(y.sum())
    spw = (n_rows - pos) / pos
    w = np.where(y == 1.0, np.float32(spw), np.float32(1.0)).astype(np.float32)
    base = float(np.float32(min(max(float((w.astype(np.float64) * y).sum() / w.astype(np.float64).sum()), 1e-6),
                                1 - 1e-6)))
    margin = np.full(n_rows, np.float32(Booster([], base_score=base, num_feature=X.shape[1]).base_margin), np.float32)
    gs, hs = gbdt_host.quant_scales(float(w.max()))
    hp = gbdt_host.HostGbdtParams(max_depth=depth, eta=0.05, reg_lambda=1.0, reg_alpha=0.0, gamma=5.0,
                                  min_child_weight=1.0, subsample=1.0, seed=78, gscale=gs, hscale=hs)
    cuts, nbins = bd.cuts.numpy(), bd.nbins.numpy()
    fmask = np.ones(X.shape[1], np.uint8)
    del X
    torch.set_num_threads(1)

    def trees():
        for t in range(n_trees):
            gq, hq = gbdt_host.gradients_host(margin, y, w, hp, t)
            yield t, gbdt_host.grow_tree_host(bd.bins_host, cuts, nbins, gq, hq, margin, hp, fmask)
    return bd.bins_host, trees()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=300_000)
    ap.add_argument("--trees", type=int, default=40)
    ap.add_argument("--depth", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--schedule", action="append", default=None, help="repeatable; see above")
    ap.add_argument("--key", action="append", choices=["dfs", "heap"], default=None, help="repeatable")
    a = ap.parse_args()
    scheds = a.schedule or ["0", "0,8,32", "every:16", "every:4", "every:1"]
    variants = [("natural", [], "dfs")] + [(f"{s} [{k}]", parse_schedule(s, a.trees), k)
                                           for s in scheds for k in (a.key or ["dfs"])]
    t0 = time.perf_counter()
    bins, trees = train_host(a.rows, a.trees, a.depth, a.seed)
    perms = [np.arange(a.rows, dtype=np.int64) for _ in variants]
    poss = [positions(p) for p in perms]
    sums = np.zeros((len(variants), a.depth, 4), dtype=np.int64)
    late = np.zeros_like(sums)  # the same over the last quarter of the trees (how a schedule ages)
    counted = n_late = 0
    for t, nodes in trees:
        at = walk_levels(nodes, bins, a.depth)
        if t >= 1:  # tree 0 runs before any reorder
            counted += 1
            n_late += t >= a.trees - a.trees // 4
            for v in range(len(variants)):
                c = level_counts(nodes, at, poss[v])
                sums[v] += c
                if t >= a.trees - a.trees // 4:
                    late[v] += c
        for v, (_, sched, key) in enumerate(variants):
            if t in sched:
                perms[v] = reorder(perms[v], leaf_keys(at, key))
                poss[v] = positions(perms[v])
        print(f"# tree {t} done, {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)
    print(f"rows {a.rows}  trees {a.trees}  depth {a.depth}  (per-tree means over trees 1..{a.trees - 1}; "
          f"'late' = the last {n_late} trees)")
    print("rec64: 64-byte units of the 32-byte records under the built children's rows (k_hist)")
    print("col32: 32-byte sectors of the split feature's byte column under the split nodes' rows (k_part_pos)")
    for name, tot, n in (("all", sums, counted), ("late", late, n_late)):
        if n == 0:
            continue
        for col, what in ((0, "rec64"), (2, "col32")):
            print(f"\n{what}, {name} trees: mean units per tree and level (ratio to natural)")
            print(f"{'schedule':<22}" + "".join(f"{'L' + str(lv):>17}" for lv in range(a.depth)) + f"{'L1..':>17}")
            rows_out = [("ideal (packed)", tot[0, :, col + 1])] + [(variants[v][0], tot[v, :, col])
                                                                   for v in range(len(variants))]
            nat = tot[0, :, col].astype(np.float64)
            for label, r in rows_out:
                cells = [f"{r[lv] / n:>10.0f} {r[lv] / max(nat[lv], 1):>5.2f}x" for lv in range(a.depth)]
                deep = f"{r[1:].sum() / n:>10.0f} {r[1:].sum() / max(nat[1:].sum(), 1):>5.2f}x"
                print(f"{label:<22}" + "".join(cells) + deep)
    print("\n" + json.dumps({"rows": a.rows, "trees": a.trees, "variants": [v[0] for v in variants],
                             "rec64": (sums[:, :, 0] / max(counted, 1)).round(1).tolist(),
                             "col32": (sums[:, :, 2] / max(counted, 1)).round(1).tolist()}))


if __name__ == "__main__":
    main()
