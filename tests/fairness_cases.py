"""Inputs shared by the fairness tests (test_fairness_cpu.py, test_gpu_fairness.py)."""
import numpy as np

SEED = 20240611
CUTOFFS = {1: [0.5], 2: [0.5, 0.35], 16: [0.5, 0.9, 0.1, 0.35, 0.35, 0.75, 0.2, 0.6, 0.05, 0.45, 0.55, 0.65, 0.3, 0.8,
                                         0.95, 0.5]}   # unsorted, with duplicates


def population(n: int, G: int, seed: int = 0, labels: bool = True):
    """``rows`` (the original indices, a permutation of ``0 .. n - 1``: no row stands where its index says),
    float32 ``score`` in [0, 1] (the values 0, 1 and the cutoff 0.5 among them when there is room), ``group`` codes
    in ``0 .. G - 1`` and 0/1 ``y`` (or None). Scores and bad rates differ by group."""
    rng = np.random.default_rng([seed, n, G])
    rows = rng.permutation(n).astype(np.int64)
    group = rng.integers(0, G, size=n).astype(np.int64)
    score = np.clip(rng.beta(2.0, 2.0, size=n) + 0.04 * (group % 3), 0.0, 1.0).astype(np.float32)
    for pos, v in zip(rng.permutation(n)[:6], (0.0, 1.0, 0.5, 0.5, 0.35, np.float32(0.5) + np.float32(2.0 ** -24))):
        score[pos] = v
    y = (rng.random(n) < 0.15 + 0.7 * score).astype(np.int64) if labels else None
    return rows, score, group, y


def audit_population(n: int = 1200, seed: int = 1):
    """Scores, two attributes (strings) and outcomes for the report tests: three and two groups, the smallest of
    at least 50 rows, approval and bad rates of every group between 0.2 and 0.8 at the cutoff 0.5."""
    rng = np.random.default_rng(seed)
    region = rng.choice(["north", "south", "west"], size=n, p=[0.5, 0.3, 0.2])
    age = rng.choice(["under40", "over40"], size=n)
    shift = 0.06 * (region == "south") - 0.04 * (age == "over40")
    score = np.clip(rng.beta(2.5, 2.5, size=n) + shift, 0.0, 1.0).astype(np.float32)
    y = (rng.random(n) < 0.2 + 0.6 * score).astype(np.int64)
    return score, {"region": region, "age": age}, y


def two_groups(n_a: int, declined_a: int, n_b: int, declined_b: int, cutoff: float = 0.5):
    """Scores and string groups with exact counts: group A has ``n_a`` rows, ``declined_a`` of them above the
    cutoff; group B likewise."""
    score = np.concatenate([np.full(declined_a, cutoff + 0.2), np.full(n_a - declined_a, cutoff - 0.2),
                            np.full(declined_b, cutoff + 0.2), np.full(n_b - declined_b, cutoff - 0.2)])
    group = np.array(["A"] * n_a + ["B"] * n_b)
    return score.astype(np.float32), group
