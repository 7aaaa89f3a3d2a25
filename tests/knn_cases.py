"""Inputs, a plain fp64 reference and the accuracy contract of the SMOTE k-nearest-neighbour search
(csrc/knn.hip k_knn<K> behind nn/smote.py kneighbors), shared by test_knn_cases_cpu.py (which checks the
contract and every case against a NumPy model of the kernel's arithmetic, so that a wrong contract or a
toothless case cannot pass a GPU test) and test_gpu_knn_edges.py (which checks the kernel). NumPy only.

The kernel forms d^2 = |r|^2 + |q|^2 - 2 r.q in fp32, so it cannot be exact and the tests cannot ask for the
reference's indices: two rows whose distances differ by less than the formula's error may come out in either
order. ``tau`` bounds that error, ``assert_knn_contract`` asks for everything the bound decides, and each case is
built so that the bound decides at least ``MIN_DECIDED`` of its (query, slot) pairs -- a contract that decided
little would pass anything.

Known limit, deliberately not a case: tau is relative to the spread of R about its column mean, so two tight
clusters at +-1000 with spacing 0.01 stay undecided after centring (tau ~ 2e-6 * 1e6 against gaps of 1e-4).
That is a property of the fp32 formula, not a defect the tests could pin; such data belongs on device="cpu".
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24                                  # fp32 unit roundoff
COMPILED_K = (1, 2, 3, 4, 5, 6, 7, 8, 11, 16)   # the K the kernel is instantiated for
MIN_DECIDED = 0.95


# ------------------------------------------------------------------------------------------ reference, bound
def sqdist(Q, R) -> np.ndarray:
    """[nq, nr] exact-as-fp64-gets squared distances by brute force on the differences (no norm trick)."""
    Q, R = np.asarray(Q, dtype=np.float64), np.asarray(R, dtype=np.float64)
    D = np.empty((len(Q), len(R)), dtype=np.float64)
    for a in range(0, len(Q), 128):
        diff = Q[a:a + 128, None, :] - R[None, :, :]
        D[a:a + 128] = np.einsum("qrf,qrf->qr", diff, diff)
    return D


def reference(Q, R, k):
    """(idx [nq, k] int64, d2 [nq, k] float64): the k nearest rows of R for every row of Q from fp64 brute-force
    squared distances of the inputs as given (no fp32 cast), ordered by (d^2, index) -- a stable argsort."""
    D = sqdist(Q, R)
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int64), np.take_along_axis(D, idx, axis=1)


def tau(Q, R) -> np.ndarray:
    """[nq, nr] bound on |d^2_kernel - d^2_exact| for every pair, derived from the formula, not measured:

        tau(q, r) = (2 F + 8) u S,   S = |q - mu|^2 + |r - mu|^2,   u = 2^-24,   mu = fp64 column mean of R.

    kneighbors subtracts mu in fp64 and casts to fp32; the kernel then computes, all in fp32,
    fl(fl(rn + qn) - 2 acc) with rn, qn chains of F fmas and acc a chain of F exact products. First order in u:
      * the two norms: each chain of F fmas errs by at most F u |x|^2 ................................ F u S
      * the dot product: F u sum|q_i r_i| <= F u S / 2, and the formula doubles it ................... F u S
      * the two final adds: u (rn + qn) = u S, then u d^2 <= 2 u S .................................. 3 u S
      * the fp32 rounding of each centred coordinate, x(1 + delta): 2 u sum|q_i - r_i|(|q_i| + |r_i|)
        <= 2 u sqrt(d^2) sqrt(2 S) <= 4 u S ......................................................... 4 u S
    which is (2 F + 7) u S for every distance the kernel compares; the eighth unit is slack. The distance that
    kneighbors returns went through an fp32 sqrt as well, and squaring it back costs 2 u d^2: inside the slack
    while d^2 <= S / 2, and up to 4 u S (constant 2 F + 11) for two rows opposite each other about mu. The
    F-proportional terms are worst-case sums that random roundings come nowhere near, so the returned distances
    are held to the same (2 F + 8); ``worst_dist_ratio`` reports how much of it a run used. On an MI355X no case
    needed a larger constant: the largest |dist^2 - d^2_ref| / tau over all cases was 0.35 (F1_wide_1e5), 0.23 on
    the N(0,1) cases; the NumPy model of the formula gives the same 0.35."""
    Q, R = np.asarray(Q, dtype=np.float64), np.asarray(R, dtype=np.float64)
    mu = R.mean(axis=0)
    nq2 = ((Q - mu) ** 2).sum(axis=1)
    nr2 = ((R - mu) ** 2).sum(axis=1)
    return (2 * Q.shape[1] + 8) * U * (nq2[:, None] + nr2[None, :])


def _checked(idx, dist, Q, R, k):
    idx, dist = np.asarray(idx), np.asarray(dist, dtype=np.float64)
    nq, nr = len(Q), len(R)
    assert idx.shape == (nq, k) and dist.shape == (nq, k), (idx.shape, dist.shape, (nq, k))
    assert idx.dtype.kind in "iu", idx.dtype
    return idx.astype(np.int64), dist, nq, nr


def worst_dist_ratio(idx, dist, Q, R) -> float:
    """max |dist^2 - d^2_ref| / tau over the returned pairs (0 where tau is 0 and the distance exact)."""
    idx, dist = np.asarray(idx, dtype=np.int64), np.asarray(dist, dtype=np.float64)
    err = np.abs(dist * dist - np.take_along_axis(sqdist(Q, R), idx, axis=1))
    t = np.take_along_axis(tau(Q, R), idx, axis=1)
    r = np.where(err == 0, 0.0, err / np.where(t > 0, t, 1.0))
    r[(t == 0) & (err > 0)] = np.inf
    return float(r.max(initial=0.0))


def assert_knn_contract(idx, dist, Q, R, k) -> float:
    """Everything tau decides about ``idx`` [nq, k] and the Euclidean ``dist`` [nq, k]; tau_q = max_r tau(q, r).

    1. every reference row with d^2_ref < d^2_ref[(k+1)-th nearest] - 2 tau_q is in ``idx`` (if it were not, a
       returned row of true rank > k would have to beat it, and their computed distances cannot cross);
    2. every returned row has d^2_ref <= d^2_ref[k-th nearest] + 2 tau_q (else the k true nearest all beat it);
    3. every returned distance has |dist^2 - d^2_ref| <= tau(q, r);
    and indices lie in [0, nr), no row repeats an index, ``dist`` is >= 0 and non-decreasing along each row.
    Returns the decided share: the fraction of (query, slot) pairs that rule 1 forces."""
    idx, dist, nq, nr = _checked(idx, dist, Q, R, k)
    assert 1 <= k <= nr
    assert idx.min() >= 0 and idx.max() < nr, ("index outside [0, nr)", int(idx.min()), int(idx.max()), nr)
    srt = np.sort(idx, axis=1)
    assert not (srt[:, 1:] == srt[:, :-1]).any(), ("a row repeats an index", np.argwhere(srt[:, 1:] == srt[:, :-1])[:4])
    assert not np.isnan(dist).any() and dist.min() >= 0, "negative or NaN distance"
    assert (np.diff(dist, axis=1) >= 0).all(), ("dist decreases along a row", np.argwhere(np.diff(dist, axis=1) < 0)[:4])

    D, T = sqdist(Q, R), tau(Q, R)
    tq = T.max(axis=1)
    Ds = np.sort(D, axis=1)
    d_k = Ds[:, k - 1]
    d_k1 = Ds[:, k] if nr > k else np.full(nq, np.inf)
    forced = D < (d_k1 - 2 * tq)[:, None]
    present = np.zeros((nq, nr), dtype=bool)
    np.put_along_axis(present, idx, True, axis=1)
    miss = np.argwhere(forced & ~present)
    assert len(miss) == 0, ("decided neighbours missing (query, ref)", len(miss), miss[:6].tolist())
    d_ret = np.take_along_axis(D, idx, axis=1)
    far = np.argwhere(d_ret > (d_k + 2 * tq)[:, None])
    assert len(far) == 0, ("returned rows beyond the k-th nearest + 2 tau (query, slot)", len(far), far[:6].tolist())
    err = np.abs(dist * dist - d_ret)
    off = np.argwhere(err > np.take_along_axis(T, idx, axis=1))
    assert len(off) == 0, ("returned distances off by more than tau (query, slot)", len(off), off[:6].tolist(),
                           worst_dist_ratio(idx, dist, Q, R))
    return float(forced.sum()) / (nq * k)


def self_is_decided_first(R) -> np.ndarray:
    """[nr] bool, for Q = R: the row's nearest other row is more than 2 tau_q away, so the row itself (d^2 = 0,
    computed within tau) must come out in column 0."""
    if len(R) < 2:
        return np.ones(len(R), dtype=bool)
    return np.sort(sqdist(R, R), axis=1)[:, 1] > 2 * tau(R, R).max(axis=1)


# ------------------------------------------------------------------------------------------ exact duplicates
def assert_duplicates_in_index_order(idx, R) -> int:
    """Rows of R that are exact copies of each other get bit-identical distances wherever they sit in a tile, so
    the (distance, index) order must list the copies it returns by ascending index and, when it returns only
    some of a group, the lowest indices of it. Exact; returns the number of groups seen split."""
    R = np.asarray(R, dtype=np.float64)
    _, gid = np.unique(R, axis=0, return_inverse=True)
    gid = gid.reshape(-1)
    members = {g: np.flatnonzero(gid == g) for g in np.unique(gid)}
    split = 0
    for q, row in enumerate(np.asarray(idx, dtype=np.int64)):
        g = gid[row]
        for grp in np.unique(g):
            pos = np.flatnonzero(g == grp)
            got = row[pos]
            assert (np.diff(got) > 0).all(), ("copies not by ascending index", q, row.tolist())
            assert np.array_equal(got, members[grp][:len(got)]), ("not the lowest copies", q, row.tolist())
            split += len(got) < len(members[grp])
    return split


# ------------------------------------------------------------------------------------------ the kernel's arithmetic
def _fma32(a, b, s):
    """fp32 fma through fp64: the product of two fp32 is exact in fp64; the sum rounds twice (fp64, fp32)."""
    return (a.astype(np.float64) * b.astype(np.float64) + s.astype(np.float64)).astype(np.float32)


def model_knn(Q, R, k, centre=True):
    """(idx, dist) of a NumPy model of the kernel's formula: fp32 norms and dot product by sequential fma on
    ``float32(X - mu)`` (``centre=False``: on ``float32(X)``, the formula before kneighbors centred),
    d = fl(fl(rn + qn) - 2 dot), order (d, index), dist = fp32 sqrt(max(d, 0)). The MFMA's summation order is not
    modelled -- this checks the contract and the cases, not the kernel."""
    Q, R = np.asarray(Q, dtype=np.float64), np.asarray(R, dtype=np.float64)
    mu = R.mean(axis=0) if centre else np.zeros(R.shape[1])
    q, r = (Q - mu).astype(np.float32), (R - mu).astype(np.float32)
    qn, rn = np.zeros(len(q), np.float32), np.zeros(len(r), np.float32)
    dot = np.zeros((len(q), len(r)), np.float32)
    for f in range(q.shape[1]):
        qn, rn = _fma32(q[:, f], q[:, f], qn), _fma32(r[:, f], r[:, f], rn)
        dot = _fma32(q[:, f:f + 1], r[None, :, f], dot)
    t = (rn[None, :] + qn[:, None]).astype(np.float32)
    d = (t.astype(np.float64) - 2.0 * dot.astype(np.float64)).astype(np.float32)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int64), np.sqrt(np.maximum(np.take_along_axis(d, idx, axis=1), np.float32(0)))


# ------------------------------------------------------------------------------------------ the cases
MIXED_OFFSET = np.array([5e4, 1.2e4, 700.0, 15.0, 0.0, 3e3, 1.0])
MIXED_SCALE = np.array([1.0, 10.0, 100.0, 1.0, 1.0, 5.0, 0.1])


def mixed_frame(rng, n) -> np.ndarray:
    """A loan-like frame: 7 columns of very different offset and scale (amounts, incomes, day counts, rates)."""
    return rng.normal(size=(n, 7)) * MIXED_SCALE + MIXED_OFFSET


def _case(name, Q, R, k, **kw):
    assert R.shape[1] == Q.shape[1] and 1 <= k <= len(R) and k in COMPILED_K
    return dict(name=name, Q=Q, R=R, k=k, **kw)


def _build_cases():
    out = []
    seed = iter(range(1000, 2000))

    def rng():
        return np.random.default_rng(next(seed))

    # shape edges on N(0,1): the reference count around the 32-row sub-tile and the 256-row LDS pass
    for k in (1, 6, 16):
        for nr in sorted({k, k + 1, 31, 32, 33, 255, 256, 257, 513}):
            g = rng()
            R = g.normal(size=(nr, 20))
            out.append(_case(f"nr{nr}_k{k}", R, R, k) if nr <= 33 else _case(f"nr{nr}_k{k}", g.normal(size=(70, 20)), R, k))
    # K = 16 where a lane half holds fewer than K rows: INF sentinels pass through the half merge
    for nr in (16, 17, 20):
        g = rng()
        out.append(_case(f"sentinel_nr{nr}_k16", g.normal(size=(35, 9)), g.normal(size=(nr, 9)), 16))
    # the query count around the 32-query wave and the 128-query workgroup, Q != R
    for nq in (1, 31, 33, 127, 128, 129, 300):
        g = rng()
        out.append(_case(f"nq{nq}", g.normal(size=(nq, 7)), g.normal(size=(200, 7)), 5))
    # the width: odd F zero-pads the last MFMA k pair, 32 is the widest
    for F in (1, 2, 3, 19, 20, 31, 32):
        g = rng()
        out.append(_case(f"F{F}", g.normal(size=(150, F)), g.normal(size=(300, F)), 6))
    # every compiled K
    for k in COMPILED_K:
        g = rng()
        out.append(_case(f"K{k}", g.normal(size=(129, 7)), g.normal(size=(300, 7)), k))
    # off the origin: what the un-centred formula gets wrong
    g = rng()
    R = g.normal(size=(777, 20)) + 1e4
    out.append(_case("plus1e4", R, R, 6, off_origin=True))
    R = mixed_frame(rng(), 600)
    out.append(_case("mixed_scale", R, R, 6, off_origin=True))
    R = rng().normal(1e5, 100.0, size=(257, 1))
    out.append(_case("F1_wide_1e5", R, R, 6, off_origin=True))
    g = rng()
    R = g.normal(size=(300, 20)) - 1e4
    out.append(_case("minus1e4", g.normal(size=(140, 20)) - 1e4, R, 6, off_origin=True))
    # exact duplicates: every row three times, shuffled; k a multiple of 3 keeps whole groups decided
    for name, off in (("dups_origin", 0.0), ("dups_plus1e4", 1e4)):
        g = rng()
        base = g.normal(size=(100, 8)) + off
        R = np.repeat(base, 3, axis=0)[g.permutation(300)]
        out.append(_case(name, R, R, 6, duplicates=True, off_origin=off != 0))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return {c["name"]: c for c in out}


CASES = _build_cases()
CASE_NAMES = tuple(CASES)
OFF_ORIGIN_CASES = tuple(n for n, c in CASES.items() if c.get("off_origin"))
DUPLICATE_CASES = tuple(n for n, c in CASES.items() if c.get("duplicates"))
GRID_CASES = ("nq300", "mixed_scale", "K16")     # re-run with the queries reversed and shifted by 37 rows
# The duplicate cases are run a second time with this k, which cuts the second group of three copies: which copies
# of a 3-way exact tie are returned is then decided by the index rule alone (no distance bound can decide it, so
# these runs are held to the contract and the duplicate order, not to MIN_DECIDED, and are not in CASES).
DUPLICATE_CUT_K = 4


def regrid(Q, rng_seed=7):
    """The two re-arrangements of the grid-independence check: ``(Q2, rows)`` pairs with ``Q2[rows] == Q``:
    Q reversed, and Q behind 37 other rows (so every query changes wave, lane and, past 91, workgroup)."""
    Q = np.asarray(Q, dtype=np.float64)
    n = len(Q)
    g = np.random.default_rng(rng_seed)
    pad = Q.mean(axis=0) + g.normal(size=(37, Q.shape[1])) * Q.std(axis=0).clip(1e-3)
    return [(Q[::-1].copy(), np.arange(n)[::-1]), (np.vstack([pad, Q]), np.arange(37, 37 + n))]


@functools.lru_cache(maxsize=None)
def decided_share_of_reference(name) -> float:
    """The decided share of the case as the fp64 reference itself sees it (its own answer always passes)."""
    c = CASES[name]
    idx, d2 = reference(c["Q"], c["R"], c["k"])
    return assert_knn_contract(idx, np.sqrt(d2), c["Q"], c["R"], c["k"])


# ------------------------------------------------------------------------------------------ the SMOTE frame
SMOTE_SEED = 1  # the first seed that meets smote_neighbours_decided (test_knn_cases_cpu.py asserts it does)


def smote_neighbours_decided(Xc, k_neighbors) -> bool:
    """True when, for every row of the class, the squared distances to its k+2 nearest rows (itself, its k
    neighbours and the first row left out) are pairwise more than 2 tau_q apart: then no fp32 rounding within tau
    can change which rows SMOTE sees or the column each sits in, and cuda and cpu must agree exactly."""
    Ds = np.sort(sqdist(Xc, Xc), axis=1)[:, :k_neighbors + 2]
    tq = tau(Xc, Xc).max(axis=1)
    return bool((np.diff(Ds, axis=1) > 2 * tq[:, None]).all())


def smote_frame(seed=SMOTE_SEED):
    """(X [600, 7] mixed scale and offset, y with a 13 % minority) for the cuda-vs-cpu fit_resample comparison."""
    g = np.random.default_rng(seed)
    X = mixed_frame(g, 600)
    y = np.zeros(600, dtype=np.int64)
    y[g.permutation(600)[:78]] = 1
    return X, y
