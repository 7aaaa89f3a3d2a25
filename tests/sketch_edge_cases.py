"""Small hand-shaped inputs and a plain oracle for the exact device quantile sketch (csrc/sketch.hip,
models/sketch.py _exact_core), shared by test_sketch_edges_cpu.py (which checks the oracle against
``compute_cuts`` and every case's designed properties) and test_gpu_sketch_edges.py (which checks the kernels
against the oracle). Everything here is NumPy with int64 / Python integers; nothing calls ``compute_cuts``.

A case is a named function returning a :class:`Built`: ``X`` (a CPU tensor, possibly a view), optional weights,
optional ``sample_rows`` and the properties it was designed to have, as a dict that ``measure`` recomputes from
the inputs alone (the NumPy mirror of the sketch's bucket arithmetic). Every case runs unit-weighted and
weighted: with its own weights where it has them, else with ``arange % 11`` (zero-weight rows included).
"""
from __future__ import annotations

import dataclasses
import functools
import math
from typing import Callable

import numpy as np
import torch

FLT_MAX = np.float32(np.finfo(np.float32).max)
WEIGHT_SCALE = 1 << 20
NBND = 4096                 # boundary table (kSkMaxBounds): <= 4095 real boundaries, +inf padding
KPOS = NBND - 1             # positions k * cnt // 4095 of the sorted sample
NB = 2 * NBND + 1           # buckets (kSkBuckets): 2k+1 = {u_k}, 2k = (u_{k-1}, u_k)
SORT_CAP = 8192             # kSkSortCap: the largest segment the select kernels sort in LDS
SAMPLE_CAP = 32768          # kSkSampleCap: the largest sample k_sk_sample_bounds sorts
DEFAULT_SAMPLE_ROWS = 1 << 15
MAX_ROWS, MAX_FEATURES = 131_076, 33


# ------------------------------------------------------------------------------------------ the oracle
def quantize_np(w, n: int) -> np.ndarray:
    """Integer sketch weights: ``round(w / max(w) * 2^20)``; ones when ``w`` is None or ``max(w) <= 0``."""
    if w is None:
        return np.ones(n, dtype=np.int64)
    wd = np.asarray(w, dtype=np.float64).reshape(-1)
    if wd.size == 0 or float(wd.max()) <= 0:
        return np.ones(n, dtype=np.int64)
    return np.round(wd * (WEIGHT_SCALE / float(wd.max()))).astype(np.int64)


def _cuts_np(X, w, max_bin, has_missing, strict: bool, canon: bool, shift: int = 0):
    X = np.asarray(X, dtype=np.float32)
    n, F = X.shape
    wq = quantize_np(w, n)
    cuts = np.full((F, 256), FLT_MAX, dtype=np.float32)
    nbins = np.ones(F, dtype=np.int32)
    for f in range(F):
        x = X[:, f] + np.float32(0.0)
        ok = ~np.isnan(x)
        miss = bool((~ok).any()) if has_missing is None else bool(has_missing[f])
        maxb = min(int(max_bin), 255 if miss else 256)
        order = np.argsort(x, kind="stable")
        order = order[ok[order]]
        xs = x[order]
        if len(xs) == 0:
            continue
        if canon:
            first = np.r_[True, xs[1:] != xs[:-1]]
        else:  # the wrong variant that tells -0.0 from +0.0 (test_sketch_edges_cpu.py sensitivity checks)
            bits = X[order, f].view(np.int32)
            first = np.r_[True, bits[1:] != bits[:-1]]
        distinct = xs[first]
        if len(distinct) <= maxb:
            out = list(distinct[1:])
        else:
            cum = np.cumsum(wq[order])
            W = int(cum[-1])
            key = cum * maxb
            out = []
            for j in range(1, maxb):
                i = int(np.searchsorted(key, j * W, side="right" if strict else "left"))
                v = xs[min(i + shift, len(xs) - 1)]
                if v > xs[0] and (not out or v != out[-1]):
                    out.append(v)
        cuts[f, :len(out)] = np.asarray(out, dtype=np.float32)
        nbins[f] = len(out) + 1
        cuts[f, nbins[f] - 1:] = FLT_MAX
    return cuts, nbins


def cuts_oracle_np(X, w, max_bin: int = 256, has_missing=None):
    """(cuts [F, 256] float32, nbins [F] int32) of every row of ``X`` [n, F]: per feature the values are
    canonicalised (``+ 0.0``), NaN dropped, stable-sorted; ``maxb`` = 255 with a missing value, else 256, capped
    by ``max_bin``; <= maxb distinct values give one bin each (cuts = the distinct values from the second on);
    otherwise cut j = 1..maxb-1 is the first value whose cumulative integer weight satisfies
    ``cum_i * maxb > j * W`` (clamped to the last valid row), kept when above the minimum and different from
    its predecessor. FLT_MAX sits in slot ``nbins - 1`` and every later slot; no valid value: ``nbins = 1``."""
    return _cuts_np(X, w, max_bin, has_missing, True, True)


def cuts_off_by_one_np(X, w, max_bin: int = 256, has_missing=None):
    """A deliberately WRONG sketch: ``>=`` for ``>`` in the threshold rule (one order statistic early)."""
    return _cuts_np(X, w, max_bin, has_missing, False, True)


def cuts_one_late_np(X, w, max_bin: int = 256, has_missing=None):
    """A deliberately WRONG sketch: every target answered by the next order statistic."""
    return _cuts_np(X, w, max_bin, has_missing, True, True, 1)


def cuts_signed_zero_np(X, w, max_bin: int = 256, has_missing=None):
    """A deliberately WRONG sketch: -0.0 and +0.0 counted as two distinct values."""
    return _cuts_np(X, w, max_bin, has_missing, True, False)


# ------------------------------------------------------------------------------- the bucket arithmetic
def sample_stride(n: int, sample_rows: int | None) -> int:
    sr = DEFAULT_SAMPLE_ROWS if sample_rows is None else int(sample_rows)
    return 1 if sr <= 0 or n <= sr else int(math.ceil(n / sr))


def bounds_np(col) -> tuple[np.ndarray, int]:
    """Boundaries of one sample column: the sorted valid values at positions ``k * cnt // 4095`` that differ
    from their predecessor, in a [4096] table padded with +inf; and their number ``m``."""
    v = np.asarray(col, dtype=np.float32) + np.float32(0.0)
    v = np.sort(v[~np.isnan(v)], kind="stable")
    u = np.full(NBND, np.inf, dtype=np.float32)
    if len(v) == 0:
        return u, 0
    x = v[(np.arange(KPOS, dtype=np.int64) * len(v)) // KPOS]
    d = x[np.r_[True, x[1:] != x[:-1]]]
    u[:len(d)] = d
    return u, len(d)


def buckets_np(u: np.ndarray, m: int, col) -> np.ndarray:
    """Bucket of every value of ``col`` (int64; 0xFFFF for NaN): ``2k + 1`` when it equals boundary k, else
    ``2k`` with k = the number of boundaries below it."""
    v = np.asarray(col, dtype=np.float32) + np.float32(0.0)
    ok = ~np.isnan(v)
    k = np.searchsorted(u[:m], v[ok], side="left")
    eq = (k < m) & (u[np.minimum(k, NBND - 1)] == v[ok])
    b = np.full(len(v), 0xFFFF, dtype=np.int64)
    b[ok] = 2 * k + eq
    return b


def nblk_of(n: int) -> int:
    return max(1, min(64, -(-n // 65536)))


@dataclasses.dataclass
class Built:
    X: torch.Tensor                       # [n, F] CPU tensor (any float dtype, any strides)
    w: np.ndarray | None = None           # the case's own weights (float64), else None
    sample_rows: int | None = None        # None: the sketch's default (2^15)
    props: dict = dataclasses.field(default_factory=dict)
    on_device: Callable | None = None     # dev -> the same X on the device with the same layout

    def x32(self) -> np.ndarray:
        return self.X.to(torch.float32).contiguous().numpy()

    def weights(self, weighted: bool) -> np.ndarray | None:
        if not weighted:
            return None
        return self.w if self.w is not None else (np.arange(self.X.shape[0]) % 11).astype(np.float64)

    def to(self, dev) -> torch.Tensor:
        return self.on_device(dev) if self.on_device is not None else self.X.to(dev)


def measure(b: Built, weighted: bool) -> dict:
    """What the sketch does with this input, recomputed in NumPy: the sample size ``S``, pass 1's block count and
    row-range alignment, and per feature the boundaries ``m``, the distinct count ``nd`` against ``maxb``, the
    class k_sk_plan1 decides (many / exact / uncertain), the rows of the largest open bucket that holds a
    target (``seg_target``) and of the largest selected open bucket (``seg_any``: for an uncertain feature every
    open bucket with rows is selected). ``nseg``: selected buckets over all features."""
    X = b.x32()
    n, F = X.shape
    stride = sample_stride(n, b.sample_rows)
    samp = X[::stride]
    nblk = nblk_of(n)
    wq = quantize_np(b.weights(weighted), n)
    out = dict(n=n, F=F, S=samp.shape[0], stride=stride, nblk=nblk, n_mod4=n % 4, per_mod4=(-(-n // nblk)) % 4,
               contiguous=b.X.is_contiguous(), aligned16=(b.X.storage_offset() * b.X.element_size()) % 16 == 0,
               dtype=str(b.X.dtype).replace("torch.", ""), m=[], nd=[], maxb=[], cls=[], seg_target=[], seg_any=[],
               W=[], nseg=0)
    for f in range(F):
        col = X[:, f] + np.float32(0.0)
        ok = ~np.isnan(col)
        mb = 255 if (~ok).any() else 256
        u, m = bounds_np(samp[:, f])
        bk = buckets_np(u, m, col)[ok]
        cnt = np.bincount(bk, minlength=NB).astype(np.int64)
        wh = np.zeros(NB, dtype=np.int64)
        np.add.at(wh, bk, wq[ok])
        E, O = int((cnt[1::2] > 0).sum()), int((cnt[0::2] > 0).sum())
        many, exact_known = E + O > mb, O == 0 and E <= mb
        uncertain = not many and O > 0
        C = np.cumsum(wh)
        W = int(C[-1])
        j = np.arange(1, 256, dtype=np.int64)
        bt = np.minimum(np.searchsorted(C * mb, j * W, side="right"), NB - 1)
        need = (j < mb) & (bt % 2 == 0) & (W > 0) & (not exact_known)
        sel = np.zeros(NB, dtype=bool)
        sel[bt[need]] = True
        seg_t = int(cnt[sel].max()) if sel.any() else 0
        if uncertain:
            sel[0::2] |= cnt[0::2] > 0
        sel[NB - 1] = False
        out["m"].append(m)
        out["nd"].append(len(np.unique(col[ok])))
        out["maxb"].append(mb)
        out["cls"].append("many" if many else "exact" if exact_known else "uncertain")
        out["seg_target"].append(seg_t)
        out["seg_any"].append(int(cnt[sel].max()) if sel.any() else 0)
        out["W"].append(W)
        out["nseg"] += int(sel.sum())
    return out


# ------------------------------------------------------------------------------------------ the cases
CASES: dict[str, Callable[[], Built]] = {}


def case(name):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def build(name: str) -> Built:
    b = CASES[name]()
    n, F = b.X.shape
    assert n <= MAX_ROWS and F <= MAX_FEATURES, name
    return b


@functools.lru_cache(maxsize=None)
def oracle(name: str, weighted: bool):
    """The oracle's (cuts, nbins) of a case, computed once per session and shared (read-only)."""
    b = build(name)
    c, nb = cuts_oracle_np(b.x32(), b.weights(weighted))
    c.setflags(write=False)
    nb.setflags(write=False)
    return c, nb


def _continuous(n, F, seed):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, F)) * 100).astype(np.float32)
    if F > 1:  # the last column carries the missing values
        X[rng.random(n) < 0.1, F - 1] = np.nan
    return X


# ---- A. row count and layout
A_SHAPES = [(1, 1), (2, 3), (3, 4), (255, 3), (256, 32), (257, 32), (1025, 33), (65536, 4), (65537, 3), (65540, 4),
            (131073, 5), (131076, 4)]


def _a_case(n, F):
    def fn():
        nblk = nblk_of(n)
        return Built(torch.from_numpy(_continuous(n, F, 1000 + 37 * n + F)),
                     props=dict(n=n, F=F, nblk=nblk, n_mod4=n % 4, per_mod4=(-(-n // nblk)) % 4, contiguous=True,
                                aligned16=True, S=-(-n // sample_stride(n, None))))
    return fn


for _n, _F in A_SHAPES:
    case(f"A_{_n}x{_F}")(_a_case(_n, _F))


@case("A_misaligned_base_4099x5")
def _a_misaligned():
    n, F = 4099, 5
    flat = torch.zeros(1 + n * F, dtype=torch.float32)
    flat[1:] = torch.from_numpy(_continuous(n, F, 11)).reshape(-1)

    def view(t):
        return t[1:].view(n, F)
    return Built(view(flat), props=dict(contiguous=True, aligned16=False, n_mod4=3, nblk=1),
                 on_device=lambda dev: view(flat.to(dev)))


@case("A_noncontiguous_4099x5")
def _a_noncontiguous():
    n = 4099
    wide = torch.from_numpy(_continuous(n, 10, 12))
    wide[::9, 8] = float("nan")
    return Built(wide[:, ::2], props=dict(contiguous=False, F=5, n_mod4=3),
                 on_device=lambda dev: wide.to(dev)[:, ::2])


@case("A_float64_1025x3")
def _a_f64():
    rng = np.random.default_rng(13)
    X = rng.standard_normal((1025, 3)) * 100  # float64 values that round to float32
    X[::7, 2] = np.nan
    return Built(torch.from_numpy(X), props=dict(dtype="float64", n_mod4=1))


@case("A_float16_1025x3")
def _a_f16():
    X = torch.from_numpy(_continuous(1025, 3, 14)).to(torch.float16)
    return Built(X, props=dict(dtype="float16", n_mod4=1))


# ---- B. segment length: the sample is row 0 alone (0.0); the other L rows are positive, one open bucket
B_LENGTHS = [1, 2, 3, 1000, 4096, 4097, 8191, 8192, 8193, 20000]


def _b_distinct(L):
    def fn():
        rng = np.random.default_rng(2000 + L)
        x = np.r_[0.0, rng.permutation(L) + 1.0].astype(np.float32)
        return Built(torch.from_numpy(x[:, None]), sample_rows=1,
                     props=dict(S=1, m={0: 1}, cls={0: "uncertain"}, nd={0: L + 1}, seg_target={0: L},
                                seg_any={0: L}, nseg=1))
    return fn


def _b_dup(L):
    def fn():
        rng = np.random.default_rng(3000 + L)
        k = min(L, 200)
        vals = np.r_[np.arange(k), rng.integers(0, k, L - k)] * 0.5 + 1.0   # every one of the k values occurs
        x0 = np.r_[0.0, rng.permutation(vals)]
        x1 = np.r_[0.0, rng.permutation(L) + 1.0]                            # a distinct-valued neighbour
        X = np.stack([x0, x1], 1).astype(np.float32)
        return Built(torch.from_numpy(X), sample_rows=1,
                     props=dict(S=1, m={0: 1, 1: 1}, cls={0: "uncertain", 1: "uncertain"}, nd={0: k + 1, 1: L + 1},
                                seg_any={0: L, 1: L}, seg_target={0: L, 1: L}, nseg=2))
    return fn


for _L in B_LENGTHS:
    case(f"B_L{_L}_distinct")(_b_distinct(_L))
    case(f"B_L{_L}_dup200")(_b_dup(_L))


# ---- C. distinct-count thresholds
def _split(total, k):
    return [total // k + (1 if i < total % k else 0) for i in range(k)]


def _c_threshold(d, nan, mode):
    """Exactly ``d`` distinct values 0..d-1 over ``16 * maxb`` valid rows (plus one NaN row). mode "unsampled":
    the sample is row 0 (the minimum), every other value sits in one open bucket (k_sk_exact's count);
    "sampled": every value is a sample value (k_sk_plan1's equal-bucket count); "interleaved": every second
    value is a sample value, the others sit one per open bucket (k_sk_plan1's many / uncertain decision over
    equal + open buckets). Past ``maxb`` the multiplicities are 16 per value, but for one run of values that
    shares 16 rows: with unit weights every target rank j * W / maxb = 16 j then ends a run of equal values,
    so a rule that is off by one order statistic answers with the neighbouring value."""
    def fn():
        maxb = 255 if nan else 256
        W = 16 * maxb
        n = W + nan
        rng = np.random.default_rng(4000 + 10 * d + nan)
        counts = _split(W, d) if d <= maxb else [16] * 100 + _split(16, d - maxb + 1) + [16] * (maxb - 101)
        assert len(counts) == d and sum(counts) == W and min(counts) >= 5
        left = np.asarray(counts)
        x = np.full(n, -1.0)
        r = np.arange(n)
        if mode == "unsampled":
            sample_rows, sampled = 1, r[:1]
            x[0] = 0
            props = dict(S=1, m={0: 1}, cls={0: "uncertain"}, nseg=1)
        elif mode == "sampled":
            sample_rows, sampled = n, r[:0]
            props = dict(S=n, m={0: d}, cls={0: "many" if d > maxb else "exact"}, nseg=0)
        else:
            stride = 8
            sample_rows, sampled = -(-n // stride), r[::stride]
            ev = np.arange(0, d, 2)
            x[sampled] = ev[np.arange(len(sampled)) % len(ev)]           # the sampled rows hold the even values only
            props = dict(S=len(sampled), stride=stride, m={0: len(ev)}, cls={0: "many" if d > maxb else "uncertain"})
        np.subtract.at(left, x[x >= 0].astype(np.int64), 1)
        assert left.min() >= (0 if mode != "interleaved" else 1)          # (every odd value keeps unsampled rows)
        free = r[x < 0]
        nan_row = int(free[-1]) if nan else None
        free = free[:len(free) - nan]
        x[free] = rng.permutation(np.repeat(np.arange(d), left))
        assert np.array_equal(np.bincount(x[x >= 0].astype(np.int64)), counts)
        props.update(nd={0: d}, maxb={0: maxb}, W={0: W})
        X = np.stack([x, -3.0 * x], 1)         # the same thresholds mirrored: the sample value 0 is the maximum
        for key in ("m", "cls", "nd", "maxb", "W"):
            props[key][1] = props[key][0]
        if "nseg" in props:
            props["nseg"] *= 2
        if nan:  # one NaN row, unsampled unless every row is
            assert mode == "sampled" or nan_row % sample_stride(n, sample_rows) != 0
            X[nan_row, :] = np.nan
        props["unit"] = dict(W=props.pop("W"))
        return Built(torch.from_numpy(X.astype(np.float32)), sample_rows=sample_rows, props=props)
    return fn


for _mode in ("unsampled", "sampled", "interleaved"):
    for _d in (255, 256, 257):
        for _nan in (0, 1):
            case(f"C_{_mode}_{_d}" + ("_nan" if _nan else ""))(_c_threshold(_d, _nan, _mode))


@case("C_signed_zero_in_open_bucket")
def _c_signed_zero():
    """256 distinct values when -0.0 and +0.0 count as one (one bin each), 257 when they count as two (the
    quantile path): both zeros sit in the one open bucket above the sample value -1."""
    n = 3001
    rng = np.random.default_rng(41)
    x = np.r_[np.arange(1, 255), rng.integers(1, 255, n - 1 - 254 - 600)].astype(np.float32)
    x = np.r_[x, np.full(300, -0.0, np.float32), np.full(300, 0.0, np.float32)]
    x = np.r_[np.float32(-1.0), rng.permutation(x)].astype(np.float32)
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    return Built(torch.from_numpy(x[:, None]), sample_rows=1,
                 props=dict(S=1, m={0: 1}, cls={0: "uncertain"}, nd={0: 256}, maxb={0: 256}, seg_any={0: n - 1}))


@case("C_every_value_sampled_no_segment")
def _c_no_segment():
    rng = np.random.default_rng(42)
    x = rng.permutation(np.repeat(np.arange(3000), 2)).astype(np.float32) * 0.25 - 100.0
    return Built(torch.from_numpy(np.stack([x, -x], 1)), sample_rows=1 << 20,
                 props=dict(S=6000, m={0: 3000, 1: 3000}, cls={0: "many", 1: "many"}, nseg=0,
                            seg_target={0: 0, 1: 0}))


# ---- D. boundary sort: the sample is every row
D_SIZES = [1, 2, 4094, 4095, 4096, 5000, 32768, 32769]


def _d_distinct(S):
    def fn():
        rng = np.random.default_rng(5000 + S)
        x = (rng.permutation(S).astype(np.float32) - np.float32(S // 2)) * np.float32(0.5)
        return Built(torch.from_numpy(x[:, None]), sample_rows=1 << 20,
                     props=dict(S=S, n=S, nd={0: S}, m={0: min(S, KPOS)}))
    return fn


def _d_dups(S):
    def fn():
        rng = np.random.default_rng(6000 + S)
        x0 = np.round(rng.standard_normal(S) * 3).astype(np.float32)          # heavy duplicates, -0.0 among them
        x1 = (rng.standard_normal(S) * 10).astype(np.float32)
        X = np.stack([x0, x1], 1)
        if S >= 64:
            X[rng.random(S) < 0.1, 0] = np.nan
            X[rng.random(S) < 0.1, 1] = np.nan
            for f in (0, 1):
                X[rng.integers(0, S, 4), f] = np.inf
                X[rng.integers(0, S, 4), f] = -np.inf
            X[5, 0], X[6, 0] = -0.0, 0.0
        else:
            X[0, 0] = -0.0
        return Built(torch.from_numpy(X), sample_rows=1 << 20, props=dict(S=S, n=S))
    return fn


for _S in D_SIZES:
    case(f"D_S{_S}_distinct")(_d_distinct(_S))
    case(f"D_S{_S}_dups_nan_inf")(_d_dups(_S))


# ---- E. values
E_COLUMNS = ("inf", "flt_max", "denormal", "constant", "all_nan", "one_valid", "nan_last_row")


def _e_values(n, seed):
    rng = np.random.default_rng(seed)
    odd = np.arange(1, n, 2)
    c_inf = (rng.standard_normal(n) * 50).astype(np.float32)
    c_inf[rng.choice(odd, 40, replace=False)] = np.inf
    c_inf[rng.choice(odd, 40, replace=False)] = -np.inf
    c_max = (rng.standard_normal(n) * 1e30).astype(np.float32)
    c_max[rng.choice(odd, 30, replace=False)] = FLT_MAX
    c_max[rng.choice(odd, 30, replace=False)] = -FLT_MAX
    c_den = (rng.integers(-2000, 2000, n) * np.float64(1.401298464324817e-45)).astype(np.float32)  # k * 2^-149
    c_den[rng.choice(odd, 50, replace=False)] = -0.0
    c_const = np.full(n, 3.25, np.float32)
    c_nan = np.full(n, np.nan, np.float32)
    c_one = np.full(n, np.nan, np.float32)
    c_one[n // 2 | 1] = -7.5
    c_last = (rng.standard_normal(n) * 5).astype(np.float32)
    c_last[n - 1] = np.nan
    return np.stack([c_inf, c_max, c_den, c_const, c_nan, c_one, c_last], 1)


@case("E_values_every_row_sampled")
def _e_all():
    X = _e_values(5003, 51)
    return Built(torch.from_numpy(X), props=dict(S=5003, nd={3: 1, 4: 0, 5: 1}, maxb={0: 256, 4: 255, 6: 255}))


@case("E_values_sparse_sample")
def _e_sparse():
    # stride 126: the sampled rows are even, the +-inf / +-FLT_MAX / -0.0 rows odd -- none is a boundary
    X = _e_values(5003, 52)
    return Built(torch.from_numpy(X), sample_rows=40, props=dict(stride=126, S=40, nd={3: 1, 4: 0, 5: 1}))


# ---- F. weights
@case("F_zero_weight_on_one_feature")
def _f_zero_feature():
    n = 4000
    rng = np.random.default_rng(61)
    X = (rng.standard_normal((n, 2)) * 10).astype(np.float32)
    X[1::2, 0] = np.nan                                   # feature 0 is valid on the even rows only ...
    w = rng.uniform(0.5, 2.0, n)
    w[0::2] = 0.0                                         # ... and those carry no weight
    return Built(torch.from_numpy(X), w=w, props=dict(weighted=dict(W={0: 0}, cls={0: "many", 1: "many"})))


@case("F_all_weights_zero")
def _f_all_zero():
    X = _continuous(3001, 3, 62)
    return Built(torch.from_numpy(X), w=np.zeros(3001), props=dict(weighted=dict(W={0: 3001, 1: 3001})))


@case("F_one_heavy_row")
def _f_one_heavy():
    n = 9001
    X = _continuous(n, 3, 63)
    w = np.full(n, 1e-9)
    w[4321] = 1.0
    X[4321, 2] = 0.5                                      # (valid in the NaN column too)
    return Built(torch.from_numpy(X), w=w, sample_rows=512,
                 props=dict(weighted=dict(W={0: WEIGHT_SCALE, 1: WEIGHT_SCALE, 2: WEIGHT_SCALE})))


@case("F_equal_weights_70001")
def _f_equal():
    n = 70_001
    return Built(torch.from_numpy(_continuous(n, 3, 64)), w=np.full(n, 0.37),
                 props=dict(nblk=2, n_mod4=1, weighted=dict(W={0: n * WEIGHT_SCALE, 1: n * WEIGHT_SCALE})))


@case("F_low_cardinality_weighted")
def _f_lowcard():
    n = 20_003
    rng = np.random.default_rng(65)
    X = np.stack([rng.integers(0, 12, n).astype(np.float32), (rng.standard_normal(n) * 7).astype(np.float32)], 1)
    return Built(torch.from_numpy(X), w=rng.uniform(0.0, 3.0, n),
                 props=dict(nd={0: 12}, cls={0: "exact", 1: "many"}, m={0: 12}))


# ---- the data-parallel input: 70 001 x 5 with a host-fallback segment of 8193 rows spread over the ranks
DP_ROWS, DP_SEG = 70_001, 8193


@case("DP_70001x5")
def _dp_case():
    n = DP_ROWS
    rng = np.random.default_rng(71)
    X = _continuous(n, 5, 72)
    X[:, 4] = _continuous(n, 1, 73)[:, 0]                 # no NaN from the generator in the last column
    X[:, 2] = rng.integers(0, 30, n)
    X[n - 7, 1] = np.nan                                  # the only NaN of column 1: an unsampled row of the last rank
    stride = sample_stride(n, None)                       # 3
    col = np.zeros(n, np.float32)                         # column 3: every sampled row is 0.0 ...
    free = np.nonzero(np.arange(n) % stride != 0)[0]
    rows = rng.choice(free, DP_SEG, replace=False)        # ... and 8193 unsampled rows hold distinct values above it
    col[rows] = 1.0 + np.arange(DP_SEG, dtype=np.float32)
    X[:, 3] = col
    w = rng.uniform(0.5, 1.5, n)
    w[DP_WORLD3[2][0]:] *= 50.0                            # the last rank of the 3-rank run carries 50x the weight
    return Built(torch.from_numpy(X), w=w,
                 props=dict(stride=3, nblk=2, maxb={1: 255, 3: 256}, m={3: 1}, cls={3: "uncertain"}, nd={3: DP_SEG + 1},
                            seg_target={3: DP_SEG}, seg_any={3: DP_SEG}))


DP_WORLD2 = [(0, 30_001), (30_001, DP_ROWS)]                           # uneven, offsets not multiples of the stride
DP_WORLD3 = [(0, 23_335), (23_335, 23_335), (23_335, DP_ROWS)]         # the middle rank's shard is empty

# case -> sample_rows of the streamed run: 43 691 sample rows (past the LDS sample sort) and 94 (open buckets exist)
STREAM_CASES = {"A_131073x5": 1 << 16, "A_1025x33": 100}
STREAM_CHUNKS = (1, 0, 257, 65537)                                     # then the rest


def stream_bounds(n: int) -> list[int]:
    b = [0]
    for c in STREAM_CHUNKS:
        b.append(min(n, b[-1] + c))
    b.append(n)
    return b


CASE_NAMES = list(CASES)
