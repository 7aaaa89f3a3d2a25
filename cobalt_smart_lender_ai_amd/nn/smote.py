"""SMOTE oversampling (K29) and MinMaxScaler (K30) for the NN challenger.

Reference: ``SMOTE(random_state=123).fit_resample(X_train, y_train)`` then ``MinMaxScaler`` fit on
the resampled rows (notebooks/04_model_training.ipynb cell 38). imblearn is not installed here; this
re-implements its documented algorithm and random-number sequence:

* per minority class: k+1 nearest neighbours of every class row among the class rows, first
  column (the row itself) dropped;
* ``rs = RandomState(random_state)``; ``idx = rs.randint(0, n_class*k, n_new)``;
  ``steps = rs.uniform(size=n_new)``; ``rows, cols = divmod(idx, k)``;
  ``new = X[rows] + steps * (X[nn[rows, cols]] - X[rows])``;
* output = original rows followed by the synthetic rows of each class, in class order.

The neighbour search runs on the GPU (``csrc/knn.hip``: fp32 MFMA distance tiles + register
top-k), on CPU with scikit-learn's NearestNeighbors. Parity with imblearn itself is unpinned (not
importable); the algorithm is tested against a scikit-learn oracle.
"""
from __future__ import annotations

import ctypes
import json

import numpy as np
import torch

from .. import _native

_native.register("cobalt_knn", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
_native.register("cobalt_smote_interp", ctypes.c_int,
                 [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p])
_KNN_K = (1, 2, 3, 4, 5, 6, 7, 8, 11, 16)


def _device(device) -> torch.device:
    if device is not None:
        return torch.device(device)
    return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")


def kneighbors(Q: np.ndarray, R: np.ndarray, k: int, device=None) -> tuple[np.ndarray, np.ndarray]:
    """Indices [nq, k] and Euclidean distances of the k nearest rows of R for every row of Q,
    ordered by (distance, index).

    Q and R are taken as float64. Raises ``ValueError`` (on every device, before any device work)
    when ``k > len(R)`` or when Q or R holds a NaN or an infinity: scikit-learn raises for both, and
    the kernel would hand out its "empty slot" index 2^31-1 for them.

    ``device="cuda"`` (``csrc/knn.hip``) forms d^2 = |r|^2 + |q|^2 - 2 r.q in fp32, which cancels
    badly away from the origin, so the float64 column mean mu of R is subtracted from Q and R before
    the cast to fp32 (distances are translation-invariant). Accuracy contract of the cuda path, with
    u = 2^-24: every squared distance it compares or returns is within

        tau(q, r) = (2 F + 8) u (|q - mu|^2 + |r - mu|^2)

    of the exact one, so a neighbour is certain to be found when it beats the (k+1)-th nearest by
    more than 2 max_r tau(q, r), and rows closer together than that may come out in either order
    (tests/knn_cases.py derives and checks this). Known limit: tau is relative to the spread of R
    about its mean, so tight clusters far apart (two clusters at +-1000 with spacing 0.01) stay
    unresolved -- use ``device="cpu"`` for such data. Centred coordinates too large for fp32 squared
    distances (4 F max|x - mu|^2 >= FLT_MAX) raise ``ValueError`` too."""
    dev = _device(device)
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    R = np.ascontiguousarray(R, dtype=np.float64)
    if Q.ndim != 2 or R.ndim != 2 or Q.shape[1] != R.shape[1]:
        raise ValueError(f"Q {Q.shape} and R {R.shape} must be 2-D with the same number of columns")
    nq, nr, F = Q.shape[0], R.shape[0], R.shape[1]
    if k < 1 or k > nr:
        raise ValueError(f"k={k} neighbours asked of {nr} reference rows (need 1 <= k <= rows of R)")
    if not (np.isfinite(Q).all() and np.isfinite(R).all()):
        raise ValueError("kneighbors: Q and R must be finite (found NaN or infinity)")
    if dev.type == "cuda":
        if k not in _KNN_K:
            raise ValueError(f"k must be one of {_KNN_K}")
        mu = R.mean(axis=0)
        Qc, Rc = Q - mu, R - mu
        big = max(float(np.abs(Qc).max(initial=0.0)), float(np.abs(Rc).max()))
        if 4.0 * F * big * big >= float(np.finfo(np.float32).max):
            raise ValueError(f"kneighbors: |x - mean| up to {big:.3g} overflows fp32 squared distances; use device='cpu'")
        if nq == 0:
            return np.empty((0, k), dtype=np.int64), np.empty((0, k), dtype=np.float32)
        Qd = torch.as_tensor(Qc.astype(np.float32), device=dev)
        Rd = torch.as_tensor(Rc.astype(np.float32), device=dev)
        idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
        dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
        rc = _native.lib().cobalt_knn(Qd.data_ptr(), nq, Rd.data_ptr(), nr, F, k,
                                      idx.data_ptr(), dist.data_ptr(), _native.stream_handle())
        _native.check(rc, "cobalt_knn")
        return idx.cpu().numpy().astype(np.int64), np.sqrt(dist.cpu().numpy())
    from sklearn.neighbors import NearestNeighbors

    nn = NearestNeighbors(n_neighbors=k).fit(R)
    d, i = nn.kneighbors(Q)
    return i, d


class SMOTE:
    def __init__(self, sampling_strategy="auto", random_state=None, k_neighbors: int = 5, device=None):
        if sampling_strategy != "auto":
            raise NotImplementedError("only sampling_strategy='auto' (the reference's setting)")
        self.random_state = random_state
        self.k_neighbors = k_neighbors
        self.device = device

    def fit_resample(self, X, y):
        cols = getattr(X, "columns", None)
        Xn = np.asarray(X.to_numpy() if hasattr(X, "to_numpy") else X, dtype=np.float64)
        yn = np.asarray(y.to_numpy() if hasattr(y, "to_numpy") else y)
        classes, counts = np.unique(yn, return_counts=True)
        n_max = counts.max()
        outs_X, outs_y = [Xn], [yn]
        self.sampling_strategy_ = {c: int(n_max - n) for c, n in zip(classes, counts) if n < n_max}
        for cls, n_new in self.sampling_strategy_.items():
            if n_new == 0:
                continue
            Xc = Xn[yn == cls]
            k = self.k_neighbors
            if len(Xc) <= k:
                raise ValueError(f"SMOTE: class {cls} has {len(Xc)} rows, but k_neighbors={k} needs at least "
                                 f"{k + 1} (every row needs k neighbours besides itself)")
            nn, _ = kneighbors(Xc, Xc, k + 1, self.device)
            nn = nn[:, 1:]
            rs = np.random.RandomState(self.random_state) if not isinstance(self.random_state, np.random.RandomState) \
                else self.random_state
            idx = rs.randint(low=0, high=nn.size, size=n_new)
            steps = rs.uniform(size=n_new)
            rows = np.floor_divide(idx, nn.shape[1])
            cidx = np.mod(idx, nn.shape[1])
            outs_X.append(self._interp(Xc, nn, rows, cidx, steps))
            outs_y.append(np.full(n_new, cls, dtype=yn.dtype))
        Xr = np.vstack(outs_X)
        yr = np.hstack(outs_y)
        if cols is not None:
            import pandas as pd

            Xr = pd.DataFrame(Xr, columns=cols)
            yr = pd.Series(yr, name=getattr(y, "name", None))
        return Xr, yr

    def _interp(self, Xc, nn, rows, cols, steps) -> np.ndarray:
        dev = _device(self.device)
        if dev.type == "cuda":
            F = Xc.shape[1]
            Xd = torch.as_tensor(np.ascontiguousarray(Xc), device=dev)
            nnd = torch.as_tensor(nn.astype(np.int32), device=dev).contiguous()
            rd = torch.as_tensor(rows.astype(np.int64), device=dev)
            cd = torch.as_tensor(cols.astype(np.int64), device=dev)
            sd = torch.as_tensor(steps.astype(np.float64), device=dev)
            out = torch.empty((len(rows), F), dtype=torch.float64, device=dev)
            rc = _native.lib().cobalt_smote_interp(Xd.data_ptr(), F, nnd.data_ptr(), nn.shape[1], rd.data_ptr(),
                                                   cd.data_ptr(), sd.data_ptr(), len(rows), out.data_ptr(),
                                                   _native.stream_handle())
            _native.check(rc, "cobalt_smote_interp")
            return out.cpu().numpy()
        return Xc[rows] + steps[:, None] * (Xc[nn[rows, cols]] - Xc[rows])


class MinMaxScaler:
    """Column min/max scaling to [0, 1] (sklearn semantics: constant columns map to 0; NaN ignored
    in the fit and passed through)."""

    def fit(self, X):
        Xn = np.asarray(X.to_numpy() if hasattr(X, "to_numpy") else X, dtype=np.float64)
        self.data_min_ = np.nanmin(Xn, axis=0)
        self.data_max_ = np.nanmax(Xn, axis=0)
        rng = self.data_max_ - self.data_min_
        rng[rng == 0.0] = 1.0
        self.scale_ = 1.0 / rng
        self.min_ = -self.data_min_ * self.scale_
        self.n_features_in_ = Xn.shape[1]
        if hasattr(X, "columns"):
            self.feature_names_in_ = np.asarray(X.columns, dtype=object)
        return self

    def transform(self, X):
        Xn = np.asarray(X.to_numpy() if hasattr(X, "to_numpy") else X, dtype=np.float64)
        return Xn * self.scale_ + self.min_

    def fit_transform(self, X):
        return self.fit(X).transform(X)

    def inverse_transform(self, X):
        return (np.asarray(X, dtype=np.float64) - self.min_) / self.scale_

    def to_json(self) -> str:
        return json.dumps({k: getattr(self, k).tolist() for k in ("data_min_", "data_max_", "scale_", "min_")}
                          | {"feature_names_in_": list(getattr(self, "feature_names_in_", []))})

    @classmethod
    def from_json(cls, s: str) -> "MinMaxScaler":
        d = json.loads(s)
        m = cls()
        for k in ("data_min_", "data_max_", "scale_", "min_"):
            setattr(m, k, np.asarray(d[k], dtype=np.float64))
        if d.get("feature_names_in_"):
            m.feature_names_in_ = np.asarray(d["feature_names_in_"], dtype=object)
        m.n_features_in_ = len(m.scale_)
        return m
