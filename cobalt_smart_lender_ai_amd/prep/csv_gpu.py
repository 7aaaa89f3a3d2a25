"""GPU CSV ingest for :class:`~.device_frame.DeviceFrame` (the "GPU tokenizer").

The reference reads its raw LendingClub export with ``pandas.read_csv``
(src/data_preprocessing/clean_data.py:44-67); the device prep path used pyarrow's multithreaded C++
reader on the host, which was ~95% of the full-data prep wall time. Here the file's bytes go to HBM
once and ``csrc/csv.hip`` does the rest: quote-parity / delimiter prefix sums find every field, one
pass parses every field to a status byte + float64, string columns are hashed and dictionary-encoded
on the device (codes verified byte-for-byte against each code's first row).

Column typing follows the pyarrow reader it replaces (and pandas' defaults): pandas' missing-value
strings are null; a column whose non-null values all parse as numbers is numeric (``int64`` when every
value has integer syntax and none is missing, else ``float64``); ``True``/``False`` literals make a bool
column; anything else is a string column. Unlike pyarrow, ISO date strings stay strings (as in pandas).
Numbers are converted exactly (see csv.hip); the rare value outside the exact fast path is re-parsed on
the host. Like those readers, the device reads "inf" / "infinity" in any letter case, strips blanks
(space, tab) around a number, and reads integer syntax past the int64 range as a float.

The device may defer, never differ: :class:`CsvLayoutError` is raised, and the caller falls back to
pyarrow, for a file the tokenizer cannot lay out as a rectangle (ragged rows, blank lines -- in a
one-column file too, where pyarrow skips an empty line), for malformed quoting (a quote inside an unquoted
field, ``"x"y``), for a hex literal (``0x10``) or a ``nan`` spelling outside pandas' list (``NAN``, ``+nan``)
in a column that holds no other text (pyarrow reads those as numbers), and for an integer column with a
value past 2^53, which the frame's float64 cannot hold (pyarrow's own upload refuses it too).
"""
from __future__ import annotations

import ctypes
import csv as _csv
import gzip
import io
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _native

ST_INT, ST_NULL, ST_TRUE, ST_FALSE, ST_STR, ST_HOST, ST_FRAC, ST_BIGINT, ST_HOSTNUM, ST_NEGZERO = range(10)

_P, _I64, _I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
_native.register("cobalt_csv_chunk", ctypes.c_int, [])
_native.register("cobalt_csv_quotes", ctypes.c_int, [_P, _I64, _P, _P])
_native.register("cobalt_csv_delims", ctypes.c_int, [_P, _I64, _P, _P, _P])
_native.register("cobalt_csv_fields", ctypes.c_int, [_P, _I64, _P, _P, _I32, _P, _P, _P])
_native.register("cobalt_csv_parse", ctypes.c_int, [_P, _P, _I64, _I32, _P, _P, _I32, _P])
_native.register("cobalt_csv_hash", ctypes.c_int, [_P, _P, _I64, _I32, _P, _I32, _P, _P, _P])
_native.register("cobalt_csv_verify", ctypes.c_int, [_P, _P, _I64, _I32, _P, _I32, _P, _P, _P])
_native.register("cobalt_csv_span", ctypes.c_int, [_P, _P, _I64, _I32, _P, _P, _P, _P, _P])
_native.register("cobalt_csv_gather", ctypes.c_int, [_P, _P, _I64, _I32, _P, _P, _P, _P, _P])


class CsvLayoutError(ValueError):
    """The file is not a rectangular RFC 4180 table (the caller falls back to pyarrow)."""


def read_file_pinned(path: str, threads: int = 8) -> torch.Tensor:
    """The whole file in page-locked host memory, read by ``threads`` parallel ``preadv`` calls."""
    size = os.path.getsize(path)
    host = torch.empty(size, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    view = host.numpy()
    if size == 0:
        return host
    step = max(1 << 24, -(-size // threads))
    fd = os.open(path, os.O_RDONLY)
    try:
        def part(o: int) -> None:
            end = min(size, o + step)
            while o < end:
                got = os.preadv(fd, [memoryview(view[o:end])], o)
                if got <= 0:
                    raise OSError(f"short read of {path} at {o}")
                o += got
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(part, range(0, size, step)))
    finally:
        os.close(fd)
    return host


def _host_bytes(src) -> torch.Tensor:
    if isinstance(src, (bytes, bytearray, memoryview)):
        b = bytes(src)
        if b[:2] == b"\x1f\x8b":
            b = gzip.decompress(b)
        return torch.frombuffer(bytearray(b), dtype=torch.uint8) if b else torch.empty(0, dtype=torch.uint8)
    path = str(src)
    if path.endswith((".gz", ".gzip")):
        with gzip.open(path, "rb") as f:
            b = f.read()
        return torch.frombuffer(bytearray(b), dtype=torch.uint8) if b else torch.empty(0, dtype=torch.uint8)
    return read_file_pinned(path)


def dedup_names(names: list[str]) -> list[str]:
    """pandas.read_csv's (C parser) renaming of repeated header names: the second ``a`` becomes
    ``a.1``, the third ``a.2``, skipping suffixed names the header already holds."""
    out = list(names)
    counts: dict[str, int] = {}
    for i, col in enumerate(out):
        old = col
        cur = counts.get(col, 0)
        while cur > 0:
            counts[old] = cur + 1
            col = f"{old}.{cur}"
            cur = cur + 1 if col in out else counts.get(col, 0)
        out[i] = col
        counts[col] = cur + 1
    return out


def _header(host: np.ndarray) -> tuple[list[str], int]:
    """Column names and the byte offset of the first data row (the header may be quoted)."""
    inq = False
    i = 0
    n = len(host)
    lim = min(n, 1 << 24)
    head = host[:lim].tobytes()
    while i < lim:
        c = head[i]
        if c == 0x22:
            inq = not inq
        elif c == 0x0A and not inq:
            break
        i += 1
    line = head[:i].decode("utf-8").rstrip("\r")
    names = next(_csv.reader(io.StringIO(line))) if line else []
    return dedup_names(names), min(i + 1, n)


def _chk(rc: int, name: str) -> None:
    _native.check(rc, name)


def _strings_array(host_data: np.ndarray, off: np.ndarray, quoted: np.ndarray, valid: np.ndarray):
    """pyarrow large_string array from concatenated UTF-8 bytes (``""`` escapes of quoted fields undone)."""
    import pyarrow as pa

    n = len(valid)
    vbits = np.packbits(valid.astype(np.uint8), bitorder="little")
    arr = pa.Array.from_buffers(pa.large_string(), n, [pa.py_buffer(vbits), pa.py_buffer(off.astype(np.int64)),
                                                        pa.py_buffer(host_data)], null_count=int(n - valid.sum()))
    fix = np.nonzero(quoted & valid)[0]
    if len(fix):
        vals = arr.to_pylist()
        changed = False
        for r in fix:
            v = vals[r]
            if '""' in v:
                vals[r] = v.replace('""', '"')
                changed = True
        if changed:
            arr = pa.array(vals, type=pa.large_string())
    return arr


def read_csv_gpu(src, device, hash_unique_share: float = 0.2, timings: dict | None = None,
                 float_precision: str = "round_trip"):
    """Parse a CSV (path, bytes, optionally gzip) on the GPU into a DeviceFrame (see module doc).

    ``float_precision``: ``"round_trip"`` (correctly rounded, = pandas ``float_precision="round_trip"``)
    or ``"high"`` (= pandas' DEFAULT conversion, which is up to ~1 ulp off on 17-digit inputs; the
    device reproduces its arithmetic, csrc/csv.hip pandas_xstrtod)."""
    from .device_frame import DCol, DeviceFrame

    if float_precision not in ("round_trip", "high"):
        raise ValueError(f"float_precision must be 'round_trip' or 'high', got {float_precision!r}")
    pandas_fp = float_precision == "high"
    dev = torch.device(device)
    if dev.type != "cuda":
        raise CsvLayoutError("the GPU CSV reader needs a GPU device")
    lib = _native.lib()
    stream = _native.stream_handle()
    t0 = time.perf_counter()
    host = _host_bytes(src)
    t_read = time.perf_counter()
    hnp = host.numpy()
    names, start = _header(hnp)
    C = len(names)
    if C == 0 or start >= len(hnp):
        raise CsvLayoutError("no data rows")
    buf = host[start:].to(dev, non_blocking=True)
    n = buf.numel()
    chunk = lib.cobalt_csv_chunk()
    nch = -(-n // chunk)
    qc = torch.empty(nch, dtype=torch.int64, device=dev)
    _chk(lib.cobalt_csv_quotes(buf.data_ptr(), n, qc.data_ptr(), stream), "cobalt_csv_quotes")
    qp = torch.cumsum(qc, 0) - qc
    dc = torch.empty(nch, dtype=torch.int64, device=dev)
    _chk(lib.cobalt_csv_delims(buf.data_ptr(), n, qp.data_ptr(), dc.data_ptr(), stream), "cobalt_csv_delims")
    dp = torch.cumsum(dc, 0)
    D = int(dp[-1])
    dp = dp - dc
    last_nl = bool(hnp[-1] == 0x0A)
    nf = D if last_nl else D + 1
    if nf % C != 0:
        raise CsvLayoutError(f"{nf} fields is not a multiple of {C} columns")
    N = nf // C
    fend = torch.empty(max(nf, 1), dtype=torch.int64, device=dev)
    if not last_nl:
        fend[D] = n
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    _chk(lib.cobalt_csv_fields(buf.data_ptr(), n, qp.data_ptr(), dp.data_ptr(), C, fend.data_ptr(), bad.data_ptr(),
                               stream), "cobalt_csv_fields")
    if int(bad) != 0:
        raise CsvLayoutError(f"{int(bad)} rows with a field count other than {C}")
    if C == 1:  # every newline is a legal row end here, but the host readers skip an empty line
        fs = torch.cat([fend.new_zeros(1), fend[:nf - 1] + 1])
        ln = fend[:nf] - fs
        if bool(((ln == 0) | ((ln == 1) & (buf[fs.clamp(max=n - 1)] == 0x0D))).any()):
            raise CsvLayoutError("blank line in a one-column file")
    t_tok = time.perf_counter()
    status = torch.empty((C, N), dtype=torch.uint8, device=dev)
    vals = torch.empty((C, N), dtype=torch.float64, device=dev)
    _chk(lib.cobalt_csv_parse(buf.data_ptr(), fend.data_ptr(), N, C, status.data_ptr(), vals.data_ptr(),
                              int(pandas_fp), stream), "cobalt_csv_parse")
    counts = torch.bincount((torch.arange(C, device=dev)[:, None] * 16 + status.long()).reshape(-1),
                            minlength=C * 16).reshape(C, 16).cpu().numpy()
    t_parse = time.perf_counter()

    def host_reparse(c: int) -> None:
        rows = torch.nonzero(status[c] == ST_HOST).reshape(-1)
        txt = _texts(lib, stream, buf, fend, C, torch.full_like(rows, c, dtype=torch.int32), rows, None, dev)
        if pandas_fp:  # the few fields the device left: pandas itself (it types overflows as text)
            import pandas as pd

            col = pd.read_csv(io.StringIO("x\n" + "\n".join(txt) + "\n"), dtype=None)["x"]
            if col.dtype != np.float64:
                raise CsvLayoutError(f"column {names[c]!r} holds values pandas reads as text")
            vals[c][rows] = torch.from_numpy(col.to_numpy()).to(dev)
            return
        vals[c][rows] = torch.tensor([float(t) for t in txt], dtype=torch.float64, device=dev)

    kinds: dict[int, str] = {}
    str_cols = []
    for c in range(C):
        cnt = counts[c]
        n_null, n_bool = cnt[ST_NULL], cnt[ST_TRUE] + cnt[ST_FALSE]
        n_num = cnt[ST_INT] + cnt[ST_FRAC] + cnt[ST_HOST] + cnt[ST_BIGINT] + cnt[ST_NEGZERO]
        if cnt[ST_HOSTNUM] and cnt[ST_STR] == 0 and n_bool == 0:  # with other text it is text to pyarrow too
            raise CsvLayoutError(f"column {names[c]!r} holds hex or nan spellings only the host reader takes")
        if cnt[ST_BIGINT] and cnt[ST_FRAC] == 0 and cnt[ST_HOST] == 0 and cnt[ST_STR] == 0 and n_bool == 0:
            raise CsvLayoutError(f"integer column {names[c]!r} holds values past 2^53")
        if n_null == N:
            kinds[c] = "null"
        elif cnt[ST_STR] + cnt[ST_HOSTNUM] == 0 and n_bool == 0:
            kinds[c] = "num"
        elif cnt[ST_STR] + cnt[ST_HOSTNUM] == 0 and n_num == 0:
            kinds[c] = "bool"
        else:
            kinds[c] = "str"
            str_cols.append(c)
    scols = _string_columns(lib, stream, buf, fend, N, C, str_cols, dev, hash_unique_share) if str_cols else {}
    cols: dict[str, DCol] = {}
    for c, name in enumerate(names):
        k = kinds[c]
        cnt = counts[c]
        if k == "null":
            cols[name] = DCol("f", torch.full((N,), float("nan"), dtype=torch.float64, device=dev), "float64")
        elif k == "num":  # a row of the parsed block (no copy)
            if cnt[ST_HOST]:
                host_reparse(c)
            is_int = cnt[ST_FRAC] == 0 and cnt[ST_NULL] == 0 and cnt[ST_HOST] == 0
            # "-0" is +0.0 where the host reader types the column int64, -0.0 where it parses floats
            if cnt[ST_NEGZERO] and (cnt[ST_FRAC] or cnt[ST_HOST] or (pandas_fp and not is_int)):
                vals[c][status[c] == ST_NEGZERO] = -0.0
            cols[name] = DCol("f", vals[c], "int64" if is_int else "float64")
        elif k == "bool":
            st = status[c]
            if cnt[ST_NULL] == 0:
                cols[name] = DCol("b", (st == ST_TRUE).to(torch.uint8), "bool")
            else:
                v = torch.where(st == ST_TRUE, 1.0, torch.where(st == ST_FALSE, 0.0, float("nan"))).to(torch.float64)
                cols[name] = DCol("f", v, "boolnull")  # 1 / 0 / NaN; exported as pandas' object bools
        else:
            cols[name] = scols[c]
    if timings is not None:
        torch.cuda.synchronize(dev)
        t_end = time.perf_counter()
        timings.update({"read": t_read - t0, "tokenize": t_tok - t_read, "parse": t_parse - t_tok,
                        "columns": t_end - t_parse, "rows": N, "cols": C, "bytes": n})
    return DeviceFrame(cols, N, dev)


class DeviceStrings:
    """Text of a near-unique string column kept in HBM (content bytes + offsets + masks); copied to the
    host as a pyarrow large_string array only when first decoded (:meth:`arrow`, cached)."""

    def __init__(self, data: torch.Tensor, off: torch.Tensor, valid: torch.Tensor, quoted: torch.Tensor):
        self.data, self.off, self.valid, self.quoted = data, off, valid, quoted
        self._arr = None

    def __len__(self) -> int:
        return self.valid.numel()

    def arrow(self):
        if self._arr is None:
            self._arr = _strings_array(self.data.cpu().numpy(), self.off.cpu().numpy(),
                                       self.quoted.cpu().numpy().astype(bool), self.valid.cpu().numpy())
        return self._arr

    def take(self, rows):
        """pyarrow array of the given rows' text; only those rows' bytes leave the device."""
        if self._arr is not None:
            import pyarrow.compute as pc

            return pc.take(self._arr, np.asarray(rows.cpu() if torch.is_tensor(rows) else rows))
        dev = self.data.device
        r = torch.as_tensor(rows, device=dev, dtype=torch.int64)
        lens = torch.where(self.valid[r], self.off[r + 1] - self.off[r], 0)
        noff = torch.zeros(r.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=noff[1:])
        total = int(noff[-1])
        if total:
            idx = torch.repeat_interleave(self.off[r] - noff[:-1], lens, output_size=total) + torch.arange(total, device=dev)
            data = self.data[idx].cpu().numpy()
        else:
            data = np.zeros(0, np.uint8)
        return _strings_array(data, noff.cpu().numpy(), self.quoted[r].cpu().numpy(), self.valid[r].cpu().numpy())


def _texts(lib, stream, buf, fend, C, pcol: torch.Tensor, prow: torch.Tensor, valid: torch.Tensor | None, dev,
           as_device: bool = False):
    """Text of m (col, row) fields: a list of str, or (as_device) a :class:`DeviceStrings` whose entries
    with ``valid == False`` are null."""
    m = prow.numel()
    pcol = pcol.to(torch.int32).contiguous()
    prow = prow.to(torch.int64).contiguous()
    lens = torch.empty(m, dtype=torch.int64, device=dev)
    quoted = torch.empty(m, dtype=torch.uint8, device=dev)
    _chk(lib.cobalt_csv_span(buf.data_ptr(), fend.data_ptr(), m, C, pcol.data_ptr(), prow.data_ptr(), lens.data_ptr(),
                             quoted.data_ptr(), stream), "cobalt_csv_span")
    if valid is not None:
        lens = torch.where(valid, lens, torch.zeros_like(lens))
    off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=off[1:])
    total = int(off[-1])
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    _chk(lib.cobalt_csv_gather(buf.data_ptr(), fend.data_ptr(), m, C, pcol.data_ptr(), prow.data_ptr(), off.data_ptr(),
                               out.data_ptr(), stream), "cobalt_csv_gather")
    if as_device:
        v = valid if valid is not None else torch.ones(m, dtype=torch.bool, device=dev)
        return DeviceStrings(out[:total], off, v, quoted.bool())
    data, offh, qh = out[:total].cpu().numpy(), off.cpu().numpy(), quoted.cpu().numpy().astype(bool)
    res = []
    for i in range(m):
        t = data[offh[i]:offh[i + 1]].tobytes().decode("utf-8")
        res.append(t.replace('""', '"') if qh[i] else t)
    return res


def _string_columns(lib, stream, buf, fend, N, C, str_cols: list[int], dev, share: float) -> dict:
    """DCols of all string columns at once: device hashes, then per column either dictionary codes
    (first-occurrence order, as pyarrow's dictionary_encode; verified byte-for-byte) or, for a
    near-unique column, the hash with the text kept in HBM (:class:`DeviceStrings`, decoded lazily)."""
    from .device_frame import DCol

    S = len(str_cols)
    cols_t = torch.tensor(str_cols, dtype=torch.int32, device=dev)
    H = torch.empty((S, N), dtype=torch.int64, device=dev)
    badq = torch.zeros(1, dtype=torch.int64, device=dev)
    _chk(lib.cobalt_csv_hash(buf.data_ptr(), fend.data_ptr(), N, C, cols_t.data_ptr(), S, H.data_ptr(),
                             badq.data_ptr(), stream), "cobalt_csv_hash")
    valid = H != 0
    nh = min(N, 20_000)
    hs = torch.sort(H[:, :nh], dim=1).values
    distinct = (hs[:, 0] != 0).long() + ((hs[:, 1:] != hs[:, :-1]) & (hs[:, 1:] != 0)).sum(1)
    near = ((distinct > share * nh) & (N >= 1000)).cpu().tolist()
    if int(badq):
        raise CsvLayoutError(f"{int(badq)} fields with malformed quoting")
    out = {}
    dj = [j for j in range(S) if not near[j]]
    if dj:
        dj_t = torch.tensor(dj, device=dev)
        Hd, vd = H[dj_t], valid[dj_t]
        srt, perm = torch.sort(Hd, dim=1, stable=True)
        newseg = torch.ones_like(srt, dtype=torch.bool)
        newseg[:, 1:] = srt[:, 1:] != srt[:, :-1]
        pos = torch.arange(N, device=dev).expand_as(srt)
        start = torch.cummax(torch.where(newseg, pos, torch.zeros_like(pos)), dim=1).values
        first = torch.empty_like(perm)
        first.scatter_(1, perm, perm.gather(1, start))  # first row holding each row's value
        isfirst = (first == torch.arange(N, device=dev)) & vd
        codes = torch.where(vd, torch.cumsum(isfirst, 1).gather(1, first) - 1, -1).to(torch.int32)
        rep = torch.where(vd, first, -1).contiguous()
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        cd = cols_t[dj_t].contiguous()
        _chk(lib.cobalt_csv_verify(buf.data_ptr(), fend.data_ptr(), N, C, cd.data_ptr(), len(dj), rep.data_ptr(),
                                   bad.data_ptr(), stream), "cobalt_csv_verify")
        if int(bad):
            raise CsvLayoutError("string hash collision")
        pj, prow = torch.nonzero(isfirst, as_tuple=True)  # (column, row) in row order per column
        nvoc = isfirst.sum(1).cpu().tolist()
        texts = _texts(lib, stream, buf, fend, C, cd[pj], prow, None, dev) if prow.numel() else []
        o = 0
        for k, j in enumerate(dj):
            out[str_cols[j]] = DCol("c", codes[k], "object", texts[o:o + nvoc[k]])
            o += nvoc[k]
    for j in range(S):
        if near[j]:
            c = str_cols[j]
            rows = torch.arange(N, device=dev)
            txt = _texts(lib, stream, buf, fend, C, torch.full((N,), c, dtype=torch.int32, device=dev), rows, valid[j],
                         dev, as_device=True)
            out[c] = DCol("h", H[j], "object", src=txt)
    return out


# ------------------------------------------------------------------------------------------ writer
_native.register("cobalt_csv_wcol_size", ctypes.c_int, [])
_native.register("cobalt_csv_write_len", ctypes.c_int, [_P, _I32, _I64, _P, _P, _P, _P])
_native.register("cobalt_csv_write_bytes", ctypes.c_int, [_P, _I32, _I64, _P, _P, _P, _P, _P, _P])

W_FLOAT, W_INT, W_BOOL, W_BOOLINT, W_VOCAB, W_TEXT = range(6)


class _WCol(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("pad", ctypes.c_int32), ("data", ctypes.c_void_p), ("off", ctypes.c_void_p),
                ("text", ctypes.c_void_p), ("valid", ctypes.c_void_p), ("quoted", ctypes.c_void_p),
                ("rowid", ctypes.c_void_p), ("pad2", ctypes.c_int64)]


assert ctypes.sizeof(_WCol) == 64


def csv_escape(s: str) -> str:
    """The csv module's QUOTE_MINIMAL (pandas.to_csv's default) for one field."""
    if any(ch in s for ch in ',"\n\r'):
        return '"' + s.replace('"', '""') + '"'
    return s


def _text_buffers(src, dev):
    """(bytes, int64 offsets, uint8 valid, uint8 quoted | None) on the device for a string column source."""
    if hasattr(src, "arrow"):  # DeviceStrings
        return src.data, src.off, src.valid.to(torch.uint8), src.quoted.to(torch.uint8)
    import pyarrow as pa

    arr = src.combine_chunks() if hasattr(src, "combine_chunks") else src
    arr = arr.cast(pa.large_string())
    valid = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), dtype=np.uint8)
    bufs = arr.buffers()
    off = np.frombuffer(bufs[1], dtype=np.int64, count=len(arr) + 1, offset=arr.offset * 8).copy()
    data = np.frombuffer(bufs[2], dtype=np.uint8) if bufs[2] is not None else np.zeros(0, np.uint8)
    data = data[off[0]:off[-1]].copy() if len(data) else np.zeros(1, np.uint8)
    off -= off[0]
    return (torch.from_numpy(data).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(valid).to(dev), None)


def frame_to_csv_bytes(frame, timings: dict | None = None) -> memoryview | bytes | None:
    """``frame.to_pandas().to_csv(index=False)`` as UTF-8 bytes, formatted on the GPU (``csrc/csv.hip``
    writer), as a bytes-like buffer. The rare float the device cannot certify (subnormal, beyond
    1e290, a decimal tie within the double-double error bound) is formatted by Python's repr and spliced
    in. None off the GPU. Cumulative phase times go to ``timings`` when given."""
    dev = frame.device
    if dev.type != "cuda":
        return None
    lib = _native.lib()
    stream = _native.stream_handle()
    t0 = time.perf_counter()
    names = frame.columns
    C, N = len(names), frame.n
    header = (",".join(csv_escape(str(n)) for n in names) + "\n").encode("utf-8")
    if C == 0:
        return header
    descs = (_WCol * C)()
    keep = []
    fdata: dict[int, torch.Tensor] = {}
    for j, name in enumerate(names):
        c = frame[name]
        d = descs[j]
        if c.kind == "f" and c.dtype == "boolnull":  # pandas writes object bools: True / False / empty
            from .device_frame import DCol

            c = DCol("c", torch.where(torch.isnan(c.data), -1.0, c.data).to(torch.int32), "object", [False, True])
        if c.kind == "f":
            v = c.data.to(torch.float64).contiguous()
            keep.append(v)
            fdata[j] = v
            d.data = v.data_ptr()
            d.kind = W_INT if (c.dtype == "int64" and not bool(torch.isnan(v).any())) else W_FLOAT
        elif c.kind == "b":
            v = c.data.to(torch.uint8).contiguous()
            keep.append(v)
            d.data = v.data_ptr()
            d.kind = W_BOOL if c.dtype == "bool" else W_BOOLINT
        elif c.kind == "c":
            codes = c.data.to(torch.int32).contiguous()
            txt = [csv_escape(str(x)).encode("utf-8") for x in c.vocab]
            offs = np.zeros(len(txt) + 1, dtype=np.int64)
            np.cumsum([len(t) for t in txt], out=offs[1:])
            vt = torch.from_numpy(np.frombuffer(b"".join(txt) or b"\0", dtype=np.uint8).copy()).to(dev)
            vo = torch.from_numpy(offs).to(dev)
            keep += [codes, vt, vo]
            d.kind, d.data, d.off, d.text = W_VOCAB, codes.data_ptr(), vo.data_ptr(), vt.data_ptr()
        else:  # "h": text of the ingest rows, indexed through rowid
            data, off, valid, quoted = _text_buffers(c.src, dev)
            rid = frame.rowid.to(torch.int64).contiguous()
            keep += [data, off, valid, rid] + ([quoted] if quoted is not None else [])
            d.kind, d.off, d.text, d.valid = W_TEXT, off.data_ptr(), data.data_ptr(), valid.data_ptr()
            d.quoted = quoted.data_ptr() if quoted is not None else None
            d.rowid = rid.data_ptr()
    dbuf = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    tm = {"columns": time.perf_counter() - t0}
    lens = torch.empty((C, N), dtype=torch.int32, device=dev)
    dig = torch.empty((C, N), dtype=torch.int64, device=dev)     # float digits, cached between the passes
    dpk = torch.full((C, N), -2, dtype=torch.int32, device=dev)  # p | (k + 512) << 8; -1 = host text
    _chk(lib.cobalt_csv_write_len(dbuf.data_ptr(), C, N, lens.data_ptr(), dig.data_ptr(), dpk.data_ptr(), stream),
         "cobalt_csv_write_len")
    host_fix = None
    if N and bool((lens < 0).any()):  # host-formatted fields: their text lengths go into the layout
        ci, ri = torch.nonzero(lens < 0, as_tuple=True)
        ch = ci.cpu().numpy()
        texts = []
        for cc in np.unique(ch):
            sel = ch == cc
            v = fdata[int(cc)][ri[torch.as_tensor(sel, device=dev)]].cpu().numpy()
            if descs[int(cc)].kind == W_INT:
                texts += [str(x) for x in v.astype(np.int64)]
            else:
                texts += ["" if np.isnan(x) else repr(float(x)) for x in v]
        order = np.concatenate([np.nonzero(ch == cc)[0] for cc in np.unique(ch)])
        tb = [t.encode("utf-8") for t in texts]
        L = torch.tensor([len(t) for t in tb], dtype=torch.int32, device=dev)
        ci_o, ri_o = ci[torch.as_tensor(order, device=dev)], ri[torch.as_tensor(order, device=dev)]
        lens[ci_o, ri_o] = L
        host_fix = (ci_o, ri_o, L, b"".join(tb))
    torch.cuda.synchronize(dev)
    tm["lengths"] = time.perf_counter() - t0
    pos = torch.cumsum(lens + 1, dim=0, dtype=torch.int64)  # inclusive over columns (field + separator)
    row_len = pos[-1].clone()
    pos -= (lens + 1)
    row_off = torch.cumsum(row_len, 0) - row_len + len(header)
    pos += row_off
    total = len(header) + int(row_len.sum())
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    out[: len(header)] = torch.frombuffer(bytearray(header), dtype=torch.uint8).to(dev)
    _chk(lib.cobalt_csv_write_bytes(dbuf.data_ptr(), C, N, pos.data_ptr(), lens.data_ptr(), dig.data_ptr(),
                                    dpk.data_ptr(), out.data_ptr(), stream), "cobalt_csv_write_bytes")
    if host_fix is not None and host_fix[3]:
        ci_o, ri_o, L, blob = host_fix
        L64 = L.to(torch.int64)
        start = pos[ci_o, ri_o]
        excl = torch.cumsum(L64, 0) - L64
        nb = len(blob)
        idx = torch.repeat_interleave(start - excl, L64, output_size=nb) + torch.arange(nb, device=dev)
        out[idx] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize(dev)
    tm["format"] = time.perf_counter() - t0
    data = memoryview(out.cpu().numpy())  # bytes-like, no further host copy
    del keep
    if timings is not None:
        tm["to_host"] = time.perf_counter() - t0
        timings.update({k + "_s": v for k, v in tm.items()})
        timings["bytes"] = total
    return data
