"""Hand-placed inputs and plain references for the GPU CSV reader (csrc/csv.hip, prep/csv_gpu.py), shared by
test_csv_edges_cpu.py (which checks these references against Python's csv module, pyarrow and pandas) and
test_gpu_csv_edges.py (which checks the kernels against them).

Offsets are offsets into the BODY: ``read_csv_gpu`` drops the header line before it uploads the buffer, so the
kernels' chunk (64 KB) and segment (256 B) boundaries fall at body offsets whatever the header's length, and an
end-to-end file is simply ``header(C) + body``.
"""
from __future__ import annotations

import functools
import struct

from cobalt_smart_lender_ai_amd.prep.device_frame import PANDAS_NA

SEG = 256  # bytes one thread walks (kCsvSeg)
_M = (1 << 64) - 1


def csv_chunk() -> int:
    """Bytes per tokenizer block: the library's own figure where it is loaded, else 65536."""
    from cobalt_smart_lender_ai_amd import _native

    if _native._lib is not None:
        from cobalt_smart_lender_ai_amd.prep import csv_gpu  # noqa: F401  (declares the signature)

        return int(_native._lib.cobalt_csv_chunk())
    return 65536


# ------------------------------------------------------------------------------------------ references
def ref_tokenize(body: bytes, C: int, chunk: int | None = None):
    """Sequential RFC 4180 state machine: (quotes per chunk, delimiters per chunk, offsets of the delimiters
    that end a field, delimiters whose kind -- newline or comma -- disagrees with ``ordinal % C``)."""
    ch = chunk or csv_chunk()
    nch = -(-len(body) // ch)
    qc, dc, fend, bad, inq = [0] * nch, [0] * nch, [], 0, False
    for p, c in enumerate(body):
        if c == 0x22:
            inq = not inq
            qc[p // ch] += 1
        elif not inq and (c == 0x2C or c == 0x0A):
            bad += (c == 0x0A) != (len(fend) % C == C - 1)
            fend.append(p)
            dc[p // ch] += 1
    return qc, dc, fend, bad


def ref_fields(body: bytes, C: int) -> list[list[str]]:
    """Rows of unescaped field texts cut at ``ref_tokenize``'s offsets (the end of the body ends a last field
    that has no newline); a row's trailing ``\\r`` and enclosing quotes are stripped, ``""`` undone."""
    fend = ref_tokenize(body, C)[2]
    if body and body[-1] != 0x0A:
        fend = fend + [len(body)]
    out, s = [], 0
    for k, e in enumerate(fend):
        f = body[s:e]
        s = e + 1
        if k % C == C - 1 and f.endswith(b"\r"):
            f = f[:-1]
        if len(f) >= 2 and f[:1] == b'"' and f[-1:] == b'"':
            f = f[1:-1].replace(b'""', b'"')
        out.append(f.decode("utf-8"))
    return [out[i:i + C] for i in range(0, len(out), C)]


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M
    return x ^ (x >> 31)


def ref_field_hash(content: bytes) -> int:
    """k_csv_hash of a field's unescaped content: 8-byte little-endian words folded through splitmix64 from the
    seed, the last (partial, possibly empty) word XOR ``len << 56``; 0 is kept for missing values."""
    if content.decode("utf-8", "replace") in PANDAS_NA:
        return 0
    h = 0x9E3779B97F4A7C15
    n = len(content)
    full = n - n % 8
    for (w,) in struct.iter_unpack("<Q", content[:full]):
        h = splitmix64(h ^ w)
    w = int.from_bytes(content[full:], "little")
    h = splitmix64(h ^ w ^ ((n << 56) & _M))
    return h or 1


COLLISION_PAIR = (b"collide-me-00001", b"KK4zuWqDGBBeUjke")


def find_collision(first: bytes = COLLISION_PAIR[0], seed: int = 0) -> bytes:
    """A second 16-byte alphanumeric string with ``first``'s hash: splitmix64 is a bijection, so for any other
    first word the second word that collides is determined; try first words until it is alphanumeric."""
    import random

    rng = random.Random(seed)
    alnum = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"
    s0 = 0x9E3779B97F4A7C15
    a1, a2 = struct.unpack("<QQ", first)
    target = splitmix64(s0 ^ a1) ^ a2
    while True:
        p = bytes(rng.choice(alnum) for _ in range(8))
        w2 = (splitmix64(s0 ^ struct.unpack("<Q", p)[0]) ^ target).to_bytes(8, "little")
        if p != first[:8] and all(c in alnum for c in w2):
            return p + w2


# ------------------------------------------------------------------------------------------ builders
def place(prefix: bytes, at: int, fill: bytes = b"x") -> bytes:
    """``prefix`` extended with filler bytes (the start, or all, of a field) so that the next byte appended
    lands at body offset ``at``."""
    assert at >= len(prefix) and len(fill) == 1, (at, len(prefix))
    return prefix + fill * (at - len(prefix))


COLS = ["id", "name", "amount", "text", "tag", "tail"]  # string and numeric columns on both sides of "text"
_NAMES = [b"alpha", b'"Gamma, Inc."', "ünïcødé".encode(), b'"NA"', b'""', b"beta", b'"say ""hi"""']
_AMOUNTS = [b"1.5", b"-2", b"", b"1e3"]
_TAGS = [b"red", b'"blue"', b"", "grün".encode()]


def header(C: int) -> bytes:
    names = COLS if C == len(COLS) else [f"c{j}" for j in range(C)]
    return (",".join(names) + "\n").encode()


def _row(i: int, name: bytes | None = None, text: bytes | None = None) -> bytes:
    return b",".join([b"%d" % i, _NAMES[i % 7] if name is None else name, _AMOUNTS[i % 4],
                      b"t%d" % (i % 5) if text is None else text, _TAGS[i % 4], b"%d" % (i % 3)]) + b"\n"


def _rows_until(limit: int, start: int = 0) -> tuple[bytes, int]:
    """Whole ordinary rows, as many as end at or before body offset ``limit``; and the next row number."""
    out, n, i = [], 0, start
    while True:
        r = _row(i)
        if n + len(r) > limit:
            return b"".join(out), i
        out.append(r)
        n += len(r)
        i += 1


def _boundary_body(kind: str, at: int) -> bytes:
    """A 6-column body whose token of ``kind`` has its first byte at body offset ``at``."""
    pre, i = _rows_until(at - 64)
    tail = _TAGS[i % 4] + b",%d" % (i % 3)
    if kind == "esc":        # "" inside a quoted field, one quote on each side of ``at``
        b = place(pre + b'%d,alpha,1.5,"' % i, at) + b'""rest",' + tail + b"\n"
    elif kind == "open":     # the opening quote of a field
        b = place(pre + b"%d," % i, at - 5) + b',1.5,"q, r",' + tail + b"\n"
    elif kind == "close":    # the closing quote of a field
        b = place(pre + b'%d,alpha,1.5,"a,' % i, at) + b'",' + tail + b"\n"
    elif kind == "crlf":     # \r at ``at``, \n after it
        b = place(pre + b"%d," % i, at - len(b",1.5,t1," + tail)) + b",1.5,t1," + tail + b"\r\n"
    elif kind == "lf":
        b = place(pre + b"%d," % i, at - len(b",1.5,t1," + tail)) + b",1.5,t1," + tail + b"\n"
    elif kind == "comma":    # an unquoted delimiter
        b = place(pre + b"%d," % i, at) + b",1.5,t1," + tail + b"\n"
    else:
        raise ValueError(kind)
    token = {"esc": b'""', "open": b'"', "close": b'"', "crlf": b"\r\n", "lf": b"\n", "comma": b","}[kind]
    assert b[at:at + len(token)] == token, (kind, at)
    return b + b"".join(_row(j) for j in range(i + 1, i + 4))


def _ragged_body(kind: str, at: int) -> bytes:
    """As _boundary_body, with the newline at ``at`` ending a row one field short, one field long, or a short
    row that a long row follows (the field total stays a multiple of 6)."""
    pre, i = _rows_until(at - 64)
    short, long_ = b",1.5,t1,red\n", b",1.5,t1,red,0,9\n"
    end = long_ if kind == "long" else short
    b = place(pre + b"%d," % i, at + 1 - len(end)) + end
    assert b[at] == 0x0A
    if kind == "short_long":
        b += b"%d,beta" % (i + 1) + long_
    return b + b"".join(_row(j) for j in range(i + 2, i + 5))


def _long_field_body(start: int, field: bytes) -> bytes:
    pre, i = _rows_until(start)
    return pre + _row(i, text=field) + _row(i + 1) + _row(i + 2)


def _length_body(n: int, newline: bool) -> tuple[bytes, int]:
    """A body of exactly ``n`` bytes that does (not) end in a newline; two columns (one when n == 1)."""
    if n == 1:
        return (b"\n" if newline else b"7"), 1
    rows = b"12,xy\n" * ((n - 8) // 6 if n >= 14 else 0)
    last = place(rows + b"3,", n - 1 if newline else n, b"z") + (b"\n" if newline else b"")
    assert len(last) == n
    return last, 2


def _short_columns_body(C: int, rows: int) -> bytes:
    return b"".join(b",".join(b"%d" % ((r + j) % 10) for j in range(C)) + b"\n" for r in range(rows))


@functools.lru_cache(maxsize=None)
def positions() -> tuple[int, ...]:
    """B - 1 and B for both chunk boundaries B inside a three-chunk body, and S - 1 for a segment boundary S
    in the first chunk and in the second."""
    ch = csv_chunk()
    return (ch - 1, ch, 2 * ch - 1, 2 * ch, 3 * SEG - 1, ch + 2 * SEG - 1)


BOUNDARY_KINDS = ("esc", "open", "close", "crlf", "lf", "comma")
RAGGED_KINDS = ("short", "long", "short_long")
_LONG_UNIT = b'ab,c\nd\r\ne""f'  # commas, newlines and an escaped quote, 12 bytes
LENGTHS = (1, 15, 16, 17, 65535, 65536, 65537, 131072)


@functools.lru_cache(maxsize=None)
def wellformed_bodies() -> dict[str, tuple[bytes, int]]:
    """name -> (body, C). Every second boundary body has its final newline removed."""
    ch = csv_chunk()
    out: dict[str, tuple[bytes, int]] = {}
    for kind in BOUNDARY_KINDS:
        for k, at in enumerate(positions()):
            b = _boundary_body(kind, at)
            out[f"{kind}@{at}"] = (b[:-1] if k % 2 else b, 6)
    # a 70,000-byte quoted field that covers the whole second chunk, and a chunk-long run of quotes
    fld = b'"' + _LONG_UNIT * 5834 + b'"'
    long_ = _long_field_body(ch - 4000, fld)
    s = long_.index(fld)
    assert len(fld) >= 70000 and s < ch and s + len(fld) > 2 * ch and len(long_) < 3 * ch
    out["long_quoted_field"] = (long_, 6)
    out["quote_run"] = (_long_field_body(100, b'"' + b'""' * (ch // 2 + 200) + b'"'), 6)
    for n in LENGTHS:
        for nl in (True, False):
            out[f"len{n}{'nl' if nl else ''}"] = _length_body(n, nl)
    out["ends_in_cr"] = (b"1,x\r\n2,y\r", 2)
    for C, rows in ((1, 900), (2, 700), (15, 60), (300, 5)):
        out[f"C{C}"] = (_short_columns_body(C, rows), C)
    return out


# bodies the GPU engine may refuse where the host readers read something: "\n" alone is a blank line
MAY_DEFER = ("len1nl",)


@functools.lru_cache(maxsize=None)
def ragged_bodies() -> dict[str, tuple[bytes, int]]:
    return {f"{kind}@{at}": (_ragged_body(kind, at), 6) for kind in RAGGED_KINDS for at in positions()}


# ------------------------------------------------------------------------------------------ literals
def arrow_table(data: bytes):
    """pyarrow's reading of ``data`` with the options of DeviceFrame.read_csv's arrow engine."""
    import pyarrow as pa
    import pyarrow.csv as pcsv

    return pcsv.read_csv(pa.BufferReader(data), read_options=pcsv.ReadOptions(use_threads=False),
                         convert_options=pcsv.ConvertOptions(strings_can_be_null=True, null_values=PANDAS_NA,
                                                             quoted_strings_can_be_null=True))


def literal_files(lit: str) -> dict[str, bytes]:
    """Shape (a): the literal alone beside an integer column; shape (b): among ordinary integers / floats."""
    return {"alone": f"a,b\n{lit},1\n".encode(),
            "ints": f"a,b\n3,1\n{lit},2\n25,3\n".encode(),
            "floats": f"a,b\n3,1\n{lit},2\n2.5,3\n".encode()}


_INF = float("inf")
_D, _I, _S, _B, _N = "double", "int64", "string", "bool", "null"
# literal, pyarrow's type and value of column a alone, its type among integers, among floats
LITERALS = [
    ("inf", _D, _INF, _D, _D), ("Inf", _D, _INF, _D, _D), ("INF", _D, _INF, _D, _D), ("-inf", _D, -_INF, _D, _D),
    ("-Inf", _D, -_INF, _D, _D), ("+inf", _D, _INF, _D, _D), ("Infinity", _D, _INF, _D, _D),
    ("-Infinity", _D, -_INF, _D, _D), ("infinity", _D, _INF, _D, _D),
    ("1e5", _D, 1e5, _D, _D), ("1E5", _D, 1e5, _D, _D), ("1.", _D, 1.0, _D, _D), (".5", _D, 0.5, _D, _D),
    ("5.", _D, 5.0, _D, _D), ("-.5", _D, -0.5, _D, _D), ("+.5e1", _D, 5.0, _D, _D), ("1.0e+00", _D, 1.0, _D, _D),
    ("1e400", _D, _INF, _D, _D), ("1e-400", _D, 0.0, _D, _D),
    ("1e", _S, "1e", _S, _S), ("1e+", _S, "1e+", _S, _S), (".", _S, ".", _S, _S), ("-", _S, "-", _S, _S),
    ("+", _S, "+", _S, _S), ("1_5", _S, "1_5", _S, _S), ("٣", _S, "٣", _S, _S),
    (" 1", _I, 1, _I, _D), ("1 ", _I, 1, _I, _D), (" 1.5 ", _D, 1.5, _D, _D),
    ("0x10", _I, 16, _I, _S), ("00012", _I, 12, _I, _D), ("-0", _I, 0, _I, _D), ("+0", _D, 0.0, _D, _D),
    ("9223372036854775807", _I, 9223372036854775807, _I, _D), ("9223372036854775808", _D, 9223372036854775808.0, _D, _D),
    ("-9223372036854775808", _I, -9223372036854775808, _I, _D),
    ("-9223372036854775809", _D, -9223372036854775808.0, _D, _D),
    ("9999999999999999999", _D, 1e19, _D, _D), ("12345678901234567890", _D, 1.2345678901234567e19, _D, _D),
    ("TRUE", _B, True, _S, _S), ("tRUE", _S, "tRUE", _S, _S), ("T", _S, "T", _S, _S),
    ('"12"', _I, 12, _I, _D), ('"1.5"', _D, 1.5, _D, _D), ('"True"', _B, True, _S, _S), ('"NA"', _N, None, _I, _D),
    ('""', _N, None, _I, _D),
    # beyond the issue's list: the other spellings pyarrow's float parser takes
    ("NAN", _D, float("nan"), _D, _D), ("+nan", _D, float("nan"), _D, _D), ("nan(1)", _D, float("nan"), _D, _D),
    ("\t1", _I, 1, _I, _D), (" 0X1f", _I, 31, _I, _S), ("-0x10", _S, "-0x10", _S, _S), (" inf", _D, _INF, _D, _D),
    ("9007199254740992", _I, 9007199254740992, _I, _D), ("9007199254740993", _I, 9007199254740993, _I, _D),
] + [(s, _N, None, _I, _D) for s in PANDAS_NA if s]

SHAPE_FILES = {"blank_line_one_column": b"a\n1\n\n2\n", "blank_crlf_line_one_column": b"a\r\n1\r\n\r\n2\r\n",
               "header_only": b"a,b\n", "quote_then_text": b'a,b\n1,"x"y\n', "quote_then_blank": b'a,b\n1,"x" \n',
               "quote_inside_unquoted": b'a,b\n1,x"y"\n2,z\n', "one_column_quoted_empty": b'a\n1\n""\n2\n'}

# float_precision="high" against pandas' default conversion: infinity spellings, padded and int64-edge literals
# in float syntax
HIGH_LITERALS = [s for s, *_ in LITERALS[:9]] + [
    " 1.5 ", " 1.0", "1.0 ", "\t2.5", " inf", "1e5 ", "9223372036854775807.0", "9223372036854775808.0",
    "-9223372036854775808.0", "-9223372036854775809.0", "9999999999999999999.0", "12345678901234567890.0",
    "9007199254740993.0", "00012.50"]


# ------------------------------------------------------------------------------------------ rounding
def rounding_strings() -> list[str]:
    """Decimal strings at the rounding edges of the float conversion (reference: Python's ``float``)."""
    from decimal import ROUND_CEILING, ROUND_FLOOR, Context, Decimal

    out = ["9007199254740993.0", "9007199254740992.0", "9007199254740991.0", "9007199254740995.0",
           "9007199254740992", "9007199254740993", "-9007199254740993.0",
           "0.500000000000000166533453693773481063544750213623046875",
           "0.50000000000000016653345369377348106354475021362304687500000001",
           "1.00000000000000011102230246251565404236316680908203125",
           "1.7976931348623157e308", "1.7976931348623159e308", "1.7976931348623158e308", "2.2250738585072014e-308",
           "2.2250738585072011e-308", "5e-324", "2.4703282292062328e-324", "2.4703282292062327e-324", "4.9e-324",
           "1234567890123456789e0", "12345678901234567890e0", "1234567890123456789.0", "12345678901234567890.0",
           "9999999999999999999e0", "0.1234567890123456789", "0.12345678901234567890", "0.0", "-0.0", "0e999",
           "1e22", "1e23", "1e-22", "1e-23", "8.5e22", "8.5e23", "3.3e-22", "3.3e-23"]
    for m in ("9007199254740992", "9007199254740993", "9007199254740991", "1.2345678901234567", "7", "1.5",
              "9.999999999999999999"):
        out += [f"{m}e{e}" for e in (22, -22, 23, -23, 290, -290, 291, -291, 272, -272, 308, -308)]
    for e in range(-1000, 1001, 40):  # 17..19 digits just below and just above 2^e
        p = Decimal(2) ** e
        for nd in (17, 18, 19):
            for rnd in (ROUND_FLOOR, ROUND_CEILING):
                out.append(format(Context(prec=nd, rounding=rnd).create_decimal(p), "e"))
    return out


def random_reprs(n: int = 20000, seed: int = 5) -> list[str]:
    """``repr`` of random doubles with a decimal exponent within +-290."""
    import random

    rng = random.Random(seed)
    out = []
    while len(out) < n:
        v = rng.uniform(1.0, 10.0) * 10.0 ** rng.randint(-290, 289)
        if 1e-290 <= v < 1e290:
            out.append(repr(v if rng.random() < 0.5 else -v))
    return out
