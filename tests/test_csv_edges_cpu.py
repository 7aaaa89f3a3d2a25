"""The references of csv_edge_cases.py against independent readers, so that a wrong reference cannot pass a
wrong kernel (test_gpu_csv_edges.py): the sequential tokenizer against Python's csv module and pyarrow on every
well-formed boundary body, the hash mirror on the constructed collision, and the literal table against the
pyarrow installed here."""
import csv
import io
import math

import pytest

import csv_edge_cases as ce

BODIES = ce.wellformed_bodies()


def _arrow_rows(data: bytes) -> list[list[str]]:
    import pyarrow as pa
    import pyarrow.csv as pcsv

    names = next(csv.reader(io.StringIO(data.split(b"\n", 1)[0].decode())))
    opts = pcsv.ConvertOptions(column_types={n: pa.large_string() for n in names}, strings_can_be_null=False)
    tab = pcsv.read_csv(pa.BufferReader(data), read_options=pcsv.ReadOptions(use_threads=False, block_size=1 << 22),
                        parse_options=pcsv.ParseOptions(newlines_in_values=True), convert_options=opts)
    cols = [c.to_pylist() for c in tab.columns]
    return [list(r) for r in zip(*cols)]


@pytest.mark.parametrize("name", sorted(BODIES))
def test_ref_tokenize_cuts_the_fields_csv_and_pyarrow_cut(name):
    body, C = BODIES[name]
    qc, dc, fend, bad = ce.ref_tokenize(body, C)
    assert bad == 0 and sum(qc) == body.count(b'"') and sum(dc) == len(fend)
    got = ce.ref_fields(body, C)
    assert all(len(r) == C for r in got)
    if name not in ce.MAY_DEFER:  # a lone "\n" is no row to either reader
        want = list(csv.reader(io.StringIO(body.decode("utf-8"), newline="")))
        assert got == want
        if C > 1:  # pyarrow skips the empty line that a one-column row with an empty value is
            assert got == _arrow_rows(ce.header(C) + body)


@pytest.mark.parametrize("name", sorted(ce.ragged_bodies()))
def test_ref_tokenize_counts_ragged_rows(name):
    body, C = ce.ragged_bodies()[name]
    _, _, fend, bad = ce.ref_tokenize(body, C)
    assert bad > 0
    rows = list(csv.reader(io.StringIO(body.decode("utf-8"), newline="")))
    assert {len(r) for r in rows} - {C}  # the csv module sees a row of another width too
    assert len(fend) == sum(len(r) for r in rows)


def test_boundary_tokens_sit_on_the_boundaries():
    ch = ce.csv_chunk()
    assert ch % ce.SEG == 0
    for at in ce.positions():
        assert (at + 1) % ch == 0 or at % ch == 0 or ((at + 1) % ce.SEG == 0 and (at + 1) % ch != 0)
        body = BODIES[f"esc@{at}"][0]
        assert body[at - 1:at + 3] == b'x""r'
        assert BODIES[f"open@{at}"][0][at - 1:at + 2] == b',"q'
        assert BODIES[f"close@{at}"][0][at - 1:at + 2] == b'x",'
        assert BODIES[f"crlf@{at}"][0][at:at + 2] == b"\r\n"
        assert BODIES[f"lf@{at}"][0][at] == 0x0A and BODIES[f"comma@{at}"][0][at] == 0x2C
    for n in ce.LENGTHS:
        assert len(BODIES[f"len{n}"][0]) == n == len(BODIES[f"len{n}nl"][0])
        assert BODIES[f"len{n}nl"][0].endswith(b"\n") and not BODIES[f"len{n}"][0].endswith(b"\n")
    long_ = BODIES["long_quoted_field"][0]
    qc, dc, _, _ = ce.ref_tokenize(long_, 6)
    assert dc[1] == 0 and qc[1] > 0  # the whole second chunk lies inside one quoted field
    assert max(len(b) for b, _ in BODIES.values()) < 200_000


def test_ref_field_hash_collides_on_the_constructed_pair_only():
    a, b = ce.COLLISION_PAIR
    assert a != b and ce.ref_field_hash(a) == ce.ref_field_hash(b)
    assert ce.ref_field_hash(ce.find_collision(a, seed=1)) == ce.ref_field_hash(a)
    plain = [b"a", b"b", b"ab", b"ba", b"abcdefgh", b"abcdefghi", b"abcdefgh\0", b"collide-me-00002", b"x" * 16, b"x" * 17]
    assert len({ce.ref_field_hash(s) for s in plain}) == len(plain)
    assert all(ce.ref_field_hash(s.encode()) == 0 for s in ce.PANDAS_NA)
    assert ce.ref_field_hash(b"NAN") != 0


def _same(x, y) -> bool:
    if isinstance(x, float) and isinstance(y, float):
        return (math.isnan(x) and math.isnan(y)) or (x == y and math.copysign(1, x) == math.copysign(1, y))
    return type(x) is type(y) and x == y


@pytest.mark.parametrize("row", ce.LITERALS, ids=[repr(r[0]) for r in ce.LITERALS])
def test_literal_table_is_what_pyarrow_returns(row):
    lit, typ, val, typ_ints, typ_floats = row
    files = ce.literal_files(lit)
    col = ce.arrow_table(files["alone"]).column("a")
    assert str(col.type) == typ
    assert _same(col.to_pylist()[0], val), (col.to_pylist(), val)
    for shape, want in (("ints", typ_ints), ("floats", typ_floats)):
        c = ce.arrow_table(files[shape]).column("a")
        assert str(c.type) == want, shape
        assert c.to_pylist()[0] == ("3" if want == "string" else 3) and len(c) == 3


def test_shape_files_as_pyarrow_reads_them():
    t = {k: ce.arrow_table(v) for k, v in ce.SHAPE_FILES.items()}
    assert t["blank_line_one_column"].column("a").to_pylist() == [1, 2]
    assert t["blank_crlf_line_one_column"].column("a").to_pylist() == [1, 2]
    assert t["header_only"].num_rows == 0 and t["header_only"].column_names == ["a", "b"]
    assert t["quote_then_text"].column("b").to_pylist() == ["xy"]
    assert t["quote_then_blank"].column("b").to_pylist() == ["x "]
    assert t["one_column_quoted_empty"].column("a").to_pylist() == [1, None, 2]
    assert t["quote_inside_unquoted"].num_rows == 2
