"""The aimed FASTA texts of fasta_texts.py on the CPU: the builders' own placement assertions run here, the two
independent statements of the record rules (reference_parse over whole-text arrays, loop_parse line by line) must
agree on every small text, and the host reader (host_parsers.cpp) must agree with reference_parse on every text --
the two of more than 32 MiB included, and one of 33 MiB whose chunk-cut targets are placed, which is the host
reader's cutting at a known size.  The GPU parse meets the same texts in test_gpu_fasta_device.py."""
import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd._native import MSVError
import fasta_texts as ft

MSV_ERR_PARSE = 3


def host_parse(path):
    """The host reader's result in reference_parse's shape, headers in place of spans."""
    try:
        fa = msv.FASTA_protein_sequences(str(path))
    except MSVError as e:
        assert e.status == MSV_ERR_PARSE, e
        return "parse error"
    return fa.codes, fa.offsets, fa.headers, fa.rejected


def check_host(tmp_path, name, text, want=None):
    path = tmp_path / "case.fsa"
    path.write_bytes(text)
    got = host_parse(path)
    want = ft.parse_or_error(ft.reference_parse, text) if want is None else want
    if isinstance(got, str) or isinstance(want, str):
        said = [r if isinstance(r, str) else "records" for r in (got, want)]
        assert said[0] == said[1], f"{name}: host reader gave {said[0]}, reference {said[1]}"
        return
    codes, offsets, headers, rejected = got
    # the header strings become spans by position in the reference's list: equal lists <=> equal strings
    want_headers = ft.headers_of(text, want[2])
    diff = ft.first_difference((codes, offsets, want[2], rejected), want)
    assert diff is None, f"{name}: host reader vs reference: {diff}"
    if headers != want_headers:
        r = next(i for i, (a, b) in enumerate(zip(headers, want_headers)) if a != b)
        raise AssertionError(f"{name}: header of kept record {r}: {headers[r][:60]!r}, want {want_headers[r][:60]!r}")


FAMILIES = ("boundary", "span", "copyout", "record_count", "soup")


@pytest.fixture(scope="module")
def families():
    return ft.small_families()  # every builder's placement assertions run in here


def test_builders_place_what_they_claim(families):
    names = [name for fam in families.values() for name, _ in fam]
    assert len(names) == len(set(names))
    assert len(families["boundary"]) == 144 and len(families["soup"]) == 200
    # the soup must hold both kinds of text, or its parse-error half tests nothing
    results = [ft.parse_or_error(ft.reference_parse, t) for _, t in families["soup"]]
    errors = sum(isinstance(r, str) for r in results)
    assert 40 <= errors <= 100, errors
    assert sum(1 for r in results if not isinstance(r, str) and r[3] > 0 and len(r[1]) > 1) >= 50
    for name, text in ft.scan_block_cases():
        assert len(text) > ft.SCAN_BLOCK * ft.TILE, name
    ft.chunk_cut_text()


@pytest.mark.parametrize("family", FAMILIES)
def test_reference_parse_equals_loop_parse(families, family):
    for name, text in families[family]:
        assert len(text) < 1 << 20
        got = ft.parse_or_error(ft.reference_parse, text)
        want = ft.parse_or_error(ft.loop_parse, text)
        diff = ft.first_difference(got, want)
        assert diff is None, f"{name}: reference_parse vs loop_parse: {diff}"


def test_reference_parse_on_known_texts():
    """The rules on texts small enough to check by eye."""
    codes, offsets, spans, rejected = ft.reference_parse(b"\n\n>a b\r\nAC\n\nD#\n>bad\nAzC\n>\n>end")
    assert codes.tolist() == [0, 1, 2, 255] and offsets.tolist() == [0, 4, 4, 4] and rejected == 1
    assert spans.tolist() == [[3, 4], [25, 0], [27, 3]]
    assert ft.parse_or_error(ft.reference_parse, b"\n\nA\n>a\n") == "parse error"
    assert ft.parse_or_error(ft.reference_parse, b"\r\n>a\n") == "parse error"
    assert ft.reference_parse(b"")[1].tolist() == [0] and ft.reference_parse(b"\n")[1].tolist() == [0]
    assert ft.reference_parse(b">x")[2].tolist() == [[1, 1]]
    assert ft.reference_parse(b">\n>\nA")[1].tolist() == [0, 0, 1]
    assert ft.reference_parse(b">a\nA>C\n")[3] == 1  # '>' inside a line is a bad residue, not a header


@pytest.mark.parametrize("family", FAMILIES)
def test_host_reader_equals_reference(families, family, tmp_path):
    for name, text in families[family]:
        check_host(tmp_path, name, text)


def test_host_reader_on_texts_past_one_scan_block(tmp_path):
    for name, text in ft.scan_block_cases():
        check_host(tmp_path, name, text)


def test_host_reader_chunk_cuts_at_placed_targets(tmp_path):
    """33 MiB: the reader cuts it into up to 8 chunks, and every target it starts looking from sits inside a long
    record, on a residue line's newline, directly before a "\\n>" or on a header's '>'."""
    name, text = ft.chunk_cut_text()
    want = ft.reference_parse(text)
    assert want[3] > 100 and len(want[1]) > 50_000  # rejected records on both sides of every cut
    check_host(tmp_path, name, text, want)
