"""The GPU FASTA parse (fasta_device.hip) at every tile, scan and alignment edge, EXACTLY against an
independent reference.

The four ingest tests of test_gpu_parity.py draw random text, read it from a file and compare with the host reader.
Here the texts are aimed (fasta_texts.py: each builder asserts what it places, checked on the CPU by
test_fasta_texts.py) and the oracle is fasta_texts.reference_parse.  Every parse but the file reader's goes through
msv_fasta_parse_device on text already in device memory -- the entry the file-based tests never reach, and the only
way to a text pointer that is not 16-byte aligned (load32's byte-wise branch) and to a caller's stream.

What is placed: '>', a header's newline, a residue line's newline, a bad byte, '#', a blank line and the end of the
text at 32-byte chunk, 2 KiB wave and 8 KiB tile boundaries +-2; tiles wholly inside a header line, of newlines only,
of 4096 header starts and of 8192 residues; tiles of 0-7 residues at every alignment of the output (the copy-out's
head, words and tail); 4095-8193 records and the rejection patterns first / last / all / all but one / the longest;
more than 4096 tiles with a header or a residue line open across byte 32 Mi (the tile scans' second block); and a
file of three 64 MiB pieces (the reader's pinned double buffer reused).  Every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd._native import MSVError
import fasta_texts as ft
from oracle_lib import bits, profile_path

MSV_ERR_INVALID_ARGUMENT, MSV_ERR_PARSE = 1, 3
DEV = torch.device("cuda:0")


def upload(text: bytes, offset: int = 0) -> torch.Tensor:
    """The text in a device tensor of exactly offset + len(text) bytes, the text at byte `offset`."""
    buf = torch.empty(offset + len(text), dtype=torch.uint8, device=DEV)
    if text:
        buf[offset:] = torch.from_numpy(np.frombuffer(text, np.uint8).copy())
    return buf


def finish(dev):
    """(codes, offsets, spans, rejected) of a FASTA_device plus its (count, residues, max_length); closes it."""
    codes, offsets, spans = dev.download()
    facts = (dev.count, dev.residues, dev.max_length)
    out = (codes, offsets, spans, dev.rejected)
    dev.close()
    return out, facts


def device_parse(text: bytes, offset: int = 0, stream=None, buf=None):
    """msv_fasta_parse_device on the uploaded text: the result in reference_parse's shape, or "parse error"."""
    buf = upload(text, offset) if buf is None else buf
    assert buf.numel() >= offset + len(text)  # the pointer and the n bytes after it lie inside a live tensor
    try:
        dev = msv.FASTA_device(text_ptr=(buf.data_ptr() + offset) if buf.numel() else None, n=len(text), stream=stream)
    except MSVError as e:
        assert e.status == MSV_ERR_PARSE, e
        return "parse error", None
    return finish(dev)


def check_against(name, got, facts, want):
    diff = ft.first_difference(got, want)
    assert diff is None, f"{name}: GPU parse vs reference: {diff}"
    if not isinstance(want, str):
        lengths = np.diff(want[1].astype(np.int64))
        expect = (len(want[1]) - 1, int(want[1][-1]), int(lengths.max()) if lengths.size else 0)
        assert facts == expect, f"{name}: (count, residues, max_length) {facts}, want {expect}"


def check_text(name, text, want=None, **how):
    want = ft.parse_or_error(ft.reference_parse, text) if want is None else want
    got, facts = device_parse(text, **how)
    check_against(name, got, facts, want)
    return got, facts


@pytest.fixture(scope="module")
def families():
    return ft.small_families()


@pytest.fixture(scope="module")
def scan_block_texts():
    """The two texts of more than 4096 tiles with their references, computed once."""
    return [(name, text, ft.reference_parse(text)) for name, text in ft.scan_block_cases()]


def test_boundary_cases(families):
    for name, text in families["boundary"]:
        check_text(name, text)


def test_span_cases(families):
    for name, text in families["span"]:
        check_text(name, text)


def test_copyout_cases(families):
    for name, text in families["copyout"]:
        check_text(name, text)


def test_record_count_cases(families):
    for name, text in families["record_count"]:
        check_text(name, text)


def test_soup_cases(families):
    for name, text in families["soup"]:
        check_text(name, text)


def test_text_pointer_alignment(families):
    """The same text at tensor offsets 0, 1, 3, 15, 16 and 17: off 16-byte alignment load32 reads byte by byte, and
    the records must not change.  (torch's allocations are at least 256-byte aligned, so the offset is the
    pointer's alignment.)"""
    subset = families["boundary"][::7] + families["soup"][1:40:3] + families["copyout"][:1]
    for name, text in subset:
        want = ft.parse_or_error(ft.reference_parse, text)
        for offset in (0, 1, 3, 15, 16, 17):
            buf = upload(text, offset)
            assert buf.data_ptr() % 256 == 0
            got, facts = device_parse(text, offset, buf=buf)
            check_against(f"{name} at pointer offset {offset}", got, facts, want)


def test_parse_on_a_caller_stream(families):
    """Upload from pinned memory and parse on one side stream with no synchronisation in between: the parse must
    order itself after the copy on that stream alone."""
    side = torch.cuda.Stream(DEV)
    cases = [families["copyout"][0], families["record_count"][-1], families["boundary"][100], families["soup"][11]]
    for name, text in cases:
        want = ft.parse_or_error(ft.reference_parse, text)
        default = device_parse(text)
        pinned = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).pin_memory()
        with torch.cuda.stream(side):
            buf = pinned.to(DEV, non_blocking=True)
            got, facts = device_parse(text, stream=side.cuda_stream, buf=buf)
        side.synchronize()
        check_against(f"{name} on a side stream", got, facts, want)
        assert ft.first_difference(got, default[0]) is None and facts == default[1], name


def test_lines_open_across_a_scan_block(scan_block_texts):
    """More than 4096 tiles: the tiles of the second scan block take the header starts, the last line start and
    the residue count before them from scan_partials' carry, with a header (a residue line) open across it."""
    for name, text, want in scan_block_texts:
        assert len(text) > ft.SCAN_BLOCK * ft.TILE
        check_text(name, text, want)


def test_file_reader_reuses_its_pinned_pieces(tmp_path):
    """A file of 2 * 64 MiB + 1 MiB + 13 bytes is read in three pieces, the third into the first's pinned buffer
    once its copy is done (hipEventSynchronize(done[k & 1])).  A piece copied late, twice or out of order shows in
    the codes: the records are random and non-periodic."""
    n = 2 * (64 << 20) + (1 << 20) + 13
    text = ft.ordinary_records(n, 77)
    assert len(text) == n
    path = tmp_path / "three_pieces.fsa"
    path.write_bytes(text)
    from_file, file_facts = finish(msv.FASTA_device(str(path)))
    from_text, text_facts = device_parse(text)
    diff = ft.first_difference(from_file, from_text)
    assert diff is None, f"file reader vs uploaded text: {diff}"
    assert file_facts == text_facts
    # both ends against the reference, the slices cut at record starts
    codes, offsets, spans, _ = from_text
    slice_bytes = 8 << 20
    head_end = text.rfind(b"\n>", 0, slice_bytes) + 1
    tail_begin = text.find(b"\n>", n - slice_bytes) + 1
    assert text[head_end] == ft.GT and text[tail_begin] == ft.GT and head_end > 7 << 20 and n - tail_begin > 7 << 20
    hc, ho, hs, hr = ft.reference_parse(text[:head_end])
    k = len(ho) - 1
    got_head = (codes[:int(ho[-1])], offsets[:k + 1], spans[:k], hr)
    diff = ft.first_difference(got_head, (hc, ho, hs, hr))
    assert diff is None, f"first 8 MiB: {diff}"
    tc, to, ts, tr = ft.reference_parse(text[tail_begin:])
    k = len(to) - 1
    base = int(offsets[-1]) - int(to[-1])
    got_tail = (codes[base:], offsets[-(k + 1):] - np.uint64(base), spans[-k:] - np.array([tail_begin, 0], np.uint64), tr)
    diff = ft.first_difference(got_tail, (tc, to, ts, tr))
    assert diff is None, f"last 8 MiB: {diff}"
    assert int(offsets[-(k + 1)]) == base


def test_text_at_the_size_limit_is_refused():
    """n = 0xFFFF0000 (positions are uint32, tile indices must stay in range): MSV_ERR_INVALID_ARGUMENT from the
    size check of parse_on_device, which precedes every launch -- nothing is read."""
    buf = upload(b">a\nACD\n")
    with pytest.raises(MSVError) as err:
        msv.FASTA_device(text_ptr=buf.data_ptr(), n=0xFFFF0000)
    assert err.value.status == MSV_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()


def test_scores_reserve_by_the_longest_kept_record():
    """score_fasta_device reserves its table by max_length: with the longest record rejected that is the longest
    KEPT record's length, and the scores equal score_batch on the reference's records bitwise."""
    name, text = ft.longest_record_rejected()
    codes, offsets, _, rejected = ft.reference_parse(text)
    buf = upload(text)
    dev = msv.FASTA_device(text_ptr=buf.data_ptr(), n=len(text))
    assert dev.rejected == rejected == 1 and dev.max_length == 9 and dev.count == len(offsets) - 1
    e = msv.MSV_HMM(msv.Profile_HMM(profile_path("100.hmm")))
    got = e.score_fasta_device(dev)
    assert np.array_equal(bits(got), bits(e.score_batch(codes=codes, offsets=offsets))), name
    dev.close()
    e.close()
