"""FASTA texts aimed at the edges of the GPU parse, and an independent reference (test helper; not a conftest).

The GPU ingest (fasta_device.hip) reads the text in 32-byte thread chunks, 2 KiB waves and 8 KiB
tiles, carries a line's header-ness and the header / residue counts from tile to tile through hierarchical scans of
4096 elements per block, and copies each tile's residues out as head bytes, words and a tail.  Random text puts an
event on one of those edges only by chance.  The builders here place them: each returns (name, text) pairs and
ASSERTS what its name claims (the byte at the position, the tile a line starts in, the residue counts per tile),
so a builder that drifts fails on the CPU instead of silently testing nothing.

reference_parse states the record rules of the header comment of fasta_device.hip over whole-text numpy arrays;
loop_parse states them once more line by line.  Neither is a port of the GPU parse or of the host reader
(host_parsers.cpp); test_fasta_texts.py holds all three against each other, test_gpu_fasta_device.py the GPU parse
against reference_parse.  numpy only: no library call, no GPU.
"""
from __future__ import annotations

import functools

import numpy as np

TILE = 8192          # text bytes per block of fa_tile_summary / fa_tile_emit
SCAN_BLOCK = 4096    # elements per block of the hierarchical scans
LETTERS = b"ACDEFGHIKLMNPQRSTVWY"
NL, GT = 10, 62

_LUT = np.full(256, 254, np.uint8)
_LUT[np.frombuffer(LETTERS, np.uint8)] = np.arange(20, dtype=np.uint8)
_LUT[ord("#")] = 255
_LETTER_ARRAY = np.frombuffer(LETTERS, np.uint8)


class ParseError(Exception):
    """A non-empty line before the first header (MSV_ERR_PARSE in the library)."""


def _analyse(text: bytes):
    """(t, nl, hs, rec, res_pos): the bytes, the newline mask, the header-start mask, the number of header starts at
    or before each byte, and the positions of the residue bytes."""
    t = np.frombuffer(text, np.uint8)
    n = len(t)
    nl = t == NL
    ls = np.empty(n, bool)  # line starts: byte 0 and every byte after a newline
    ls[0] = True
    ls[1:] = nl[:-1]
    hs = ls & (t == GT)
    line = np.cumsum(ls, dtype=np.int32) - 1
    on_header = hs[np.flatnonzero(ls)][line]  # a byte is on a header line iff its line's first byte is a header start
    rec = np.cumsum(hs, dtype=np.int32)
    res_pos = np.flatnonzero(~nl & ~on_header)
    return t, nl, hs, rec, res_pos


def reference_parse(text: bytes):
    """(codes uint8, offsets uint64[kept + 1], spans uint64[kept, 2], rejected) of a FASTA text, or ParseError.

    A '>' at a line start opens a record whose header is the rest of that line ('\\r' kept; the span is
    (first byte after '>', length) and ends at the next newline or at the end of the text); every other
    non-newline byte is a residue of the record open at it, translated by the table 20 letters -> 0..19,
    '#' -> 255, anything else -> 254; a record holding a 254 is dropped; a residue before the first header is the
    parse error; empty lines do nothing; records without residues are kept."""
    n = len(text)
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros((0, 2), np.uint64), 0
    t, nl, hs, rec, res_pos = _analyse(text)
    res_rec = rec[res_pos]
    if res_rec.size and res_rec[0] == 0:  # rec is non-decreasing: the first residue is the earliest
        raise ParseError("residue bytes before the first header")
    nrec = int(rec[-1])
    all_codes = _LUT[t[res_pos]]
    per_rec = np.bincount(res_rec - 1, minlength=nrec)
    bad = np.zeros(nrec, bool)
    bad[res_rec[all_codes == 254] - 1] = True
    keep = ~bad
    codes = all_codes[keep[res_rec - 1]] if nrec else all_codes
    offsets = np.zeros(int(keep.sum()) + 1, np.uint64)
    np.cumsum(per_rec[keep], out=offsets[1:])
    hs_pos = np.flatnonzero(hs)
    nl_pos = np.append(np.flatnonzero(nl), n)  # the end of the text closes an open header line
    h_end = nl_pos[np.searchsorted(nl_pos, hs_pos)]
    spans = np.stack([hs_pos + 1, h_end - hs_pos - 1], axis=1)[keep].astype(np.uint64).reshape(-1, 2)
    return codes, offsets, spans, int(bad.sum())


def loop_parse(text: bytes):
    """The same rules line by line in plain Python (small texts only): a second, independent statement."""
    records = []  # [header start, header length, residue codes, bad]
    pos = 0
    for line in text.split(b"\n"):
        if line[:1] == b">":
            records.append([pos + 1, len(line) - 1, [], False])
        elif line:
            if not records:
                raise ParseError("residue bytes before the first header")
            for ch in line:
                k = LETTERS.find(bytes([ch]))
                if k >= 0:
                    records[-1][2].append(k)
                elif ch == ord("#"):
                    records[-1][2].append(255)
                else:
                    records[-1][3] = True
        pos += len(line) + 1
    kept = [r for r in records if not r[3]]
    codes = np.array([c for r in kept for c in r[2]], np.uint8)
    offsets = np.zeros(len(kept) + 1, np.uint64)
    np.cumsum([len(r[2]) for r in kept], out=offsets[1:])
    spans = np.array([r[:2] for r in kept], np.uint64).reshape(-1, 2)
    return codes, offsets, spans, len(records) - len(kept)


def parse_or_error(parse, text: bytes):
    """parse(text), or the string "parse error" where it raises ParseError."""
    try:
        return parse(text)
    except ParseError:
        return "parse error"


def headers_of(text: bytes, spans) -> list[str]:
    return [text[int(a):int(a) + int(b)].decode("latin-1") for a, b in spans]


def first_difference(got, want) -> str | None:
    """None where two parse results agree, otherwise a sentence naming the first differing record."""
    if isinstance(got, str) or isinstance(want, str):
        return None if isinstance(got, str) and isinstance(want, str) and got == want else \
            f"one side raised: got {got if isinstance(got, str) else 'records'}, " \
            f"want {want if isinstance(want, str) else 'records'}"
    (gc, go, gs, gr), (wc, wo, ws, wr) = got, want
    if len(go) != len(wo) or gr != wr:
        k = min(len(go), len(wo)) - 1  # the first kept record that differs, by residue end or header span
        differs = (np.asarray(go[1:k + 1]) != np.asarray(wo[1:k + 1])) | \
                  (np.asarray(gs[:k]) != np.asarray(ws[:k])).any(axis=1)
        r = int(np.flatnonzero(differs)[0]) if differs.any() else k
        return f"kept/rejected {len(go) - 1}/{gr}, want {len(wo) - 1}/{wr}; first differing kept record {r}"
    if not np.array_equal(go, wo):
        r = int(np.flatnonzero(np.asarray(go) != np.asarray(wo))[0])
        return f"offsets differ first at index {r}: {int(go[r])}, want {int(wo[r])}"
    if not np.array_equal(gs, ws):
        r = int(np.flatnonzero((np.asarray(gs) != np.asarray(ws)).any(axis=1))[0])
        return f"header span of kept record {r}: {tuple(int(x) for x in gs[r])}, want {tuple(int(x) for x in ws[r])}"
    if not np.array_equal(gc, wc):
        j = int(np.flatnonzero(np.asarray(gc) != np.asarray(wc))[0])
        r = int(np.searchsorted(np.asarray(wo), j, side="right")) - 1
        return f"codes differ first at residue {j} (kept record {r}, its residue {j - int(wo[r])}): " \
               f"{int(gc[j])}, want {int(wc[j])}"
    return None


# ---- filler -------------------------------------------------------------------------------------------------------
def _residues(rng, count: int) -> bytes:
    return _LETTER_ARRAY[rng.integers(0, 20, count)].tobytes()


def filler(length: int, rng) -> bytes:
    """Exactly `length` bytes of valid records ending in a newline (so whatever follows starts a line): a header
    first, then residue lines of varying width, a new header every seventh line."""
    out, rem, k = [], length, 0
    while rem > 0:
        if rem == 1:
            line = b"\n"
        elif k % 7 == 0 and (k == 0 or rem >= 12):
            size = min(2 + (5 * k + 3) % 11, rem)
            line = b">" + b"fillheader"[:size - 2] + b"\n"
        else:
            size = min(2 + (37 * k + 11) % 83, rem)
            line = _residues(rng, size - 1) + b"\n"
        out.append(line)
        rem -= len(line)
        k += 1
    text = b"".join(out)
    assert len(text) == length and (length == 0 or text[-1] == NL) and (length < 2 or text[0] == GT)
    return text


def _is_letter(byte: int) -> bool:
    return bytes([byte]) in LETTERS


# ---- events on chunk, wave and tile boundaries ----------------------------------------------------------------------
BOUNDARIES = (32, 2048, 8192, 16384)  # thread chunk, wave, tile, second tile
DELTAS = (-2, -1, 0, 1)
TAIL = b">tail record\nMKV\nLW\n"


def boundary_cases():
    """One text per boundary B, distance d and event, the event's byte at position B + d (for the three
    end-of-text events: len(text) == B + d)."""
    rng = np.random.default_rng(401)
    out = []
    for B in BOUNDARIES:
        for d in DELTAS:
            P = B + d
            tag = f"B{B}{d:+d}"

            text = filler(P, rng) + b">placed header\nACDEF\n" + TAIL
            assert text[P] == GT and text[P - 1] == NL
            out.append((f"header_start@{tag}", text))

            k = 5 if B == 32 else 40  # header bytes: for B > 32 the header line crosses the thread chunk before P
            text = filler(P - 1 - k, rng) + b">" + b"h" * k + b"\nACDEF\n" + TAIL
            assert text[P] == NL and text[P - 1 - k] == GT and text[P - 2 - k] == NL and NL not in text[P - k:P]
            out.append((f"header_newline@{tag}", text))

            text = filler(P - 7, rng) + _residues(rng, 7) + b"\nKLM\n" + TAIL
            assert text[P] == NL and _is_letter(text[P - 1]) and _is_letter(text[P + 1])
            out.append((f"residue_newline@{tag}", text))

            for name, byte in (("bad_byte", b"z"), ("hash", b"#")):
                text = filler(P - 5, rng) + b">e\nAC" + byte + b"DE\nFG\n" + TAIL
                assert text[P:P + 1] == byte and text[P - 5] == GT and text[P - 6] == NL
                out.append((f"{name}@{tag}", text))

            text = filler(P - 4, rng) + b"ACD\n\nEFG\n" + TAIL
            assert text[P] == NL and text[P - 1] == NL and _is_letter(text[P + 1]) and _is_letter(text[P - 2])
            out.append((f"blank_line@{tag}", text))

            text = filler(P - 4, rng) + b">end"
            assert len(text) == P and text[P - 4] == GT and text[P - 5] == NL
            out.append((f"eof_in_header@{tag}", text))

            text = filler(P - 3, rng) + b"ACD"
            assert len(text) == P and text[P - 4] == NL
            out.append((f"eof_in_residue_line@{tag}", text))

            text = filler(P - 1, rng) + b"\n"
            assert len(text) == P and text[P - 1] == NL and text[P - 2] == NL
            out.append((f"eof_after_bare_newline@{tag}", text))
    assert len(out) == len(BOUNDARIES) * len(DELTAS) * 9 and all(len(t) < 20 * 1024 for _, t in out)
    return out


# ---- whole tiles of one kind -----------------------------------------------------------------------------------------
def _tiles_inside(begin: int, end: int) -> int:
    """Whole tiles inside [begin, end)."""
    return max(0, end // TILE - (begin + TILE - 1) // TILE)


def span_cases():
    rng = np.random.default_rng(402)
    out = []

    pre = filler(5000, rng)
    text = pre + b">" + b"H" * 19999 + b"\nACDEF\n" + TAIL
    assert text[5000] == GT and text[25000] == NL and _tiles_inside(5000, 25000) >= 1
    out.append(("header_20000_from_mid_tile", text))

    pre = filler(3000, rng)
    text = pre + b">" + b"h" * 29999
    assert text[3000] == GT and NL not in text[3000:] and _tiles_inside(3000, len(text)) >= 2
    out.append(("header_30000_ended_by_eof", text))

    text = filler(TILE, rng) + b"\n" * TILE + b"ACD\n" + TAIL
    assert text[TILE:2 * TILE] == b"\n" * TILE and _is_letter(text[2 * TILE])
    out.append(("tile_of_newlines", text))

    text = b">\n" * 12288
    assert len(text) == 3 * TILE
    out.append(("4096_header_starts_per_tile", text))

    text = b">one line\n" + _residues(rng, 30000) + b"\n" + TAIL
    assert NL not in text[10:30010] and _tiles_inside(10, 30010) >= 2
    out.append(("line_of_30000_residues", text))

    for n in (1, 31, 32, 33, TILE - 1, TILE, TILE + 1):
        out.append((f"text_of_{n}_bytes", filler(n, rng)))
    out += [("empty", b""), ("one_newline", b"\n"), ("one_gt", b">"), ("one_residue", b"A"),
            ("header_without_newline", b">x"), ("two_empty_headers_then_residue", b">\n>\nA")]
    return out


# ---- the copy-out of a tile's residues ---------------------------------------------------------------------------
def tile_residue_counts(text: bytes):
    """(r_excl, count) per tile: residue bytes before the tile and in it."""
    res_pos = _analyse(text)[4]
    nt = max(1, (len(text) + TILE - 1) // TILE)
    count = np.bincount(res_pos // TILE, minlength=nt)
    return np.cumsum(count) - count, count


def copyout_cases():
    """Tiles holding a handful of residues at every alignment of their place in the output: fa_tile_emit's head
    bytes (up to a 4-byte boundary), words and tail are then the whole copy, with count < head and words == 0."""
    rng = np.random.default_rng(403)
    out = []

    # 64 records of a ~8100-byte header and c = 0..7 residues: the tile edges drift through the records
    parts = []
    for i in range(64):
        c = i % 8
        parts.append(b">" + b"d" * (8100 + 3 * (i % 5)) + b"\n" + (_residues(rng, c) + b"\n" if c else b""))
    text = b"".join(parts)
    r_excl, count = tile_residue_counts(text)
    assert set(range(8)) <= set(count.tolist()) and set((r_excl & 3).tolist()) == {0, 1, 2, 3}
    assert count.max() < 16
    out.append(("drifting_records", text))

    # one record per tile, exactly: tile t holds c[t] residues; c walks every (r_excl & 3, count) pair
    todo = {(a, c) for a in range(4) for c in range(8)}
    seq, a = [], 0
    while todo:
        here = sorted(c for (x, c) in todo if x == a)
        if here:  # an unvisited count at this alignment, preferring one that moves to an alignment with work left
            c = max(here, key=lambda c: (sum(1 for (x, y) in todo if x == (a + c) & 3 and (x, y) != (a, c)), -c))
            todo.discard((a, c))
        else:
            c = 1
        seq.append(c)
        a = (a + c) & 3
    parts = []
    for c in seq:
        body = _residues(rng, c) + b"\n" if c else b""
        parts.append(b">" + b"e" * (TILE - 2 - len(body)) + b"\n" + body)
    text = b"".join(parts)
    assert len(text) == TILE * len(seq)
    r_excl, count = tile_residue_counts(text)
    assert count.tolist() == seq
    assert {(int(a) & 3, int(c)) for a, c in zip(r_excl, count)} >= {(a, c) for a in range(4) for c in range(8)}
    out.append(("one_record_per_tile", text))
    return out


# ---- record counts across the 4096-record scan block, and rejection patterns -------------------------------------------
def _tiny_records(nrec: int, reject=()) -> bytes:
    reject = set(reject)
    return b"".join(b">\n" + (b"z" if i in reject else LETTERS[i % 20:i % 20 + 1]) + b"\n" for i in range(nrec))


def record_count_cases():
    out = [(f"{nrec}_records", _tiny_records(nrec)) for nrec in (4095, 4096, 4097, 8193)]
    n = SCAN_BLOCK + 1
    patterns = {
        "first_rejected": [0],
        "last_rejected": [n - 1],
        "all_rejected": range(n),
        "all_rejected_but_record_4096": range(n - 1),
    }
    for name, reject in patterns.items():
        text = _tiny_records(n, reject)
        kept = len(reference_parse(text)[1]) - 1
        assert kept == n - len(reject) and reference_parse(text)[3] == len(reject)
        out.append((f"4097_records_{name}", text))
    out.append(longest_record_rejected())
    return out


def longest_record_rejected():
    """4097 records of 1-9 residues and one of 500 with a bad byte in it: max_length must be the longest KEPT
    record's, and msv_score_fasta_device reserves its table by that value."""
    rng = np.random.default_rng(404)
    parts = []
    for i in range(SCAN_BLOCK + 1):
        if i == 2500:
            seq = _residues(rng, 250) + b"z" + _residues(rng, 249)
        else:
            seq = _residues(rng, 1 + i % 9)
        parts.append(b">r%d\n" % i + seq + b"\n")
    text = b"".join(parts)
    _, offsets, _, rejected = reference_parse(text)
    assert rejected == 1 and int(np.diff(offsets.astype(np.int64)).max()) == 9
    return "4097_records_longest_rejected", text


# ---- more than one scan block of tiles --------------------------------------------------------------------------------
def ordinary_records(length: int, seed: int) -> bytes:
    """`length` bytes of non-periodic records built without a Python loop: 60-column lines, a record of 1-12 lines
    opened by a numbered 60-column header line, about one record in 40 with a bad byte; ends in a newline."""
    if length == 0:
        return b""
    rng = np.random.default_rng(seed)
    t = _LETTER_ARRAY[rng.integers(0, 20, length, dtype=np.uint8)]
    t[60::61] = NL
    nlines = (length + 60) // 61
    starts = np.concatenate([[0], np.cumsum(rng.integers(1, 13, nlines // 6 + 2))])
    s = starts[starts < nlines] * 61
    t[s] = GT
    for j in range(8):  # the record's number, so no two headers are equal
        p = s + 1 + j
        ok = p < length
        t[p[ok]] = 48 + (np.arange(len(s))[ok] // 10 ** j) % 10
    bad = s[rng.random(len(s)) < 0.025] + 61 + 7  # inside the first residue line
    bad = bad[bad < length]
    t[bad[t[bad] != NL]] = ord("z")
    t[60::61] = NL
    t[-1] = NL
    return t.tobytes()


@functools.lru_cache(maxsize=None)
def scan_block_cases():
    """Two texts of more than 4096 tiles (one scan block of tiles is 32 MiB of text) with a line open across byte
    32 Mi, where the second block's tiles take that line's header-ness and the header / residue counts from the
    carry of scan_partials.  Tiles are counted from 1 here: tile 4097 is the first of the second scan block.

    header:  4096 * 8192 + 1 bytes.  A header starts in tile 4090 and runs to the end of the text, whose last byte
             is the whole of tile 4097 (56 KiB; a 60 KiB line from tile 4090 would end past this text).
    residue: 4097 * 8192 + 100 bytes.  A 60 KiB residue line starts in tile 4090 and ends in tile 4097; ordinary
             records follow to the end, 100 bytes into tile 4098."""
    edge = SCAN_BLOCK * TILE  # byte 32 Mi
    out = []

    n = edge + 1
    start = 4089 * TILE + 200
    text = ordinary_records(start, 11) + b">" + b"h" * (n - start - 1)
    assert len(text) == n and text[start] == GT and text[start - 1] == NL and NL not in text[start:]
    assert start // TILE == 4089 and start < edge < n and (n - 1) // TILE == 4096
    out.append(("header_open_across_32Mi", text))

    n = (SCAN_BLOCK + 1) * TILE + 100
    start = 4089 * TILE + 200
    end = start + 60 * 1024 - 1  # the line's newline
    pre = ordinary_records(start, 12)
    line = _LETTER_ARRAY[np.random.default_rng(13).integers(0, 20, end - start)].tobytes() + b"\n"
    text = pre + line + ordinary_records(n - end - 1, 14)
    assert len(text) == n and text[start - 1] == NL and text[end] == NL and NL not in text[start:end]
    assert GT not in text[start:end] and start // TILE == 4089 and end // TILE == 4096 and start < edge < end
    out.append(("residue_line_open_across_32Mi", text))
    return out


# ---- random soup ------------------------------------------------------------------------------------------------------
def soup_cases(seed: int, count: int = 200):
    """Random texts of 0-20,000 bytes over '>', newline, '\\r', A, C, '#', z with '>' and newline at 10-30 % each
    (line starts in every thread chunk); every other one starts with a header line so that it parses."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b">\n\rAC#z", np.uint8)
    out = []
    for i in range(count):
        n = int(rng.integers(0, 20001)) if i else 0
        p_gt, p_nl = rng.uniform(0.1, 0.3, 2)
        rest = 1.0 - p_gt - p_nl
        p = [p_gt, p_nl, 0.06 * rest, 0.41 * rest, 0.41 * rest, 0.06 * rest, 0.06 * rest]
        body = alphabet[rng.choice(7, n, p=p)].tobytes()
        out.append((f"soup{seed}_{i}", (b">s\n" if i % 2 else b"") + body))
    return out


# ---- the host reader's chunk cutting ------------------------------------------------------------------------------------
CUT_TEXT_BYTES = 33 * (1 << 20) + 77
CUT_PARTS = 8  # parse_fasta cuts a text of 32-36 MiB into min(hardware threads, 8) chunks


def cut_targets(n: int = CUT_TEXT_BYTES, parts: int = CUT_PARTS):
    """Where host_parsers.cpp:parse_fasta starts looking for the k-th cut: n k / parts."""
    return [n * k // parts for k in range(1, parts)]


@functools.lru_cache(maxsize=None)
def chunk_cut_text():
    """33 MiB whose cut targets (on a host with 8 or more threads) fall inside a long record, on a residue line's
    newline, on the newline directly before a '>' line, and on the '>' of a header line."""
    n = CUT_TEXT_BYTES
    buf, size = [], 0

    def pad_to(pos, seed):
        nonlocal size
        assert pos >= size + 2
        buf.append(ordinary_records(pos - size, seed))
        size = pos

    def add(blob):
        nonlocal size
        buf.append(blob)
        size += len(blob)

    kinds = ["in_long_record", "on_residue_newline", "before_header", "in_long_record", "on_residue_newline",
             "before_header", "on_header_start"]
    rng = np.random.default_rng(405)
    for k, (q, kind) in enumerate(zip(cut_targets(), kinds)):
        if kind == "in_long_record":
            pad_to(q - 30000, 100 + k)
            add(b">long record\n" + b"".join(_residues(rng, 60) + b"\n" for _ in range(1000)))
        elif kind == "on_residue_newline":
            pad_to(q - 4, 100 + k)
            add(b"ACDE\nFGH\n")
        elif kind == "before_header":
            pad_to(q - 2, 100 + k)
            add(b"AC\n>cut here\nKLM\n")
        else:
            pad_to(q, 100 + k)
            add(b">at the target\nAC\n")
    pad_to(n, 199)
    text = b"".join(buf)
    assert len(text) == n
    for q, kind in zip(cut_targets(), kinds):
        if kind == "in_long_record":
            lo, hi = text.rfind(b"\n>", 0, q), text.find(b"\n>", q)
            assert text[lo + 2:lo + 13] == b"long record" and hi - lo > 60000
        elif kind == "on_residue_newline":
            assert text[q] == NL and _is_letter(text[q - 1]) and _is_letter(text[q + 1])
        elif kind == "before_header":
            assert text[q] == NL and text[q + 1] == GT and _is_letter(text[q - 1])
        else:
            assert text[q] == GT and text[q - 1] == NL
    return "chunk_cut_targets", text


def small_families():
    """Every family whose texts are small (name, builder result): what the CPU and GPU files both walk."""
    return {
        "boundary": boundary_cases(),
        "span": span_cases(),
        "copyout": copyout_cases(),
        "record_count": record_count_cases(),
        "soup": soup_cases(7),
    }
