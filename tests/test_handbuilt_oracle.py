"""The hand-built corpus (tests/handbuilt_cases.py) against zlib and the oracle: the builder checks itself on every
stream RFC 1951 allows, and the oracle's verdict on every case is pinned (parse ok, bytes consumed, size bits,
decoded bytes).  The cases zlib refuses but the reference accepts are listed explicitly."""
import zlib

import pytest

import deflate_builder as DB
import handbuilt_cases as H
import oracle_lib as O

# RFC 1951 forbids these (zlib refuses them); the reference parses them — each case's note names the Java behaviour
REFERENCE_ONLY = {"hlit_287", "hlit_288", "hdist_31", "hdist_32", "cl_code_one_symbol", "rep16_crosses_into_distances",
                  "incomplete_litlen_code", "oversubscribed_eob_reachable", "oversubscribed_8bit_254_reachable",
                  "stored_nlen_cut_len0", "stored_nlen_half_len0", "stored_nlen_half_len0_other", "mixed_then_stored_nlen_cut",
                  "mixed_then_stored_nlen_half", "zlib1_sync_then_stored_nlen_cut", "stored_payload_past_eof_final"}


def test_builder_self_check():
    """Every RFC-valid stream decodes in zlib to exactly the bytes the builder meant; the reference-only cases are
    exactly the list above, and zlib refuses each of them."""
    ref_only = set()
    for c in H.cases():
        if c.rfc:
            d = zlib.decompressobj(-15)
            assert d.decompress(c.data) == c.plain and d.eof, c.name
        elif c.ok:
            ref_only.add(c.name)
            d = zlib.decompressobj(-15)
            try:
                out = d.decompress(c.data)
                refused = not d.eof or out != c.plain
            except zlib.error:
                refused = True
            assert refused, c.name
    assert ref_only == REFERENCE_ONLY


def test_builder_primitives():
    assert DB.canonical([2, 1, 3, 3]) == [2, 0, 6, 7]                        # RFC 1951 3.2.2 example shape
    assert DB.canonical([1, 1, 2]) == [0, 1, None]                          # oversubscribed: the third code does not fit
    assert DB.len_symbol(258) == (285, 0, 0) and DB.len_symbol(258, True) == (284, 31, 5)
    assert DB.dist_symbol(32768) == (29, 8191, 13)
    lens = DB.limited_lengths([1 << i for i in range(20)], 7)
    assert max(lens) == 7 and DB.kraft(lens) == 32768
    b = DB.Builder().bits(0b101, 3).code(0b110, 3)
    assert b.getvalue() == bytes([0b011101]) and b.getvalue(cut=2) == b"\x01"


@pytest.mark.parametrize("case", H.cases("small"), ids=lambda c: c.name)
def test_oracle_verdict(case):
    """Parse verdict, consumed bytes, size bits and decoded bytes of the oracle, pinned per case."""
    rc, _, _, consumed, _ = O.optimise(case.data, True)
    assert (rc >= 0) == case.ok
    assert O.size_bits(case.data) == case.size_bits
    dec, icons = O.inflate(case.data)
    assert dec == case.plain
    if case.ok:
        assert consumed == icons == case.consumed


def test_oracle_verdict_every_prefix():
    """Every bit-prefix of two mixed streams (stored, fixed, dynamic, final stored): every EOF path of the parse."""
    bad = []
    for c in H.prefixes():
        rc, _, _, consumed, _ = O.optimise(c.data, True)
        dec, _ = O.inflate(c.data)
        if (rc >= 0) != c.ok or O.size_bits(c.data) != c.size_bits or dec != c.plain or (c.ok and consumed != c.consumed):
            bad.append(c.name)
    assert not bad


def test_cut_stored_nlen_is_accepted():
    """DeflateBlockUncompressed.parse (DeflateBlockUncompressed.java:23-36) reads `readBits(16) & 0xffff`, and
    BitInputStream.readBits returns -1 once EOF is hit (BitInputStream.java:59-82): a cut-off NLEN is 0xffff == ~0,
    so LEN 0 passes and the reader sits at EOF (a following block fails its 3-bit read).  A cut LEN is 0xffff too,
    which no NLEN matches."""
    assert O.optimise(b"\x01\x00\x00", True)[0] == 1 and O.size_bits(b"\x01\x00\x00") == 40
    assert O.optimise(b"\x01\x00\x00\x37", False)[0] == 1
    for bad in (b"\x01", b"\x01\x00", b"\x01\x05\x00", b"\x00\x00\x00", b"\x00\x00\x00\xff"):
        assert O.optimise(bad, True)[0] == -1, bad


def test_optimisable_stream_ending_in_cut_stored_block():
    """zlib level 1 text, a sync flush, then a final stored block whose NLEN is cut off: the reference optimises it."""
    c = H.by_name(["zlib1_sync_then_stored_nlen_cut"])[0]
    rc, out, saved, _, _ = O.optimise(c.data, True)
    assert rc == 0 and saved > 0
    rc, out, saved_off, _, _ = O.optimise(c.data, False)
    assert rc == 0 and saved_off > 0 and out.endswith(b"\x00\x00\xff\xff")   # merge off: a complete stored header
