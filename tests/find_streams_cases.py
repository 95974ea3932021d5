"""Files with embedded zlib / gzip streams for d4g_find_streams, and what the library must report for each.

Every expected record comes from how the file was assembled — the offset a stream was put at, the header written in
front of it, the builder's own bit count and decoded bytes (tests/deflate_builder.py) — none from the library.
`brute_force` is the CPU reference: Python zlib tried at every offset whose header predicate holds, then the overlap
rule; test_case_builder_against_zlib holds the builder to it.  The streams are all valid for zlib and for the library's
parser alike (complete codes, window 32 KiB in the header), so the two notions of a valid payload coincide here."""
import functools
import random
import struct
import zlib

from deflate_builder import Builder, Ref

import handbuilt_cases as H

ZLIB, GZIP = 1, 2
KIND_NAMES = {ZLIB: "zlib", GZIP: "gzip"}
FIELDS = ("file", "kind", "kind_name", "offset", "payload_offset", "payload_len", "total_len", "decoded_len", "size_bits", "crc32", "adler32",
          "n_blocks")
FHCRC, FEXTRA, FNAME, FCOMMENT = 2, 4, 8, 16


def filler(n, seed):
    return random.Random(seed).randbytes(n)


class Payload:
    """a raw DEFLATE stream as the builder wrote it: bytes, decoded bytes, size in bits, number of blocks"""
    def __init__(self, b, n_blocks):
        self.data, self.plain, self.bits, self.n_blocks = b.getvalue(), bytes(b.final_plain), b.final_end, n_blocks
        assert b.valid and (self.bits + 7) // 8 == len(self.data)


def tokens(b, n, seed, alphabet=40):
    """n decoded bytes of literals and back-references into what `b` has decoded so far (this block's bytes included)"""
    r = random.Random(seed)
    out, have, made = [], len(b.plain), 0
    while made < n:
        if have > 8 and r.random() < 0.35:
            ln = min(r.randint(3, 60), n - made)
            if ln >= 3:
                out.append(Ref(ln, r.randint(1, min(have, 4000))))
                have += ln
                made += ln
                continue
        out.append(32 + r.randrange(alphabet))
        have += 1
        made += 1
    return out


@functools.lru_cache(maxsize=None)
def small(seed, n=300):
    """one block, fixed or dynamic by the seed"""
    b = Builder()
    t = tokens(b, n, seed)
    b.fixed(t, final=True) if seed % 3 == 0 else b.dynamic(t, final=True)
    return Payload(b, 1)


@functools.lru_cache(maxsize=None)
def multi_block(seed=7):
    """dynamic, stored, fixed, dynamic, an empty stored block, fixed: back-references cross the block borders"""
    b = Builder()
    b.dynamic(tokens(b, 2500, seed))
    b.stored(filler(700, seed + 1))
    b.fixed(tokens(b, 400, seed + 2))
    b.dynamic(tokens(b, 3000, seed + 3, alphabet=90))
    b.stored(b"")
    b.fixed(tokens(b, 50, seed + 4), final=True)
    return Payload(b, 6)


@functools.lru_cache(maxsize=None)
def long_block():
    """one dynamic block of 66 000 literals (more than 65 536 tokens: the doubling copy path decodes it)"""
    r = random.Random(11)
    b = Builder()
    b.dynamic([65 + r.randrange(16) for _ in range(66000)], final=True)
    return Payload(b, 1)


def empty_payload():
    b = Builder()
    b.fixed([], final=True)
    return Payload(b, 1)


def zlib_header(cmf=0x78, flg=0x9c):
    assert (cmf * 256 + flg) % 31 == 0
    return bytes([cmf, flg])


def gzip_header(flags=0, extra=b"", name=b"", comment=b"", good_hcrc=True):
    h = bytearray(b"\x1f\x8b\x08" + bytes([flags]) + struct.pack("<I", 0x5eadbeef) + b"\x02\x03")
    if flags & FEXTRA:
        h += struct.pack("<H", len(extra)) + extra
    if flags & FNAME:
        h += name + b"\0"
    if flags & FCOMMENT:
        h += comment + b"\0"
    if flags & FHCRC:
        h += struct.pack("<H", (zlib.crc32(bytes(h)) & 0xffff) ^ (0 if good_hcrc else 1))
    return bytes(h)


def trailer(kind, plain):
    if kind == ZLIB:
        return struct.pack(">I", zlib.adler32(plain))
    return struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff)


class Case:
    def __init__(self, name, kinds=0, min_decoded=0):
        self.name, self.kinds, self.min_decoded = name, kinds, min_decoded
        self.buf = bytearray()
        self.want = []          # the records, `file` = 0

    @property
    def data(self):
        return bytes(self.buf)

    def __repr__(self):
        return "Case(%s)" % self.name

    def fill(self, n, seed):
        self.buf += filler(n, seed)
        return self

    def raw(self, data):
        self.buf += data
        return self

    def stream(self, kind, p, header=None, report=True):
        """header + payload + trailer at the current end; the record, unless the options of the case filter it out"""
        header = header if header is not None else (zlib_header() if kind == ZLIB else gzip_header())
        off = len(self.buf)
        self.buf += header + p.data + trailer(kind, p.plain)
        if report and (self.kinds == 0 or self.kinds & (1 << kind)) and len(p.plain) >= self.min_decoded:
            self.want.append(dict(file=0, kind=kind, kind_name=KIND_NAMES[kind], offset=off, payload_offset=off + len(header),
                                  payload_len=len(p.data), total_len=len(header) + len(p.data) + (4 if kind == ZLIB else 8),
                                  decoded_len=len(p.plain), size_bits=p.bits, crc32=zlib.crc32(p.plain), adler32=zlib.adler32(p.plain),
                                  n_blocks=p.n_blocks))
        return self


def wanted(case, file_index=0):
    return [dict(w, file=file_index) for w in case.want]


def mixed_file(name, kinds=0, min_decoded=0):
    """zlib and gzip streams in 200 KiB of filler: single blocks, the multi-block stream, an empty stream"""
    c = Case(name, kinds, min_decoded)
    seed = 100
    for k in range(16):
        c.fill(12500 + 37 * k, seed + k)
        if k == 5:
            c.stream(ZLIB, multi_block())
        elif k == 9:
            c.stream(GZIP, multi_block(8), gzip_header(FNAME, name=b"multi.bin"))
        elif k == 12:
            c.raw(bytes.fromhex("789c030000000001"))
            if (kinds == 0 or kinds & (1 << ZLIB)) and min_decoded == 0:
                off = len(c.buf) - 8
                c.want.append(dict(file=0, kind=ZLIB, kind_name="zlib", offset=off, payload_offset=off + 2, payload_len=2, total_len=8,
                                   decoded_len=0, size_bits=10, crc32=0, adler32=1, n_blocks=1))
        else:
            c.stream(GZIP if k % 2 else ZLIB, small(k, 200 + 90 * k), zlib_header(0x78, (0x01, 0x5e, 0x9c, 0xda)[k % 4]) if k % 2 == 0 else None)
    return c.fill(3000, seed + 50)


def decode_with_history(hist, toks):
    out = bytearray(hist)
    for t in toks:
        if isinstance(t, Ref):
            for _ in range(t.length):
                out.append(out[-t.dist])
        else:
            out.append(t)
    return bytes(out[len(hist):])


@functools.lru_cache(maxsize=None)
def cases():
    cs = []
    cs.append(Case("zlib_at_offset_0").stream(ZLIB, small(1)).fill(900, 1))
    cs.append(Case("ends_on_last_byte").fill(3001, 2).stream(GZIP, small(2)))
    cs.append(Case("back_to_back").fill(777, 3).stream(ZLIB, small(3)).stream(GZIP, small(4)).stream(ZLIB, small(5, 40)).fill(100, 4))
    cs.append(mixed_file("mixed_200k"))
    cs.append(Case("gzip_all_optional_fields").fill(1234, 5)
              .stream(GZIP, small(6), gzip_header(FEXTRA | FNAME | FCOMMENT | FHCRC, extra=b"\x41\x70\x04\x00abcd", name=b"file.txt", comment=b"a comment"))
              .fill(2000, 6).stream(GZIP, small(7), gzip_header(FEXTRA | FHCRC, extra=b"")).fill(50, 7))
    cs.append(Case("multi_block").fill(5000, 8).stream(ZLIB, multi_block()).fill(5000, 9))
    cs.append(Case("long_block").fill(2048, 10).stream(ZLIB, long_block()).fill(100, 11))
    cs.append(Case("empty_stream_min_0").fill(500, 12).stream(ZLIB, empty_payload()).fill(500, 13).stream(GZIP, small(8, 64)).fill(20, 14))
    cs.append(Case("empty_stream_min_1", min_decoded=1).fill(500, 12).stream(ZLIB, empty_payload()).fill(500, 13).stream(GZIP, small(8, 64)).fill(20, 14))
    assert bytes(cs[-2].buf[500:508]) == bytes.fromhex("789c030000000001") and len(cs[-2].want) == 2 and len(cs[-1].want) == 1
    c = Case("dense_empty_streams").fill(100, 15)       # more wrapper headers in one scan tile than a workgroup's own list holds
    for _ in range(100):
        c.stream(ZLIB, empty_payload())
    cs.append(c.fill(50, 16))
    # ---- decoys: nothing of them is reported (the good stream after each shows the search went on) ----
    p = small(20)
    good = small(21, 100)
    c = Case("trailer_bit_flipped").fill(300, 20).stream(ZLIB, p, report=False)
    c.buf[-2] ^= 0x10
    cs.append(c.fill(300, 21).stream(GZIP, p, report=False))
    c.buf[-6] ^= 0x01                                               # (the CRC-32)
    c.fill(40, 22).stream(ZLIB, good)
    c = Case("gzip_wrong_isize").fill(300, 23).stream(GZIP, p, report=False)
    c.buf[-4:] = struct.pack("<I", len(p.plain) + 1)
    cs.append(c.fill(40, 24).stream(ZLIB, good))
    whole = zlib_header() + p.data + trailer(ZLIB, p.plain)
    cs.append(Case("truncated_in_payload").stream(ZLIB, good).fill(300, 25).raw(whole[:2 + len(p.data) // 2]))
    cs.append(Case("truncated_in_trailer").stream(ZLIB, good).fill(300, 26).raw(whole[:-1]))
    gz = gzip_header() + p.data + trailer(GZIP, p.plain)
    cs.append(Case("gzip_truncated_in_trailer").stream(ZLIB, good).fill(300, 27).raw(gz[:-3]))
    assert (0x78 * 256 + 0xbb) % 31 == 0
    cs.append(Case("fdict_set").fill(300, 28).raw(bytes([0x78, 0xbb]) + p.data + trailer(ZLIB, p.plain)).fill(30, 29).stream(ZLIB, good))
    cs.append(Case("gzip_reserved_flag").fill(300, 30).raw(gzip_header(0x20) + p.data + trailer(GZIP, p.plain)).fill(30, 31).stream(ZLIB, good))
    never = bytes(x or 1 for x in gzip_header(FNAME, name=b"x")[:-1] + b"name" + p.data + trailer(GZIP, p.plain) + filler(200, 32))
    cs.append(Case("fname_never_terminates").stream(ZLIB, good).fill(64, 33).raw(bytes(x or 7 for x in filler(100, 34))).raw(never))
    # a back-reference that reaches before the payload, into bytes that would satisfy it, with the trailer those bytes give
    c = Case("distance_before_payload").fill(400, 35)
    b = Builder()
    toks = [Ref(6, 9)] + tokens(b, 200, 36)
    b.fixed(toks, final=True)
    plain = decode_with_history(bytes(c.buf) + zlib_header(), toks)
    c.raw(zlib_header() + b.getvalue() + trailer(ZLIB, plain))
    cs.append(c.fill(30, 37).stream(ZLIB, good))
    # a complete zlib stream carried verbatim in a stored block of a reported stream
    inner = zlib_header() + good.data + trailer(ZLIB, good.plain)
    b = Builder()
    b.fixed(tokens(b, 100, 38))
    b.stored(b"before" + inner + b"after")
    b.dynamic(tokens(b, 300, 39), final=True)
    cs.append(Case("stream_in_a_stored_block").fill(300, 40).stream(ZLIB, Payload(b, 3)).fill(30, 41).raw(inner))
    cs[-1].want.append(dict(wanted(Case("x").stream(ZLIB, good))[0], offset=len(cs[-1].buf) - len(inner),
                            payload_offset=len(cs[-1].buf) - len(inner) + 2))           # (outside the outer stream it counts)
    cs.append(Case("4k_of_78_9c").raw(b"\x78\x9c" * 2048).stream(ZLIB, good))
    # ---- options ----
    cs.append(mixed_file("mixed_200k_zlib_only", kinds=1 << ZLIB))
    cs.append(mixed_file("mixed_200k_gzip_only", kinds=1 << GZIP))
    cs.append(Case("no_streams").fill(20000, 42))
    cs.append(Case("empty_file"))
    assert all(len(c.buf) <= 256 << 10 for c in cs) and len({c.name for c in cs}) == len(cs)
    return cs


def by_name(*names):
    d = {c.name: c for c in cases()}
    return [d[n] for n in names]


def calls():
    """the cases grouped by their options: each group is one d4g_find_streams call"""
    groups = {}
    for c in cases():
        groups.setdefault((c.kinds, c.min_decoded), []).append(c)
    return [(k, m, cs) for (k, m), cs in groups.items()]


def copies(n, seed=60):
    """n copies of one stream between filler that holds no wrapper header at all (so both files cost the same walk)"""
    def clean(d):
        return bytes(x if (x & 15) != 8 and x != 0x1f else x ^ 1 for x in d)
    c = Case("copies_%d" % n)
    for k in range(n):
        c.raw(clean(filler(300, seed + k))).stream(ZLIB if k % 2 else GZIP, small(9))
    return c.raw(clean(filler(100, seed - 1)))


@functools.lru_cache(maxsize=None)
def many_streams(n=1000, size=4 << 20, seed=70):
    """n small zlib streams in `size` bytes of filler: 150 of them packed back to back (more wrapper headers in one scan
    tile than a workgroup's own list holds), the rest spread evenly"""
    c = Case("many_streams")
    pool = [small(200 + k, 24 + 5 * k) for k in range(40)]
    dense = 150
    gap = (size - sum(len(pool[k % 40].data) + 6 for k in range(n))) // (n - dense + 1)
    for k in range(n):
        if k < n // 2 or k >= n // 2 + dense:
            c.fill(gap, seed + k)
        c.stream(ZLIB, pool[k % 40] if not (n // 2 <= k < n // 2 + dense) else empty_payload())
    c.fill(size - len(c.buf), seed - 1)
    assert len(c.buf) == size and len(c.want) == n
    return c


def synth_file(size, n_streams, seed=80):
    """The measurement file: n_streams zlib level-9 streams of the synth.py mix (repetitive text, every fourth one
    PNG-IDAT-like; 16-64 KiB of payload each, 32 distinct ones in turn) evenly spread in `size` bytes of random filler.
    -> (data, [(kind, offset, total_len)], the payloads)"""
    import synth
    r = random.Random(seed)
    pool = []
    for k in range(32 if n_streams else 0):
        n = r.randint(90, 250) << 10
        while True:
            raw = synth.pngidat(n, seed + k) if k % 4 == 3 else synth.reptext(n, seed + k)
            pl = H.z(raw)
            if len(pl) >= 16 << 10:
                break
            n *= 2
        while len(pl) > 64 << 10:
            raw = raw[:len(raw) * 3 // 4]
            pl = H.z(raw)
        assert 16 << 10 <= len(pl) <= 64 << 10, len(pl)
        pool.append((raw, pl))
    buf, want, payloads = bytearray(), [], []
    gap = size // max(1, n_streams)
    for k in range(n_streams):
        raw, pl = pool[k % 32]
        kind = GZIP if k % 8 == 5 else ZLIB
        s = (zlib_header() if kind == ZLIB else gzip_header()) + pl + trailer(kind, raw)
        buf += r.randbytes(max(0, gap * (k + 1) - len(s) - len(buf)))
        want.append((kind, len(buf), len(s)))
        payloads.append(pl)
        buf += s
    buf += r.randbytes(max(0, size - len(buf)))
    return bytes(buf), want, payloads


# ---- EmbeddedFile ----
def round_trip(D, L, mode=0, merge=True):
    """EmbeddedFile through optimise_files: every stream of the output is found again where `relocations` says, decodes
    to the same bytes, and the bits saved are what Batch.run gives on the same payloads alone"""
    from deft4j_amd import containers as C
    c = by_name("back_to_back")[0]
    plains = []
    for w in c.want:
        plains.append(zlib.decompress(c.data[w["payload_offset"]:w["payload_offset"] + w["payload_len"]], -15))
    E = C.EmbeddedFile(min_decoded=0)
    (out, lines), (none, fail), (out2, lines2) = C.optimise_files([c.data, by_name("no_streams")[0].data, c.data], merge,
                                                                  formats=[E, "embedded", C.EmbeddedFile(0)], lib=L, mode=mode)
    assert none is None and fail == ["Failed to read file"] and (out2, lines2) == (out, lines)
    assert lines[0] == "File type recognised as Embedded streams" and [n for n, _ in E.stream_payloads()] == \
        ["%s stream at %d" % (w["kind_name"], w["offset"]) for w in c.want]
    payloads = [pl for _, pl in E.stream_payloads()]
    assert payloads == [c.data[w["payload_offset"]:w["payload_offset"] + w["payload_len"]] for w in c.want]
    again = D.find_streams([out], lib=L)[0]
    assert len(again) == len(c.want) == len(E.relocations)
    shift = 0
    for w, a, (oo, ol, no, nl), plain in zip(c.want, again, E.relocations, plains):
        assert (oo, ol) == (w["offset"], w["total_len"]) and (no, nl) == (a["offset"], a["total_len"]) and no == oo + shift
        assert out[max(0, no - 5):no] == c.data[max(0, oo - 5):oo]
        shift += nl - ol
        assert zlib.decompress(out[a["payload_offset"]:a["payload_offset"] + a["payload_len"]], -15) == plain
        assert (a["decoded_len"], a["adler32"], a["crc32"]) == (w["decoded_len"], w["adler32"], w["crc32"])
        assert out[no:no + a["payload_offset"] - no] == c.data[oo:w["payload_offset"]]                       # the header, as it was
    assert len(out) == len(c.data) + shift and out[again[-1]["offset"] + again[-1]["total_len"]:] == c.data[c.want[-1]["offset"] + c.want[-1]["total_len"]:]
    b = D.Batch(payloads, lib=L)
    b.run_recompress(mode, merge) if mode > 0 else b.run(merge)
    saved = [b.result(i)["saved_bits"] for i in range(len(payloads))]
    sizes = [b.result(i)["out_len"] for i in range(len(payloads))]
    b.close()
    total = [int(x.split()[-1]) for x in lines if x.startswith("Total bits saved")]
    assert sum(saved) > 0 and total == [sum(saved)]
    assert [a["payload_len"] for a in again] == sizes
    return lines


# ---- the CPU reference ----
def header_ok(d, o, kinds=0):
    if (kinds == 0 or kinds & (1 << ZLIB)) and o + 2 <= len(d) and (d[o] & 15) == 8 and (d[o] >> 4) <= 7 and (d[o] * 256 + d[o + 1]) % 31 == 0 and \
            not d[o + 1] & 0x20:
        return ZLIB
    if (kinds == 0 or kinds & (1 << GZIP)) and o + 10 <= len(d) and d[o] == 0x1f and d[o + 1] == 0x8b and d[o + 2] == 8 and not d[o + 3] & 0xe0:
        return GZIP
    return 0


def brute_force(data, kinds=0, min_decoded=0, offsets=None):
    """Python zlib at every offset whose header predicate holds (zlib checks the trailer itself), then the overlap rule.
    `offsets`: a superset of those offsets found some faster way (large files).
    -> [(kind, offset, total_len, decoded_len, crc32, adler32)]"""
    mv = memoryview(data)
    out, end = [], 0
    for o in (range(len(data)) if offsets is None else offsets):
        kind = header_ok(data, o, kinds)
        if not kind:
            continue
        d = zlib.decompressobj(15 if kind == ZLIB else 31)
        pos, n, crc, adl = o, 0, 0, 1
        try:
            while not d.eof and pos < len(data):
                piece = d.decompress(mv[pos:pos + 65536])
                pos += min(65536, len(data) - pos)
                n, crc, adl = n + len(piece), zlib.crc32(piece, crc), zlib.adler32(piece, adl)
        except zlib.error:
            continue
        if not d.eof or n < min_decoded or o < end:
            continue
        end = pos - len(d.unused_data)
        out.append((kind, o, end - o, n, crc, adl))
    return out
