"""Deterministic corpus of hand-built raw DEFLATE streams (tests/deflate_builder.py): the shapes zlib never writes.

A case pins the reference's verdict: `ok` (DeflateStream.parse succeeds), `consumed` (bytes read), `size_bits`
(DeflateStream.getSizeBits, -1 when the parse fails) and `plain` (the decoded bytes).  `rfc` marks the streams
RFC 1951 allows, which zlib must decode to `plain` exactly.  Size class "small" runs in the emulator, "large" on the
GPU only.  `compare()` is the check every test of the corpus runs against the oracle."""
import random
import zlib

import deflate_builder as DB
from deflate_builder import Builder, Raw, Ref

import synth


class Case:
    def __init__(self, name, data, ok, plain=b"", consumed=0, size_bits=-1, rfc=False, size="small", note=""):
        self.name, self.data, self.ok = name, data, ok
        self.plain = bytes(plain) if ok else None
        self.consumed, self.size_bits = (consumed, size_bits) if ok else (0, -1)
        self.rfc, self.size, self.note = rfc, size, note

    def __repr__(self):
        return "Case(%s)" % self.name


def mk(name, b, cut=None, trailing=b"", ok=None, plain=None, size="small", note=""):
    """A case from a builder.  By default exactly the RFC-valid, uncut streams parse; consumed and size bits follow
    from where the first final block ends (a cut stored payload reads as 0xff bytes, BitInputStreamUtil.readFromBIS)."""
    data = b.getvalue(cut, trailing)
    rfc = b.valid and cut is None
    if ok is None:
        ok = rfc
    if not ok:
        return Case(name, data, False, size=size, note=note)
    end = b.final_end
    return Case(name, data, True, b.final_plain if plain is None else plain, min((end + 7) // 8, len(data)), end, rfc, size,
                note)


def expand(syms):
    """the code lengths a list of code-length symbols writes (a 16 repeats the previous length, a zero after 17 / 18)"""
    out = []
    for s, r in syms:
        out += [0] * r if s in (17, 18) else [out[-1]] * r if s == 16 else [s]
    return out


def lit_freq(tokens, n, extra=()):
    """literal/length symbol counts of a block (EOB included), plus one for each symbol in `extra`"""
    f = [0] * n
    for tk in list(tokens) + list(extra):
        f[Builder()._syms(tk)[0] if not isinstance(tk, int) else tk] += 1
    f[256] += 1
    return f


def chain(syms, n):
    """lengths 1, 2, ..., k-1, k, k over `syms` (complete): the last two symbols get the longest code"""
    out = [0] * n
    for i, s in enumerate(syms):
        out[s] = min(i + 1, len(syms) - 1)
    return out


def text(n, seed=1):
    return list(synth.reptext(n, seed))


def z(data, level=9, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


# ---- headers ----
def header_cases():
    cs = []
    t = text(400, 1)
    refs = t[:200] + [Ref(40, 150), Ref(258, 199)] + t[200:]
    cs.append(mk("hlit_257", Builder().dynamic(t, final=True)))
    b = Builder().dynamic(refs, final=True, lit_lens=DB.limited_lengths(lit_freq(refs, 286), 15))
    cs.append(mk("hlit_286", b))
    for hlit in (287, 288):
        # HLIT 287 / 288: RFC 1951 allows 286 at most (zlib: "too many length or distance symbols"); the reference reads
        # them (initDynamicDecoder only refuses HLIT > 288, DeflateBlockHuffman.java:892-1010).  286 / 287 get
        # nonzero lengths that the data never uses.
        f = lit_freq(refs, hlit, [286, 287][:hlit - 286])
        b = Builder().dynamic(refs, final=True, lit_lens=DB.limited_lengths(f, 15))
        cs.append(mk("hlit_%d" % hlit, b, ok=True, note="HLIT > 286: reference accepts"))
    d1 = t[:50] + [Ref(10, 1)] + t[50:80]
    cs.append(mk("hdist_1", Builder().dynamic(d1, final=True, dist_lens=[1])))
    d2 = t[:50] + [Ref(10, 1), Ref(7, 2)] + t[50:80]
    cs.append(mk("hdist_30", Builder().dynamic(d2, final=True, dist_lens=[1, 1] + [0] * 28)))
    # HDIST 31 / 32: the distance lengths of codes 30 / 31 are read and never used (DeflateBlockHuffman.java:892-1010)
    cs.append(mk("hdist_31", Builder().dynamic(d2, final=True, dist_lens=[1, 2] + [0] * 28 + [2]), ok=True,
                 note="HDIST > 30: reference accepts"))
    cs.append(mk("hdist_32", Builder().dynamic(d2, final=True, dist_lens=[1, 2] + [0] * 28 + [3, 3]), ok=True,
                 note="HDIST > 30: reference accepts"))
    cs.append(mk("hclen_19_trailing_zeros", Builder().dynamic(t, final=True, hclen=19)))
    # HCLEN 4 leaves lengths only for 16, 17, 18 and 0: every code length is zero, so no EOB can be decoded
    cl = [0] * 19
    cl[17], cl[18], cl[0] = 2, 2, 1
    cs.append(mk("hclen_4_all_zero", Builder().dynamic([], final=True, lit_lens=[0] * 257, dist_lens=[0], cl_syms=[(18, 138), (18, 119), (0, None)],
                                                       cl_lens=cl, hclen=4, eob=False), ok=False))
    # HCLEN 5 (16, 17, 18, 0, 8): literals 0..254 and EOB at 8 bits, written without runs
    ll = [8] * 255 + [0, 8]
    cl = [0] * 19
    cl[8], cl[0] = 1, 1
    raw = [random.Random(5).randrange(255) for _ in range(600)]
    cs.append(mk("hclen_5_two_cl_symbols", Builder().dynamic(raw, final=True, lit_lens=ll, dist_lens=[0], rle="none", cl_lens=cl)))
    # a code-length code of one symbol (9, one-bit code 0): 258 lengths of 9 bits — an incomplete literal/length
    # code, and an incomplete code-length code; zlib refuses both, the reference decodes them (Huffman.java:170-197)
    cl = [0] * 19
    cl[9] = 1
    cs.append(mk("cl_code_one_symbol", Builder().dynamic(t[:100], final=True, lit_lens=[9] * 257, dist_lens=[9], cl_syms=[(9, None)] * 258,
                                                         cl_lens=cl), ok=True, note="incomplete codes: reference accepts"))
    # a 16 right after a 17 / 18 repeats the zero it wrote
    syms = [(18, 97), (3, None), (16, 5), (3, None), (17, 3), (16, 3), (18, 138), (17, 8), (3, None), (0, None)]
    lens = expand(syms)
    assert len(lens) == 258 and DB.kraft(lens[:257]) == 32768
    cs.append(mk("rep16_after_zero_run", Builder().dynamic(list(b"abcdefggfedcba" * 3), final=True, lit_lens=lens[:257], dist_lens=lens[257:],
                                                           cl_syms=syms)))
    # runs that end exactly at HLIT + HDIST, and that cross from the literal/length into the distance lengths
    syms = [(18, 120), (2, None), (2, None), (2, None), (18, 133), (2, None), (17, 3), (17, 5)]
    lens = expand(syms)
    assert len(lens) == 257 + 8 and lens[256] == 2 and lens[120:123] == [2, 2, 2]
    cs.append(mk("run_ends_at_hlit_plus_hdist", Builder().dynamic(list(b"xyzzy"), final=True, lit_lens=lens[:257], dist_lens=lens[257:],
                                                                  cl_syms=syms)))
    syms = [(18, 97), (2, None), (2, None), (18, 138), (18, 19), (2, None), (16, 3), (0, None), (2, None)]
    lens = expand(syms)    # EOB (256) = 2, distance codes 0..2 = 2 (the 16 crosses), 3 = 0, 4 = 2
    assert len(lens) == 257 + 5 and lens[256] == 2 and lens[257:] == [2, 2, 2, 0, 2]
    cs.append(mk("rep16_crosses_into_distances", Builder().dynamic(list(b"abbaab"), final=True,
                                                                   lit_lens=lens[:257], dist_lens=lens[257:], cl_syms=syms,
                                                                   hlit=257, hdist=5), ok=True, note="incomplete literal code"))
    joint = t[:100] + [Ref(12, 40), Ref(30, 90)]
    lf = lit_freq(joint, 274)   # HLIT 274: lengths of 267..273 are zero, like distance codes 0..9
    b = Builder().dynamic(joint, final=True, lit_lens=DB.limited_lengths(lf, 15), dist_lens=[0] * 10 + [1, 0, 1], rle="joint")
    cs.append(mk("zero_run_crosses_into_distances", b))
    # invalid: a run that overshoots HLIT + HDIST (DeflateBlockHuffman.java:892-1010: i + n > combined), a 16 first
    syms = [(18, 97), (2, None), (2, None), (18, 138), (18, 19), (2, None), (16, 6)]
    cs.append(mk("run_overshoots", Builder().dynamic(list(b"ab"), final=True, lit_lens=expand(syms)[:257], dist_lens=[2, 2], cl_syms=syms,
                                                     hlit=257, hdist=2), ok=False))
    syms = [(16, 3)] + DB.rle_lengths([0] * 94 + [2, 2] + [0] * 160 + [1, 1])
    cs.append(mk("rep16_first", Builder().dynamic(list(b"ab"), final=True, cl_syms=syms), ok=False))
    return cs


# ---- codes ----
def code_cases():
    cs = []
    t = text(3000, 2)
    ll = [0] * 257
    ll[ord("a")] = ll[ord("b")] = ll[256] = 2
    cs.append(mk("incomplete_litlen_code", Builder().dynamic(list(b"abba" * 20), final=True, lit_lens=ll, dist_lens=[0]), ok=True,
                 note="incomplete code: reference accepts"))
    cs.append(mk("one_distance_code_len1", Builder().dynamic(t[:60] + [Ref(9, 4), Ref(20, 4)], final=True, dist_lens=[0, 0, 0, 1])))
    cs.append(mk("hdist1_zero_literal_only", Builder().dynamic(t[:500], final=True, dist_lens=[0])))
    # codes of 11..15 bits (past the 10-bit LUT): literal/length and distance chains of lengths 1..15
    lsyms = [ord(c) for c in "etaoinshrd"] + [257, 258, 265, 270, 256, 284]
    dsyms = list(range(16))
    rng = random.Random(3)
    toks = [ord(c) for c in "etaoinshrd" * 40]
    for _ in range(400):
        k = rng.randrange(len(lsyms))
        s = lsyms[k]
        if s == 256:
            continue
        if s < 256:
            toks.append(s)
        else:
            d = rng.choice([1, 2, 3, 4, 5, 9, 17, 33, 65, 129, 193, 256])
            length = {257: 3, 258: 4, 265: 11, 270: 23, 284: 258}[s]
            toks.append(Ref(length, d, use284=s == 284))
    cs.append(mk("codes_11_to_15_bits", Builder().dynamic(toks, final=True, lit_lens=chain(lsyms, 286), dist_lens=chain(dsyms, 30))))
    # oversubscribed codes (Huffman.buildCodes assigns codes past 2^len that no read can match, Huffman.java:35-64;
    # readSymbol takes the first code that matches, :170-197): zlib refuses, the reference decodes what is reachable
    ll = [0] * 257
    ll[ord("a")], ll[256], ll[ord("b")] = 1, 1, 2
    cs.append(mk("oversubscribed_eob_reachable", Builder().dynamic(list(b"aaaa"), final=True, lit_lens=ll, dist_lens=[0]), ok=True,
                 note="oversubscribed: 'b' unreachable, reference accepts"))
    ll = [8] * 256 + [7]
    raw = [random.Random(4).randrange(254) for _ in range(3000)]
    cs.append(mk("oversubscribed_8bit_254_reachable", Builder().dynamic(raw, final=True, lit_lens=ll, dist_lens=[0]), ok=True,
                 note="oversubscribed: literals 254/255 unreachable, reference accepts"))
    ll = [0] * 257
    ll[ord("a")], ll[ord("b")], ll[256] = 1, 1, 1
    cs.append(mk("oversubscribed_eob_unreachable", Builder().dynamic(list(b"ab"), final=True, lit_lens=ll, dist_lens=[0], eob=False)
                 .bits(0, 16), ok=False))
    # a fixed-length 8-bit code: every token is 8 bits, so a chunk started at a wrong phase never falls into step
    ll = [8] * 255 + [0, 8]
    for n, size in ((8000, "small"), (100 * 1024, "large")):
        raw = [random.Random(n).randrange(255) for _ in range(n)]
        cs.append(mk("fixed_length_8bit_%d" % n, Builder().dynamic(raw, final=True, lit_lens=ll, dist_lens=[0]), size=size))
    # one-bit tokens: more than 512 in every 512-bit chunk
    ll = [0] * 257
    ll[ord("a")], ll[ord("b")], ll[256] = 1, 2, 2
    cs.append(mk("one_bit_tokens", Builder().dynamic(list(b"a" * 5000 + b"b" + b"a" * 1200), final=True, lit_lens=ll, dist_lens=[0])))
    return cs


# ---- tokens ----
def token_cases():
    cs = []
    # dense 48-bit tokens: 15-bit length code 284 + 5 extra bits, 15-bit distance code 29 + 13 extra bits
    rng = random.Random(6)
    lits = list(range(97, 110))
    lead = [lits[min(int(rng.expovariate(0.9)), 12)] for _ in range(33000)]
    toks = lead + [Ref(227 + rng.randrange(32), 24577 + rng.randrange(8192), use284=True) for _ in range(2500)]
    cs.append(mk("dense_48bit_tokens", Builder().dynamic(toks, final=True, lit_lens=chain(lits + [256, 284, 285], 286),
                                                         dist_lens=chain(list(range(14)) + [28, 29], 30))))
    t = text(40000, 7)
    cs.append(mk("len258_as_284_31_and_285", Builder().dynamic(t[:300] + [Ref(258, 100, True), Ref(258, 100), Ref(258, 257, True)] + t[300:400],
                                                               final=True)))
    cs.append(mk("distance_32768", Builder().dynamic(t[:33000] + [Ref(100, 32768), Ref(258, 32768, True), Ref(3, 32767)], final=True)))
    cs.append(mk("distance_equals_history", Builder().dynamic(t[:77] + [Ref(5, 77)], final=True)))
    cs.append(mk("distance_past_history", Builder().dynamic(t[:77] + [Ref(5, 78)], final=True), ok=False))
    cs.append(mk("distance_across_stored_fixed", Builder().stored(bytes(t[:100])).fixed(t[100:110] + [Ref(9, 110)], final=True)))
    cs.append(mk("distance_past_stored_fixed", Builder().stored(bytes(t[:100])).fixed(t[100:110] + [Ref(9, 111)], final=True), ok=False))
    cs.append(mk("distance_across_fixed_stored_dyn", Builder().fixed(t[:40]).stored(bytes(t[40:90])).dynamic([Ref(30, 90), Ref(3, 1)], final=True)))
    cs.append(mk("overlap_dist1_len258", Builder().fixed([120, Ref(258, 1), Ref(258, 1, True), 121, Ref(100, 2)], final=True)))
    return cs


# ---- blocks ----
def block_cases():
    cs = []
    t = bytes(text(140000, 8))
    cs.append(mk("empty_dynamic", Builder().dynamic([]).dynamic(list(t[:50]), final=True)))
    cs.append(mk("empty_dynamic_final", Builder().dynamic([], final=True)))
    cs.append(mk("empty_fixed", Builder().fixed([]).fixed([], final=True)))
    for n, size in ((300, "small"), (3000, "large")):
        b = Builder()
        for _ in range(n):
            b.stored(b"")
        cs.append(mk("empty_stored_x%d" % n, b.fixed(list(t[:20]), final=True), size=size))
    cs.append(mk("stored_0", Builder().stored(b"", final=True)))
    cs.append(mk("stored_65535", Builder().stored(t[:65535], final=True)))
    cs.append(mk("stored_pair_65535", Builder().stored(t[:30000]).stored(t[30000:65535], final=True)))
    cs.append(mk("stored_pair_65536", Builder().stored(t[:30000]).stored(t[30000:65536], final=True)))
    cs.append(mk("stored_run_past_65535", Builder().stored(t[:65535]).stored(t[65535:65536]).stored(t[70000:71000]).fixed(list(t[:10]), final=True)))
    cs.append(mk("stored_nonzero_padding", Builder().fixed(list(t[:3])).stored(t[3:40], pad=0x5b).fixed(list(t[:2])).stored(t[:9], final=True, pad=0x7f)))
    for p in range(8):
        b = Builder().fixed([200] * ((p - 2) % 8))    # 10 + 9 n bits: the dynamic block starts at bit phase p
        assert b.nbits % 8 == p
        cs.append(mk("dynamic_at_phase_%d" % p, b.dynamic(list(t[:2000]) + [Ref(40, 1000)], final=True)))
    return cs


# ---- stream ends ----
def mixed():
    t = bytes(text(2000, 9))
    return Builder().stored(t[:7]).fixed(list(t[7:20]) + [Ref(10, 13)]).dynamic(list(t[20:90]) + [Ref(50, 60)])


def end_cases():
    cs = []
    t = bytes(text(3000, 10))
    cs.append(mk("trailing_bytes", Builder().dynamic(list(t[:300]), final=True), trailing=b"\x07\xff\x00trailing"))
    b = Builder().fixed(list(t[:30])).dynamic(list(t[30:200]), final=True).stored(t[:40]).fixed(list(t[:9]), final=True)
    cs.append(mk("bfinal_on_middle_block", b))
    # stored LEN / NLEN cut off: readBits returns -1 once EOF is hit (BitInputStream.java:59-82) and `& 0xffff` makes
    # it 0xffff (DeflateBlockUncompressed.java:23-36): a cut LEN never matches, a cut NLEN matches LEN == 0
    cs.append(Case("stored_nlen_cut_len0", b"\x01\x00\x00", True, b"", 3, 40, note="NLEN reads as 0xffff"))
    cs.append(Case("stored_nlen_half_len0", b"\x01\x00\x00\xff", True, b"", 4, 40, note="NLEN reads as 0xffff"))
    cs.append(Case("stored_nlen_half_len0_other", b"\x01\x00\x00\x12", True, b"", 4, 40, note="NLEN reads as 0xffff"))
    cs.append(Case("stored_len_cut", b"\x01", False))
    cs.append(Case("stored_len_half", b"\x01\x00", False))
    cs.append(Case("stored_nlen_cut_len5", b"\x01\x05\x00", False))
    cs.append(Case("stored_nlen_cut_len0_nonfinal", b"\x00\x00\x00", False))
    b = mixed().stored(b"", final=True)
    full = b.getvalue()
    cs.append(Case("mixed_then_stored_nlen_cut", full[:-2], True, b.final_plain, len(full) - 2, b.final_end, note="NLEN reads as 0xffff"))
    cs.append(Case("mixed_then_stored_nlen_half", full[:-1], True, b.final_plain, len(full) - 1, b.final_end, note="NLEN reads as 0xffff"))
    # an optimisable stream that ends in that cut-off final stored block
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    body = c.compress(bytes(text(20000, 11))) + c.flush(zlib.Z_SYNC_FLUSH)
    cs.append(Case("zlib1_sync_then_stored_nlen_cut", body + b"\x01\x00\x00", True, zlib.decompressobj(-15).decompress(body),
                   len(body) + 3, len(body) * 8 + 40, note="optimisable; NLEN reads as 0xffff"))
    # a stored payload past EOF: its missing bytes read as 0xff (BitInputStreamUtil.readFromBIS: (byte) -1); a
    # non-final block then fails its next 3-bit read
    b = Builder().fixed(list(t[:20])).stored(t[20:120], final=True)
    full = b.getvalue()
    cs.append(Case("stored_payload_past_eof_final", full[:-30], True, t[:90] + b"\xff" * 30, len(full) - 30, b.final_end))
    cs.append(mk("stored_payload_past_eof_nonfinal", Builder().fixed(list(t[:20])).stored(t[20:120]).fixed([1], final=True),
                 cut=(3 + 7 + 20 * 8 + 7) // 8 * 8 + 40 + 50 * 8, ok=False))
    cs.append(mk("nonfinal_ends_at_eof", Builder().stored(t[:10]), ok=False))
    cs.append(mk("nonfinal_dynamic_ends_at_eof", Builder().fixed(list(t[:10])).dynamic(list(t[10:200])), ok=False))
    return cs


def prefix_cases():
    """Every prefix of two small mixed streams (stored, fixed, dynamic, then a final stored block), cut at each bit
    (the rest of the last byte zero).  The final stored block has a payload in one, LEN 0 in the other.  A cut parses
    when every byte up to the last one the reference needs is intact: through NLEN (payload: its missing bytes read as
    0xff), through LEN for LEN 0 (a cut NLEN reads as 0xffff)."""
    cs = []
    t = bytes(text(500, 12))
    for tag, payload in (("payload", t[:23]), ("len0", b"")):
        b = mixed().stored(payload, final=True)
        full = b.getvalue()
        hdr_end = len(full) - len(payload)            # the byte after NLEN
        need = hdr_end if payload else hdr_end - 2    # bytes that must be intact
        pre = b.final_plain[:len(b.final_plain) - len(payload)]
        for cut in range(len(full) * 8 + 1):
            data = b.getvalue(cut)
            # NLEN bytes that are there are read as they are (partly zeroed by the cut); only a missing byte is EOF
            ok = len(data) >= need and data[:need] == full[:need] and (len(data) < hdr_end or data[:hdr_end] == full[:hdr_end])
            if ok:
                got = data[hdr_end:] if payload else b""
                cs.append(Case("prefix_%s_%d" % (tag, cut), data, True, pre + got + b"\xff" * (len(payload) - len(got)), len(data),
                               b.final_end))
            else:
                cs.append(Case("prefix_%s_%d" % (tag, cut), data, False))
    return cs


# ---- invalid input ----
def invalid_cases():
    cs = []
    t = list(text(300, 13))
    for k in range(3):
        b = Builder()
        for _ in range(k):
            b.fixed(t[:10])
        b.header(True, 3).bits(0, 16)
        cs.append(mk("btype3_block_%d" % k, b, ok=False))
    cs.append(mk("fixed_sym_286", Builder().fixed(t[:5] + [Raw(286)], final=True), ok=False))
    cs.append(mk("fixed_sym_287", Builder().fixed(t[:5] + [Raw(287)], final=True), ok=False))
    cs.append(mk("fixed_dist_30", Builder().fixed(t[:5] + [Raw(257, dsym=30)], final=True), ok=False))
    cs.append(mk("fixed_dist_31", Builder().fixed(t[:5] + [Raw(257, dsym=31)], final=True), ok=False))
    for d in (30, 31):
        cs.append(mk("dynamic_dist_%d" % d, Builder().dynamic(t[:40] + [Raw(258, dsym=d)], final=True, dist_lens=[1, 2] + [0] * 28 + [3, 3]),
                     ok=False))
    cs.append(mk("nlen_mismatch", Builder().stored(bytes(t[:9]), final=True, nlen=0xfff6 ^ 0x10), ok=False))
    cs.append(mk("len_larger_than_payload_nonfinal", Builder().stored(bytes(t[:9]), len_=40).fixed([], final=True), ok=False))
    return cs


# ---- decoys ----
def shifted(data, k):
    """`data` behind k junk bits (ones)"""
    v = (int.from_bytes(data, "little") << k) | ((1 << k) - 1)
    return v.to_bytes(len(data) + 1, "little")


def decoy_cases():
    cs = []
    t = bytes(text(60000, 14))
    inner = z(t[:20000]) + z(t[20000:26000], 6, zlib.Z_HUFFMAN_ONLY)
    for k in range(8):
        b = Builder().stored(shifted(inner, k)[:65535]).dynamic(list(t[:300]), final=True)
        cs.append(mk("decoy_stored_shift_%d" % k, b))
    return cs


def nested_decoys():
    """Three levels of raw deflate streams, each stored inside the next at its own bit shift, with real dynamic blocks
    at every level (~1.1 MiB).  Every level's dynamic blocks are decoys the scan confirms and the probes decode.

    The probes' chunk pool (d4g_host.h parse_probe) holds totalBytes * 8 / (64 * 512) + 2 * candidates * (threads / 64)
    + 64 records, and a probe takes threads / 64 records per batch of threads * 512 bits it decodes.  The decoys are bytes
    of the stream itself, so the confirmed blocks cover every input bit at most once, and each candidate brings two
    batches of slack: computed, the pool does NOT run out here (nor for any decoys inside stored blocks, unless false
    candidates decode more than two batches each), so the emit pass replays every recorded block.  Outputs are still
    checked exactly.
    """
    rng = random.Random(15)
    lvl = z(bytes(text(1 << 23, 16)))
    for depth in range(3):
        b = Builder()
        raw = shifted(lvl, 1 + 2 * depth)
        for i in range(0, len(raw), 65535):
            b.stored(raw[i:i + 65535])
            if rng.random() < 0.3:
                b.dynamic(text(3000, 100 + i))
        b.dynamic(text(50000, 200 + depth), final=True)
        lvl = b.getvalue()
        last = b
    return mk("nested_decoys_3", last, size="large")


_CACHE = {}


def cases(size=None):
    """the corpus (size None: small and large)"""
    if "small" not in _CACHE:
        _CACHE["small"] = header_cases() + code_cases() + token_cases() + block_cases() + end_cases() + invalid_cases() + decoy_cases()
    if size != "small" and "large" not in _CACHE:
        _CACHE["large"] = [c for c in _CACHE["small"] if c.size == "large"] + [nested_decoys()]
    if size is None:
        return [c for c in _CACHE["small"] if c.size == "small"] + _CACHE["large"]
    return _CACHE["large"] if size == "large" else [c for c in _CACHE["small"] if c.size == "small"]


def prefixes():
    if "prefix" not in _CACHE:
        _CACHE["prefix"] = prefix_cases()
    return _CACHE["prefix"]


def by_name(names):
    d = {c.name: c for c in cases()}
    return [d[n] for n in names]


# run under every executor / without memos / through the recompress loop
SUBSET = ["hlit_288", "hdist_32", "codes_11_to_15_bits", "oversubscribed_8bit_254_reachable", "dense_48bit_tokens",
          "len258_as_284_31_and_285", "stored_pair_65536", "dynamic_at_phase_5", "bfinal_on_middle_block",
          "zlib1_sync_then_stored_nlen_cut", "stored_payload_past_eof_final", "decoy_stored_shift_3", "zero_run_crosses_into_distances"]


# The level executor (D4G_EXEC=levels, which the default fused executor hands only what it and the cluster kernel cannot
# hold) stops with "phase1: chain lookup failed" on these tiny dynamic blocks: its
# round's starting size differs from the parsed block's.  Not fixed here; pinned by a strict xfail in the emulator test.
LEVEL_EXEC_BAD = ["run_ends_at_hlit_plus_hdist", "rep16_crosses_into_distances", "oversubscribed_eob_reachable",
                   "distance_across_fixed_stored_dyn", "empty_dynamic_final"]


# ---- the comparison ----
def compare(D, L, O, streams, merges=(True, False), abi=True):
    """Every stream of one batch against the oracle, merge on and off: status, saved bits, consumed bytes, the
    re-serialised output, the decoded bytes; then d4g_optimise_streams (output == oracle's when it changed, else the
    input kept by the caller), d4g_size_bits_fallback and d4g_inflate.  -> list of mismatch descriptions."""
    import abi_calls
    bad = []
    for merge in merges:
        b = D.Batch(streams, lib=L).run(merge)
        for i, a in enumerate(streams):
            rc, want, saved, consumed, _ = O.optimise(a, merge)
            r = b.result(i)
            got = (r["status"], r["saved_bits"], r["consumed"] if rc >= 0 else 0)
            exp = (rc, saved if rc == 0 else 0, consumed if rc >= 0 else 0)
            if got != exp:
                bad.append((i, merge, "result", got, exp))
                continue
            if rc >= 0:
                if b.output(i) != want:
                    bad.append((i, merge, "output"))
                dec, _ = O.inflate(a)
                if b.decoded(i) != dec:
                    bad.append((i, merge, "decoded"))
        b.close()
        if not abi or merge != merges[0]:    # (the one-shot entry point runs the same engine: one merge flag is enough)
            continue
        rc, res = abi_calls.optimise_streams(L, streams, merge)
        assert rc == 0
        for i, (a, (st, sv, data)) in enumerate(zip(streams, res)):
            orc, want, osaved, _, _ = O.optimise(a, merge)
            final = data if st == 0 else a
            if st != orc or final != (want if orc == 0 else a) or sv != (osaved if orc == 0 else 0):
                bad.append((i, merge, "optimise_streams", st, orc))
    if abi:
        for i, a in enumerate(streams):
            rc2, bits = abi_calls.size_bits_fallback(L, a)
            ob = O.size_bits(a)
            if rc2 != 0 or bits != (ob if ob >= 0 else len(a) * 8):
                bad.append((i, "size_bits_fallback", bits, ob))
            rc3, st3, dec, cons = abi_calls.inflate(L, a)
            odec, ocons = O.inflate(a)
            if rc3 != 0 or (st3 >= 0) != (odec is not None) or dec != odec or (odec is not None and cons != ocons):
                bad.append((i, "inflate", st3, cons, ocons))
    return bad


def compare_parse(D, L, O, streams):
    """DeflateStream.parse only (d4g_batch_parse): parse verdict, consumed bytes, size bits and decoded bytes of every
    stream of one batch against the oracle.  -> list of mismatch descriptions."""
    bad = []
    b = D.Batch(streams, lib=L).parse()
    for i, a in enumerate(streams):
        rc, _, _, consumed, _ = O.optimise(a, True)
        r = b.result(i)
        got = (r["status"] >= 0, r["consumed"] if rc >= 0 else 0, r["size_bits_in"] if rc >= 0 else -1)
        exp = (rc >= 0, consumed if rc >= 0 else 0, O.size_bits(a))
        if got != exp:
            bad.append((i, "parse", got, exp))
        elif rc >= 0 and b.decoded(i) != O.inflate(a)[0]:
            bad.append((i, "decoded"))
    b.close()
    return bad


def stored_after_huffman():
    """zlib level 1 of text, random bytes (zlib stores them) and text again: the optimiser shrinks the Huffman block
    in front of the stored block, which moves the stored block's padding"""
    rng = random.Random(17)
    raw = bytes(text(12000, 18)) + bytes(rng.randrange(256) for _ in range(3000)) + bytes(text(6000, 19))
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    out = bytearray()
    for i in range(0, len(raw), 5000):
        out += c.compress(raw[i:i + 5000]) + c.flush(zlib.Z_FULL_FLUSH)
    return bytes(out + c.flush())
