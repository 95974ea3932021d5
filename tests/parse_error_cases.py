"""Raw DEFLATE streams that do not parse, each with the failure a sequential decoder stops at, by construction: which
block, where that block starts, the first bit of the element that fails, the bytes decoded before it, and the offending
value.  Shared by the emulator and the GPU tests of d4g_batch_parse_error / d4g_diagnose_streams.

Every expected value comes from the builder: `Track` wraps deflate_builder.Builder, counts the decoded bytes of the
tokens it appends and notes where every element starts; `here()` is taken just before the offending element goes in.
Nothing is taken from the library, the emulator or the oracle.

Where the input ends inside an element (EOF) the reported bit is the first bit of the field that could not be read in
full: the 3 header bits, LEN or NLEN, the 14 count bits, one 3-bit code-length entry, a Huffman code, an extra-bit
field.  Streams are whole bytes, so an EOF cut is made at a byte boundary that lies strictly inside the chosen field:
a prefix of a Huffman code is never a code, so nothing else can be read from the bits that remain.

Chunk geometry: the token decoder cuts a block's bits into chunks of CHUNK bits, counted from the block's first token;
`lanes` chunks side by side are one batch (the workgroup size: 512 on the GPU, 64 or 128 in the emulator tests)."""
import random
import zlib

import deflate_builder as DB
import handbuilt_cases as H
from deflate_builder import Builder, Raw, Ref

OK, EOF, BLOCK_TYPE, STORED_LENGTHS, CODE_LENGTHS, LITLEN_SYMBOL, DIST_SYMBOL, DISTANCE_TOO_FAR = range(8)   # D4G_PARSE_*
NAMES = ["OK", "EOF", "BLOCK_TYPE", "STORED_LENGTHS", "CODE_LENGTHS", "LITLEN_SYMBOL", "DIST_SYMBOL", "DISTANCE_TOO_FAR"]
FIELDS = ("reason", "block", "block_bit_pos", "bit_pos", "decoded_offset", "value")
NONE = dict(reason=OK, block=-1, block_bit_pos=-1, bit_pos=-1, decoded_offset=-1, value=-1)
CHUNK = 512            # D4G_CHUNK_BITS
WINDOW_BITS = 33040 * 8   # the staged input window (D4G_INCH + 16 bytes): a block longer than this is staged again


class PE:
    def __init__(self, name, data, reason, at=None, value=-1, rfc_before=True):
        self.name, self.data = name, bytes(data)
        self.rfc_before = rfc_before       # everything before the failure is RFC 1951: zlib gets as far as the library
        self.want = dict(NONE) if reason == OK else dict(reason=reason, block=at["block"], block_bit_pos=at["block_bit_pos"],
                                                          bit_pos=at["bit_pos"], decoded_offset=at["decoded_offset"], value=value)

    def __repr__(self):
        return "PE(%s)" % self.name


class Track:
    """A Builder that knows where it is: the current block and its first bit, the bytes decoded so far, and the span
    (kind, start, end, decoded bytes before the token) of every element written through it."""

    def __init__(self):
        self.b = Builder()
        self.dec = 0
        self.block = -1
        self.block_pos = 0
        self.spans = []

    @property
    def nbits(self):
        return self.b.nbits

    def here(self, bit_pos=None):
        return dict(block=self.block, block_bit_pos=self.block_pos, bit_pos=self.b.nbits if bit_pos is None else bit_pos,
                    decoded_offset=self.dec)

    def next_block(self):
        """the position a block would start at (nothing is written)"""
        return dict(block=self.block + 1, block_bit_pos=self.b.nbits, bit_pos=self.b.nbits, decoded_offset=self.dec)

    def _span(self, kind, start):
        self.spans.append(dict(kind=kind, start=start, end=self.b.nbits, block=self.block, block_bit_pos=self.block_pos,
                               decoded_offset=self.dec))

    def begin(self, final, btype):
        self.block += 1
        self.block_pos = p = self.b.nbits
        self.b.header(final, btype)
        self._span("header", p)
        return self

    def tokens(self, toks, ll, dl):
        lc, dc = DB.canonical(ll), DB.canonical(dl)
        b = self.b
        for t in toks:
            p = b.nbits
            if isinstance(t, int):
                b.code(lc[t], ll[t])
                self._span("lit", p)
                self.dec += 1
            elif isinstance(t, Ref):
                s, e, ne = DB.len_symbol(t.length, t.use284)
                b.code(lc[s], ll[s])
                self._span("lencode", p)
                p = b.nbits
                b.bits(e, ne)
                if ne:
                    self._span("lenextra", p)
                d, de, nde = DB.dist_symbol(t.dist)
                p = b.nbits
                b.code(dc[d], dl[d])
                self._span("distcode", p)
                p = b.nbits
                b.bits(de, nde)
                if nde:
                    self._span("distextra", p)
                self.dec += t.length
            else:
                b.code(lc[t.sym], ll[t.sym]).bits(t.extra, t.nextra)
                if t.dsym is not None:
                    b.code(dc[t.dsym], dl[t.dsym]).bits(t.dextra, t.ndextra)
        return self

    def eob(self, ll):
        self.b.code(DB.canonical(ll)[256], ll[256])
        return self

    def fixed(self, toks, final=False, eob=True):
        self.begin(final, 1).tokens(toks, DB.FIXED_LIT, DB.FIXED_DIST)
        return self.eob(DB.FIXED_LIT) if eob else self

    def stored(self, data, final=False, len_=None, nlen=None):
        data = bytes(data)
        ln = len(data) if len_ is None else len_
        self.begin(final, 0)
        self.b.align()
        self.len_pos = self.b.nbits
        self.b.bits(ln, 16).bits((~ln) & 0xffff if nlen is None else nlen, 16)
        self.b.buf += data
        self.dec += ln
        return self

    def dyn_header(self, final, ll, dl, cl_syms=None, cl_lens=None):
        """HLIT = len(ll), HDIST = len(dl), HCLEN = 19, every field written here so that every position is known"""
        if cl_syms is None:
            cl_syms = DB.rle_lengths(list(ll) + list(dl))
        if cl_lens is None:
            cf = [0] * 19
            for s, _ in cl_syms:
                cf[s] += 1
            cl_lens = DB.limited_lengths(cf, 7)
            if sum(1 for x in cl_lens if x) == 1:
                cl_lens[0 if cl_lens[0] == 0 else 1] = 1
        b = self.b
        self.begin(final, 2)
        p = b.nbits
        b.bits(len(ll) - 257, 5).bits(len(dl) - 1, 5).bits(15, 4)
        self._span("counts", p)
        for i in range(19):
            p = b.nbits
            b.bits(cl_lens[DB.CL_ORDER[i]], 3)
            self._span("clentry", p)
        cc = DB.canonical(cl_lens)
        for s, rep in cl_syms:
            p = b.nbits
            b.code(cc[s], cl_lens[s])
            self._span("clsym", p)
            p = b.nbits
            if s == 16:
                b.bits(rep - 3, 2)
            elif s == 17:
                b.bits(rep - 3, 3)
            elif s == 18:
                b.bits(rep - 11, 7)
            if s >= 16:
                self._span("clextra", p)
        return self

    def dynamic(self, toks, final=False, eob=True, ll=None, dl=None, extra=()):
        if ll is None:
            ll, dl = auto_lens(list(toks) + list(extra))
        self.dyn_header(final, ll, dl).tokens(toks, ll, dl)
        return self.eob(ll) if eob else self

    def fill_to(self, bit, rng):
        """fixed-code literals (8 bits below 144, 9 bits from 144; about half the bits in each) up to exactly `bit`"""
        delta = bit - self.b.nbits
        nine = delta % 8
        nine += 8 * max(0, (delta - 9 * nine) // 144)
        eight = (delta - 9 * nine) // 8
        assert eight >= 0
        toks = [rng.randrange(144) for _ in range(eight)] + [144 + rng.randrange(112) for _ in range(nine)]
        rng.shuffle(toks)
        self.tokens(toks, DB.FIXED_LIT, DB.FIXED_DIST)
        assert self.b.nbits == bit
        return self

    def value(self, cut=None):
        return self.b.getvalue(cut)


def auto_lens(tokens):
    """optimal code lengths of the tokens plus an end-of-block symbol (what Builder.dynamic chooses)"""
    lf, df = [0] * 286, [0] * 32
    bb = Builder()
    for t in tokens:
        s, d = bb._syms(t)
        lf[s] += 1
        if d is not None:
            df[d] += 1
    lf[256] += 1
    ll = DB.limited_lengths(lf, 15)
    while len(ll) > 257 and ll[-1] == 0:
        ll.pop()
    dl = DB.limited_lengths(df, 15)
    if sum(1 for x in dl if x) == 1 and dl.index(1) < 29:
        dl[dl.index(1) + 1] = 1
    while len(dl) > 1 and dl[-1] == 0:
        dl.pop()
    return ll, dl


def text(n, seed):
    return H.text(n, seed)


# ---- one per reason, block 0, first chunk ----
def reason_cases():
    cs = []
    t = list(text(300, 13))
    hb = {c.name: c.data for c in H.invalid_cases()}
    for k in range(3):                                   # BTYPE 3 behind 0, 1 and 2 fixed blocks
        tr = Track()
        for _ in range(k):
            tr.fixed(t[:10])
        at = tr.next_block()
        tr.b.header(True, 3).bits(0, 16)
        cs.append(PE("btype3_block_%d" % k, tr.value(), BLOCK_TYPE, at, 3))
    for sym in (286, 287):
        tr = Track().fixed(t[:5], final=True, eob=False)
        at = tr.here()
        tr.tokens([Raw(sym)], DB.FIXED_LIT, DB.FIXED_DIST).eob(DB.FIXED_LIT)
        cs.append(PE("fixed_sym_%d" % sym, tr.value(), LITLEN_SYMBOL, at, sym))
    for d in (30, 31):
        tr = Track().fixed(t[:5], final=True, eob=False)
        at = tr.here()
        tr.tokens([Raw(257, dsym=d)], DB.FIXED_LIT, DB.FIXED_DIST).eob(DB.FIXED_LIT)
        cs.append(PE("fixed_dist_%d" % d, tr.value(), DIST_SYMBOL, at, d))
    for d in (30, 31):
        ll, _ = auto_lens(t[:40] + [Raw(258, dsym=d)])
        dl = [1, 2] + [0] * 28 + [3, 3]
        # (Builder.dynamic trims HCLEN as handbuilt_cases does; the header depends on the code lengths alone, so the block
        # without its last token ends where that token starts)
        pos = Builder().dynamic(t[:40], final=True, lit_lens=ll, dist_lens=dl, eob=False).nbits
        full = Builder().dynamic(t[:40] + [Raw(258, dsym=d)], final=True, lit_lens=ll, dist_lens=dl)
        cs.append(PE("dynamic_dist_%d" % d, full.getvalue(), DIST_SYMBOL, dict(block=0, block_bit_pos=0, bit_pos=pos, decoded_offset=40), d))
    tr = Track().stored(bytes(t[:9]), final=True, nlen=0xfff6 ^ 0x10)
    cs.append(PE("nlen_mismatch", tr.value(), STORED_LENGTHS, dict(block=0, block_bit_pos=0, bit_pos=tr.len_pos, decoded_offset=0), 9))
    tr = Track().stored(bytes(t[:9]), len_=40).fixed([], final=True)
    end = len(tr.value()) * 8                            # LEN 40 > the 11 bytes that follow: the block ends the input
    cs.append(PE("len_larger_than_payload_nonfinal", tr.value(), EOF, dict(block=1, block_bit_pos=end, bit_pos=end, decoded_offset=40)))
    for c in cs:                                         # the same streams as handbuilt_cases.invalid_cases()
        if c.name in hb:
            assert c.data == hb[c.name], c.name
    # a 16 as the first code-length symbol; a run that overshoots HLIT + HDIST
    cl = [0] * 19
    cl[16], cl[18], cl[2] = 2, 1, 2
    ll = H.expand([(18, 97), (2, None), (2, None), (18, 138), (18, 19), (2, None)])
    tr = Track().dyn_header(True, ll, [2, 2], cl_syms=[], cl_lens=cl)
    at = tr.here()
    tr.b.code(DB.canonical(cl)[16], 2).bits(0, 2).bits(0, 64)
    cs.append(PE("rep16_first", tr.value(), CODE_LENGTHS, at, 16))
    tr = Track().dyn_header(True, ll, [2, 2], cl_syms=[(18, 97), (2, None), (2, None), (18, 138), (18, 19), (2, None)], cl_lens=cl)
    at = tr.here()                                       # 257 lengths written; a 16 x 6 would make 263 > 257 + 2
    tr.b.code(DB.canonical(cl)[16], 2).bits(3, 2).bits(0, 64)
    cs.append(PE("run_overshoots", tr.value(), CODE_LENGTHS, at, 16))
    # an incomplete code-length code (lengths 1, 2 -> the pattern 11 is no code), with plenty of input left
    cl = [0] * 19
    cl[18], cl[2] = 1, 2
    tr = Track().dyn_header(True, ll, [2, 2], cl_syms=[(18, 97), (2, None)], cl_lens=cl)
    at = tr.here()
    tr.b.bits(3, 2).bits(0, 64)
    cs.append(PE("no_code_length_code", tr.value(), CODE_LENGTHS, at, -1))
    # distances
    tr = Track().begin(True, 1)
    at = tr.here()
    tr.tokens([Ref(3, 1)], DB.FIXED_LIT, DB.FIXED_DIST).eob(DB.FIXED_LIT)
    cs.append(PE("distance_1_first_token", tr.value(), DISTANCE_TOO_FAR, at, 1))
    tr = Track().fixed(t[:7], final=True, eob=False)
    at = tr.here()
    tr.tokens([Ref(4, 8)], DB.FIXED_LIT, DB.FIXED_DIST).eob(DB.FIXED_LIT)
    cs.append(PE("distance_k_plus_1", tr.value(), DISTANCE_TOO_FAR, at, 8))
    tr = Track().fixed(t[:7] + [Ref(4, 7)], final=True)
    cs.append(PE("distance_k_ok", tr.value(), OK))
    # no literal/length code and no distance code match (incomplete codes), with plenty of input left
    ll = [0] * 257
    ll[97], ll[98], ll[256], ll[0] = 2, 2, 2, 0          # 00, 01, 10 used; 11 is no code
    tr = Track().dyn_header(True, ll, [0]).tokens([97, 98, 98], ll, [0])
    at = tr.here()
    tr.b.bits(3, 2).bits(0, 64)
    cs.append(PE("no_litlen_code", tr.value(), LITLEN_SYMBOL, at, -1))
    ll, _ = auto_lens(t[:20] + [Ref(3, 1)])
    dl = [2, 2, 2]                                       # 00, 01, 10 used; 11 is no code
    tr = Track().dyn_header(True, ll, dl).tokens(t[:20], ll, dl)
    at = tr.here()
    tr.b.code(DB.canonical(ll)[257], ll[257]).bits(3, 2).bits(0, 64)
    cs.append(PE("no_dist_code", tr.value(), DIST_SYMBOL, at, -1))
    return cs


# ---- the input ends inside an element ----
def eof_stream():
    """a valid two-block dynamic stream; block 0 ends on a byte boundary"""
    rng = random.Random(21)
    for extra in range(64):
        t = list(text(260 + extra, 22))
        toks = []
        for i, c in enumerate(t):
            toks.append(c)
            if i % 9 == 8 and i > 40:
                toks.append(Ref(11 + rng.randrange(100), 5 + rng.randrange(i - 5)))
        tr = Track().dynamic(toks)
        if tr.nbits % 8 == 0:
            break
    else:
        raise AssertionError("no block 0 that ends on a byte boundary")
    end0 = dict(tr.next_block())
    tr.dynamic(list(text(50, 23)) + [Ref(20, 30)], final=True)
    assert zlib.decompressobj(-15).decompress(tr.value()) is not None
    return tr, end0


def eof_cases():
    cs = [PE("empty_input", b"", EOF, dict(block=0, block_bit_pos=0, bit_pos=0, decoded_offset=0))]
    tr, end0 = eof_stream()
    for kind in ("counts", "clentry", "clextra", "lit", "lencode", "lenextra", "distcode", "distextra"):
        for s in tr.spans:
            cut = (s["start"] // 8 + 1) * 8
            if s["kind"] == kind and s["block"] == 0 and cut < s["end"]:
                break
        else:
            raise AssertionError("no %s element across a byte boundary" % kind)
        cs.append(PE("eof_in_" + kind, tr.value(cut), EOF, dict(s, bit_pos=s["start"])))
    cs.append(PE("eof_at_end_of_nonfinal_block", tr.value(end0["bit_pos"]), EOF, end0))
    # inside the 3 header bits: a block 1 whose header starts 2 bits before a byte boundary
    rng = random.Random(24)
    t2 = Track().begin(False, 1).fill_to(199, rng).eob(DB.FIXED_LIT)     # 199 + 7 bits of end-of-block
    assert t2.nbits % 8 == 6
    at = t2.next_block()
    t2.fixed([rng.randrange(256)], final=True)
    cs.append(PE("eof_in_header_bits", t2.value(at["bit_pos"] + 2), EOF, at))
    # a stored block whose LEN / NLEN the input no longer holds
    t3 = Track().fixed(list(text(10, 26)))
    t3.stored(b"abc", final=True)
    at = dict(block=1, block_bit_pos=t3.block_pos, decoded_offset=10)
    cs.append(PE("eof_in_stored_len", t3.value(t3.len_pos + 8), EOF, dict(at, bit_pos=t3.len_pos)))
    cs.append(PE("eof_in_stored_nlen", t3.value(t3.len_pos + 24), EOF, dict(at, bit_pos=t3.len_pos + 16)))
    return cs


# ---- chunk geometry ----
def fixed_block_with(lanes, events, name, first, seed):
    """One final fixed block of literals with events [(bit offset from the block's first token, token)]; `first` is
    the index of the event a sequential decoder stops at."""
    rng = random.Random(seed)
    tr = Track().begin(True, 1)
    t0 = tr.nbits
    at = None
    for k, (off, tok) in enumerate(events):
        tr.fill_to(t0 + off, rng)
        if k == first:
            at = tr.here()
        tr.tokens([tok], DB.FIXED_LIT, DB.FIXED_DIST)
    tr.tokens([rng.randrange(256) for _ in range(40)], DB.FIXED_LIT, DB.FIXED_DIST).eob(DB.FIXED_LIT)
    tok = events[first][1]
    if isinstance(tok, Ref):
        return PE(name, tr.value(), DISTANCE_TOO_FAR, at, tok.dist)
    return PE(name, tr.value(), LITLEN_SYMBOL, at, tok.sym)


def geometry_cases(lanes):
    """`lanes` chunks make a batch (the decoder's workgroup size)"""
    bad, far = Raw(286), Ref(3, 32768)                   # (a fixed block of under 32768 literals never has that much history)
    batch = lanes * CHUNK
    cs = [
        fixed_block_with(lanes, [(CHUNK - 1, bad)], "bad_symbol_last_bit_of_chunk_0", 0, 31),
        fixed_block_with(lanes, [(CHUNK - 4, bad)], "bad_symbol_across_stream_bit_512", 0, 32),      # tokens start at bit 3
        fixed_block_with(lanes, [(5 * CHUNK + 100, bad)], "bad_symbol_in_chunk_5", 0, 33),
        fixed_block_with(lanes, [(batch - CHUNK + 77, bad)], "bad_symbol_in_last_chunk_of_batch_0", 0, 34),
        fixed_block_with(lanes, [(batch + 2 * CHUNK + 5, bad)], "bad_symbol_in_batch_1", 0, 35),
        fixed_block_with(lanes, [(max(WINDOW_BITS, batch) + 3 * CHUNK + 9, bad)], "bad_symbol_past_a_restaging", 0, 36),
        fixed_block_with(lanes, [(CHUNK + 50, far), (7 * CHUNK + 60, bad)], "far_chunk_1_then_bad_chunk_7", 0, 37),
        fixed_block_with(lanes, [(CHUNK + 50, bad), (7 * CHUNK + 60, far)], "bad_chunk_1_then_far_chunk_7", 0, 38),
        fixed_block_with(lanes, [(batch - CHUNK + 50, far), (batch + CHUNK + 60, bad)], "far_batch_0_then_bad_batch_1", 0, 39),
        fixed_block_with(lanes, [(batch - CHUNK + 50, bad), (batch + CHUNK + 60, far)], "bad_batch_0_then_far_batch_1", 0, 40),
        fixed_block_with(lanes, [(3 * CHUNK + 200, far), (3 * CHUNK + 300, bad)], "far_then_bad_in_one_chunk", 0, 41),
    ]
    assert cs[1].want["bit_pos"] + 8 > 512 > cs[1].want["bit_pos"]
    return cs


# ---- history and preceding blocks ----
def history_cases():
    t = list(text(400, 42))
    cs = []
    for dist, ok in ((170, True), (171, False)):         # block 2 reaches into block 0 / one byte before the stream
        tr = Track().fixed(t[:100]).fixed(t[100:150]).begin(True, 1).tokens(t[150:170], DB.FIXED_LIT, DB.FIXED_DIST)
        at = tr.here()
        tr.tokens([Ref(5, dist)], DB.FIXED_LIT, DB.FIXED_DIST).eob(DB.FIXED_LIT)
        cs.append(PE("distance_%d_in_block_2" % dist, tr.value(), OK if ok else DISTANCE_TOO_FAR, at, dist))
    return cs


def preceding_cases():
    t = list(text(3000, 43))
    ll = [0] * 257
    ll[ord("a")] = ll[ord("b")] = ll[256] = 2            # an incomplete code: the header scan passes over such a block

    def lead(kind):
        tr = Track()
        if kind == "stored":
            tr.fixed(t[:3]).stored(bytes(t[3:40]))
        elif kind == "fixed":
            tr.fixed(t[:33])
        elif kind == "dynamic":
            tr.dynamic(t[:500])
        else:                                            # a block the scan finds, then one only the exact probe finds
            tr.dynamic(t[:2000]).dyn_header(False, ll, [0]).tokens(list(b"abba" * 20), ll, [0]).eob(ll)
        return tr
    cs = []
    for kind in ("stored", "fixed", "dynamic", "scan_and_exact"):
        tr = lead(kind).begin(True, 1).tokens(t[:25], DB.FIXED_LIT, DB.FIXED_DIST)
        at = tr.here()
        tr.tokens([Raw(287)], DB.FIXED_LIT, DB.FIXED_DIST).eob(DB.FIXED_LIT)
        rfc = kind != "scan_and_exact"                   # (zlib refuses the incomplete code of the block in front)
        cs.append(PE("bad_symbol_behind_" + kind, tr.value(), LITLEN_SYMBOL, at, 287, rfc))
        tr = lead(kind)
        at = tr.next_block()
        tr.b.header(False, 3).bits(0, 32)
        cs.append(PE("btype3_behind_" + kind, tr.value(), BLOCK_TYPE, at, 3, rfc))
        tr = lead(kind).stored(b"xyz", final=True, nlen=0x1234)
        cs.append(PE("nlen_mismatch_behind_" + kind, tr.value(), STORED_LENGTHS,
                     dict(block=tr.block, block_bit_pos=tr.block_pos, bit_pos=tr.len_pos, decoded_offset=tr.dec - 3), 3, rfc))
    return cs


_CACHE = {}


def cases(lanes):
    """every case with exact expected values, for a decoder of `lanes` threads"""
    if "base" not in _CACHE:
        _CACHE["base"] = reason_cases() + eof_cases() + history_cases() + preceding_cases()
    if lanes not in _CACHE:
        _CACHE[lanes] = _CACHE["base"] + geometry_cases(lanes)
        names = [c.name for c in _CACHE[lanes]]
        assert len(set(names)) == len(names)
    return _CACHE[lanes]


def by_name(lanes, names):
    d = {c.name: c for c in cases(lanes)}
    return [d[n] for n in names]


ZLIB_SAYS = {BLOCK_TYPE: "invalid block type", STORED_LENGTHS: "invalid stored block lengths", DISTANCE_TOO_FAR: "invalid distance too far back"}


def zlib_error(data):
    try:
        zlib.decompressobj(-15).decompress(data)
    except zlib.error as e:
        return str(e)
    return None


def valid_streams(max_len=None):
    """every valid stream the tests already have: the golden inputs and the hand-built corpus"""
    import glob
    import os
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = [(os.path.basename(p), open(p, "rb").read()) for p in sorted(glob.glob(os.path.join(g, "*.in.deflate")))]
    out += [(c.name, c.data) for c in H.cases("small" if max_len else None) if c.ok]
    return [(n, d) for n, d in out if max_len is None or len(d) <= max_len]


def mixed_batch(lanes):
    """12 streams, 5 of them failing for different reasons, between valid ones -> (cases, the valid streams alone)"""
    bad = by_name(lanes, ["btype3_block_1", "nlen_mismatch", "run_overshoots", "bad_symbol_in_chunk_5", "distance_171_in_block_2"])
    t = bytes(text(30000, 44))
    good = [H.z(t[:9000]), H.z(t[9000:12000], 1), H.z(t[:20000], 6), Track().fixed(list(t[:50]), final=True).value(),
            H.z(t[12000:30000], 9, zlib.Z_FILTERED), Track().stored(t[:300], final=True).value(), H.z(t[5000:7000], 3)]
    order = [good[0], bad[0], good[1], bad[1], bad[2], good[2], good[3], bad[3], good[4], good[5], bad[4], good[6]]
    return [x if isinstance(x, PE) else PE("valid_%d" % i, x, OK) for i, x in enumerate(order)], good


def png_with_bad_idat():
    """A PNG whose IDAT stream has one Huffman symbol overwritten (literal/length symbol 287 in place of a literal)
    -> (file bytes, the expected record of the IDAT stream)"""
    import struct
    t = list(text(200, 45))
    tr = Track().fixed(t[:100], final=True, eob=False)
    at = tr.here()
    tr.tokens([Raw(287)] + t[101:200], DB.FIXED_LIT, DB.FIXED_DIST).eob(DB.FIXED_LIT)
    zl = b"\x78\x9c" + tr.value() + struct.pack(">I", zlib.adler32(bytes(t)))

    def chunk(ty, data):
        return struct.pack(">I", len(data)) + ty + data + struct.pack(">I", zlib.crc32(ty + data))
    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 10, 19, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zl) + chunk(b"IEND", b"")
    return png, PE("png_idat", tr.value(), LITLEN_SYMBOL, at, 287).want


def golden_file(stem):
    """a golden container file, its optimised output and its transcript -> (in, out, lines, merge_blocks)"""
    import json
    import os
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    f = [x for x in json.load(open(os.path.join(g, "manifest.json")))["files"] if x["stem"] == stem][0]
    rd = lambda n: open(os.path.join(g, n), "rb").read()   # noqa: E731
    return rd(stem + ".file.in"), rd(stem + ".file.out"), f["transcript"], f["merge_blocks"]
