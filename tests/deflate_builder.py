"""Test-only bit-level raw DEFLATE writer (RFC 1951), for streams no encoder writes on its own.

Every header field is written as given: BFINAL / BTYPE, HLIT / HDIST / HCLEN verbatim (so 287, 288, 31, 32 can be
set), the code-length-code lengths, the code-length symbols with their repeat counts (runs may cross from the
literal/length lengths into the distance lengths, or overshoot), literal/length and distance code lengths that need not
be complete, stored blocks with any LEN / NLEN / padding bits.  Tokens may pick code 284 + 31 or code 285 for length
258, or name raw symbols (286/287, distance codes 30/31).  A stream can be cut at any bit and trailing bytes appended.

The builder also tracks the bytes it means to encode (`plain`), so RFC-valid streams can be checked against
zlib.decompress(stream, -15)."""
import collections
import heapq

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EBITS = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EBITS = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def len_symbol(length, use284=False):
    """-> (symbol, extra value, extra bits) of a match length; 258 is code 285 unless use284 (284 + 31)."""
    if length == 258 and use284:
        return 284, 31, 5
    for s in range(28, -1, -1):
        if LEN_BASE[s] <= length and (s != 28 or length == 258):
            return 257 + s, length - LEN_BASE[s], LEN_EBITS[s]
    raise ValueError(length)


def dist_symbol(dist):
    for s in range(29, -1, -1):
        if DIST_BASE[s] <= dist:
            return s, dist - DIST_BASE[s], DIST_EBITS[s]
    raise ValueError(dist)


def canonical(lengths):
    """RFC 1951 3.2.2 codes (== Huffman.buildCodes of the reference for any lengths); None for unused symbols and for
    the codes of an oversubscribed table that do not fit their length."""
    count = collections.Counter(l for l in lengths if l)
    nxt, code = {}, 0
    for l in range(1, 16):
        code = (code + count.get(l - 1, 0)) << 1 if l > 1 else 0
        nxt[l] = code
    out = []
    for l in lengths:
        if not l:
            out.append(None)
            continue
        c = nxt[l]
        nxt[l] += 1
        out.append(c if c < (1 << l) else None)
    return out


def kraft(lengths):
    """sum 2^-len as a fraction of 2^15: 32768 == complete, less == incomplete, more == oversubscribed"""
    return sum(1 << (15 - l) for l in lengths if l)


def limited_lengths(freq, limit):
    """Optimal length-limited Huffman code lengths (package-merge).  One used symbol gets length 1."""
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    out = [0] * len(freq)
    if not used:
        return out
    if len(used) == 1:
        out[used[0][1]] = 1
        return out
    assert len(used) <= 1 << limit
    leaves = [(f, (s,)) for f, s in used]
    cur = leaves
    for _ in range(limit - 1):
        pk = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = list(heapq.merge(leaves, pk, key=lambda x: x[0]))
    for _, syms in cur[:2 * (len(used) - 1)]:
        for s in syms:
            out[s] += 1
    return out


def rle_lengths(lens, use16=True, use17=True, use18=True):
    """Code-length symbols (sym, repeat count or None) for a run of lengths, zlib send_tree style."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, j = lens[i], i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and (use17 or use18):
            while run >= 11 and use18:
                k = min(run, 138)
                out.append((18, k))
                run -= k
            while run >= 3 and use17:
                k = min(run, 10)
                out.append((17, k))
                run -= k
            out += [(0, None)] * run
        else:
            out.append((v, None))
            run -= 1
            while run >= 3 and use16:
                k = min(run, 6)
                out.append((16, k))
                run -= k
            out += [(v, None)] * run
        i = j
    return out


class Lit:
    """A literal byte (only needed where a raw int would be ambiguous)."""
    def __init__(self, b):
        self.b = b


class Ref:
    """A back-reference; length 258 is sent as 284 + 31 when use284."""
    def __init__(self, length, dist, use284=False):
        self.length, self.dist, self.use284 = length, dist, use284


class Raw:
    """Raw symbols written as given: a literal/length symbol with its extra bits, optionally a distance symbol with
    its extra bits.  Marks the stream as not RFC-valid."""
    def __init__(self, sym, extra=0, nextra=0, dsym=None, dextra=0, ndextra=0):
        self.sym, self.extra, self.nextra, self.dsym, self.dextra, self.ndextra = sym, extra, nextra, dsym, dextra, ndextra


class Builder:
    def __init__(self):
        self.acc = 0            # pending bits, LSB first
        self.nacc = 0
        self.buf = bytearray()  # completed bytes
        self.plain = bytearray()
        self.valid = True       # False once something RFC 1951 forbids was written
        self.final_end = None   # bit position after the first block written with BFINAL
        self.final_plain = None  # the bytes decoded up to it

    # ---- bits ----
    @property
    def nbits(self):
        return len(self.buf) * 8 + self.nacc

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.nacc
        self.nacc += n
        while self.nacc >= 8:
            self.buf.append(self.acc & 0xff)
            self.acc >>= 8
            self.nacc -= 8
        return self

    def code(self, code, length):
        """a Huffman code: most significant bit first"""
        assert code is not None, "symbol has no code"
        r = 0
        for _ in range(length):
            r = (r << 1) | (code & 1)
            code >>= 1
        return self.bits(r, length)

    def align(self, pad=0):
        """pad to a byte boundary with the low bits of `pad` (nonzero padding is legal; decoders ignore it)"""
        k = (8 - self.nacc) % 8
        return self.bits(pad & ((1 << k) - 1), k)

    def header(self, final, btype):
        self.bits(1 if final else 0, 1).bits(btype, 2)
        if btype == 3:
            self.valid = False
        return self

    def _end(self, final):
        if final and self.final_end is None:
            self.final_end = self.nbits
            self.final_plain = bytes(self.plain)

    # ---- blocks ----
    def stored(self, data=b"", final=False, len_=None, nlen=None, pad=0):
        data = bytes(data)
        ln = len(data) if len_ is None else len_
        nl = (~ln) & 0xffff if nlen is None else nlen
        if nl != (~ln) & 0xffff or ln != len(data):
            self.valid = False
        self.header(final, 0).align(pad).bits(ln, 16).bits(nl, 16)
        self.buf += data                 # byte aligned here
        self.plain += data
        self._end(final)
        return self

    def fixed(self, tokens, final=False, eob=True):
        self.header(final, 1)
        self._tokens(tokens, FIXED_LIT, FIXED_DIST, eob)
        self._end(final)
        return self

    def dynamic(self, tokens, final=False, lit_lens=None, dist_lens=None, hlit=None, hdist=None, cl_syms=None,
                cl_lens=None, hclen=None, eob=True, rle="joint"):
        """A dynamic block.  Defaults: optimal 15-bit-limited codes of the tokens (HLIT >= 257, HDIST >= 1), one RLE
        sequence over both tables (rle="joint"; "split": per table, as zlib; "none": no 16/17/18), a 7-bit-limited
        code-length code, HCLEN trimmed to the last nonzero length (>= 4).  `hlit` / `hdist` / `hclen` override the
        counts written; `cl_syms` is a verbatim list of (symbol, repeat count or None)."""
        tokens = list(tokens)
        if lit_lens is None or dist_lens is None:
            lf, df = [0] * 288, [0] * 32
            for t in tokens:
                s, d = self._syms(t)
                lf[s] += 1
                if d is not None:
                    df[d] += 1
            if eob:
                lf[256] += 1
            if lit_lens is None:
                lit_lens = limited_lengths(lf, 15)
                while len(lit_lens) > 257 and lit_lens[-1] == 0:
                    lit_lens.pop()
            if dist_lens is None:
                dist_lens = limited_lengths(df, 15)
                if sum(1 for x in dist_lens if x) == 1 and dist_lens.index(1) < 29:
                    dist_lens[dist_lens.index(1) + 1] = 1     # two one-bit codes: complete, as zlib wants
                while len(dist_lens) > 1 and dist_lens[-1] == 0:
                    dist_lens.pop()
        nlit = len(lit_lens) if hlit is None else hlit
        ndist = len(dist_lens) if hdist is None else hdist
        if not (257 <= nlit <= 286 and 1 <= ndist <= 30):
            self.valid = False
        if cl_syms is None:
            lens = (list(lit_lens) + [0] * nlit)[:nlit] + (list(dist_lens) + [0] * ndist)[:ndist]
            if rle == "joint":
                cl_syms = rle_lengths(lens)
            elif rle == "split":
                cl_syms = rle_lengths(lens[:nlit]) + rle_lengths(lens[nlit:])
            else:
                cl_syms = [(v, None) for v in lens]
        if cl_lens is None:
            cf = [0] * 19
            for s, _ in cl_syms:
                cf[s] += 1
            cl_lens = limited_lengths(cf, 7)
            if sum(1 for x in cl_lens if x) == 1:
                cl_lens[0 if cl_lens[0] == 0 else 1] = 1   # one-symbol code-length code: zlib wants it complete
        if hclen is None:
            hclen = 19
            while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
                hclen -= 1
        def rfc_code(lens, dist):   # zlib: complete, or a single one-bit code (empty too, for distances)
            k, used = kraft(lens), sum(1 for x in lens if x)
            return k == 32768 or (used == 1 and k == 16384) or (dist and used == 0)
        if not (rfc_code(lit_lens[:nlit], False) and rfc_code(dist_lens[:ndist], True) and kraft(cl_lens) == 32768):
            self.valid = False
        self.header(final, 2).bits(nlit - 257, 5).bits(ndist - 1, 5).bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(cl_lens[CL_ORDER[i]], 3)
        ccodes = canonical(cl_lens)
        for s, rep in cl_syms:
            self.code(ccodes[s], cl_lens[s])
            if s == 16:
                self.bits(rep - 3, 2)
            elif s == 17:
                self.bits(rep - 3, 3)
            elif s == 18:
                self.bits(rep - 11, 7)
        self._tokens(tokens, lit_lens, dist_lens, eob)
        self._end(final)
        return self

    def _syms(self, t):
        if isinstance(t, int):
            return t, None
        if isinstance(t, Lit):
            return t.b, None
        if isinstance(t, Ref):
            return len_symbol(t.length, t.use284)[0], dist_symbol(t.dist)[0]
        return t.sym, t.dsym

    def _tokens(self, tokens, lit_lens, dist_lens, eob):
        lc, dc = canonical(lit_lens), canonical(dist_lens)
        ll = lambda s: lit_lens[s] if s < len(lit_lens) else 0            # noqa: E731
        dl = lambda s: dist_lens[s] if s < len(dist_lens) else 0          # noqa: E731
        for t in tokens:
            if isinstance(t, (int, Lit)):
                b = t if isinstance(t, int) else t.b
                self.code(lc[b], ll(b))
                self.plain.append(b)
            elif isinstance(t, Ref):
                s, e, ne = len_symbol(t.length, t.use284)
                self.code(lc[s], ll(s)).bits(e, ne)
                d, de, nde = dist_symbol(t.dist)
                self.code(dc[d], dl(d)).bits(de, nde)
                if t.dist > len(self.plain):
                    self.valid = False
                    self.plain += b"\0" * t.length
                else:
                    for _ in range(t.length):
                        self.plain.append(self.plain[-t.dist])
            else:
                self.code(lc[t.sym], ll(t.sym)).bits(t.extra, t.nextra)
                if t.dsym is not None:
                    self.code(dc[t.dsym], dl(t.dsym)).bits(t.dextra, t.ndextra)
                self.valid = False
        if eob:
            self.code(lc[256], ll(256))

    # ---- output ----
    def getvalue(self, cut=None, trailing=b""):
        """The stream, cut after `cut` bits (the rest of the last byte is zero) and followed by `trailing` bytes."""
        data = bytes(self.buf) + (bytes([self.acc]) if self.nacc else b"")
        if cut is not None:
            data = bytearray(data[:(cut + 7) // 8])
            if cut % 8:
                data[-1] &= (1 << (cut % 8)) - 1
            data = bytes(data)
        return data + bytes(trailing)
