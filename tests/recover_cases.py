"""Damaged raw DEFLATE streams with the bytes a sequential decoder has produced when it meets the first failure, by
construction.  Shared by the emulator and the GPU tests of d4g_batch_recover / d4g_batch_copy_recovered /
d4g_recover_streams.  Nothing expected here comes from the library, the emulator or the oracle.

Truncation: valid streams of known plaintext (zlib at levels 1, 6 and 9; a hand-built stream of stored, fixed and dynamic
blocks) cut at byte boundaries.  The expected bytes are zlib's own: `zlib.decompressobj(-15).decompress(data[:cut])` emits
exactly the tokens that are complete, and they are a prefix of the plaintext.  Cuts inside a stored block's payload are
left out: there the library follows the reference (the missing bytes read as 0xff and the block parses), which is no part of
recovery.

Corruption: the where-and-why cases of parse_error_cases.py, rebuilt through `ByteTrack`, a Track that also keeps the
decoded bytes of the tokens appended through it (a literal is a byte, a Ref a copy out of its own output, stored data as
given).  A case's expected bytes are its track's bytes cut at the case's decoded_offset; the track of a case is found by
its bits: the one whose stream equals the case's up to the failing element."""
import zlib

import deflate_builder as DB
import handbuilt_cases as H
import parse_error_cases as P
from deflate_builder import Raw, Ref

INF = float("inf")


class ByteTrack(P.Track):
    live = None            # the tracks made while a case list is being built

    def __init__(self):
        super().__init__()
        self.out = bytearray()
        self.good = INF    # bytes of `out` that are what a decoder produces (a copy from before the stream has no bytes)
        if ByteTrack.live is not None:
            ByteTrack.live.append(self)

    def tokens(self, toks, ll, dl):
        toks = list(toks)
        super().tokens(toks, ll, dl)
        for t in toks:
            if isinstance(t, int):
                self.out.append(t)
            elif isinstance(t, Ref):
                if t.dist > len(self.out):
                    self.good = min(self.good, len(self.out))
                    self.out += bytes(t.length)
                else:
                    for _ in range(t.length):
                        self.out.append(self.out[-t.dist])
        return self

    def stored(self, data, final=False, len_=None, nlen=None):
        data = bytes(data)
        super().stored(data, final, len_, nlen)
        ln = len(data) if len_ is None else len_
        if ln != len(data):
            self.good = min(self.good, len(self.out))
        self.out += (data + bytes(ln))[:ln]
        return self


class RC:
    """one stream: its bytes, the expected parse_error record (`want`; truncations: reason and decoded_offset alone) and
    the expected recovered bytes"""

    def __init__(self, name, data, want, expected, plain=None):
        self.name, self.data, self.want, self.expected, self.plain = name, bytes(data), want, bytes(expected), plain
        assert want["reason"] == P.OK or len(self.expected) == want["decoded_offset"], name

    def __repr__(self):
        return "RC(%s)" % self.name


def _lowbits(data, n):
    return int.from_bytes(data[:(n + 7) // 8], "little") & ((1 << n) - 1)


def _with_tracks(build):
    """runs build() with parse_error_cases.Track replaced by ByteTrack -> (its result, the tracks it made)"""
    keep, ByteTrack.live = P.Track, []
    P.Track = ByteTrack
    try:
        res = build()
        return res, ByteTrack.live
    finally:
        P.Track = keep
        ByteTrack.live = None


def _expected(c, tracks, special):
    if c.want["reason"] == P.OK:
        return zlib.decompressobj(-15).decompress(c.data)
    n, bit = c.want["decoded_offset"], c.want["bit_pos"]
    if n == 0:
        return b""
    if c.name in special:
        return special[c.name]
    found = {bytes(t.out[:n]) for t, v in tracks
             if t.nbits >= bit and len(t.out) >= n and t.good >= n and _lowbits(v, bit) == _lowbits(c.data, bit)}
    assert len(found) == 1, (c.name, len(found))
    return found.pop()


def _overlap_and_reach_cases():
    """the last token before the failure is an overlapping copy; copies of the failing block reach into earlier blocks"""
    t = list(P.text(45000, 71))
    cs = []
    for name, ref in (("overlap_dist_1_len_258_last", Ref(258, 1)), ("overlap_dist_3_len_10_last", Ref(10, 3))):
        tr = P.Track().fixed(t[:20]).begin(True, 1).tokens(t[20:31] + [ref], DB.FIXED_LIT, DB.FIXED_DIST)
        at = tr.here()
        tr.tokens([Raw(286)] + t[31:40], DB.FIXED_LIT, DB.FIXED_DIST).eob(DB.FIXED_LIT)
        cs.append(P.PE(name, tr.value(), P.LITLEN_SYMBOL, at, 286))
    # six blocks of 7000 bytes (each a copy segment of its own), then a block whose copies reach 32768, 7001 and 5 bytes
    # back and which fails behind them: a prefix of more than 32 KiB plus an 8 KiB segment
    tr = P.Track()
    for k in range(6):
        tr.dynamic(t[7000 * k:7000 * (k + 1)])
    tail = t[42000:42040] + [Ref(100, 32768), Ref(30, 7001)] + t[42040:42050] + [Ref(12, 5), Ref(258, 32768)]
    tr.begin(True, 1).tokens(tail, DB.FIXED_LIT, DB.FIXED_DIST)
    at = tr.here()
    tr.tokens([Raw(257, dsym=31)] + t[42050:42060], DB.FIXED_LIT, DB.FIXED_DIST).eob(DB.FIXED_LIT)
    cs.append(P.PE("copies_reach_32768_across_segments", tr.value(), P.DIST_SYMBOL, at, 31))
    return cs


_CACHE = {}


def corruption_cases(lanes):
    """every case of parse_error_cases.cases(lanes), and the overlap / reach cases, with its expected bytes"""
    if lanes in _CACHE:
        return _CACHE[lanes]
    cs, tracks = _with_tracks(lambda: P.reason_cases() + P.eof_cases() + P.history_cases() + P.preceding_cases() +
                              P.geometry_cases(lanes) + _overlap_and_reach_cases())
    ref = {c.name: c for c in P.cases(lanes)}
    for c in cs:                                         # the same streams and records as the where-and-why tests use
        assert c.name not in ref or (ref[c.name].data == c.data and ref[c.name].want == c.want), c.name
    assert set(ref) <= {c.name for c in cs}
    tracks = [(t, t.value()) for t in tracks]
    lit40 = bytes(P.text(300, 13)[:40])                  # (built with Builder alone: 40 literals, then the bad distance code)
    special = {"dynamic_dist_30": lit40, "dynamic_dist_31": lit40}
    for c in cs:
        if c.name == "len_larger_than_payload_nonfinal":
            # LEN 40 with 11 bytes left: the block parses by the reference's rule (what follows LEN / NLEN at byte 5, then 0xff)
            special[c.name] = (c.data[5:] + b"\xff" * 40)[:40]
    out = [RC(c.name, c.data, c.want, _expected(c, tracks, special)) for c in cs]
    _CACHE[lanes] = out
    return out


def by_name(lanes, names):
    d = {c.name: c for c in corruption_cases(lanes)}
    return [d[n] for n in names]


def mixed_batch(lanes):
    """parse_error_cases.mixed_batch with expected bytes -> (cases, the valid streams alone)"""
    cs, good = P.mixed_batch(lanes)
    d = {c.name: c for c in corruption_cases(lanes)}
    return [d[c.name] if c.name in d else RC(c.name, c.data, c.want, zlib.decompressobj(-15).decompress(c.data)) for c in cs], good


# ---- truncation ----
def png_rows(width=96, rows=40, seed=5):
    """filtered image rows as a PNG encoder leaves them: a filter byte, then slowly varying samples"""
    import random
    rng = random.Random(seed)
    out = bytearray()
    for y in range(rows):
        out.append(y % 5)
        v = rng.randrange(256)
        for x in range(width * 3):
            v = (v + rng.choice((0, 0, 0, 1, 255, 2))) & 255
            out.append(v)
    return bytes(out)


def handbuilt_stream():
    """stored, fixed and dynamic blocks with copies across them -> (the ByteTrack that built it)"""
    t = list(P.text(1200, 81))
    tr = ByteTrack()
    tr.fixed(t[:60] + [Ref(20, 33), Ref(258, 1)] + t[60:90])
    tr.stored(bytes(t[90:150]))
    toks = []
    for i, c in enumerate(t[150:700]):
        toks.append(c)
        if i % 11 == 10:
            toks.append(Ref(3 + (i * 7) % 200, 1 + (i * 13) % (150 + i)))
    tr.dynamic(toks)
    tr.stored(bytes(t[700:720]))
    tr.fixed(t[720:760] + [Ref(40, 700)], final=True)
    return tr


def _cut_case(name, data, cut, plain):
    exp = zlib.decompressobj(-15).decompress(data[:cut])
    assert plain.startswith(exp), name
    return RC("%s_cut_%d" % (name, cut), data[:cut], dict(reason=P.EOF, decoded_offset=len(exp)), exp, plain)


def truncation_cases(n=6000):
    """valid streams cut short -> RC list (want: reason EOF and decoded_offset)"""
    if ("cut", n) in _CACHE:
        return _CACHE[("cut", n)]
    plains = {"text": bytes(H.text(n, 61)), "png": png_rows(rows=max(8, n // 289)), "run": b"\x07" * n + bytes(H.text(50, 62)) + b"ab" * (n // 4)}
    cs = []
    for pname, plain in sorted(plains.items()):
        for level in (1, 6, 9):
            data = H.z(plain, level)
            ln = len(data)
            for cut in sorted({1, 2, 3, ln // 4, ln // 2, 3 * ln // 4, ln - 6, ln - 1}):
                if 0 < cut < ln:
                    cs.append(_cut_case("%s_level_%d" % (pname, level), data, cut, plain))
    # the hand-built stream: a byte boundary strictly inside one element of every kind, in the first block that has one and
    # in the last; a stored block's LEN and NLEN; the end of every block that ends on a byte boundary
    tr = handbuilt_stream()
    data, plain = tr.value(), bytes(tr.out)
    assert zlib.decompressobj(-15).decompress(data) == plain
    cuts = set()
    for kind in ("header", "counts", "clentry", "clsym", "clextra", "lit", "lencode", "lenextra", "distcode", "distextra"):
        inside = [(s["start"] // 8 + 1) for s in tr.spans if s["kind"] == kind and (s["start"] // 8 + 1) * 8 < s["end"]]
        if kind not in ("header", "clsym"):
            assert inside, kind
        cuts.update(inside[:1] + inside[-1:])
    cuts.update({tr.len_pos // 8 + 1, tr.len_pos // 8 + 3})
    for cut in sorted(cuts):
        cs.append(_cut_case("handbuilt", data, cut, plain))
    _CACHE[("cut", n)] = cs
    return cs
