"""Test-only restatement, in plain Python, of the two predicates by which the header scan (k_scan_headers,
deft4j_amd/csrc/d4g_parse.h) decides which bit positions of a raw DEFLATE stream are worth a probe.  Written from
RFC 1951 section 3.2.7 and the comments above the kernel; it is the reference of the scan tests, the library's own counts
never are.

A position p (bits are numbered LSB-first through the bytes) of a stream of `nbits` bits is

  a *candidate* when it reads as the start of a dynamic block whose code-length code is usable:
    bits p+1..p+2   BTYPE == 2 (BFINAL, bit p, is free)
    bits p+3..p+7   HLIT <= 29, bits p+8..p+12 HDIST <= 29
    bits p+13..p+16 HCLEN; the HCLEN + 4 three-bit lengths that follow end inside the stream (p + 17 + 3 * ncl <= nbits)
    those lengths form a complete prefix code (sum of 2^(7 - l) over the nonzero l == 128) of at least two codes;

  a *survivor* when, further, the HLIT + 257 + HDIST + 1 code lengths coded with that code (symbols 0..15, 16 = repeat
  the previous length 3..6 times, 17 / 18 = 3..10 / 11..138 zeros; one sequence over both tables) decode without
    a repeat before any length, a run past the last length, or a symbol that ends after the stream's last bit,
  and give a complete literal/length code that has the end-of-block symbol 256 and a distance code that is complete or has
  at most one code.  The walk gives up where fewer than 14 bits are left 64 bits after the stream's end
  (pos + 14 > nbits + 64): bits after the stream read as what lies there in memory, which is zero padding.
"""
import numpy as np

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
PAD = 32   # zero bytes after the stream: more than the 81-bit window and the walk's 64 + 14 bits can reach


def prolog_positions(data):
    """-> (bit array with padding, positions whose 13 prolog bits pass), for all positions of `data`"""
    raw = np.frombuffer(bytes(data) + bytes(PAD), dtype=np.uint8)
    bits = np.unpackbits(raw, bitorder="little")
    n = len(data) * 8
    if n == 0:
        return bits, np.zeros(0, dtype=np.int64)

    def field(off, width):
        v = np.zeros(n, dtype=np.int32)
        for k in range(width):
            v |= bits[off + k:off + k + n].astype(np.int32) << k
        return v
    ok = (field(1, 2) == 2) & (field(3, 5) <= 29) & (field(8, 5) <= 29)
    return bits, np.nonzero(ok)[0].astype(np.int64)


def candidates(data):
    """-> sorted bit positions that pass the prolog and the code-length code test"""
    bits, p = prolog_positions(data)
    n = len(data) * 8
    if len(p) == 0:
        return []
    ncl = 4 + sum(bits[p + 13 + k].astype(np.int64) << k for k in range(4))
    inside = p + 17 + 3 * ncl <= n
    p, ncl = p[inside], ncl[inside]
    kraft = np.zeros(len(p), dtype=np.int64)
    used = np.zeros(len(p), dtype=np.int64)
    for i in range(19):
        length = sum(bits[p + 17 + 3 * i + k].astype(np.int64) << k for k in range(3))
        length = np.where(i < ncl, length, 0)
        kraft += np.where(length > 0, 128 >> length, 0)
        used += length > 0
    return [int(x) for x in p[(kraft == 128) & (used >= 2)]]


class _Bits:
    def __init__(self, data):
        self.buf = bytes(data) + bytes(PAD)

    def get(self, pos, n):
        b = pos >> 3
        return (int.from_bytes(self.buf[b:b + 8], "little") >> (pos & 7)) & ((1 << n) - 1)


def survives(data, p):
    """the walk over the coded code lengths of candidate p (which must be one)"""
    rd = _Bits(data)
    nbits = len(data) * 8
    nlit = rd.get(p + 3, 5) + 257
    ndist = rd.get(p + 8, 5) + 1
    ncl = rd.get(p + 13, 4) + 4
    cl = [0] * 19
    for i in range(ncl):
        cl[CL_ORDER[i]] = rd.get(p + 17 + 3 * i, 3)
    pos = p + 17 + 3 * ncl
    # canonical codes (RFC 1951 3.2.2), keyed by (length, code read most significant bit first)
    count = [0] * 8
    for l in cl:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 8, 0
    for l in range(1, 8):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    table = {}
    for s, l in enumerate(cl):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    combined = nlit + ndist
    kraft_lit = kraft_dist = ndist_codes = 0
    eob = False
    i = prev = 0
    while i < combined:
        if pos + 14 > nbits + 64:
            return False
        code, sym = 0, None
        for l in range(1, 8):
            code = (code << 1) | rd.get(pos + l - 1, 1)
            if (l, code) in table:
                sym = table[(l, code)]
                pos += l
                break
        if sym is None:
            return False
        run, value = 1, sym
        if sym == 16:
            if i < 1:
                return False
            run, value = rd.get(pos, 2) + 3, prev
            pos += 2
        elif sym == 17:
            run, value = rd.get(pos, 3) + 3, 0
            pos += 3
        elif sym == 18:
            run, value = rd.get(pos, 7) + 11, 0
            pos += 7
        if pos > nbits or i + run > combined:
            return False
        if value:
            for j in range(i, i + run):
                if j < nlit:
                    kraft_lit += 1 << (15 - value)
                    eob = eob or j == 256
                else:
                    kraft_dist += 1 << (15 - value)
                    ndist_codes += 1
        prev = value
        i += run
    return kraft_lit == 1 << 15 and eob and (kraft_dist == 1 << 15 or ndist_codes <= 1)


def scan(data):
    """-> (candidates, survivors): sorted bit positions"""
    c = candidates(data)
    return c, [p for p in c if survives(data, p)]
