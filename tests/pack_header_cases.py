"""Inputs of d4g_debug_pack_header (rewriteHeader(flags) by one wave: d4g_wave_pack_header, the packer both search
executors call) and its comparison with the oracle, shared by the emulator test (test_pack_header_hostsim.py) and the
GPU test (test_gpu_pack_header.py).

The vectors are the smallest ones where the wave's run finder can go wrong: it looks at the combined code lengths in
chunks of 64, so runs are placed on, before and across the chunk borders, over whole chunks, across the border between
the literal/length and the distance lengths, and up to the last length."""
import ctypes

import abi_calls
import oracle_lib as O

NLIT, NDIST, MAXPAIRS = 288, 32, 320
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
F_OHH, F_USE8, F_USE7, F_ALT8, F_NOREP, F_NOZREP, F_NOZREP2, F_NOREPZEROS = 1, 2, 4, 8, 16, 32, 64, 128
F_DEFAULT = F_OHH | F_USE8 | F_USE7                      # DeflateBlockHuffman.rewriteHeader() :480-482
EXTRA = {16: 2, 17: 3, 18: 7}


def program_flag_sets():
    """The 56 (flags, prune) pairs of the header search in addOptimisedRecoded's loop order — DeflateStream.java:281-315"""
    out = []
    for no_rep_zeros in (0, 1):
        for prune in (0, 1):
            for no_rep in ((0,) if no_rep_zeros else (0, 1)):
                for no_zrep in ((1,) if no_rep_zeros else (0, 1)):
                    for no_zrep2 in (0, 1):
                        base = no_rep * F_NOREP | no_zrep * F_NOZREP | no_zrep2 * F_NOZREP2 | no_rep_zeros * F_NOREPZEROS
                        if not no_rep:
                            out += [(base | F_OHH | u8 * F_USE8 | u7 * F_USE7, prune) for u8, u7 in ((1, 1), (1, 0), (0, 1))]
                        out.append((base, prune))
    assert len(out) == 56
    return out


def flag_sets():
    """the default flags, then the program's 56 (the packer does not see `prune`: equal flags are packed once)"""
    return [F_DEFAULT] + [f for f, _ in program_flag_sets()]


def _runs(n, runs, fill=(5, 6)):
    """n lengths: runs = [(start, length, value)], the rest alternating `fill` (runs of one)"""
    v = [fill[i & 1] for i in range(n)]
    for s, l, x in runs:
        assert 0 <= s and s + l <= n
        v[s:s + l] = [x] * l
        if s + l < n and v[s + l] == x:        # keep the run's end where it was put
            v[s + l] = fill[0] if x != fill[0] else fill[1]
        if s > 0 and v[s - 1] == x:
            v[s - 1] = fill[0] if x != fill[0] else fill[1]
    return v


def vectors():
    """-> [(name, nLit, nDist, combined lengths)]"""
    out = []
    for nlit, ndist in ((257, 1), (288, 32)):
        n = nlit + ndist
        t = "%d" % n
        add = lambda name, v: out.append(("%s_%s" % (name, t), nlit, ndist, v))
        add("all_equal", [7] * n)
        add("all_zero", [0] * n)
        add("alternating", _runs(n, []))
        add("start_0", _runs(n, [(0, 9, 3)]))
        add("end_63", _runs(n, [(50, 14, 4)]))
        add("start_64", _runs(n, [(64, 20, 4)]))
        add("end_63_start_64", _runs(n, [(40, 24, 4), (64, 30, 0)]))
        for b in (64, 128, 192, 256):
            add("straddle_%d" % b, _runs(n, [(b - 5, min(12, n - (b - 5)), 9)]))
            add("straddle_%d_zeros" % b, _runs(n, [(b - 1, 2, 0)]))
        add("three_chunks", _runs(n, [(64, 192, 2)]))
        add("three_chunks_zeros", _runs(n, [(64, 192, 0)]))
        add("zeros_138", _runs(n, [(3, 138, 0)]))
        add("zeros_139", _runs(n, [(60, 139, 0)]))
        if n >= 290:
            add("zeros_277", _runs(n, [(7, 277, 0)]))
        add("lit_into_dist", _runs(n, [(nlit - 1, 2, 8)]) if ndist > 1 else _runs(n, [(nlit - 6, 7, 8)]))
        add("zeros_lit_into_dist", _runs(n, [(nlit - 20, min(21 + 9, n - nlit + 20), 0)]))
        add("ends_at_n", _runs(n, [(n - 13, 13, 3)]))
        add("zeros_end_at_n", _runs(n, [(n - 70, 70, 0)]))
        add("last_alone", _runs(n, [(n - 1, 1, 15)]))
        # the literal then 7 / 8 repeats (F_USE7 / F_USE8 / F_ALT8), and one more and one fewer, at a chunk border too
        add("runs_of_7_8_9", _runs(n, [(2, 8, 4), (20, 9, 3), (40, 10, 2), (58, 8, 1), (70, 9, 0), (90, 8, 0), (100, 9, 10), (126, 9, 11), (150, 7, 12), (189, 9, 13)]))
        add("short_runs", _runs(n, [(1, 2, 0), (5, 3, 0), (10, 3, 4), (15, 4, 4), (62, 3, 0), (126, 4, 7), (200, 10, 0), (215, 11, 0)]))
    return out


def state_lengths(nlit, ndist, combined):
    """the state's layout: literal/length[288] then distance[32]"""
    assert len(combined) == nlit + ndist and 1 <= nlit <= NLIT and 1 <= ndist <= NDIST
    return list(combined[:nlit]) + [0] * (NLIT - nlit) + list(combined[nlit:]) + [0] * (NDIST - ndist)


def pack_header(L, nlit, ndist, combined, flags):
    """d4g_debug_pack_header -> (pairs as u16, clLen[19], nCl, bits)"""
    lens = (ctypes.c_uint8 * (NLIT + NDIST))(*state_lengths(nlit, ndist, combined))
    pairs = (ctypes.c_uint16 * MAXPAIRS)()
    cl = (ctypes.c_uint8 * 19)()
    np_, ncl, bits = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = abi_calls.pack_header_fn(L)(lens, nlit, ndist, flags, pairs, ctypes.byref(np_), cl, ctypes.byref(ncl), ctypes.byref(bits))
    assert rc == 0, L.d4g_last_error()
    assert 0 < np_.value <= MAXPAIRS
    return list(pairs[:np_.value]), list(cl), ncl.value, bits.value


def decode(pairs):
    """u16 pairs (d4g_types.h) -> the oracle's list: a symbol, and after 16 / 17 / 18 the run as it is transmitted"""
    out = []
    last = None
    for p in pairs:
        sym, x = p & 31, (p >> 5) & 0xff
        assert p >> 13 == 0 and sym <= 18, hex(p)
        if sym < 16:
            assert x == 0
            out.append(sym)
            last = sym
        elif sym == 16:
            assert x >> 2 == last, (hex(p), last)       # the pair carries the length it repeats
            out += [16, x & 3]
        else:
            out += [sym, x - (3 if sym == 17 else 11)]
            last = 0
    return out


_expected = {}


def expected(combined, flags):
    """the oracle's packing and what follows from it -> (pack list, clLen[19], nCl, bits); kept per (vector, flags)"""
    key = (tuple(combined), flags)
    if key not in _expected:
        want = O.pack(list(combined), *[bool(flags >> b & 1) for b in range(8)])
        count = [0] * 19
        i = 0
        while i < len(want):
            count[want[i]] += 1
            i += 2 if want[i] >= 16 else 1
        cl = O.huffman_lengths(count, 7)[0]
        used = [i for i in range(19) if cl[CL_ORDER[i]]]       # everything up to the last non-zero length, in transmit order
        ncl = used[-1] + 1 if used else 19
        bits = 14 + 3 * ncl + sum(count[s] * (cl[s] + EXTRA.get(s, 0)) for s in range(19))
        _expected[key] = (want, cl, ncl, bits, sum(count))
    return _expected[key]


def mismatches(L):
    """every vector under every flag set -> [(name, flags, what)]"""
    bad = []
    for name, nlit, ndist, v in vectors():
        for flags in sorted(set(flag_sets())):
            want, cl, ncl, bits, npairs = expected(v, flags)
            got_pairs, got_cl, got_ncl, got_bits = pack_header(L, nlit, ndist, v, flags)
            if decode(got_pairs) != want or len(got_pairs) != npairs:
                bad.append((name, flags, "pairs"))
            if got_cl != cl:
                bad.append((name, flags, "clLen", got_cl, cl))
            if (got_ncl, got_bits) != (ncl, bits):
                bad.append((name, flags, "nCl/bits", (got_ncl, got_bits), (ncl, bits)))
    return bad
