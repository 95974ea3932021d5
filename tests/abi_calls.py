"""Direct ctypes calls of the one-shot C-ABI entry points (include/deft4g.h) — shared by the GPU boundary tests
and the emulator tests.  These are the functions the JNI shim (jni/deft4g_jni.c) binds."""
import ctypes


def optimise_streams(L, streams, merge):
    """d4g_optimise_streams -> (rc, [(status, saved_bits, bytes-or-None)])"""
    n = len(streams)
    keep = [bytes(s) for s in streams]
    arr = (ctypes.c_char_p * n)(*keep)
    lens = (ctypes.c_size_t * n)(*[len(s) for s in keep])
    out = (ctypes.c_void_p * n)(*([0xdead] * n))        # poisoned: the call must define every slot
    olen = (ctypes.c_size_t * n)(*([12345] * n))
    saved = (ctypes.c_int64 * n)(*([-7] * n))
    status = (ctypes.c_int32 * n)(*([99] * n))
    rc = L.d4g_optimise_streams(n, arr, lens, 1 if merge else 0, out, olen, saved, status)
    res = []
    for i in range(n):
        data = None
        if out[i]:
            data = ctypes.string_at(out[i], olen[i])
            L.d4g_free(out[i])
        res.append((status[i], saved[i], data))
    return rc, res


def size_bits_fallback(L, data):
    bits = ctypes.c_int64(-1)
    rc = L.d4g_size_bits_fallback(bytes(data), len(data), ctypes.byref(bits))
    return rc, bits.value


def inflate(L, data):
    """d4g_inflate -> (rc, status, decoded-or-None, consumed)"""
    out = ctypes.c_void_p(0xdead)
    ol = ctypes.c_size_t(777)
    co = ctypes.c_size_t(0)
    st = ctypes.c_int32(99)
    rc = L.d4g_inflate(bytes(data), len(data), ctypes.byref(out), ctypes.byref(ol), ctypes.byref(co), ctypes.byref(st))
    dec = None
    if rc == 0 and out.value:
        dec = ctypes.string_at(out.value, ol.value)
        L.d4g_free(out)
    return rc, st.value, dec, co.value


def check_one_shot_entry_points(L, O, streams, merge):
    """Every stream of one d4g_optimise_streams call against the oracle; the NULL-out contract of deft4g.h:
    out[i] is set only for D4G_STREAM_CHANGED."""
    import zlib
    rc, res = optimise_streams(L, streams, merge)
    assert rc == 0
    kinds = set()
    for a, (st, sv, data) in zip(streams, res):
        orc, want, osaved, oconsumed, _ = O.optimise(a, merge)
        assert st == orc, (st, orc)
        kinds.add(st)
        if st == 0:
            assert data == want and sv == osaved and sv > 0
        else:
            assert data is None and sv == 0          # unchanged / parse error: the caller keeps its ORIGINAL array
        rc2, bits = size_bits_fallback(L, a)
        ob = O.size_bits(a)                          # -1: DeflateStream.parse failed
        assert rc2 == 0 and bits == (ob if ob >= 0 else len(a) * 8)   # parse failure -> len * 8 (B/Deft.java:48-54)
        rc3, st3, dec, consumed = inflate(L, a)
        assert rc3 == 0
        if orc >= 0:
            assert st3 >= 0 and dec == zlib.decompress(a, -15) and consumed == oconsumed
        else:
            assert st3 < 0 and dec is None
    return kinds


def pack_header_fn(L):
    """d4g_debug_pack_header with its prototype (include/deft4g.h)"""
    f = L.d4g_debug_pack_header
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p]
    return f


def pack_header_call(L, null=False):
    """d4g_debug_pack_header on 257 + 1 lengths of 8 under the default flags (null: every pointer NULL) -> rc"""
    if null:
        return pack_header_fn(L)(None, 257, 1, 7, None, None, None, None, None)
    lens = (ctypes.c_uint8 * 320)(*([8] * 320))
    pairs, cl = (ctypes.c_uint16 * 320)(), (ctypes.c_uint8 * 19)()
    n, ncl, bits = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    return pack_header_fn(L)(lens, 257, 1, 7, pairs, ctypes.byref(n), cl, ctypes.byref(ncl), ctypes.byref(bits))


class Slots:
    """Poisoned result arrays of a one-shot call with n streams: the call must define every slot it is given."""

    def __init__(self, n):
        self.n = n
        self.out = (ctypes.c_void_p * n)(*([0xdead] * n))
        self.len = (ctypes.c_size_t * n)(*([12345] * n))
        self.status = (ctypes.c_int32 * n)(*([99] * n))
        self.saved = (ctypes.c_int64 * n)(*([-7] * n))
        self.rsaved = (ctypes.c_int64 * n)(*([-7] * n))
        self.winner = (ctypes.c_int32 * n)(*([99] * n))

    def unchanged(self, status=False, saved=False, rsaved=False, winner=False):
        """every slot of the named arrays holds the "unchanged" value of deft4g.h: out NULL, out_len 0, status
        D4G_STREAM_UNCHANGED, saved_bits / recompress_saved 0, winner -1"""
        return all(self.out[i] is None and self.len[i] == 0 and (not status or self.status[i] == 1) and
                   (not saved or self.saved[i] == 0) and (not rsaved or self.rsaved[i] == 0) and (not winner or self.winner[i] == -1)
                   for i in range(self.n))


def one_shot_calls(L, streams, mode=1, level=6, iterations=3, master_block=8 << 20):
    """Every one-shot entry point on `streams` with poisoned result arrays: name -> (call, Slots, which arrays to check)."""
    n = len(streams)
    keep = [bytes(s) for s in streams]
    arr = (ctypes.c_char_p * n)(*keep)
    lens = (ctypes.c_size_t * n)(*[len(s) for s in keep])
    s = {k: Slots(n) for k in ("optimise", "sharded", "deflate", "level", "zopfli", "compress", "recompress")}
    return {
        "d4g_optimise_streams": (lambda: L.d4g_optimise_streams(n, arr, lens, 1, s["optimise"].out, s["optimise"].len, s["optimise"].saved,
                                                                s["optimise"].status), s["optimise"], dict(status=True, saved=True)),
        "d4g_optimise_streams_sharded": (lambda: L.d4g_optimise_streams_sharded(n, arr, lens, 1, s["sharded"].out, s["sharded"].len,
                                                                                s["sharded"].saved, s["sharded"].status),
                                         s["sharded"], dict(status=True, saved=True)),
        "d4g_deflate_streams": (lambda: L.d4g_deflate_streams(n, arr, lens, 0, 0, s["deflate"].out, s["deflate"].len), s["deflate"], {}),
        "d4g_deflate_streams_level": (lambda: L.d4g_deflate_streams_level(n, arr, lens, 0, level, 0, s["level"].out, s["level"].len),
                                      s["level"], {}),
        "d4g_zopfli_streams": (lambda: L.d4g_zopfli_streams(n, arr, lens, iterations, 0, 15, master_block, s["zopfli"].out, s["zopfli"].len),
                               s["zopfli"], {}),
        "d4g_compress": (lambda: L.d4g_compress(n, arr, lens, mode, 1, 1, s["compress"].out, s["compress"].len, s["compress"].winner),
                         s["compress"], dict(winner=True)),
        "d4g_recompress_streams": (lambda: L.d4g_recompress_streams(n, arr, lens, mode, 1, 1, s["recompress"].out, s["recompress"].len,
                                                                    s["recompress"].saved, s["recompress"].rsaved, s["recompress"].status),
                                   s["recompress"], dict(status=True, saved=True, rsaved=True)),
    }
