"""The LZ77 encoder with preset dictionaries on the GPU (d4g_batch_create_encode_dict / d4g_deflate_streams_dict):
byte-identical to the committed zlib 1.2.11 vectors and to live zlib at every shape of lz_dict_cases.py and past two window
slides, encode + optimise equal to parse + optimise under both executors, every output slot of the one-shot call defined,
whole zlib streams, and 1 MiB behind a 32 KiB dictionary with a bounded number of parse passes."""
import ctypes
import zlib

import pytest

import lz_dict_cases as C

pytestmark = pytest.mark.gpu
live = pytest.mark.skipif(not C.LIVE_ZLIB, reason="live comparisons need zlib 1.2.11")


@pytest.fixture(scope="module")
def D():
    import deft4j_amd
    deft4j_amd.init(0)
    return deft4j_amd


def encode_all(D, cases, pairs, optimise=False, merge=True):
    specs = [(i, D.ENC_JVM, st, lv) for i in range(len(cases)) for lv, st in pairs]
    b = D.EncodeBatch([c[2] for c in cases], specs, dictionaries=[c[1] for c in cases], dictionary_of=list(range(len(cases)))).run(optimise, merge)
    return b, specs


def test_golden_vectors(D):
    cases = C.small_cases()
    want, made_from = C.golden()
    b, specs = encode_all(D, cases, C.PAIRS)
    assert len(want) == len(specs)
    for k, (i, _, st, lv) in enumerate(specs):
        name, d, data = cases[i]
        assert made_from[name] == (C.sha(d), C.sha(data)), name
        assert b.output(k) == want[(name, lv, st)], (name, lv, st)
    assert all(v["verdict"] == 0 for v in b.verify())
    assert b.stats()["dict_streams"] == sum(1 for c in cases if c[1]) * len(C.PAIRS)
    b.close()


@live
def test_every_shape_every_pair_vs_zlib(D):
    """the small shapes, the slide behind a full dictionary, the stored blocks under a moving window base and the 70 000-byte
    inputs (a second slide): one batch, every (level, strategy) pair"""
    cases = C.small_cases() + [C.slide_case()] + C.noise_cases() + C.long_cases()
    b, specs = encode_all(D, cases, C.PAIRS)
    for k, (i, _, st, lv) in enumerate(specs):
        name, d, data = cases[i]
        out = b.output(k)
        assert out == C.zref(data, lv, st, d), (name, lv, st)
        assert zlib.decompressobj(-15, zdict=d).decompress(out) == data, (name, lv, st)
    b.close()


@live
def test_mixed_dictionaries_and_shared_parses(D):
    t = C.text()
    A, Bd = t[:5000], t[60000:62049]
    ins = [t[5000:45000], t[62049:100000], t[5000:45000], t[9000:12000], b""]
    of = [0, 1, None, 1, 0]
    specs = [(i, D.ENC_JVM, st, lv) for i in range(len(ins)) for lv, st in ((6, 0), (6, 4), (1, 0), (1, 1), (9, 3), (6, 2))]
    b = D.EncodeBatch(ins, specs, dictionaries=[A, Bd], dictionary_of=of).run(False)
    for k, (i, _, st, lv) in enumerate(specs):
        d = None if of[i] is None else (A, Bd)[of[i]]
        want = C.zref_plain(ins[i], lv, st) if d is None else C.zref(ins[i], lv, st, d)
        assert b.output(k) == want, (i, lv, st)
    assert b.stats()["dict_streams"] == 4 * 6
    b.close()


@live
@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("executor", ["fused", "levels"])
def test_encode_then_optimise_equals_parse_then_optimise(D, monkeypatch, executor, merge):
    monkeypatch.setenv("D4G_EXEC", executor)
    names = ("prefix3", "prefix2049", "prefix32768", "straddle30000", "same3000", "len0_dict700", "arun258", "pngidat", "nomatch")
    cases = [c for c in C.small_cases() if c[0] in names] + [C.slide_case(), C.noise_cases()[0], C.long_cases()[1]]
    pairs = ((1, 0), (6, 0), (6, 4), (9, 3))
    e, specs = encode_all(D, cases, pairs, True, merge)
    enc = [C.zref(cases[i][2], lv, st, cases[i][1]) for i, _, st, lv in specs]
    p = D.Batch(enc, dictionaries=[c[1] for c in cases], dictionary_of=[i for i, _, _, _ in specs]).run(merge)
    for k, sp in enumerate(specs):
        re_, rp = e.result(k), p.result(k)
        assert (re_["status"], re_["saved_bits"], re_["size_bits_in"]) == (rp["status"], rp["saved_bits"], rp["size_bits_in"]), (cases[sp[0]][0], sp)
        assert e.output(k) == p.output(k), (cases[sp[0]][0], sp)
    assert all(v["verdict"] == 0 for v in e.verify())
    e.close()
    p.close()


@live
def test_one_shot_call_defines_every_output_slot(D):
    L = D._need()
    t = C.text()
    ins = [t[3000:9000], b"", t[3000:3001], C.noise(3000, 5)]
    dicts = [t[:3000], b"", t[100:200]]
    of = [0, 2, -1, 1]                                     # (dictionary 1 has length 0: none)
    n = len(ins)
    arr = (ctypes.c_char_p * n)(*ins)
    lens = (ctypes.c_size_t * n)(*[len(s) for s in ins])
    darr = (ctypes.c_char_p * 3)(*dicts)
    dlens = (ctypes.c_size_t * 3)(*[len(d) for d in dicts])
    out = (ctypes.c_void_p * n)()
    olen = (ctypes.c_size_t * n)(*([77] * n))
    assert L.d4g_deflate_streams_dict(n, arr, lens, D.ENC_JVM, 6, 0, 3, darr, dlens, (ctypes.c_int32 * n)(*of), out, olen) == 0
    for i in range(n):
        assert out[i]
        got = ctypes.string_at(out[i], olen[i])
        L.d4g_free(out[i])
        d = dicts[of[i]] if of[i] >= 0 else b""
        assert got == (C.zref(ins[i], 6, 0, d) if d else C.zref_plain(ins[i], 6, 0)), i
    # a refused call hands back no buffers: every slot NULL / 0
    out = (ctypes.c_void_p * n)()
    olen = (ctypes.c_size_t * n)(*([77] * n))
    assert L.d4g_deflate_streams_dict(n, arr, lens, D.ENC_JZLIB, 9, 0, 3, darr, dlens, (ctypes.c_int32 * n)(*of), out, olen) == -2
    assert not any(out) and list(olen) == [0] * n
    assert L.d4g_deflate_streams_dict(n, arr, lens, D.ENC_JVM, 6, 0, 3, darr, dlens, (ctypes.c_int32 * n)(0, 3, -1, 1), out, olen) == -2
    assert not any(out) and list(olen) == [0] * n


@live
def test_zlib_streams_whole_streams(D):
    t = C.text()
    ins = [t[3000:40000], b"", b"a" * 500, C.noise(20000, 9)]
    for d in (None, t[:3000], t[:40000]):
        for lv, st in ((1, 0), (4, 0), (6, 0), (9, 0), (6, 1), (6, 2), (6, 3), (6, 4), (-1, 0)):
            got = D.zlib_streams(ins, lv, st, dictionaries=d)
            for i, data in enumerate(ins):
                c = zlib.compressobj(lv, 8, 15, 8, C.ZS[st]) if d is None else zlib.compressobj(lv, 8, 15, 8, C.ZS[st], d)
                assert got[i] == c.compress(data) + c.flush(), (i, lv, st, d is not None)


@live
@pytest.mark.parametrize("level", [6, 9])
def test_1mib_behind_a_full_dictionary(D, level):
    t = C.text()
    import synth
    raw = synth.reptext(1 << 20, 0xD1C8)
    d = t[:32768]
    b = D.EncodeBatch([raw], [(0, D.ENC_JVM, 0, level)], dictionaries=d).run(False)
    s = b.stats()
    assert b.output(0) == C.zref(raw, level, 0, d)
    assert 1 <= s["lz_parse_passes"] <= 8, s["lz_parse_passes"]   # deflate_slow converges as level 9 does (test_gpu_lz_levels.py)
    b.close()
