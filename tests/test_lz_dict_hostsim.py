"""The LZ77 encoder with preset dictionaries (d4g_batch_create_encode_dict / d4g_deflate_streams_dict) in the test-only
CPU emulator: byte-identical to zlib 1.2.11's deflateSetDictionary output and to the committed vectors at every shape of
lz_dict_cases.py; encode + optimise equal to parse + optimise of zlib's bytes; verification, zlib_streams, the refusals, and
the no-dictionary encoder unchanged."""
import ctypes
import os
import subprocess
import sys
import zlib

import pytest

import lz_dict_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "hostsim", "libdeft4g_hostsim.so")
live = pytest.mark.skipif(not C.LIVE_ZLIB, reason="live comparisons need zlib 1.2.11")


@pytest.fixture(scope="module")
def sim():
    os.environ["D4G_SIM_BLOCK"] = "64"
    subprocess.check_call([os.path.join(ROOT, "tests", "hostsim", "build.sh")])
    import deft4j_amd as D
    L = D.load_library(SO)
    D.init(0, lib=L)
    return D, L


def device_blocks(L):
    n = ctypes.c_int64()
    assert L.d4g_debug_device_blocks(ctypes.byref(n)) == 0
    return n.value


@pytest.fixture(scope="module")
def small_outputs(sim):
    """every small case at every (level, strategy) pair, one batch with one dictionary per input: {(name, level, strategy):
    bytes}, and the batch's verification and statistics"""
    D, L = sim
    cases = C.small_cases()
    specs = [(i, D.ENC_JVM, st, lv) for i in range(len(cases)) for lv, st in C.PAIRS]
    b = D.EncodeBatch([c[2] for c in cases], specs, lib=L, dictionaries=[c[1] for c in cases], dictionary_of=list(range(len(cases)))).run(False)
    got = {(cases[i][0], lv, st): b.output(k) for k, (i, _, st, lv) in enumerate(specs)}
    verdicts = b.verify()
    stats = b.stats()
    b.close()
    return cases, got, verdicts, stats


@live
def test_small_cases_every_pair_vs_zlib(small_outputs):
    cases, got, _, _ = small_outputs
    for name, d, data in cases:
        for lv, st in C.PAIRS:
            out = got[(name, lv, st)]
            assert out == C.zref(data, lv, st, d), (name, lv, st)
            assert zlib.decompressobj(-15, zdict=d).decompress(out) == data, (name, lv, st)


def test_small_cases_every_pair_vs_golden(small_outputs):
    cases, got, verdicts, stats = small_outputs
    want, made_from = C.golden()
    assert len(want) == len(cases) * len(C.PAIRS)
    for name, d, data in cases:
        assert made_from[name] == (C.sha(d), C.sha(data)), name   # the vectors were made from these bytes
        for lv, st in C.PAIRS:
            assert got[(name, lv, st)] == want[(name, lv, st)], (name, lv, st)
    # the written streams parse against their dictionaries and decode to the inputs (d4g_batch_verify)
    assert all(v["verdict"] == 0 for v in verdicts), [k for k, v in enumerate(verdicts) if v["verdict"] != 0]
    assert stats["dict_streams"] == sum(1 for c in cases if c[1]) * len(C.PAIRS)


def test_known_bytes(sim):
    """The outputs the feature was specified with: the NIL slot, the run from the dictionary's last byte."""
    D, L = sim
    assert D.deflate_streams([b"aaaaaaaa"], D.ENC_JVM, D.STRATEGY_RLE, lib=L, level=6, dictionaries=b"xa")[0] == bytes.fromhex("830100")
    assert D.deflate_streams([b"aaaaaaaa"], D.ENC_JVM, D.STRATEGY_RLE, lib=L, level=6)[0] == bytes.fromhex("4b840200")
    b = D.EncodeBatch([b"abcdefgh", b"bcdefgh"], [(0, 0, 0, 9), (1, 0, 0, 9)], lib=L, dictionaries=b"abcdefgh").run(False)
    first, second = b.block_info(0, final=True), b.block_info(1, final=True)
    assert [x["tokens"] for x in first] == [3] and [x["tokens"] for x in second] == [2]   # literal + match + end / match + end
    b.close()


@live
@pytest.mark.parametrize("pair", [(1, 0), (6, 0)])
def test_window_slide_behind_a_full_dictionary(sim, pair):
    D, L = sim
    lv, st = pair
    name, d, data = C.slide_case()
    assert D.deflate_streams([data], D.ENC_JVM, st, lib=L, level=lv, dictionaries=d)[0] == C.zref(data, lv, st, d)


@live
def test_stored_blocks_while_the_window_base_moves(sim):
    D, L = sim
    cases = C.noise_cases()
    pairs = ((1, 0), (6, 0), (6, 2))
    specs = [(i, D.ENC_JVM, st, lv) for i in range(len(cases)) for lv, st in pairs]
    b = D.EncodeBatch([c[2] for c in cases], specs, lib=L, dictionaries=[c[1] for c in cases], dictionary_of=[0, 1]).run(False)
    for k, (i, _, st, lv) in enumerate(specs):
        assert b.output(k) == C.zref(cases[i][2], lv, st, cases[i][1]), (cases[i][0], lv, st)
    b.close()


@live
def test_mixed_dictionaries_and_shared_parses(sim):
    """Inputs with dictionary A, with dictionary B and with none in one batch; two specs that share one parse (FIXED parses
    as DEFAULT does)."""
    D, L = sim
    t = C.text()
    A, Bd = t[:5000], t[60000:62049]
    ins = [t[5000:8000], t[62049:65000], t[5000:8000], t[9000:12000]]
    of = [0, 1, None, 1]
    specs = [(i, D.ENC_JVM, st, lv) for i in range(len(ins)) for lv, st in ((6, 0), (6, 4), (1, 0), (9, 3))]
    b = D.EncodeBatch(ins, specs, lib=L, dictionaries=[A, Bd], dictionary_of=of).run(False)
    for k, (i, _, st, lv) in enumerate(specs):
        d = None if of[i] is None else (A, Bd)[of[i]]
        want = C.zref_plain(ins[i], lv, st) if d is None else C.zref(ins[i], lv, st, d)
        assert b.output(k) == want, (i, lv, st)
    assert b.stats()["dict_streams"] == 3 * 4
    b.close()


@live
@pytest.mark.parametrize("merge", [False, True])
def test_encode_then_optimise_equals_parse_then_optimise(sim, merge):
    """The differential against the parse path: the encoder hands the optimiser what the parser makes of zlib's bytes."""
    D, L = sim
    cases = [c for c in C.small_cases() if c[0] in ("prefix3", "prefix2049", "prefix32768", "straddle30000", "same3000", "len0_dict700",
                                                   "arun258", "pngidat", "nomatch")]
    pairs = ((1, 0), (6, 0), (6, 4), (9, 3))
    specs = [(i, D.ENC_JVM, st, lv) for i in range(len(cases)) for lv, st in pairs]
    dicts = [c[1] for c in cases]
    e = D.EncodeBatch([c[2] for c in cases], specs, lib=L, dictionaries=dicts, dictionary_of=list(range(len(cases)))).run(True, merge)
    enc = [C.zref(cases[i][2], lv, st, cases[i][1]) for i, _, st, lv in specs]
    p = D.Batch(enc, lib=L, dictionaries=dicts, dictionary_of=[i for i, _, _, _ in specs]).run(merge)
    for k, sp in enumerate(specs):
        re_, rp = e.result(k), p.result(k)
        assert (re_["status"], re_["saved_bits"], re_["size_bits_in"]) == (rp["status"], rp["saved_bits"], rp["size_bits_in"]), (cases[sp[0]][0], sp)
        assert e.output(k) == p.output(k), (cases[sp[0]][0], sp)
        assert zlib.decompressobj(-15, zdict=cases[sp[0]][1]).decompress(e.output(k)) == cases[sp[0]][2]
    assert all(v["verdict"] == 0 for v in e.verify())
    e.close()
    p.close()


VERIFY_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import deft4j_amd as D
import lz_dict_cases as C
L = D.load_library(sys.argv[2])
D.init(0, lib=L)
t = C.text()
out = D.deflate_streams([t[2049:5000], b""], D.ENC_JVM, 0, lib=L, level=6, dictionaries=t[:2049])
b = D.EncodeBatch([t[2049:5000]], [(0, 0, 0, 6), (0, 0, 3, 1)], lib=L, dictionaries=t[:2049]).run(True, True)
assert b.stats()["verify_streams"] == 2, b.stats()["verify_streams"]
print("verified", len(out))
"""


def test_verify_switch_passes_on_a_dictionary_encode(sim):
    env = dict(os.environ, D4G_VERIFY="1", D4G_SIM_BLOCK="64")
    r = subprocess.run([sys.executable, "-c", VERIFY_CHILD, ROOT, SO], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "verified 2" in r.stdout, r.stderr[-2000:]


@live
def test_zlib_streams_whole_streams(sim):
    D, L = sim
    t = C.text()
    ins = [t[3000:6000], b"", b"a" * 500]
    for d in (None, t[:3000]):
        for lv, st in ((1, 0), (4, 0), (6, 0), (9, 0), (6, 1), (6, 2), (6, 3), (6, 4), (-1, 0)):
            got = D.zlib_streams(ins, lv, st, dictionaries=d, lib=L)
            for i, data in enumerate(ins):
                c = zlib.compressobj(lv, 8, 15, 8, C.ZS[st]) if d is None else zlib.compressobj(lv, 8, 15, 8, C.ZS[st], d)
                assert got[i] == c.compress(data) + c.flush(), (i, lv, st, d is not None)
    assert D.zlib_streams([b"abc"], 6, 0, dictionaries=t[:100], lib=L)[0][:2] == b"\x78\xbb"
    assert D.zlib_streams([b"abc"], 9, 0, dictionaries=t[:100], lib=L)[0][:2] == b"\x78\xf9"
    assert D.zlib_streams([b"abc"], 1, 0, dictionaries=t[:100], lib=L)[0][:2] == b"\x78\x3f"
    # DICTID is the Adler-32 of the whole dictionary, before the tail is cut
    long_dict = t[:40000]
    z = D.zlib_streams([t[40000:41000]], 6, 0, dictionaries=long_dict, lib=L)[0]
    assert z[2:6] == zlib.adler32(long_dict).to_bytes(4, "big")
    assert zlib.decompressobj(15, zdict=long_dict).decompress(z) == t[40000:41000]


@live
def test_tail_rule_and_empty_dictionary(sim):
    D, L = sim
    t = C.text()
    data = t[40000:43000]
    for lv, st in ((1, 0), (6, 0)):
        a = D.deflate_streams([data], D.ENC_JVM, st, lib=L, level=lv, dictionaries=t[:40000])[0]
        assert a == D.deflate_streams([data], D.ENC_JVM, st, lib=L, level=lv, dictionaries=t[40000 - 32768:40000])[0]
        # a dictionary of length 0 is none: the same bytes, no dictionary stream counted
        assert D.deflate_streams([data], D.ENC_JVM, st, lib=L, level=lv, dictionaries=b"")[0] == C.zref_plain(data, lv, st)
    b = D.EncodeBatch([data], [(0, 0, 0, 6)], lib=L, dictionaries=[b""], dictionary_of=[0]).run(False)
    assert b.stats()["dict_streams"] == 0 and b.stats()["dict_bytes"] == 0
    b.close()


@live
def test_no_dictionary_encoder_gives_what_it_gave(sim):
    D, L = sim
    t = C.text()
    ins = [t[:3000], b"", b"q", C.noise(1500, 3), b"\0" * 5000]
    specs = [(i, D.ENC_JVM, st, lv) for i in range(len(ins)) for lv, st in C.PAIRS]
    b = D.EncodeBatch(ins, specs, lib=L).run(False)
    for k, (i, _, st, lv) in enumerate(specs):
        assert b.output(k) == C.zref_plain(ins[i], lv, st), (i, lv, st)
    assert b.stats()["dict_streams"] == 0
    b.close()


def test_refusals_leave_no_device_blocks(sim):
    D, L = sim
    raw = b"abcabcabcabc"
    before = device_blocks(L)
    assert D.deflate_streams([raw], D.ENC_JVM, 0, lib=L, level=6, dictionaries=b"abc")[0]
    assert device_blocks(L) == before
    arr = (ctypes.c_char_p * 1)(raw)
    lens = (ctypes.c_size_t * 1)(len(raw))
    darr = (ctypes.c_char_p * 1)(b"abcabc")
    dlens = (ctypes.c_size_t * 1)(6)

    def one_shot(enc, lv, st, n_dict, da, dl, of):
        out = (ctypes.c_void_p * 1)()
        olen = (ctypes.c_size_t * 1)(77)
        rc = L.d4g_deflate_streams_dict(1, arr, lens, enc, lv, st, n_dict, da, dl, of, out, olen)
        return rc, out[0], olen[0]

    def create(enc, lv, st, n_dict, da, dl, of):
        sp = (D.d4g_encoder_spec_level * 1)(D.d4g_encoder_spec_level(0, enc, st, lv))
        return L.d4g_batch_create_encode_dict(1, arr, lens, n_dict, da, dl, of, 1, sp)

    of0, of_bad, of_low = (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(1), (ctypes.c_int32 * 1)(-2)
    null_dict = (ctypes.c_char_p * 1)(None)
    refused = [(D.ENC_JZLIB, 9, 0, 1, darr, dlens, of0),        # the jzlib flavour with a dictionary
               (D.ENC_JVM, 6, 0, 1, darr, dlens, of_bad),       # dict_of names no dictionary
               (D.ENC_JVM, 6, 0, 1, darr, dlens, of_low),
               (D.ENC_JVM, 6, 0, 1, null_dict, dlens, of0),     # a NULL dictionary with a length
               (D.ENC_JVM, 0, 0, 1, darr, dlens, of0),          # and what the level entry points refuse
               (D.ENC_JVM, 6, 5, 1, darr, dlens, of0)]
    for args in refused:
        rc, out, olen = one_shot(*args)
        assert rc == -2 and not out and olen == 0, args[:4]     # D4G_ERR_ARG, the outputs defined
        assert L.d4g_last_error()
        assert not create(*args), args[:4]
        assert device_blocks(L) == before
    rc, _, _ = one_shot(D.ENC_JZLIB, 9, 0, 1, darr, dlens, of0)
    assert b"jzlib" in L.d4g_last_error()
    with pytest.raises(RuntimeError):
        D.EncodeBatch([raw], [(0, D.ENC_JZLIB, 0, 9)], lib=L, dictionaries=b"abc")
    # the jzlib flavour next to a dictionary of length 0, or for an input that names none, is not refused
    b = D.EncodeBatch([raw, raw], [(0, D.ENC_JZLIB, 0, 9), (1, D.ENC_JVM, 0, 9)], lib=L, dictionaries=[b"abc"], dictionary_of=[None, 0]).run(False)
    b.close()
    assert device_blocks(L) == before


REFUSE_BEFORE_INIT = r"""
import ctypes, os, sys
sys.path.insert(0, sys.argv[1])
import deft4j_amd as D
L = D.load_library(sys.argv[2])
raw = b"abcabc"
arr = (ctypes.c_char_p * 1)(raw); lens = (ctypes.c_size_t * 1)(len(raw))
darr = (ctypes.c_char_p * 1)(b"abc"); dlens = (ctypes.c_size_t * 1)(3); of = (ctypes.c_int32 * 1)(0)
out = (ctypes.c_void_p * 1)(); olen = (ctypes.c_size_t * 1)(5)
rc = L.d4g_deflate_streams_dict(1, arr, lens, 0, 6, 0, 1, darr, dlens, of, out, olen)
assert rc == -1 and not out[0] and olen[0] == 0, rc          # D4G_ERR_NODEVICE
sp = (D.d4g_encoder_spec_level * 1)(D.d4g_encoder_spec_level(0, 0, 0, 6))
assert not L.d4g_batch_create_encode_dict(1, arr, lens, 1, darr, dlens, of, 1, sp)
assert b"d4g_init" in L.d4g_last_error()
print("refused")
"""


def test_new_entry_points_refuse_before_init(sim):
    r = subprocess.run([sys.executable, "-c", REFUSE_BEFORE_INIT, ROOT, SO], capture_output=True, text=True)
    assert r.returncode == 0 and "refused" in r.stdout, r.stderr[-2000:]
