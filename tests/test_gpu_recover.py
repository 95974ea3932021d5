"""The bytes that decode before a stream's first failure, on the GPU through the C ABI (d4g_batch_recover,
d4g_batch_copy_recovered, d4g_recover_streams; k_recover_count / k_recover_emit with 512-thread block decoders).  Every
expected byte and record comes from the case builder (tests/recover_cases.py): zlib for the truncated streams, the
builder's own token bytes for the corrupted ones; len(recovered) == decoded_offset everywhere."""
import ctypes
import gzip
import os
import zlib

import pytest

import handbuilt_cases as H
import parse_error_cases as P
import recover_cases as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = 512
BATCH = LANES * P.CHUNK

# the smallest shapes at which the partial decode can still go wrong: each has to be among the cases
ZERO_BYTES = ["empty_input", "distance_1_first_token", "btype3_block_0"]
HEADER_BEHIND = [k + "_behind_" + b for k in ("btype3", "nlen_mismatch") for b in ("stored", "fixed", "dynamic", "scan_and_exact")]
GEOMETRY = ["bad_symbol_last_bit_of_chunk_0", "bad_symbol_across_stream_bit_512", "bad_symbol_in_chunk_5", "bad_symbol_in_last_chunk_of_batch_0",
            "bad_symbol_in_batch_1", "bad_symbol_past_a_restaging", "far_chunk_1_then_bad_chunk_7", "bad_chunk_1_then_far_chunk_7",
            "far_batch_0_then_bad_batch_1", "bad_batch_0_then_far_batch_1", "far_then_bad_in_one_chunk"]
LENGTH_TOKENS = ["fixed_dist_30", "dynamic_dist_31", "no_dist_code", "eof_in_distextra", "eof_in_distcode", "eof_in_lenextra", "distance_171_in_block_2"]
OVERLAP = ["overlap_dist_1_len_258_last", "overlap_dist_3_len_10_last"]
REACH = ["copies_reach_32768_across_segments"]


@pytest.fixture(scope="module")
def lib():
    import deft4j_amd as D
    return D, D.init(0)


@pytest.fixture(scope="module")
def cases():
    """built once, shared, never changed"""
    return R.corruption_cases(LANES) + R.truncation_cases() + R.truncation_cases(150000)


def live_blocks(L):
    n = ctypes.c_int64(-1)
    assert L.d4g_debug_device_blocks(ctypes.byref(n)) == 0
    return n.value


def wrong(c, got, err):
    """what is wrong with the recovered bytes `got` and the record `err` of case c (None: nothing)"""
    want = c.want
    if want["reason"] == P.OK:
        return None if got == c.expected and err["reason"] == P.OK else "a valid stream's bytes"
    if len(got) != want["decoded_offset"] or err["decoded_offset"] != want["decoded_offset"]:
        return "length %d, decoded_offset %d, want %d" % (len(got), err["decoded_offset"], want["decoded_offset"])
    if got != c.expected:
        return "bytes differ at %d" % next(i for i in range(len(got)) if got[i] != c.expected[i])
    if any(err[k] != v for k, v in want.items()):
        return "record %r, want %r" % (err, want)
    return None


def test_the_shapes_are_there(cases):
    """guards the case list, not the library"""
    d = {c.name: c for c in cases}
    for n in ZERO_BYTES:
        assert d[n].want["decoded_offset"] == 0 and d[n].expected == b""
    for n in HEADER_BEHIND:                              # only whole blocks are recovered
        assert d[n].want["bit_pos"] <= d[n].want["block_bit_pos"] + 48 and d[n].want["decoded_offset"] > 0
    g = [d[n].want["bit_pos"] - 3 for n in GEOMETRY]     # bits from the block's first token
    assert g[0] == P.CHUNK - 1 and g[1] < 512 - 3 < g[1] + 8 and g[2] // P.CHUNK == 5 and g[3] // P.CHUNK == LANES - 1
    assert g[4] > BATCH and g[5] > P.WINDOW_BITS and g[8] // P.CHUNK == g[9] // P.CHUNK == LANES - 1 and g[10] // P.CHUNK == 3
    assert all(d[n].expected for n in GEOMETRY + LENGTH_TOKENS + OVERLAP + REACH)
    assert d[OVERLAP[0]].expected[-258:] == d[OVERLAP[0]].expected[-1:] * 258
    assert len(d[REACH[0]].expected) > 32768 + 8192
    assert sum(1 for c in cases if "_cut_" in c.name) > 150 and sum(1 for c in cases if len(c.expected) > 100000) >= 6


def test_every_case_as_one_batch(lib, cases):
    """one batch, one recovery for all its failed streams; the diagnosis is what it was before anybody asked for bytes,
    copy_decoded still refuses a failed stream, and the one-shot call answers the same"""
    D, L = lib
    cs = cases
    b = D.Batch([c.data for c in cs]).parse()
    before = [b.parse_error(i) for i in range(len(cs))]
    got = [b.recovered(i) for i in range(len(cs))]
    st = b.stats()
    assert [b.recovered(i) for i in range(0, len(cs), 9)] == got[::9] and b.stats() == st      # kept, not made again
    assert [b.parse_error(i) for i in range(len(cs))] == before
    assert not [(c.name, w) for c, g, e in zip(cs, got, before) for w in [wrong(c, g, e)] if w]
    failed = [c for c in cs if c.want["reason"] != P.OK and c.want["decoded_offset"] > 0]
    assert st["recover_streams"] == len(failed) and st["recover_bytes"] == sum(len(c.expected) for c in failed)
    assert st["ms_recover"] > 0 and st["ms_recover_kernels"] > 0
    for i, c in enumerate(cs):
        if c.want["reason"] == P.OK:
            assert b.decoded(i) == c.expected
        else:
            assert L.d4g_batch_copy_decoded(b.h, i, None, 0, None) == -2 and L.d4g_last_error() == b"stream did not parse"
    b.close()
    assert D.recover_streams([c.data for c in cs]) == list(zip(got, before))


def test_every_case_alone(lib, cases):
    """a stream's recovered bytes do not depend on its neighbours, nor on whether the batch parsed or ran"""
    D, L = lib
    bad = []
    for k, c in enumerate(cases):
        b = D.Batch([c.data])
        b.parse() if k % 2 or len(c.data) > 20000 else b.run(True)
        w = wrong(c, b.recovered(0), b.parse_error(0))
        if w:
            bad.append((c.name, w))
        b.close()
    assert not bad


def test_copy_paths_agree(lib, cases, monkeypatch):
    """the side batch routes like any other: block-local copies, byte doubling and the default give the same bytes"""
    D, L = lib
    cs = [c for c in cases if c.want["reason"] != P.OK and c.expected]
    got = {}
    for mode in ("blocks", "doubling", "auto"):
        monkeypatch.setenv("D4G_COPY", mode)
        got[mode] = D.recover_streams([c.data for c in cs])
        assert not [(mode, c.name, w) for c, (g, e) in zip(cs, got[mode]) for w in [wrong(c, g, e)] if w]
    assert got["blocks"] == got["doubling"] == got["auto"]


@pytest.mark.parametrize("how", ["parse", "run", "run_recompress"])
def test_mixed_batch(lib, how):
    """12 streams, 5 of them failing: recovery after parse, after run(merge) and after run_recompress(1); whatever the valid
    streams report is what a batch that never asked reports"""
    D, L = lib
    cs, good = R.mixed_batch(LANES)

    def go(streams):
        b = D.Batch(streams)
        return b.parse() if how == "parse" else b.run(True) if how == "run" else b.run_recompress(D.MODE_CHEAP, True)
    quiet, b = go([c.data for c in cs]), go([c.data for c in cs])
    b.recover()
    launches = b.stats()["kernel_launches"]
    b.recover()
    assert b.stats()["kernel_launches"] == launches     # idempotent
    for i, c in enumerate(cs):
        assert wrong(c, b.recovered(i), b.parse_error(i)) is None, c.name
        assert b.result(i) == quiet.result(i) and b.parse_error(i) == quiet.parse_error(i)
        if c.want["reason"] == P.OK:
            assert b.decoded(i) == quiet.decoded(i) == b.recovered(i) and b.checksums(i) == quiet.checksums(i)
            assert b.block_info(i) == quiet.block_info(i)
            if how != "parse":
                assert b.output(i) == quiet.output(i)
        else:
            assert b.result(i)["status"] == -1
    if how != "parse":
        assert b.verify() == quiet.verify()
    b.close()
    quiet.close()


def test_emulator_and_gpu_agree(lib, cases, monkeypatch):
    """The recovered bytes do not depend on the decoder's width: the emulator with 64-thread decoders gives what the GPU
    gives with 512, for the cases under 20000 bytes."""
    D, L = lib
    monkeypatch.setenv("D4G_SIM_BLOCK", "64")
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    S = D.load_library(os.path.join(ROOT, "tests", "hostsim", "libdeft4g_hostsim.so"))
    D.init(0, lib=S)
    streams = [c.data for c in cases if len(c.data) < 20000 and len(c.expected) < 20000]      # (the emulator is slow)
    assert len(streams) > 150
    assert D.recover_streams(streams, lib=S) == D.recover_streams(streams)


def test_device_memory(lib, cases):
    """live device blocks: equal before a batch is created and after it is destroyed, whether recovery ran or was refused;
    a batch without failed streams launches and allocates nothing"""
    D, L = lib
    cs = R.by_name(LANES, ["bad_symbol_in_batch_1", "distance_171_in_block_2", "distance_k_ok", "empty_input"])
    base = live_blocks(L)
    b = D.Batch([c.data for c in cs])
    n = ctypes.c_size_t(7)
    assert L.d4g_batch_recover(b.h) == -2 and L.d4g_last_error() == b"the batch has not been parsed"
    b.parse()
    held = live_blocks(L)
    assert L.d4g_batch_copy_recovered(b.h, 4, None, 0, ctypes.byref(n)) == -2 and L.d4g_last_error() == b"bad stream index"
    assert L.d4g_batch_copy_recovered(None, 0, None, 0, ctypes.byref(n)) == -2 and L.d4g_batch_recover(None) == -2
    assert live_blocks(L) == held
    assert [b.recovered(i) for i in range(4)] == [c.expected for c in cs]
    assert live_blocks(L) == held + 1                    # the recovered bytes, and nothing else, stay with the batch
    b.close()
    assert live_blocks(L) == base
    assert [g for g, _ in D.recover_streams([c.data for c in cs])] == [c.expected for c in cs]
    assert L.d4g_recover_streams(2, None, None, None, None, None) == -2
    assert live_blocks(L) == base
    t = bytes(H.text(60000, 51))
    b = D.Batch([H.z(t[:30000]), H.z(t[30000:], 1)]).run(True)
    held, st = live_blocks(L), b.stats()
    assert b.recover().recovered(1) == t[30000:]
    assert b.stats() == st and live_blocks(L) == held
    b.close()
    assert live_blocks(L) == base


def test_recover_files(lib):
    """containers.recover_files on a gzip file cut inside its last block"""
    from deft4j_amd import containers as C
    whole = open(os.path.join(ROOT, "tests", "golden", "asyoulik_asyoulik-gzip.txt.gz.file.in"), "rb").read()
    plain = gzip.decompress(whole)
    cut = whole[:len(whole) - 8 - 300]                   # the trailer and 300 bytes of the last block are gone
    got = C.recover_files([whole, cut, b"no container"])
    assert [len(g) for g in got] == [1, 1, 0]
    assert got[0][0]["complete"] and got[0][0]["error"] is None and got[0][0]["data"] == plain
    r = got[1][0]
    n = r["error"]["decoded_offset"]
    assert not r["complete"] and r["stream"] == 0 and r["error"]["reason"] == P.EOF
    assert 0 < n < len(plain) and r["data"] == plain[:n]
    g = C.GZFile()
    assert g.read(cut) and r["data"] == zlib.decompressobj(-15).decompress(g.payload)       # what zcat would have delivered
    D, L = lib
    b = D.Batch([g.payload + whole[len(cut):-8]]).parse()
    assert r["error"]["block"] == len(b.block_info(0)) - 1                                   # the cut lies in the last block
    b.close()
