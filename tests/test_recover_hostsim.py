"""The bytes that decode before a stream's first failure (d4g_batch_recover, d4g_batch_copy_recovered,
d4g_recover_streams, k_recover_count / k_recover_emit) through the HIP kernels in the CPU emulator (tests/hostsim), with
block decoders of 64 and of 128 threads.  Every expected byte and record comes from the case builder
(tests/recover_cases.py): zlib for the truncated streams, the builder's own token bytes for the corrupted ones."""
import ctypes
import os
import subprocess

import pytest

import handbuilt_cases as H
import parse_error_cases as P
import recover_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    os.environ["D4G_SIM_BLOCK"] = "64"
    so = os.path.join(ROOT, "tests", "hostsim", "libdeft4g_hostsim.so")
    subprocess.check_call([os.path.join(ROOT, "tests", "hostsim", "build.sh")])
    import deft4j_amd as D
    L = D.load_library(so)
    D.init(0, lib=L)
    return D, L


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


def all_cases(lanes):
    return R.corruption_cases(lanes) + R.truncation_cases()


@pytest.mark.parametrize("lanes", [64, 128])
def test_every_case_as_one_batch(sim, monkeypatch, lanes):
    """one batch, one recovery for all its failed streams; the diagnosis is what it was before anybody asked for bytes"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", str(lanes))
    D, L = sim
    cs = all_cases(lanes)
    b = D.Batch([c.data for c in cs], lib=L).parse()
    before = [b.parse_error(i) for i in range(len(cs))]
    got = [b.recovered(i) for i in range(len(cs))]
    st = b.stats()
    assert [b.recovered(i) for i in range(len(cs))] == got and b.stats() == st       # kept, not made again
    assert [b.parse_error(i) for i in range(len(cs))] == before
    bad = [(c.name, w) for c, g, e in zip(cs, got, before) for w in [wrong(c, g, e)] if w]
    assert not bad
    failed = [c for c in cs if c.want["reason"] != P.OK and c.want["decoded_offset"] > 0]
    assert st["recover_streams"] == len(failed) and st["recover_bytes"] == sum(len(c.expected) for c in failed)
    for i, c in enumerate(cs):                           # copy_decoded answers what it answered
        if c.want["reason"] == P.OK:
            assert b.decoded(i) == c.expected
        else:
            assert L.d4g_batch_copy_decoded(b.h, i, None, 0, None) == -2 and L.d4g_last_error() == b"stream did not parse"
    b.close()
    assert D.recover_streams([c.data for c in cs], lib=L) == list(zip(got, before))
    assert {c.want["reason"] for c in cs} == set(range(8))
    assert sum(1 for c in cs if c.want["reason"] and not c.expected) >= 8 and sum(1 for c in cs if len(c.expected) > 32768) >= 1


@pytest.mark.parametrize("lanes", [64, 128])
def test_every_case_alone(sim, monkeypatch, lanes):
    """a stream's recovered bytes do not depend on its neighbours, nor on whether the batch parsed or ran"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", str(lanes))
    D, L = sim
    bad = []
    for k, c in enumerate(all_cases(lanes)):
        if len(c.data) > 8192 and lanes == 128:          # (the long blocks ran alone with 64 threads)
            continue
        b = D.Batch([c.data], lib=L)
        b.parse() if k % 2 else b.run(True)
        w = wrong(c, b.recovered(0), b.parse_error(0))
        if w:
            bad.append((c.name, w))
        b.close()
    assert not bad


def test_copy_paths_agree(sim, monkeypatch):
    """block-local copies and byte doubling give the same recovered bytes"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    D, L = sim
    cs = R.by_name(64, ["copies_reach_32768_across_segments", "overlap_dist_1_len_258_last", "overlap_dist_3_len_10_last",
                        "distance_171_in_block_2", "bad_symbol_behind_scan_and_exact", "eof_in_distextra"]) + R.truncation_cases()[::7]
    for mode in ("blocks", "doubling"):
        monkeypatch.setenv("D4G_COPY", mode)
        got = D.recover_streams([c.data for c in cs], lib=L)
        assert not [(mode, c.name, w) for c, (g, e) in zip(cs, got) for w in [wrong(c, g, e)] if w]


def test_mixed_batch(sim, monkeypatch):
    """12 streams, 5 of them failing: the valid streams' results and outputs are those of a batch that never asked, whether
    recovery is asked for before the run's results are read or after"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    D, L = sim
    cs, good = R.mixed_batch(64)
    g = D.Batch(good, lib=L).run(True)
    outs = {bytes(s): (g.result(i), g.output(i), g.decoded(i), g.checksums(i)) for i, s in enumerate(good)}
    g.close()
    quiet = D.Batch([c.data for c in cs], lib=L).run(True)
    b = D.Batch([c.data for c in cs], lib=L).run(True)
    launches = b.stats()["kernel_launches"]
    b.recover()
    assert b.stats()["kernel_launches"] > launches
    launches = b.stats()["kernel_launches"]
    b.recover()
    assert b.stats()["kernel_launches"] == launches      # idempotent
    for i, c in enumerate(cs):
        assert wrong(c, b.recovered(i), b.parse_error(i)) is None, c.name
        assert b.result(i) == quiet.result(i)
        if c.want["reason"] == P.OK:
            assert (b.result(i), b.output(i), b.decoded(i), b.checksums(i)) == outs[c.data], c.name
            assert b.recovered(i) == b.decoded(i)
        else:
            assert b.result(i)["status"] == -1
    assert b.verify() == quiet.verify()
    b.close()
    quiet.close()


def test_no_cost_when_nothing_failed(sim):
    D, L = sim
    t = bytes(H.text(6000, 51))
    streams = [H.z(t[:3000]), H.z(t[3000:], 1), P.Track().fixed(list(t[:40]), final=True).value()]
    base = live_blocks(L)
    b = D.Batch(streams, lib=L).run(True)
    held, st = live_blocks(L), b.stats()
    b.recover()
    assert [b.recovered(i) for i in range(3)] == [t[:3000], t[3000:], t[:40]]
    assert b.stats() == st and live_blocks(L) == held   # no launch, no allocation
    b.close()
    assert live_blocks(L) == base
    # failed streams whose failure lies in the first element need no side batch either
    cs = R.by_name(64, ["empty_input", "btype3_block_0", "distance_1_first_token"])
    b = D.Batch([c.data for c in cs], lib=L).parse()
    assert [b.parse_error(i)["decoded_offset"] for i in range(3)] == [0, 0, 0]
    held, launches = live_blocks(L), b.stats()["kernel_launches"]
    assert [b.recovered(i) for i in range(3)] == [b"", b"", b""]
    assert live_blocks(L) == held and b.stats()["kernel_launches"] == launches and b.stats()["recover_streams"] == 0
    b.close()
    assert live_blocks(L) == base


def test_device_blocks_and_refusals(sim, monkeypatch):
    """every device block comes back: after a recovery, after a one-shot call, after a refused call"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    D, L = sim
    cs = R.by_name(64, ["bad_symbol_in_chunk_5", "distance_171_in_block_2", "distance_k_ok", "empty_input"])
    base = live_blocks(L)
    b = D.Batch([c.data for c in cs], lib=L)
    n = ctypes.c_size_t(7)
    assert L.d4g_batch_recover(b.h) == -2 and L.d4g_last_error() == b"the batch has not been parsed"
    assert L.d4g_batch_copy_recovered(b.h, 0, None, 0, ctypes.byref(n)) == -2
    b.parse()
    held = live_blocks(L)
    assert L.d4g_batch_copy_recovered(b.h, 4, None, 0, ctypes.byref(n)) == -2 and L.d4g_last_error() == b"bad stream index"
    assert L.d4g_batch_copy_recovered(None, 0, None, 0, ctypes.byref(n)) == -2 and L.d4g_batch_recover(None) == -2
    assert live_blocks(L) == held
    buf = ctypes.create_string_buffer(4)
    assert L.d4g_batch_copy_recovered(b.h, 0, buf, 4, ctypes.byref(n)) == -2 and L.d4g_last_error() == b"output buffer too small"
    assert n.value == len(cs[0].expected)
    assert [b.recovered(i) for i in range(4)] == [c.expected for c in cs]
    b.close()
    assert live_blocks(L) == base
    assert [g for g, _ in D.recover_streams([c.data for c in cs], lib=L)] == [c.expected for c in cs]
    assert D.recover_streams([], lib=L) == []
    assert live_blocks(L) == base


def test_one_shot_slots(sim):
    """d4g_recover_streams: every slot is defined whatever happens — buffers for every stream when it succeeds (an empty
    prefix is a buffer too), NULL / 0 / OK and nothing to free when it does not"""
    D, L = sim
    cs = R.by_name(64, ["empty_input", "fixed_sym_286", "distance_k_ok"])
    n = len(cs)
    arr = (ctypes.c_char_p * n)(*[c.data for c in cs])
    lens = (ctypes.c_size_t * n)(*[len(c.data) for c in cs])

    def slots():
        out = (ctypes.c_void_p * n)(*[0xdead] * n)
        olen = (ctypes.c_size_t * n)(*[777] * n)
        why = (D.d4g_parse_error * n)()
        for w in why:
            w.reason, w.decoded_offset = 99, 99
        return out, olen, why
    out, olen, why = slots()
    assert L.d4g_recover_streams(n, arr, lens, out, olen, why) == 0
    assert all(out[i] for i in range(n)) and list(olen) == [len(c.expected) for c in cs]
    assert [ctypes.string_at(out[i], olen[i]) for i in range(n)] == [c.expected for c in cs]
    assert [{k: getattr(why[i], k) for k in P.FIELDS} for i in range(n)] == [c.want for c in cs]
    for i in range(n):
        L.d4g_free(out[i])
    out, olen, _ = slots()
    assert L.d4g_recover_streams(n, arr, lens, out, olen, None) == 0 and list(olen) == [len(c.expected) for c in cs]
    for i in range(n):
        L.d4g_free(out[i])
    out, olen, why = slots()
    assert L.d4g_recover_streams(n, None, lens, out, olen, why) == -2 and L.d4g_last_error() == b"null argument"
    # a library that was never initialised refuses the call: the slots read "nothing recovered", nothing is allocated
    import deft4j_amd
    fresh = ctypes.CDLL(deft4j_amd.LIB_PATH)
    fresh.d4g_recover_streams.argtypes = L.d4g_recover_streams.argtypes
    fresh.d4g_free.argtypes = [ctypes.c_void_p]
    out, olen, why = slots()
    rc = fresh.d4g_recover_streams(n, arr, lens, out, olen, why)
    if rc == 0:                                          # (a GPU is present and another test initialised the library)
        assert list(olen) == [len(c.expected) for c in cs]
        for i in range(n):
            fresh.d4g_free(out[i])
    else:
        assert rc == -1 and not any(out[i] for i in range(n)) and list(olen) == [0] * n
        assert [(w.reason, w.decoded_offset) for w in why] == [(0, -1)] * n


def test_encoder_batch_recovers_its_decoded_bytes(sim):
    D, L = sim
    t = bytes(H.text(3000, 52))
    e = D.EncodeBatch([t], [(0, D.ENC_JVM, D.STRATEGY_DEFAULT)], lib=L).run(False)
    held = live_blocks(L)
    assert e.recover().recovered(0) == e.decoded(0)
    assert live_blocks(L) == held
    e.close()


def test_recover_files(sim, monkeypatch):
    """containers.recover_files: a gzip file cut inside its last block, a PNG with a broken IDAT, a file no reader accepts"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    import gzip
    from deft4j_amd import containers as C
    D, L = sim
    gz_in = P.golden_file("lz-twice-twice.txt.gz")[0]
    png, want = P.png_with_bad_idat()
    cut = gz_in[:len(gz_in) - 12]
    got = C.recover_files([gz_in, cut, png, b"\x00\x01garbage"], lib=L)
    whole = gzip.decompress(gz_in)
    assert [len(g) for g in got] == [1, 1, 1, 0]
    assert got[0][0]["complete"] and got[0][0]["error"] is None and got[0][0]["data"] == whole and got[0][0]["stream"] == 0
    n = got[1][0]["error"]["decoded_offset"]
    assert not got[1][0]["complete"] and 0 < n < len(whole) and got[1][0]["data"] == whole[:n] and got[1][0]["error"]["reason"] == P.EOF
    assert got[2][0]["name"] == "IDAT chunk" and {k: got[2][0]["error"][k] for k in P.FIELDS} == want
    assert got[2][0]["data"] == bytes(P.text(200, 45)[:100])
    assert C.explain_failures([png], lib=L)[0]["error"] == got[2][0]["error"]
