"""Where and why a DEFLATE stream fails to parse (d4g_batch_parse_error, d4g_diagnose_streams, k_diagnose_blocks)
through the HIP kernels in the CPU emulator (tests/hostsim), with block decoders of 64 and of 128 threads.  Every
expected record comes from the case builder (tests/parse_error_cases.py), none from the library."""
import ctypes
import os
import subprocess

import pytest

import handbuilt_cases as H
import parse_error_cases as P

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


def record(r):
    return {k: r[k] for k in P.FIELDS}


def live_blocks(L):
    n = ctypes.c_int64(-1)
    assert L.d4g_debug_device_blocks(ctypes.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("lanes", [64, 128])
def test_every_case_as_one_batch(sim, monkeypatch, lanes):
    """d4g_diagnose_streams on all cases at once: one launch, one workgroup per failed stream"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", str(lanes))
    D, L = sim
    cs = P.cases(lanes)
    got = D.diagnose_streams([c.data for c in cs], lib=L)
    bad = [(c.name, record(g), c.want) for c, g in zip(cs, got) if record(g) != c.want]
    assert not bad
    assert all(g["reason_name"] == P.NAMES[g["reason"]] == D.PARSE_REASON_NAMES[g["reason"]] == L.d4g_parse_reason_name(g["reason"]).decode()
               for g in got)
    assert L.d4g_parse_reason_name(99) == b"UNKNOWN"
    assert {c.want["reason"] for c in cs} == set(range(8))     # every reason is covered


@pytest.mark.parametrize("lanes", [64, 128])
def test_every_case_alone_after_parse_and_run(sim, monkeypatch, lanes):
    """Batch.parse_error after d4g_batch_parse and after d4g_batch_run: a stream's answer does not depend on its
    neighbours, and whether it parses is what it was"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", str(lanes))
    D, L = sim
    bad = []
    for k, c in enumerate(P.cases(lanes)):
        if len(c.data) > 8192 and lanes == 128:    # (the long blocks ran alone with 64 threads)
            continue
        b = D.Batch([c.data], lib=L)
        b.parse() if k % 2 else b.run(True)
        r = b.parse_error(0)
        if record(r) != c.want or (b.result(0)["status"] < 0) != (c.want["reason"] != 0):
            bad.append((c.name, record(r), c.want))
        assert b.parse_error(0) == r               # the cached answer
        b.close()
    assert not bad


def test_case_builder_against_zlib():
    """guards the case builder, not the library: where deft4j and zlib agree, zlib names the same failure"""
    for c in P.cases(64):
        msg = P.zlib_error(c.data)
        if c.want["reason"] in P.ZLIB_SAYS and c.rfc_before:
            assert msg is not None and P.ZLIB_SAYS[c.want["reason"]] in msg, (c.name, msg)
        elif c.want["reason"] == P.OK:
            assert msg is None, (c.name, msg)


def test_mixed_batch(sim, monkeypatch):
    """12 streams, 5 failing for different reasons: per-stream answers equal the single-stream ones, and the valid
    streams optimise to the bytes they give in a batch of their own"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    D, L = sim
    cs, good = P.mixed_batch(64)
    assert len(cs) == 12 and len({c.want["reason"] for c in cs if c.want["reason"]}) == 5
    b = D.Batch([c.data for c in cs], lib=L).run(True)
    before = b.stats()["kernel_launches"]
    got = [b.parse_error(i) for i in range(len(cs))]
    assert b.stats()["kernel_launches"] == before + 1          # one launch for the whole batch
    assert [b.parse_error(i) for i in range(len(cs))] == got
    assert b.stats()["kernel_launches"] == before + 1          # and none for a second round of questions
    assert [record(g) for g in got] == [c.want for c in cs]
    alone = [D.diagnose_streams([c.data], lib=L)[0] for c in cs]
    assert alone == got
    g = D.Batch(good, lib=L).run(True)
    outs = {bytes(s): (g.result(i), g.output(i)) for i, s in enumerate(good)}
    for i, c in enumerate(cs):
        if c.want["reason"] == 0:
            assert (b.result(i), b.output(i)) == outs[c.data], c.name
        else:
            assert b.result(i)["status"] == -1
    b.close()
    g.close()


def test_no_cost_when_nothing_failed(sim):
    D, L = sim
    t = bytes(H.text(6000, 51))
    streams = [H.z(t[:3000]), H.z(t[3000:], 1), P.Track().fixed(list(t[:40]), final=True).value()]
    base = live_blocks(L)
    b = D.Batch(streams, lib=L).run(True)
    held = live_blocks(L)
    st = b.stats()
    assert [b.parse_error(i)["reason"] for i in range(3)] == [0, 0, 0]
    assert b.stats() == st and live_blocks(L) == held          # no launch, no allocation
    b.close()
    assert live_blocks(L) == base
    # the one-shot call gives every block back, with failed streams too; a refused call takes none
    cs = P.by_name(64, ["btype3_block_1", "bad_symbol_in_chunk_5", "distance_k_ok", "empty_input"])
    assert [r["reason"] for r in D.diagnose_streams([c.data for c in cs], lib=L)] == [c.want["reason"] for c in cs]
    assert live_blocks(L) == base
    assert L.d4g_diagnose_streams(2, None, None, None) == -2 and L.d4g_last_error() == b"null argument"
    assert L.d4g_batch_parse_error(None, 0, None) == -2
    assert live_blocks(L) == base
    b = D.Batch(streams, lib=L)
    assert L.d4g_batch_parse_error(b.h, 0, ctypes.byref(D.d4g_parse_error())) == -2     # not parsed yet
    b.parse()
    assert L.d4g_batch_parse_error(b.h, 3, ctypes.byref(D.d4g_parse_error())) == -2     # no such stream
    b.close()
    assert live_blocks(L) == base


def test_encoder_batch_answers_ok(sim):
    D, L = sim
    e = D.EncodeBatch([bytes(H.text(3000, 52))], [(0, D.ENC_JVM, D.STRATEGY_DEFAULT)], lib=L).run(False)
    assert record(e.parse_error(0)) == P.NONE
    e.close()


def test_valid_streams_are_ok(sim):
    """every golden input and every valid hand-built stream that is small enough for the emulator"""
    D, L = sim
    vs = P.valid_streams(max_len=50000)
    assert len(vs) > 60
    got = D.diagnose_streams([d for _, d in vs], lib=L)
    assert not [(n, g) for (n, _), g in zip(vs, got) if record(g) != P.NONE]


def test_every_prefix(sim):
    """every bit-prefix of two mixed streams: OK exactly where the corpus says it parses; else a reason and positions in range"""
    D, L = sim
    cs = H.prefixes()
    got = D.diagnose_streams([c.data for c in cs], lib=L)
    bad = []
    for c, g in zip(cs, got):
        if c.ok:
            good = record(g) == P.NONE
        else:
            good = g["reason"] > 0 and 0 <= g["block_bit_pos"] <= g["bit_pos"] <= 8 * len(c.data) and g["block"] >= 0 and \
                g["decoded_offset"] >= 0
        if not good:
            bad.append((c.name, g))
    assert not bad
    assert len({g["reason"] for g in got}) >= 3


def test_explain_failures(sim):
    """containers.explain_failures names the file, the stream and the stream's name; optimise_files is what it was: the
    readable file comes out as its golden output with its transcript, the PNG with the broken IDAT is answered with "Failed to read file" alone"""
    from deft4j_amd import containers as C
    D, L = sim
    gz_in, gz_out, lines, merge = P.golden_file("lz-twice-twice.txt.gz")
    png, want = P.png_with_bad_idat()
    files = [gz_in, png, b"\x00\x01garbage"]
    got = C.explain_failures(files, lib=L)
    assert len(got) == 1 and (got[0]["file"], got[0]["stream"], got[0]["name"]) == (1, 0, "IDAT chunk")
    assert record(got[0]["error"]) == want and got[0]["error"]["reason_name"] == "LITLEN_SYMBOL"
    assert C.explain_failures([gz_in], lib=L) == [] and C.explain_failures([b"junk"], lib=L) == []
    assert C.optimise_files(files, merge, lib=L) == [(gz_out, lines), (None, ["Failed to read file"]), (None, ["Failed to read file"])]
