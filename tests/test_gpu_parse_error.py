"""Where and why a DEFLATE stream fails to parse, on the GPU through the C ABI (d4g_batch_parse_error,
d4g_diagnose_streams, k_diagnose_blocks with 512-thread block decoders): the cases of tests/parse_error_cases.py, whose
expected records come from the case builder alone; every valid stream the suite has; every bit-prefix of two mixed
streams; and the emulator's records next to the GPU's."""
import ctypes
import os

import pytest

import handbuilt_cases as H
import parse_error_cases as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = 512


@pytest.fixture(scope="module")
def lib():
    import deft4j_amd as D
    return D, D.init(0)


def record(r):
    return {k: r[k] for k in P.FIELDS}


def live_blocks(L):
    n = ctypes.c_int64(-1)
    assert L.d4g_debug_device_blocks(ctypes.byref(n)) == 0
    return n.value


def test_every_case_as_one_batch(lib):
    """one d4g_diagnose_streams call: one launch, one workgroup per failed stream"""
    D, L = lib
    cs = P.cases(LANES)
    got = D.diagnose_streams([c.data for c in cs])
    assert not [(c.name, record(g), c.want) for c, g in zip(cs, got) if record(g) != c.want]
    assert all(g["reason_name"] == P.NAMES[g["reason"]] == L.d4g_parse_reason_name(g["reason"]).decode() for g in got)
    assert {c.want["reason"] for c in cs} == set(range(8))
    second = [c for c in cs if c.want["bit_pos"] > 3 + LANES * P.CHUNK]     # failures in the second batch of a 512-thread decoder
    assert len(second) >= 2 and all(len(c.data) > 32768 for c in second)


def test_every_case_alone_after_parse_and_run(lib):
    """a stream's answer does not depend on its neighbours or on the call that parsed it, and whether it parses is what it was"""
    D, L = lib
    bad = []
    for k, c in enumerate(P.cases(LANES)):
        b = D.Batch([c.data])
        b.parse() if k % 2 else b.run(True)
        r = b.parse_error(0)
        if record(r) != c.want or (b.result(0)["status"] < 0) != (c.want["reason"] != 0) or b.parse_error(0) != r:
            bad.append((c.name, record(r), c.want))
        b.close()
    assert not bad


def test_after_run_recompress(lib):
    D, L = lib
    cs = P.by_name(LANES, ["distance_171_in_block_2", "distance_170_in_block_2", "eof_in_lenextra"])
    b = D.Batch([c.data for c in cs]).run_recompress(D.MODE_CHEAP, True)
    assert [record(b.parse_error(i)) for i in range(len(cs))] == [c.want for c in cs]
    b.close()


def test_mixed_batch(lib):
    """12 streams, 5 failing for different reasons: per-stream answers equal the single-stream ones, one launch for the
    batch, and the valid streams optimise to the bytes they give in a batch of their own"""
    D, L = lib
    cs, good = P.mixed_batch(LANES)
    b = D.Batch([c.data for c in cs]).run(True)
    before = b.stats()["kernel_launches"]
    got = [b.parse_error(i) for i in range(len(cs))]
    assert [b.parse_error(i) for i in range(len(cs))] == got
    assert b.stats()["kernel_launches"] == before + 1
    assert [record(g) for g in got] == [c.want for c in cs]
    assert [D.diagnose_streams([c.data])[0] for c in cs] == got
    g = D.Batch(good).run(True)
    outs = {bytes(s): (g.result(i), g.output(i)) for i, s in enumerate(good)}
    for i, c in enumerate(cs):
        if c.want["reason"] == 0:
            assert (b.result(i), b.output(i)) == outs[c.data], c.name
        else:
            assert b.result(i)["status"] == -1
    b.close()
    g.close()


def test_no_cost_when_nothing_failed(lib):
    D, L = lib
    t = bytes(H.text(60000, 51))
    streams = [H.z(t[:30000]), H.z(t[30000:], 1), P.Track().fixed(list(t[:40]), final=True).value()]
    base = live_blocks(L)
    b = D.Batch(streams).run(True)
    held, st = live_blocks(L), b.stats()
    assert [b.parse_error(i)["reason"] for i in range(3)] == [0, 0, 0]
    assert b.stats()["kernel_launches"] == st["kernel_launches"] and b.stats() == st and live_blocks(L) == held
    b.close()
    assert live_blocks(L) == base
    cs = P.by_name(LANES, ["btype3_block_1", "bad_symbol_in_batch_1", "distance_k_ok", "empty_input"])
    assert [r["reason"] for r in D.diagnose_streams([c.data for c in cs])] == [c.want["reason"] for c in cs]
    assert live_blocks(L) == base
    assert L.d4g_diagnose_streams(2, None, None, None) == -2 and L.d4g_last_error() == b"null argument"
    assert L.d4g_batch_parse_error(None, 0, None) == -2
    assert live_blocks(L) == base


def test_valid_streams_are_ok(lib):
    """every golden input and every valid hand-built stream, the large ones included"""
    D, L = lib
    vs = P.valid_streams()
    got = D.diagnose_streams([d for _, d in vs])
    assert len(vs) > 90 and not [(n, g) for (n, _), g in zip(vs, got) if record(g) != P.NONE]


def test_every_prefix(lib):
    D, L = lib
    cs = H.prefixes()
    got = D.diagnose_streams([c.data for c in cs])
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


@pytest.mark.parametrize("part", range(8))
def test_emulator_and_gpu_agree(lib, monkeypatch, part):
    """The records do not depend on the decoder's width: the emulator with 64-thread decoders gives what the GPU gives
    with 512, for the cases laid out for 512 threads and for every prefix (the emulator is slow: eight slices, the
    cases with the first)."""
    D, L = lib
    monkeypatch.setenv("D4G_SIM_BLOCK", "64")
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    S = D.load_library(os.path.join(ROOT, "tests", "hostsim", "libdeft4g_hostsim.so"))
    D.init(0, lib=S)
    streams = ([c.data for c in P.cases(LANES)] if part == 0 else []) + [c.data for c in H.prefixes()[part::8]]
    assert D.diagnose_streams(streams, lib=S) == D.diagnose_streams(streams)


def test_explain_failures(lib):
    from deft4j_amd import containers as C
    gz_in, gz_out, lines, merge = P.golden_file("lz-twice-twice.txt.gz")
    png, want = P.png_with_bad_idat()
    files = [gz_in, png]
    got = C.explain_failures(files)
    assert len(got) == 1 and (got[0]["file"], got[0]["stream"], got[0]["name"]) == (1, 0, "IDAT chunk")
    assert record(got[0]["error"]) == want
    assert C.optimise_files(files, merge) == [(gz_out, lines), (None, ["Failed to read file"])]
