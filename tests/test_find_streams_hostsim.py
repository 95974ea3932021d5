"""zlib and gzip streams embedded in arbitrary files (d4g_find_streams, k_find_wrappers, k_find_confirm,
containers.EmbeddedFile) through the HIP kernels in the CPU emulator (tests/hostsim), with block decoders of 64 and of
128 threads.  Every expected record comes from the case builder (tests/find_streams_cases.py), none from the library."""
import ctypes
import os
import subprocess
import zlib

import pytest

import find_streams_cases as F
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


def live_blocks(L):
    n = ctypes.c_int64(-1)
    assert L.d4g_debug_device_blocks(ctypes.byref(n)) == 0
    return n.value


def wrong(cs, got):
    """the cases whose file (index = position in the call) did not give the builder's records"""
    return [(c.name, g, F.wanted(c, i)) for i, (c, g) in enumerate(zip(cs, got)) if g != F.wanted(c, i)]


def test_case_builder_against_zlib():
    """guards the case builder, not the library: Python zlib at every offset whose header predicate holds, its own
    trailer check, then the overlap rule, names exactly the builder's streams"""
    for c in list(F.cases()) + [F.copies(8), F.copies(64)]:
        want = [(w["kind"], w["offset"], w["total_len"], w["decoded_len"], w["crc32"], w["adler32"]) for w in c.want]
        assert F.brute_force(c.data, c.kinds, c.min_decoded) == want, c.name
    names = {c.name for c in F.cases()}
    assert len(names) == 25 and sum(len(c.want) for c in F.cases()) == 156


@pytest.mark.parametrize("lanes", [64, 128])
def test_every_case_in_one_call(sim, monkeypatch, lanes):
    """the cases that share their options as one call: the records equal the builder's, and every offset was looked at"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", str(lanes))
    D, L = sim
    for kinds, min_decoded, cs in F.calls():
        if lanes == 128:
            cs = [c for c in cs if c.name != "long_block"]          # (the long block ran with 64 threads)
        got, st = D.find_streams([c.data for c in cs], kinds, min_decoded, lib=L, stats=True)
        assert not wrong(cs, got)
        assert all(set(g) == set(F.FIELDS) for f in got for g in f)
        assert st["bytes_scanned"] == sum(len(c.data) for c in cs)
        n = sum(len(c.want) for c in cs)
        assert st["reported"] == n and st["header_candidates"] >= st["first_block_ok"] >= st["parsed"] >= st["confirmed"] >= n


def test_every_case_alone(sim, monkeypatch):
    """a file's answer does not depend on its neighbours in the call"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    D, L = sim
    bad = []
    for c in F.cases():
        if c.name == "long_block" or c.name.startswith("mixed_200k"):
            continue                                                # (slow in the emulator: they ran in the calls above)
        got = D.find_streams([c.data], c.kinds, c.min_decoded, lib=L)
        bad += wrong([c], got)
    assert not bad
    two = F.by_name("back_to_back", "no_streams", "empty_file", "stream_in_a_stored_block")
    assert not wrong(two, D.find_streams([c.data for c in two], lib=L))
    assert not wrong(two[::-1], D.find_streams([c.data for c in two[::-1]], lib=L))


def test_reported_streams_inflate(sim, monkeypatch):
    """for every reported stream d4g_inflate(file[payload_offset:]) consumes payload_len, and its bytes give the
    reported checksums"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    D, L = sim
    cs = F.by_name("multi_block", "back_to_back", "gzip_all_optional_fields", "stream_in_a_stored_block", "empty_stream_min_0", "ends_on_last_byte")
    n = 0
    for c, found in zip(cs, D.find_streams([c.data for c in cs], lib=L)):
        for f in found:
            s = D.DeflateStream(lib=L)
            assert s.parse(c.data[f["payload_offset"]:]) and s.consumed == f["payload_len"], (c.name, f)
            plain = s.getUncompressedData()
            assert (len(plain), zlib.adler32(plain), zlib.crc32(plain)) == (f["decoded_len"], f["adler32"], f["crc32"])
            assert D.Deft.getSizeBitsFallback(c.data[f["payload_offset"]:f["payload_offset"] + f["payload_len"]], lib=L) == f["size_bits"]
            n += 1
    assert n == 11


def test_launches_do_not_grow_with_candidates(sim, monkeypatch):
    """64 embedded copies of one stream cost no more kernel launches than 8 copies: every live chain of every file goes
    in one launch per step, and both files are decoded as one group.  The allowance of 4 is for the scan's second
    attempt when a candidate list overflows (k_scan_headers, k_find_wrappers) and for the compose rounds of the
    block-local copy, none of which depends on the number of candidates here."""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    D, L = sim
    few, many = F.copies(8), F.copies(64)
    gf, sf = D.find_streams([few.data], lib=L, stats=True)
    gm, sm = D.find_streams([many.data], lib=L, stats=True)
    assert not wrong([few], gf) and not wrong([many], gm)
    assert sf["header_candidates"] == sf["reported"] == 8 and sm["header_candidates"] == sm["reported"] == 64
    assert sm["kernel_launches"] <= sf["kernel_launches"] + 4, (sf, sm)


def test_device_blocks_and_refusals(sim, monkeypatch):
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    D, L = sim
    base = live_blocks(L)
    cs = F.by_name("back_to_back", "distance_before_payload", "4k_of_78_9c", "empty_file")
    assert not wrong(cs, D.find_streams([c.data for c in cs], lib=L))
    assert live_blocks(L) == base
    found, n = ctypes.POINTER(D.d4g_found_stream)(), ctypes.c_size_t(77)
    arr = (ctypes.c_char_p * 1)(cs[0].data)
    lens = (ctypes.c_size_t * 1)(len(cs[0].data))
    assert L.d4g_find_streams(1, arr, lens, None, None, ctypes.byref(n), None) == -2 and L.d4g_last_error() == b"null argument"
    assert L.d4g_find_streams(1, arr, lens, None, ctypes.byref(found), None, None) == -2
    assert L.d4g_find_streams(1, None, lens, None, ctypes.byref(found), ctypes.byref(n), None) == -2
    assert L.d4g_find_streams(1, arr, None, None, ctypes.byref(found), ctypes.byref(n), None) == -2
    big = (ctypes.c_size_t * 1)(1 << 31)                             # refused before a byte is read
    assert L.d4g_find_streams(1, arr, big, None, ctypes.byref(found), ctypes.byref(n), None) == -2
    assert L.d4g_find_streams(1, arr, lens, ctypes.byref(D.d4g_find_options(1 << 3, 0, 0)), ctypes.byref(found), ctypes.byref(n), None) == -2
    assert L.d4g_find_streams(1, arr, lens, ctypes.byref(D.d4g_find_options(0, 0, -1)), ctypes.byref(found), ctypes.byref(n), None) == -2
    assert not found and n.value == 77 and live_blocks(L) == base
    assert L.d4g_find_streams(1, arr, lens, None, ctypes.byref(found), ctypes.byref(n), None) == 0 and n.value == 3   # NULL options and stats
    assert [found[k].offset for k in range(3)] == [w["offset"] for w in cs[0].want]
    L.d4g_free(found)
    assert L.d4g_find_streams(0, None, None, None, ctypes.byref(found), ctypes.byref(n), None) == 0 and n.value == 0 and not found
    assert live_blocks(L) == base
    assert "d4g_find_streams" in D.EXPORTS


def test_embedded_file_round_trip(sim, monkeypatch):
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    D, L = sim
    base = live_blocks(L)
    lines = F.round_trip(D, L)
    named = [x[x.index("(") + 1:-1] for x in lines if " bits saved in stream " in x]
    assert named and set(named) <= {"%s stream at %d" % (w["kind_name"], w["offset"]) for w in F.by_name("back_to_back")[0].want}
    assert live_blocks(L) == base
    from deft4j_amd import containers as C
    assert C.detect(F.by_name("ends_on_last_byte")[0].data) is None                      # never chosen by itself
    assert C.explain_failures([F.by_name("back_to_back")[0].data], formats=["embedded"], lib=L) == []
    assert C.EmbeddedFile().min_decoded == 64 and C.EmbeddedFile.file_type == "Embedded streams"


def test_existing_containers_unchanged(sim, monkeypatch):
    """the golden gzip and PNG files still give their golden outputs and transcripts through the auto-detect path"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    from deft4j_amd import containers as C
    D, L = sim
    for stem in ("lz-twice-twice.txt.gz", "text.png"):
        f_in, f_out, lines, merge = P.golden_file(stem)
        assert C.optimise_files([f_in], merge, lib=L) == [(f_out, lines)], stem
