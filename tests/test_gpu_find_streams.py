"""zlib and gzip streams embedded in arbitrary files, on the GPU through the C ABI (d4g_find_streams with 512-thread
block decoders, k_find_wrappers, k_find_confirm, containers.EmbeddedFile): the cases of tests/find_streams_cases.py,
whose expected records come from the case builder alone, as one call and each file alone; the emulator's records next to
the GPU's; the EmbeddedFile round trip; and a 4 MiB file with 1 000 streams."""
import ctypes
import os

import pytest

import find_streams_cases as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import deft4j_amd as D
    return D, D.init(0)


def live_blocks(L):
    n = ctypes.c_int64(-1)
    assert L.d4g_debug_device_blocks(ctypes.byref(n)) == 0
    return n.value


def wrong(cs, got):
    return [(c.name, g, F.wanted(c, i)) for i, (c, g) in enumerate(zip(cs, got)) if g != F.wanted(c, i)]


def test_every_case_in_one_call(lib):
    D, L = lib
    base = live_blocks(L)
    for kinds, min_decoded, cs in F.calls():
        got, st = D.find_streams([c.data for c in cs], kinds, min_decoded, stats=True)
        assert not wrong(cs, got)
        n = sum(len(c.want) for c in cs)
        assert st["bytes_scanned"] == sum(len(c.data) for c in cs) and st["reported"] == n
        assert st["header_candidates"] >= st["first_block_ok"] >= st["parsed"] >= st["confirmed"] >= n
    assert live_blocks(L) == base


def test_every_case_alone(lib):
    """a file's answer does not depend on its neighbours in the call"""
    D, L = lib
    bad = []
    for c in F.cases():
        bad += wrong([c], D.find_streams([c.data], c.kinds, c.min_decoded))
    assert not bad


def test_emulator_and_gpu_agree(lib, monkeypatch):
    """the records do not depend on the decoder's width: the emulator with 64-thread decoders beside the GPU with 512"""
    D, L = lib
    monkeypatch.setenv("D4G_SIM_BLOCK", "64")
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    S = D.load_library(os.path.join(ROOT, "tests", "hostsim", "libdeft4g_hostsim.so"))
    D.init(0, lib=S)
    cs = [c for c in F.cases() if c.kinds == 0 and c.min_decoded == 0 and len(c.data) < 20000]
    assert len(cs) >= 17
    files = [c.data for c in cs]
    assert D.find_streams(files, lib=S) == D.find_streams(files)


@pytest.mark.parametrize("mode", [0, 1])
def test_embedded_file_round_trip(lib, mode):
    D, L = lib
    base = live_blocks(L)
    F.round_trip(D, None, mode=mode)
    assert live_blocks(L) == base


def test_many_streams(lib):
    """4 MiB, 1 000 small zlib streams between filler, 150 of them back to back: one scan tile there holds more wrapper
    headers than a workgroup's own candidate list (the rest go straight to the global list), and the streams are
    confirmed in two groups"""
    D, L = lib
    c = F.many_streams()
    dense = [w for w in c.want if w["decoded_len"] == 0]
    assert len(c.data) == 4 << 20 and len(c.want) == 1000 and len(dense) == 150 and dense[149]["offset"] - dense[0]["offset"] == 149 * 8
    got, st = D.find_streams([c.data], stats=True)
    assert not wrong([c], got)
    assert st["reported"] == 1000 and st["header_candidates"] > 2000 and st["bytes_scanned"] == 4 << 20
