"""Decoded bytes by block-local copies with window markers against pointer jumping (D4G_COPY=blocks / doubling / auto)
through the HIP kernels in the CPU emulator (tests/hostsim): the cases of tests/copy_blocks_cases.py."""
import ctypes
import os
import subprocess
import zlib

import pytest

import copy_blocks_cases as C

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


@pytest.mark.parametrize("name", [c.name for c in C.all_cases()])
def test_case(sim, name):
    """(the cases marked large are parsed, the others also optimised: the search is what the emulator is slow at)"""
    D, L = sim
    c = next(c for c in C.all_cases() if c.name == name)
    base = live_blocks(L)
    assert not C.check_case(D, L, c, run=not c.large)
    assert live_blocks(L) == base


def test_two_waves_per_workgroup(sim, monkeypatch):
    """the group loop with 128 threads: other strides through the staged tokens and the ring"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "128")
    D, L = sim
    for c in C.all_cases():
        if not c.large and not c.fails:
            assert not C.check_case(D, L, c, run=False)


def test_mixed_batch(sim, monkeypatch):
    """a stream that `auto` sends the doubling way beside ordinary ones and a failing one: both paths run in one parse, every
    stream decodes as it does alone, and the device blocks all come back"""
    D, L = sim
    cs = {c.name: c for c in C.all_cases()}
    pick = [cs[k] for k in ("forty_small_blocks", "block_past_token_bound", "before_stream_start", "distance_32768", "empty_stream")]
    base = live_blocks(L)
    monkeypatch.setenv("D4G_COPY", "auto")
    b = D.Batch([c.data for c in pick], lib=L)
    b.parse()
    st = b.stats()
    assert st["copy_segments"] >= 4 + 2 + 1 and st["copy_rounds"] >= 2 and st["jump_rounds"] > 0
    for i, c in enumerate(pick):
        if c.fails:
            assert b.parse_error(i)["reason"] == C.DISTANCE_TOO_FAR
        else:
            assert b.decoded(i) == c.plain == zlib.decompress(c.data, -15), c.name
    b.close()
    assert live_blocks(L) == base
    with pytest.raises(Exception):
        monkeypatch.setenv("D4G_COPY", "sideways")
        D.Batch([pick[0].data], lib=L).parse()
    assert live_blocks(L) == base
