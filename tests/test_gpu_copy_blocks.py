"""Decoded bytes by block-local copies with window markers against pointer jumping (D4G_COPY=blocks / doubling / auto) on
the GPU: the cases of tests/copy_blocks_cases.py, each optimised under both paths."""
import ctypes
import zlib

import pytest

import copy_blocks_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import deft4j_amd as D
    return D, D.init(0)


def live_blocks(L):
    n = ctypes.c_int64(-1)
    assert L.d4g_debug_device_blocks(ctypes.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("name", [c.name for c in C.all_cases()])
def test_case(lib, name):
    D, L = lib
    c = next(c for c in C.all_cases() if c.name == name)
    C.check_case(D, L, c, run=True)        # (the pool keeps what a first run of this size took)
    base = live_blocks(L)
    assert not C.check_case(D, L, c, run=True)
    assert live_blocks(L) == base


def test_mixed_batch(lib, monkeypatch):
    """both paths in one parse: a stream past a bound beside ordinary ones and a failing one"""
    D, L = lib
    cs = {c.name: c for c in C.all_cases()}
    pick = [cs[k] for k in ("forty_small_blocks", "block_past_byte_bound", "before_stream_start", "reptext_1MiB", "block_past_token_bound",
                            "empty_stream")]
    monkeypatch.setenv("D4G_COPY", "auto")
    outs = []
    for rep in range(2):
        base = live_blocks(L)
        b = D.Batch([c.data for c in pick], lib=L).run(True)
        st = b.stats()
        assert st["copy_segments"] >= 4 + 2 + 1 and st["copy_rounds"] >= 2 and st["jump_rounds"] > 0
        for i, c in enumerate(pick):
            if c.fails:
                assert b.result(i)["status"] == -1 and b.parse_error(i)["reason"] == C.DISTANCE_TOO_FAR
            else:
                assert b.decoded(i) == c.plain == zlib.decompress(c.data, -15), c.name
                assert zlib.decompress(b.output(i), -15) == c.plain
        outs.append([b.output(i) for i, c in enumerate(pick) if not c.fails])
        b.close()
        if rep:
            assert live_blocks(L) == base
    assert outs[0] == outs[1]
