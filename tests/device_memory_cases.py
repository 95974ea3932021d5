"""Calls after which the device-memory pool must be where it was (d4g_debug_device_blocks): shared by the emulator test
(test_device_memory_hostsim.py) and the GPU test (test_gpu_device_memory.py).  Every case closes the batches it makes;
the failing ones are refused or raised by the host code, nothing goes wrong on the device."""
import ctypes
import os
import zlib

import pytest

import abi_calls
import handbuilt_cases as H

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def live_blocks(L):
    n = ctypes.c_int64(-1)
    assert L.d4g_debug_device_blocks(ctypes.byref(n)) == 0
    return n.value


def text():
    return zlib.decompress(open(os.path.join(G, "asyoulik_asyoulik-gzip.s00.in.deflate"), "rb").read(), -15)


def small_subset():
    small = {c.name for c in H.cases("small")}
    return [c.data for c in H.by_name([n for n in H.SUBSET if n in small])]


def warm_up(D, L):
    """What lives as long as the library (the search programs and tables) is made by the first batch."""
    D.Batch([H.by_name(["hlit_288"])[0].data], lib=L).run(True).close()
    return live_blocks(L)


# ---- calls that succeed ----
def run_merge(D, L, env):
    D.Batch(small_subset(), lib=L).run(True).close()


def run_no_merge(D, L, env):
    D.Batch(small_subset(), lib=L).run(False).close()


def deflate_level_1(D, L, env):
    D.deflate_streams([text()[:5000]], lib=L, level=1)


def deflate_level_9(D, L, env):
    D.deflate_streams([text()[:5000]], lib=L, level=9)


def zopfli(D, L, env):
    D.zopfli_streams([text()[:12000]], 3, lib=L)


def zopfli_growing_pool(D, L, env):
    env("D4G_ZF_POOL_WORDS", "64")
    D.zopfli_streams([text()[:12000]], 3, lib=L)


def recompress_cheap(D, L, env):
    streams = [H.by_name(["zlib1_sync_then_stored_nlen_cut"])[0].data, H.stored_after_huffman()]
    D.recompress_streams(streams, D.MODE_CHEAP, True, lib=L)


def verify_and_block_info(D, L, env):
    b = D.Batch([open(os.path.join(G, "text.s02.in.deflate"), "rb").read()], lib=L).run(True)
    assert b.result(0)["saved_bits"] > 0                      # a rewritten stream
    assert b.verify()[0]["verdict"] == 0
    assert b.block_info(0, final=True) and b.block_info(0, final=False)
    b.close()


def one_shot_with_a_corrupt_stream(D, L, env):
    rc, res = abi_calls.optimise_streams(L, [H.stored_after_huffman(), b"\x07garbage", H.by_name(["hlit_288"])[0].data], True)
    assert rc == 0 and res[1][0] < 0 and res[0][0] == 0


# ---- calls the host refuses or fails by itself ----
def levels_chain_lookup(D, L, env):
    """the level executor on the tiny dynamic blocks it cannot follow: raised in phase 1, with the whole working set made"""
    env("D4G_EXEC", "levels")
    for c in H.by_name(H.LEVEL_EXEC_BAD):
        b = D.Batch([c.data], lib=L)
        with pytest.raises(RuntimeError, match="phase1: chain lookup failed"):
            b.run(True)
        b.close()


def encoder_level_0(D, L, env):
    with pytest.raises(RuntimeError, match="level 0 is not supported"):
        D.deflate_streams([text()[:5000]], lib=L, level=0)


def zopfli_master_block_too_large(D, L, env):
    with pytest.raises(RuntimeError, match="bad zopfli options"):
        D.zopfli_streams([text()[:12000]], 3, master_block=(8 << 20) + 1, lib=L)


def second_run(D, L, env):
    b = D.Batch(small_subset()[:2], lib=L).run(True)
    with pytest.raises(RuntimeError, match="batch already ran"):
        b.run(True)
    b.close()


CASES = [run_merge, run_no_merge, deflate_level_1, deflate_level_9, zopfli, zopfli_growing_pool, recompress_cheap,
         verify_and_block_info, one_shot_with_a_corrupt_stream,
         levels_chain_lookup, encoder_level_0, zopfli_master_block_too_large, second_run]
