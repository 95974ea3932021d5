"""tests/test_gpu_sort_one_key.py in the test-only CPU emulator: sort blocks whose positions all share one hash (a full
block of 32768 in one bucket, the buckets behind it starting at 32768, every placement step one group of duplicates),
byte-identical to live zlib under deflate_slow (level 9) and deflate_fast (level 1)."""
import os
import subprocess

import pytest

import lz_levels_lib as LL

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


@pytest.mark.parametrize("level", [9, pytest.param(1, marks=pytest.mark.skipif(not LL.LIVE_ZLIB, reason="deflate_fast is pinned to zlib 1.2.11"))])
def test_sort_block_of_one_key(sim, level):
    D, L = sim
    ins = [bytes(32770), bytes(65600)]
    outs = D.deflate_streams(ins, D.ENC_JVM, D.STRATEGY_DEFAULT, lib=L, level=level)
    for d, o in zip(ins, outs):
        assert o == LL.zref(d, level, 0), (len(d), level)
