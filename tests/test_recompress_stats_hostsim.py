"""The counters of a recompression run (tests/recompress_stats_cases.py) through the HIP kernels in the CPU emulator
(tests/hostsim): modes NONE, CHEAP, ZOPFLI and ZOPFLI_EXTENSIVE, with and without mergeBlocks."""
import os
import subprocess

import pytest

import recompress_stats_cases as R

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


def test_recompress_counters(sim):
    R.check(*sim)
