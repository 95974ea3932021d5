"""Device-memory ownership (d4g_rt.h: RtBuf, RtScratch) in the CPU emulator: the number of pool blocks handed out and not
yet returned (d4g_debug_device_blocks) is the same before and after every call, once the batches it made are closed —
whether the call succeeds or the host refuses or fails it half way."""
import os
import subprocess

import pytest

import device_memory_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    os.environ["D4G_SIM_BLOCK"] = "64"
    so = os.path.join(ROOT, "tests", "hostsim", "libdeft4g_hostsim.so")
    subprocess.check_call([os.path.join(ROOT, "tests", "hostsim", "build.sh")])
    import deft4j_amd as D
    L = D.load_library(so)
    D.init(0, lib=L)
    M.warm_up(D, L)
    return D, L


@pytest.mark.parametrize("case", M.CASES, ids=[c.__name__ for c in M.CASES])
def test_blocks_come_back(sim, monkeypatch, case):
    D, L = sim
    before = M.live_blocks(L)
    case(D, L, monkeypatch.setenv)
    assert M.live_blocks(L) == before
