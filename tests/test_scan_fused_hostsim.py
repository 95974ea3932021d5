"""The header scan (k_scan_headers: prolog, code-length code, walk over the coded lengths, in one launch) through the CPU
emulator (tests/hostsim): the batches of tests/scan_fused_cases.py against the Python model of the two predicates
(tests/scan_model.py), zlib and the oracle."""
import os
import subprocess

import pytest

import find_streams_cases as F
import oracle_lib as O
import scan_fused_cases as C
import scan_model as M

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


def test_model_on_known_streams():
    """guards the model, not the library: in a stream zlib wrote, every dynamic block's header survives, and a pattern's
    stated densities hold"""
    import synth
    s = synth.deflate9(synth.reptext(300000))
    cands, kept = M.scan(s)
    pos, starts = 0, []
    for typ, _, size, _, _ in O.block_info(s):
        if typ == 2:
            starts.append(pos)
        pos += 3 + size
    assert len(starts) >= 2 and set(starts) <= set(kept) <= set(cands)
    tile = C.SCAN_TILE
    assert len(M.prolog_positions(b"\x55" * (tile + 32))[1]) >= tile * 4 > C.LIST_A
    assert len([p for p in M.candidates(b"\x5e\xdb" * (tile // 2 + 16)) if p < tile * 8]) == tile * 8 * 3 // 16 > C.LIST_B
    assert not any(M.candidates(bytes([v]) * 64) for v in range(256))


@pytest.mark.parametrize("name", [c.name for c in C.all_cases()])
def test_case(sim, name):
    """(the emulator is slow at the search: the batches with real data or thousands of blocks are parsed, the others also
    optimised)"""
    D, L = sim
    c = next(c for c in C.all_cases() if c.name == name)
    assert not C.check_case(D, L, c, run=not name.startswith(("real_", "more_blocks")))


def test_find_path(sim):
    """d4g_find_streams goes through the same scan: a file's reported streams are the builder's"""
    D, L = sim
    c = F.by_name("back_to_back")[0]
    assert D.find_streams([c.data], c.kinds, c.min_decoded, lib=L) == [F.wanted(c, 0)]
