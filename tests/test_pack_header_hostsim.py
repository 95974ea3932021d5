"""The shared header packer (d4g_wave_pack_header, through d4g_debug_pack_header) against the oracle's
HuffmanTable.pack, HuffmanTree(counts, 7) and the header size they give, in the CPU emulation of the kernels."""
import os
import subprocess

import pytest

import pack_header_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(ROOT, "tests", "hostsim", "libdeft4g_hostsim.so")
    subprocess.check_call([os.path.join(ROOT, "tests", "hostsim", "build.sh")])
    import deft4j_amd as D
    L = D.load_library(so)
    D.init(0, lib=L)
    return L


def test_vectors_are_what_they_claim():
    """(oracle only) the shapes the run finder is tested on, and no packing longer than the pair buffer"""
    vs = {name: (nlit, ndist, v) for name, nlit, ndist, v in P.vectors()}
    assert 40 <= len(vs) <= 60
    assert {nlit + ndist for nlit, ndist, _ in vs.values()} == {258, 320}
    assert all(len(v) == nlit + ndist and all(0 <= x <= 15 for x in v) for nlit, ndist, v in vs.values())

    def runs(v):
        out, s = [], 0
        for i in range(1, len(v) + 1):
            if i == len(v) or v[i] != v[s]:
                out.append((s, i - s, v[s]))
                s = i
        return out
    assert runs(vs["all_equal_320"][2]) == [(0, 320, 7)] and len(runs(vs["alternating_320"][2])) == 320
    assert (0, 9, 3) in runs(vs["start_0_320"][2]) and (50, 14, 4) in runs(vs["end_63_320"][2]) and (64, 20, 4) in runs(vs["start_64_320"][2])
    for b in (64, 128, 192, 256):
        assert (b - 5, 12, 9) in runs(vs["straddle_%d_320" % b][2]) and (b - 1, 2, 0) in runs(vs["straddle_%d_zeros_258" % b][2])
    assert (64, 192, 2) in runs(vs["three_chunks_258"][2])
    assert (3, 138, 0) in runs(vs["zeros_138_320"][2]) and (60, 139, 0) in runs(vs["zeros_139_258"][2]) and (7, 277, 0) in runs(vs["zeros_277_320"][2])
    assert (287, 2, 8) in runs(vs["lit_into_dist_320"][2]) and (251, 7, 8) in runs(vs["lit_into_dist_258"][2])
    assert (307, 13, 3) in runs(vs["ends_at_n_320"][2]) and (251, 7, 9) in runs(vs["straddle_256_258"][2])
    assert {l for _, l, x in runs(vs["runs_of_7_8_9_320"][2]) if l > 1} == {7, 8, 9, 10}
    flags = set(P.flag_sets())
    assert P.F_DEFAULT in flags and len(P.program_flag_sets()) == 56
    for nlit, ndist, v in vs.values():
        for f in flags:
            assert 0 < P.expected(v, f)[4] <= P.MAXPAIRS


def test_packer_matches_the_oracle(sim):
    assert not P.mismatches(sim)
