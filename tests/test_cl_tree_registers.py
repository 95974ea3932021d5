"""The header search's register-resident 19-symbol code-length tree (d4g_cl_tree_regs, with the depth limiter taken
through d4g_build_tree) against the oracle's HuffmanTree(freq, 7), in the CPU emulation of the kernels."""
import os
import subprocess

import pytest

import oracle_lib as O
from cl_tree_cases import exact_limiter, histograms, lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(ROOT, "tests", "hostsim", "libdeft4g_hostsim.so")
    subprocess.check_call([os.path.join(ROOT, "tests", "hostsim", "build.sh")])
    import deft4j_amd as D
    L = D.load_library(so)
    D.init(0, lib=L)
    return L


def test_register_tree_matches_the_oracle(sim):
    hs = histograms(11)
    got, lim = lengths(sim, hs)
    fell = 0
    for h, g, l in zip(hs, got, lim):
        want, _ = O.huffman_lengths(h, 7)
        assert g == want, (h, g, want)
        fell += l
    assert fell > 100   # the Fibonacci-like histograms took the limiter


def test_limiter_is_taken_exactly_for_deep_trees(sim):
    """Every histogram a header can produce has at most 316 symbols: Fibonacci chains up to 11 leaves (10 deep)."""
    hs, flags = exact_limiter()
    got, lim = lengths(sim, hs)
    for h, g, l in zip(hs, got, lim):
        want, _ = O.huffman_lengths(h, 7)
        deep = max(O.huffman_lengths(h, 15)[0]) > 7
        assert g == want
        assert l == deep
    assert lim == flags == [0] * 7 + [1] * 3 + [0, 0, 1]
