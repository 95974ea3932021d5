"""The header search's register-resident 19-symbol code-length tree (d4g_cl_tree_regs, with the depth limiter taken
through d4g_build_tree) against the oracle's HuffmanTree(freq, 7), in the CPU emulation of the kernels."""
import ctypes
import os
import random
import subprocess

import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    so = os.path.join(ROOT, "tests", "hostsim", "libdeft4g_hostsim.so")
    subprocess.check_call([os.path.join(ROOT, "tests", "hostsim", "build.sh")])
    import deft4j_amd as D
    L = D.load_library(so)
    D.init(0, lib=L)
    return L


def lengths(L, hists):
    n = len(hists)
    f = (ctypes.c_uint32 * (19 * n))(*[x for h in hists for x in h])
    out = (ctypes.c_uint32 * (19 * n))()
    lim = (ctypes.c_int32 * n)()
    assert L.d4g_debug_cl_tree_lengths(f, n, out, lim) == 0
    return [list(out[19 * i:19 * i + 19]) for i in range(n)], list(lim)


def histograms(seed):
    rng = random.Random(seed)
    hs = [[0] * 19]
    for s in range(19):                        # one used symbol: a dummy leaf beside it
        h = [0] * 19; h[s] = rng.choice((1, 5, 300)); hs.append(h)
    for a in range(19):                        # two used symbols
        for b in range(a + 1, 19, 3):
            h = [0] * 19; h[a] = rng.randrange(1, 40); h[b] = rng.randrange(1, 40); hs.append(h)
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    while len(hs) < 12000:
        kind = rng.randrange(5)
        h = [0] * 19
        used = rng.sample(range(19), rng.randrange(1, 20))
        if kind == 0:                          # equal weights: the queue's tie order decides the shape
            w = rng.randrange(1, 8)
            for s in used: h[s] = w
        elif kind == 1:                        # few distinct small weights
            for s in used: h[s] = rng.choice((1, 2, 3))
        elif kind == 2:                        # Fibonacci-like: deeper than 7, the limiter (sum below 316)
            k = rng.randrange(9, 12)
            for i, s in enumerate(rng.sample(range(19), k)): h[s] = fib[i] + rng.randrange(2)
        else:                                  # what a header's packing gives: counts summing to at most 316
            total = rng.randrange(2, 317)
            for _ in range(total): h[rng.choice(used)] += 1
        hs.append(h)
    return hs


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
    fib = [1, 1]
    while len(fib) < 11:
        fib.append(fib[-1] + fib[-2])
    hs = [fib[:k] + [0] * (19 - k) for k in range(2, 12)] + [[1] * 19, [2] * 18 + [0], [0] * 8 + fib]
    got, lim = lengths(sim, hs)
    for h, g, l in zip(hs, got, lim):
        want, _ = O.huffman_lengths(h, 7)
        deep = max(O.huffman_lengths(h, 15)[0]) > 7
        assert g == want
        assert l == deep
    assert lim == [0] * 7 + [1] * 3 + [0, 0, 1]
