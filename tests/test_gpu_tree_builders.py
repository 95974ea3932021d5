"""Every Huffman tree builder of the GPU library against the oracle on inputs built for it.

The tree-builder corpus (tests/tree_cases.py: blocks with a chosen histogram, so that the rebuild makes the tree of
exactly that histogram) under the fused executor (d4g_build_tree_wave64 up to 64 used symbols,
d4g_build_tree_wave_path for 65-127, d4g_build_tree_wave from 128 on), with the cluster kernel forced, and under the
level executor (d4g_build_tree_wave for every histogram); and the two debug entry points: the header search's
register tree (d4g_cl_tree_regs / d4g_cl_lengths) and the Zopfli package-merge (zf_pm_wave)."""
import ctypes

import pytest

import cl_tree_cases as CL
import handbuilt_cases as H
import oracle_lib as O
import tree_cases as T
import zopf_lib as ZF
from test_gpu_handbuilt import CONFIGS

pytestmark = pytest.mark.gpu


class MemoOracle:
    """oracle_lib with the results of optimise / inflate kept per module: the three configurations and the case-alone
    run compare the same streams."""
    def __init__(self):
        self.memo = {}

    def _get(self, key, fn):
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]

    def optimise(self, data, merge_blocks=True):
        return self._get(("o", data, bool(merge_blocks)), lambda: O.optimise(data, merge_blocks))

    def inflate(self, data):
        return self._get(("i", data), lambda: O.inflate(data))

    def size_bits(self, data):
        return self._get(("s", data), lambda: O.size_bits(data))


@pytest.fixture(scope="module")
def lib():
    import deft4j_amd as D
    return D, D.init(0)


@pytest.fixture(scope="module")
def oracle():
    return MemoOracle()


def names(cs, bad):
    return [(cs[m[0]].name,) + m[1:] if isinstance(m[0], int) else m for m in bad]


@pytest.mark.parametrize("merge", [False, True], ids=["merge_off", "merge_on"])
@pytest.mark.parametrize("cfg", list(CONFIGS), ids=list(CONFIGS))
def test_corpus_as_one_batch(lib, oracle, monkeypatch, cfg, merge):
    """(the cluster configuration sends dist_18_fib's 6 764 references, and every block above 2 000, to the cluster kernel;
    no case needs keeping out of the level executor: see handbuilt_cases.LEVEL_EXEC_BAD.  The first case of each merge
    flag pays for the oracle's 108 results, 7 s; the GPU's part is 0.1 s)"""
    for k, v in CONFIGS[cfg].items():
        monkeypatch.setenv(k, v)
    D, L = lib
    cs = T.cases()
    assert not names(cs, H.compare(D, L, oracle, [c.data for c in cs], merges=(merge,), abi=False))


def test_every_pinning_case_alone(lib, oracle):
    """merge off, as in the pinning rule"""
    D, L = lib
    cs = [c for c in T.cases() if T.pins(c).ok]
    assert 4 * len(cs) >= 3 * len(T.cases())
    bad = []
    for c in cs:
        bad += [(c.name,) + m[1:] for m in H.compare(D, L, oracle, [c.data], merges=(False,), abi=False)]
    assert not bad


def test_register_cl_tree_matches_the_oracle(lib):
    """d4g_debug_cl_tree_lengths on the GPU: the 12 000 histograms of the emulator test, lengths and `limited` flags
    (the flag is set exactly when the unlimited tree is deeper than 7)."""
    _, L = lib
    hs = CL.histograms(11)
    got, lim = CL.lengths(L, hs)
    for h, g, l in zip(hs, got, lim):
        assert g == O.huffman_lengths(h, 7)[0], (h, g)
        assert l == (max(O.huffman_lengths(h, 15)[0]) > 7), h
    assert sum(lim) > 100
    hs, flags = CL.exact_limiter()
    got, lim = CL.lengths(L, hs)
    assert got == [O.huffman_lengths(h, 7)[0] for h in hs]
    assert lim == flags


def test_zopfli_package_merge_matches_the_oracle(lib):
    """d4g_debug_zopfli_code_lengths on the GPU, one one-wave launch per vector."""
    _, L = lib
    vs = T.zopfli_vectors()
    assert len(vs) >= 2000
    for f, maxbits in vs:
        n = len(f)
        out = (ctypes.c_uint32 * n)()
        assert L.d4g_debug_zopfli_code_lengths((ctypes.c_uint32 * n)(*f), n, maxbits, out) == 0
        assert list(out) == ZF.length_limited(f, maxbits), (f, maxbits)
