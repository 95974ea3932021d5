"""The tree-builder corpus (tests/tree_cases.py) through the HIP kernels in the CPU emulator (tests/hostsim) against the
oracle: all of it through the default build (the one-lane d4g_build_tree and the limiter), and its small cases
through the `waveheap` build, which runs the wave-wide builders the GPU runs."""
import os
import subprocess

import pytest

import handbuilt_cases as H
import oracle_lib as O
import tree_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The wave-wide build takes the cases of at most 3 000 tokens.  A tree deeper than 15 needs a total weight of 2 584 at
# the very least, and 4 180 as a plain Fibonacci chain, so the corpus has none under that cap: these limiter cases are
# let in by name, one behind each builder and one for the distance tree, the smallest the corpus has.
WAVE_CAP = 3000
WAVE_DEEP = ["lit_20_fib", "lit_64_chain11", "lit_65_chain11", "lit_128_chain10", "dist_18_fib"]


def load(variant, so):
    os.environ["D4G_SIM_BLOCK"] = "64"
    subprocess.check_call([os.path.join(ROOT, "tests", "hostsim", "build.sh")] + variant)
    import deft4j_amd as D
    L = D.load_library(os.path.join(ROOT, "tests", "hostsim", so))
    D.init(0, lib=L)
    return D, L


def named(cases, bad):
    return [(cases[m[0]].name,) + m[1:] if isinstance(m[0], int) else m for m in bad]


def test_corpus_in_the_emulator():
    """The whole corpus as one batch, merge on and off.  Measured: 50 s, 14 s of them the oracle."""
    D, L = load([], "libdeft4g_hostsim.so")
    cs = T.cases()
    assert not named(cs, H.compare(D, L, O, [c.data for c in cs], abi=False))


def wave_subset():
    return [c for c in T.cases() if c.tokens <= WAVE_CAP or c.name in WAVE_DEEP]


def test_wave_subset_still_covers_every_builder():
    cs = [c for c in wave_subset() if T.pins(c).ok]
    assert {c.cls for c in cs} == {"<=64", "65-127", "128+"}
    for cls in ("<=64", "65-127"):
        assert [c for c in cs if c.cls == cls and T.pins(c).deep_lit], cls
    assert [c for c in cs if T.pins(c).deep_dist]
    for used in (64, 65, 127, 128):     # (127 only above the cap: its smallest case has 4 256 tokens)
        assert [c for c in (T.cases() if used == 127 else cs) if sum(1 for f in c.lit_hist if f) == used]


def test_small_cases_through_the_wave_wide_builders():
    """d4g_build_tree_wave64, d4g_build_tree_wave_path and d4g_build_tree_wave in the emulator, every case alone (the
    level executor's d4g_build_tree_wave is reached by the test below and on the GPU).  Measured: 20 s."""
    D, L = load(["waveheap"], "libdeft4g_hostsim_wh.so")
    bad = []
    for c in wave_subset():
        bad += [(c.name,) + m[1:] for m in H.compare(D, L, O, [c.data], merges=(False,), abi=False)]
    assert not bad


LEVELS = ["lit_3_ties", "lit_63_ties", "lit_64_ties", "lit_65_ties", "lit_128_ties_half", "lit_20_fib", "lit_65_chain11"]


def test_level_executor_through_the_lds_builder(monkeypatch):
    """The level executor builds every tree with d4g_build_tree_wave, the small ones included: one case per class and
    two that end in the limiter.  Measured: 5 s."""
    monkeypatch.setenv("D4G_EXEC", "levels")
    D, L = load(["waveheap"], "libdeft4g_hostsim_wh.so")
    cs = [c for c in T.cases() if c.name in LEVELS]
    assert len(cs) == len(LEVELS)
    bad = []
    for c in cs:
        bad += [(c.name,) + m[1:] for m in H.compare(D, L, O, [c.data], merges=(False,), abi=False)]
    assert not bad


def test_zopfli_package_merge_vectors_in_the_emulator():
    """zf_pm_wave on the vectors of the GPU test (2 s).  The weights near 2^31 need a package's weight to saturate: as a
    32-bit sum it wrapped, and the package sorted to the front of its level."""
    import ctypes
    import zopf_lib as ZF
    _, L = load([], "libdeft4g_hostsim.so")
    for f, maxbits in T.zopfli_vectors():
        n = len(f)
        out = (ctypes.c_uint32 * n)()
        assert L.d4g_debug_zopfli_code_lengths((ctypes.c_uint32 * n)(*f), n, maxbits, out) == 0
        assert list(out) == ZF.length_limited(f, maxbits), (f, maxbits)
