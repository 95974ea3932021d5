"""Inputs for the fused search's tree step (d4g_fused.h: d4f_tree_lit / d4f_tree_dist, d4f_tree_bits / d4f_tree_probe,
d4f_tree_publish, d4f_def_header): a rebuilt tree is looked up in the code table first, a code's default header is
built once in a launch, after the step's last batch, and registered again from the code's record in later rounds.
tests/test_tree_step_hostsim.py runs them in the CPU emulator, tests/test_gpu_tree_step.py on the GPU; every run is
compared byte for byte with the oracle and with the level executor (D4G_EXEC=levels), merge off and on.

The cases, all single final blocks (after a stored block where distances need something to point at):
    refs_N          N back-references among skewed literals (fused_exit_cases.edge_block), N = 64 .. 300
    deep_cl         every literal, frequencies 2^(12 - L) for a chosen length L per symbol, so that the rebuilt code has
                    exactly those lengths: 1, 1, 2, 4, 8, 16, 32, 64 and 129 symbols of nine different lengths.  Its
                    default header's code-length code then has about doubling frequencies and is deeper than 7
                    unlimited (cl_depth() computes that here, in Python).  No distance code: handleZero.
    dist_1          exactly one distance symbol (tree_cases): handleOne
    lit_63_ties     no distance symbol, tie-heavy literal tree (tree_cases)
What a test asserts about the path a case takes it reads from the counters of D4G_FUSED_STATS (d4f_block_rounds lists
them; past the first 64 they come from d4g_debug_fused_stats_all)."""
import ctypes
import random

import deflate_builder as DB
import fused_exit_cases as F
import tree_cases as T
from deflate_builder import Builder

REFS = [64, 100, 200, 300]

# index into the counters
BUILT, REREG, SUBSTEPS, KNOWN, SAME_BATCH, REFUSED_DEF, ROUNDS = 64, 66, 68, 70, 71, 72, 27
NSTATS = 80

# deep_cl: (code length, how many symbols have it) — 257 symbols, Kraft sum exactly 1, the longest length 12 (EOB's)
DEEP_CL_COUNTS = [(8, 129), (9, 64), (11, 32), (12, 16), (10, 8), (5, 4), (6, 2), (3, 1), (4, 1)]

_CACHE = {}


def deep_cl():
    """-> (stream, literal/length histogram, the designed lengths of symbols 0 .. 256)"""
    def make():
        lmax = max(length for length, _ in DEEP_CL_COUNTS)
        assert sum(n << (lmax - length) for length, n in DEEP_CL_COUNTS) == 1 << lmax
        # the most frequent lengths spread out (every other place first), so that no length repeats four times in a row:
        # the header has no repeat codes and its code-length symbols are the lengths themselves
        n = sum(k for _, k in DEEP_CL_COUNTS)
        lens = [0] * n
        places = list(range(0, n, 2)) + list(range(1, n, 2))
        i = 0
        for length, k in sorted(DEEP_CL_COUNTS, key=lambda x: -x[1]):
            for _ in range(k):
                lens[places[i]] = length
                i += 1
        k = lens.index(lmax)     # EOB (weight 1) is the last symbol and has a longest code
        lens[k], lens[-1] = lens[-1], lens[k]
        assert all(len(set(lens[j:j + 4])) > 1 for j in range(n - 3))
        hist = [0] * 286
        for s, length in enumerate(lens):
            hist[s] = 1 << (lmax - length)
        assert n == 257 and hist[256] == 1 and sum(hist) == 1 << lmax
        rng = random.Random(7)
        toks = [s for s in range(256) for _ in range(hist[s])]
        rng.shuffle(toks)
        b = Builder().dynamic(toks, final=True, lit_lens=T.trimmed(T.flat_lengths(hist), 257), dist_lens=[0], rle="none")
        assert b.valid
        return b.getvalue(), hist, lens
    return _cached("deep_cl", make)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def cl_depth(lit_lens, dist_lens):
    """depth of the unlimited code-length tree of the default header of these lengths (every repeat code allowed)"""
    syms = DB.rle_lengths(list(lit_lens) + list(dist_lens))
    freq = [0] * 19
    for s in syms:
        freq[s[0] if isinstance(s, (tuple, list)) else s] += 1
    return max(DB.limited_lengths(freq, 40))


def tree_case(name):
    return [c for c in T.cases() if c.name == name][0].data


def streams():
    """name -> stream"""
    def make():
        out = {"refs_%d" % n: F.edge_block(n) for n in REFS}
        out["deep_cl"] = deep_cl()[0]
        out["dist_1"] = tree_case("dist_1")
        out["lit_63_ties"] = tree_case("lit_63_ties")
        return out
    return _cached("streams", make)


TWO_ROUNDS = ["refs_64", "refs_100", "refs_200", "refs_300", "deep_cl"]    # the second round meets the first one's codes again
REREG_CASE = "refs_100"
SAME_BATCH_CASE = "refs_100"
HDR_CAPS = (1, 5)                   # D4G_FUSED_CAP_HDRS on REREG_CASE: the first id of a round / an id after the first tree step's
CODE_CAP = ("refs_200", 48)         # D4G_FUSED_CAP_CODES: its second round overflows (47 codes pass the first); the next launch starts with an empty table


def run(D, L, data, merge, env=None, monkeypatch=None):
    """one stream -> ((status, saved_bits, output), the d4g_stats counters, the D4G_FUSED_STATS counters)"""
    buf = (ctypes.c_longlong * NSTATS)()
    with monkeypatch.context() as m:
        m.setenv("D4G_FUSED_STATS", "1")
        for k, v in (env or {}).items():
            m.setenv(k, str(v))
        assert L.d4g_debug_fused_stats_all(buf) == 0      # (read and cleared)
        b = D.Batch([data], lib=L).run(merge)
        try:
            r = b.result(0)
            res = (r["status"], r["saved_bits"], b.output(0))
            st = b.stats()
        finally:
            b.close()
        assert L.d4g_debug_fused_stats_all(buf) == 0
    return res, {k: st[k] for k in F.COUNTERS}, list(buf)


def check(O, data, merge, res):
    """status, saved bits and bytes == the oracle's -> list of mismatches"""
    rc, want, osaved = F.oracle(O, data, merge)
    st, saved, out = res
    if (st, saved if st == 0 else 0) != (rc, osaved if rc == 0 else 0):
        return [("result", (st, saved), (rc, osaved))]
    return [("output",)] if out != want else []
