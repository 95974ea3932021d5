"""Inputs of d4g_debug_cl_tree_lengths (the header search's 19-symbol code-length tree, limit 7), shared by the emulator
test (test_cl_tree_registers.py) and the GPU test (test_gpu_tree_builders.py)."""
import ctypes
import random


def lengths(L, hists):
    """-> (the 19 code lengths of every histogram, the `limited` flag of every histogram)"""
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


def exact_limiter():
    """Every histogram a header can produce has at most 316 symbols: Fibonacci chains up to 11 leaves (10 deep).
    -> (histograms, the `limited` flags they must give)"""
    fib = [1, 1]
    while len(fib) < 11:
        fib.append(fib[-1] + fib[-2])
    hs = [fib[:k] + [0] * (19 - k) for k in range(2, 12)] + [[1] * 19, [2] * 18 + [0], [0] * 8 + fib]
    return hs, [0] * 7 + [1] * 3 + [0, 0, 1]
