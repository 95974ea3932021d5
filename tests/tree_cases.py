"""Deterministic corpus of hand-built raw DEFLATE streams whose blocks have a chosen token histogram, so that
recodeHuffman (oracle recode_huffman; on the GPU d4f_wave_tree / wg_recode_huffman) builds the Huffman tree of exactly
that histogram: the way the suite chooses which tree builder a test reaches (d4g_build_tree_wave64 up to 64 used
symbols, d4g_build_tree_wave_path for 65-127, d4g_build_tree_wave from 128 on), with which tie order, and whether the
depth limiter (d4g_tree_finish) runs.

Two families.  Literal: one final dynamic block of literals over a seeded subset of the 256 bytes plus EOB (whose
weight is always 1: one block, one EOB).  Back-reference: a stored block of 32 768 seeded random bytes, so that every
distance is reachable, then a dynamic block with every literal 1..19 times, a chosen set of length symbols and a chosen
distance histogram.  Both are written with a deliberately poor but complete code (lengths k-1 / k over the used
symbols, the shorter codes on the lightest symbols) and a header without repeat codes, so the rebuilt tree wins.

A case *pins* its builder when the oracle's output (merge off) carries exactly the code lengths of the designed
histograms' trees: `pins()` reads them back from the output's block header.  A case's `cell` names what it is meant to
cover; CELLS lists every cell the corpus must cover with a pinning case, LIMITER_CELLS those that must do so with a
tree deeper than 15."""
import random

import deflate_builder as DB
from deflate_builder import Builder, Ref

MAX_TOKENS = 70000
LIT_COUNTS = (2, 3, 4, 63, 64, 65, 66, 126, 127, 128, 129, 257)
LIT_SHAPES = ("ties", "rand", "asc", "desc", "heavy")
DIST_COUNTS = (2, 3, 17, 18, 29, 30)
DIST_SHAPES = ("ties", "rand", "asc", "desc")

FIB = [1, 1]
while len(FIB) < 40:
    FIB.append(FIB[-1] + FIB[-2])


def dispatch_class(hist):
    """The builder d4g_build_tree_wave64 hands a histogram to, computed the way it counts: the non-zero entries below
    the last non-zero one, and the total weight (2^24 - 4 and more goes to the LDS builder whatever the count)."""
    last = max((i + 1 for i, f in enumerate(hist) if f), default=0)
    used = sum(1 for f in hist[:last] if f)
    if used > 127 or sum(hist[:last]) >= (1 << 24) - 4:
        return "128+"
    return "65-127" if used > 64 else "<=64"


def intended_class(used):
    return "<=64" if used <= 64 else "65-127" if used <= 127 else "128+"


class TreeCase:
    def __init__(self, name, cell, b, lit_hist, dist_hist, used, tokens):
        assert b.valid and tokens <= MAX_TOKENS, (name, tokens)
        self.name, self.cell, self.data, self.plain = name, cell, b.getvalue(), bytes(b.plain)
        self.lit_hist, self.dist_hist, self.tokens = lit_hist, dist_hist, tokens
        self.cls = intended_class(used)          # from the count the case was asked for, not from the histogram
        self.dist_used = sum(1 for f in dist_hist if f)

    def __repr__(self):
        return "TreeCase(%s)" % self.name


def flat_lengths(hist):
    """A complete code of lengths k-1 / k over the used symbols; the lightest symbols get the shorter codes."""
    used = sorted((f, s) for s, f in enumerate(hist) if f)
    out = [0] * len(hist)
    n = len(used)
    if n == 1:
        out[used[0][1]] = 1
        return out
    k = (n - 1).bit_length()
    short = (1 << k) - n
    for i, (_, s) in enumerate(used):
        out[s] = k - 1 if i < short else k
    if short == 0 and n >= 4:    # a power of two: flat is the only such code, and optimal for near-equal weights; skew it
        out[used[0][1]], out[used[-1][1]], out[used[-2][1]] = k - 1, k + 1, k + 1
    assert DB.kraft(out) == 32768
    return out


def trimmed(lens, least):
    lens = list(lens)
    while len(lens) > least and lens[-1] == 0:
        lens.pop()
    return lens


def weights(shape, m, rng, small):
    """m weights in symbol order.  `small`: a block of 2-4 used symbols, which needs a few hundred tokens to stay
    dynamic."""
    k = 100 if small else 1
    if shape == "ties":        # few distinct weights: the queue's tie order decides the shape
        return [rng.choice((16, 32, 48)) * (8 if small else 1) for _ in range(m)]
    if shape == "ties_half":   # the same with half the tokens (for the slow wave-wide emulator build)
        return [rng.choice((8, 16, 24)) for _ in range(m)]
    if shape == "rand":
        return [rng.randrange(100, 600) if small else rng.randrange(1, 300) for _ in range(m)]
    if shape == "asc":         # rising with the symbol number: no offer sifts up
        return [k * (i + 2) for i in range(m)]
    if shape == "desc":        # falling: every offer sifts up to the root
        return [k * (m + 1 - i) for i in range(m)]
    if shape == "heavy":       # one heavy symbol among ones
        w = [1] * m
        w[rng.randrange(m)] = 5000
        return w
    if shape == "equal":
        return [9] * m
    if shape == "fib":         # a plain Fibonacci chain behind EOB's 1: depth m
        return FIB[1:m + 1][::-1]
    if shape.startswith("chain"):    # a Fibonacci chain of the given length (behind EOB's 1) under a flat top:
        p = int(shape[5:])           # the chain's depth plus log2 of the rest, with far fewer tokens than a full chain
        return ([FIB[p + 1]] * m + FIB[1:p + 1][::-1])[-m:]
    if shape.startswith("ladder"):   # repeated Fibonacci ladders of the given period
        p = int(shape[6:])
        return [FIB[i % p] for i in range(m)]
    raise ValueError(shape)


def lit_case(used, shape, seed, cell=None):
    """One final dynamic block of literals: `used` symbols, EOB among them."""
    rng = random.Random(seed * 1000 + used)
    m = used - 1
    syms = sorted(rng.sample(range(256), m))
    w = weights(shape, m, rng, used <= 4)
    hist = [0] * 286
    for s, f in zip(syms, w):
        hist[s] = f
    hist[256] = 1
    toks = [s for s, f in zip(syms, w) for _ in range(f)]
    rng.shuffle(toks)
    b = Builder().dynamic(toks, final=True, lit_lens=trimmed(flat_lengths(hist), 257), dist_lens=[0], rle="none")
    return TreeCase("lit_%d_%s" % (used, shape), cell or "lit/%d/%s" % (used, shape), b, hist, [0] * 30, used, len(toks))


def dist_weights(shape, k, rng):
    if shape == "fib":
        return FIB[:k]
    if shape.startswith("chain"):
        p = int(shape[5:])
        return (FIB[:p] + [FIB[p]] * k)[:k]
    if shape == "equal":
        return [40] * k
    if shape == "asc":
        return [10 * (i + 1) for i in range(k)]
    if shape == "desc":
        return [10 * (k - i) for i in range(k)]
    if shape == "rand":        # (at least as many references as there are length symbols to use)
        return [rng.randrange(15, 300) for _ in range(k)]
    return weights(shape, k, rng, False)


def ref_case(name, cell, ndist, shape, seed, first_len=265, n284=0, dsyms=None, sort_pairs=False):
    """A stored block of 32 768 random bytes, then a final dynamic block: every literal 1..19 times, the length symbols
    first_len..285 (n284 of the references are length 258 written as 284 + 31), `ndist` distance symbols weighted by
    `shape`."""
    rng = random.Random(seed)
    b = Builder().stored(bytes(rng.randrange(256) for _ in range(32768)))
    lit_hist = [0] * 286
    for s in range(256):
        lit_hist[s] = rng.randrange(1, 20)
    lit_hist[256] = 1
    dist_hist = [0] * 30
    if dsyms is None:
        dsyms = sorted(rng.sample(range(30), ndist))
    for s, f in zip(dsyms, dist_weights(shape, ndist, rng)):
        dist_hist[s] = f
    nref = sum(dist_hist)
    lsyms = list(range(first_len, 286))
    assert nref >= len(lsyms) + n284
    ls = lsyms + [rng.choice(lsyms) for _ in range(nref - len(lsyms) - n284)]
    lengths = [(258, True)] * n284
    for s in ls:
        i = s - 257
        span = (1 << DB.LEN_EBITS[i]) - (1 if s == 284 else 0)     # 284 + 31 is length 258: only where asked for
        lengths.append((DB.LEN_BASE[i] + rng.randrange(span), False))
    dists = [DB.DIST_BASE[s] + rng.randrange(1 << DB.DIST_EBITS[s]) for s in range(30) for _ in range(dist_hist[s])]
    if sort_pairs:      # short lengths with near distances, so that no reference is cheaper as literals
        lengths.sort()
        dists.sort()
    else:
        rng.shuffle(lengths)
        rng.shuffle(dists)
    toks = [s for s in range(256) for _ in range(lit_hist[s])] + [Ref(ln, d, e) for (ln, e), d in zip(lengths, dists)]
    rng.shuffle(toks)
    for t in toks:
        if isinstance(t, Ref):
            lit_hist[DB.len_symbol(t.length, t.use284)[0]] += 1
    b.dynamic(toks, final=True, lit_lens=trimmed(flat_lengths(lit_hist), 257), dist_lens=trimmed(flat_lengths(dist_hist), 1),
              rle="none")
    return TreeCase(name, cell, b, lit_hist, dist_hist, sum(1 for f in lit_hist if f), len(toks))


def build():
    cs = []
    for used in LIT_COUNTS:
        for shape in LIT_SHAPES:
            cs.append(lit_case(used, shape, 1))
    # equal weights pin where the count is a power of two
    cs.append(lit_case(64, "equal", 2, "lit/64/equal"))
    cs.append(lit_case(128, "equal", 2, "lit/128/equal"))
    # trees deeper than 15: the limiter behind each builder
    cs.append(lit_case(20, "fib", 3, "lit/limiter/<=64"))
    for used, shape in ((63, "chain11"), (64, "chain11"), (64, "chain14"), (65, "chain11"), (66, "chain11"), (127, "chain10"),
                        (128, "chain10"), (257, "chain9")):
        cs.append(lit_case(used, shape, 3, "lit/limiter/" + intended_class(used)))
    cs.append(lit_case(127, "ladder19", 3, "lit/limiter/65-127"))
    for used in (128, 129):
        cs.append(lit_case(used, "ladder19", 3, "lit/limiter/128+"))
    cs.append(lit_case(257, "ladder17", 3, "lit/limiter/128+"))
    # a small block of the largest class for the slow wave-wide emulator build
    cs.append(lit_case(128, "ties_half", 4, "lit/128/ties"))
    # literal/length trees with length symbols
    cs.append(ref_case("ref_286_used", "litlen/286", 30, "rand", 11, first_len=257, sort_pairs=True))
    cs.append(ref_case("ref_267_used", "litlen/258-286", 3, "rand", 12, first_len=276))
    cs.append(ref_case("ref_278_used", "litlen/258-286", 30, "equal", 13))
    cs.append(ref_case("ref_258_as_285", "litlen/258_as_285", 5, "rand", 14, first_len=281))
    cs.append(ref_case("ref_258_as_284", "litlen/258_as_284", 5, "rand", 15, first_len=281, n284=40))
    # distance trees
    for k in DIST_COUNTS:
        for shape in DIST_SHAPES:
            cs.append(ref_case("dist_%d_%s" % (k, shape), "dist/%d/%s" % (k, shape), k, shape, 100 + k))
    cs.append(ref_case("dist_18_fib", "dist/limiter", 18, "fib", 21))
    cs.append(ref_case("dist_30_chain13", "dist/limiter", 30, "chain13", 22))
    cs.append(ref_case("dist_1", "dist/1", 1, "equal", 23))
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return cs


# "dist/0" (handleZero): every literal-family case has no distance symbol; lit/257/rand stands for the cell
CELLS = (["lit/%d/%s" % (u, s) for u in LIT_COUNTS for s in LIT_SHAPES] + ["lit/64/equal", "lit/128/equal"] +
         ["lit/limiter/<=64", "lit/limiter/65-127", "lit/limiter/128+"] +
         ["litlen/286", "litlen/258-286", "litlen/258_as_285", "litlen/258_as_284"] +
         ["dist/%d/%s" % (k, s) for k in DIST_COUNTS for s in DIST_SHAPES] + ["dist/limiter", "dist/0", "dist/1"])
LIMITER_CELLS = ["lit/limiter/<=64", "lit/limiter/65-127", "lit/limiter/128+", "dist/limiter"]

_CACHE = {}


def cases():
    if "cases" not in _CACHE:
        _CACHE["cases"] = build()
    return _CACHE["cases"]


def cells_of(c):
    return [c.cell] + (["dist/0"] if c.dist_used == 0 else [])


# ---- reading the code lengths back ----
class Bits:
    def __init__(self, data):
        self.v, self.pos = int.from_bytes(data, "little"), 0

    def take(self, n):
        r = (self.v >> self.pos) & ((1 << n) - 1)
        self.pos += n
        return r


def first_huffman_header(data):
    """Skips stored blocks.  -> ("dynamic", literal/length lengths (286), distance lengths (30)), ("fixed", ...) for a
    fixed block, or ("stored", None, None) when the stream ends with no Huffman block."""
    r = Bits(data)
    while True:
        final, btype = r.take(1), r.take(2)
        if btype == 0:
            r.pos = (r.pos + 7) // 8 * 8
            n = r.take(16)
            r.pos += 16 + 8 * n
            if final:
                return "stored", None, None
            continue
        if btype == 1:
            return "fixed", DB.FIXED_LIT[:286], DB.FIXED_DIST[:30]
        assert btype == 2
        hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
        cl = [0] * 19
        for i in range(hclen):
            cl[DB.CL_ORDER[i]] = r.take(3)
        sym_of = {(l, c): s for s, (l, c) in enumerate(zip(cl, DB.canonical(cl))) if l}
        lens = []
        while len(lens) < hlit + hdist:
            code, n = 0, 0
            while (n, code) not in sym_of:
                code, n = (code << 1) | r.take(1), n + 1
                assert n <= 7
            s = sym_of[(n, code)]
            if s < 16:
                lens.append(s)
            elif s == 16:
                lens += [lens[-1]] * (3 + r.take(2))
            else:
                lens += [0] * (3 + r.take(3) if s == 17 else 11 + r.take(7))
        assert len(lens) == hlit + hdist
        return "dynamic", lens[:hlit] + [0] * (286 - hlit), lens[hlit:] + [0] * (30 - hdist)


def tree_of(hist, limit=15):
    """the oracle's HuffmanTree(hist up to its last used symbol, limit) lengths, padded back to len(hist)"""
    import oracle_lib as O
    last = max((i + 1 for i, f in enumerate(hist) if f), default=0)
    return O.huffman_lengths(hist[:last], limit)[0] + [0] * (len(hist) - last)


class Pin:
    """outcome: what the oracle's output holds ("dynamic", "fixed", "stored", or "unchanged" when it kept the input);
    lit / dist: the output's lengths are the designed histograms' trees (dist: None for fewer than two used distance
    symbols, where no tree is built — handleZero / handleOne); deep_lit / deep_dist: the unlimited tree is deeper
    than 15, so the limiter ran."""
    def __init__(self, outcome, lit, dist, deep_lit, deep_dist):
        self.outcome, self.lit, self.dist, self.deep_lit, self.deep_dist = outcome, lit, dist, deep_lit, deep_dist
        self.ok = outcome == "dynamic" and lit and dist is not False

    def why_not(self):
        if self.ok:
            return None
        if self.outcome != "dynamic":
            return "went " + self.outcome
        return "the search chose other lengths"


def pins(case):
    if case.name not in _CACHE:
        import oracle_lib as O
        rc, out, _, _, _ = O.optimise(case.data, False)
        deep_lit = max(DB.limited_lengths(case.lit_hist, 40)) > 15
        deep_dist = case.dist_used >= 2 and max(DB.limited_lengths(case.dist_hist, 40)) > 15
        if rc != 0:
            p = Pin("unchanged", False, None, deep_lit, deep_dist)
        else:
            kind, ll, dl = first_huffman_header(out)
            lit = kind == "dynamic" and ll == tree_of(case.lit_hist)
            if case.dist_used >= 2:
                dist = kind == "dynamic" and dl == tree_of(case.dist_hist)
            else:
                dist = None
                if kind == "dynamic" and dl != [1 if f else 0 for f in case.dist_hist]:
                    lit = False     # (a lost or added distance symbol: not the designed block)
            p = Pin(kind, lit, dist, deep_lit, deep_dist)
        _CACHE[case.name] = p
    return _CACHE[case.name]


# ---- vectors of d4g_debug_zopfli_code_lengths (zf_pm_wave, the wave-wide package-merge) ----
def zopfli_vectors(seeds=28):
    """(frequencies, maxbits): the three alphabets the Zopfli block-size evaluation builds codes for, with used-symbol
    counts around the wave width and its double, and four shapes: ties (a package sorts before a leaf of equal weight),
    Fibonacci (needs the limit), one weight near 2^31 - 1 among ones (the sum of all stays below 2^32), random."""
    out = []
    for n, maxbits in ((288, 15), (32, 15), (19, 7)):
        for used in sorted({u for u in (1, 2, 3, 63, 64, 65, 127, 128, 129, n) if u <= n}):
            for seed in range(seeds):
                rng = random.Random((n * 1000 + used) * 100 + seed)
                for shape in ("ties", "fib", "huge", "rand"):
                    syms = rng.sample(range(n), used)
                    if shape == "ties":
                        vals = rng.choice(((1, 2, 4, 8), (1, 2, 3), (5,), (3, 6, 12, 24, 48)))
                        w = [rng.choice(vals) for _ in range(used)]
                    elif shape == "fib":
                        p = rng.randrange(max(2, min(maxbits, used)), 41)
                        w = [FIB[i % p] for i in range(used)]
                    elif shape == "huge":
                        w = [1] * used
                        w[rng.randrange(used)] = (1 << 31) - 1 - rng.randrange(3)
                    else:
                        w = [rng.choice((1, 1, 2, 3, rng.randrange(1, 50), rng.randrange(1, 100000))) for _ in range(used)]
                    assert sum(w) < 1 << 32
                    f = [0] * n
                    for s, x in zip(syms, w):
                        f[s] = x
                    out.append((f, maxbits))
    return out
