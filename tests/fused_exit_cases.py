"""Inputs, cap lists and the comparison for the fused executor's exits (k_search_fused / k_search_cluster, d4g_fused.h;
Batch::run_fused / run_cluster, d4g_host_search.h): the table overflow that hands a round to the level executor, the
per-launch round limit that launches a block again, the cluster kernel's refusal, and the mask-word edges at which the
mask tasks change lanes, words and form.  tests/test_fused_exits_hostsim.py runs a part of it in the CPU emulator,
tests/test_gpu_fused_exits.py all of it on the GPU.

The D4G_FUSED_CAP_* knobs lower the number of ids a round may hand out, so small blocks take exits that otherwise need
more than 256 masks, 96 codes, 384 headers or 16 rounds.  What each input needs was measured in the emulator (masks /
codes / headers in the tables at the end of each round of an uncapped run; the code table lasts a launch, the other
two start afresh every round; a cap of N refuses the id N, so a round that ends with N ids passes under cap N):

    png64_l9    m120 c43 h95  | m11 c45 h22 | m11 c48 h26 | m1 c48 h12
    mix25k_l9   m119 c58 h126 | m25 c62 h38 | m3 c63 h18  | m1 c63 h12
    png16_l9    m101 c42 h111 | m11 c45 h26 | m11 c46 h20 | m1 c46 h12
    png64_l6    m117 c49 h111 | m11 c52 h26 | m11 c54 h22 | m3 c55 h18 | m1 c55 h12
    png16_l1    m77 c28 h87   | m36 c28 h34
    mix20k_l9   m108 c59 h139 | m1 c59 h12  | m1 c59 h12
    apng_s11    m56 c27 h63   | m75 c42 h73 | m58 c43 h67

On the GPU (every cap from 1 up, 512-thread workgroups) the codes and headers are the same; the first round's masks are
106, 120, 110, 130, 77, 101 and (second round) 77: a mask id is taken before equal masks are found, and how many tasks
of a step find the same mask depends on how the ops are spread over the threads.  The largest mask caps below stay
under both figures.

The first round needs the most masks on every zlib-made input measured (60 streams), so a uniform mask cap never stops
a launch after its first round there; of the golden fixtures, apng_ball.s07 and apng_ball.s11 do need more masks in
their second round, and apng_s11 is here for that."""
import os
import random
import zlib

import synth
from deflate_builder import Builder, Ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def z(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def mix(n, seed, noise=0.15, alphabet=b"abcdef"):
    """n bytes: `noise` of them random, the rest drawn from a small alphabet"""
    r = random.Random(seed)
    return bytes(r.randrange(256) if r.random() < noise else r.choice(alphabet) for _ in range(n))


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- single-block streams that run several rounds ----
_INPUTS = {
    "png64_l9": lambda: synth.deflate9(synth.pngidat(20000, 3, 64)),
    "mix25k_l9": lambda: z(mix(25000, 5, 0.05), 9),
    "png16_l9": lambda: z(synth.pngidat(30000, 3, 16), 9),
    "png64_l6": lambda: z(synth.pngidat(20000, 3, 64), 6),
    "png16_l1": lambda: z(synth.pngidat(30000, 3, 16), 1),
    "mix20k_l9": lambda: z(mix(20000, 2), 9),
    "apng_s11": lambda: open(os.path.join(GOLDEN, "apng_ball.s11.in.deflate"), "rb").read(),
}
ROUNDS = {"png64_l9": 4, "mix25k_l9": 4, "png16_l9": 4, "png64_l6": 5, "png16_l1": 2, "mix20k_l9": 3, "apng_s11": 3}
FOUR_ROUNDS = ["png64_l9", "mix25k_l9", "png16_l9", "png64_l6"]   # a per-launch limit of 3 rounds still launches them again


def stream(name):
    return _cached(name, _INPUTS[name])


# Caps per table and input, each below what the input needs uncapped (so every run hands at least one round over): from
# "every round that needs an id overflows" to just under the largest need.  Chosen from the table above.
KNOB = {"masks": "D4G_FUSED_CAP_MASKS", "codes": "D4G_FUSED_CAP_CODES", "hdrs": "D4G_FUSED_CAP_HDRS"}
SWEEPS = {
    "masks": {"png64_l9": [1, 10, 12, 64, 100], "mix25k_l9": [1, 4, 26, 64, 110], "png16_l9": [1, 11, 50, 95], "png64_l6": [1, 3, 11, 110],
              "png16_l1": [1, 36, 70], "mix20k_l9": [1, 54, 95], "apng_s11": [1, 24, 58, 64, 75]},
    "codes": {"png64_l9": [2, 6, 30, 44, 47], "mix25k_l9": [2, 8, 40, 60, 62], "png16_l9": [2, 12, 43, 45], "png64_l6": [2, 20, 50, 53, 54],
              "png16_l1": [2, 14, 27], "mix20k_l9": [2, 30, 58], "apng_s11": [2, 26, 30, 42]},
    "hdrs": {"png64_l9": [1, 16, 24, 64, 94], "mix25k_l9": [1, 16, 32, 64, 125], "png16_l9": [1, 19, 25, 110], "png64_l6": [1, 17, 25, 110],
             "png16_l1": [1, 33, 86], "mix20k_l9": [1, 11, 138], "apng_s11": [1, 32, 66, 72]},
}
# the emulator's part (merge off): every table still meets a launch stopped after its first round and one stopped in it
SWEEPS_SIM = {
    "masks": {"png64_l9": [1, 12], "apng_s11": [58, 75]},
    "codes": {"mix25k_l9": [2, 8, 60, 62]},
    "hdrs": {"png64_l9": [1, 16, 24, 94]},
}
ONE_CAP = {"masks": ("apng_s11", 64), "codes": ("png64_l9", 44), "hdrs": ("png64_l9", 24)}   # merge on in the emulator; D4G_MEMO=0


# ---- hand-built blocks with an exact number of back-references ----
def edge_block(nrefs):
    """One dynamic block of `nrefs` back-references among literals of a skewed alphabet: most are short matches at long
    distances, which cost more than their bytes as literals, so the optimiser expands some of them."""
    def make():
        r = random.Random(nrefs)
        alphabet = b"eeeeeeeettttttaaaaooinshrdlu"
        toks = [r.choice(alphabet) for _ in range(300)]
        n = len(toks)
        for k in range(nrefs):
            if r.random() < 0.3:
                m = r.randrange(1, 4)
                toks += [r.choice(alphabet) for _ in range(m)]
                n += m
            length = r.choice((3, 3, 3, 4, 5, 8, 20))
            dist = r.randrange(1, min(n, 32768) + 1) if r.random() < 0.7 else r.randrange(1, 65)
            if k == 0:
                length, dist = 3, n    # (the first one surely costs more than its three bytes: a lone block of one must expand it)
            toks.append(Ref(length, dist))
            n += length
        return Builder().dynamic(toks, final=True).getvalue()
    return _cached(("edge", nrefs), make)


EDGE_REFS = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 16383, 16384]   # one mask word is 64 back-references
EDGE_REFS_CHUNKED = [16385, 16449]      # 257 and 258 words: past the 256 the register form holds (D4G_FUSED_MAX_REFS lets them in)
EDGE_REFS_SIM = [63, 64, 65, 255, 256, 257]   # the same edges with D4G_FUSED_REG_WORDS at 1 and at 4


# ---- a batch of single-block streams of different kinds, and the same blocks as one stream ----
MIXED_SIM = 20   # the emulator's batch: the zlib-made ones


def mixed_batch():
    def make():
        t, p16, p64, p256, m = synth.reptext(2500, 31), synth.pngidat(3000, 3, 16), synth.pngidat(2500, 3, 64), synth.pngidat(2500, 3, 256), mix(2500, 7)
        out = [z(d, lv) for d in (t, p16, p64, m) for lv in (1, 6, 9)]
        out += [z(t, 9, zlib.Z_FIXED), z(p64, 1, zlib.Z_FIXED), z(t, 9, zlib.Z_HUFFMAN_ONLY), z(t[:1500], 9, zlib.Z_RLE), z(p256, 9, zlib.Z_FILTERED),
                z(p256, 9), z(mix(2500, 8, 0.05), 9), z(mix(2000, 9, 0.3, b"abcdefghij"), 1)]
        out += [edge_block(63), edge_block(257), stream("apng_s11"), open(os.path.join(GOLDEN, "apng_ball.s07.in.deflate"), "rb").read()]
        return out
    return _cached("mixed", make)


def as_one_stream(streams, size_bits):
    """The blocks of single-block streams as one stream: each block keeps its bits (its back-references stay inside its own
    bytes), BFINAL cleared on all but the last.  size_bits(stream) -> the stream's length in bits."""
    acc, total = 0, 0
    for k, a in enumerate(streams):
        n = size_bits(a)
        v = int.from_bytes(a, "little") & ((1 << n) - 1)
        assert v & 1, "not a single final block"
        if k + 1 < len(streams):
            v &= ~1
        acc |= v << total
        total += n
    return acc.to_bytes((total + 7) // 8, "little")


def cluster_stream():
    """Two blocks whose merged candidate holds about 5000 back-references: with D4G_CLUSTER_MIN_REFS and D4G_FUSED_MAX_REFS at
    2000 the merge attempt is the cluster kernel's (it only ever runs merge candidates: Batch::run_round)."""
    def make():
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        raw = synth.pngidat(24000, 3, 16)
        return c.compress(raw[:12000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(raw[12000:]) + c.flush()
    return _cached("cluster", make)


CLUSTER_ENV = {"D4G_EXEC": "fused", "D4G_CLUSTER_MIN_REFS": "2000", "D4G_FUSED_MAX_REFS": "2000"}

COUNTERS = ("rounds_fused", "fused_fallbacks", "fused_fallbacks_mid", "fused_relaunches", "rounds_cluster", "cluster_fallbacks")


# ---- the comparison ----
_ORACLE = {}


def oracle(O, a, merge):
    """(status, output, saved_bits) of the reference, once per input"""
    key = (a, merge)
    if key not in _ORACLE:
        rc, want, saved, _, _ = O.optimise(a, merge)
        _ORACLE[key] = (rc, want, saved)
    return _ORACLE[key]


def run(D, L, streams, merge):
    """One batch -> ([(status, saved_bits, output)], the counters)"""
    b = D.Batch(streams, lib=L).run(merge)
    try:
        res = []
        for i in range(len(streams)):
            r = b.result(i)
            res.append((r["status"], r["saved_bits"], b.output(i)))
        st = b.stats()
        return res, {k: st[k] for k in COUNTERS + ("n_blocks", "rounds")}
    finally:
        b.close()


def check(O, streams, merge, res, uncapped=None):
    """Every stream: status, saved bits and output bytes == the oracle's, the output decodes to the input's bytes, and all
    of it == the same batch run with no cap set.  -> list of mismatch descriptions."""
    bad = []
    for i, (a, (st, saved, out)) in enumerate(zip(streams, res)):
        rc, want, osaved = oracle(O, a, merge)
        if (st, saved if st == 0 else 0) != (rc, osaved if rc == 0 else 0):
            bad.append((i, merge, "result", (st, saved), (rc, osaved)))
        elif out != want:
            bad.append((i, merge, "output"))
        elif zlib.decompress(out, -15) != zlib.decompress(a, -15):
            bad.append((i, merge, "decoded"))
    if uncapped is not None and res != uncapped:
        bad.append((merge, "differs from the uncapped run"))
    return bad
