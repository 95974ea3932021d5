"""Streams that pin the static bin statistics of a block (k_block_bins, read through d4g_debug_batch_bins), and the checks the
emulator and the GPU run on them.

Every stream is written with tests/deflate_builder.py from an explicit token list, so each back-reference's length symbol,
distance symbol, extra bits and position are known here; the decoded bytes are the builder's own, checked against
zlib.decompress(stream, -15).  Nothing expected comes from the library: the table (byte counts per length symbol, distance
symbols, record count, extra bits), the record masks and every record's x / y / z / w are computed below.

The kernel stages a block TILE decoded bytes at a time, and one workgroup takes up to SPAN_TILES tiles of a block; the cases
sit on those boundaries."""
import collections
import random
import struct
import zlib

from deflate_builder import LEN_BASE, Builder, Ref, dist_symbol, len_symbol

TILE = 16384          # D4G_BINS_TILE (deft4j_amd/csrc/d4g_ops.h)
SPAN_TILES = 4        # D4G_BINS_SPAN_TILES (d4g_host.h): tiles one workgroup sums before it adds to the block's table
NBINS, STRIDE = 29, 320
BIN_DIST, BIN_COUNT, BIN_EBITS = 256, 286, 287


def mix(rng, n, have):
    """tokens that decode to exactly n bytes: literals of a small alphabet and back-references of all sizes; `have` bytes
    are already there to copy from"""
    out, made = [], 0
    while made < n:
        left = n - made
        if have + made >= 1 and left >= 3 and rng.random() < 0.45:
            ln = min(left, rng.choice((3, 3, 4, 5, 6, 8, 11, 19, 35, 70, 130, 258)))
            out.append(Ref(ln, rng.randint(1, min(have + made, 400))))
            made += ln
        else:
            out.append(rng.choice(b"abcdefgh"))
            made += 1
    return out


class Case:
    """streams: per stream a list of blocks, ("dyn" | "fixed", tokens) or ("stored", bytes)"""

    def __init__(self, name, streams, dictionary=None, env=None, large=False, optimise=True):
        self.name, self.env, self.large, self.optimise, self.dictionary = name, env or {}, large, optimise, dictionary
        self.data, self.plain, self.records = [], [], []
        for blocks in streams:
            b = Builder()
            b.plain = bytearray((dictionary or b"")[-32768:])
            nd = len(b.plain)
            per_block = []
            for k, (kind, body) in enumerate(blocks):
                final = k == len(blocks) - 1
                if kind == "stored":
                    b.stored(body, final)
                    continue
                recs, pos = [], len(b.plain) - nd
                for t in body:
                    if isinstance(t, Ref):
                        ls, _, le = len_symbol(t.length, t.use284)
                        ds, _, de = dist_symbol(t.dist)
                        recs.append((pos, t.length, ls, ds, le + de))
                        pos += t.length
                    else:
                        pos += 1
                (b.fixed if kind == "fixed" else b.dynamic)(body, final)
                per_block.append(recs)
            assert b.valid, name
            data, plain = b.getvalue(), bytes(b.plain[nd:])
            o = zlib.decompressobj(-15, zdict=dictionary) if dictionary else zlib.decompressobj(-15)
            assert o.decompress(data) == plain, name
            self.data.append(data)
            self.plain.append(plain)
            self.records.append(per_block)

    def batch(self, D, L):
        if self.dictionary:
            return D.Batch(self.data, lib=L, dictionaries=self.dictionary)
        return D.Batch(self.data, lib=L)


def expected(plain, recs):
    """-> (table, masks, records) of one block; a record is (x, y, its first bytes as far as the stream has them)"""
    table = [[0] * STRIDE for _ in range(NBINS)]
    masks = [[0] * ((len(recs) + 63) // 64) for _ in range(NBINS)]
    out = []
    for r, (pos, ln, ls, ds, eb) in enumerate(recs):
        row = table[ls - 257]
        for v, k in collections.Counter(plain[pos:pos + ln]).items():
            row[v] += k
        row[BIN_DIST + ds] += 1
        row[BIN_COUNT] += 1
        row[BIN_EBITS] += eb
        masks[ls - 257][r >> 6] |= 1 << (r & 63)
        out.append((ln | (ls - 257) << 9 | ds << 14 | eb << 19, pos, plain[pos:pos + 8]))
    return table, masks, out


def one_block(name, seed, *parts, **kw):
    """a stream of one dynamic block: each part is a byte count (filled by mix) or a token list"""
    rng = random.Random(seed)
    toks, n = [], 0
    for p in parts:
        if isinstance(p, int):
            p = mix(rng, p, n)
        toks += p
        n += sum(t.length if isinstance(t, Ref) else 1 for t in p)
    return Case(name, [[("dyn", toks)]], **kw)


def lits(rng, n):
    return [rng.choice(b"abcdefgh") for _ in range(n)]


_cases = None


def all_cases():
    global _cases
    if _cases is not None:
        return _cases
    T = TILE
    rng = random.Random(2718)
    cs = [one_block("tile_minus_1", 1, T - 1), one_block("tile_exact", 2, T), one_block("tile_plus_1", 3, T + 1),
          one_block("three_tiles_plus_5", 4, 3 * T + 5, large=True)]
    # the last record starts three bytes before the end of its block: z / w run past the block, into the next block in the
    # first stream and past the stream in the second
    # (dynamic blocks of a few KiB: the level executor stops on tiny dynamic ones, handbuilt_cases.LEVEL_EXEC_BAD)
    cs.append(Case("short_after_last_record", [[("dyn", mix(rng, 2000, 0) + [97, 98, 99, Ref(3, 3)]), ("dyn", mix(rng, 1500, 2006))],
                                               [("dyn", mix(rng, 2500, 0) + [97, 98, 99, Ref(3, 3)])],
                                               [("fixed", [97, 98, 99, Ref(3, 3)])]]))
    cs.append(one_block("len258_on_last_byte_of_tile", 5, T - 1, [Ref(258, 7)], 600))
    cs.append(one_block("record_across_boundary", 6, T - 100, [Ref(258, 300)], 500))
    cs.append(one_block("record_ends_on_boundary", 7, T - 10, [Ref(10, 20), Ref(5, 33)], 500))
    cs.append(one_block("literals_around_boundary", 8, T - 300, lits(rng, 600), 500))
    for nb in (63, 64, 65):   # records 0..nb-1 start in the first tile, the next hundred in the second: mask word 0 or 1 is shared
        cs.append(one_block("records_%d_before_boundary" % nb, 9, lits(rng, T - 3 * nb), [Ref(3, 1)] * nb, [Ref(4, 2)] * 100, 50))
    cs.append(one_block("no_record", 10, lits(rng, 1000)))
    cs.append(Case("stored_between_dynamic", [[("dyn", mix(rng, 3000, 0)), ("stored", bytes(lits(rng, 777))), ("dyn", mix(rng, 2500, 3777))]]))
    cs.append(Case("fixed_block", [[("fixed", mix(rng, T + 100, 0))]]))
    every = []
    for s in range(28):
        every += [Ref(LEN_BASE[s], 1 + s), Ref(LEN_BASE[s + 1] - 1, 40), 100 + s]   # the symbol's shortest and longest length
    every += [Ref(258, 9, use284=True), 120, Ref(258, 11), Ref(258, 500, use284=True), Ref(257, 3)]
    cs.append(one_block("all_29_length_symbols", 11, lits(rng, 600), every, 300))
    # every lane on one LDS address: one byte value, distance 1, length 258, 1500 times (two bins: 285 and 284 + 31)
    cs.append(Case("one_byte_flood", [[("dyn", [65] + [Ref(258, 1)] * 1200 + [Ref(258, 1, use284=True)] * 300)]], large=True))
    cs.append(Case("mixed_batch", [[("fixed", [1, 2, 3, Ref(7, 2)])],
                                   [("dyn", mix(rng, 1500, 0)), ("dyn", mix(rng, 2 * T + 900, 1500)), ("fixed", [5, 5, Ref(5, 1)])],
                                   [("dyn", mix(rng, 2 * T + 3, 0))],
                                   [("stored", b"only stored")]], large=True))
    d = bytes(rng.choice(b"abcdefgh") for _ in range(5000))
    cs.append(Case("preset_dictionary", [[("dyn", [Ref(40, 5000), Ref(3, 17)] + mix(rng, T + 50, 43))]], dictionary=d))
    cs.append(one_block("doubling_route", 12, 2 * T + 77, env={"D4G_COPY": "doubling"}))
    # more tiles than one workgroup takes: the block is cut into two spans, and the second looks its first record up
    cs.append(one_block("two_spans", 13, (SPAN_TILES + 2) * T - 3, large=True))
    _cases = cs
    return cs


def check_tables(c, D, L):
    """every block's table, masks and records through the hook against the expected ones -> list of complaints"""
    bad = []
    b = c.batch(D, L)
    try:
        k = 0
        for si, per_block in enumerate(c.records):
            plain = c.plain[si]
            for recs in per_block:
                got = b.debug_bins(k)
                table, masks, want = expected(plain, recs)
                for row in range(NBINS):
                    if got["table"][row] != table[row]:
                        diff = [(i, got["table"][row][i], table[row][i]) for i in range(STRIDE) if got["table"][row][i] != table[row][i]]
                        bad.append((c.name, "block", k, "table row", row, diff[:6]))
                    if got["masks"][row] != masks[row]:
                        bad.append((c.name, "block", k, "mask row", row))
                if len(got["records"]) != len(want):
                    bad.append((c.name, "block", k, "records", len(got["records"]), len(want)))
                    continue
                for r, ((x, y, z, w), (wx, wy, first)) in enumerate(zip(got["records"], want)):
                    if (x, y) != (wx, wy) or struct.pack("<II", z, w)[:len(first)] != first:
                        bad.append((c.name, "block", k, "record", r, (x, y, z, w), (wx, wy, first)))
                        break
                k += 1
        if k:
            if b.debug_bins(0)["n_blocks"] != k:
                bad.append((c.name, "blocks", b.debug_bins(0)["n_blocks"], k))
        try:
            b.debug_bins(k)
            bad.append((c.name, "a block index past the last is accepted"))
        except RuntimeError:
            pass
        for si, plain in enumerate(c.plain):
            if b.decoded(si) != plain:
                bad.append((c.name, "decoded bytes of stream", si))
    finally:
        b.close()
    return bad


def check_optimise(c, D, L, O, setenv):
    """the optimised streams under both executors against the oracle (a stream with a dictionary has no oracle twin: the two
    executors against each other, and the output decodes with the dictionary) -> list of complaints"""
    bad, outs = [], {}
    oracle = [None if c.dictionary else O.optimise(s, True) for s in c.data]
    for ex in ("fused", "levels"):
        setenv("D4G_EXEC", ex)
        b = c.batch(D, L).run(True)
        try:
            outs[ex] = [(b.result(i)["status"], b.result(i)["saved_bits"], b.output(i)) for i in range(len(c.data))]
        finally:
            b.close()
        for i, (status, saved, out) in enumerate(outs[ex]):
            if c.dictionary:
                if zlib.decompressobj(-15, zdict=c.dictionary).decompress(out) != c.plain[i]:
                    bad.append((c.name, ex, i, "does not decode"))
                continue
            rc, res, osaved, _, _ = oracle[i]
            if rc == 0 and (status != 0 or out != res or saved != osaved):
                bad.append((c.name, ex, i, "differs from the oracle", status, saved, osaved))
            if rc != 0 and (status == 0 or saved != 0):
                bad.append((c.name, ex, i, "the oracle leaves it unchanged", status, saved))
    if outs["fused"] != outs["levels"]:
        bad.append((c.name, "the executors differ"))
    return bad
