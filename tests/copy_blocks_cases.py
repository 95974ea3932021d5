"""Streams for the two ways the parse resolves decoded bytes (D4G_COPY=blocks: block-local copies with window markers,
k_seg_symbols / k_seg_compose / k_seg_substitute; D4G_COPY=doubling: pointer jumping over the whole stream), shared by
test_copy_blocks_hostsim.py and test_gpu_copy_blocks.py.  Each case is the smallest shape that reaches one branch of the
block-local path; what a case must show beyond right bytes (segments, rounds of the window scan, the path that `auto`
takes) is stated with it and read back from d4g_stats.  Expected bytes come from the builder and from zlib, never from
the library."""
import zlib

import synth
from deflate_builder import Builder, Ref
from handbuilt_cases import text, z

# the bounds of deft4j_amd/csrc (d4g_parse.h, d4g_host.h): what the cases are sized against
WIN = 32768
GROUP_TOKENS = 511
GROUP_BYTES = 4096
SEG_TARGET_BYTES = 8192
SEG_MAX_BYTES = 1 << 20
SEG_MAX_TOKENS = 1 << 16
DISTANCE_TOO_FAR = 7


class Case:
    def __init__(self, name, data, plain, segments=1, rounds=0, auto="blocks", fails=False, large=False):
        self.name, self.data, self.plain = name, bytes(data), None if plain is None else bytes(plain)
        self.segments, self.rounds, self.auto, self.fails, self.large = segments, rounds, auto, fails, large


def built(name, b, **kw):
    data = b.getvalue()
    if b.valid:
        assert zlib.decompress(data, -15) == bytes(b.plain), name     # guards the builder
    return Case(name, data, b.plain, **kw)


def lits(data):
    return list(data)


def run_of(n):
    """tokens that decode to n bytes 'a': a literal, then copies at distance 1 (258 bytes each, and the remainder)"""
    k, r = divmod(n - 1, 258)
    assert r == 0 or r >= 3
    return [ord("a")] + [Ref(258, 1)] * k + ([Ref(r, 1)] if r else [])


def cases():
    t = bytes(text(70000, 77))
    out = []
    # a copy whose source is half window, half own output: 10 bytes before the block's start and the block's first 10
    b = Builder().dynamic(lits(t[:9000])).dynamic(lits(t[9000:9010]) + [Ref(20, 20), Ref(30, 9005)] + lits(t[100:200]), final=True)
    out.append(built("straddle_block_start", b, segments=2))
    # distance 32768 exactly: the first token of a block that starts at decoded position 32768, and once more from inside
    b = Builder().dynamic(lits(t[:WIN])).dynamic([Ref(258, WIN)] + lits(t[:40]) + [Ref(17, WIN), Ref(3, 1)], final=True)
    out.append(built("distance_32768", b, segments=2))
    # dist = 1 with len = 258; dist < len with a period that does not divide len; then the same across a segment boundary
    b = Builder().dynamic([ord("x"), Ref(258, 1)] + lits(b"abcdefg") + [Ref(100, 7), Ref(258, 5), Ref(11, 3)] + lits(t[:9000]))
    b.dynamic([Ref(258, 1), Ref(100, 7), Ref(258, 9001)], final=True)
    out.append(built("overlapping_copies", b, segments=2))
    # every token copies what the one before produced: more tokens than a group holds, then more bytes than a group holds
    b = Builder().dynamic(lits(b"ab") + [Ref(3, 2)] * (2 * GROUP_TOKENS + 100) + lits(b"xyz") + [Ref(4, 3)] * (3 * GROUP_BYTES // 4), final=True)
    out.append(built("dependency_chain", b, segments=1))
    # 40 blocks of under 1 KiB: segments of several blocks, copies that reach back over many of them
    b = Builder()
    pos = 0
    for k in range(40):
        tok = lits(t[700 * k:700 * k + 650])
        if pos > 200:
            tok += [Ref(258, min(pos, 30000 + k)), Ref(40, min(pos + 258, 5000 + 31 * k))]
        b.dynamic(tok, final=k == 39) if k % 3 else b.fixed(tok, final=k == 39)
        pos = len(b.plain)
    assert len(b.plain) > 3 * SEG_TARGET_BYTES
    out.append(built("forty_small_blocks", b, segments=4, rounds=2, large=True))
    # a stored block between two dynamic ones, copied from afterwards (alone in its segment: the blocks around it are long)
    b = Builder().dynamic(lits(t[:500])).stored(t[20000:20300]).dynamic([Ref(100, 350), Ref(50, 120)] + lits(t[:50]) + [Ref(258, 700)], final=True)
    out.append(built("stored_between_dynamic", b, segments=1))
    b = Builder().dynamic(lits(t[:9000])).stored(t[20000:29000]).dynamic([Ref(100, 8950), Ref(258, 17000)] + lits(t[:50]), final=True)
    out.append(built("stored_segment_between", b, segments=3, rounds=1))
    # a fixed-Huffman block
    b = Builder().fixed(lits(t[:300]) + [Ref(30, 200), Ref(258, 1), Ref(5, 3)], final=True)
    out.append(built("fixed_block", b))
    # the bounds of `auto`: a block exactly at each bound stays, one past it sends the stream the doubling way
    b = Builder().dynamic(run_of(SEG_MAX_BYTES), final=True)
    out.append(built("block_at_byte_bound", b, auto="blocks", large=True))
    b = Builder().dynamic(run_of(SEG_MAX_BYTES + 4), final=True)
    out.append(built("block_past_byte_bound", b, auto="doubling", large=True))
    b = Builder().dynamic(lits(t[:SEG_MAX_TOKENS - 1]), final=True)           # the end-of-block token is the 65536th
    out.append(built("block_at_token_bound", b, auto="blocks", large=True))
    b = Builder().dynamic(lits(t[:SEG_MAX_TOKENS]), final=True)
    out.append(built("block_past_token_bound", b, auto="doubling", large=True))
    # a back-reference before the start of the stream: in the first block, and from a later segment
    b = Builder().dynamic([ord("a"), Ref(3, 5)], final=True)
    out.append(Case("before_stream_start", b.getvalue(), None, fails=True))
    b = Builder().dynamic(lits(t[:9000])).dynamic(lits(t[:10]) + [Ref(3, 9011)], final=True)
    out.append(Case("before_stream_start_later_block", b.getvalue(), None, fails=True))
    out.append(Case("empty_stream", z(b""), b"", segments=1))
    r = synth.reptext(1 << 20)
    out.append(Case("reptext_1MiB", synth.deflate9(r), r, segments=2, rounds=1, large=True))
    p = synth.pngidat(1 << 20)
    out.append(Case("pngidat_1MiB", synth.deflate9(p), p, segments=2, large=True))
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES


def check_case(D, L, c, run):
    """One case alone under both forced paths and under auto: decoded bytes against the builder's / zlib's, batch results
    equal between the paths, and the branch the case is there for seen in the stats.  -> list of complaints."""
    import os
    bad = []
    seen = {}
    for mode in ("blocks", "doubling", "auto"):
        os.environ["D4G_COPY"] = mode
        try:
            b = D.Batch([c.data], lib=L)
            b.run(True) if run else b.parse()
            st = b.stats()
            res = b.result(0) if run else None
            seen[mode] = (res, b.output(0) if run and res["status"] == 0 else None, b.parse_error(0)["reason"])
            if c.fails:
                if b.parse_error(0)["reason"] != DISTANCE_TOO_FAR or (run and res["status"] != -1):
                    bad.append((c.name, mode, "should fail", seen[mode]))
            else:
                if b.decoded(0) != c.plain:
                    bad.append((c.name, mode, "decoded bytes differ"))
                took_blocks = mode == "blocks" or (mode == "auto" and c.auto == "blocks")
                if took_blocks and not (st["copy_segments"] >= c.segments and st["copy_rounds"] >= c.rounds and st["jump_rounds"] == 0):
                    bad.append((c.name, mode, "blocks path not as meant", st["copy_segments"], st["copy_rounds"], st["jump_rounds"]))
                if not took_blocks and not (st["copy_segments"] == 0 and st["copy_rounds"] == 0 and st["jump_rounds"] > 0):
                    bad.append((c.name, mode, "doubling path not taken", st["copy_segments"], st["copy_rounds"], st["jump_rounds"]))
            b.close()
        finally:
            del os.environ["D4G_COPY"]
    if not (seen["blocks"] == seen["doubling"] == seen["auto"]):
        bad.append((c.name, "results differ between the paths"))
    return bad
