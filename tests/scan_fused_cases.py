"""Batches for the header scan (k_scan_headers: prolog, code-length code and the walk over the coded code lengths in one
launch), shared by test_scan_fused_hostsim.py and test_gpu_scan_fused.py.  A case is a batch of streams, each at most
64 KiB, and the number of exact probes its parse must need; everything else that is asserted is computed from the
streams themselves: the scan's two counts by tests/scan_model.py, the parse result by zlib, block counts and the
optimised stream by the oracle.

exact_probes counts the blocks the parse had to probe at a position the scan did not report.  The chain of a stream starts
at bit 0 and follows the block ends, so from a case's construction it is: the stored and fixed blocks of a stream that
parses (its dynamic blocks all have complete codes, which the scan reports), and one for a stream that does not parse (the
block at which it stops: a first byte with BTYPE 3, an empty input, or a block that the input's end cuts short, which the
scan may report but the speculative probe cannot confirm)."""
import zlib

import numpy as np

import oracle_lib as O
import scan_model as M
import synth
from deflate_builder import Builder, Ref, CL_ORDER
from handbuilt_cases import text

SCAN_TILE = 4096     # D4G_SCAN_TILE of deft4j_amd/csrc/d4g_parse.h: bytes of a stream per scan workgroup
LIST_A = 2048        # D4G_SCAN_LIST_A: prolog passers a workgroup collects before it tests their code-length codes
LIST_B = 1024        # D4G_SCAN_LIST_B: candidates a workgroup collects before it walks their coded lengths
BAD_FIRST = b"\x07"  # BTYPE 3 at bit 0: the stream's only block fails at once


class Case:
    def __init__(self, name, streams, exact, note=""):
        self.name, self.streams, self.exact, self.note = name, [bytes(s) for s in streams], exact, note
        assert all(len(s) <= 65536 for s in self.streams), name


def header_at(bit, tokens=None, **dyn):
    """A stream whose last block is a dynamic block that begins exactly at bit `bit`: a stored block of text up to a byte
    boundary shortly before it, then a fixed block whose 8-bit and 9-bit literals make up the distance (3 + 8a + 9c + 7
    bits), then the block.  -> (stream, plain)"""
    t = text(70000, 31)
    n = (bit - 200) // 8 - 5
    assert n >= 0
    b = Builder().stored(t[:n])
    gap = bit - b.nbits - 10
    c = gap % 8
    a = (gap - 9 * c) // 8
    assert a >= 0 and 8 * a + 9 * c == gap
    b.fixed([ord("e")] * a + [200] * c)
    assert b.nbits == bit
    b.dynamic(tokens if tokens is not None else list(t[n:n + 400]) + [Ref(30, 100), Ref(258, 7)], final=True, **dyn)
    assert not b.valid or zlib.decompress(b.getvalue(), -15) == bytes(b.plain)
    return b.getvalue()


def longest_header_args():
    """The longest header a block with usable codes can have: all 19 code-length-code lengths sent, and every one of the
    286 + 30 lengths sent on its own with a 7-bit code (a repeat symbol would add 2..7 extra bits but stand for three
    lengths or more, so it only shortens the header): 17 + 57 + 316 x 7 = 2286 bits.  The lengths are 8 and 9 (226 + 60
    literal/length codes) and 4 and 5 (2 + 28 distance codes), whose code-length symbols take the four 7-bit codes of a
    complete code-length code; symbols 0, 1, 2, 3 and 6 hold the short codes and are never sent."""
    cl = [0] * 19
    for s, l in ((0, 1), (1, 2), (2, 3), (3, 4), (6, 5), (4, 7), (5, 7), (8, 7), (9, 7)):
        cl[s] = l
    return dict(lit_lens=[8] * 226 + [9] * 60, dist_lens=[4] * 2 + [5] * 28, cl_lens=cl, hclen=19, rle="none")


def zero_tail_args():
    """A header whose last 28 coded lengths are explicit zeros sent with the one-bit all-zero code (code-length code:
    0 -> 1 bit, 8 -> 2 bits, 9 and 1 -> 3 bits; no repeat symbols): its last 28 bits are zero, as is whatever lies
    behind a stream in memory."""
    cl = [0] * 19
    for s, l in ((0, 1), (8, 2), (9, 3), (1, 3)):
        cl[s] = l
    return dict(lit_lens=[8] * 226 + [9] * 60, dist_lens=[1, 1] + [0] * 28, hdist=30, cl_lens=cl, rle="none")


def unseen_blocks(full, n=None):
    """the stored and fixed blocks of a stream zlib wrote, by the oracle's block list; with n, those that end inside the
    first n bytes, plus the one block that the cut makes fail"""
    pos, k = 0, 0
    for typ, _, size, _, _ in O.block_info(full):
        pos += 3 + size
        if n is not None and pos > n * 8:
            return k + 1
        k += typ != 2
    return k


def cases():
    out = []
    boundary = SCAN_TILE * 8
    # tile end: the header begins d bits before the first tile boundary; its code lengths lie in the next tile (the halo)
    ends = [header_at(boundary - d) for d in (1, 7, 8, 17, 18, 73, 74, 0)]
    out.append(Case("tile_end_batch", ends, exact=2 * len(ends)))
    # lone stream: the same headers, each in a batch of its own, where the halo of the last tile is padding
    for d, s in zip((1, 7, 8, 17, 18, 73, 74, 0), ends):
        out.append(Case("tile_end_alone_%d" % d, [s], exact=2))
    # longest header, begun in the last byte of a tile; alone, and behind another stream
    t = text(3000, 32)
    long_ = header_at(boundary - 3, tokens=list(t[:1000]) + [Ref(100, 500), Ref(258, 1)], **longest_header_args())
    b = Builder().dynamic(list(t[:1000]) + [Ref(100, 500)], final=True, **longest_header_args())
    assert Builder().dynamic([], final=True, **longest_header_args()).final_end == 2286 + 9   # (the header and a 9-bit end of block)
    out.append(Case("longest_header_alone", [long_], exact=2))
    out.append(Case("longest_header_second", [ends[0], long_], exact=4))
    # two streams: the first is `whole` (one block, the longest header at bit 0, 1000 literals) cut c bytes after its header's
    # first bit, the second is `whole` itself.  The cuts straddle the bound of the code-length code (p + 17 + 3 x 19 <= nbits:
    # 9 bytes fail, 10 pass) and then end the input inside the coded lengths, where the walk must stop at a symbol that ends
    # after the last bit (pos > nbits; its other bound, pos + 14 > nbits + 64, cannot come first: pos <= nbits on entry), and
    # behind the header.
    whole = b.getvalue()
    assert zlib.decompress(whole, -15) == bytes(b.plain) and len(whole) > 600
    cuts = (1, 2, 3, 9, 10, 11, 64, 150, 285, 286, 287, 300, 600)
    two = []
    for c in cuts:
        two += [whole[:c], whole]
    out.append(Case("two_streams_cut", two, exact=len(cuts)))
    # The batch above cannot tell a walk that stops at nbits from one that runs on: every stream is followed by at least 16
    # zero bytes of padding, so the second stream's bytes are out of any walk's reach, and zeros are not how `whole`'s header
    # goes on.  Here they are: the header (begun 5 bytes before a tile end) ends in 28 zero bits, and the input is cut inside
    # them, at each byte boundary they hold.  A walk that ran on into the padding would read the header's true continuation and
    # keep the position; the model, which stops at the stream's last bit, does not.  The last cut lies behind the header,
    # which then survives.  (Each cut stream parses its stored and its fixed block and fails at the dynamic one.)
    t = text(3000, 33)
    start = boundary - 40
    full = header_at(start, tokens=list(t[:600]) + [Ref(50, 2)], **zero_tail_args())
    end = start + Builder().dynamic([], eob=False, **zero_tail_args()).nbits
    inside = [c for c in range(start // 8, end // 8 + 1) if end - 28 < c * 8 < end]
    assert len(inside) >= 3 and len(full) * 8 > end + 64
    zero_cuts = [full[:c] for c in inside] + [full[:(end + 7) // 8]]
    assert [M.scan(z)[1] for z in zero_cuts] == [[]] * len(inside) + [[start]]
    out.append(Case("cut_inside_zero_tail", zero_cuts + [full], exact=3 * len(zero_cuts) + 2))
    # overfull lists.  A tile of 0x55 passes the prolog at every other position: 16384 of a tile's positions, list A filled to
    # its last entry by every 512 bytes.  0x5e 0xdb is the densest pattern of period 2 for the whole test (model, every pattern of periods 1 and 2: 3 of its
    # 16 positions are candidates, none of period 1 is; 60 000 random patterns each of periods 3 and 4 reached 3 of 24 and 2
    # of 32, and those periods were not searched exhaustively): 6144 candidates in a tile, six times what list B holds.
    out.append(Case("overfull_prolog_list", [BAD_FIRST + b"\x55" * (2 * SCAN_TILE + 100)], exact=1))
    out.append(Case("overfull_candidate_list", [BAD_FIRST + b"\x5e\xdb" * (SCAN_TILE + 50)], exact=1))
    out.append(Case("overfull_both_and_text", [BAD_FIRST + b"\x5e\xdb" * 3000, ends[3], BAD_FIRST + b"\x55" * 5000], exact=4))
    # seeded random data: many false candidates
    for seed in (11, 12, 13):
        r = np.random.default_rng(seed).integers(0, 256, 65535, dtype=np.uint8).tobytes()
        out.append(Case("random_%d" % seed, [BAD_FIRST + r], exact=1))
    # real data: the first 64 KiB of zlib-9 streams (dynamic blocks only; the input ends inside a block)
    rep = synth.deflate9(synth.reptext(1 << 20))
    i = next(k for k in range(64) if synth.mixed_spec(k)[0] == "idat" and synth.mixed_spec(k)[1] <= (2 << 20))
    idat = synth.mixed_stream(i)[2]
    out.append(Case("real_reptext_slice", [rep[:65536]], exact=unseen_blocks(rep, 65536)))
    out.append(Case("real_idat_slice", [idat[:65536]], exact=unseen_blocks(idat, 65536)))
    small = [synth.deflate9(synth.reptext(200000)), synth.deflate9(synth.pngidat(150000))]
    out.append(Case("real_whole_small", small, exact=sum(unseen_blocks(s) for s in small)))
    # more survivors than the scan's list is first sized for (4096, or a block per 128 input bytes) and more probe hits than
    # come back with the hit count (512): 4200 blocks of 13 bytes, so the scan runs a second time with a longer list and
    # the hits are read in two parts
    b = Builder()
    for k in range(4200):
        b.dynamic([97 + k % 3, 98, 97 + k % 5], final=k == 4199)
    many = b.getvalue()
    assert zlib.decompress(many, -15) == bytes(b.plain) and len(M.scan(many)[1]) > 4096 + 100
    out.append(Case("more_blocks_than_the_list", [many], exact=0))
    # short streams: nothing, and 1, 2 and 3 bytes (an empty fixed block is 10 bits)
    out.append(Case("short_streams", [b"", b"\x03", b"\x03\x00", b"\x03\x00\x00", ends[1]], exact=4 + 2))
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES


_MODEL = {}


def model(s):
    if s not in _MODEL:
        c, k = M.scan(s)
        _MODEL[s] = (len(c), len(k))
    return _MODEL[s]


def inflate(s):
    """-> the stream's bytes when it is a complete raw DEFLATE stream, else None"""
    d = zlib.decompressobj(-15)
    try:
        plain = d.decompress(s)
    except zlib.error:
        return None
    return plain if d.eof else None


def check_case(D, L, c, run):
    """-> list of complaints.  `run`: also optimise the batch and compare every stream that parses with the oracle."""
    bad = []
    b = D.Batch(c.streams, lib=L).parse()
    st = b.stats()
    want_c, want_k = sum(model(s)[0] for s in c.streams), sum(model(s)[1] for s in c.streams)
    print(c.name, "candidates", st["scan_candidates"], want_c, "kept", st["scan_kept"], want_k, "exact", st["exact_probes"], c.exact)
    if (st["scan_candidates"], st["scan_kept"]) != (want_c, want_k):
        bad.append(("scan counts", st["scan_candidates"], st["scan_kept"], "model", want_c, want_k))
    if st["exact_probes"] != c.exact:
        bad.append(("exact probes", st["exact_probes"], c.exact))
    blocks = 0
    for i, s in enumerate(c.streams):
        plain = inflate(s)
        ok = b.parse_error(i)["reason"] == 0
        if ok != (plain is not None):
            bad.append(("status of stream", i, ok))
        elif ok:
            blocks += len(O.block_info(s, 8192))
            if b.decoded(i) != plain:
                bad.append(("decoded bytes of stream", i))
    if st["n_blocks"] != blocks:
        bad.append(("blocks", st["n_blocks"], blocks))
    b.close()
    if run and blocks:
        b = D.Batch(c.streams, lib=L).run(True)
        for i, s in enumerate(c.streams):
            rc, res, saved, _, _ = O.optimise(s, True)
            r = b.result(i)
            if rc < 0:
                if r["status"] != -1:
                    bad.append(("optimise status of stream", i, r["status"]))
            elif r["saved_bits"] != saved or (res is not None and b.output(i) != res):
                bad.append(("optimised stream differs from the oracle", i, r["saved_bits"], saved))
        b.close()
    return bad
