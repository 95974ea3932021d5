"""The counters of a recompression run (d4g_batch_run_recompress -> d4g_batch_stats, d4g_batch_recompress_result): what the
original batch reports once the chained batches — every compressor output's, the winners' re-optimisation — are folded
into its stats.  Shared by the emulator and the GPU test.  Nothing expected here comes from a run of the library: the sums
follow from the modes' compressor lists (C/CompressionUtil.java:44-78) and from which batch a counter describes."""
import random
import zlib

import synth

# compressors per input of a mode (CHEAP, ZOPFLI, ZOPFLI_EXTENSIVE), two of them HUFFMAN_ONLY in every mode
LIST_LENGTH = {1: 6, 2: 7, 3: 9}
ITERATIONS = 2
ORIGINALS = ["n_streams", "n_blocks", "n_tokens", "bytes_in", "bytes_decoded"]            # describe the batch's own streams
CHAINED = ["rounds", "kernel_launches", "state_launches", "search_bytes_algorithmic"]       # summed over the chained batches


def streams():
    """five streams, four of which parse; the first two decode to repetitive bytes (their entropy bound loses at once)"""
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    rng = random.Random(7)
    return [c.compress(synth.reptext(2500, 21)) + c.flush(), synth.deflate9(b"ab" * 900), b"\x07junk", synth.deflate9(b""),
            synth.deflate9(bytes(rng.getrandbits(8) for _ in range(700)))]


def integers(st):
    return {k: v for k, v in st.items() if isinstance(v, int)}


def check(D, L):
    s = streams()
    parsed = 4
    for merge in (False, True):
        b = D.Batch(s, lib=L).run(merge)
        plain = integers(b.stats())
        b.close()
        assert plain["n_streams"] == 5 and plain["recompress_outputs"] == 0
        b = D.Batch(s, lib=L).run_recompress(D.MODE_NONE, merge, ITERATIONS)
        assert integers(b.stats()) == plain
        assert [b.recompress_result(i) for i in range(5)] == [(False, 0)] * 5
        b.close()
        for mode in (D.MODE_CHEAP, D.MODE_ZOPFLI, D.MODE_ZOPFLI_EXTENSIVE):
            b = D.Batch(s, lib=L).run_recompress(mode, merge, ITERATIONS)
            st = integers(b.stats())
            what = "mode %d merge %s: %r" % (mode, merge, st)
            assert st["recompress_outputs"] + st["recompress_outputs_pruned"] == LIST_LENGTH[mode] * parsed, what
            assert st["recompress_outputs_pruned"] % 2 == 0 and 2 <= st["recompress_outputs_pruned"] <= 8, what
            assert [st[k] for k in ORIGINALS] == [plain[k] for k in ORIGINALS], what
            assert all(st[k] > plain[k] for k in CHAINED), what
            assert st["lz_symbols"] > 0 and st["lz_parse_passes"] >= 1, what
            if mode == D.MODE_CHEAP:
                assert st["zopfli_blocks"] == 0 and st["zopfli_position_iterations"] == 0, what
            else:
                assert st["zopfli_blocks"] > 0 and st["zopfli_position_iterations"] > 0, what
            grafted, saved = b.recompress_result(0)
            assert grafted and saved > 0, what
            assert b.recompress_result(2) == (False, 0), what
            b.close()
