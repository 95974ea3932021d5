"""zlib levels 1-9 and the Z_RLE / Z_FIXED strategies on the GPU (d4g_batch_create_encode_level /
d4g_deflate_streams_level): byte-identical to the committed zlib 1.2.11 vectors and to live zlib, exact at the block
fill edges and on long and pathological streams with a bounded number of parse passes, encode + optimise equal to the
oracle, level 9 identical to the old entry points, level -1 = 6, and refused arguments refused."""
import os
import random
import threading
import time

import pytest

import lz_levels_lib as LL
import oracle_lib as O
import synth

pytestmark = pytest.mark.gpu
live = pytest.mark.skipif(not LL.LIVE_ZLIB, reason="live comparisons need zlib 1.2.11")


@pytest.fixture(scope="module")
def D():
    import deft4j_amd
    deft4j_amd.init(0)
    return deft4j_amd


def test_golden_vectors(D):
    gold = LL.golden()
    ins = [d for d, _ in gold]
    specs, want = [], []
    for i, (_, outs) in enumerate(gold):
        for lv, st, o in outs:
            specs.append((i, D.ENC_JVM, st, lv))
            want.append(o)
    b = D.EncodeBatch(ins, specs).run(False)
    for k, sp in enumerate(specs):
        assert LL.matches(b.output(k), want[k]), sp
    b.close()


@live
def test_ragged_inputs_every_pair_one_batch(D):
    rng = random.Random(0x1E7E)
    ins = [synth.reptext(n, 70 + i) for i, n in enumerate((1, 2, 3, 257, 2047, 2049, 32769, 65274, 65275, 200000, 1 << 20))]
    ins += [b"", b"z" * 300000, bytes(rng.choice(b"ACGT") for _ in range(150000)), os.urandom(100000), synth.pngidat(300000),
            os.urandom(40000) + synth.reptext(90000, 3), b"ab" * 60000, synth.reptext(16383 * 4, 8)[:16383 * 3 + 5], b"\0" * 70000]
    specs = [(i, D.ENC_JVM, st, lv) for i in range(len(ins)) for lv, st in LL.PAIRS]
    b = D.EncodeBatch(ins, specs).run(False)
    for k, (i, _, st, lv) in enumerate(specs):
        want = LL.zref(ins[i], lv, st)
        assert b.output(k) == want, (i, len(ins[i]), lv, st)
        assert b.result(k)["size_bits_in"] == O.size_bits(want)
    b.close()


@live
def test_exact_block_fill_edges(D):
    lits = os.urandom(16383)
    two = os.urandom(16382) + b"\x00" * 300
    for d in (lits, lits + lits, two, os.urandom(16383 * 2 - 1) + b"abcabcabcabc"):
        for lv, st in ((1, 0), (1, 4), (4, 0), (4, 1), (6, 0), (6, 4), (6, 3), (1, 3)):
            assert D.deflate_streams([d], D.ENC_JVM, st, level=lv)[0] == LL.zref(d, lv, st), (len(d), lv, st)


@live
@pytest.mark.parametrize("gen", ["reptext", "pngidat"])
def test_16mib_streams(D, gen):
    raw = getattr(synth, gen)(16 << 20, 0xD4F7)
    pairs = ((1, 0), (3, 0), (6, 0), (9, 3))
    for lv, st in pairs:   # one parse per batch: its own pass count
        b = D.EncodeBatch([raw], [(0, D.ENC_JVM, st, lv)]).run(False)
        s = b.stats()
        assert b.output(0) == LL.zref(raw, lv, st), (gen, lv, st)
        # deflate_fast converges by generations of insertion-bit changes; the others as level 9 does
        assert 1 <= s["lz_parse_passes"] <= (128 if lv <= 3 and st != 3 else 8), (gen, lv, st, s["lz_parse_passes"])
        print(gen, lv, st, "passes", s["lz_parse_passes"], "rerun", s["lz_chunks_rerun"], "parse ms %.1f" % s["ms_lz_parse"])
        b.close()


@live
def test_pathological_runs_level_1(D):
    for d in (b"\0" * (8 << 20), b"ab" * (2 << 20)):
        t = time.time()
        b = D.EncodeBatch([d], [(0, D.ENC_JVM, 0, 1)]).run(False)
        dt = time.time() - t
        assert b.output(0) == LL.zref(d, 1, 0), len(d)
        assert dt < 60, dt
        b.close()


@live
@pytest.mark.parametrize("merge", [False, True])
def test_encode_then_optimise_equals_the_oracle(D, merge):
    ins = [synth.reptext(n, 40 + i) for i, n in enumerate((5000, 70000, 300000))] + [os.urandom(30000) + synth.reptext(50000, 2), b"k" * 50000,
                                                                                   synth.pngidat(60000), b""]
    specs = [(i, D.ENC_JVM, st, lv) for i in range(len(ins)) for lv, st in ((1, 0), (1, 4), (6, 0), (6, 1), (6, 4), (9, 3))]
    b = D.EncodeBatch(ins, specs).run(True, merge)
    for k, (i, _, st, lv) in enumerate(specs):
        enc = LL.zref(ins[i], lv, st)
        rc, want, saved, _, _ = O.optimise(enc, merge)
        r = b.result(k)
        assert r["status"] == rc and r["saved_bits"] == saved, (i, lv, st)
        assert b.output(k) == (want if rc == 0 else enc), (i, lv, st)
        assert r["size_bits_in"] == O.size_bits(enc)
    b.close()


def test_level_9_through_the_new_entry_points_equals_the_old(D):
    ins = [synth.reptext(200000, 5), os.urandom(20000), b"", synth.pngidat(100000)]
    for enc in (D.ENC_JVM, D.ENC_JZLIB):
        for st in (0, 1, 2):
            old = D.deflate_streams(ins, enc, st)
            b = D.EncodeBatch(ins, [(i, enc, st, 9) for i in range(len(ins))]).run(False)
            assert [b.output(i) for i in range(len(ins))] == old, (enc, st)
            b.close()
    # 3-tuples next to 4-tuples mean level 9
    b = D.EncodeBatch(ins, [(0, D.ENC_JVM, 1), (0, D.ENC_JVM, 1, 2)]).run(False)
    assert b.output(0) == D.deflate_streams(ins[:1], D.ENC_JVM, 1)[0]
    assert b.output(1) == D.deflate_streams(ins[:1], D.ENC_JVM, 1, level=2)[0]
    b.close()


def test_default_level_is_6(D):
    ins = [synth.reptext(300000, 9), synth.pngidat(200000)]
    for st in range(5):
        assert D.deflate_streams(ins, D.ENC_JVM, st, level=-1) == D.deflate_streams(ins, D.ENC_JVM, st, level=6), st


def test_refused_arguments(D):
    import ctypes
    L = D._need()
    raw = b"abcabcabc"
    arr = (ctypes.c_char_p * 1)(raw)
    lens = (ctypes.c_size_t * 1)(len(raw))
    for enc, st, lv in ((0, 0, 0), (0, 0, 10), (0, 0, -2), (0, 5, 6), (0, -1, 6), (1, 0, 6), (1, 0, -1), (1, 3, 9), (1, 4, 9), (2, 0, 6)):
        out = (ctypes.c_void_p * 1)()
        olen = (ctypes.c_size_t * 1)(77)
        rc = L.d4g_deflate_streams_level(1, arr, lens, enc, lv, st, out, olen)
        assert rc != 0 and not out[0] and olen[0] == 0, (enc, st, lv)
        assert L.d4g_last_error()
        sp = (D.d4g_encoder_spec_level * 1)(D.d4g_encoder_spec_level(0, enc, st, lv))
        assert not L.d4g_batch_create_encode_level(1, arr, lens, 1, sp), (enc, st, lv)
        assert L.d4g_last_error()
    sp = (D.d4g_encoder_spec_level * 1)(D.d4g_encoder_spec_level(1, 0, 0, 6))   # input out of range
    assert not L.d4g_batch_create_encode_level(1, arr, lens, 1, sp)
    for st in (D.STRATEGY_RLE, D.STRATEGY_FIXED):                           # the old entry points keep refusing 3 and 4
        out = (ctypes.c_void_p * 1)()
        olen = (ctypes.c_size_t * 1)()
        assert L.d4g_deflate_streams(1, arr, lens, D.ENC_JVM, st, out, olen) != 0 and not out[0]
        sp = (D.d4g_encoder_spec * 1)(D.d4g_encoder_spec(0, D.ENC_JVM, st))
        assert not L.d4g_batch_create_encode(1, arr, lens, 1, sp)


@live
def test_two_threads_level_2(D):
    jobs = [[synth.reptext(100000 + 5000 * k, 200 + k), synth.pngidat(80000 + k)] for k in range(4)]
    want = [[LL.zref(d, 2, 0) for d in j] for j in jobs]
    got, errs = {}, []

    def worker(tid):
        try:
            for rep in range(2):
                for k in range(tid, len(jobs), 2):
                    got[(tid, rep, k)] = D.deflate_streams(jobs[k], D.ENC_JVM, 0, level=2)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert len(got) == 2 * len(jobs)
    for (tid, rep, k), r in got.items():
        assert r == want[k], (tid, rep, k)
