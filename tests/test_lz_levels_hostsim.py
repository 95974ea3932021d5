"""zlib levels 1-9 and the Z_RLE / Z_FIXED strategies (d4g_batch_create_encode_level) in the test-only CPU emulator:
deflate_fast's chunked parse over the insertion map, deflate_slow's level parameters, deflate_rle and the Z_FIXED block
choice, byte-identical to zlib 1.2.11 and to the committed vectors; encode + optimise equals the oracle's optimise of
zlib's bytes."""
import os
import random
import subprocess

import pytest

import lz_levels_lib as LL
import oracle_lib as O
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    os.environ["D4G_SIM_BLOCK"] = "64"
    so = os.path.join(ROOT, "tests", "hostsim", "libdeft4g_hostsim.so")
    subprocess.check_call([os.path.join(ROOT, "tests", "hostsim", "build.sh")])
    import deft4j_amd as D
    L = D.load_library(so)
    D.init(0, lib=L)
    return D, L


def inputs():
    rng = random.Random(0x1E7E1)
    lits = bytes(rng.randrange(256) for _ in range(16383))
    return [b"", b"q", b"qq", b"abc", synth.reptext(3000, 5), bytes(rng.randrange(256) for _ in range(1500)), b"\0" * 5000,
            b"ab" * 1500, synth.pngidat(5000), lits]


@pytest.mark.skipif(not LL.LIVE_ZLIB, reason="live comparisons need zlib 1.2.11")
def test_every_pair_in_one_batch_vs_zlib(sim):
    D, L = sim
    ins = inputs()
    specs = [(i, D.ENC_JVM, st, lv) for i in range(len(ins)) for lv, st in LL.PAIRS]
    b = D.EncodeBatch(ins, specs, lib=L).run(False)
    for k, (i, _, st, lv) in enumerate(specs):
        assert b.output(k) == LL.zref(ins[i], lv, st), (i, len(ins[i]), lv, st)
    b.close()


@pytest.mark.skipif(not LL.LIVE_ZLIB, reason="live comparisons need zlib 1.2.11")
def test_window_slide_and_block_fill(sim):
    """Past the 65 274-byte window slide and a block the last symbol fills (16 383 symbols), a few parses of each kind."""
    D, L = sim
    rng = random.Random(0x5117)
    ins = [synth.reptext(65274 + 900, 7), bytes(rng.randrange(256) for _ in range(16383))]
    pairs = ((1, 0), (3, 4), (6, 0), (9, 3))
    specs = [(i, D.ENC_JVM, st, lv) for i in range(len(ins)) for lv, st in pairs]
    b = D.EncodeBatch(ins, specs, lib=L).run(False)
    for k, (i, _, st, lv) in enumerate(specs):
        assert b.output(k) == LL.zref(ins[i], lv, st), (i, lv, st)
    b.close()


def test_golden_vectors(sim):
    """The committed vectors of the smaller cases (the GPU suite runs all of them)."""
    D, L = sim
    gold = [g for g in LL.golden() if len(g[0]) <= 30000]
    ins = [d for d, _ in gold]
    specs, want = [], []
    for i, (_, outs) in enumerate(gold):
        for lv, st, o in outs:
            specs.append((i, D.ENC_JVM, st, lv))
            want.append(o)
    b = D.EncodeBatch(ins, specs, lib=L).run(False)
    for k, sp in enumerate(specs):
        assert LL.matches(b.output(k), want[k]), sp
    b.close()


@pytest.mark.skipif(not LL.LIVE_ZLIB, reason="live comparisons need zlib 1.2.11")
def test_encode_then_optimise_equals_the_oracle(sim):
    D, L = sim
    ins = [synth.reptext(4000, 9), b"k" * 3000, synth.pngidat(4000), b""]
    specs = [(i, D.ENC_JVM, st, lv) for i in range(len(ins)) for lv, st in ((1, 0), (3, 4), (6, 0), (5, 3))]
    b = D.EncodeBatch(ins, specs, lib=L).run(True, True)
    for k, (i, _, st, lv) in enumerate(specs):
        enc = LL.zref(ins[i], lv, st)
        rc, want, saved, _, _ = O.optimise(enc, True)
        r = b.result(k)
        assert r["status"] == rc and r["saved_bits"] == saved, (i, lv, st)
        assert b.output(k) == (want if rc == 0 else enc), (i, lv, st)
        assert r["size_bits_in"] == O.size_bits(enc)
    b.close()


def test_refused_arguments(sim):
    D, L = sim
    for enc, st, lv in ((0, 0, 0), (0, 0, 10), (0, 0, -2), (0, 5, 6), (1, 0, 6), (1, 3, 9), (1, 4, 9), (1, 0, -1)):
        with pytest.raises(RuntimeError):
            D.EncodeBatch([b"abc"], [(0, enc, st, lv)], lib=L)
        with pytest.raises(RuntimeError):
            D.deflate_streams([b"abc"], enc, st, lib=L, level=lv)
    with pytest.raises(RuntimeError):                      # the level-9 entry points keep refusing strategies above 2
        D.EncodeBatch([b"abc"], [(0, 0, 3)], lib=L)
