"""Round-trip verification (d4g_batch_verify, d4g_verify_streams, D4G_VERIFY=1) and per-block info (d4g_batch_block_info)
in the test-only CPU emulator.  Expected verdicts and block lists come from the oracle."""
import ctypes
import glob
import json
import os
import subprocess

import pytest

import oracle_lib as O
import synth
import verify_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
MAN = {p["stem"]: p for p in json.load(open(os.path.join(G, "manifest.json")))["pairs"]}
STEMS = ["lz-twice-twice.s00", "deflate-store-2.s00", "text.s00", "text.s01", "text.s02", "apng_ball.s12", "apng_ball.s09"]


@pytest.fixture(scope="module")
def sim():
    os.environ["D4G_SIM_BLOCK"] = "64"
    so = os.path.join(ROOT, "tests", "hostsim", "libdeft4g_hostsim.so")
    subprocess.check_call([os.path.join(ROOT, "tests", "hostsim", "build.sh")])
    import deft4j_amd as D
    L = D.load_library(so)
    D.init(0, lib=L)
    return D, L


def rd(n):
    return open(os.path.join(G, n), "rb").read()


@pytest.fixture(scope="module")
def table():
    t = VC.pair_table()
    VC.check_table_covers_the_kernel_paths(t)
    return t


def test_pair_table_in_one_call_and_one_at_a_time(sim, table):
    D, L = sim
    want = [VC.oracle_verdict(a, b) for _, a, b, _ in table]
    assert {v for v, _ in want} == {VC.OK, VC.SKIPPED, VC.PARSE, VC.LENGTH, VC.BYTES}
    got = D.verify_streams([a for _, a, _, _ in table], [b for _, _, b, _ in table], lib=L)
    for (name, a, b, _), w, g in zip(table, want, got):
        assert (g["verdict"], g["first_mismatch"]) == w, name
        one = D.verify_streams([a], [b], lib=L)[0]
        assert (one["verdict"], one["first_mismatch"]) == w, name
    assert D.verify_streams([], [], lib=L) == []


def test_compare_kernel_at_every_relative_alignment(sim):
    """The decoded ranges the library compares all start on 16-byte boundaries, so the kernel's funnel-shift path is
    driven through its test hook: both sides at every skew against each other, lengths that give a head, whole vectors
    (with and without an unrolled step) and a tail, a difference in each part, and none."""
    D, L = sim
    data = synth.reptext(VC.STEP + 16 * 40 + 11 + 15, 9)
    first = ctypes.c_int64()
    seen = set()
    for xs in (0, 5):
        for ys in range(16):
            for n in (3, 40, 16 * 40 + 11, len(data)):
                x = data[:n]
                head = (16 - xs) % 16
                spots = {0, n - 1, n // 2, min(n - 1, head), min(n - 1, head + 16), min(n - 1, max(0, head - 1))}
                for k in sorted(spots) + [None]:
                    y = x if k is None else VC.flip(x, k)
                    assert L.d4g_debug_verify_compare(x, xs, y, ys, n, ctypes.byref(first)) == 0
                    assert first.value == (-1 if k is None else k), (xs, ys, n, k)
            seen.add((ys - xs) % 16)
    assert seen == set(range(16))          # equal alignment and every difference 1..15
    assert L.d4g_debug_verify_compare(b"", 0, b"", 3, 0, ctypes.byref(first)) == 0 and first.value == -1
    assert L.d4g_debug_verify_compare(b"a", 16, b"a", 0, 1, ctypes.byref(first)) == -2


def _check_batch(b, n, inputs=None):
    """verify() against the batch's own results: OK where the library wrote the stream, SKIPPED elsewhere."""
    v = b.verify()
    for i in range(n):
        r = b.result(i)
        want = VC.OK if r["status"] == 0 else VC.SKIPPED
        assert v[i] == {"verdict": want, "first_mismatch": -1}, i
        if r["status"] == 0:
            out = b.output(i)
            dec, consumed = O.inflate(out)
            assert consumed == len(out) == r["out_len"]
            assert dec == b.decoded(i)
    return v


@pytest.mark.parametrize("merge", [True, False])
def test_batch_run_verifies(sim, merge):
    D, L = sim
    ins = [rd(s + ".in.deflate") for s in STEMS] + [b"\x07garbage", VC.deflate(b"")]
    b = D.Batch(ins, lib=L).run(merge)
    v = _check_batch(b, len(ins))
    assert sum(1 for x in v if x["verdict"] == VC.OK) >= 3 and v[-2]["verdict"] == VC.SKIPPED
    for i in range(len(ins)):
        r = b.result(i)
        if r["status"] == 0:   # the size the caller computes from the results is the size the re-parse read
            assert O.size_bits(b.output(i)) == r["size_bits_in"] - r["saved_bits"]
    st = b.stats()
    assert st["verify_streams"] == sum(1 for x in v if x["verdict"] == VC.OK) and st["verify_bytes"] > 0
    b.close()


def test_recompress_and_encode_batches_verify(sim):
    D, L = sim
    t = synth.reptext(5000, 3)
    ins = [VC.deflate(t, 1), VC.deflate(t, 9), rd("text.s01.in.deflate"), VC.deflate(t[:300], 1, 2)]
    b = D.Batch(ins, lib=L).run_recompress(D.MODE_CHEAP, True)
    assert any(b.recompress_result(i)[0] for i in range(len(ins)))        # at least one grafted stream
    _check_batch(b, len(ins))
    for i in range(len(ins)):
        r, (grafted, rs) = b.result(i), b.recompress_result(i)
        if r["status"] == 0:
            assert O.size_bits(b.output(i)) == r["size_bits_in"] - r["saved_bits"] - rs
    b.close()
    for optimise in (False, True):
        e = D.EncodeBatch([t, t[:700], b""], [(0, D.ENC_JVM, D.STRATEGY_DEFAULT), (1, D.ENC_JZLIB, D.STRATEGY_FILTERED),
                                              (0, D.ENC_JVM, D.STRATEGY_HUFFMAN_ONLY), (2, D.ENC_JVM, D.STRATEGY_DEFAULT)], lib=L).run(optimise, True)
        v = e.verify()
        assert [x["verdict"] for x in v] == [VC.OK] * 4          # every output of an encoder batch is the library's
        e.close()


def _oracle_verdict_of_output(out, want_bits, decoded):
    dec, consumed = O.inflate(out)
    if dec is None:
        return VC.PARSE, -1
    if consumed != len(out) or O.size_bits(out) != want_bits:
        return VC.SIZE, -1
    common = min(len(dec), len(decoded))
    for k in range(common):
        if dec[k] != decoded[k]:
            return VC.BYTES, k
    if len(dec) != len(decoded):
        return VC.LENGTH, common
    return VC.OK, -1


def test_poked_output_is_refused(sim, monkeypatch):
    D, L = sim
    a = rd("text.s02.in.deflate")
    negatives = 0
    for frac, mask in ((0.05, 0x10), (0.5, 0x01), (0.6, 0x80), (0.9, 0x04)):
        b = D.Batch([a, rd("text.s01.in.deflate")], lib=L).run(True)
        r = b.result(0)
        assert r["status"] == 0
        off = int(r["out_len"] * frac)
        b.poke_output(0, off, mask)
        poked = b.output(0)
        want = _oracle_verdict_of_output(poked, r["size_bits_in"] - r["saved_bits"], b.decoded(0))
        v = b.verify()
        assert (v[0]["verdict"], v[0]["first_mismatch"]) == want, (frac, mask)
        assert v[1]["verdict"] == VC.OK
        negatives += want[0] < 0
        if want[0] in (VC.BYTES, VC.LENGTH):
            k, j = b.locate(0, want[1], final=False)
            assert 0 <= k <= len(b.block_info(0)) and j >= 0
        for bad in (r["out_len"], r["out_len"] + 1, 1 << 40):      # outside the stream's own output
            assert L.d4g_debug_batch_poke_output(b.h, 0, bad, 1) == -2
        b.close()
    assert negatives >= 3
    # the switch: the same poke cannot be made before a run returns, so show the gate on a run that is sound, and the
    # failure path through verify() above; with the switch on, runs still succeed and are counted
    monkeypatch.setenv("D4G_VERIFY", "1")
    b = D.Batch([a, b"\x07garbage"], lib=L).run(True)
    st = b.stats()
    assert st["verify_streams"] == 1 and st["verify_bytes"] == len(b.decoded(0))
    b.close()


def test_switch_counts_and_costs_nothing_when_off(sim, monkeypatch):
    D, L = sim
    ins = [rd(s + ".in.deflate") for s in STEMS[:4]]
    t = synth.reptext(3000, 8)

    changed = []

    def runs():
        out = []
        b = D.Batch(ins, lib=L).run(True)
        out.append(b.stats())
        changed.append(sum(1 for i in range(len(ins)) if b.result(i)["status"] == 0))
        b.close()
        b = D.Batch(ins[:2] + [VC.deflate(t, 1)], lib=L).run_recompress(D.MODE_CHEAP, True)
        out.append(b.stats())
        b.close()
        e = D.EncodeBatch([t], [(0, D.ENC_JVM, D.STRATEGY_DEFAULT)], lib=L).run(True, True)
        out.append(e.stats())
        e.close()
        assert D.deflate_streams([t], lib=L)[0] == synth.deflate9(t)
        res, saved, status = D.optimise_streams_sharded(ins, True, lib=L)
        assert [r is not None for r in res] == [s == 0 for s in status]
        assert D.recompress_streams([VC.deflate(t, 1)], D.MODE_CHEAP, lib=L)[0]["status"] == 0
        assert O.inflate(D.CompressionUtil(D.MODE_CHEAP, lib=L).compress(t))[0] == t
        return out

    monkeypatch.delenv("D4G_VERIFY", raising=False)
    for st in runs():
        assert st["verify_streams"] == 0 and st["verify_bytes"] == 0 and st["ms_verify"] == 0 and st["ms_verify_kernels"] == 0
    monkeypatch.setenv("D4G_VERIFY", "0")
    assert all(st["verify_streams"] == 0 for st in runs())
    monkeypatch.setenv("D4G_VERIFY", "1")
    on = runs()
    assert on[0]["verify_streams"] == changed[-1] >= 2 and on[1]["verify_streams"] >= 1 and on[2]["verify_streams"] == 1
    assert all(st["ms_verify"] > 0 for st in on)


def _rows(info):
    return [(b["type"], b["tokens"], b["size_bits"] - 3, b["header_bits"], b["decoded_len"]) for b in info]


def _check_positions(info):
    pos = 0
    for b in info:
        assert b["bit_pos"] == pos
        pos += b["size_bits"]
    assert [b["bfinal"] for b in info] == [0] * (len(info) - 1) + [1]
    return pos


def test_block_info_matches_the_oracle(sim):
    D, L = sim
    small = sorted(p for p in glob.glob(os.path.join(G, "*.in.deflate")) if os.path.getsize(p) <= 6000)
    assert len(small) >= 10
    ins = [open(p, "rb").read() for p in small]
    merges = [MAN.get(os.path.basename(p)[:-len(".in.deflate")], {}).get("merge_blocks", True) for p in small]
    for merge in (True, False):
        idx = [i for i in range(len(ins)) if merges[i] == merge and O.block_info(ins[i]) is not None]
        if not idx:
            continue
        b = D.Batch([ins[i] for i in idx], lib=L).run(merge)
        for j, i in enumerate(idx):
            info = b.block_info(j)
            assert _rows(info) == O.block_info(ins[i]), small[i]
            assert _check_positions(info) == b.result(j)["size_bits_in"]
            fin = b.block_info(j, final=True)
            r = b.result(j)
            assert _rows(fin) == O.block_info(b.output(j) if r["status"] == 0 else ins[i]), small[i]
            assert _check_positions(fin) == r["size_bits_in"] - r["saved_bits"]
            part = (D.d4g_block_info * 1)()
            n = ctypes.c_size_t()
            assert L.d4g_batch_block_info(b.h, j, 0, part, 1, ctypes.byref(n)) == 0 and n.value == len(info)
            assert part[0].size_bits == info[0]["size_bits"]
        b.close()
    # every golden output parses to the oracle's list too; the zopfli fixture's numbers are the pinned ones
    z = rd("asyoulik_asyoulik-zopfli.s00.out.deflate")
    outs = [z] + [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(G, "*.out.deflate"))) if os.path.getsize(p) <= 6000]
    b = D.Batch(outs, lib=L).parse()
    for j, o in enumerate(outs):
        assert _rows(b.block_info(j)) == O.block_info(o), j
        assert b.block_info(j, final=True) == b.block_info(j)
    assert [x["tokens"] for x in b.block_info(0)] == [553, 850, 2970, 2296, 20832]
    b.close()


def test_print_block_info_text(sim):
    D, L = sim
    a = rd("lz-twice-twice.s00.in.deflate")
    names = ("STORED", "FIXED", "DYNAMIC")

    def text(name, data):
        pos, lines = 0, ""
        for k, (ty, _, size, _, _) in enumerate(O.block_info(data)):
            lines += "\nBlock %d position %d size %d type %s" % (k, pos, size + 3, names[ty])
            pos += size + 3
        return "Stream name: " + name + "\nBlock info:" + lines + "\nTotal blocks: %d" % len(O.block_info(data))

    s = D.DeflateStream("twice", lib=L)
    assert s.parse(a)
    assert s.printBlockInfo() == text("twice", a)
    assert "Block 0 position 0 size 184 type FIXED\nBlock 1 position 184 size 29 type FIXED\nTotal blocks: 2" in s.printBlockInfo()
    s.optimise(True)
    assert s.printBlockInfo() == text("twice", s.asBytes())
    s.close()
    s = D.DeflateStream(lib=L)
    assert s.parse(rd("deflate-store-2.s00.in.deflate")) and s.printBlockInfo() == text("unnamed stream", rd("deflate-store-2.s00.in.deflate"))
    s.close()
