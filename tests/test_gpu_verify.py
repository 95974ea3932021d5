"""Round-trip verification and per-block info on the GPU, through the C ABI of libdeft4g.so.  Expected verdicts come from
the oracle (verify_cases.py)."""
import ctypes
import json
import os
import threading

import pytest

import oracle_lib as O
import synth
import verify_cases as VC

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAN = json.load(open(os.path.join(G, "manifest.json")))


@pytest.fixture(scope="module")
def D():
    import deft4j_amd
    deft4j_amd.init(0)
    return deft4j_amd


def rd(name):
    return open(os.path.join(G, name), "rb").read()


def test_pair_table(D):
    t = VC.pair_table()
    VC.check_table_covers_the_kernel_paths(t)
    want = [VC.oracle_verdict(a, b) for _, a, b, _ in t]
    got = D.verify_streams([a for _, a, _, _ in t], [b for _, _, b, _ in t])
    for (name, a, b, _), w, g in zip(t, want, got):
        assert (g["verdict"], g["first_mismatch"]) == w, name
        one = D.verify_streams([a], [b])[0]
        assert (one["verdict"], one["first_mismatch"]) == w, name


def test_compare_kernel_at_every_relative_alignment(D):
    L = D.load_library()
    data = synth.reptext(VC.TILE + VC.STEP + 16 * 40 + 11 + 15, 9)
    first = ctypes.c_int64()
    for xs in (0, 5):
        for ys in range(16):
            for n in (3, 40, 16 * 40 + 11, VC.STEP + 16 * 40 + 11, len(data) - 15):
                x = data[:n]
                head = (16 - xs) % 16
                spots = {0, n - 1, n // 2, min(n - 1, head), min(n - 1, head + 16), min(n - 1, max(0, head - 1))}
                for k in sorted(spots) + [None]:
                    y = x if k is None else VC.flip(x, k)
                    assert L.d4g_debug_verify_compare(x, xs, y, ys, n, ctypes.byref(first)) == 0
                    assert first.value == (-1 if k is None else k), (xs, ys, n, k)


def _fixture_pairs_verify(D, label):
    for merge in (True, False):
        pairs = [p for p in MAN["pairs"] if p["merge_blocks"] == merge]
        ins = [rd(p["stem"] + ".in.deflate") for p in pairs]
        b = D.Batch(ins).run(merge)
        v = b.verify()
        for i, p in enumerate(pairs):
            r = b.result(i)
            assert b.output(i) == rd(p["stem"] + ".out.deflate"), (label, p["stem"])
            assert v[i] == {"verdict": VC.OK if r["status"] == 0 else VC.SKIPPED, "first_mismatch": -1}, (label, p["stem"])
            for final in (False, True):
                data = ins[i] if not final else b.output(i)
                rows = [(x["type"], x["tokens"], x["size_bits"] - 3, x["header_bits"], x["decoded_len"]) for x in b.block_info(i, final)]
                assert rows == O.block_info(data), (label, p["stem"], final)
        b.close()


def test_all_reference_fixture_pairs_verify(D):
    assert len(MAN["pairs"]) == 30
    _fixture_pairs_verify(D, "default")


@pytest.mark.parametrize("mode", ["levels", "fused"])
def test_fixture_pairs_verify_under_each_executor(D, monkeypatch, mode):
    monkeypatch.setenv("D4G_EXEC", mode)
    _fixture_pairs_verify(D, mode)


def test_large_streams_under_the_switch_and_poked(D, monkeypatch):
    raws = [synth.reptext(16 << 20, 41), synth.pngidat(4 << 20, 42)]
    ins = [synth.deflate9(r) for r in raws]
    monkeypatch.setenv("D4G_VERIFY", "1")
    b = D.Batch(ins).run(False)
    st = b.stats()
    changed = [i for i in range(2) if b.result(i)["status"] == 0]
    assert changed == [0, 1]
    assert st["verify_streams"] == 2 and st["verify_bytes"] == sum(len(r) for r in raws) and st["ms_verify_kernels"] > 0
    print("verify of %d decoded bytes: %.3f ms wall, %.3f ms kernels; parse kernels of the run %.3f ms"
          % (st["verify_bytes"], st["ms_verify"], st["ms_verify_kernels"], st["ms_parse_kernels"]))
    outs = [b.output(i) for i in range(2)]
    assert [v["verdict"] for v in b.verify()] == [VC.OK, VC.OK]
    for i in range(2):
        b.poke_output(i, len(outs[i]) - 1, 0xFF)
    v = b.verify()
    for i in range(2):
        poked = b.output(i)
        assert poked[:-1] == outs[i][:-1] and poked[-1] == outs[i][-1] ^ 0xFF
        dec, consumed = O.inflate(poked)
        r = b.result(i)
        if dec is None:
            want = VC.PARSE
        elif consumed != len(poked) or O.size_bits(poked) != r["size_bits_in"] - r["saved_bits"]:
            want = VC.SIZE
        elif dec != raws[i]:
            want = VC.BYTES if dec[:min(len(dec), len(raws[i]))] != raws[i][:min(len(dec), len(raws[i]))] else VC.LENGTH
        else:
            want = VC.OK
        assert want < 0 and v[i]["verdict"] == want, (i, v[i], want)
    b.close()
    monkeypatch.delenv("D4G_VERIFY")
    assert [x["verdict"] for x in D.verify_streams(ins, outs)] == [VC.OK, VC.OK]


def test_one_shot_calls_under_the_switch(D, monkeypatch):
    monkeypatch.setenv("D4G_VERIFY", "1")
    t = synth.reptext(60000, 5)
    out = D.CompressionUtil(D.MODE_CHEAP).compress_many([t, t[:1000], b""])
    assert [O.inflate(o)[0] for o in out] == [t, t[:1000], b""]
    z = D.zopfli_streams([t[:12000], b""], 3)
    assert [O.inflate(o)[0] for o in z] == [t[:12000], b""]
    assert O.inflate(D.deflate_streams([t])[0])[0] == t
    res = D.recompress_streams([VC.deflate(t, 1), b"\x07garbage"], D.MODE_CHEAP)
    assert res[0]["status"] == 0 and O.inflate(res[0]["out"])[0] == t and res[1]["status"] == -1
    outs, saved, status = D.optimise_streams_sharded([VC.deflate(t, 9), b"\x07"], True)
    assert status[1] == -1 and (outs[0] is None) == (status[0] != 0)


def test_optimise_files_with_verify_gives_the_same_files(D):
    from deft4j_amd import containers as C
    for merge in (True, False):
        sel = [f for f in MAN["files"] if f["merge_blocks"] == merge]
        files = [rd(f["stem"] + ".file.in") for f in sel]
        plain = C.optimise_files(files, merge)
        assert C.optimise_files(files, merge, verify=True) == plain
        for f, (out, _) in zip(sel, plain):
            assert out == rd(f["stem"] + ".file.out"), f["stem"]


def test_two_threads_two_contexts_verify_concurrently():
    import deft4j_amd as D
    D.init(0)
    D.init_devices([0, 0])
    lib = D.load_library()
    t = VC.pair_table(150000)
    want = [VC.oracle_verdict(a, b) for _, a, b, _ in t]
    got, errs = {}, []

    def work(ctx):
        try:
            assert lib.d4g_set_device(ctx) == 0
            for _ in range(3):
                got[ctx] = [(g["verdict"], g["first_mismatch"]) for g in D.verify_streams([a for _, a, _, _ in t], [b for _, _, b, _ in t])]
                assert got[ctx] == want
        except Exception as ex:   # noqa: BLE001 (reported below, from the main thread)
            errs.append(ex)
    ts = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
    [x.start() for x in ts]
    [x.join() for x in ts]
    assert not errs, errs
    assert got[0] == want and got[1] == want
