"""The hand-built corpus (tests/handbuilt_cases.py) through the HIP kernels in the CPU emulator (tests/hostsim),
against the oracle: one batch of every small case, with one wave and with a whole 512-thread workgroup decoding each
block; every bit-prefix of two mixed streams; a subset under each executor and without memos."""
import os
import subprocess

import pytest

import handbuilt_cases as H
import oracle_compose as OC
import oracle_lib as O

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


def named(cases, bad):
    return [(cases[m[0]].name,) + m[1:] if isinstance(m[0], int) else m for m in bad]


def test_corpus_in_the_emulator(sim):
    """one wave per block decoder; merge on and off; the one-shot C-ABI entry points"""
    D, L = sim
    cs = H.cases("small")
    assert not named(cs, H.compare(D, L, O, [c.data for c in cs]))


def test_corpus_with_512_thread_decoders(sim, monkeypatch):
    """a whole workgroup (8 waves) per block decoder, as on the GPU: the chunk starts travel between waves"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "512")
    D, L = sim
    cs = H.cases("small")
    assert not named(cs, H.compare(D, L, O, [c.data for c in cs], merges=(True,), abi=False))


def test_cut_stored_nlen_in_the_emulator(sim):
    """A final stored block whose NLEN is cut off by EOF parses when LEN is 0 (DeflateBlockUncompressed.java:23-36 reads
    `readBits(16) & 0xffff`, and readBits returns -1 at EOF); a cut LEN does not, nor a non-final such block."""
    D, L = sim
    cs = H.by_name(["stored_nlen_cut_len0", "stored_nlen_half_len0", "stored_len_cut", "stored_nlen_cut_len5",
                    "stored_nlen_cut_len0_nonfinal", "zlib1_sync_then_stored_nlen_cut"])
    b = D.Batch([c.data for c in cs], lib=L).run(True)
    assert [b.result(i)["status"] for i in range(len(cs))] == [1, 1, -1, -1, -1, 0]
    assert [b.result(i)["consumed"] for i in (0, 1)] == [3, 4]
    b.close()


def test_every_prefix_in_the_emulator(sim):
    """Every bit-prefix of two mixed streams: every EOF path of the parse (parse only: the optimiser adds nothing here)."""
    D, L = sim
    cs = H.prefixes()
    assert not named(cs, H.compare_parse(D, L, O, [c.data for c in cs]))


@pytest.mark.parametrize("cfg", [{"D4G_EXEC": "fused"}, {"D4G_EXEC": "levels"}, {"D4G_MEMO": "0"}],
                         ids=["fused", "levels", "memo0"])
def test_subset_under_each_executor(sim, monkeypatch, cfg):
    for k, v in cfg.items():
        monkeypatch.setenv(k, v)
    D, L = sim
    cs = H.by_name([n for n in H.SUBSET if n in {c.name for c in H.cases("small")}])
    assert not named(cs, H.compare(D, L, O, [c.data for c in cs], abi=False))


def test_recompress_loop_in_the_emulator(sim):
    """CMDUtil's recompress-compare-graft loop (M/CMDUtil.java:70-105) compares stream.getSizeBits() of the optimised
    streams: their written sizes, in which a stored block behind a shrunk block pads from its new position."""
    D, L = sim
    streams = [H.by_name(["zlib1_sync_then_stored_nlen_cut"])[0].data, H.stored_after_huffman()]
    for merge in (True, False):
        for a, r in zip(streams, D.recompress_streams(streams, D.MODE_CHEAP, merge, lib=L)):
            assert r == OC.recompress(a, merge), merge


@pytest.mark.xfail(strict=True, raises=RuntimeError, reason="level executor: chain lookup fails on tiny dynamic blocks")
@pytest.mark.parametrize("mode", ["levels"])
def test_level_executor_on_tiny_dynamic_blocks(sim, monkeypatch, mode):
    monkeypatch.setenv("D4G_EXEC", mode)
    D, L = sim
    for c in H.by_name(H.LEVEL_EXEC_BAD):
        D.Batch([c.data], lib=L).run(True).close()
