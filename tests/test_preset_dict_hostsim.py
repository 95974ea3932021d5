"""Streams written against a preset dictionary through the HIP kernels in the CPU emulator (tests/hostsim), with block
decoders of 64 and of 128 threads, under both copy paths.  The cases, their expected bytes (zlib with zdict=, or the
builder's own token bytes) and the checks are tests/preset_dict_cases.py's."""
import os
import subprocess

import pytest

import preset_dict_cases as C

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


def test_exports(sim):
    D, L = sim
    for name in ("d4g_batch_create_dict", "d4g_batch_create_dict_on", "d4g_inflate_dict", "d4g_find_streams_dict"):
        assert name in D.EXPORTS and hasattr(L, name)


@pytest.mark.parametrize("copy", C.COPY_MODES)
@pytest.mark.parametrize("lanes", [64, 128])
def test_parse(sim, monkeypatch, lanes, copy):
    """shapes 1-4: dictionary lengths, reach, straddling copies, through the windows"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", str(lanes))
    monkeypatch.setenv("D4G_COPY", copy)
    D, L = sim
    assert not C.check_parse(D, L, C.all_parse_cases())
    names = {c.name for c in C.all_parse_cases()}
    assert {"dict_len_%d" % n for n in C.DICT_LENGTHS} <= names and "reach_block2_L1_too_far" in names and "windows_five_blocks_L32768" in names


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_windows_are_segments(sim, monkeypatch, copy):
    """the five blocks are five segments of the block-local copy (four window slots, composed in two rounds)"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    monkeypatch.setenv("D4G_COPY", copy)
    D, L = sim
    c = [x for x in C.window_cases() if x.name == "windows_five_blocks_L32768"][0]
    b = D.Batch([c.data], lib=L, dictionaries=c.d).parse()
    st = b.stats()
    assert b.decoded(0) == c.plain
    assert (st["copy_segments"], st["copy_rounds"], st["jump_rounds"] > 0) == ((5, 2, False) if copy == "blocks" else (0, 0, True))
    b.close()


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_tail_only_and_empty_dictionary(sim, monkeypatch, copy):
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    monkeypatch.setenv("D4G_COPY", copy)
    C.check_tail_only(*sim)


@pytest.mark.parametrize("copy", C.COPY_MODES)
@pytest.mark.parametrize("lanes", [64, 128])
def test_mixed_batch(sim, monkeypatch, lanes, copy):
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", str(lanes))
    monkeypatch.setenv("D4G_COPY", copy)
    C.check_mixed(*sim)


def test_mixed_batch_with_verify_switch(sim, monkeypatch):
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    monkeypatch.setenv("D4G_VERIFY", "1")
    C.check_mixed(*sim)


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_merge_off_equals_the_oracle_twin(sim, monkeypatch, copy):
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "128")
    monkeypatch.setenv("D4G_COPY", copy)
    D, L = sim
    assert not C.check_twins(D, L)


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_merge_on(sim, monkeypatch, copy):
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    monkeypatch.setenv("D4G_COPY", copy)
    D, L = sim
    cs = C.merge_on_cases(("dict_len_257", "dict_len_32769", "windows_five_blocks_L32768", "windows_first_block_stored_L1000", "straddle_p1_dist3_len10",
                           "reach_block2_L4_ok"))
    assert len(cs) == 6
    C.check_merge_on(D, L, cs, monkeypatch.setenv)


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_optimise_every_case(sim, monkeypatch, copy):
    """every stream that parses, optimised with mergeBlocks by the default executor: the output decodes under zlib with the
    dictionary to the original bytes and verifies"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "128")
    monkeypatch.setenv("D4G_COPY", copy)
    D, L = sim
    assert not C.check_optimise(D, L, C.all_parse_cases(), True)[0]


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_verification(sim, monkeypatch, copy):
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    monkeypatch.setenv("D4G_COPY", copy)
    C.check_verification(*sim)


@pytest.mark.parametrize("copy", C.COPY_MODES)
@pytest.mark.parametrize("lanes", [64, 128])
def test_diagnosis_and_recovery(sim, monkeypatch, lanes, copy):
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", str(lanes))
    monkeypatch.setenv("D4G_COPY", copy)
    D, L = sim
    assert not C.check_recovery(D, L)


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_find_streams(sim, monkeypatch, copy):
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    monkeypatch.setenv("D4G_COPY", copy)
    C.check_find(*sim)


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_containers(sim, monkeypatch, copy):
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    monkeypatch.setenv("D4G_COPY", copy)
    C.check_containers(*sim)


def test_contracts(sim, monkeypatch):
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "64")
    C.check_contracts(*sim)
