"""Streams written against a preset dictionary on the GPU through the C ABI, with the 512-thread block decoders, under both
copy paths; and one block of more than 65 536 tokens under D4G_COPY=auto, which the router itself sends the doubling way
with its dictionary.  The cases, their expected bytes (zlib with zdict=, or the builder's own token bytes) and the checks
are tests/preset_dict_cases.py's."""
import pytest

import preset_dict_cases as C
from deflate_builder import Ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import deft4j_amd as D
    return D, D.init(0)


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_parse(lib, monkeypatch, copy):
    """shapes 1-4: dictionary lengths, reach, straddling copies, through the windows"""
    monkeypatch.setenv("D4G_COPY", copy)
    D, L = lib
    assert not C.check_parse(D, L, C.all_parse_cases())


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_tail_only_and_empty_dictionary(lib, monkeypatch, copy):
    monkeypatch.setenv("D4G_COPY", copy)
    C.check_tail_only(*lib)


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_mixed_batch(lib, monkeypatch, copy):
    monkeypatch.setenv("D4G_COPY", copy)
    C.check_mixed(*lib)


def test_mixed_batch_with_verify_switch(lib, monkeypatch):
    monkeypatch.setenv("D4G_VERIFY", "1")
    C.check_mixed(*lib)


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_merge_off_equals_the_oracle_twin(lib, monkeypatch, copy):
    monkeypatch.setenv("D4G_COPY", copy)
    D, L = lib
    assert not C.check_twins(D, L)


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_merge_on(lib, monkeypatch, copy):
    monkeypatch.setenv("D4G_COPY", copy)
    D, L = lib
    assert not C.check_optimise(D, L, C.all_parse_cases(), True)[0]      # (the default executor: every case)
    C.check_merge_on(D, L, C.merge_on_cases(), monkeypatch.setenv)


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_verification(lib, monkeypatch, copy):
    monkeypatch.setenv("D4G_COPY", copy)
    C.check_verification(*lib)


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_diagnosis_and_recovery(lib, monkeypatch, copy):
    monkeypatch.setenv("D4G_COPY", copy)
    D, L = lib
    assert not C.check_recovery(D, L)


@pytest.mark.parametrize("copy", C.COPY_MODES)
def test_find_streams(lib, monkeypatch, copy):
    monkeypatch.setenv("D4G_COPY", copy)
    C.check_find(*lib)


def test_containers(lib):
    C.check_containers(*lib)


def test_contracts(lib):
    C.check_contracts(*lib)


def test_router_takes_the_doubling_path_with_a_dictionary(lib, monkeypatch):
    """about 80 KiB of literals with a reference into the dictionary every 64 bytes, one block of more than 65 536 tokens:
    under D4G_COPY=auto the stream goes the doubling way (jump_rounds > 0, no segment), and decodes to the builder's bytes,
    which zlib confirms"""
    monkeypatch.setenv("D4G_COPY", "auto")
    D, L = lib
    d = C.text(C.WIN, 17)
    lits = C.H.text(80000, 18)
    toks, p = [], 0
    for i in range(0, len(lits), 64):
        toks += lits[i:i + 64]
        p += 64
        toks.append(Ref(4 + i // 64 % 30, min(p + C.WIN, C.WIN) - (i * 7) % 3000))
        p += toks[-1].length
    assert len(toks) > 65536
    c = C.built("router_doubling", C.seeded(d).dynamic(toks, final=True), d)
    b = D.Batch([c.data], lib=L, dictionaries=d).run(True)
    st = b.stats()
    assert b.decoded(0) == c.plain and C.zinflate(b.output(0), d) == c.plain
    assert st["jump_rounds"] > 0 and st["copy_segments"] == 0 and st["dict_streams"] == 1
    assert b.verify()[0]["verdict"] in (0, 1)
    b.close()
