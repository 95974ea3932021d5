"""The hand-built corpus (tests/handbuilt_cases.py), small and large cases, on the GPU against the oracle: once as one
batch and once with every case alone (a case's place in a batch changes the scan tiles), under each executor and
with cluster mode forced; a subset through the recompress loop (recompress_streams, MODE_CHEAP), which parses its
inputs the same way."""
import pytest

import handbuilt_cases as H
import oracle_compose as OC
import oracle_lib as O

pytestmark = pytest.mark.gpu

CONFIGS = {"fused": {"D4G_EXEC": "fused"},
           "cluster": {"D4G_EXEC": "fused", "D4G_CLUSTER_MIN_REFS": "2000", "D4G_FUSED_MAX_REFS": "2000"},
           "levels": {"D4G_EXEC": "levels"}}


@pytest.fixture(scope="module")
def lib():
    import deft4j_amd as D
    return D, D.init(0)


def names(cs, bad):
    return [(cs[m[0]].name,) + m[1:] if isinstance(m[0], int) else m for m in bad]


@pytest.mark.parametrize("cfg", list(CONFIGS), ids=list(CONFIGS))
def test_corpus_as_one_batch(lib, monkeypatch, cfg):
    for k, v in CONFIGS[cfg].items():
        monkeypatch.setenv(k, v)
    D, L = lib
    cs = [c for c in H.cases() if cfg in ("fused", "cluster") or c.name not in H.LEVEL_EXEC_BAD]
    assert not names(cs, H.compare(D, L, O, [c.data for c in cs], abi=cfg == "fused"))


def test_every_case_alone(lib):
    D, L = lib
    bad = []
    for c in H.cases():
        bad += [(c.name,) + m[1:] for m in H.compare(D, L, O, [c.data], abi=False)]
    assert not bad


def test_every_prefix(lib):
    D, L = lib
    cs = H.prefixes()
    assert not names(cs, H.compare_parse(D, L, O, [c.data for c in cs]))
    assert not names(cs, H.compare(D, L, O, [c.data for c in cs], merges=(True,), abi=False))


def test_subset_through_the_recompress_loop(lib):
    D, L = lib
    cs = [c.data for c in H.by_name(H.SUBSET) if len(c.data) < 40000] + [H.stored_after_huffman()]
    for merge in (True, False):
        got = D.recompress_streams(cs, D.MODE_CHEAP, merge)
        for c, g in zip(cs, got):
            want = OC.recompress(c, merge)
            assert (g["status"], g["saved_bits"], g["recompress_saved"], g["out"]) == \
                (want["status"], want["saved_bits"], want["recompress_saved"], want["out"]), (len(c), merge)
