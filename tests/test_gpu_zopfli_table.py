"""The Zopfli match table on the GPU, position by position: both table builds (the sorted buckets, and the window scan
D4G_ZF_TABLE=scan selects) and the tail tables of block ends inside the input against the oracle's zopf_match_table
(tests/zopfli_table_cases.py), and whole streams of the inputs that reach the hit cap and the window's edge."""
import functools
import zlib

import pytest

import deft4j_amd as D
import zopf_lib as Z
import zopfli_table_cases as T

pytestmark = pytest.mark.gpu

# the build varies fastest: the oracle's side of an (input, end) or (input, options) is computed once for the two of them
TABLES = [(c.name, k, b) for c in T.CASES for k in c.end_keys() for b in T.BUILDS]
STREAMS = [(n, s, 8 << 20) for n in ("cap", "edge", "two") for s in (Z.SPLIT_FIRST, Z.SPLIT_NONE)] + [("cap", Z.SPLIT_FIRST, 20000)]
STREAMS = [s + (b,) for s in STREAMS for b in T.BUILDS]


@pytest.fixture(scope="module", autouse=True)
def _init():
    D.init(0)


@pytest.mark.parametrize("name,end,build", TABLES, ids=["%s-%s-%s" % t for t in TABLES])
def test_match_table_equals_the_oracle(monkeypatch, name, end, build):
    """len16, dist16 and every sublen[3..len] of every position below the end; the case's own condition (does the input still
    reach its edge?) is asked of the oracle first"""
    c = T.BY_NAME[name]
    e = c.end(end)
    ora = T.oracle(name, e)
    if e == 0:
        c.check_condition(ora)
    else:
        c.check_ends()
    monkeypatch.setenv("D4G_ZF_TABLE", build)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    T.check(D.load_library(), c.data, e, ora, "%s, end %s, %s build:" % (name, end, build))


@functools.lru_cache(maxsize=2)
def _oracle_stream(name, split, master):
    return Z.deflate(T.BY_NAME[name].data, 2, split, 15, master, Z.LOG_PORTABLE)


@pytest.mark.parametrize("name,split,master,build", STREAMS, ids=["%s-split%d-%d-%s" % s for s in STREAMS])
def test_streams_of_the_cap_and_edge_inputs(monkeypatch, name, split, master, build):
    """what the encoder makes of those tables (a 20000-byte master block: its ends cut the table of `cap` three times)"""
    monkeypatch.setenv("D4G_ZF_TABLE", build)
    d = T.BY_NAME[name].data
    out = D.zopfli_streams([d], 2, split, 15, master)[0]
    assert out == _oracle_stream(name, split, master)
    assert zlib.decompress(out, -15) == d
