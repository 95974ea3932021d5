"""The static bin statistics (k_block_bins through d4g_debug_batch_bins) on the GPU: every case of tests/bins_cases.py, its
tables, masks and records entry for entry against the values computed in Python, and its optimised output against the
oracle under both executors."""
import pytest

import bins_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import deft4j_amd as D
    return D, D.init(0)


def case(name):
    return next(c for c in C.all_cases() if c.name == name)


@pytest.mark.parametrize("name", [c.name for c in C.all_cases()])
def test_tables(lib, monkeypatch, name):
    D, L = lib
    c = case(name)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    assert not C.check_tables(c, D, L)


@pytest.mark.parametrize("name", [c.name for c in C.all_cases() if c.optimise])
def test_optimised_output(lib, monkeypatch, name):
    import oracle_lib as O
    D, L = lib
    c = case(name)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    assert not C.check_optimise(c, D, L, O, monkeypatch.setenv)


def test_no_table(lib):
    """d4g_batch_parse makes no tables, and a finished run has released them: the hook says so"""
    D, L = lib
    c = case("short_after_last_record")
    for b in (c.batch(D, L).parse(), c.batch(D, L).run(False)):
        try:
            with pytest.raises(RuntimeError, match="no table"):
                b.debug_bins(0)
        finally:
            b.close()
