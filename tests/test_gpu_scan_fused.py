"""The header scan (k_scan_headers: prolog, code-length code, walk over the coded lengths, in one launch) on the GPU: the
batches of tests/scan_fused_cases.py against the Python model of the two predicates (tests/scan_model.py), zlib and the
oracle; every batch is also optimised and compared with the oracle, but the one of 4200 blocks, which is there for the scan's
second attempt and the probe's second read (merging thousands of blocks takes minutes)."""
import pytest

import find_streams_cases as F
import scan_fused_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import deft4j_amd as D
    return D, D.init(0)


@pytest.mark.parametrize("name", [c.name for c in C.all_cases()])
def test_case(lib, name):
    D, L = lib
    c = next(c for c in C.all_cases() if c.name == name)
    assert not C.check_case(D, L, c, run=not name.startswith("more_blocks"))


def test_find_path(lib):
    """d4g_find_streams goes through the same scan: a file's reported streams are the builder's"""
    D, L = lib
    c = F.by_name("back_to_back")[0]
    assert D.find_streams([c.data], c.kinds, c.min_decoded, lib=L) == [F.wanted(c, 0)]
