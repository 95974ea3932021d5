"""Device-memory ownership on the GPU: the cases of test_device_memory_hostsim.py at the same sizes.  The pool's count of
blocks handed out and not yet returned (d4g_debug_device_blocks) is the same before and after every call, and at the end
what it was at the start.  The failing cases are refused or raised by the host code; nothing goes wrong on the device."""
import pytest

import device_memory_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import deft4j_amd as D
    L = D.init(0)
    return D, L, M.warm_up(D, L)


@pytest.mark.parametrize("case", M.CASES, ids=[c.__name__ for c in M.CASES])
def test_blocks_come_back(lib, monkeypatch, case):
    D, L, _ = lib
    before = M.live_blocks(L)
    case(D, L, monkeypatch.setenv)
    assert M.live_blocks(L) == before


def test_count_at_the_end_is_the_count_at_the_start(lib):
    D, L, start = lib
    assert M.live_blocks(L) == start
