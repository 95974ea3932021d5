"""The fused search's tree step (tests/tree_step_cases.py) on the GPU: every case byte for byte against the oracle and
against the level executor, merge off and on; and, through the D4G_FUSED_STATS counters, the paths the step is meant to
take — a default header built once and registered again in a later round, a code two slots of one batch yield, a
default header refused its id, a launch that starts again with an empty code table."""
import pytest

import oracle_lib as O
import tree_step_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import deft4j_amd as D
    return D, D.init(0)


_LEVELS = {}


def both_executors(D, L, monkeypatch, name, merge, env=None):
    """-> the fused run's (d4g_stats counters, D4G_FUSED_STATS counters); asserts fused == oracle == levels"""
    a = C.streams()[name]
    res, st, buf = C.run(D, L, a, merge, env, monkeypatch)
    assert not C.check(O, a, merge, res), (name, merge, env)
    if (name, merge) not in _LEVELS:     # (no knob of the fused kernel reaches the level executor: once per input)
        lev, lst, _ = C.run(D, L, a, merge, {"D4G_EXEC": "levels"}, monkeypatch)
        assert lst["rounds_fused"] == 0
        _LEVELS[(name, merge)] = lev
    assert _LEVELS[(name, merge)] == res, (name, merge, env)
    return st, buf


@pytest.mark.parametrize("merge", [False, True], ids=["merge_off", "merge_on"])
@pytest.mark.parametrize("name", list(C.streams()))
def test_case_against_oracle_and_levels(lib, monkeypatch, name, merge):
    D, L = lib
    st, buf = both_executors(D, L, monkeypatch, name, merge)
    print(name, merge, st, buf[C.ROUNDS], buf[C.BUILT], buf[C.REREG], buf[C.SUBSTEPS], buf[C.KNOWN], buf[C.SAME_BATCH])
    assert st["fused_fallbacks"] == 0 and st["rounds_fused"] == buf[C.ROUNDS] > 0, st
    assert buf[C.BUILT] > 0 and 0 < buf[C.SUBSTEPS] <= buf[C.BUILT]
    if name in C.TWO_ROUNDS:
        assert st["rounds_fused"] >= 2, st


def test_second_round_registers_the_header_again(lib, monkeypatch):
    """One launch, two rounds: the codes of the first round that the second one's trees yield again take their default
    header from the record; launched one round at a time, the same headers are all built."""
    D, L = lib
    st, buf = both_executors(D, L, monkeypatch, C.REREG_CASE, False)
    assert st["rounds_fused"] == 2 and st["fused_relaunches"] == 0, st
    assert buf[C.REREG] > 0 and buf[C.REREG] <= buf[C.KNOWN]
    _, _, b1 = C.run(D, L, C.streams()[C.REREG_CASE], False, {"D4G_FUSED_CAP_ROUNDS": 1}, monkeypatch)
    assert b1[C.REREG] == 0 and b1[C.BUILT] == buf[C.BUILT] + buf[C.REREG], (b1[C.BUILT], buf[C.BUILT], buf[C.REREG])


def test_two_slots_of_a_batch_yield_one_new_code(lib, monkeypatch):
    """four tree slots: the second slot's read-only probe cannot see the first one's insert"""
    D, L = lib
    st, buf = both_executors(D, L, monkeypatch, C.SAME_BATCH_CASE, False)
    assert buf[C.SAME_BATCH] > 0 and st["fused_fallbacks"] == 0, (buf[C.SAME_BATCH], st)


def test_header_cap_refuses_a_default_header(lib, monkeypatch):
    D, L = lib
    for cap in C.HDR_CAPS:
        st, buf = both_executors(D, L, monkeypatch, C.REREG_CASE, False, {"D4G_FUSED_CAP_HDRS": cap})
        assert st["fused_fallbacks"] > 0 and buf[C.REFUSED_DEF] > 0, (cap, st, buf[C.REFUSED_DEF])


def test_code_cap_starts_the_next_launch_with_an_empty_table(lib, monkeypatch):
    """The launch overflows in its second round, after it has kept the first round's headers; the launch after the level
    executor's round builds every header it needs again"""
    D, L = lib
    name, cap = C.CODE_CAP
    st, buf = both_executors(D, L, monkeypatch, name, False, {"D4G_FUSED_CAP_CODES": cap})
    assert st["fused_fallbacks_mid"] > 0 and st["fused_relaunches"] > 0, st
    _, base = both_executors(D, L, monkeypatch, name, False)
    assert buf[C.BUILT] > base[C.BUILT], (buf[C.BUILT], base[C.BUILT])
