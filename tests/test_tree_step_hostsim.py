"""The fused search's tree step (tests/tree_step_cases.py) through the HIP kernels in the CPU emulator (tests/hostsim):
every case byte for byte against the oracle and against the level executor, merge off and on; and, through the
D4G_FUSED_STATS counters, the paths the step is meant to take — a default header built once and registered again in a
later round, a code two slots of one batch yield, a default header refused its id, a launch that starts again with an
empty code table.  One check runs on the oracle alone: the cases are what the other tests take them for."""
import os
import subprocess

import pytest

import oracle_lib as O
import tree_cases as T
import tree_step_cases as C

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


def test_the_cases_are_what_they_are_taken_for():
    """On the oracle alone: every case shrinks and stays one block (an improving round is followed by another, so each has
    two rounds or more: the emulator tests read the count from the fused kernel's round counter); deep_cl's output
    carries the designed lengths, whose default header needs a code-length tree deeper than 7; dist_1 keeps exactly one
    distance symbol, the literal cases have none."""
    for name, a in C.streams().items():
        rc, want, saved = C.F.oracle(O, a, False)
        assert rc == 0 and saved > 0, name
        assert len(O.block_info(want)) == len(O.block_info(a)), name
    data, hist, lens = C.deep_cl()
    assert T.tree_of(hist)[:257] == lens
    kind, ll, dl = T.first_huffman_header(C.F.oracle(O, data, False)[1])
    assert kind == "dynamic" and ll[:257] == lens and not any(dl)
    assert C.cl_depth(lens, [0]) > 7
    kind, _, dl = T.first_huffman_header(C.F.oracle(O, C.streams()["dist_1"], False)[1])
    assert kind == "dynamic" and sum(1 for x in dl if x) == 1
    kind, _, dl = T.first_huffman_header(C.F.oracle(O, C.streams()["lit_63_ties"], False)[1])
    assert kind == "dynamic" and not any(dl)


@pytest.mark.parametrize("merge", [False, True], ids=["merge_off", "merge_on"])
@pytest.mark.parametrize("name", list(C.streams()))
def test_case_against_oracle_and_levels(sim, monkeypatch, name, merge):
    D, L = sim
    st, buf = both_executors(D, L, monkeypatch, name, merge)
    print(name, merge, st, buf[C.ROUNDS], buf[C.BUILT], buf[C.REREG], buf[C.SUBSTEPS], buf[C.KNOWN])
    assert st["fused_fallbacks"] == 0 and st["rounds_fused"] == buf[C.ROUNDS] > 0, st
    assert buf[C.BUILT] > 0 and 0 < buf[C.SUBSTEPS] <= buf[C.BUILT]
    if name in C.TWO_ROUNDS:
        assert st["rounds_fused"] >= 2, st


def test_second_round_registers_the_header_again(sim, monkeypatch):
    """One launch, two rounds: the codes of the first round that the second one's trees yield again take their default
    header from the record — as many registrations as built trees that met such a code for the first time in the round,
    and every header built belongs to a code of its own (the table is not emptied: as many as codes inserted by a tree)."""
    D, L = sim
    st, buf = both_executors(D, L, monkeypatch, C.REREG_CASE, False)
    assert st["rounds_fused"] == 2 and st["fused_relaunches"] == 0, st
    assert buf[C.REREG] > 0 and buf[C.REREG] <= buf[C.KNOWN]
    one_round, _, b1 = C.run(D, L, C.streams()[C.REREG_CASE], False, {"D4G_FUSED_CAP_ROUNDS": 1}, monkeypatch)
    assert b1[C.REREG] == 0 and b1[C.BUILT] == buf[C.BUILT] + buf[C.REREG], (b1[C.BUILT], buf[C.BUILT], buf[C.REREG])


def test_two_slots_of_a_batch_yield_one_new_code(sim, monkeypatch):
    """512 threads, four tree slots: the second slot's read-only probe cannot see the first one's insert"""
    D, L = sim
    monkeypatch.setenv("D4G_SIM_BLOCK", "512")
    st, buf = both_executors(D, L, monkeypatch, C.SAME_BATCH_CASE, False)
    assert buf[C.SAME_BATCH] > 0 and st["fused_fallbacks"] == 0, (buf[C.SAME_BATCH], st)


def test_header_cap_refuses_a_default_header(sim, monkeypatch):
    D, L = sim
    for cap in C.HDR_CAPS:
        st, buf = both_executors(D, L, monkeypatch, C.REREG_CASE, False, {"D4G_FUSED_CAP_HDRS": cap})
        assert st["fused_fallbacks"] > 0 and buf[C.REFUSED_DEF] > 0, (cap, st, buf[C.REFUSED_DEF])


def test_code_cap_starts_the_next_launch_with_an_empty_table(sim, monkeypatch):
    """The launch overflows in its second round, after it has kept the first round's headers; the launch after the level
    executor's round builds every header it needs again"""
    D, L = sim
    name, cap = C.CODE_CAP
    st, buf = both_executors(D, L, monkeypatch, name, False, {"D4G_FUSED_CAP_CODES": cap})
    assert st["fused_fallbacks_mid"] > 0 and st["fused_relaunches"] > 0, st
    _, base = both_executors(D, L, monkeypatch, name, False)
    assert buf[C.BUILT] > base[C.BUILT], (buf[C.BUILT], base[C.BUILT])
