"""The fused executor's exits (tests/fused_exit_cases.py) through the HIP kernels in the CPU emulator (tests/hostsim),
against the oracle and against the same batch with no cap set: table overflows in the first and in a later round of a
launch, the per-launch round limit, both together, a batch in which only some blocks overflow, the cluster kernel's
refusal, a capped case without memos, and the mask-word edges under a lowered D4G_FUSED_REG_WORDS.  Every test asserts
the path it means to take through the counters of d4g_stats."""
import os
import subprocess

import pytest

import fused_exit_cases as F
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


_UNCAPPED = {}


def uncapped(sim, key, streams, merge):
    """the batch with no cap set (run once, by the first test that needs it, before that test sets its knobs)"""
    if (key, merge) not in _UNCAPPED:
        D, L = sim
        res, st = F.run(D, L, streams, merge)
        assert not F.check(O, streams, merge, res)
        assert st["fused_fallbacks"] == st["fused_relaunches"] == st["cluster_fallbacks"] == 0, st
        _UNCAPPED[(key, merge)] = (res, st)
    return _UNCAPPED[(key, merge)]


def capped(sim, monkeypatch, env, key, streams, merge):
    """-> the counters of the batch under `env`, its results checked against the oracle and the uncapped batch"""
    base, _ = uncapped(sim, key, streams, merge)
    D, L = sim
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, str(v))
        res, st = F.run(D, L, streams, merge)
    assert not F.check(O, streams, merge, res, base), (key, env)
    return st


@pytest.mark.parametrize("table", list(F.SWEEPS_SIM))
def test_table_cap_sweep(sim, monkeypatch, table):
    """Every cap hands at least one round to the level executor.  Across the sweep: a launch that overflowed after it had
    completed a round, and one that overflowed in its first round and whose block came back to the fused kernel."""
    seen = []
    for name, caps in F.SWEEPS_SIM[table].items():
        for cap in caps:
            st = capped(sim, monkeypatch, {F.KNOB[table]: cap}, name, [F.stream(name)], False)
            print(table, name, cap, st)
            assert st["fused_fallbacks"] > 0, (name, cap, st)
            seen.append(st)
    assert any(st["fused_fallbacks_mid"] > 0 for st in seen)
    # (no launch of that run stopped after a round of its own, some rounds did run in the fused kernel, and the only way back
    # into it is an improving level-executor round: a first-round fallback was followed by a relaunch that ran)
    assert any(st["fused_fallbacks"] > 0 and st["fused_fallbacks_mid"] == 0 and st["fused_relaunches"] > 0 and st["rounds_fused"] > 0 for st in seen)


@pytest.mark.parametrize("table", list(F.ONE_CAP))
def test_one_cap_per_table_with_merge_on(sim, monkeypatch, table):
    name, cap = F.ONE_CAP[table]
    st = capped(sim, monkeypatch, {F.KNOB[table]: cap}, name, [F.stream(name)], True)
    assert st["fused_fallbacks_mid"] > 0, st


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_round_cap(sim, monkeypatch, cap):
    """D4F_INFO_MORE: the block is launched again until its chain ends; no round leaves the fused kernel"""
    a = F.stream("png64_l9")
    _, base = uncapped(sim, "png64_l9", [a], False)
    assert base["rounds_fused"] == F.ROUNDS["png64_l9"]
    st = capped(sim, monkeypatch, {"D4G_FUSED_CAP_ROUNDS": cap}, "png64_l9", [a], False)
    assert st["rounds_fused"] == base["rounds_fused"] and st["fused_relaunches"] > 0 and st["fused_fallbacks"] == 0, st


def test_round_cap_1_with_a_code_cap(sim, monkeypatch):
    """both hand-overs interleaved: every launch is one round, and the rounds that need the most codes go to the level executor"""
    st = capped(sim, monkeypatch, {"D4G_FUSED_CAP_ROUNDS": 1, "D4G_FUSED_CAP_CODES": 20}, "png64_l9", [F.stream("png64_l9")], False)
    assert 0 < st["fused_fallbacks"] < F.ROUNDS["png64_l9"] and st["fused_fallbacks_mid"] == 0, st
    assert st["rounds_fused"] + st["fused_fallbacks"] == F.ROUNDS["png64_l9"] and st["fused_relaunches"] >= 2, st


def test_mixed_batch(sim, monkeypatch):
    """20 single-block streams of different kinds, merge on, one cap that only some of them exceed, some in their first round
    and some later: the fb / next / todo bookkeeping of Batch::run_fused while the neighbours finish normally.  (The same
    blocks as one stream are the GPU file's: the emulator needs over a minute for them.)"""
    streams = F.mixed_batch()[:F.MIXED_SIM]
    st = capped(sim, monkeypatch, {"D4G_FUSED_CAP_CODES": 48}, "mixed", streams, True)
    assert st["n_blocks"] == len(streams) >= 20
    assert 0 < st["fused_fallbacks"] < st["n_blocks"] and st["fused_relaunches"] > 0, st


def test_cluster_refusal(sim, monkeypatch):
    """run_cluster returns false when the cluster kernel's round did not fit: the merge candidate goes to the level
    executor; uncapped, the cluster kernel runs it"""
    for k, v in F.CLUSTER_ENV.items():
        monkeypatch.setenv(k, v)
    a = [F.cluster_stream()]
    _, base = uncapped(sim, "cluster", a, True)
    assert base["rounds_cluster"] > 0, base
    st = capped(sim, monkeypatch, {"D4G_FUSED_CAP_MASKS": 8}, "cluster", a, True)
    assert st["cluster_fallbacks"] > 0 and st["rounds_cluster"] < base["rounds_cluster"], st


def test_capped_case_without_memos(sim, monkeypatch):
    """D4G_MEMO=0: the level executor computes every op of the round it is handed — no memo entry hides a dirty table"""
    name, cap = F.ONE_CAP["codes"]
    st = capped(sim, monkeypatch, {"D4G_MEMO": "0", F.KNOB["codes"]: cap}, name, [F.stream(name)], False)
    assert st["fused_fallbacks_mid"] > 0 and st["fused_relaunches"] > 0, st


def test_edge_blocks_are_worth_optimising():
    """on the oracle alone: every hand-built edge block shrinks, and its output holds more tokens (expanded back-references)"""
    for n in F.EDGE_REFS_SIM:
        a = F.edge_block(n)
        rc, want, saved = F.oracle(O, a, False)
        assert rc == 0 and saved > 0, n
        assert len(O.block_info(a)) == 1 and O.block_info(want)[0][1] > O.block_info(a)[0][1], n


@pytest.mark.parametrize("reg_words", [1, 4])
def test_mask_word_edges(sim, monkeypatch, reg_words):
    """Blocks of 63 / 64 / 65 and 255 / 256 / 257 back-references with the register form holding 1 and 4 mask words: the last
    lane of a word, a full word, one bit of the next, and the step from the register form to the chunked one"""
    streams = [F.edge_block(n) for n in F.EDGE_REFS_SIM]
    st = capped(sim, monkeypatch, {"D4G_FUSED_REG_WORDS": reg_words}, "edges", streams, False)
    assert st["rounds_fused"] >= 2 * len(streams) and st["fused_fallbacks"] == 0, st
