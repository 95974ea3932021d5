"""The fused executor's exits (tests/fused_exit_cases.py) on the GPU, the full lists: every table's cap sweep over every
input with merge off and on, the per-launch round limit alone and with a code cap, a batch in which only some blocks
overflow and the same blocks as one stream, the cluster kernel's refusal, a capped case without memos, and the mask-word
edges up to the step from the register form of the mask tasks to the chunked one.  Everything is compared exactly with
the oracle and with the same batch with no cap set; every test asserts the path it means to take through the counters
of d4g_stats."""
import pytest

import fused_exit_cases as F
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import deft4j_amd as D
    return D, D.init(0)


_UNCAPPED = {}


def uncapped(lib, key, streams, merge):
    """the batch with no cap set (run once, by the first test that needs it, before that test sets its knobs)"""
    if (key, merge) not in _UNCAPPED:
        D, L = lib
        res, st = F.run(D, L, streams, merge)
        assert not F.check(O, streams, merge, res)
        assert st["fused_fallbacks"] == st["fused_relaunches"] == st["cluster_fallbacks"] == 0, st
        _UNCAPPED[(key, merge)] = (res, st)
    return _UNCAPPED[(key, merge)]


def capped(lib, monkeypatch, env, key, streams, merge):
    """-> the counters of the batch under `env`, its results checked against the oracle and the uncapped batch"""
    base, _ = uncapped(lib, key, streams, merge)
    D, L = lib
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, str(v))
        res, st = F.run(D, L, streams, merge)
    assert not F.check(O, streams, merge, res, base), (key, env)
    return st


@pytest.mark.parametrize("merge", [False, True], ids=["merge_off", "merge_on"])
@pytest.mark.parametrize("table", list(F.SWEEPS))
def test_table_cap_sweep(lib, monkeypatch, table, merge):
    """Every cap hands at least one round to the level executor.  Across the sweep: a launch that overflowed after it had
    completed a round, and one that overflowed in its first round and whose block came back to the fused kernel."""
    seen = []
    for name, caps in F.SWEEPS[table].items():
        _, base = uncapped(lib, name, [F.stream(name)], merge)
        assert base["n_blocks"] == 1 and base["rounds_fused"] == F.ROUNDS[name], (name, base)
        for cap in caps:
            st = capped(lib, monkeypatch, {F.KNOB[table]: cap}, name, [F.stream(name)], merge)
            print(table, name, cap, st)
            assert st["fused_fallbacks"] > 0, (name, cap, st)
            assert st["rounds_fused"] + st["fused_fallbacks"] == F.ROUNDS[name], (name, cap, st)
            seen.append(st)
    assert any(st["fused_fallbacks_mid"] > 0 for st in seen)
    # (no launch of that run stopped after a round of its own, some rounds did run in the fused kernel, and the only way back
    # into it is an improving level-executor round: a first-round fallback was followed by a relaunch that ran)
    assert any(st["fused_fallbacks"] > 0 and st["fused_fallbacks_mid"] == 0 and st["fused_relaunches"] > 0 and st["rounds_fused"] > 0 for st in seen)


@pytest.mark.parametrize("merge", [False, True], ids=["merge_off", "merge_on"])
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_round_cap(lib, monkeypatch, cap, merge):
    """D4F_INFO_MORE: the block is launched again until its chain ends; no round leaves the fused kernel"""
    for name in F.FOUR_ROUNDS:
        a = [F.stream(name)]
        _, base = uncapped(lib, name, a, merge)
        st = capped(lib, monkeypatch, {"D4G_FUSED_CAP_ROUNDS": cap}, name, a, merge)
        assert st["rounds_fused"] == base["rounds_fused"] == F.ROUNDS[name] and st["fused_relaunches"] > 0 and st["fused_fallbacks"] == 0, (name, st)


@pytest.mark.parametrize("merge", [False, True], ids=["merge_off", "merge_on"])
def test_round_cap_1_with_a_code_cap(lib, monkeypatch, merge):
    """both hand-overs interleaved: every launch is one round, and the rounds that need the most codes go to the level executor"""
    for name in F.FOUR_ROUNDS:
        st = capped(lib, monkeypatch, {"D4G_FUSED_CAP_ROUNDS": 1, "D4G_FUSED_CAP_CODES": 20}, name, [F.stream(name)], merge)
        assert 0 < st["fused_fallbacks"] < F.ROUNDS[name] and st["fused_fallbacks_mid"] == 0, (name, st)
        assert st["rounds_fused"] + st["fused_fallbacks"] == F.ROUNDS[name] and st["fused_relaunches"] >= 2, (name, st)


@pytest.mark.parametrize("merge", [False, True], ids=["merge_off", "merge_on"])
@pytest.mark.parametrize("table,cap", [("masks", 90), ("codes", 40), ("hdrs", 100)])
def test_mixed_batch(lib, monkeypatch, table, cap, merge):
    """24 single-block streams of different kinds, one cap that only some of them exceed: the fb / next / todo bookkeeping of
    Batch::run_fused while the neighbours finish normally"""
    streams = F.mixed_batch()
    st = capped(lib, monkeypatch, {F.KNOB[table]: cap}, "mixed", streams, merge)
    assert st["n_blocks"] == len(streams) >= 20
    assert 0 < st["fused_fallbacks"] < st["n_blocks"] and st["fused_relaunches"] > 0, st


@pytest.mark.parametrize("table,cap", [("masks", 90), ("codes", 40)])
def test_mixed_blocks_as_one_stream(lib, monkeypatch, table, cap):
    """the same blocks as one stream, merge on: capped rounds of parsed blocks and of merge candidates"""
    one = [F.as_one_stream(F.mixed_batch(), O.size_bits)]
    st = capped(lib, monkeypatch, {F.KNOB[table]: cap}, "mixed_one", one, True)
    assert st["n_blocks"] == len(F.mixed_batch()) and st["fused_fallbacks"] > 0, st


def test_cluster_refusal(lib, monkeypatch):
    """run_cluster returns false when the cluster kernel's round did not fit: the merge candidate goes to the level
    executor; uncapped, the cluster kernel runs it"""
    for k, v in F.CLUSTER_ENV.items():
        monkeypatch.setenv(k, v)
    a = [F.cluster_stream()]
    _, base = uncapped(lib, "cluster", a, True)
    assert base["rounds_cluster"] > 0, base
    st = capped(lib, monkeypatch, {"D4G_FUSED_CAP_MASKS": 8}, "cluster", a, True)
    assert st["cluster_fallbacks"] > 0 and st["rounds_cluster"] < base["rounds_cluster"], st


@pytest.mark.parametrize("table", list(F.ONE_CAP))
def test_capped_case_without_memos(lib, monkeypatch, table):
    """D4G_MEMO=0: the level executor computes every op of the round it is handed — no memo entry hides a dirty table"""
    name, cap = F.ONE_CAP[table]
    st = capped(lib, monkeypatch, {"D4G_MEMO": "0", F.KNOB[table]: cap}, name, [F.stream(name)], False)
    assert st["fused_fallbacks_mid"] > 0 and st["fused_relaunches"] > 0, st


def worth_optimising(n):
    """on the oracle alone: the hand-built block shrinks, and its output holds more tokens (expanded back-references)"""
    a = F.edge_block(n)
    rc, want, saved = F.oracle(O, a, False)
    assert rc == 0 and saved > 0, n
    assert len(O.block_info(a)) == 1 and O.block_info(want)[0][1] > O.block_info(a)[0][1], n
    return a


def test_mask_word_edges(lib):
    """One batch of blocks with 1 ... 16384 back-references: the last lane of a mask word, a full word, one bit of the next, at
    1, 4, 64 and 256 words — the most the register form of the mask tasks holds"""
    streams = [worth_optimising(n) for n in F.EDGE_REFS]
    _, st = uncapped(lib, "edges", streams, False)
    # `rounds` counts the fused pass once and every fix-point round of the level executor: 1 = no block left k_search_fused
    assert st["n_blocks"] == len(streams) and st["rounds_fused"] >= 2 * len(streams) and st["rounds"] == 1, st
    # 16384 is the most Batch::phase1 hands the fused kernel by default: that block as a batch of its own
    one = [F.edge_block(16384)]
    _, st = uncapped(lib, "edge_16384", one, False)
    assert st["rounds_fused"] >= 2 and st["rounds"] == 1, st


def test_mask_word_edges_in_the_chunked_form(lib, monkeypatch):
    """16385 and 16449 back-references are 257 and 258 mask words: with D4G_FUSED_MAX_REFS raised the fused kernel takes them,
    in the chunked form of its mask tasks; left alone they are the level executor's (the uncapped batch)"""
    streams = [worth_optimising(n) for n in F.EDGE_REFS_CHUNKED]
    _, base = uncapped(lib, "edges_chunked", streams, False)
    assert base["rounds_fused"] == 0 and base["rounds"] >= 2, base
    st = capped(lib, monkeypatch, {"D4G_FUSED_MAX_REFS": 131072}, "edges_chunked", streams, False)
    assert st["rounds_fused"] >= 2 * len(streams) and st["fused_fallbacks"] == 0 and st["rounds"] == 1, st
