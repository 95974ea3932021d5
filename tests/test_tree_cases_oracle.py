"""The tree-builder corpus (tests/tree_cases.py) against the oracle alone: every stream is RFC-valid, every cell has a
case whose output carries exactly the designed histogram's tree, the limiter cells with a tree deeper than 15, and the
builder each pinning case reaches on the GPU is the intended one."""
import zlib

import deflate_builder as DB
import tree_cases as T


def test_every_stream_is_rfc_valid():
    for c in T.cases():
        assert c.tokens <= T.MAX_TOKENS
        assert zlib.decompress(c.data, -15) == c.plain, c.name


def test_header_reader_reads_what_the_builder_wrote():
    for c in T.cases()[::7]:
        kind, ll, dl = T.first_huffman_header(c.data)
        assert kind == "dynamic"
        assert [bool(x) for x in ll] == [bool(f) for f in c.lit_hist], c.name
        assert [bool(x) for x in dl] == [bool(f) for f in c.dist_hist], c.name
        assert DB.kraft(ll) == 32768


def test_every_cell_has_a_pinning_case():
    covered = {cell for c in T.cases() if T.pins(c).ok for cell in T.cells_of(c)}
    assert {c.cell for c in T.cases()} <= set(T.CELLS)
    assert not [cell for cell in T.CELLS if cell not in covered]
    # handleOne builds no distance tree: the one distance symbol has length 1, and the literal tree is still pinned
    one = [c for c in T.cases() if c.dist_used == 1]
    assert one and all(T.pins(c).ok and T.pins(c).dist is None for c in one)


def test_limiter_cells_have_a_deep_pinning_case():
    for cell in T.LIMITER_CELLS:
        deep = [c for c in T.cases() if c.cell == cell and T.pins(c).ok and
                (T.pins(c).deep_dist if cell.startswith("dist") else T.pins(c).deep_lit)]
        assert deep, cell
        for c in deep:   # the reference's own unlimited tree is deeper than 15 too, and 15 is what its limiter leaves
            h = c.dist_hist if cell.startswith("dist") else c.lit_hist
            assert max(T.tree_of(h, 40)) > 15 and max(T.tree_of(h)) == 15, c.name
    # the register queue (at most 64 used symbols) ends in d4g_tree_finish only from 20 used symbols on
    assert any(20 <= sum(1 for f in c.lit_hist if f) <= 64 for c in T.cases() if c.cell == "lit/limiter/<=64" and T.pins(c).ok)


def test_at_most_a_quarter_does_not_pin():
    bad = [(c.name, T.pins(c).why_not()) for c in T.cases() if not T.pins(c).ok]
    assert 4 * len(bad) <= len(T.cases()), bad


def test_pinning_cases_reach_the_intended_builder():
    """d4g_build_tree_wave64 counts the non-zero entries below the last non-zero one and the total weight."""
    seen = set()
    for c in T.cases():
        if not T.pins(c).ok:
            continue
        assert T.dispatch_class(c.lit_hist) == c.cls, c.name
        seen.add(c.cls)
        if c.dist_used >= 2:
            assert T.dispatch_class(c.dist_hist) == "<=64", c.name
    assert seen == {"<=64", "65-127", "128+"}
    # the thresholds from both sides
    for used, cls in ((64, "<=64"), (65, "65-127"), (127, "65-127"), (128, "128+")):
        assert [c for c in T.cases() if T.pins(c).ok and sum(1 for f in c.lit_hist if f) == used and c.cls == cls], used
    assert T.dispatch_class([1] * 3 + [(1 << 24) - 7]) == "128+" and T.dispatch_class([1] * 3 + [(1 << 24) - 8]) == "<=64"
