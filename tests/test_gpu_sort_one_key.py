"""The LZ77 encoder on the GPU (d4g_deflate_streams / d4g_deflate_streams_level) on sort blocks whose positions all share
one hash, against live Python zlib: the block sort (d4g_block_sort_by_key under k_lz_sort) puts all 32768 positions of a
full block into one bucket, so the buckets behind it start at 32768, and every 64-position placement step is one group of
duplicates.  32770 zeros end right behind a full sort block (the last position that has three bytes is the block's last);
65600 leave 62 positions in a third block.  deflate_slow (level 9) and deflate_fast (level 1)."""
import pytest

import lz_levels_lib as LL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import deft4j_amd
    deft4j_amd.init(0)
    return deft4j_amd


@pytest.mark.parametrize("level", [9, pytest.param(1, marks=pytest.mark.skipif(not LL.LIVE_ZLIB, reason="deflate_fast is pinned to zlib 1.2.11"))])
def test_sort_block_of_one_key(D, level):
    ins = [bytes(32770), bytes(65600)]
    outs = D.deflate_streams(ins, D.ENC_JVM, D.STRATEGY_DEFAULT, level=level)
    for d, o in zip(ins, outs):
        assert o == LL.zref(d, level, 0), (len(d), level)
