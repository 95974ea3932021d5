"""The counters of a recompression run (tests/recompress_stats_cases.py) on the GPU through the C ABI: modes NONE, CHEAP,
ZOPFLI and ZOPFLI_EXTENSIVE, with and without mergeBlocks; there the Zopfli stage runs on its own host thread."""
import pytest

import recompress_stats_cases as R

pytestmark = pytest.mark.gpu


def test_recompress_counters():
    import deft4j_amd as D
    R.check(D, D.init(0))
