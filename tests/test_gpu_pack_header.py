"""The shared header packer (d4g_wave_pack_header, through d4g_debug_pack_header) on the GPU against the oracle:
the vectors and the comparison of the emulator test (pack_header_cases.py), every vector under every flag set."""
import pytest

import pack_header_cases as P

pytestmark = pytest.mark.gpu


def test_packer_matches_the_oracle():
    import deft4j_amd as D
    L = D.init(0)
    assert not P.mismatches(L)
