"""The static bin statistics (k_block_bins through d4g_debug_batch_bins) in the CPU emulator (tests/hostsim): the cases of
tests/bins_cases.py.

The emulator runs the tables, masks and records of every case that is not marked large (three_tiles_plus_5, one_byte_flood,
mixed_batch and two_spans are the GPU's alone: the emulator's fibers are slow), with workgroups of 64 and of 128 threads and
with spans of four tiles and of one, and the optimised output against the oracle for three cases of a few KiB (the search is
what the emulator is slowest at)."""
import os
import subprocess

import pytest

import bins_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c.name for c in C.all_cases() if not c.large]
OPTIMISED = ["short_after_last_record", "no_record", "stored_between_dynamic"]


@pytest.fixture(scope="module")
def sim():
    os.environ["D4G_SIM_BLOCK"] = "64"
    so = os.path.join(ROOT, "tests", "hostsim", "libdeft4g_hostsim.so")
    subprocess.check_call([os.path.join(ROOT, "tests", "hostsim", "build.sh")])
    import deft4j_amd as D
    L = D.load_library(so)
    D.init(0, lib=L)
    return D, L


def case(name):
    return next(c for c in C.all_cases() if c.name == name)


@pytest.mark.parametrize("name", SMALL)
def test_tables(sim, monkeypatch, name):
    D, L = sim
    c = case(name)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    assert not C.check_tables(c, D, L)


@pytest.mark.parametrize("name", ["tile_plus_1", "records_64_before_boundary", "all_29_length_symbols"])
def test_two_waves_per_workgroup(sim, monkeypatch, name):
    """128 threads: the carry of the covering bin crosses from one wave to the next"""
    monkeypatch.setenv("D4G_SIM_PARSE_THREADS", "128")
    D, L = sim
    assert not C.check_tables(case(name), D, L)


@pytest.mark.parametrize("name", ["tile_plus_1", "len258_on_last_byte_of_tile", "record_across_boundary", "record_ends_on_boundary",
                                  "records_64_before_boundary", "doubling_route"])
def test_one_tile_per_workgroup(sim, monkeypatch, name):
    """spans of one tile: a block's second workgroup looks up the first record that reaches into its span, and two
    workgroups share a mask word (with the default span the cases above run their tiles in one workgroup's loop)"""
    monkeypatch.setenv("D4G_SIM_BINS_SPAN_TILES", "1")
    D, L = sim
    c = case(name)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    assert not C.check_tables(c, D, L)


@pytest.mark.parametrize("name", OPTIMISED)
def test_optimised_output(sim, monkeypatch, name):
    import oracle_lib as O
    D, L = sim
    assert not C.check_optimise(case(name), D, L, O, monkeypatch.setenv)


def test_no_table(sim):
    """d4g_batch_parse makes no tables, and a finished run has released them: the hook says so"""
    D, L = sim
    c = case("short_after_last_record")
    for b in (c.batch(D, L).parse(), c.batch(D, L).run(False)):
        try:
            with pytest.raises(RuntimeError, match="no table"):
                b.debug_bins(0)
        finally:
            b.close()
