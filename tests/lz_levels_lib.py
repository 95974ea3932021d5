"""Shared by the level tests (test_lz_levels_hostsim.py, test_gpu_lz_levels.py): zlib 1.2.11 as the reference for every
(level, strategy) pair of d4g_batch_create_encode_level, and the committed vectors of make_lz_levels_golden.py."""
import hashlib
import json
import os
import zlib

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZS = {0: zlib.Z_DEFAULT_STRATEGY, 1: zlib.Z_FILTERED, 2: zlib.Z_HUFFMAN_ONLY, 3: zlib.Z_RLE, 4: zlib.Z_FIXED}
GOLDEN_STRATEGY = {"default": 0, "filtered": 1, "rle": 3, "fixed": 4}
LEVELS = (1, 2, 3, 4, 5, 6, 7, 8, 9)
PAIRS = [(lv, st) for lv in LEVELS for st in range(5)]
LIVE_ZLIB = zlib.ZLIB_RUNTIME_VERSION == "1.2.11"   # the version the encoders are pinned to


def zref(data, level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, ZS[strategy])
    return c.compress(data) + c.flush()


def golden():
    """[(input bytes, [(level, strategy, expected)])] in lz_manifest.json's case order; expected = (len, sha256, bytes or
    None: the bytes are packed for the smaller inputs only)"""
    man = json.load(open(os.path.join(G, "lz_manifest.json")))
    lv = json.load(open(os.path.join(G, "lz_levels.json")))
    blob = open(os.path.join(G, "lz_levels.bin"), "rb").read()
    assert hashlib.sha256(blob).hexdigest() == lv["sha256"]
    res = []
    for c in man["cases"]:
        data = open(os.path.join(G, "lz_%s.bin" % c["name"]), "rb").read()
        outs = []
        for e in lv["entries"]:
            if e["case"] == c["name"]:
                o = None
                if e["offset"] is not None:
                    o = blob[e["offset"]:e["offset"] + e["len"]]
                    assert hashlib.sha256(o).hexdigest() == e["sha256"]
                outs.append((e["level"], GOLDEN_STRATEGY[e["strategy"]], (e["len"], e["sha256"], o)))
        res.append((data, outs))
    return res


def matches(out, expected):
    """an encoder output against a golden entry: length and sha256, and the bytes where they are packed"""
    n, h, o = expected
    return len(out) == n and hashlib.sha256(out).hexdigest() == h and (o is None or out == o)
