"""Shared by the encoder's preset-dictionary tests (test_lz_dict_hostsim.py, test_gpu_lz_dict.py) and by
golden/make_lz_dict_golden.py: the cases — (name, dictionary, input), the smallest shapes at which each piece of the
position-aware front end can go wrong — the reference (zlib 1.2.11 with zdict=) and the committed vectors."""
import hashlib
import json
import os
import random
import zlib

import synth

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZS = {0: zlib.Z_DEFAULT_STRATEGY, 1: zlib.Z_FILTERED, 2: zlib.Z_HUFFMAN_ONLY, 3: zlib.Z_RLE, 4: zlib.Z_FIXED}
LIVE_ZLIB = zlib.ZLIB_RUNTIME_VERSION == "1.2.11"   # the version the encoders are pinned to
# levels 1, 3 (deflate_fast), 4, 6, 9 (deflate_slow) x DEFAULT, FILTERED, RLE, FIXED, and HUFFMAN_ONLY once
PAIRS = [(lv, st) for lv in (1, 3, 4, 6, 9) for st in (0, 1, 3, 4)] + [(6, 2)]
# 1-3: the deferred insertion (the hash spans dictionary and input); 2047-2049: the first parsed chunk starts mid-chunk and
# exactly at a chunk start; 32505-32507: MAX_DIST from the input's first byte; 32767 / 32768: the input begins at sort
# block 1; 32769 / 40000: the tail rule
DICT_LENS = (1, 2, 3, 258, 262, 2047, 2048, 2049, 32505, 32506, 32507, 32767, 32768, 32769, 40000)


def zref(data, level, strategy, dictionary):
    c = zlib.compressobj(level, 8, -15, 8, ZS[strategy], dictionary)
    return c.compress(data) + c.flush()


def zref_plain(data, level, strategy):
    c = zlib.compressobj(level, 8, -15, 8, ZS[strategy])
    return c.compress(data) + c.flush()


def noise(n, seed):
    return random.Random(seed).getrandbits(8 * n).to_bytes(n, "little")


_TEXT = []


def text():
    if not _TEXT:
        _TEXT.append(synth.reptext(150000, 0xD1C7))
    return _TEXT[0]


def small_cases():
    """Inputs of a few KB: what the emulator runs at every (level, strategy) pair, and what the committed vectors hold."""
    t = text()
    c = [("prefix%d" % dl, t[:dl], t[dl:dl + 3000]) for dl in DICT_LENS]   # the dictionary is the text's own prefix
    c.append(("straddle30000", t[:30000], t[30000:35000]))                 # the input straddles the sort-block border
    for dl in (700, 2048, 32768):
        for n in (0, 1, 2, 3):
            c.append(("len%d_dict%d" % (n, dl), t[:dl], t[dl:dl + n]))
    c.append(("same8", b"abcdefgh", b"abcdefgh"))                          # the first byte is a literal: the NIL slot
    c.append(("same8_from1", b"abcdefgh", b"bcdefgh"))
    c.append(("same3000", t[:3000], t[:3000]))
    c.append(("nomatch", bytes(0x80 | b for b in noise(1000, 11)), t[5000:7000]))   # (the text is ASCII)
    c.append(("rle_xa", b"xa", b"aaaaaaaa"))
    c.append(("arun_after_text", t[:300] + b"a", b"a" * 1000))             # runs that start from the dictionary's last byte
    c.append(("arun258", b"x" + b"a" * 300, b"a" * 2000))                  # 258-matches that start in the dictionary
    png = synth.pngidat(9000)
    c.append(("pngidat", png[:5000], png[5000:8000]))
    return c


def slide_case():
    """33 000 bytes behind a 32 768-byte dictionary: past the window slide at input position 32 506"""
    t = text()
    return ("slide33000", t[:32768], t[32768:32768 + 33000])


def noise_cases():
    """stored blocks while the window base moves: block_start >= 0 in the concatenation's coordinates"""
    t = text()
    return [("noise40000_dict20000", t[:20000], noise(40000, 21)), ("noise40000_dict32768", t[:32768], noise(40000, 22))]


def long_cases():
    """about 70 000 bytes: a second slide (the GPU suite)"""
    t = text()
    png = synth.pngidat(110000)
    return [("text70000_dict32768", t[:32768], t[32768:32768 + 70000]), ("text70001_dict2049", t[:2049], t[2049:2049 + 70001]),
            ("noise70000_dict32768", t[:32768], noise(70000, 23)), ("png70000_dict30000", png[:30000], png[30000:100000]),
            ("arun70000", t[:100] + b"a", b"a" * 70000)]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def golden():
    """{(case name, level, strategy): expected bytes} of the committed vectors, and per case name the (dictionary, input)
    hashes they were made from"""
    man = json.load(open(os.path.join(G, "lz_dict_manifest.json")))
    blob = open(os.path.join(G, "lz_dict_outputs.bin"), "rb").read()
    assert sha(blob) == man["sha256"]
    want, made_from = {}, {}
    for c in man["cases"]:
        made_from[c["name"]] = (c["dict_sha256"], c["input_sha256"])
        for e in c["outputs"]:
            o = blob[e["offset"]:e["offset"] + e["len"]]
            assert sha(o) == e["sha256"]
            want[(c["name"], e["level"], e["strategy"])] = o
    return want, made_from
