"""Generates tests/golden/lz_levels.bin + lz_levels.json: what Python's zlib 1.2.11 — `compressobj(level, 8, -15, 8,
strategy)` — makes of the lz_*.bin inputs of lz_manifest.json at levels 1-8 x {DEFAULT, FILTERED, RLE, FIXED} and at
level 9 x {RLE, FIXED} (level 9 DEFAULT / FILTERED / HUFFMAN_ONLY are lz_manifest.json's own vectors).  The manifest
gives every output's length and sha256, which is what the tests check.  The output bytes themselves are packed, each
distinct output once, only for the inputs of at most PACK_MAX bytes (`offset` into lz_levels.bin; null for the others),
which keeps the file small while the larger cases stay pinned by their hashes.
Run from the repo root: python tests/golden/make_lz_levels_golden.py"""
import hashlib
import json
import os
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
PACK_MAX = 20000
STRATS = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "rle": zlib.Z_RLE, "fixed": zlib.Z_FIXED}


def combos():
    for level in range(1, 9):
        for s in STRATS:
            yield level, s
    yield 9, "rle"
    yield 9, "fixed"


def main():
    if zlib.ZLIB_RUNTIME_VERSION != "1.2.11":
        raise SystemExit("zlib %s: the vectors pin zlib 1.2.11" % zlib.ZLIB_RUNTIME_VERSION)
    man = json.load(open(os.path.join(HERE, "lz_manifest.json")))
    blob = bytearray()
    packed = {}
    entries = []
    for c in man["cases"]:
        data = open(os.path.join(HERE, "lz_%s.bin" % c["name"]), "rb").read()
        assert hashlib.sha256(data).hexdigest() == c["sha256_in"], c["name"]
        for level, s in combos():
            co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, STRATS[s])
            out = co.compress(data) + co.flush()
            h = hashlib.sha256(out).hexdigest()
            if len(data) <= PACK_MAX and h not in packed:
                packed[h] = len(blob)
                blob += out
            entries.append({"case": c["name"], "level": level, "strategy": s, "offset": packed.get(h), "len": len(out), "sha256": h})
    open(os.path.join(HERE, "lz_levels.bin"), "wb").write(bytes(blob))
    json.dump({"zlib": zlib.ZLIB_RUNTIME_VERSION, "sha256": hashlib.sha256(blob).hexdigest(), "entries": entries},
              open(os.path.join(HERE, "lz_levels.json"), "w"), indent=0)
    print("%d outputs, %d distinct packed, %d bytes" % (len(entries), len(packed), len(blob)))


if __name__ == "__main__":
    main()
