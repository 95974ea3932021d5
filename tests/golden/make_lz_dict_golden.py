"""Regenerates the committed vectors of the encoder's preset-dictionary tests: for every small case of lz_dict_cases.py and
every (level, strategy) pair, what zlib 1.2.11 writes with deflateSetDictionary — zlib.compressobj(level, 8, -15, 8,
strategy, zdict).  lz_dict_outputs.bin packs the outputs; lz_dict_manifest.json lists them (offset, length, sha256) with the hashes of the
dictionary and the input each case was made from, so a drifting generator shows.  Run from the repository root:
    python tests/golden/make_lz_dict_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lz_dict_cases as C  # noqa: E402


def main():
    assert C.LIVE_ZLIB, "the vectors are zlib 1.2.11's"
    blob = bytearray()
    cases = []
    for name, d, data in C.small_cases():
        assert len(data) <= 8192 and len(d) <= 40000
        outs = []
        for lv, st in C.PAIRS:
            o = C.zref(data, lv, st, d)
            outs.append({"level": lv, "strategy": st, "offset": len(blob), "len": len(o), "sha256": C.sha(o)})
            blob += o
        cases.append({"name": name, "dict_len": len(d), "input_len": len(data), "dict_sha256": C.sha(d), "input_sha256": C.sha(data),
                      "outputs": outs})
    open(os.path.join(HERE, "lz_dict_outputs.bin"), "wb").write(bytes(blob))
    json.dump({"zlib": "1.2.11", "sha256": C.sha(bytes(blob)), "cases": cases}, open(os.path.join(HERE, "lz_dict_manifest.json"), "w"), indent=1)
    print(len(cases), "cases,", len(blob), "bytes")


if __name__ == "__main__":
    main()
