"""Throughput of the LZ77 encoder at zlib levels (d4g_deflate_streams_level) per (level, strategy) on three inputs:
128 x 1 MiB text members (config 3's shape), 64 MiB of PNG-like filtered rows, 8 MiB of zeros.  For each: MB/s of the
entry point (best of --reps wall-clock runs, input bytes / s), the parse's passes and re-run chunks, the parse kernels'
device time, and Python zlib's single-core MB/s on the same bytes (timed on at most --zlib-mib MiB of them).
Usage: python scripts/lz_levels_bench.py [--out FILE] [--reps N] [--inputs NAMES]"""
import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deft4j_amd as D  # noqa: E402
import synth  # noqa: E402

ZS = {0: zlib.Z_DEFAULT_STRATEGY, 1: zlib.Z_FILTERED, 2: zlib.Z_HUFFMAN_ONLY, 3: zlib.Z_RLE, 4: zlib.Z_FIXED}
SNAME = {0: "default", 1: "filtered", 2: "huffman", 3: "rle", 4: "fixed"}
PAIRS = [(lv, 0) for lv in range(1, 10)] + [(1, 1), (6, 1), (9, 1), (6, 2), (6, 3), (6, 4), (1, 4)]


def zlib_mbs(members, level, strategy, cap):
    done, t = 0, 0.0
    for m in members:
        if done >= cap:
            break
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, ZS[strategy])
        t0 = time.perf_counter()
        c.compress(m)
        c.flush()
        t += time.perf_counter() - t0
        done += len(m)
    return done / t / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lz_levels.json"))
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--zlib-mib", type=int, default=16)
    ap.add_argument("--inputs", default="text_128x1MiB,pngidat_64MiB,zeros_8MiB", help="comma-separated subset of the three")
    a = ap.parse_args()
    D.init(0)
    gens = {
        "text_128x1MiB": lambda: [synth.reptext(1 << 20, 0xD4F7 + i) for i in range(128)],
        "pngidat_64MiB": lambda: [synth.pngidat(64 << 20)],
        "zeros_8MiB": lambda: [b"\0" * (8 << 20)],
    }
    inputs = {k: gens[k]() for k in a.inputs.split(",")}
    res = {"note": "MB/s = input bytes per second of wall clock through d4g_deflate_streams_level (best of reps); "
                   "zlib_mbs = Python zlib, one core, on at most %d MiB of the same input" % a.zlib_mib, "rows": []}
    D.deflate_streams([b"warm up" * 1000], D.ENC_JVM, 0, level=1)
    for name, members in inputs.items():
        nbytes = sum(len(m) for m in members)
        for lv, st in PAIRS:
            best = None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                outs = D.deflate_streams(members, D.ENC_JVM, st, level=lv)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            b = D.EncodeBatch(members, [(i, D.ENC_JVM, st, lv) for i in range(len(members))]).run(False)
            s = b.stats()
            b.close()
            row = {"input": name, "bytes": nbytes, "level": lv, "strategy": SNAME[st], "mbs": round(nbytes / best / 1e6, 1),
                   "ms": round(best * 1e3, 1), "out_bytes": sum(len(o) for o in outs), "lz_parse_passes": s["lz_parse_passes"],
                   "lz_chunks_rerun": s["lz_chunks_rerun"], "ms_lz_sort": round(s["ms_lz_sort"], 2), "ms_lz_parse": round(s["ms_lz_parse"], 2),
                   "ms_lz_emit": round(s["ms_lz_emit"], 2), "zlib_mbs": round(zlib_mbs(members, lv, st, a.zlib_mib << 20), 1)}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
