"""A lone parse (d4g_batch_parse) of one workload, timed: usage scripts/lone_parse.py png16|members128 [reps]
(png16: 16 MiB of PNG-like rows, synth.pngidat, as one zlib-9 stream; members128: 128 streams of 1 MiB of text each).  D4G_LIB
selects another build of the library.  The inputs are kept in the system's temporary directory between processes.
Prints one JSON line: wall ms of every repetition (first = warm-up, reported apart) and the parse kernels' device ms."""
import json
import os
import pickle
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402


def member(i):
    return synth.deflate9(synth.reptext(1 << 20, 0xD4F7 + i))


def inputs(kind):
    path = os.path.join(tempfile.gettempdir(), "d4g_bench_cache", "probe_%s.pkl" % kind)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if os.path.exists(path):
        return pickle.load(open(path, "rb"))
    if kind == "png16":
        s = [synth.deflate9(synth.pngidat(16 << 20))]
    else:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(16) as pool:
            s = pool.map(member, range(128), 4)
    tmp = path + ".%d" % os.getpid()
    pickle.dump(s, open(tmp, "wb"))
    os.replace(tmp, path)
    return s


if __name__ == "__main__":
    kind = sys.argv[1]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    streams = inputs(kind)
    import deft4j_amd as D
    D.init(0)
    wall, dev, st = [], [], None
    for r in range(reps):
        b = D.Batch(streams)
        t0 = time.perf_counter()
        b.parse()
        wall.append(round((time.perf_counter() - t0) * 1e3, 3))
        st = b.stats()
        dev.append(round(st["ms_parse_kernels"], 3))
        b.close()
    print(json.dumps({"workload": kind, "lib": os.environ.get("D4G_LIB", "this"), "streams": len(streams), "bytes_in": sum(map(len, streams)),
                      "warmup_wall_ms": wall[0], "wall_ms": wall[1:], "parse_kernels_ms": dev[1:], "n_blocks": st["n_blocks"],
                      "scan_candidates": st["scan_candidates"], "kernel_launches": st["kernel_launches"]}))
