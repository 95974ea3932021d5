"""Runs bench.py unchanged, with the synthetic inputs of 4 MiB and more (tests/synth.py: reptext, deflate9) kept in the
system's temporary directory, so that the processes of an A/B series do not each generate the same 64 MiB text again.
Usage: scripts/bench_cached.py <bench.py arguments>"""
import os
import runpy
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402

CACHE = os.path.join(tempfile.gettempdir(), "d4g_bench_cache")
os.makedirs(CACHE, exist_ok=True)


def cached(path, make):
    if os.path.exists(path):
        with open(path, "rb") as f:
            return f.read()
    data = make()
    tmp = path + ".%d" % os.getpid()
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)
    return data


_rep, _def, _png = synth.reptext, synth.deflate9, synth.pngidat
synth.reptext = lambda n, seed=0xD4F7: cached("%s/rep_%d_%d" % (CACHE, n, seed), lambda: _rep(n, seed)) if n >= (4 << 20) else _rep(n, seed)
synth.deflate9 = lambda data, strategy=zlib.Z_DEFAULT_STRATEGY: cached(
    "%s/def_%d_%08x_%d" % (CACHE, len(data), zlib.crc32(data), strategy), lambda: _def(data, strategy)) if len(data) >= (4 << 20) else _def(data, strategy)
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
