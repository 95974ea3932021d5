#!/usr/bin/env python3
"""Dev tool (GPU box): which executor runs the search rounds the fused and cluster kernels do not take, and what they cost.
The library comes from D4G_LIB when set (a build of another commit), else from the tree.

usage: exec_rounds.py [--runs N] [workload ...]      workloads: bench_merge_off bench_merge_on config5_mix (default: all)

Every workload runs in a child process of its own: `--runs` timed runs (ms_optimise + ms_merge of each, from the stats), then
one more with D4G_DEBUG_ROUNDS set, whose "search round" lines on stderr are counted by the executor they name.  Prints one
JSON line per workload."""
import argparse
import collections
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = ("bench_merge_off", "bench_merge_on", "config5_mix")
STAT_KEYS = ("rounds", "rounds_fused", "rounds_cluster", "fused_fallbacks", "fused_fallbacks_mid", "cluster_fallbacks", "n_blocks")
ROUND_LINE = re.compile(r"^search round \d+ \(\w+ program, (\w+)\)", re.M)


def child(name, runs):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import deft4j_amd as D
    import synth
    from deft4j_amd import shard
    D.init(0)
    seen = []

    class Counted(D.Batch):   # shard.optimise_sharded closes its batches: keep their stats first
        def close(self):
            if self.h:
                seen.append(self.stats())
            super().close()

    if name == "config5_mix":   # tests/test_gpu_parity.py::test_config5_mix_through_the_sharded_path
        streams = []
        for i in range(14):
            kind, n = synth.mixed_spec(i)
            n = max(32 << 10, n // 32)
            streams.append(synth.deflate9(synth.pngidat(n, 0x1DA7 + i) if kind == "idat" else synth.reptext(n, 0xD4F7 + i)))

        def once():
            shard.optimise_sharded([len(s) for s in streams], lambda i: streams[i], True, Counted, batch_bytes=1 << 20)
    else:                       # bench.py's default stream
        stream = synth.deflate9(synth.reptext(64 << 20, 0xD4F7))

        def once():
            Counted([stream]).run(name == "bench_merge_on").close()

    once()   # untimed: fills the device-memory pool
    ms = []
    for _ in range(runs):
        del seen[:]
        once()
        ms.append(round(sum(s["ms_optimise"] + s["ms_merge"] for s in seen), 3))
    del seen[:]
    os.environ["D4G_DEBUG_ROUNDS"] = "1"
    once()
    stats = {k: sum(s[k] for s in seen) for k in STAT_KEYS}
    print(json.dumps({"workload": name, "batches": len(seen), "stats": stats, "ms_optimise_plus_merge": ms}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--child", default=None)
    ap.add_argument("workloads", nargs="*", default=list(WORKLOADS))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.runs)
    for w in args.workloads:
        if w not in WORKLOADS:
            ap.error("unknown workload " + w)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", w, "--runs", str(args.runs)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            sys.exit("exec_rounds.py: workload %s failed with status %d" % (w, p.returncode))
        line = json.loads(p.stdout.strip().splitlines()[-1])
        line["rounds_by_executor"] = dict(collections.Counter(ROUND_LINE.findall(p.stderr)))
        line["lib"] = os.environ.get("D4G_LIB", "tree")
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
