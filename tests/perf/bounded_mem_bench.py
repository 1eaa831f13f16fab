#!/usr/bin/env python3
"""The maximum match length of the break records and the MEM hits (gcsa2_match_breaks_bounded_device /
gcsa2_mem_hits_bounded_device) on config 5's batch: 1 M x 256-bp walks through the chr22-like snp graph (order 32), every
second one with a substitution every 41 bp; min_length 20, hit_max 64 with the SAMPLE policy.

Every figure is the median of --calls calls (HIP events around each call, after a warm-up call), taken --repeats times in
every process; the driver starts --rounds processes per library, alternating, so that the spread of one library's own
repeated medians is known before two libraries are compared.

    python tests/perf/bounded_mem_bench.py [--log2-bases 25] [--queries 1000000] [--baseline DIR]

--baseline DIR: a directory that holds the gcsa2_amd package (with its built library) of the commit to compare against; its
unbounded calls are timed on the same box and the same batch, in processes that alternate with this tree's.  Without it
only this tree is measured.  Prints a markdown report.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIN_LENGTH, HIT_MAX, SAMPLE = 20, 64, 1
NEVER = 0xFFFFFFFF          # a cap the kernel tests in every round and no pattern reaches


def the_index(args):
    from workload import graphs, builder, cache
    g = graphs.snp_graph(1 << args.log2_bases, 0x6C5A0010, 0x6C5A0011)
    path = os.path.join(args.cache_dir, f"snp_{args.log2_bases}_{args.order}_mem.npz")
    if os.path.exists(path):
        return g, cache.load(path)
    ix = builder.build(g, args.order, keep_table=False)
    os.makedirs(args.cache_dir, exist_ok=True)
    cache.save(path + ".tmp.npz", ix)
    os.replace(path + ".tmp.npz", path)
    return g, ix


def the_batch(args, g):
    from workload import patterns
    nq, m = args.queries, args.length
    path = os.path.join(args.cache_dir, f"snp_{args.log2_bases}_batch_{nq}_{m}.npy")      # (every process takes the same batch)
    if os.path.exists(path):
        pats = np.load(path)
    else:
        pats = patterns.walk_patterns(g, nq, m, 0x6C5A0050)
        sub = np.frombuffer(b"ACGT", dtype=np.uint8)
        for col in range(37, m, 41):               # config 5: a substitution every 41 bp in every second pattern
            pats[1::2, col] = sub[(np.searchsorted(sub, pats[1::2, col]) + 1) % 4]
        os.makedirs(args.cache_dir, exist_ok=True)
        np.save(path + ".tmp.npy", pats)
        os.replace(path + ".tmp.npy", path)
    return patterns.as_batch(pats)


def measure(args):
    """One process, one library: a JSON line {name: {"medians_ms": [...], ...}}."""
    sys.path.insert(0, ROOT)
    if args.package:
        sys.path.insert(0, args.package)
    import torch
    from gcsa2_amd.binding import GCSA, Gcsa2Error
    g, ix = the_index(args)
    flat, off = the_batch(args, g)
    nq, total = args.queries, int(off[-1])
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    gpu = GCSA(ix)
    bounded = not args.package                  # the baseline has no bounded calls
    d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_boff = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    d_rng = torch.zeros((nq, 2), dtype=torch.int64, device=dev)
    d_fb = torch.zeros(nq, dtype=torch.int64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def medians(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeats):
            times = []
            for _ in range(args.calls):
                e0.record(stream)
                fn()
                e1.record(stream)
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            out.append(float(np.median(times)))
        return out

    def breaks(cap):
        kw = {"max_length": cap} if bounded else {}
        try:
            need = gpu.match_breaks_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, d_boff.data_ptr(), 0, 0, stream=st, min_length=MIN_LENGTH, **kw)
        except Gcsa2Error as e:
            need = e.needed
        d_brk = torch.zeros((max(need, 1), 4), dtype=torch.int64, device=dev)
        ms = medians(lambda: gpu.match_breaks_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, d_boff.data_ptr(), d_brk.data_ptr(), need,
                                                     d_rng.data_ptr(), d_fb.data_ptr(), st, min_length=MIN_LENGTH, **kw))
        lengths = d_brk[:need, 1]
        return {"medians_ms": ms, "records": int(need), "records_per_pattern": need / nq, "longest": int(lengths.max().item()) if need else 0,
                "parent_calls_per_pattern": float(d_fb.double().mean().item())}

    def mem_hits(cap):
        kw = {"max_length": cap} if bounded else {}
        try:
            m, h = gpu.mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, MIN_LENGTH, HIT_MAX, SAMPLE, d_boff.data_ptr(), 0, 0,
                                       d_rng.data_ptr(), 0, 0, st, **kw)
        except Gcsa2Error as e:
            m, h = e.needed
        d_mems = torch.zeros((max(m, 1), 5), dtype=torch.int64, device=dev)
        d_hoff = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        d_hits = torch.zeros(max(h, 1), dtype=torch.int64, device=dev)
        ms = medians(lambda: gpu.mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, MIN_LENGTH, HIT_MAX, SAMPLE, d_boff.data_ptr(),
                                                 d_mems.data_ptr(), m, d_hoff.data_ptr(), d_hits.data_ptr(), h, st, **kw))
        return {"medians_ms": ms, "mems": int(m), "hits": int(h)}

    out = {"path_nodes": int(ix.n), "order": int(args.order), "kmer_k": gpu.kmer_table_k(), "breaks_uncapped": breaks(0), "mem_hits_uncapped": mem_hits(0)}
    if bounded:
        out["breaks_cap_never"] = breaks(NEVER)
        out["breaks_cap_order"] = breaks(args.order)
        out["mem_hits_cap_never"] = mem_hits(NEVER)
        out["mem_hits_cap_order"] = mem_hits(args.order)
    gpu.close()
    print("RESULT " + json.dumps(out), flush=True)


def spread(values):
    return (max(values) - min(values)) / min(values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-bases", type=int, default=25)
    ap.add_argument("--order", type=int, default=32)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=256)
    ap.add_argument("--calls", type=int, default=7, help="calls per median (at least 7)")
    ap.add_argument("--repeats", type=int, default=3, help="medians per process")
    ap.add_argument("--rounds", type=int, default=2, help="processes per library, alternating")
    ap.add_argument("--baseline", default="", help="directory with the gcsa2_amd package of the commit to compare against")
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds a measuring process may take")
    ap.add_argument("--measure", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--package", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.calls >= 7
    if args.measure:
        return measure(args)

    def child(package):
        cmd = [sys.executable, os.path.abspath(__file__), "--measure", "--log2-bases", str(args.log2_bases), "--order", str(args.order),
               "--queries", str(args.queries), "--length", str(args.length), "--calls", str(args.calls), "--repeats", str(args.repeats),
               "--cache-dir", args.cache_dir] + (["--package", package] if package else [])
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        if done.returncode != 0:                 # (a process that failed ends the run: nothing more is started on the device)
            sys.stderr.write(done.stdout + done.stderr)
            sys.exit(done.returncode if done.returncode > 0 else 1)
        return json.loads([line for line in done.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])

    runs = {"baseline": [], "this": []}
    for _ in range(args.rounds):
        if args.baseline:
            runs["baseline"].append(child(os.path.abspath(args.baseline)))
        runs["this"].append(child(""))
    first = runs["this"][0]
    nq = args.queries
    print(f"snp graph of 2^{args.log2_bases} bases, order {first['order']}, {first['path_nodes']} path nodes, k-mer seeds of {first['kmer_k']}; "
          f"{nq} x {args.length} bp, every second pattern with a substitution every 41 bp; min_length {MIN_LENGTH}, hit_max {HIT_MAX} (SAMPLE).  "
          f"Each median is of {args.calls} calls; {args.repeats} medians per process, {args.rounds} processes per library, alternating.\n")

    def pool(which, name):
        return [v for r in runs[which] for v in r[name]["medians_ms"]]

    print("| call | library | medians ms | median of medians ms | spread (max - min) / min |")
    print("|---|---|---|---|---|")
    for name in ("breaks_uncapped", "mem_hits_uncapped"):
        for which in ("baseline", "this"):
            if runs[which]:
                v = pool(which, name)
                print(f"| {name} | {which} | {' '.join(f'{x:.3f}' for x in v)} | {np.median(v):.3f} | {spread(v):.2%} |")
    if runs["baseline"]:
        print()
        for name in ("breaks_uncapped", "mem_hits_uncapped"):
            a, b = pool("baseline", name), pool("this", name)
            print(f"{name}: this / baseline = {np.median(b) / np.median(a):.4f}; the baseline's own spread is {spread(a):.2%}")
    print("\n| call | max_length | median of medians ms | patterns/s | records (MEMs) per pattern | longest | parent() calls per pattern | against the unbounded call |")
    print("|---|---|---|---|---|---|---|---|")
    for kind in ("breaks", "mem_hits"):
        base = float(np.median(pool("this", kind + "_uncapped")))
        for cap, label in (("uncapped", "0"), ("cap_never", str(NEVER)), ("cap_order", str(first["order"]))):
            r = first[f"{kind}_{cap}"]
            t = float(np.median(pool("this", f"{kind}_{cap}")))
            count = r.get("records", r.get("mems"))
            print(f"| {kind} | {label} | {t:.3f} | {nq / (t * 1e-3):.4g} | {count / nq:.3f} | {r.get('longest', '-')} | "
                  f"{r.get('parent_calls_per_pattern', float('nan')):.2f} | {t / base:.4f} |")


if __name__ == "__main__":
    main()
