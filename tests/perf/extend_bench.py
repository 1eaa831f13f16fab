#!/usr/bin/env python3
"""Batched extend (gcsa2_extend_device) on the snp graph against what the library offered for the same job before it: a loop
of one gcsa2_lf_device call per character over the same states.  States of `--length` characters each, starting at find() of
the `--seed-length`-mer to their right, then the same windows from the root; gcsa2_find_device on the windows for comparison.
Device events around each call sequence, warm-up runs first, the median of `--reps` timed runs; the two sides alternate.
The ranges of both sides must be the same.

    python tests/perf/extend_bench.py [--log2-bases 22] [--order 32] [--states 1000000] [--length 32] [--seed-length 16]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-bases", type=int, default=22)
    ap.add_argument("--order", type=int, default=32)
    ap.add_argument("--states", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--seed-length", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    args = ap.parse_args()
    import torch
    from workload import graphs, builder, patterns, cache
    from gcsa2_amd.binding import GCSA
    g = graphs.snp_graph(1 << args.log2_bases, 0x6C5A0010, 0x6C5A0011)
    path = os.path.join(args.cache_dir, f"snp_{args.log2_bases}_{args.order}_extend.npz")
    t0 = time.perf_counter()
    if os.path.exists(path):
        ix = cache.load(path)
    else:
        ix = builder.build(g, args.order, keep_table=False)
        os.makedirs(args.cache_dir, exist_ok=True)
        cache.save(path, ix)
    print(f"index: 2^{args.log2_bases} bases, order {args.order}, {ix.n} path nodes ({time.perf_counter() - t0:.1f} s)")
    gpu = GCSA(ix)
    print(f"pair blocks {gpu.pair_block_bytes()} B, seed table k = {gpu.kmer_table_k()}")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    ns, L, S = args.states, args.length, args.seed_length
    reads = patterns.walk_patterns(g, ns, L + S, 0x6C5A0070)                      # (ns, L + S) bytes: window | seed
    flat, off = patterns.as_batch(reads)
    d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(8, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    seeds = gpu.find_batch(*patterns.as_batch(np.ascontiguousarray(reads[:, L:])))
    root = np.tile(np.array([0, ix.n - 1], dtype=np.uint64), (ns, 1))
    # the loop's input: the comp of every step, step t consumes character L - 1 - t of the window
    comps = np.ascontiguousarray(np.asarray(ix.char2comp, dtype=np.uint8)[reads[:, :L]][:, ::-1].T)      # (L, ns)
    d_comps = torch.from_numpy(comps).to(dev)
    d_ping = torch.zeros((ns, 2), dtype=torch.int64, device=dev)
    d_pong = torch.zeros((ns, 2), dtype=torch.int64, device=dev)
    d_states = torch.zeros((ns, 5), dtype=torch.int64, device=dev)
    d_out = torch.zeros((ns, 5), dtype=torch.int64, device=dev)
    # the windows as patterns of their own, for find()
    wflat, woff = patterns.as_batch(np.ascontiguousarray(reads[:, :L]))
    d_wpat = torch.from_numpy(np.concatenate([wflat, np.zeros(8, dtype=np.uint8)])).to(dev)
    d_woff = torch.from_numpy(woff.view(np.int64)).to(dev)
    d_found = torch.zeros((ns, 2), dtype=torch.int64, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    print("| start | states | characters | extend | lf_device loop | loop / extend | find_device (windows) | same ranges |")
    print("|---|---|---|---|---|---|---|---|")
    ok = True
    for name, start in (("find() of the seed", seeds), ("root", root)):
        states = np.zeros((ns, 5), dtype=np.uint64)
        states[:, 0] = np.arange(ns, dtype=np.uint64)
        states[:, 2] = L
        states[:, 3:] = start
        d_states.copy_(torch.from_numpy(states.view(np.int64)))
        d_start = torch.from_numpy(np.ascontiguousarray(start).view(np.int64)).to(dev)

        def extend():
            gpu.extend_device(d_pat.data_ptr(), d_off.data_ptr(), ns, d_states.data_ptr(), ns, d_out.data_ptr(), st)

        def loop():
            src, dst = d_start, d_ping
            for t in range(L):
                gpu.lf_device(src.data_ptr(), d_comps[t].data_ptr(), ns, dst.data_ptr(), st)
                src, dst = dst, (d_pong if dst is d_ping else d_ping)
            return src

        def find():
            gpu.find_device(d_wpat.data_ptr(), d_woff.data_ptr(), ns, d_found.data_ptr(), st)

        for _ in range(args.warmup):
            extend(), loop(), find()
        torch.cuda.synchronize()
        t_ext, t_loop, t_find = [], [], []
        for _ in range(args.reps):                                                 # the sides alternate
            t_ext.append(timed(extend))
            t_loop.append(timed(loop))
            t_find.append(timed(find))
        last = loop()
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(np.uint64)
        looped = last.cpu().numpy().view(np.uint64)
        live = int((got[:, 0] == L).sum())
        same = np.array_equal(got[:, 1:3], looped) and live == ns                  # walks of the graph: every step stays non-empty
        if name == "root":
            same = same and np.array_equal(got[:, 1:3], d_found.cpu().numpy().view(np.uint64))
        ok = ok and same
        e, l, f = statistics.median(t_ext), statistics.median(t_loop), statistics.median(t_find)
        print(f"| {name} | {ns} | {L} | {e:.3f} ms ({min(t_ext):.3f}-{max(t_ext):.3f}) | {l:.3f} ms ({min(t_loop):.3f}-{max(t_loop):.3f}) | "
              f"{l / e:.2f}x | {f:.3f} ms | {'yes' if same else 'NO'} ({live} ran through) |", flush=True)
    gpu.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
