#!/usr/bin/env python3
"""Batched k-mer support (gcsa2_kmer_support_device) on the repeat graph against the composition that gave the same array
before it: gcsa2_kmer_hits_device (SKIP, the same hit_max) and torch.Tensor.index_add_ on the device over hits >> shift.
`--reads` walks of `--read-length` bases, every window of k characters at stride 1, drawn twice: as independent walks over the
whole graph, and as walks whose starts lie in a region that the reads cover `--depth` times (sequencing-depth duplication).

Rows: k in --k, both batches.  Device events around each side's whole call sequence, warm-up runs first, then `--reps` timed
runs, the two sides alternating; both sides must give the same array.  Per row also the number of 64-bit atomic adds that
k_support_add issues (one per run of equal bins in a wavefront, worked out here from gcsa2_locate_into of the distinct ranges),
and with --sweep the time of the new call for every GCSA2_SUPPORT_CHUNK in the list.  --only-new runs the new call alone, a
few times, for a kernel trace.

    python tests/perf/kmer_support_bench.py [--log2-bases 23] [--order 32] [--reads 1000000] [--read-length 150] [--k 16 32]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def walks(graph, nq, m, seed, first, span):
    """(nq, m) bytes: walks that start uniformly in backbone positions [first, first + span), successors chosen uniformly
    (workload.patterns.walk_patterns with a start region)."""
    rng = np.random.default_rng(seed)
    cur = rng.integers(first, first + span, nq, dtype=np.int64)
    out = np.empty((nq, m), dtype=np.uint8)
    soff, succ, comp = graph.succ_off.astype(np.int64), graph.succ, graph.comp
    c2b = np.frombuffer(b"$ACGTN#", dtype=np.uint8)
    for i in range(m):
        out[:, i] = c2b[comp[cur]]
        begin = soff[cur]
        cur = succ[begin + rng.integers(0, 1 << 30, nq, dtype=np.int64) % (soff[cur + 1] - begin)].astype(np.int64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-bases", type=int, default=23)
    ap.add_argument("--order", type=int, default=32)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--hit-max", type=int, default=64)
    ap.add_argument("--shift", type=int, default=11)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep", type=int, nargs="*", default=[], help="log2 of the GCSA2_SUPPORT_CHUNK budgets to time the new call with")
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    args = ap.parse_args()
    import torch
    from workload import graphs, builder, patterns, cache
    from gcsa2_amd.binding import GCSA, Gcsa2Error, STATUS_BUFFER_TOO_SMALL
    g = graphs.repeat_graph(1 << args.log2_bases, 0x6C5A0010, 0x6C5A0011)
    path = os.path.join(args.cache_dir, f"repeat_{args.log2_bases}_{args.order}_support.npz")
    t0 = time.perf_counter()
    if os.path.exists(path):
        ix = cache.load(path)
    else:
        ix = builder.build(g, args.order, keep_table=False)
        os.makedirs(args.cache_dir, exist_ok=True)
        cache.save(path, ix)
    print(f"index: 2^{args.log2_bases} bases, order {args.order}, {ix.n} path nodes ({time.perf_counter() - t0:.1f} s)", flush=True)
    gpu = GCSA(ix)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    nr, L, hit_max, shift = args.reads, args.read_length, args.hit_max, args.shift
    backbone = g.sink - 1
    whole = max(1, backbone - L - 1)
    region = min(whole, nr * L // args.depth)
    batches = (("independent walks", walks(g, nr, L, 0x6C5A0090, 1, whole)),
               (f"{args.depth}x over {region} bases", walks(g, nr, L, 0x6C5A0091, 1 + (whole - region) // 2, region)))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), out

    print("| k | batch | windows | found | counted | distinct | counted / distinct | values | added | kmer_support_device | composition | "
          "composition / new | atomics | same |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    ok = True
    for k in args.k:
        for name, reads in batches:
            flat, off = patterns.as_batch(reads)
            d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(8, dtype=np.uint8)])).to(dev)
            d_off = torch.from_numpy(off.view(np.int64)).to(dev)
            d_soff = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
            try:                                                                  # the sizes, from a refusal (not timed)
                m, h = gpu.kmer_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, False, 0, d_soff.data_ptr(), 0, 0,
                                            d_soff.data_ptr(), 0, 0, st)
            except Gcsa2Error as e:
                if e.code != STATUS_BUFFER_TOO_SMALL:
                    raise
                m, h = e.needed
            d_seeds = torch.zeros((max(m, 1), 5), dtype=torch.int64, device=dev)
            d_hoff = torch.zeros(m + 1, dtype=torch.int64, device=dev)
            d_hits = torch.zeros(max(h, 1), dtype=torch.int64, device=dev)
            gpu.kmer_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, False, 0, d_soff.data_ptr(), d_seeds.data_ptr(), m,
                                 d_hoff.data_ptr(), d_hits.data_ptr(), h, st)
            n_bins = int((d_hits[:h] >> shift).max()) + 1 if h else 1
            d_new = torch.zeros(n_bins, dtype=torch.int64, device=dev)
            d_old = torch.zeros(n_bins, dtype=torch.int64, device=dev)
            ones = torch.ones(max(h, 1), dtype=torch.int64, device=dev)

            def new():
                return gpu.kmer_support_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, shift, 0, d_new.data_ptr(), n_bins, st)

            def composition():
                gpu.kmer_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, False, 0, d_soff.data_ptr(), d_seeds.data_ptr(), m,
                                     d_hoff.data_ptr(), d_hits.data_ptr(), h, st)
                d_old.index_add_(0, d_hits[:h] >> shift, ones[:h])

            if args.only_new:
                for _ in range(args.warmup + args.reps):
                    stats = new()
                torch.cuda.synchronize()
                print(f"# {k} | {name}: {stats}", flush=True)
                continue
            for _ in range(args.warmup):
                new(), composition()
            torch.cuda.synchronize()
            t_new, t_old = [], []
            for _ in range(args.reps):                                            # the sides alternate
                t, stats = timed(new)
                t_new.append(t)
                t_old.append(timed(composition)[0])
            d_new.zero_(), d_old.zero_()
            new(), composition()
            torch.cuda.synchronize()
            same = bool((d_new == d_old).all()) and stats["dropped"] == 0
            ok = ok and same
            # the atomic adds of k_support_add: the distinct counted ranges in (sp, ep) order, their values, one add per run of
            # equal bins inside 64 consecutive values
            seeds = d_seeds[:m]
            counted = seeds[seeds[:, 4] <= hit_max][:, 2:4] if hit_max else seeds[:, 2:4]
            distinct = torch.unique(counted, dim=0).contiguous()
            d = int(distinct.shape[0])
            d_o = torch.zeros(d + 1, dtype=torch.int64, device=dev)
            d_v = torch.zeros(max(stats["values"], 1), dtype=torch.int64, device=dev)
            total = gpu.locate_into(distinct.data_ptr(), d, d_o.data_ptr(), d_v.data_ptr(), d_v.shape[0], st) if d else 0
            bins = d_v[:total] >> shift
            ends = torch.ones(total, dtype=torch.bool, device=dev)
            if total > 1:
                ends[:-1] = (bins[1:] != bins[:-1]) | (torch.arange(total - 1, device=dev) % 64 == 63)
            atomics = int(ends.sum())
            assert d == stats["distinct"] and total == stats["values"], (d, total, stats)
            a, b = statistics.median(t_new), statistics.median(t_old)
            print(f"| {k} | {name} | {stats['windows']} | {stats['found']} | {stats['counted']} | {d} | {stats['counted'] / max(d, 1):.2f} | {total} | "
                  f"{stats['added']} | {a:.3f} ms ({min(t_new):.3f}-{max(t_new):.3f}) | {b:.3f} ms ({min(t_old):.3f}-{max(t_old):.3f}) | {b / a:.2f}x | "
                  f"{atomics} | {'yes' if same else 'NO'} |", flush=True)
            for log2 in args.sweep:
                os.environ["GCSA2_SUPPORT_CHUNK"] = str(1 << log2)
                new()
                ts = [timed(new)[0] for _ in range(args.reps)]
                print(f"# chunk 2^{log2}: {statistics.median(ts):.3f} ms ({min(ts):.3f}-{max(ts):.3f})", flush=True)
            os.environ.pop("GCSA2_SUPPORT_CHUNK", None)
            del d_pat, d_off, d_soff, d_seeds, d_hoff, d_hits, d_new, d_old, ones, d_o, d_v, bins, ends, seeds, counted, distinct
            torch.cuda.empty_cache()
    gpu.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
