#!/usr/bin/env python3
"""Batched k-mer classes (gcsa2_kmer_classes_device) on the repeat graph against the composition that a caller had before it,
in the same process: gcsa2_kmer_hits_device (SKIP, the same hit_max, buffers of the exact sizes), then torch on the device --
class_of_bin[hits >> shift], the (window, class) pairs made unique for PER_WINDOW, index_add_ into the reads x classes matrix
and the row maximum for the calls.  The setup is that of tests/perf/kmer_support_bench.py: `--reads` walks of `--read-length`
bases, every window of k characters at stride 1, drawn twice -- independent walks over the whole graph, and walks whose starts
lie in a region that the reads cover `--depth` times.

Rows: k in --k, both batches, the maps of --maps (`blocked25`: 25 classes blocked over the node ids; `interleaved1024`: 1024
classes, bin % 1024), with and without PER_WINDOW.  Both sides must give the same matrix and the same best class first.  Then
device events around each side's whole call sequence, warm-up runs, `--reps` timed runs, the two sides alternating; and the
new call again without the matrix (d_votes = NULL: 48 bytes per read leave the device).  --only-new runs the new call alone, a
few times per row, for a kernel trace.

    python tests/perf/kmer_classes_bench.py [--log2-bases 23] [--order 32] [--reads 1000000] [--read-length 150] [--k 16 32]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kmer_support_bench import walks      # noqa: E402

PER_WINDOW = 1


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
    ap.add_argument("--maps", nargs="+", default=["blocked25", "interleaved1024"])
    ap.add_argument("--flags", type=int, nargs="+", default=[0, PER_WINDOW])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
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

    def spread(ts):
        return f"{statistics.median(ts):.3f} ms ({min(ts):.3f}-{max(ts):.3f})"

    print("| k | batch | map | flags | counted | distinct | values | votes | ambiguous | kmer_classes_device | composition | composition / new | "
          "calls only | same |")
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
            ones = torch.ones(max(h, 1), dtype=torch.int64, device=dev)
            read_ids = torch.arange(nr, dtype=torch.int64, device=dev)
            seed_ids = torch.arange(max(m, 1), dtype=torch.int64, device=dev)
            d_calls = torch.zeros((nr, 6), dtype=torch.int64, device=dev)
            for which in args.maps:
                bins = torch.arange(n_bins, dtype=torch.int64, device=dev)
                if which == "blocked25":
                    C, long_map = 25, bins * 25 // n_bins
                elif which == "interleaved1024":
                    C, long_map = 1024, bins % 1024
                else:
                    raise SystemExit(f"unknown map {which}")
                d_map = long_map.to(torch.int32)
                d_new = torch.zeros((nr, C), dtype=torch.int64, device=dev)
                d_old = torch.zeros((nr, C), dtype=torch.int64, device=dev)
                for flags in args.flags:
                    def new(votes=True):
                        return gpu.kmer_classes_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, shift, flags, d_map.data_ptr(), n_bins, C,
                                                       d_new.data_ptr() if votes else 0, d_calls.data_ptr(), st)

                    def composition():
                        gpu.kmer_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, False, 0, d_soff.data_ptr(), d_seeds.data_ptr(), m,
                                             d_hoff.data_ptr(), d_hits.data_ptr(), h, st)
                        d_old.zero_()
                        cls = long_map[d_hits[:h] >> shift]
                        seed_of_hit = torch.repeat_interleave(seed_ids[:m], d_hoff[1:m + 1] - d_hoff[:m], output_size=h)
                        read_of_seed = torch.repeat_interleave(read_ids, d_soff[1:] - d_soff[:-1], output_size=m)
                        if flags & PER_WINDOW:
                            pairs = torch.unique(seed_of_hit * C + cls)
                            where = read_of_seed[pairs // C] * C + pairs % C
                        else:
                            where = read_of_seed[seed_of_hit] * C + cls
                        d_old.view(-1).index_add_(0, where, ones[:where.shape[0]])
                        return d_old.max(dim=1)

                    if args.only_new:
                        for _ in range(args.warmup + args.reps):
                            stats = new()
                        torch.cuda.synchronize()
                        print(f"# {k} | {name} | {which} | {flags}: {stats}", flush=True)
                        continue
                    stats = new()
                    best_votes, best = composition()
                    torch.cuda.synchronize()
                    voted = best_votes > 0
                    # the same matrix; the call's best class holds the row maximum (the maximum's own index is any of a tie)
                    mine = d_old[voted].gather(1, d_calls[:, 0][voted].unsqueeze(1)).squeeze(1)
                    same = bool((d_new == d_old).all()) and bool((d_calls[:, 1] == best_votes).all()) and \
                        bool((mine == best_votes[voted]).all()) and bool((d_calls[:, 4] == d_old.sum(dim=1)).all())
                    del best, best_votes, voted, mine
                    ok = ok and same
                    for _ in range(args.warmup - 1):
                        new(), composition()
                    torch.cuda.synchronize()
                    t_new, t_old, t_calls = [], [], []
                    for _ in range(args.reps):                                            # the sides alternate
                        t_new.append(timed(new)[0])
                        t_old.append(timed(composition)[0])
                        t_calls.append(timed(lambda: new(False))[0])
                    a, b = statistics.median(t_new), statistics.median(t_old)
                    print(f"| {k} | {name} | {which} | {flags} | {stats['counted']} | {stats['distinct']} | {stats['values']} | {stats['votes']} | "
                          f"{stats['ambiguous']} | {spread(t_new)} | {spread(t_old)} | {b / a:.2f}x | {spread(t_calls)} | {'yes' if same else 'NO'} |", flush=True)
                del d_new, d_old, d_map, long_map, bins
                torch.cuda.empty_cache()
            del d_pat, d_off, d_soff, d_seeds, d_hoff, d_hits, ones, read_ids, seed_ids, d_calls
            torch.cuda.empty_cache()
    gpu.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
