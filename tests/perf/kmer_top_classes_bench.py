#!/usr/bin/env python3
"""Batched k-mer top classes (gcsa2_kmer_top_classes_device) on the repeat graph against the composition that a caller had
before it, in the same process: gcsa2_kmer_hits_device (SKIP, the same hit_max, buffers of the exact sizes), then torch on the
device -- class_of_bin[hits >> shift], the (read, class) keys made unique with their counts (the de-duplication and the
segmented sum in one sort), a second sort by (read, votes descending, class) and the first top_n of every read.  The setup is
that of tests/perf/kmer_classes_bench.py: `--reads` independent walks of `--read-length` bases over the whole graph, every
window of k characters at stride 1.

Rows: k in --k, the maps of --maps (`identity`: class = bin, n_classes = n_bins -- the node ids at shift 11; `blockedN`: N
classes blocked over the bins), top_n in --top.  Both sides must give the same top rows, and the new call's summaries the
composition's voted and total.  Then device events around each side's whole call sequence, warm-up runs and `--reps` timed
runs, the sides alternating; the new call again with d_top = NULL (24 bytes per read leave the device); for blocked maps of at
most 4096 classes gcsa2_kmer_classes_device with and without the dense matrix.  --slots times the new call again under each
GCSA2_TOP_SLOTS and prints the share of reads that vote for more classes than the table has slots (they need more than one
pass whatever the hash does; probe sequences cut at 16 add a few below that).  --only-new runs the new call alone, a few times
per row, for a kernel trace.

    python tests/perf/kmer_top_classes_bench.py [--log2-bases 23] [--order 32] [--reads 1000000] [--read-length 150] [--k 16 32]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-bases", type=int, default=23)
    ap.add_argument("--order", type=int, default=32)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--hit-max", type=int, default=64)
    ap.add_argument("--shift", type=int, default=11)
    ap.add_argument("--maps", nargs="+", default=["identity", "blocked25", "blocked4096", "blocked100000"])
    ap.add_argument("--top", type=int, nargs="+", default=[5, 64])
    ap.add_argument("--slots", type=int, nargs="*", default=[256, 512, 1024, 2048, 4096])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    args = ap.parse_args()
    import torch
    from workload import graphs, builder, patterns, cache
    from gcsa2_amd.binding import GCSA, Gcsa2Error, STATUS_BUFFER_TOO_SMALL, TOP_SLOTS_DEFAULT
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
    whole = max(1, g.sink - 1 - L - 1)
    reads = walks(g, nr, L, 0x6C5A0090, 1, whole)
    flat, off = patterns.as_batch(reads)
    d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(8, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    os.environ.pop("GCSA2_TOP_SLOTS", None)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), out

    def spread(ts):
        return f"{statistics.median(ts):.3f} ms ({min(ts):.3f}-{max(ts):.3f})"

    print("| k | map | classes | top_n | counted | distinct | values | votes | most voted | mean voted | kmer_top_classes_device | composition | "
          "composition / new | summaries only | kmer_classes_device | calls only | same |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    ok = True
    sweep = []
    for k in args.k:
        d_soff = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
        try:                                                                  # the sizes, from a refusal (not timed)
            m, h = gpu.kmer_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, False, 0, d_soff.data_ptr(), 0, 0, d_soff.data_ptr(), 0, 0, st)
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
        read_ids = torch.arange(nr, dtype=torch.int64, device=dev)
        seed_ids = torch.arange(max(m, 1), dtype=torch.int64, device=dev)
        d_sums = torch.zeros((nr, 3), dtype=torch.int64, device=dev)
        for which in args.maps:
            bins = torch.arange(n_bins, dtype=torch.int64, device=dev)
            if which == "identity":
                C, long_map = n_bins, bins
            elif which.startswith("blocked"):
                C = int(which[len("blocked"):])
                long_map = bins * C // n_bins
            else:
                raise SystemExit(f"unknown map {which}")
            assert C < (1 << 24) and nr < (1 << 24)
            d_map = long_map.to(torch.int32)
            for top_n in args.top:
                d_top = torch.zeros((nr, top_n, 2), dtype=torch.int64, device=dev)

                def new(rows=True):
                    return gpu.kmer_top_classes_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, shift, 0, d_map.data_ptr(), n_bins, C, top_n,
                                                       d_top.data_ptr() if rows else 0, d_sums.data_ptr(), st)

                def composition():
                    gpu.kmer_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, False, 0, d_soff.data_ptr(), d_seeds.data_ptr(), m,
                                         d_hoff.data_ptr(), d_hits.data_ptr(), h, st)
                    cls = long_map[d_hits[:h] >> shift]
                    seed_of_hit = torch.repeat_interleave(seed_ids[:m], d_hoff[1:m + 1] - d_hoff[:m], output_size=h)
                    read_of_seed = torch.repeat_interleave(read_ids, d_soff[1:] - d_soff[:-1], output_size=m)
                    pairs, votes = torch.unique(read_of_seed[seed_of_hit] * C + cls, return_counts=True)     # sorted: the segmented sum
                    rd, cl = pairs // C, pairs % C
                    voted = torch.bincount(rd, minlength=nr)
                    total = torch.zeros(nr, dtype=torch.int64, device=dev).index_add_(0, rd, votes)
                    key = (rd << 38) | (((1 << 14) - 1 - votes) << 24) | cl                                  # votes <= 135 windows x 64 hits
                    key = torch.sort(key).values
                    first = torch.cumsum(voted, 0) - voted
                    rd = key >> 38
                    rank = torch.arange(key.shape[0], dtype=torch.int64, device=dev) - first[rd]
                    keep = rank < top_n
                    out = torch.zeros((nr, top_n, 2), dtype=torch.int64, device=dev)
                    out[:, :, 0] = -1
                    out[rd[keep], rank[keep], 0] = key[keep] & ((1 << 24) - 1)
                    out[rd[keep], rank[keep], 1] = (1 << 14) - 1 - ((key[keep] >> 24) & ((1 << 14) - 1))
                    return out, voted, total

                if args.only_new:
                    for _ in range(args.warmup + 3):
                        stats = new()
                    torch.cuda.synchronize()
                    print(f"# {k} | {which} | {top_n}: {stats}", flush=True)
                    continue
                stats = new()
                want, voted, total = composition()
                torch.cuda.synchronize()
                same = bool((d_top == want).all()) and bool((d_sums[:, 0] == voted).all()) and bool((d_sums[:, 1] == total).all())
                most, mean = int(voted.max()), float(voted.double().mean())
                if top_n == args.top[0]:
                    sweep.append((k, which, C, top_n, d_map, n_bins, voted.clone()))
                del want, total
                ok = ok and same
                for _ in range(args.warmup - 1):
                    new(), composition()
                torch.cuda.synchronize()
                t_new, t_old, t_sums = [], [], []
                for _ in range(args.reps):                                            # the sides alternate
                    t_new.append(timed(new)[0])
                    t_old.append(timed(composition)[0])
                    t_sums.append(timed(lambda: new(False))[0])
                dense_with = dense_without = "-"
                if which != "identity" and C <= 4096 and top_n == args.top[0]:
                    d_votes = torch.empty((nr, C), dtype=torch.int64, device=dev)
                    d_calls = torch.zeros((nr, 6), dtype=torch.int64, device=dev)

                    def dense(matrix=True):
                        return gpu.kmer_classes_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, shift, 0, d_map.data_ptr(), n_bins, C,
                                                       d_votes.data_ptr() if matrix else 0, d_calls.data_ptr(), st)
                    dense(), dense(False)
                    torch.cuda.synchronize()
                    dense_with = spread([timed(dense)[0] for _ in range(args.reps)])
                    dense_without = spread([timed(lambda: dense(False))[0] for _ in range(args.reps)])
                    same = same and bool((d_calls[:, 0] == d_top[:, 0, 0]).all()) and bool((d_calls[:, 1] == d_top[:, 0, 1]).all())
                    ok = ok and same
                    del d_votes, d_calls
                    torch.cuda.empty_cache()
                a, b = statistics.median(t_new), statistics.median(t_old)
                print(f"| {k} | {which} | {C} | {top_n} | {stats['counted']} | {stats['distinct']} | {stats['values']} | {stats['votes']} | {most} | {mean:.1f} | "
                      f"{spread(t_new)} | {spread(t_old)} | {b / a:.2f}x | {spread(t_sums)} | {dense_with} | {dense_without} | {'yes' if same else 'NO'} |", flush=True)
                del d_top
                torch.cuda.empty_cache()
            del d_map, long_map, bins
        del d_soff, d_seeds, d_hoff, d_hits, read_ids, seed_ids
        torch.cuda.empty_cache()
    if args.slots and not args.only_new:
        print()
        print(f"GCSA2_TOP_SLOTS (default {TOP_SLOTS_DEFAULT}); per cell the call's time and the share of reads with voted > slots")
        print("| k | map | top_n | " + " | ".join(str(s) for s in args.slots) + " |")
        print("|---|---|---|" + "---|" * len(args.slots))
        for k, which, C, top_n, d_map, n_bins, voted in sweep:
            d_top = torch.zeros((nr, top_n, 2), dtype=torch.int64, device=dev)
            cells = []
            for slots in args.slots:
                os.environ["GCSA2_TOP_SLOTS"] = str(slots)

                def new():
                    return gpu.kmer_top_classes_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, shift, 0, d_map.data_ptr(), n_bins, C, top_n,
                                                       d_top.data_ptr(), 0, st)
                new()
                torch.cuda.synchronize()
                ts = [timed(new)[0] for _ in range(args.reps)]
                cells.append(f"{spread(ts)}, {100.0 * float((voted > slots).double().mean()):.3f} %")
            os.environ.pop("GCSA2_TOP_SLOTS", None)
            print(f"| {k} | {which} | {top_n} | " + " | ".join(cells) + " |", flush=True)
    gpu.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
