#!/usr/bin/env python3
"""Batched capped seeds (gcsa2_capped_seeds_device) on the snp graph beside the only route a caller had to the ranges and counts
on the way before it: one gcsa2_lf_device plus one gcsa2_count_device per character over the same reads.  `--reads` walks of
`--read-length` bases, once as drawn and once with a substitution about every `--period` bases.

The per-character loop is a floor of that route, not an implementation of the walk: it takes exactly read-length rounds (the
walk takes up to twice as many LF steps per read), its characters are laid out beforehand as one contiguous row of components
per round (not timed), a torch `where` puts every emptied range back to the root and nothing selects, emits or restarts.  It
evaluates count() in every round, the walk only once a match has min_length characters.

Rows: (min_length, max_length, max_count) in --params, both batches, hit_max 0.  Device events around each side's whole call
sequence, warm-up runs first, then the median and min-max of `--reps` timed runs, the two sides alternating.  The new call runs
on buffers of the exact sizes (found out beforehand, not timed).

    python tests/perf/capped_seeds_bench.py [--log2-bases 22] [--order 32] [--reads 1000000] [--read-length 150]
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

from kmer_hits_bench import substitute  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-bases", type=int, default=22)
    ap.add_argument("--order", type=int, default=32)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--params", type=int, nargs="+", default=[16, 32, 1, 12, 0, 1, 8, 0, 4], help="triples min_length max_length max_count")
    ap.add_argument("--period", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    args = ap.parse_args()
    assert len(args.params) % 3 == 0
    import torch
    from workload import graphs, builder, patterns, cache
    from gcsa2_amd.binding import GCSA, Gcsa2Error, STATUS_BUFFER_TOO_SMALL
    g = graphs.snp_graph(1 << args.log2_bases, 0x6C5A0010, 0x6C5A0011)
    path = os.path.join(args.cache_dir, f"snp_{args.log2_bases}_{args.order}_extend.npz")
    t0 = time.perf_counter()
    if os.path.exists(path):
        ix = cache.load(path)
    else:
        ix = builder.build(g, args.order, keep_table=False)
        os.makedirs(args.cache_dir, exist_ok=True)
        cache.save(path, ix)
    print(f"index: 2^{args.log2_bases} bases, order {args.order}, {ix.n} path nodes ({time.perf_counter() - t0:.1f} s)", flush=True)
    gpu = GCSA(ix)
    print(f"image {gpu.device_bytes()} B, pair blocks {gpu.pair_block_bytes()} B, seed table k = {gpu.kmer_table_k()}", flush=True)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    nr, L = args.reads, args.read_length
    drawn = patterns.walk_patterns(g, nr, L, 0x6C5A0080)                          # (nr, L) bytes
    batches = (("as drawn", drawn), (f"substituted every {args.period}", substitute(drawn, args.period, 0x6C5A0081)))
    char2comp = np.asarray(ix.char2comp, dtype=np.uint8)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), out

    print("| min_length, max_length, max_count | batch | seeds | hits | capped_seeds_device | M reads/s | M seeds/s | lf + count per character | "
          "M reads/s | loop / new |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name, reads in batches:
        flat, off = patterns.as_batch(reads)
        d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(8, dtype=np.uint8)])).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_soff = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
        # round j of the loop steps with character L - 1 - j of every read: one contiguous row of components per round
        d_comps = torch.from_numpy(np.ascontiguousarray(char2comp[np.asarray(reads).reshape(nr, L)][:, ::-1].T)).to(dev)
        root = torch.tensor([0, ix.n - 1], dtype=torch.int64, device=dev).repeat(nr, 1)
        d_a, d_b = root.clone(), root.clone()
        d_cnt = torch.zeros(nr, dtype=torch.int64, device=dev)

        def loop():
            d_a.copy_(root)
            for j in range(L):
                gpu.lf_device(d_a.data_ptr(), d_comps[j].data_ptr(), nr, d_b.data_ptr(), st)
                gpu.count_device(d_b.data_ptr(), nr, d_cnt.data_ptr(), st)
                torch.where((d_b[:, 0] > d_b[:, 1]).unsqueeze(1), root, d_b, out=d_a)      # an empty range has sp = ep + 1
            return None

        for t in range(0, len(args.params), 3):
            params = tuple(args.params[t:t + 3])
            try:                                                                  # the sizes, from a refusal (not timed)
                m, h = gpu.capped_seeds_device(d_pat.data_ptr(), d_off.data_ptr(), nr, *params, 0, False, d_soff.data_ptr(), 0, 0,
                                               d_soff.data_ptr(), 0, 0, st)
            except Gcsa2Error as e:                                               # BUFFER_TOO_SMALL carries the sizes
                if e.code != STATUS_BUFFER_TOO_SMALL:
                    raise
                m, h = e.needed
            d_seeds = torch.zeros((max(m, 1), 5), dtype=torch.int64, device=dev)
            d_hoff = torch.zeros(m + 1, dtype=torch.int64, device=dev)
            d_hits = torch.zeros(max(h, 1), dtype=torch.int64, device=dev)

            def new():
                return gpu.capped_seeds_device(d_pat.data_ptr(), d_off.data_ptr(), nr, *params, 0, False, d_soff.data_ptr(), d_seeds.data_ptr(), m,
                                               d_hoff.data_ptr(), d_hits.data_ptr(), h, st)

            for _ in range(args.warmup):
                new(), loop()
            torch.cuda.synchronize()
            t_new, t_old = [], []
            for _ in range(args.reps):                                            # the sides alternate
                t_new.append(timed(new)[0])
                t_old.append(timed(loop)[0])
            a, b = statistics.median(t_new), statistics.median(t_old)
            print(f"| {params[0]}, {params[1]}, {params[2]} | {name} | {m} | {h} | {a:.3f} ms ({min(t_new):.3f}-{max(t_new):.3f}) | {nr / a / 1e3:.2f} | "
                  f"{m / a / 1e3:.2f} | {b:.3f} ms ({min(t_old):.3f}-{max(t_old):.3f}) | {nr / b / 1e3:.2f} | {b / a:.2f}x |", flush=True)
            del d_seeds, d_hoff, d_hits
            torch.cuda.empty_cache()
        del d_pat, d_off, d_soff, d_comps, d_a, d_b, d_cnt, root
    gpu.close()


if __name__ == "__main__":
    main()
