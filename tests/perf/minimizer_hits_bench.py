#!/usr/bin/env python3
"""Batched minimizer seeds (gcsa2_minimizer_hits_device) on the repeat graph against what a caller ran for the same seeds
before it: gcsa2_kmer_hits_device at stride 1 on the same batch, of whose seeds the minimizers are a subset.  Also the
selection alone (gcsa2_minimizers_device) and its share of the fused call, and the selected fraction next to 2 / (w + 1).
`--reads` walks of `--read-length` bases; rows: (k, w) in --kw, hit_max = --hit-max, SKIP.

Device events around each call, warm-up runs first, then the median and min-max of `--reps` timed runs, the three calls
alternating in the same process.  All run on buffers of the exact sizes (found out beforehand, not timed).  The seeds of the
new call must be the stride-1 call's seeds at the selected positions.

    python tests/perf/minimizer_hits_bench.py [--log2-bases 23] [--order 32] [--reads 1000000] [--read-length 150] [--kw 16,5 16,11 29,11]
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
    ap.add_argument("--log2-bases", type=int, default=23)
    ap.add_argument("--order", type=int, default=32)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--kw", nargs="+", default=["16,5", "16,11", "29,11"])
    ap.add_argument("--hit-max", type=int, default=64)
    ap.add_argument("--hash-seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
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
    print(f"image {gpu.device_bytes()} B, pair blocks {gpu.pair_block_bytes()} B, seed table k = {gpu.kmer_table_k()}", flush=True)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    nr, L, hit_max, seed = args.reads, args.read_length, args.hit_max, args.hash_seed
    reads = patterns.walk_patterns(g, nr, L, 0x6C5A0090)                          # (nr, L) bytes
    flat, off = patterns.as_batch(reads)
    d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(8, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_off2 = torch.zeros(nr + 1, dtype=torch.int64, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), out

    def sizes(call):
        try:
            return call()
        except Gcsa2Error as e:                                                   # BUFFER_TOO_SMALL carries the sizes
            if e.code != STATUS_BUFFER_TOO_SMALL:
                raise
            return e.needed

    def row(ts):
        return f"{statistics.median(ts):.3f} ms ({min(ts):.3f}-{max(ts):.3f})"

    print("| k | w | windows | minimizers | selected | 2 / (w + 1) | seeds | hits | minimizers_device | share of the fused call | minimizer_hits_device | "
          "stride-1 seeds | stride-1 hits | kmer_hits_device, stride 1 | stride 1 / new | new faster beyond both spreads | M minimizers/s | same |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    ok = True
    for kw in args.kw:
        k, w = (int(x) for x in kw.split(","))
        nw = nr * (L - k + 1)
        P, O = d_pat.data_ptr(), d_off.data_ptr()
        total = sizes(lambda: gpu.minimizers_device(P, O, nr, k, w, seed, d_off2.data_ptr(), 0, 0, st))
        m, h = sizes(lambda: gpu.minimizer_hits_device(P, O, nr, k, w, seed, hit_max, False, 0, d_off2.data_ptr(), 0, 0, d_off2.data_ptr(), 0, 0, st))
        m1, h1 = sizes(lambda: gpu.kmer_hits_device(P, O, nr, k, 1, hit_max, False, 0, d_off2.data_ptr(), 0, 0, d_off2.data_ptr(), 0, 0, st))
        d_moff = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
        d_mins = torch.zeros((max(total, 1), 2), dtype=torch.int64, device=dev)
        d_soff = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
        d_seeds = torch.zeros((max(m, 1), 5), dtype=torch.int64, device=dev)
        d_hoff = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        d_hits = torch.zeros(max(h, 1), dtype=torch.int64, device=dev)
        d_soff1 = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
        d_seeds1 = torch.zeros((max(m1, 1), 5), dtype=torch.int64, device=dev)
        d_hoff1 = torch.zeros(m1 + 1, dtype=torch.int64, device=dev)
        d_hits1 = torch.zeros(max(h1, 1), dtype=torch.int64, device=dev)

        def select():
            return gpu.minimizers_device(P, O, nr, k, w, seed, d_moff.data_ptr(), d_mins.data_ptr(), total, st)

        def new():
            return gpu.minimizer_hits_device(P, O, nr, k, w, seed, hit_max, False, 0, d_soff.data_ptr(), d_seeds.data_ptr(), m, d_hoff.data_ptr(),
                                             d_hits.data_ptr(), h, st)

        def old():
            return gpu.kmer_hits_device(P, O, nr, k, 1, hit_max, False, 0, d_soff1.data_ptr(), d_seeds1.data_ptr(), m1, d_hoff1.data_ptr(),
                                        d_hits1.data_ptr(), h1, st)

        for _ in range(args.warmup):
            select(), new(), old()
        torch.cuda.synchronize()
        t_sel, t_new, t_old = [], [], []
        for _ in range(args.reps):                                                # the calls alternate
            t_sel.append(timed(select)[0])
            t_new.append(timed(new)[0])
            t_old.append(timed(old)[0])
        torch.cuda.synchronize()
        # the new seeds are the stride-1 seeds at the selected positions: (read, position) keys, both lists in read order
        owner1 = torch.repeat_interleave(torch.arange(nr, device=dev), d_soff1[1:] - d_soff1[:-1])
        owner_m = torch.repeat_interleave(torch.arange(nr, device=dev), d_moff[1:] - d_moff[:-1])
        key1 = owner1 * L + d_seeds1[:m1, 0]
        key_m = owner_m * L + d_mins[:total, 0]
        keep = torch.isin(key1, key_m)
        same = int(keep.sum()) == m and bool((d_seeds1[:m1][keep] == d_seeds[:m]).all())
        ok = ok and same
        a, b, s = statistics.median(t_new), statistics.median(t_old), statistics.median(t_sel)
        clear = max(t_new) < min(t_old)
        print(f"| {k} | {w} | {nw} | {total} | {total / nw:.4f} | {2 / (w + 1):.4f} | {m} | {h} | {row(t_sel)} | {s / a:.1%} | {row(t_new)} | {m1} | {h1} | "
              f"{row(t_old)} | {b / a:.2f}x | {'yes' if clear else 'NO'} | {total / s / 1e3:.1f} | {'yes' if same else 'NO'} |", flush=True)
        del d_moff, d_mins, d_soff, d_seeds, d_hoff, d_hits, d_soff1, d_seeds1, d_hoff1, d_hits1
        torch.cuda.empty_cache()
    gpu.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
