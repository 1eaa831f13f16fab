#!/usr/bin/env python3
"""Batched k-mer windows (gcsa2_kmer_windows_device / _batch) on the snp graph against the routes the library offered for the
same answers before it.  `--reads` walks of `--read-length` bases, every window of `--k` characters at `--stride`.

Device rows (device events around each call sequence, warm-up runs first, median and min-max of `--reps` timed runs, the two
sides alternating):
  ranges only          kmer_windows_device   |  extend_device from the root over one prebuilt state per window
  profiles only        kmer_windows_device   |  the same extend call + a per-read reduction in torch
  profiles and counts  kmer_windows_device   |  that + count_device on the ranges + its per-read sum
Host row (wall clock around the blocking calls, pageable numpy arrays, same repetitions):
  profiles only        kmer_windows_batch    |  find_batch on the materialised windows
The results of both sides must be the same.

    python tests/perf/kmer_windows_bench.py [--log2-bases 22] [--order 32] [--reads 1000000] [--read-length 150] [--k 32] [--stride 1]
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
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-host", action="store_true", help="skip the host row (it materialises every window in host memory)")
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    args = ap.parse_args()
    import torch
    from workload import graphs, builder, patterns, cache
    from gcsa2_amd.binding import GCSA, KMER_COUNTS
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
    nr, L, k, stride = args.reads, args.read_length, args.k, args.stride
    per = (L - k) // stride + 1
    nw = nr * per
    reads = patterns.walk_patterns(g, nr, L, 0x6C5A0080)                          # (nr, L) bytes
    flat, off = patterns.as_batch(reads)
    d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(8, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    print(f"{nr} reads of {L} bases, k = {k}, stride {stride}: {nw} windows", flush=True)
    # the new call's outputs
    d_rng = torch.zeros((nw, 2), dtype=torch.int64, device=dev)
    d_prof = torch.zeros((nr, 4), dtype=torch.int64, device=dev)
    # the baseline's: one search state per window, from the root (built here, not timed)
    w = torch.arange(nw, dtype=torch.int64, device=dev)
    d_states = torch.empty((nw, 5), dtype=torch.int64, device=dev)
    d_states[:, 0] = w // per
    d_states[:, 1] = (w % per) * stride
    d_states[:, 2] = d_states[:, 1] + k
    d_states[:, 3] = 0
    d_states[:, 4] = ix.n - 1
    del w
    d_out = torch.empty((nw, 5), dtype=torch.int64, device=dev)
    d_pairs = torch.empty((nw, 2), dtype=torch.int64, device=dev)
    d_cnt = torch.empty(nw, dtype=torch.int64, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def windows(flags, profiles, ranges):
        gpu.kmer_windows_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, stride, flags, 0, d_prof.data_ptr() if profiles else 0,
                                d_rng.data_ptr() if ranges else 0, 0, nw, st)

    def extend():
        gpu.extend_device(d_pat.data_ptr(), d_off.data_ptr(), nr, d_states.data_ptr(), nw, d_out.data_ptr(), st)

    def reduce(counts):
        """The baseline's profiles from the extensions: (found, nodes[, occurrences]) per read."""
        sp, ep = d_out[:, 1], d_out[:, 2]
        nonempty = sp <= ep                                                       # both below 2^63; an empty range has sp = ep + 1
        found = nonempty.view(nr, per).sum(1)
        nodes = torch.where(nonempty, ep + 1 - sp, torch.zeros_like(sp)).view(nr, per).sum(1)
        if not counts:
            return found, nodes, None
        d_pairs.copy_(d_out[:, 1:3])
        gpu.count_device(d_pairs.data_ptr(), nw, d_cnt.data_ptr(), st)
        return found, nodes, d_cnt.view(nr, per).sum(1)

    rows = (("ranges only", lambda: windows(0, False, True), extend),
            ("profiles only", lambda: windows(0, True, False), lambda: (extend(), reduce(False))),
            ("profiles and counts", lambda: windows(KMER_COUNTS, True, False), lambda: (extend(), reduce(True))))
    print("| device | windows | kmer_windows_device | baseline | baseline / new | new within the baseline's spread | G windows/s |")
    print("|---|---|---|---|---|---|---|")
    ok = True
    for name, new, base in rows:
        for _ in range(args.warmup):
            new(), base()
        torch.cuda.synchronize()
        t_new, t_base = [], []
        for _ in range(args.reps):                                                # the sides alternate
            t_new.append(timed(new))
            t_base.append(timed(base))
        a, b = statistics.median(t_new), statistics.median(t_base)
        spread = max(t_base) - min(t_base)
        print(f"| {name} | {nw} | {a:.3f} ms ({min(t_new):.3f}-{max(t_new):.3f}) | {b:.3f} ms ({min(t_base):.3f}-{max(t_base):.3f}) | "
              f"{b / a:.2f}x | {'yes' if a <= b + spread else 'NO'} (spread {spread:.3f} ms) | {nw / a / 1e6:.2f} |", flush=True)
    # the same answers on both sides
    windows(KMER_COUNTS, True, True)
    extend()
    found, nodes, occ = reduce(True)
    torch.cuda.synchronize()
    same_ranges = bool((d_rng == d_out[:, 1:3]).all())
    prof = d_prof.cpu().numpy().view(np.uint64)
    same_prof = (bool((prof[:, 0] == per).all()) and np.array_equal(prof[:, 1], found.cpu().numpy().astype(np.uint64)) and
                 np.array_equal(prof[:, 2], nodes.cpu().numpy().astype(np.uint64)) and np.array_equal(prof[:, 3], occ.cpu().numpy().astype(np.uint64)))
    print(f"same ranges: {same_ranges}; same profiles: {same_prof}; found {int(prof[:, 1].sum())} of {nw}", flush=True)
    ok = ok and same_ranges and same_prof
    del d_states, d_out, d_pairs, d_cnt
    if not args.no_host:
        view = np.lib.stride_tricks.sliding_window_view(reads, k, axis=1)[:, ::stride, :]
        wins = np.ascontiguousarray(view).reshape(nw, k)
        wflat, woff = patterns.as_batch(wins)
        del wins
        t_new, t_base = [], []
        for r in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            _, hprof, _, _ = gpu.kmer_windows_batch(flat, off, k, stride, ranges=False)
            t1 = time.perf_counter()
            hrng = gpu.find_batch(wflat, woff)
            t2 = time.perf_counter()
            if r >= args.warmup:
                t_new.append((t1 - t0) * 1e3)
                t_base.append((t2 - t1) * 1e3)
        a, b = statistics.median(t_new), statistics.median(t_base)
        gap = b - a
        clear = min(t_base) > max(t_new)
        same = np.array_equal(hprof, np.concatenate([prof[:, :3], np.zeros((nr, 1), dtype=np.uint64)], axis=1)) and \
            np.array_equal(hrng, d_rng.cpu().numpy().view(np.uint64))
        ok = ok and same
        print("| host, pageable | windows | kmer_windows_batch (profiles) | find_batch (materialised windows) | baseline / new | faster by more than either spread | G windows/s | same |")
        print("|---|---|---|---|---|---|---|---|")
        print(f"| profiles only | {nw} | {a:.1f} ms ({min(t_new):.1f}-{max(t_new):.1f}) | {b:.1f} ms ({min(t_base):.1f}-{max(t_base):.1f}) | {b / a:.2f}x | "
              f"{'yes' if clear and gap > max(max(t_new) - min(t_new), max(t_base) - min(t_base)) else 'NO'} | {nw / a / 1e6:.2f} | {'yes' if same else 'NO'} |", flush=True)
    gpu.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
