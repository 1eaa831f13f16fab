#!/usr/bin/env python3
"""Batched chain pairs on the repeat graph: `--reads` / 2 pairs of interleaved mates of `--read-length` bases -- mate 1 the first
bases of a walk of `--fragment` bases, mate 2 the reverse complement of its last ones, every second walk reverse-complemented
first --, (k, w) minimizers, hit_max = --hit-max (SKIP), a linear coordinate map at --shift (coord = bin << shift, so a
fragment spans 2^shift per node: the chain and pair parameters are as wide as that needs).  Device events around each side,
warm-up runs first, then `--reps` timed runs a side, the sides alternating in one process (profiles/jump_mid.md):

  1. gcsa2_minimizer_chain_pairs_device, chain rows written to the caller's buffer;
  2. the composition on the same buffers: gcsa2_stranded_minimizer_hits_device (exact sizes, found out beforehand),
     gcsa2_seed_chains_device over the 2 n groups, gcsa2_chain_pairs_device over the n / 2 pairs;
  3. gcsa2_chain_pairs_device alone on those chain rows (chain_top_n = --top), and on generated rows at every chain_top_n of
     --alone, next to the time its own bytes -- 4 x chain_top_n x 32 read and (top_n + 1) x 64 written per pair -- take at
     --bandwidth (the achievable HBM rate of an MI355X, 6.3 TB/s).

The fused call must return the stats of the composition.

    python tests/perf/chain_pairs_bench.py [--log2-bases 23] [--order 32] [--reads 1000000] [--read-length 150] [--kw 16,11]
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
    ap.add_argument("--fragment", type=int, default=400)
    ap.add_argument("--kw", default="16,11")
    ap.add_argument("--hit-max", type=int, default=64)
    ap.add_argument("--shift", type=int, default=11)
    ap.add_argument("--top", type=int, default=5)
    ap.add_argument("--pair-top", type=int, default=2)
    ap.add_argument("--alone", default="5,64")
    ap.add_argument("--bandwidth", type=float, default=6.3e12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    args = ap.parse_args()
    import torch
    from workload import graphs, builder, patterns, cache
    from gcsa2_amd.binding import GCSA, Gcsa2Error, STATUS_BUFFER_TOO_SMALL, STRAND_BOTH
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
    k, w = (int(x) for x in args.kw.split(","))
    nr, L, F, hit_max, shift, top_n, pair_top = args.reads - args.reads % 2, args.read_length, args.fragment, args.hit_max, args.shift, args.top, args.pair_top
    n_pairs = nr // 2
    walks = torch.from_numpy(patterns.walk_patterns(g, n_pairs, F, 0x6C5A00A0)).to(dev)          # (n_pairs, F) bytes
    # reverse complements through the index's char2comp and its inverse; a byte without a code stays as it is
    c2c = np.asarray(ix.char2comp, dtype=np.int64)
    first = {}
    for byte in range(256):
        first.setdefault(int(c2c[byte]), byte)
    table = np.arange(256, dtype=np.uint8)
    for byte in range(256):
        if 1 <= c2c[byte] <= 4:
            table[byte] = first[5 - int(c2c[byte])]
    d_table = torch.from_numpy(table).to(dev)
    rc = lambda t: d_table[t.long()].flip(1)
    walks[1::2] = rc(walks[1::2])
    mates = torch.stack([walks[:, :L], rc(walks[:, F - L:])], dim=1)                              # (n_pairs, 2, L): interleaved
    d_pat = torch.cat([mates.reshape(-1), torch.zeros(8, dtype=torch.uint8, device=dev)])
    d_off = torch.arange(nr + 1, dtype=torch.int64, device=dev) * L
    del walks, mates
    P, O = d_pat.data_ptr(), d_off.data_ptr()
    d_size = torch.zeros(2 * nr + 1, dtype=torch.int64, device=dev)
    S = d_size.data_ptr()
    try:
        m, h = gpu.stranded_minimizer_hits_device(P, O, nr, k, w, 0, STRAND_BOTH, hit_max, False, 0, S, 0, 0, S, 0, 0, st)
    except Gcsa2Error as e:                                                       # BUFFER_TOO_SMALL carries the sizes
        if e.code != STATUS_BUFFER_TOO_SMALL:
            raise
        m, h = e.needed
    d_soff = torch.zeros(2 * nr + 1, dtype=torch.int64, device=dev)
    d_seeds = torch.zeros((max(m, 1), 5), dtype=torch.int64, device=dev)
    d_hoff = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    d_hits = torch.zeros(max(h, 1), dtype=torch.int64, device=dev)

    def hits():
        return gpu.stranded_minimizer_hits_device(P, O, nr, k, w, 0, STRAND_BOTH, hit_max, False, 0, d_soff.data_ptr(), d_seeds.data_ptr(), m, d_hoff.data_ptr(),
                                                  d_hits.data_ptr(), h, st)

    hits()
    n_bins = int((d_hits[:h] >> shift).max()) + 1 if h else 1
    coord = torch.arange(n_bins, dtype=torch.int64, device=dev) << shift
    wide = (1 << 32) - 1
    chain = dict(band=(1 << 64) - 1, max_gap=wide, lookback=16, match=1, gap=0, min_score=0, top_n=top_n, member_cap=0)
    pair = dict(orientation=0, min_fragment=0, max_fragment=wide, mean_fragment=(F // 32) << shift, unit=1 << shift, cost=1, min_score=0, top_n=pair_top)
    d_rows = torch.zeros((2 * nr, top_n, 8), dtype=torch.int64, device=dev)
    d_csums = torch.zeros((2 * nr, 3), dtype=torch.int64, device=dev)
    d_top = torch.zeros((n_pairs, pair_top, 8), dtype=torch.int64, device=dev)
    d_sums = torch.zeros((n_pairs, 8), dtype=torch.int64, device=dev)

    def one():
        return gpu.minimizer_chain_pairs_device(P, O, nr, k, w, 0, hit_max, False, shift, coord.data_ptr(), n_bins, d_rows.data_ptr(), 0, d_csums.data_ptr(),
                                                d_top.data_ptr(), d_sums.data_ptr(), st, pair=pair, **chain)

    def pairs_alone(rows, chain_top_n, want_stats=True):
        return gpu.chain_pairs_device(rows.data_ptr(), n_pairs, chain_top_n, d_top.data_ptr(), d_sums.data_ptr(), st, want_stats=want_stats, **pair)

    def three():
        hits()
        chain_stats = gpu.seed_chains_device(d_soff.data_ptr(), 2 * nr, d_seeds.data_ptr(), m, d_hoff.data_ptr(), d_hits.data_ptr(), h, shift, coord.data_ptr(), n_bins,
                                             d_rows.data_ptr(), 0, d_csums.data_ptr(), st, **chain)
        return chain_stats, pairs_alone(d_rows, top_n)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), out

    def row(ts):
        return f"{statistics.median(ts):.3f} ms ({min(ts):.3f}-{max(ts):.3f})"

    for _ in range(args.warmup):
        got, want = one(), three()
        assert got == want, (got, want)
    torch.cuda.synchronize()
    chain_stats, stats = got
    print(f"reads {nr} x {L} bases ({n_pairs} pairs of walks of {F}), (k, w) = ({k}, {w}), hit_max {hit_max}, shift {shift}, chain top_n {top_n}, pair top_n {pair_top}; "
          f"seeds {m}, hits {h}, chains {chain_stats['chains']}", flush=True)
    print(f"pairs: candidates {stats['candidates']}, proper {stats['proper']}, kept {stats['kept']}, paired {stats['paired']}, unique {stats['unique']}", flush=True)
    t_one, t_three, t_pairs = [], [], []
    for _ in range(args.reps):                                                    # the sides alternate
        t_one.append(timed(one)[0])
        t_three.append(timed(three)[0])
        t_pairs.append(timed(lambda: pairs_alone(d_rows, top_n))[0])
    torch.cuda.synchronize()
    a, b = statistics.median(t_one), statistics.median(t_three)
    clear = max(t_one) < min(t_three) and b - a >= 2 * (max(t_three) - min(t_three))
    print("| side | time |")
    print("|---|---|")
    print(f"| minimizer_chain_pairs_device | {row(t_one)} |")
    print(f"| stranded_minimizer_hits_device + seed_chains_device + chain_pairs_device | {row(t_three)} |")
    print(f"| chain_pairs_device alone on those rows | {row(t_pairs)} |")
    print(f"composition / fused {b / a:.3f}x; fused faster by the rule of profiles/jump_mid.md: {'yes' if clear else 'NO'}", flush=True)

    # the pair call alone: generated rows, about half of the entries chains of one locus, so that most candidates are proper
    print("| chain_top_n | pair top_n | candidates per pair | kept per pair | chain_pairs_device | without stats | bytes per pair | time of the bytes | bytes time / call |")
    print("|---|---|---|---|---|---|---|---|---|")
    pair = dict(orientation=0, min_fragment=100, max_fragment=1000, mean_fragment=400, unit=16, cost=1, min_score=0, top_n=pair_top)
    for chain_top_n in (int(x) for x in args.alone.split(",")):
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x6C5A00B0 + chain_top_n)
        shape = (4 * n_pairs, chain_top_n)
        rows = torch.zeros(shape + (8,), dtype=torch.int64, device=dev)
        begin = torch.randint(1000, 1200, shape, device=dev, generator=gen) + torch.randint(0, 2, shape, device=dev, generator=gen) * 300
        rows[:, :, 0] = torch.randint(0, 300, shape, device=dev, generator=gen)
        rows[:, :, 1] = (torch.rand(shape, device=dev, generator=gen) < 0.5).long() * 3
        rows[:, :, 6] = begin
        rows[:, :, 7] = begin + torch.randint(30, 150, shape, device=dev, generator=gen)
        for _ in range(args.warmup):
            stats = pairs_alone(rows, chain_top_n)
        torch.cuda.synchronize()
        t_with, t_without = [], []
        for _ in range(args.reps):
            t_with.append(timed(lambda: pairs_alone(rows, chain_top_n))[0])
            t_without.append(timed(lambda: pairs_alone(rows, chain_top_n, want_stats=False))[0])
        bytes_per_pair = 4 * chain_top_n * 32 + (pair_top + 1) * 64
        floor_ms = bytes_per_pair * n_pairs / args.bandwidth * 1e3
        print(f"| {chain_top_n} | {pair_top} | {stats['candidates'] / n_pairs:.1f} | {stats['kept'] / n_pairs:.1f} | {row(t_with)} | {row(t_without)} | {bytes_per_pair} | "
              f"{floor_ms:.3f} ms | {floor_ms / statistics.median(t_with):.1%} |", flush=True)
        del rows
    gpu.close()


if __name__ == "__main__":
    main()
