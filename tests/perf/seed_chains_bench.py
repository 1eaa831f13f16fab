#!/usr/bin/env python3
"""Batched seed chains on the repeat graph: the batch of tests/perf/seed_clusters_bench.py (`--reads` walks of `--read-length`
bases), (k, w) minimizers, hit_max = --hit-max (SKIP), a linear coordinate map at --shift (coord = bin << shift).  Timed with
device events around each call in alternating rounds in one process:

  1. gcsa2_minimizer_hits_device alone, buffers of the exact sizes;
  2. gcsa2_minimizer_clusters_device (band --band, top_n --top);
  3. gcsa2_minimizer_chains_device, once per (lookback, member_cap) of --lookbacks x --member-caps (top_n --top);
  4. gcsa2_seed_chains_device alone on the hits of (1), at the first (lookback, member_cap).

Every chains call must return the stats of the seed form.  Then, separately, the large path: gcsa2_seed_chains_device on one
group of --large anchors (three diagonals with a little noise), which no LDS holds.  --only-new runs the first fused chains
call alone, a few times, for a kernel trace.

    python tests/perf/seed_chains_bench.py [--log2-bases 23] [--order 32] [--reads 1000000] [--read-length 150]
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
    ap.add_argument("--kw", default="16,11")
    ap.add_argument("--hit-max", type=int, default=64)
    ap.add_argument("--shift", type=int, default=10)
    ap.add_argument("--band", type=int, default=16)
    ap.add_argument("--max-gap", type=int, default=500)
    ap.add_argument("--top", type=int, default=4)
    ap.add_argument("--lookbacks", default="16,64")
    ap.add_argument("--member-caps", default="0,32")
    ap.add_argument("--large", type=int, default=100_000)
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
    nr, L, hit_max, shift, top_n = args.reads, args.read_length, args.hit_max, args.shift, args.top
    k, w = (int(x) for x in args.kw.split(","))
    shapes = [(int(lb), int(cap)) for lb in args.lookbacks.split(",") for cap in args.member_caps.split(",")]
    reads = patterns.walk_patterns(g, nr, L, 0x6C5A0090)
    flat, off = patterns.as_batch(reads)
    d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(8, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    P, O = d_pat.data_ptr(), d_off.data_ptr()
    os.environ.pop("GCSA2_CLUSTER_LDS", None)
    os.environ.pop("GCSA2_CHAIN_LDS", None)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), out

    def spread(ts):
        return f"{statistics.median(ts):.3f} ms ({min(ts):.3f}-{max(ts):.3f})"

    d_soff = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
    try:                                                                      # the sizes, from a refusal (not timed)
        m, h = gpu.minimizer_hits_device(P, O, nr, k, w, 0, hit_max, False, 0, d_soff.data_ptr(), 0, 0, d_soff.data_ptr(), 0, 0, st)
    except Gcsa2Error as e:
        if e.code != STATUS_BUFFER_TOO_SMALL:
            raise
        m, h = e.needed
    d_seeds = torch.zeros((max(m, 1), 5), dtype=torch.int64, device=dev)
    d_hoff = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    d_hits = torch.zeros(max(h, 1), dtype=torch.int64, device=dev)

    def hits_alone():
        return gpu.minimizer_hits_device(P, O, nr, k, w, 0, hit_max, False, 0, d_soff.data_ptr(), d_seeds.data_ptr(), m, d_hoff.data_ptr(), d_hits.data_ptr(), h, st)

    hits_alone()
    n_bins = int((d_hits[:h] >> shift).max()) + 1 if h else 1
    coord = torch.arange(n_bins, dtype=torch.int64, device=dev) << shift
    max_cap = max(cap for _, cap in shapes)
    d_top = torch.zeros((nr, top_n, 8), dtype=torch.int64, device=dev)
    d_mem = torch.zeros((nr, top_n, max(max_cap, 1), 2), dtype=torch.int64, device=dev)
    d_sums = torch.zeros((nr, 3), dtype=torch.int64, device=dev)

    def clusters():
        return gpu.minimizer_clusters_device(P, O, nr, k, w, 0, hit_max, False, shift, coord.data_ptr(), n_bins, args.band, top_n, d_top.data_ptr(), d_sums.data_ptr(), st)

    def chains(lookback, cap):
        return lambda: gpu.minimizer_chains_device(P, O, nr, k, w, 0, hit_max, False, shift, coord.data_ptr(), n_bins, d_top.data_ptr(), d_mem.data_ptr(),
                                                   d_sums.data_ptr(), st, band=args.band, max_gap=args.max_gap, lookback=lookback, match=1, gap=1,
                                                   min_score=0, top_n=top_n, member_cap=cap)

    def seed_form():
        lookback, cap = shapes[0]
        return gpu.seed_chains_device(d_soff.data_ptr(), nr, d_seeds.data_ptr(), m, d_hoff.data_ptr(), d_hits.data_ptr(), h, shift, coord.data_ptr(), n_bins,
                                      d_top.data_ptr(), d_mem.data_ptr(), d_sums.data_ptr(), st, band=args.band, max_gap=args.max_gap, lookback=lookback,
                                      match=1, gap=1, min_score=0, top_n=top_n, member_cap=cap)

    if args.only_new:
        for _ in range(args.warmup + 3):
            stats = chains(*shapes[0])()
        torch.cuda.synchronize()
        print(f"# {stats}", flush=True)
        gpu.close()
        return
    sides = [("1. minimizer_hits_device", hits_alone), ("2. minimizer_clusters_device", clusters)]
    sides += [(f"3. minimizer_chains_device, lookback {lb}, member_cap {cap}", chains(lb, cap)) for lb, cap in shapes]
    sides += [(f"4. seed_chains_device on the hits of (1), lookback {shapes[0][0]}, member_cap {shapes[0][1]}", seed_form)]
    stats = chains(*shapes[0])()
    same = seed_form() == stats
    for _ in range(args.warmup):
        for _, fn in sides:
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name, _ in sides}
    for _ in range(args.reps):                                                                # the sides alternate
        for name, fn in sides:
            t[name].append(timed(fn)[0])
    med = {name: statistics.median(ts) for name, ts in t.items()}
    base, clu = med[sides[0][0]], med[sides[1][0]]
    print(f"reads {nr} x {L} bases, (k, w) = ({k}, {w}), hit_max {hit_max}, shift {shift}, band {args.band}, max_gap {args.max_gap}, top_n {top_n}; seeds {m}, hits {h}")
    print(f"anchors per read {stats['anchors'] / nr:.1f} (unplaced {stats['unplaced']}), chains per read {stats['chains'] / nr:.2f}, "
          f"spilled groups {stats['spilled']} ({100.0 * stats['spilled'] / nr:.4f} %)")
    print("| side | time | added over (1) | against what (2) adds |")
    print("|---|---|---|---|")
    for name, _ in sides:
        added = med[name] - base
        ratio = f"{added / (clu - base):.2f}x" if name[0] in "23" and clu > base else "-"
        print(f"| {name} | {spread(t[name])} | {added:.3f} ms | {ratio} |")
    print(f"same stats from the fused and the seed form: {'yes' if same else 'NO'}", flush=True)
    # the large path: one group of --large anchors on three diagonals, seeds of 16 bases at rising positions
    rng = np.random.default_rng(0x1A26E)
    n = args.large
    pos = np.sort(rng.integers(0, 1 << 20, n)).astype(np.int64)
    seeds = np.zeros((n, 5), dtype=np.int64)
    seeds[:, 0], seeds[:, 1] = pos, 16
    values = (rng.integers(0, 3, n).astype(np.int64) << 22) + (1 << 24) + pos + rng.integers(-3, 4, n)
    l_goff = torch.tensor([0, n], dtype=torch.int64, device=dev)
    l_seeds, l_hoff, l_hits = torch.from_numpy(seeds).to(dev), torch.arange(n + 1, dtype=torch.int64, device=dev), torch.from_numpy(values).to(dev)
    l_map = torch.arange(1 << 15, dtype=torch.int64, device=dev) << 10

    def large():
        return gpu.seed_chains_device(l_goff.data_ptr(), 1, l_seeds.data_ptr(), n, l_hoff.data_ptr(), l_hits.data_ptr(), n, 10, l_map.data_ptr(), 1 << 15,
                                      d_top.data_ptr(), d_mem.data_ptr(), d_sums.data_ptr(), st, band=args.band, max_gap=args.max_gap, lookback=shapes[0][0],
                                      match=1, gap=1, min_score=0, top_n=top_n, member_cap=shapes[0][1])

    large_stats = large()
    ts = [timed(large)[0] for _ in range(args.reps)]
    print(f"large path: one group of {n} anchors, lookback {shapes[0][0]}: {spread(ts)}; {large_stats}", flush=True)
    gpu.close()
    if not same or large_stats["spilled"] != 1:
        sys.exit(1)


if __name__ == "__main__":
    main()
