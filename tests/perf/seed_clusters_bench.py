#!/usr/bin/env python3
"""Batched seed clusters on the repeat graph: the batch of tests/perf/minimizer_hits_bench.py (`--reads` walks of
`--read-length` bases), (k, w) minimizers, hit_max = --hit-max (SKIP), a linear coordinate map at --shift (coord = bin <<
shift), --band and --top.  Four sides, timed with device events around each side's whole call sequence in alternating rounds
in one process:

  1. gcsa2_minimizer_hits_device alone, buffers of the exact sizes;
  2. the same call followed by the clustering in torch on the device: the anchors' (read, diagonal) keys sorted, boundaries
     where the read changes or the gap exceeds the band, a second sort by (cluster, position) with a running maximum of the
     end for `covered`, segment sums, and a stable sort by (read, covered and anchors descending) for the top_n;
  3. gcsa2_minimizer_clusters_device;
  4. gcsa2_seed_clusters_device alone on the hits of (1).

(2) and (3) must agree on diag_min, anchors and covered of every top entry and on the clusters of every read.  --only-new
runs (3) and (4) alone, a few times, for a kernel trace.

    python tests/perf/seed_clusters_bench.py [--log2-bases 23] [--order 32] [--reads 1000000] [--read-length 150]
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
    ap.add_argument("--top", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
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
    nr, L, hit_max, shift, band, top_n = args.reads, args.read_length, args.hit_max, args.shift, args.band, args.top
    k, w = (int(x) for x in args.kw.split(","))
    reads = patterns.walk_patterns(g, nr, L, 0x6C5A0090)
    flat, off = patterns.as_batch(reads)
    d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(8, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    P, O = d_pat.data_ptr(), d_off.data_ptr()
    os.environ.pop("GCSA2_CLUSTER_LDS", None)

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
    assert n_bins << shift < (1 << 40) and nr < (1 << 22) and L < (1 << 12)
    d_top = torch.zeros((nr, top_n, 8), dtype=torch.int64, device=dev)
    d_sums = torch.zeros((nr, 3), dtype=torch.int64, device=dev)
    read_ids = torch.arange(nr, dtype=torch.int64, device=dev)
    seed_ids = torch.arange(max(m, 1), dtype=torch.int64, device=dev)

    def fused():
        return gpu.minimizer_clusters_device(P, O, nr, k, w, 0, hit_max, False, shift, coord.data_ptr(), n_bins, band, top_n, d_top.data_ptr(), d_sums.data_ptr(), st)

    def seed_form():
        return gpu.seed_clusters_device(d_soff.data_ptr(), nr, d_seeds.data_ptr(), m, d_hoff.data_ptr(), d_hits.data_ptr(), h, shift, coord.data_ptr(), n_bins,
                                        band, top_n, d_top.data_ptr(), d_sums.data_ptr(), st)

    def composition():
        hits_alone()
        v = d_hits[:h]
        seed_of_hit = torch.repeat_interleave(seed_ids[:m], d_hoff[1:m + 1] - d_hoff[:m], output_size=h)
        read_of_seed = torch.repeat_interleave(read_ids, d_soff[1:] - d_soff[:-1], output_size=m)
        rd, pos = read_of_seed[seed_of_hit], d_seeds[seed_of_hit, 0]
        end = pos + d_seeds[seed_of_hit, 1]
        diag = coord[v >> shift] + (v & ((1 << shift) - 1)) - pos + (1 << 12)                  # every diagonal is above -2^12
        key, order = torch.sort((rd << 41) | diag)                                             # by (read, diagonal)
        rd, diag, pos, end = key >> 41, key & ((1 << 41) - 1), pos[order], end[order]
        head = torch.ones(h, dtype=torch.bool, device=dev)
        head[1:] = (rd[1:] != rd[:-1]) | (diag[1:] - diag[:-1] > band)
        cid = torch.cumsum(head, 0) - 1
        nc = int(cid[-1]) + 1 if h else 0
        c_read, c_diag = rd[head], diag[head] - (1 << 12)
        anchors = torch.bincount(cid, minlength=nc)
        key2, order2 = torch.sort((cid << 12) | pos)                                           # by (cluster, position)
        c2, p2, e2 = key2 >> 12, key2 & ((1 << 12) - 1), end[order2]
        reach = torch.cummax((c2 << 12) | e2, 0).values
        before = torch.cat([torch.full((1,), -1, dtype=torch.int64, device=dev), reach[:-1]])
        reached = torch.where((before >> 12) == c2, before & ((1 << 12) - 1), torch.zeros_like(before))
        lo = torch.maximum(p2, reached)
        covered = torch.zeros(nc, dtype=torch.int64, device=dev).index_add_(0, c2, torch.clamp(e2 - lo, min=0))
        clusters = torch.bincount(c_read, minlength=nr)
        # the clusters are in (read, diag_min) order: a stable sort by (read, covered and anchors descending) ranks them
        rank_key = (c_read << 40) | (((1 << 12) - 1 - covered) << 24) | ((1 << 24) - 1 - anchors)
        ranked = torch.sort(rank_key, stable=True).indices
        first = torch.cumsum(clusters, 0) - clusters
        r_read = c_read[ranked]
        place = torch.arange(nc, dtype=torch.int64, device=dev) - first[r_read]
        keep = place < top_n
        out = torch.zeros((nr, top_n, 3), dtype=torch.int64, device=dev)
        out[r_read[keep], place[keep], 0] = c_diag[ranked][keep]
        out[r_read[keep], place[keep], 1] = anchors[ranked][keep]
        out[r_read[keep], place[keep], 2] = covered[ranked][keep]
        return out, clusters

    if args.only_new:
        for _ in range(args.warmup + 3):
            stats = fused()
            seed_form()
        torch.cuda.synchronize()
        print(f"# {stats}", flush=True)
        gpu.close()
        return
    stats = fused()
    want, clusters = composition()
    torch.cuda.synchronize()
    same = bool((d_top[:, :, 0] == want[:, :, 0]).all()) and bool((d_top[:, :, 2] == want[:, :, 1]).all()) and bool((d_top[:, :, 4] == want[:, :, 2]).all())
    same = same and bool((d_sums[:, 2] == clusters).all())
    seed_stats = seed_form()
    torch.cuda.synchronize()
    same = same and seed_stats == stats
    del want, clusters
    for _ in range(args.warmup - 1):
        hits_alone(), composition(), fused(), seed_form()
    torch.cuda.synchronize()
    t = {"hits": [], "composition": [], "fused": [], "seed": []}
    for _ in range(args.reps):                                                                # the sides alternate
        t["hits"].append(timed(hits_alone)[0])
        t["composition"].append(timed(composition)[0])
        t["fused"].append(timed(fused)[0])
        t["seed"].append(timed(seed_form)[0])
    med = {name: statistics.median(ts) for name, ts in t.items()}
    print(f"reads {nr} x {L} bases, (k, w) = ({k}, {w}), hit_max {hit_max}, shift {shift}, band {band}, top_n {top_n}; seeds {m}, hits {h}")
    print(f"anchors per read {stats['anchors'] / nr:.1f} (unplaced {stats['unplaced']}), clusters per read {stats['clusters'] / nr:.2f}, "
          f"spilled groups {stats['spilled']} ({100.0 * stats['spilled'] / nr:.4f} %)")
    print("| side | time | against (1) |")
    print("|---|---|---|")
    print(f"| 1. minimizer_hits_device | {spread(t['hits'])} | 1.00x |")
    print(f"| 2. minimizer_hits_device + torch clustering | {spread(t['composition'])} | {med['composition'] / med['hits']:.2f}x |")
    print(f"| 3. minimizer_clusters_device | {spread(t['fused'])} | {med['fused'] / med['hits']:.2f}x |")
    print(f"| 4. seed_clusters_device on the hits of (1) | {spread(t['seed'])} | {med['seed'] / med['hits']:.2f}x |")
    print(f"(2) / (3) = {med['composition'] / med['fused']:.2f}x; (3) - (1) = {med['fused'] - med['hits']:.3f} ms; same = {'yes' if same else 'NO'}", flush=True)
    gpu.close()
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
