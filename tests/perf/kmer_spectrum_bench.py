#!/usr/bin/env python3
"""Index k-mer spectrum (gcsa2_kmer_spectrum, gcsa2_index_kmer_support_device) on the 2^23-base repeat graph and on a de
Bruijn index in closed form (workload/dbg_torch.py, samples and counters included).

(a) gcsa2_kmer_spectrum with and without GCSA2_SPECTRUM_COUNTS against gcsa2_count_kmers at the same k on the same handle:
    count_kmers walks the same tree and keeps nothing but the number of leaves, so it is the floor of the walk.  The three
    alternate, `--reps` times each after a warm-up round; the best time of each is reported with the ratio to the floor.
(b) gcsa2_index_kmer_support_device against the composition a caller has with the list: gcsa2_list_kmers to the host, the
    records {0, k, sp, ep, count} uploaded, gcsa2_seed_support_device.  Both must give the same array.

All calls are complete on return, so wall-clock time around the call is the measurement.

    python tests/perf/kmer_spectrum_bench.py [--log2-bases 23] [--order 32] [--degree 28] [--k 8 12 16] [--support-k 16] [--dbg-support-k 12]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def alternate(calls, reps):
    """calls: {name: fn}; one warm-up round, then `reps` rounds in which the calls alternate: {name: (value, seconds)} of the
    fastest run of each."""
    best = {}
    for r in range(reps + 1):
        for name, fn in calls.items():
            t = time.perf_counter()
            value = fn()
            dt = time.perf_counter() - t
            if r > 0 and (name not in best or dt < best[name][1]):
                best[name] = (value, dt)
    return best


def spectrum_rows(gpu, what, ks, reps, n_hist, counters):
    for k in ks:
        if k > gpu.order():
            continue
        calls = {"count_kmers": lambda: gpu.count_kmers(k), "spectrum_length": lambda: gpu.kmer_spectrum(k, n_hist=n_hist, counts=False)}
        if counters:
            calls["spectrum_counts"] = lambda: gpu.kmer_spectrum(k, n_hist=n_hist, counts=True)
        got = alternate(calls, reps)
        floor = got["count_kmers"][1]
        row = {"index": what, "k": k, "kmers": got["count_kmers"][0], "count_kmers_ms": round(floor * 1e3, 3)}
        for name in ("spectrum_length", "spectrum_counts"):
            if name in got:
                (hist, stats), seconds = got[name]
                assert stats["kmers"] == row["kmers"] and int(hist.sum()) == row["kmers"]
                row[name + "_ms"] = round(seconds * 1e3, 3)
                row[name + "_over_floor"] = round(seconds / floor, 3)
                row[name + "_stats"] = stats
        print(json.dumps(row), flush=True)


def support_rows(gpu, what, ks, reps, hit_max, shift):
    import torch
    from gcsa2_amd.binding import SPECTRUM_STATS  # noqa: F401  (the binding must carry the calls)
    dev = torch.device("cuda", 0)
    for k in ks:
        if k > gpu.order():
            continue
        n_bins = 1 << 24
        a, b = torch.zeros(n_bins, dtype=torch.int64, device=dev), torch.zeros(n_bins, dtype=torch.int64, device=dev)

        def fused():
            a.zero_()
            return gpu.index_kmer_support_device(k, hit_max, shift, 0, a.data_ptr(), n_bins)

        def composed():
            b.zero_()
            t0 = time.perf_counter()
            rows = gpu.list_kmers(k)
            t1 = time.perf_counter()
            seeds = np.ascontiguousarray(np.column_stack([np.zeros(rows.shape[0], dtype=np.uint64), rows[:, 4], rows[:, 0], rows[:, 1], rows[:, 2]]))
            d_seeds = torch.from_numpy(seeds.view(np.int64)).to(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            stats = gpu.seed_support_device(d_seeds.data_ptr(), rows.shape[0], 0, hit_max, shift, 0, b.data_ptr(), n_bins)
            return stats, dict(list_ms=round((t1 - t0) * 1e3, 3), upload_ms=round((t2 - t1) * 1e3, 3), seed_support_ms=round((time.perf_counter() - t2) * 1e3, 3))

        got = alternate({"fused": fused, "composed": composed}, reps)
        (composed_stats, parts) = got["composed"][0]
        equal = bool(torch.equal(a, b)) and all(got["fused"][0][f] == composed_stats[f] for f in ("windows", "found", "counted", "added", "dropped"))
        print(json.dumps({"index": what, "k": k, "hit_max": hit_max, "shift": shift, "stats": got["fused"][0], "fused_ms": round(got["fused"][1] * 1e3, 3),
                          "composed_ms": round(got["composed"][1] * 1e3, 3), "composed_over_fused": round(got["composed"][1] / got["fused"][1], 3),
                          "composed_parts": parts, "equal": equal}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-bases", type=int, default=23)
    ap.add_argument("--order", type=int, default=32)
    ap.add_argument("--degree", type=int, default=28, help="the de Bruijn index: a maximal LFSR text of this degree, order degree / 2 (0: skip)")
    ap.add_argument("--k", type=int, nargs="+", default=[8, 12, 16])
    ap.add_argument("--support-k", type=int, nargs="*", default=[16])
    ap.add_argument("--dbg-support-k", type=int, nargs="*", default=[12],
                    help="a k-mer of the de Bruijn index occurs 4^(order - k) times: 4^k k-mers, 4^order values in all")
    ap.add_argument("--hit-max", type=int, default=64)
    ap.add_argument("--shift", type=int, default=11)
    ap.add_argument("--n-hist", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    args = ap.parse_args()
    import torch
    from workload import graphs, builder, cache
    from gcsa2_amd.binding import GCSA
    if args.log2_bases > 0:
        g = graphs.repeat_graph(1 << args.log2_bases, 0x6C5A0010, 0x6C5A0011)
        path = os.path.join(args.cache_dir, f"repeat_{args.log2_bases}_{args.order}_support.npz")
        t0 = time.perf_counter()
        if os.path.exists(path):
            ix = cache.load(path)
        else:
            ix = builder.build(g, args.order, keep_table=False)
            os.makedirs(args.cache_dir, exist_ok=True)
            cache.save(path, ix)
        what = f"repeat 2^{args.log2_bases} order {args.order}"
        print(f"index: {what}, {ix.n} path nodes ({time.perf_counter() - t0:.1f} s)", flush=True)
        gpu = GCSA(ix)
        spectrum_rows(gpu, what, args.k, args.reps, args.n_hist, True)
        support_rows(gpu, what, args.support_k, args.reps, args.hit_max, args.shift)
        gpu.close()
        del ix
    if args.degree > 0:
        from workload import dbg_torch
        t0 = time.perf_counter()
        ix, dbg = dbg_torch.build_dbg(args.degree, junctions=80, device=torch.device("cuda", 0), full=True)
        del dbg
        torch.cuda.empty_cache()
        what = f"de Bruijn (LFSR degree {args.degree}) order {args.degree // 2}"
        print(f"index: {what}, {ix.n} path nodes ({time.perf_counter() - t0:.1f} s)", flush=True)
        gpu = GCSA(ix, device=0, with_lcp=False)
        spectrum_rows(gpu, what, args.k, args.reps, args.n_hist, True)
        support_rows(gpu, what, args.dbg_support_k, args.reps, args.hit_max, args.shift)
        gpu.close()


if __name__ == "__main__":
    main()
