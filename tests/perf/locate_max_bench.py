#!/usr/bin/env python3
"""Batched locate(range, max_positions) (gcsa2_locate_max_into) on the snp graph: the ranges of find batches of several
pattern lengths, max_positions in {1, 8, 64, 256}; against the per-range gcsa2_locate_max loop on a subsample, whose values
must be the same.

    python tests/perf/locate_max_bench.py [--log2-bases 23] [--lengths 6,8,10,12,16] [--maxes 1,8,64,256] [--sub 300]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-bases", type=int, default=23)
    ap.add_argument("--order", type=int, default=32)
    ap.add_argument("--lengths", default="6,8,10,12,16")
    ap.add_argument("--maxes", default="1,8,64,256")
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--sub", type=int, default=300, help="ranges of the per-range loop")
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    args = ap.parse_args()
    import torch
    from workload import graphs, builder, patterns, cache
    from gcsa2_amd.binding import GCSA
    g = graphs.snp_graph(1 << args.log2_bases, 0x6C5A0010, 0x6C5A0011)
    path = os.path.join(args.cache_dir, f"snp_{args.log2_bases}_{args.order}_lmax.npz")
    t0 = time.perf_counter()
    if os.path.exists(path):
        ix = cache.load(path)
    else:
        ix = builder.build(g, args.order, keep_table=False)
        os.makedirs(args.cache_dir, exist_ok=True)
        cache.save(path, ix)
    print(f"index: 2^{args.log2_bases} bases, order {args.order}, {ix.n} path nodes ({time.perf_counter() - t0:.1f} s)")
    gpu = GCSA(ix)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    print("| pattern length | max_positions | ranges | random branch | batched | ranges/s | values/s | per-range loop (sub) "
          "| per range: loop / batched | same values |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for plen in (int(x) for x in args.lengths.split(",")):
        nq = args.queries
        pats = patterns.walk_patterns(g, nq, plen, 0x6C5A0060 + plen)
        flat, off = patterns.as_batch(pats)
        d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(8, dtype=np.uint8)])).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_rng = torch.zeros((nq, 2), dtype=torch.int64, device=dev)
        gpu.find_device(d_pat.data_ptr(), d_off.data_ptr(), nq, d_rng.data_ptr(), st)
        torch.cuda.synchronize()
        ranges = d_rng.cpu().numpy().view(np.uint64)
        counts = gpu.count_batch(ranges)
        d_off_out = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        for mx in (int(x) for x in args.maxes.split(",")):
            m = np.minimum(counts, np.uint64(mx))
            random_share = float(np.mean((m > 0) & (m < counts // np.uint64(2))))
            need = int(m.sum())
            d_val = torch.zeros(max(need, 1), dtype=torch.int64, device=dev)
            gpu.locate_max_into(d_rng.data_ptr(), nq, mx, d_off_out.data_ptr(), d_val.data_ptr(), need, st)   # warm-up
            torch.cuda.synchronize()
            reps = 3
            t0 = time.perf_counter()
            for _ in range(reps):
                total = gpu.locate_max_into(d_rng.data_ptr(), nq, mx, d_off_out.data_ptr(), d_val.data_ptr(), need, st)
            torch.cuda.synchronize()
            t_batch = (time.perf_counter() - t0) / reps
            offs = d_off_out.cpu().numpy().view(np.uint64)
            vals = d_val.cpu().numpy().view(np.uint64)
            # the per-range loop on a subsample of non-empty ranges (the ones a caller would ask)
            live = np.nonzero(counts > 0)[0]
            sub = live[np.linspace(0, len(live) - 1, min(args.sub, len(live))).astype(np.int64)] if len(live) else live
            same = True
            t0 = time.perf_counter()
            for q in sub:
                got = gpu.locate((int(ranges[q, 0]), int(ranges[q, 1])), max_positions=mx)
                same = same and np.array_equal(got, vals[int(offs[q]):int(offs[q + 1])])
            t_loop = time.perf_counter() - t0
            per_loop = t_loop / max(len(sub), 1)
            per_batch = t_batch / nq
            print(f"| {plen} | {mx} | {nq} | {random_share:.1%} | {t_batch * 1e3:.2f} ms | {nq / t_batch:.3g} | "
                  f"{total / t_batch:.3g} | {per_loop * 1e6:.0f} us/range ({len(sub)}) | {per_loop / per_batch:.0f}x | "
                  f"{'yes' if same else 'NO'} |", flush=True)
            if not same:
                sys.exit(1)


if __name__ == "__main__":
    main()
