#!/usr/bin/env python3
"""Sub-MEM reseeding (gcsa2_sub_mem_hits_device): 256-bp patterns with a substitution about every 40 bp on the snp graph and
the repeat-rich graph; the MEMs of gcsa2_mem_hits_device (no cap) reseeded for min_length x hit_max x batch size, with
reseed_length = ceil(1.5 x min_length).  For each run: reseeded MEMs, sub-MEMs per reseeded MEM, hits, the fused call next
to the mem_hits_device call on the same batch, and the host composition -- the walk through the public batched calls
(lf_batch, count_batch, parent_batch per round, then locate_batch / locate_max_batch) -- with whether the two agree.

    python tests/perf/sub_mem_hits_bench.py [--graphs snp,repeat] [--log2-bases 22] [--queries 100000,1000000] [--mins 12,20] [--maxes 0,64]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "perf"))

from mem_hits_bench import substitute, timed     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="snp,repeat")
    ap.add_argument("--log2-bases", type=int, default=22)
    ap.add_argument("--order", type=int, default=32)
    ap.add_argument("--queries", default="100000,1000000")
    ap.add_argument("--mins", default="12,20")
    ap.add_argument("--maxes", default="0,64")
    ap.add_argument("--length", type=int, default=256)
    ap.add_argument("--period", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host", type=int, default=1, help="time the host composition too (and check the results against it)")
    ap.add_argument("--host-max-queries", type=int, default=1_000_000, help="largest batch the host composition runs on")
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    args = ap.parse_args()
    import torch
    from workload import graphs, builder, patterns, cache
    from gcsa2_amd.binding import GCSA, LCPArray, Gcsa2Error
    from test_sub_mems import composition_core, with_hits
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    print("| graph | patterns | min | reseed | hit_max | MEMs | reseeded | sub-MEMs | per reseeded | hits | mem_hits ms | fused ms "
          "| fused / mem_hits | host composition ms | host / fused | same |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for kind in args.graphs.split(","):
        make = graphs.snp_graph if kind == "snp" else graphs.repeat_graph
        g = make(1 << args.log2_bases, 0x6C5A0010, 0x6C5A0011)
        path = os.path.join(args.cache_dir, f"{kind}_{args.log2_bases}_{args.order}_mem.npz")
        t0 = time.perf_counter()
        if os.path.exists(path):
            ix = cache.load(path)
        else:
            ix = builder.build(g, args.order, keep_table=False)
            os.makedirs(args.cache_dir, exist_ok=True)
            cache.save(path, ix)
        print(f"<!-- {kind}: 2^{args.log2_bases} bases, order {args.order}, {ix.n} path nodes ({time.perf_counter() - t0:.1f} s) -->", flush=True)
        gpu = GCSA(ix)
        lcp = LCPArray(gpu, int(gpu._L.gcsa2_lcp_values(gpu.handle)), int(gpu._L.gcsa2_lcp_size(gpu.handle)))
        char2comp = np.asarray(ix.char2comp, dtype=np.uint8)
        for nq in (int(x) for x in args.queries.split(",")):
            pats = substitute(patterns.walk_patterns(g, nq, args.length, 0x6C5A0070 + nq), args.period, nq)
            flat, off = patterns.as_batch(pats)
            total = int(off[-1])
            d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(16, dtype=np.uint8)])).to(dev)
            d_off = torch.from_numpy(off.view(np.int64)).to(dev)
            d_moff = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            for L in (int(x) for x in args.mins.split(",")):
                R = (3 * L + 1) // 2
                for mx in (int(x) for x in args.maxes.split(",")):
                    sample = mx > 0
                    # the MEMs: mem_hits_device with the same hit_max (its time is the yardstick), MEMs kept on the device
                    try:
                        mem_need, hit_need = gpu.mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, L, mx, int(sample),
                                                                 d_moff.data_ptr(), 0, 0, d_moff.data_ptr(), 0, 0, st)
                    except Gcsa2Error as e:
                        mem_need, hit_need = e.needed
                    d_mems = torch.zeros((max(mem_need, 1), 5), dtype=torch.int64, device=dev)
                    d_mhoff = torch.zeros(mem_need + 1, dtype=torch.int64, device=dev)
                    d_mhits = torch.zeros(max(hit_need, 1), dtype=torch.int64, device=dev)
                    t_mem, (m, _) = timed(lambda: gpu.mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, L, mx, int(sample),
                                                                      d_moff.data_ptr(), d_mems.data_ptr(), mem_need, d_mhoff.data_ptr(),
                                                                      d_mhits.data_ptr(), hit_need, st), args.reps)
                    d_soff = torch.zeros(m + 1, dtype=torch.int64, device=dev)
                    try:
                        s_need, h_need = gpu.sub_mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, d_moff.data_ptr(), d_mems.data_ptr(),
                                                                 m, L, R, mx, int(sample), d_soff.data_ptr(), 0, 0, d_soff.data_ptr(), 0, 0, st)
                    except Gcsa2Error as e:
                        s_need, h_need = e.needed
                    d_subs = torch.zeros((max(s_need, 1), 5), dtype=torch.int64, device=dev)
                    d_hoff = torch.zeros(s_need + 1, dtype=torch.int64, device=dev)
                    d_hits = torch.zeros(max(h_need, 1), dtype=torch.int64, device=dev)
                    fused = lambda: gpu.sub_mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, d_moff.data_ptr(), d_mems.data_ptr(),
                                                            m, L, R, mx, int(sample), d_soff.data_ptr(), d_subs.data_ptr(), s_need,
                                                            d_hoff.data_ptr(), d_hits.data_ptr(), h_need, st)
                    t_fused, (s, h) = timed(fused, args.reps)
                    mems = d_mems[:m].cpu().numpy().view(np.uint64)
                    moff = d_moff.cpu().numpy().view(np.uint64)
                    reseeded = int((mems[:, 1] >= np.uint64(R)).sum())
                    t_host, same = float("nan"), "-"
                    if args.host and nq <= args.host_max_queries:
                        t0 = time.perf_counter()
                        soff, subs = composition_core(gpu, lcp, flat, off, moff, mems, L, R, int(ix.n), char2comp)
                        hoff, hits = with_hits(gpu, subs, mx, sample)
                        t_host = time.perf_counter() - t0
                        got = (d_soff.cpu().numpy().view(np.uint64), d_subs[:s].cpu().numpy().view(np.uint64),
                               d_hoff[: s + 1].cpu().numpy().view(np.uint64), d_hits[:h].cpu().numpy().view(np.uint64))
                        same = "yes" if all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, (soff, subs, hoff, hits))) else "NO"
                    per = f"{s / reseeded:.2f}" if reseeded else "-"
                    print(f"| {kind} | {nq} | {L} | {R} | {mx} | {m} | {reseeded} | {s} | {per} | {h} | {t_mem * 1e3:.2f} | {t_fused * 1e3:.2f} | "
                          f"{t_fused / t_mem:.2f} | {t_host * 1e3:.1f} | {t_host / t_fused:.1f}x | {same} |", flush=True)
                    if same == "NO":
                        sys.exit(1)
                    del d_mems, d_mhoff, d_mhits, d_subs, d_hoff, d_hits
        gpu.close()


if __name__ == "__main__":
    main()
