#!/usr/bin/env python3
"""MEM hits (gcsa2_mem_hits_device): 256-bp patterns with a substitution about every 40 bp, min_length 20, on the snp graph
and the repeat-rich graph; hit_max x policy x batch size.  For each run: MEMs/s, hits/s, the share of MEMs per class, the
fused call against the sum of its parts on the same batch (match_breaks_device + locate_into of the full class +
locate_max_into of the sampled class, each timed alone) and against the host composition through the public calls
(match_breaks_batch -> count_batch -> locate_batch / locate_max_batch -> interleave).  The fused call's results are checked
against the host composition.

    python tests/perf/mem_hits_bench.py [--graphs snp,repeat] [--log2-bases 25] [--queries 100000,1000000] [--maxes 0,8,64,512]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def substitute(pats, period, seed):
    """A substitution about every `period` bases: each base changes with probability 1 / period to one of the other three."""
    rng = np.random.default_rng(seed)
    codes = np.frombuffer(b"ACGT", dtype=np.uint8)
    lut = np.full(256, 0, dtype=np.int64)
    lut[codes] = np.arange(4)
    hit = rng.random(pats.shape) < 1.0 / period
    shifted = codes[(lut[pats] + rng.integers(1, 4, size=pats.shape)) % 4]
    return np.where(hit & np.isin(pats, codes), shifted, pats).astype(np.uint8)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best.append(time.perf_counter() - t0)
    return float(np.median(best)), out


def host_composition(gpu, flat, off, min_length, hit_max, sample):
    boff, brk, _, _ = gpu.match_breaks_batch(flat, off, min_length)
    ranges = np.ascontiguousarray(brk[:, 2:4])
    counts = gpu.count_batch(ranges)
    full = (counts > 0) & ((hit_max == 0) | (counts <= np.uint64(hit_max)))
    samp = (counts > np.uint64(hit_max)) & (hit_max > 0) & sample
    sizes = np.zeros(ranges.shape[0], dtype=np.uint64)
    pieces = []
    for mask, fn in ((full, lambda r: gpu.locate_batch(r)), (samp, lambda r: gpu.locate_max_batch(r, hit_max))):
        idx = np.nonzero(mask)[0]
        if idx.shape[0]:
            o, v = fn(np.ascontiguousarray(ranges[idx]))
            sizes[idx] = np.diff(o)
            pieces.append((idx, o, v))
    hoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    hits = np.zeros(int(hoff[-1]), dtype=np.uint64)
    for idx, o, v in pieces:                         # interleave the two CSRs into MEM order
        n = np.diff(o).astype(np.int64)
        dest = np.repeat(hoff[idx].astype(np.int64) - o[:-1].astype(np.int64), n) + np.arange(int(o[-1]), dtype=np.int64)
        hits[dest] = v
    return boff, np.concatenate([brk, counts.reshape(-1, 1)], axis=1), hoff, hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="snp,repeat")
    ap.add_argument("--log2-bases", type=int, default=25)
    ap.add_argument("--order", type=int, default=32)
    ap.add_argument("--queries", default="100000,1000000")
    ap.add_argument("--maxes", default="0,8,64,512")
    ap.add_argument("--length", type=int, default=256)
    ap.add_argument("--period", type=int, default=40)
    ap.add_argument("--min-length", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host", type=int, default=1, help="time the host composition too (and check the results against it)")
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    args = ap.parse_args()
    import torch
    from workload import graphs, builder, patterns, cache
    from gcsa2_amd.binding import GCSA, Gcsa2Error
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    L = args.min_length
    print("| graph | patterns | hit_max | policy | MEMs | hits | full / sampled / none | fused ms | MEMs/s | hits/s "
          "| parts ms (breaks + full + sampled) | fused / parts | host composition ms | host / fused | same |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
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
        for nq in (int(x) for x in args.queries.split(",")):
            pats = substitute(patterns.walk_patterns(g, nq, args.length, 0x6C5A0070 + nq), args.period, nq)
            flat, off = patterns.as_batch(pats)
            total = int(off[-1])
            d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(16, dtype=np.uint8)])).to(dev)
            d_off = torch.from_numpy(off.view(np.int64)).to(dev)
            d_moff = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            d_boff = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            for mx in (int(x) for x in args.maxes.split(",")):
                for sample in ((False,) if mx == 0 else (False, True)):
                    try:                                  # no room: BUFFER_TOO_SMALL with the sizes needed
                        mem_need, hit_need = gpu.mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, L, mx, int(sample),
                                                                 d_moff.data_ptr(), 0, 0, d_boff.data_ptr(), 0, 0, st)
                    except Gcsa2Error as e:
                        mem_need, hit_need = e.needed
                    mcap, hcap = mem_need, hit_need
                    d_mems = torch.zeros((max(mcap, 1), 5), dtype=torch.int64, device=dev)
                    d_hoff = torch.zeros(mcap + 1, dtype=torch.int64, device=dev)
                    d_hits = torch.zeros(max(hcap, 1), dtype=torch.int64, device=dev)
                    fused = lambda: gpu.mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, L, mx, int(sample), d_moff.data_ptr(),
                                                        d_mems.data_ptr(), mcap, d_hoff.data_ptr(), d_hits.data_ptr(), hcap, st)
                    t_fused, (m, h) = timed(fused, args.reps)
                    mems = d_mems[:m].cpu().numpy().view(np.uint64)
                    counts = mems[:, 4]
                    full = (counts > 0) & ((mx == 0) | (counts <= np.uint64(mx)))
                    samp = (counts > np.uint64(mx)) & (mx > 0) & sample
                    # the parts, each alone on the same batch
                    d_brk = torch.zeros((max(m, 1), 4), dtype=torch.int64, device=dev)
                    t_breaks, _ = timed(lambda: gpu.match_breaks_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, d_boff.data_ptr(),
                                                                        d_brk.data_ptr(), m, stream=st, min_length=L), args.reps)
                    t_full = t_samp = 0.0
                    for mask, kind_ in ((full, "full"), (samp, "sampled")):
                        idx = np.nonzero(mask)[0]
                        if not idx.shape[0]:
                            continue
                        rr = torch.from_numpy(np.ascontiguousarray(mems[idx, 2:4]).view(np.int64)).to(dev)
                        d_o = torch.zeros(idx.shape[0] + 1, dtype=torch.int64, device=dev)
                        need = int(counts[idx].sum()) if kind_ == "full" else int(np.minimum(counts[idx], np.uint64(mx)).sum())
                        d_v = torch.zeros(max(need, 1), dtype=torch.int64, device=dev)
                        if kind_ == "full":
                            t_full, _ = timed(lambda: gpu.locate_into(rr.data_ptr(), idx.shape[0], d_o.data_ptr(), d_v.data_ptr(), need, st), args.reps)
                        else:
                            t_samp, _ = timed(lambda: gpu.locate_max_into(rr.data_ptr(), idx.shape[0], mx, d_o.data_ptr(), d_v.data_ptr(), need, st),
                                              args.reps)
                    t_parts = t_breaks + t_full + t_samp
                    t_host, same = float("nan"), "-"
                    if args.host:
                        t0 = time.perf_counter()
                        want = host_composition(gpu, flat, off, L, mx, sample)
                        t_host = time.perf_counter() - t0
                        got = (d_moff.cpu().numpy().view(np.uint64), mems, d_hoff[: m + 1].cpu().numpy().view(np.uint64),
                               d_hits[:h].cpu().numpy().view(np.uint64))
                        same = "yes" if all(np.array_equal(a, b) for a, b in zip(got, want)) else "NO"
                    share = f"{full.mean():.1%} / {samp.mean():.1%} / {max(0.0, 1 - full.mean() - samp.mean()):.1%}" if m else "-"
                    print(f"| {kind} | {nq} | {mx} | {'sample' if sample else 'skip'} | {m} | {h} | {share} | {t_fused * 1e3:.2f} | "
                          f"{m / t_fused:.3g} | {h / t_fused:.3g} | {t_parts * 1e3:.2f} ({t_breaks * 1e3:.2f} + {t_full * 1e3:.2f} + "
                          f"{t_samp * 1e3:.2f}) | {t_fused / t_parts:.2f} | {t_host * 1e3:.1f} | {t_host / t_fused:.1f}x | {same} |", flush=True)
                    if same == "NO":
                        sys.exit(1)
                    del d_mems, d_hoff, d_hits, d_brk
        gpu.close()


if __name__ == "__main__":
    main()
