#!/usr/bin/env python3
"""Batched k-mer hits (gcsa2_kmer_hits_device) on the snp graph against the composition of the public calls that gave the same
arrays before it: gcsa2_kmer_windows_device with ranges and counts, a torch selection of the found windows and their split at
the cap, gcsa2_locate_into and gcsa2_locate_max_into on the two classes, and the interleave of their values in seed order.
`--reads` walks of `--read-length` bases, every window of k characters at stride 1; once as drawn and once with a substitution
about every `--period` bases, so that most windows are not found.

Rows: k in --k, both batches, (hit_max, policy) in (0, skip), (0, sample), (8, skip), (8, sample).  Device events around each
side's whole call sequence, warm-up runs first, then the median and min-max of `--reps` timed runs, the two sides alternating.
Both sides run on buffers of the exact sizes (found out beforehand, not timed) and must give the same four arrays.

    python tests/perf/kmer_hits_bench.py [--log2-bases 22] [--order 32] [--reads 1000000] [--read-length 150] [--k 32 16]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def substitute(reads, period, seed):
    """`reads` (n, L) bytes with a different base at about every period-th position."""
    rng = np.random.default_rng(seed)
    out = reads.copy()
    where = rng.random(reads.shape) < 1.0 / period
    code = np.zeros(256, dtype=np.uint8)
    code[list(b"ACGT")] = (0, 1, 2, 3)
    shifted = np.frombuffer(b"ACGT", dtype=np.uint8)[(code[reads] + rng.integers(1, 4, reads.shape, dtype=np.uint8)) % 4]
    out[where] = shifted[where]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-bases", type=int, default=22)
    ap.add_argument("--order", type=int, default=32)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--k", type=int, nargs="+", default=[32, 16])
    ap.add_argument("--period", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    args = ap.parse_args()
    import torch
    from workload import graphs, builder, patterns, cache
    from gcsa2_amd.binding import GCSA, KMER_COUNTS, Gcsa2Error, STATUS_BUFFER_TOO_SMALL
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

    def take(t, idx, chunk=1 << 24):
        """t[idx] along the first dimension, in chunks: one gather of 119 M two-column rows returned zeros for its last 2^26
        rows with the torch build this was measured with (gcsa2_find_batch on the windows sided with the library)."""
        return torch.cat([t.index_select(0, idx[a:a + chunk]) for a in range(0, idx.shape[0], chunk)] or [t[:0]])

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        out = fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), out

    print("| k | batch | hit_max, policy | windows | seeds | hits | kmer_hits_device | composition | composition / new | new within the composition's spread | "
          "M seeds/s | M hits/s | same |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    ok = True
    for k in args.k:
        per = L - k + 1
        nw = nr * per
        for name, reads in batches:
            flat, off = patterns.as_batch(reads)
            d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(8, dtype=np.uint8)])).to(dev)
            d_off = torch.from_numpy(off.view(np.int64)).to(dev)
            d_soff = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
            d_rng = torch.zeros((nw, 2), dtype=torch.int64, device=dev)
            d_cnt = torch.zeros(nw, dtype=torch.int64, device=dev)
            for hit_max, sample in ((0, False), (0, True), (8, False), (8, True)):
                # the sizes, from a refusal (not timed)
                try:
                    m, h = gpu.kmer_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, sample, 0, d_soff.data_ptr(), 0, 0,
                                                d_soff.data_ptr(), 0, 0, st)
                except Gcsa2Error as e:                                           # BUFFER_TOO_SMALL carries the sizes
                    if e.code != STATUS_BUFFER_TOO_SMALL:
                        raise
                    m, h = e.needed
                d_seeds = torch.zeros((max(m, 1), 5), dtype=torch.int64, device=dev)
                d_hoff = torch.zeros(m + 1, dtype=torch.int64, device=dev)
                d_hits = torch.zeros(max(h, 1), dtype=torch.int64, device=dev)
                d_foff = torch.zeros(m + 1, dtype=torch.int64, device=dev)        # the composition's class CSRs
                d_fval = torch.zeros(max(h, 1), dtype=torch.int64, device=dev)
                d_moff = torch.zeros(m + 1, dtype=torch.int64, device=dev)
                d_mval = torch.zeros(max(h, 1), dtype=torch.int64, device=dev)

                def new():
                    return gpu.kmer_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, hit_max, sample, 0, d_soff.data_ptr(),
                                                d_seeds.data_ptr(), m, d_hoff.data_ptr(), d_hits.data_ptr(), h, st)

                def composition():
                    gpu.kmer_windows_device(d_pat.data_ptr(), d_off.data_ptr(), nr, k, 1, KMER_COUNTS, 0, 0, d_rng.data_ptr(), d_cnt.data_ptr(), nw, st)
                    found = d_rng[:, 0] <= d_rng[:, 1]                            # both below 2^63; an empty range has sp = ep + 1
                    w = torch.nonzero(found).view(-1)
                    seeds = torch.cat([(w % per).unsqueeze(1), torch.full((w.shape[0], 1), k, dtype=torch.int64, device=dev),
                                       take(d_rng, w), take(d_cnt, w).unsqueeze(1)], dim=1)
                    soff = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
                    soff[1:] = torch.cumsum(found.view(nr, per).sum(1), 0)
                    full = (seeds[:, 4] <= hit_max) if hit_max else torch.ones(w.shape[0], dtype=torch.bool, device=dev)
                    sizes = torch.zeros(w.shape[0], dtype=torch.int64, device=dev)
                    parts = []
                    for mask, call, d_o, d_v in ((full, lambda r, n, o, v: gpu.locate_into(r, n, o, v, d_fval.shape[0], st), d_foff, d_fval),
                                                 (~full, lambda r, n, o, v: gpu.locate_max_into(r, n, hit_max, o, v, d_mval.shape[0], st), d_moff, d_mval)):
                        which = torch.nonzero(mask).view(-1)
                        n = int(which.shape[0])
                        if n == 0 or (mask is not full and not sample):
                            continue
                        ranges = take(seeds, which)[:, 2:4].contiguous()
                        total = call(ranges.data_ptr(), n, d_o.data_ptr(), d_v.data_ptr())
                        sizes[which] = d_o[1:n + 1] - d_o[:n]
                        parts.append((which, n, total, d_o, d_v))
                    hoff = torch.zeros(w.shape[0] + 1, dtype=torch.int64, device=dev)
                    hoff[1:] = torch.cumsum(sizes, 0)
                    hits = torch.empty(int(hoff[-1]), dtype=torch.int64, device=dev)
                    for which, n, total, d_o, d_v in parts:                        # every value to its seed's slot
                        shift = torch.repeat_interleave(take(hoff, which) - d_o[:n], d_o[1:n + 1] - d_o[:n])
                        hits[torch.arange(total, dtype=torch.int64, device=dev) + shift] = d_v[:total]
                    return soff, seeds, hoff, hits

                for _ in range(args.warmup):
                    new(), composition()
                torch.cuda.synchronize()
                t_new, t_old = [], []
                for _ in range(args.reps):                                        # the sides alternate
                    t_new.append(timed(new)[0])
                    t, want = timed(composition)
                    t_old.append(t)
                new()
                torch.cuda.synchronize()
                pairs = (("seed_offsets", d_soff, want[0]), ("seeds", d_seeds[:m], want[1]), ("hit_offsets", d_hoff, want[2]), ("hits", d_hits[:h], want[3]))
                differ = [label for label, x, y in pairs if x.shape != y.shape or not bool((x == y).all())]
                for label, x, y in pairs:
                    if label in differ and x.shape == y.shape:
                        at = int(torch.nonzero((x != y).view(x.shape[0], -1).any(1)).view(-1)[0])
                        print(f"# {label} differ first at {at}: {x[at].tolist()} against {y[at].tolist()}", flush=True)
                same = not differ
                ok = ok and same
                a, b = statistics.median(t_new), statistics.median(t_old)
                spread = max(t_old) - min(t_old)
                print(f"| {k} | {name} | {hit_max}, {'sample' if sample else 'skip'} | {nw} | {m} | {h} | {a:.3f} ms ({min(t_new):.3f}-{max(t_new):.3f}) | "
                      f"{b:.3f} ms ({min(t_old):.3f}-{max(t_old):.3f}) | {b / a:.2f}x | {'yes' if a <= b + spread else 'NO'} (spread {spread:.3f} ms) | "
                      f"{m / a / 1e3:.1f} | {h / a / 1e3:.1f} | {'yes' if same else 'NO'} |", flush=True)
                del d_seeds, d_hoff, d_hits, d_foff, d_fval, d_moff, d_mval, want, pairs
                torch.cuda.empty_cache()
            del d_pat, d_off, d_soff, d_rng, d_cnt
    gpu.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
