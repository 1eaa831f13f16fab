#!/usr/bin/env python3
"""Stranded minimizer seeds (gcsa2_stranded_minimizer_hits_device, GCSA2_STRAND_BOTH) on the repeat graph against what a caller
ran for both strands before it: gcsa2_minimizer_hits_device on the batch plus the same call on its reverse complements, which
are already resident on the device (made with torch, not timed).  Also the canonical selection alone
(gcsa2_canonical_minimizers_device) and its share of the new call, and the time per searched window of both sides: the two
sides select different windows (canonical against plain minimizers on either strand).
`--reads` walks of `--read-length` bases; rows: (k, w) in --kw, hit_max = --hit-max, SKIP, each on two batches: the walks as
they are (every read is found as written and nothing on the other strand, so the second of the two calls ends its searches
early, whole wavefronts at a time), and the same walks with every second read reverse-complemented (what a sequencer gives:
either call then holds found and unfound reads side by side, as the groups of the new call do).

Device events around each side, warm-up runs first, then `--reps` timed runs a side, the sides alternating in one process.  All
run on buffers of the exact sizes (found out beforehand, not timed).  The verdict is the rule of profiles/jump_mid.md: every run
of the new call faster than every run of the two calls, and the medians at least twice the two calls' spread apart.

    python tests/perf/stranded_hits_bench.py [--log2-bases 23] [--order 32] [--reads 1000000] [--read-length 150] [--kw 16,11 16,5]
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
    ap.add_argument("--kw", nargs="+", default=["16,11", "16,5"])
    ap.add_argument("--hit-max", type=int, default=64)
    ap.add_argument("--hash-seed", type=int, default=0)
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
    print(f"image {gpu.device_bytes()} B, pair blocks {gpu.pair_block_bytes()} B, seed table k = {gpu.kmer_table_k()}", flush=True)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    nr, L, hit_max, seed = args.reads, args.read_length, args.hit_max, args.hash_seed
    reads = patterns.walk_patterns(g, nr, L, 0x6C5A0090)                          # (nr, L) bytes
    flat, off = patterns.as_batch(reads)
    d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(8, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    # the reverse complements, through the index's char2comp and its inverse; a byte without a code stays as it is
    c2c = np.asarray(ix.char2comp, dtype=np.int64)
    first = {}
    for byte in range(256):
        first.setdefault(int(c2c[byte]), byte)
    table = np.arange(256, dtype=np.uint8)
    for byte in range(256):
        if 1 <= c2c[byte] <= 4:
            table[byte] = first[5 - int(c2c[byte])]
    d_table = torch.from_numpy(table).to(dev)
    d_rc = torch.cat([d_table[d_pat[:nr * L].long()].reshape(nr, L).flip(1).reshape(-1), torch.zeros(8, dtype=torch.uint8, device=dev)])
    d_size = torch.zeros(2 * nr + 1, dtype=torch.int64, device=dev)
    as_written, mirrored = d_pat[:nr * L].reshape(nr, L), d_rc[:nr * L].reshape(nr, L)
    d_mix, d_mix_rc = as_written.clone(), mirrored.clone()
    d_mix[1::2], d_mix_rc[1::2] = mirrored[1::2], as_written[1::2]
    pad = torch.zeros(8, dtype=torch.uint8, device=dev)
    d_mix, d_mix_rc = torch.cat([d_mix.reshape(-1), pad]), torch.cat([d_mix_rc.reshape(-1), pad])
    batches = (("walks", d_pat, d_rc), ("every second read reversed", d_mix, d_mix_rc))
    torch.cuda.synchronize()

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

    def csr(groups, m, h):
        return (torch.zeros(groups + 1, dtype=torch.int64, device=dev), torch.zeros((max(m, 1), 5), dtype=torch.int64, device=dev),
                torch.zeros(m + 1, dtype=torch.int64, device=dev), torch.zeros(max(h, 1), dtype=torch.int64, device=dev))

    print("| batch | k | w | canonical minimizers | searched windows (new) | seeds (new) | hits (new) | canonical_minimizers_device | share of the new call | "
          "stranded_minimizer_hits_device, BOTH | searched windows (two calls) | seeds (two calls) | two minimizer_hits_device calls | two calls / new | "
          "ns per searched window, new | ns per searched window, two calls | new faster by the rule |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for kw, (batch, d_fwd, d_rev) in ((kw, b) for kw in args.kw for b in batches):
        k, w = (int(x) for x in kw.split(","))
        P, R, O = d_fwd.data_ptr(), d_rev.data_ptr(), d_off.data_ptr()
        S = d_size.data_ptr()
        total = sizes(lambda: gpu.canonical_minimizers_device(P, O, nr, k, w, seed, S, 0, 0, st))
        m, h = sizes(lambda: gpu.stranded_minimizer_hits_device(P, O, nr, k, w, seed, STRAND_BOTH, hit_max, False, 0, S, 0, 0, S, 0, 0, st))
        plain = [sizes(lambda: gpu.minimizers_device(x, O, nr, k, w, seed, S, 0, 0, st)) for x in (P, R)]
        mf, hf = sizes(lambda: gpu.minimizer_hits_device(P, O, nr, k, w, seed, hit_max, False, 0, S, 0, 0, S, 0, 0, st))
        mr, hr = sizes(lambda: gpu.minimizer_hits_device(R, O, nr, k, w, seed, hit_max, False, 0, S, 0, 0, S, 0, 0, st))
        d_moff = torch.zeros(nr + 1, dtype=torch.int64, device=dev)
        d_mins = torch.zeros((max(total, 1), 4), dtype=torch.int64, device=dev)
        new_out, fwd_out, rev_out = csr(2 * nr, m, h), csr(nr, mf, hf), csr(nr, mr, hr)

        def select():
            return gpu.canonical_minimizers_device(P, O, nr, k, w, seed, d_moff.data_ptr(), d_mins.data_ptr(), total, st)

        def new():
            a, b, c, d = new_out
            return gpu.stranded_minimizer_hits_device(P, O, nr, k, w, seed, STRAND_BOTH, hit_max, False, 0, a.data_ptr(), b.data_ptr(), m, c.data_ptr(),
                                                      d.data_ptr(), h, st)

        def old():
            a, b, c, d = fwd_out
            gpu.minimizer_hits_device(P, O, nr, k, w, seed, hit_max, False, 0, a.data_ptr(), b.data_ptr(), mf, c.data_ptr(), d.data_ptr(), hf, st)
            a, b, c, d = rev_out
            gpu.minimizer_hits_device(R, O, nr, k, w, seed, hit_max, False, 0, a.data_ptr(), b.data_ptr(), mr, c.data_ptr(), d.data_ptr(), hr, st)

        for _ in range(args.warmup):
            select(), new(), old()
        torch.cuda.synchronize()
        t_sel, t_new, t_old = [], [], []
        for _ in range(args.reps):                                                # the sides alternate
            t_sel.append(timed(select)[0])
            t_new.append(timed(new)[0])
            t_old.append(timed(old)[0])
        torch.cuda.synchronize()
        a, b, s = statistics.median(t_new), statistics.median(t_old), statistics.median(t_sel)
        clear = max(t_new) < min(t_old) and b - a >= 2 * (max(t_old) - min(t_old))
        print(f"| {batch} | {k} | {w} | {total} | {2 * total} | {m} | {h} | {row(t_sel)} | {s / a:.1%} | {row(t_new)} | {sum(plain)} | {mf + mr} | {row(t_old)} | "
              f"{b / a:.2f}x | {a * 1e6 / max(2 * total, 1):.2f} | {b * 1e6 / max(sum(plain), 1):.2f} | {'yes' if clear else 'NO'} |", flush=True)
        del d_moff, d_mins, new_out, fwd_out, rev_out
        torch.cuda.empty_cache()
    gpu.close()


if __name__ == "__main__":
    main()
