#!/usr/bin/env python3
"""Where the requests of the headline batch go, with and without the jump table of a find-only image: the headline's
index (workload/dbg_torch.py, junction edges) and walks, one find_stats_device call per image for the counters per query,
a few timed find_device launches, the image's bytes and the device memory left.  The images are created one after the
other in one process on the same index arrays; GCSA2_JUMP_BUILD is passed through to the second.

    python tests/perf/find_only_jump.py [--degree 34] [--queries 100000000] [--steps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree", type=int, default=34)
    ap.add_argument("--junctions", type=int, default=80)
    ap.add_argument("--queries", type=int, default=100_000_000)
    ap.add_argument("--pattern-len", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", choices=["both", "off", "on"], default="both")
    args = ap.parse_args()
    import torch
    from workload import dbg_torch
    from gcsa2_amd.binding import GCSA

    def log(msg):
        print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    dev = torch.device("cuda", 0)
    t = time.time()
    ix, dbg = dbg_torch.build_dbg(args.degree, junctions=args.junctions, device=dev, verbose=log)
    torch.cuda.empty_cache()
    log(f"index arrays: n = {ix.n}, e = {ix.e} ({time.time() - t:.1f} s)")
    nq, m = args.queries, args.pattern_len
    pats, _, expected = dbg_torch.walk_patterns_device(dbg, 0, nq, m, 0x6C5A0041)
    d_pat = torch.zeros(nq * m + 16, dtype=torch.uint8, device=dev)
    d_pat[: nq * m] = pats.reshape(-1)
    del pats
    d_off = torch.arange(nq + 1, dtype=torch.int64, device=dev) * m
    d_out = torch.zeros((nq, 2), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream()
    torch.cuda.empty_cache()
    res = {"path_nodes": int(ix.n), "edges": int(ix.e), "queries": nq, "pattern_len": m, "images": {}}
    for name, setting in (("off", "0"), ("on", None)):
        if args.only not in ("both", name):
            continue
        if setting is None:
            os.environ.pop("GCSA2_JUMP_TABLE", None)
        else:
            os.environ["GCSA2_JUMP_TABLE"] = setting
        free_before = torch.cuda.mem_get_info(dev)[0]
        t = time.time()
        gpu = GCSA(ix, device=0, with_samples=False, with_counters=False, with_lcp=False)
        create_s = time.time() - t
        free_after, total = torch.cuda.mem_get_info(dev)
        log(f"{name}: image {gpu.device_bytes() / 1e9:.2f} GB, jump table {gpu.jump_table_bytes() / 1e9:.2f} GB ({create_s:.1f} s)")

        def run():
            gpu.find_device(d_pat.data_ptr(), d_off.data_ptr(), nq, d_out.data_ptr(), st.cuda_stream)
        run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(args.steps):
            run()
        e1.record(st)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.steps
        exact = bool(torch.equal(d_out[:, 0], expected)) and bool(torch.equal(d_out[:, 1], expected))
        d_stats = torch.zeros(8, dtype=torch.int64, device=dev)
        d_out2 = torch.zeros_like(d_out)
        gpu.find_stats_device(d_pat.data_ptr(), d_off.data_ptr(), nq, d_out2.data_ptr(), d_stats.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        same = bool(torch.equal(d_out, d_out2))
        del d_out2
        blocks, steps, lookups, jumps, fetch_steps, second = (int(x) for x in d_stats.cpu()[:6])
        requests = blocks + lookups + jumps
        res["images"][name] = {
            "device_bytes": gpu.device_bytes(), "jump_table_bytes": gpu.jump_table_bytes(), "pair_block_bytes": gpu.pair_block_bytes(),
            "kmer_table_k": gpu.kmer_table_k(), "create_s": create_s, "device_total_bytes": total, "free_before_create": free_before,
            "free_after_create": free_after, "kernel_ms": ms, "queries_per_s": nq / (ms * 1e-3),
            "per_query": {"blocks": blocks / nq, "lf_steps": steps / nq, "seed_lookups": lookups / nq, "jumps": jumps / nq,
                          "fetch_steps": fetch_steps / nq, "second_fetches": second / nq, "requests": requests / nq},
            "requests_G_per_s": requests / (ms * 1e-3) / 1e9, "all_results_equal_closed_form": exact, "instrumented_twin_equal": same}
        gpu.close()
        del gpu
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
