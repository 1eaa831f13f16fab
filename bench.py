#!/usr/bin/env python3
"""Benchmark of the GCSA2 query hot path on MI355X: batched k-mer find().

Default workload = BASELINE.json configs[3], the configuration the metric is
quoted on: a whole-human-pangenome-sized BRANCHING index -- 5 726 623 061 path nodes, e = 1.08 n, the
figures of the paper's whole-human index (paper.tex:380); order-17 de Bruijn graph of a degree-34 LFSR
cycle plus junction edges, every answer known in closed form (workload/dbg_torch.py) -- replicated on
every GPU, ONE batch of 100 M 32-mers sharded contiguously over the N ranks (strong scaling), hit ranges
gathered in the root's HBM by the library's single RCCL gather (gcsa2_comm_gather: grouped ncclSend /
ncclRecv over xGMI; u64 pairs on the wire, the path nodes do not fit 32 bits).  One step = one pass of the hot
path (gcsa2_find_device, kernel k_find2) over the rank's shard, inputs resident in HBM, + that gather.
Prints ONE JSON line on rank 0 (contract: task statement / DESIGN.md section 5).

A plain run does only what the headline needs: it builds the find() image, warms up, times the steps, writes --dump-outputs
and prints the line.  Everything else runs with `--full` only: the closed-form check of the ranges, the instrumented twin
behind `roofline` and the config's per-query figures, the request-rate ceiling, `cpu_baseline`, the device telemetry, the
host-batch and locate() legs, the secondaries below, the measured-traffic pass and, at N > 1, the gather timed alone.

With `--full` at N = 1 the same run also measures, as secondary objects of that line (never part of `value`):
  config5  BASELINE configs[4]: 1 M 256-bp patterns on the same index, half of them with a substitution
           every 41 bp: find() with parent() on failure (fused matching statistics), then locate()
  chr22    BASELINE configs[1] and [2]: 10 M 32-mer find() and locate() on the chr22-like SNP graph
  human32  rounds 1-2's headline for continuity: the 2^32 - 1 node index of the degree-32 m-sequence text

`--workload chr22 | linear` run those indexes as the primary workload (10 M queries per GPU, weak
scaling), for the profiles under profiles/.
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8 TB/s; ~6.3 TB/s achievable)
HBM_MEASURED_GBS = 6290.0
REQUEST_CEILING_GPS = 48.5       # dependent random 128-byte fetches/s at HBM footprints (gather_bench lds128, profiles/r01_gather_bench.md; r04: 48.47)
MEASURED_CEILING = None          # ... as measured on this box at the start of the run (N = 1, unless --no-extras)
LINEAR_SEED = 0x6C5A0040
HUMAN_PATTERN_SEED = 0x6C5A0041
CONFIG5_SEED = 0x6C5A0050


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=["pangenome", "pangenome_plain", "pangenome_snp", "human", "human_snp", "chr22", "repeats", "repeats30", "linear"], default="pangenome",
                    help="pangenome: whole-human-pangenome-sized branching index (5.73 G path nodes, e = 1.08 n), one batch sharded over "
                         "the GPUs (config 4); pangenome_plain / pangenome_snp: the same text without junction edges / with SNP bubbles "
                         "(6.9 G path nodes); human: rounds 1-2's 2^32 - 1 node index; human_snp: that text with SNP bubbles; "
                         "chr22: chr22-like SNP-bubble graph (config 2); linear: 2^30-base linear graph built on the GPU")
    ap.add_argument("--junctions", type=int, default=80, help="pangenome: junction edges, per mille of the candidates (80 -> e = 1.08 n)")
    ap.add_argument("--snp-period", type=int, default=50, help="human_snp: one SNP per this many positions")
    ap.add_argument("--degree", type=int, default=0, help="pangenome: degree of the LFSR (default 34: (2^34 - 1) / 3 path nodes); "
                                                            "human: degree of the m-sequence (default 32: 2^degree - 1 path nodes)")
    ap.add_argument("--log2-bases", type=int, default=0, help="chr22 / linear: backbone length (default 25 / 30)")
    ap.add_argument("--order", type=int, default=256)
    ap.add_argument("--queries", type=int, default=0,
                    help="human: patterns in the whole batch (default 100 M); chr22 / linear: patterns per GPU (default 10 M)")
    ap.add_argument("--pattern-len", type=int, default=32)
    ap.add_argument("--set", choices=["S", "U"], default="S", help="S: patterns that occur (full-depth matches); U: uniform random")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target CPU-baseline duration")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="N = 1: skip the config-5 and chr22 measurements")
    ap.add_argument("--no-extras", action="store_true", help="skip the request-rate ceiling, the device telemetry and the host-batch leg "
                                                               "(profiler passes: only the timed kernel and its instrumented twin run)")
    ap.add_argument("--secondary", choices=["all", "config5", "wide", "ladder", "chr22", "repeats", "repeats30", "human32", "human_snp"], default="all", help="N = 1: which secondary measurements to run")
    ap.add_argument("--pipeline-sweep", default="", help="diagnostic: lanes:chunk_log2[,...] -- the host-batch leg repeated per shape of the host pipeline (gcsa2_index_set_pipeline)")
    ap.add_argument("--locate-ranges", type=int, default=0, help="ranges of the locate() leg (default: 400 k on the repeat-rich indexes, every range on chr22)")
    ap.add_argument("--locate", action="store_true", help="--full, chr22 / repeats / repeats30: run the locate() leg even with --no-extras (profiler passes)")
    ap.add_argument("--variant", type=int, default=2, help="find launch shape (2 = one lane per query in batch order, 4 = queries ordered by length first)")
    ap.add_argument("--full-json", default="bench_full.json", help="where the full result object goes (every leg in full; the stdout line is the compact form)")
    ap.add_argument("--full-line", action="store_true", help="print the full object as the stdout line (profiles/; the driver needs the compact line)")
    ap.add_argument("--cache-dir", default=os.environ.get("GCSA2_CACHE", "/tmp/gcsa2_bench_cache"))
    ap.add_argument("--no-measured-traffic", action="store_true", help="N = 1: do not re-run the headline under rocprofv3 --pmc at the end (roofline.traffic stays the committed lookup)")
    ap.add_argument("--gather-only", action="store_true", help="N > 1: time the gather alone (no kernel, no packing) after the timed steps -- on by default; this flag skips the secondaries instead")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps, write the (sp, ep) ranges of the last step -- a fixed seeded "
                                                                      "sample of at most 2^21 queries -- to DIR/find_ranges.npy and the queries' ids to DIR/find_query_ids.npy (float64)")
    ap.add_argument("--full", action="store_true", help="run everything beyond the headline as well (module docstring); the options above that "
                                                         "select or skip legs apply within a --full run")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if not args.full:                       # a plain run: the headline alone, on the find()-only image
        args.no_cpu = args.no_secondary = args.no_extras = True
        args.locate = False
    return args


def free_port():
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def launch_ranks(args):
    """`python bench.py --gpus N` launched plainly (no RANK / WORLD_SIZE in the environment) measures N GPUs by itself:
    it runs `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <same arguments>` as a child process,
    one rank per GPU, rank 0 prints the line, and this process ends with the child's exit code.  Under a launcher it checks
    that the launcher's world is the one asked for.  Anything else -- fewer GPUs than ranks, a world that differs from --gpus -- ends with a non-zero exit code
    instead of a line that says n_gpus: 1 (VERDICT r03 / ADVICE r03)."""
    world_env = os.environ.get("WORLD_SIZE")
    backend = os.environ.get("GCSA2_BENCH_BACKEND", "nccl")
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be at least 1")
    if world_env is not None and "RANK" in os.environ:
        if int(world_env) != args.gpus:
            print(f"bench.py: launched with WORLD_SIZE={world_env} but --gpus {args.gpus}; refusing to report a line for "
                  f"a world that was not asked for", file=sys.stderr, flush=True)
            raise SystemExit(2)
        return
    if args.gpus == 1:
        return
    import torch
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if backend == "nccl" and have < args.gpus:
        print(f"bench.py: --gpus {args.gpus} but this host shows {have} GPU(s); refusing to measure fewer devices than "
              f"asked for", file=sys.stderr, flush=True)
        raise SystemExit(2)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    log("launching " + " ".join(cmd))
    sys.stdout.flush()
    sys.stderr.flush()
    # (a child, not an exec: this process has initialised the GPU runtime above)
    import subprocess
    rc = subprocess.call(cmd, env=dict(os.environ, GCSA2_BENCH_SELF_LAUNCHED="1"))
    raise SystemExit(rc if rc >= 0 else 128 - rc)


class Dist:
    """torch.distributed for the launch contract (rendezvous, barrier, max over ranks); the data-path gather
    is the library's own RCCL communicator (gcsa2_comm_*), created from an id broadcast through torch."""

    def __init__(self, dev):
        import torch.distributed as dist
        self.dist = dist
        self.active = "RANK" in os.environ and "WORLD_SIZE" in os.environ
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        # GCSA2_BENCH_BACKEND=gloo is a control-flow check for boxes with fewer GPUs than ranks (the gather
        # then goes through host memory and ranks may share a device); the measured configuration is nccl.
        self.backend = os.environ.get("GCSA2_BENCH_BACKEND", "nccl")
        self.comm = None
        self.dev = dev
        if self.active:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if self.backend == "nccl":
                dist.init_process_group(backend="nccl", device_id=dev)
            else:
                dist.init_process_group(backend=self.backend)

    def make_comm(self, binding, device_index):
        import torch
        if not self.active or os.environ.get("GCSA2_BENCH_NO_COMM"):    # the env knob tests the fallback
            return
        if self.backend != "nccl":
            # control-flow runs with ranks sharing a GPU (RCCL refuses that): the library's communicator over a gather through
            # host memory (gcsa2_comm_create_custom), so that everything above the transport is the C++ that runs under RCCL
            # (GCSA2_BENCH_TRANSPORT=blocking: the gather completes inside the call, as rounds 3-4 had it; the default only enqueues,
            # so that gather k really runs under kernel k + 1 and `gather_hidden_frac` means something on one GPU)
            from gcsa2_amd.host_transport import HostGather, AsyncHostGather
            kind = HostGather if os.environ.get("GCSA2_BENCH_TRANSPORT", "async") == "blocking" else AsyncHostGather
            self.transport = None
            try:
                self.transport = kind(self.dist, self.rank, self.world)
                self.comm = binding.Comm.custom(self.rank, self.world, device_index, self.transport)
            except Exception as e:
                print(f"[bench] rank {self.rank}: gcsa2_comm_create_custom failed ({e})", file=sys.stderr, flush=True)
            if not self.all_true(self.comm is not None):
                if self.comm is not None:
                    self.comm.close()
                self.comm = None
            return
        # Safety net: if the library's communicator cannot be created on some rank (RCCL not loadable there, ...), every
        # rank falls back to torch.distributed.gather for the data path and the line says so (config.parallelism).
        uid = torch.zeros(binding.Comm.ID_BYTES + 1, dtype=torch.uint8, device=self.dev)
        if self.rank == 0:
            try:
                uid[: binding.Comm.ID_BYTES].copy_(torch.frombuffer(bytearray(binding.Comm.unique_id()), dtype=torch.uint8))
                uid[binding.Comm.ID_BYTES] = 1
            except Exception as e:
                log(f"warning: gcsa2_comm_unique_id failed ({e}); using torch.distributed.gather")
        self.dist.broadcast(uid, 0)
        ok = bool(uid[binding.Comm.ID_BYTES].item())
        if ok:
            try:
                self.comm = binding.Comm(uid[: binding.Comm.ID_BYTES].cpu().numpy().tobytes(), self.rank, self.world, device_index)
            except Exception as e:
                print(f"[bench] rank {self.rank}: gcsa2_comm_create failed ({e})", file=sys.stderr, flush=True)
                ok = False
        if not self.all_true(ok):
            if self.comm is not None:
                self.comm.close()
            self.comm = None
            log("warning: the library communicator is not available on every rank; using torch.distributed.gather")

    def probe_comm(self):
        """The library's gather has never run with RCCL peers on the box this was built on (one GPU): before anything is timed,
        one small ragged gather of known bytes goes through it, and if any rank sees an error -- or the root wrong bytes --
        every rank drops the communicator together and the data path falls back (torch.distributed.gather under RCCL, host
        copies under gloo); the line's `config.parallelism` / `multi_gpu.gather` says which path ran."""
        if self.comm is None:
            return
        import torch
        counts = [(1 << 16) + 8 * r for r in range(self.world)]
        ok = True
        try:
            send = torch.full((counts[self.rank],), self.rank + 1, dtype=torch.uint8, device=self.dev)
            recv = torch.zeros(sum(counts), dtype=torch.uint8, device=self.dev) if self.rank == 0 else None
            stream = torch.cuda.current_stream()
            self.comm.gather(send.data_ptr(), counts, recv.data_ptr() if self.rank == 0 else 0, 0, stream.cuda_stream)
            torch.cuda.synchronize()
            if os.environ.get("GCSA2_BENCH_FAIL_PROBE") == str(self.rank):     # tests: the probe fails on one rank
                raise RuntimeError("GCSA2_BENCH_FAIL_PROBE")
            if self.rank == 0:
                expect = torch.cat([torch.full((c,), r + 1, dtype=torch.uint8) for r, c in enumerate(counts)])
                ok = bool(torch.equal(recv.cpu(), expect))
                if not ok:
                    log("warning: the probe gather through the library communicator delivered wrong bytes")
        except Exception as e:
            print(f"[bench] rank {self.rank}: probe gather failed ({e})", file=sys.stderr, flush=True)
            ok = False
        if not self.all_true(ok):
            self.comm.close()
            self.comm = None
            log("warning: the library communicator failed its probe gather; using the fallback data path")

    def barrier(self):
        if self.active:
            self.dist.barrier()

    def _reduce(self, value, op):
        import torch
        t = torch.tensor([value], dtype=torch.float64, device=self.dev if self.backend == "nccl" else "cpu")
        if self.active:
            self.dist.all_reduce(t, op=op)
        return float(t.item())

    def max(self, value):
        return self._reduce(value, self.dist.ReduceOp.MAX)

    def all_true(self, flag):
        return self._reduce(1.0 if flag else 0.0, self.dist.ReduceOp.MIN) > 0.5

    def close(self):
        if self.comm is not None:
            self.comm.close()
        if getattr(self, "transport", None) is not None and hasattr(self.transport, "close"):
            self.transport.close()
        if self.active:
            self.dist.destroy_process_group()


def shard_bounds(n_queries, world):
    from gcsa2_amd.shard import shard_bounds as sb
    return sb(n_queries, world)


def measured_request_ceiling():
    """Dependent random 128-byte fetches per second on THIS box (gather_bench's lds128 mode, the fetch pattern of k_find2, on a
    32 GB buffer): the ceiling the headline's request rate is held against.  Boxes differ by a few per cent; the constant of
    rounds 1-2 (50 G/s) was one box's figure.  Run before the index takes the memory.  None if the tool is missing."""
    import subprocess
    tool = os.path.join(ROOT, "gcsa2_amd", "lib", "gather_bench")
    if not os.path.exists(tool):
        return None
    try:
        out = subprocess.run([tool, "--mode", "lds128", "35"], capture_output=True, text=True, timeout=120)
        for line in out.stdout.splitlines():
            parts = line.split()
            if len(parts) >= 4 and parts[1] == "lds128":
                return float(parts[2])
    except (OSError, subprocess.SubprocessError, ValueError):
        pass
    return None


def device_telemetry(under_load):
    """Clocks, power and temperatures from rocm-smi while `under_load()` keeps the GPU busy (it enqueues ~1 s of the timed kernel
    and returns); explains box-to-box differences of the headline.  Whatever rocm-smi reports for device 0, verbatim."""
    import subprocess
    import torch
    info = {}
    try:
        under_load()
        out = subprocess.run(["rocm-smi", "-d", str(torch.cuda.current_device()), "--showclocks", "--showpower", "--showtemp", "--showperflevel",
                              "--json"], capture_output=True, text=True, timeout=60)
        torch.cuda.synchronize()
        try:
            data = json.loads(out.stdout)
            card = next(iter(data.values())) if isinstance(data, dict) and data else {}
            info = {k: v for k, v in card.items() if any(w in k.lower() for w in ("sclk", "mclk", "fclk", "socclk", "power", "temperature", "performance"))}
        except ValueError:
            info = {"raw": out.stdout[-600:]}
    except (OSError, subprocess.SubprocessError) as e:
        info = {"error": str(e)}
    torch.cuda.synchronize()
    return info


# ---- workloads -------------------------------------------------------------------------------------------

class Workload:
    """One rank's view: the index image on its GPU, its shard of the batch in HBM, and how to check results."""

    def __init__(self):
        self.label = ""
        self.scaling = "weak"
        self.gpu = None
        self.ix = None
        self.d_pat = None
        self.d_off = None
        self.nq = 0
        self.m = 0
        self.total_queries = 0
        self.first = 0                      # global id of the shard's first query
        self.verify = lambda d_ranges, first, count: None     # True / False / None (no closed form)


def padded_bytes(t):
    """Flat uint8 copy with 8 spare bytes (the find kernels read patterns as aligned 8-byte words)."""
    import torch
    flat = torch.zeros(t.numel() + 8, dtype=torch.uint8, device=t.device)
    flat[: t.numel()] = t.reshape(-1)
    return flat


def uniform_patterns_device(first, count, m, seed, dev):
    """Set U on the device: 2 bits per character from SplitMix64(seed), ceil(m / 32) words per query."""
    import torch
    from workload import mseq_torch
    words = (m + 31) // 32
    r = mseq_torch.splitmix64_range_torch(seed, first * words, count * words, dev).view(count, words)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    out = torch.empty((count, m), dtype=torch.uint8, device=dev)
    for i in range(m):
        out[:, i] = lut[(r[:, i // 32] >> (2 * (i % 32))) & 3]
    return out


def host_memory_ok(bytes_needed):
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) * 1024 >= bytes_needed
    except OSError:
        pass
    return True


def setup_human(args, D, dev, local_rank, branching=False, total_queries=None):
    """branching = False: the plain m-sequence text (every structure in closed form: find, locate, parent);
    branching = True: the same text with one SNP bubble per --snp-period positions (find(); at N = 1 also the LCP array
    of the node set, for the matching statistics of config 5)."""
    import torch
    from workload import mseq_torch
    from gcsa2_amd.binding import GCSA
    wl = Workload()
    wl.scaling = "strong"
    degree = args.degree or 32
    # every rank stages its own replica: ~12 bytes of host memory per path node while it does
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", D.world))
    available = sorted(d for d in mseq_torch.TAPS if d <= degree)
    if degree not in available:
        raise SystemExit(f"--degree must be one of {sorted(mseq_torch.TAPS)}")
    # (decided together: ranks that read /proc/meminfo at different moments must not end up with different indexes;
    # the staging copy of rounds 1-2 is gone, what a rank holds on the host now is the plain arrays: ~5 bytes per path node)
    while len(available) > 1 and available[-1] > 24 and not D.all_true(host_memory_ok(local_world * 5 * (1 << available[-1]))):
        available.pop()
    degree = available[-1]
    if degree != (args.degree or 32):
        log(f"warning: host memory too small for {local_world} replicas of degree {args.degree or 32}; using degree {degree}")
    full = (D.world == 1 and not args.no_secondary and not branching)
    t = time.time()
    alt_t = None
    if branching:
        with_lcp = (D.world == 1 and not args.no_secondary)      # N = 1: the matching-statistics leg needs the LCP array
        ix, sym_t, rank, alt_t = mseq_torch.build_mseq_snp(degree, period=args.snp_period, device=dev, verbose=log, with_lcp=with_lcp)
        torch.cuda.empty_cache()
    else:
        ix, sym_t, rank = mseq_torch.build_mseq(degree, device=dev, verbose=log, full=full)
    rank_t = torch.from_numpy(rank.view(np.int32)).to(dev)          # rank of every rotation: the closed-form answers
    del rank
    log(f"index arrays: n = {ix.n} ({time.time() - t:.1f} s)")
    t = time.time()
    wl.gpu = GCSA(ix, device=local_rank, with_samples=full, with_counters=full, with_lcp=(full or (branching and ix.lcp_size > 0)))
    log(f"device image: {wl.gpu.device_bytes() / 1e9:.2f} GB in HBM, seed table k = {wl.gpu.kmer_table_k()}, "
        f"pair blocks {wl.gpu.pair_block_bytes() / 1e9:.2f} GB ({time.time() - t:.1f} s)")
    wl.ix, wl.sym_t, wl.rank_t, wl.full, wl.degree, wl.alt_t = ix, sym_t, rank_t, full, degree, alt_t

    def long_patterns(first, count, m, seed):          # (patterns, start positions, closed-form node) for config 5
        if branching:
            pats, exp = mseq_torch.walk_patterns_device(sym_t, alt_t, rank_t, first, count, m, seed)
            return pats, None, exp
        pats, start = mseq_torch.substring_patterns_device(sym_t, first, count, m, seed)
        return pats, start, rank_t[start].to(torch.int64) & 0xFFFFFFFF
    wl.long_patterns = long_patterns
    wl.total_queries = total_queries or args.queries or 100_000_000
    wl.m = args.pattern_len
    b, e = shard_bounds(wl.total_queries, D.world)[D.rank]
    wl.first, wl.nq = b, e - b
    t = time.time()
    expected = None
    if args.set == "S" and branching:
        pats, expected = mseq_torch.walk_patterns_device(sym_t, alt_t, rank_t, b, e - b, wl.m, HUMAN_PATTERN_SEED)
    elif args.set == "S":
        pats, _ = mseq_torch.substring_patterns_device(sym_t, b, e - b, wl.m, HUMAN_PATTERN_SEED)
    else:
        pats = uniform_patterns_device(b, e - b, wl.m, HUMAN_PATTERN_SEED, dev)
    wl.d_pat = padded_bytes(pats)
    del pats
    wl.d_off = torch.arange(wl.nq + 1, dtype=torch.int64, device=dev) * wl.m
    log(f"patterns: shard [{b}, {e}) of {wl.total_queries} x {wl.m}, set {args.set} ({time.time() - t:.1f} s)")
    what = (f"degree-{degree} m-sequence text with one SNP bubble per {args.snp_period} positions: order-{degree // 2} de Bruijn graph, "
            f"{ix.n} path nodes, {ix.e} edges = {ix.e / ix.n:.3f} n" if branching else f"degree-{degree} m-sequence text, {ix.n} path nodes")
    wl.label = (f"whole-human-footprint index ({what}), one batch of "
                f"{wl.total_queries} x {wl.m}-mer find() sharded over {D.world} GPU(s), pattern set {args.set}"
                + (" (walks through the graph, alternative base taken at half of the SNP sites met)" if branching and args.set == "S" else ""))

    def verify(d_ranges, first, count):
        if args.set != "S" or wl.m < degree // 2:
            return None
        if branching:
            # find() of a walk = the single node of its first k characters (workload/mseq_torch.py); a shard other than
            # this rank's own is regenerated
            exp = expected if (first, count) == (b, e - b) else None
            ok = True
            step = 1 << 23
            for c in range(0, count, step):
                n = min(step, count - c)
                ex = exp[c:c + n] if exp is not None else mseq_torch.walk_patterns_device(sym_t, alt_t, rank_t, first + c, n, wl.m, HUMAN_PATTERN_SEED)[1]
                got = d_ranges[c:c + n]
                ok = ok and bool(torch.equal(got[:, 0], ex)) and bool(torch.equal(got[:, 1], ex))
            return ok
        # find(T[p .. p + m)) = (rank[p], rank[p]): every degree/2-mer occurs exactly once in the cyclic text
        ok = True
        chunk = 1 << 25
        for c in range(0, count, chunk):
            n = min(chunk, count - c)
            start = mseq_torch._lsr(mseq_torch.splitmix64_range_torch(HUMAN_PATTERN_SEED, first + c, n, dev), 11) % ix.n
            exp = rank_t[start].to(torch.int64) & 0xFFFFFFFF
            got = d_ranges[c:c + n]
            ok = ok and bool(torch.equal(got[:, 0], exp)) and bool(torch.equal(got[:, 1], exp))
        return ok
    wl.verify = verify
    return wl


def setup_pangenome(args, D, dev, local_rank, total_queries=None):
    """BASELINE configs[3] as SURVEY 8(d) wrote it: n = 5.73 G path nodes, e = 1.08 n (workload/dbg_torch.py).  The same
    index serves config 5 at N = 1 (samples, counters and LCP array in closed form)."""
    import torch
    from workload import dbg_torch, mseq_torch
    from gcsa2_amd.binding import GCSA
    wl = Workload()
    wl.scaling = "strong"
    degree = args.degree or 34
    if degree not in dbg_torch.LFSR:
        raise SystemExit(f"--degree must be one of {sorted(dbg_torch.LFSR)}")
    kind = {"pangenome": "junction", "pangenome_plain": "plain", "pangenome_snp": "snp"}[args.workload if args.workload.startswith("pangenome") else "pangenome"]
    # every rank holds the plain arrays of its own replica on the host (the image itself is built on the device): ~1 byte
    # per path node for find() alone (7 B_c + edges as bits), ~6 with samples (packed and plain), counters and LCP, ~8.5 at the peak of the generator; budgeted at 3 and 9
    # (config 5 runs sharded at N > 1, so every rank needs them)
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", D.world))
    # (both decisions are taken together: ranks that read /proc/meminfo at different moments must not disagree)
    full = (not args.no_secondary and kind != "snp" and args.secondary in ("all", "config5", "ladder")
            and (degree <= 20 or D.all_true(host_memory_ok(local_world * 9 * dbg_torch.text_length(degree)))))
    need = local_world * (9 if full else 3) * dbg_torch.text_length(degree) * (1.25 if kind == "snp" else 1.0)
    if degree > 20 and not D.all_true(host_memory_ok(need)):
        log(f"warning: host memory too small for {local_world} replicas of the degree-{degree} index ({need / 1e9:.0f} GB); "
            f"falling back to the 2^32 - 1 node index of rounds 1-2")
        args.degree = 0
        return setup_human(args, D, dev, local_rank, total_queries=total_queries)
    t = time.time()
    ix, dbg = dbg_torch.build_dbg(degree, period=(args.snp_period if kind == "snp" else 0),
                                  junctions=(args.junctions if kind == "junction" else 0), device=dev, verbose=log,
                                  full=full, with_lcp=(kind == "snp" and D.world == 1 and not args.no_secondary))
    torch.cuda.empty_cache()
    log(f"index arrays: n = {ix.n}, e = {ix.e} ({time.time() - t:.1f} s)")
    t = time.time()
    wl.gpu = GCSA(ix, device=local_rank, with_samples=full, with_counters=full, with_lcp=ix.lcp_size > 0)
    log(f"device image: {wl.gpu.device_bytes() / 1e9:.2f} GB in HBM, seed table k = {wl.gpu.kmer_table_k()}, "
        f"pair blocks {wl.gpu.pair_block_bytes() / 1e9:.2f} GB, locate table {wl.gpu.locate_table_bytes() / 1e9:.2f} GB ({time.time() - t:.1f} s)")
    wl.ix, wl.dbg, wl.full, wl.degree = ix, dbg, full, degree
    wl.total_queries = total_queries or args.queries or 100_000_000
    wl.m = args.pattern_len
    b, e = shard_bounds(wl.total_queries, D.world)[D.rank]
    wl.first, wl.nq = b, e - b
    t = time.time()
    expected = None
    short = args.set == "S" and wl.m < dbg.k          # prefixes of path labels: wide ranges, closed form = a rank interval
    if short:
        pats, exp_sp, exp_ep = dbg_torch.prefix_patterns_device(dbg, b, e - b, wl.m, HUMAN_PATTERN_SEED + 0x100 + wl.m)
    elif args.set == "S":
        pats, _, expected = dbg_torch.walk_patterns_device(dbg, b, e - b, wl.m, HUMAN_PATTERN_SEED)
    else:
        pats = uniform_patterns_device(b, e - b, wl.m, HUMAN_PATTERN_SEED, dev)
    wl.d_pat = padded_bytes(pats)
    del pats
    wl.d_off = torch.arange(wl.nq + 1, dtype=torch.int64, device=dev) * wl.m
    log(f"patterns: shard [{b}, {e}) of {wl.total_queries} x {wl.m}, set {args.set} ({time.time() - t:.1f} s)")
    graph = {"junction": f"+ junction edges between existing nodes ({args.junctions} per mille of the candidates)",
             "plain": "(no branching)", "snp": f"+ one SNP bubble per {args.snp_period} positions"}[kind]
    wl.label = (f"whole-human-pangenome-sized index: order-{degree // 2} de Bruijn graph of a degree-{degree} LFSR cycle of "
                f"{dbg.P} positions {graph}: {ix.n} path nodes, {ix.e} edges = {ix.e / ix.n:.3f} n; one batch of "
                f"{wl.total_queries} x {wl.m}-mer find() sharded over {D.world} GPU(s), pattern set {args.set}"
                + (" (walks through the graph)" if args.set == "S" else ""))

    def verify(d_ranges, first, count):
        # find() of a walk of >= k characters = the single node of its first k characters, in closed form (the bitmap
        # rank of that k-mer); a shard other than this rank's own is regenerated
        if short:
            if (first, count) == (b, e - b):
                sp_, ep_ = exp_sp, exp_ep
            else:
                _, sp_, ep_ = dbg_torch.prefix_patterns_device(dbg, first, count, wl.m, HUMAN_PATTERN_SEED + 0x100 + wl.m)
            return bool(torch.equal(d_ranges[:, 0], sp_)) and bool(torch.equal(d_ranges[:, 1], ep_))
        if args.set != "S":
            return None
        ok = True
        step = 1 << 23
        for c in range(0, count, step):
            n = min(step, count - c)
            ex = expected[c:c + n] if (first, count) == (b, e - b) else dbg_torch.walk_patterns_device(dbg, first + c, n, wl.m, HUMAN_PATTERN_SEED)[2]
            got = d_ranges[c:c + n]
            ok = ok and bool(torch.equal(got[:, 0], ex)) and bool(torch.equal(got[:, 1], ex))
        return ok
    wl.verify = verify
    wl.long_patterns = lambda first, count, m, seed: dbg_torch.walk_patterns_device(dbg, first, count, m, seed)
    return wl


def build_snp_index(args, log2_bases, rank, barrier):
    """Rank 0 builds the index once per node and caches it; the others load it."""
    from workload import graphs, builder, cache
    path = os.path.join(args.cache_dir, f"snp_{log2_bases}_{args.order}_v2.npz")
    t = time.time()
    graph = graphs.snp_graph(1 << log2_bases, 0x6C5A0010, 0x6C5A0011)
    log(f"graph: {graph.size} positions ({time.time() - t:.1f} s)")
    ix = None
    if rank == 0 and not os.path.exists(path):
        os.makedirs(args.cache_dir, exist_ok=True)
        t = time.time()
        ix = builder.build(graph, args.order, keep_table=False)
        log(f"index built: n={ix.n} e={ix.e} samples={ix.sample_count} ({time.time() - t:.1f} s)")
        cache.save(path + ".tmp.npz", ix)
        os.replace(path + ".tmp.npz", path)
    barrier()
    if ix is None:
        ix = cache.load(path)
    return ix, graph


def setup_chr22(args, D, dev, local_rank, nq=None):
    import torch
    from workload import patterns
    from gcsa2_amd.binding import GCSA
    wl = Workload()
    log2_bases = args.log2_bases or 25
    ix, graph = build_snp_index(args, log2_bases, D.rank, D.barrier)
    t = time.time()
    wl.gpu = GCSA(ix, device=local_rank)
    log(f"device image: {wl.gpu.device_bytes() / 1e6:.1f} MB in HBM ({time.time() - t:.1f} s)")
    wl.ix = ix
    wl.nq = nq or args.queries or 10_000_000
    wl.m = args.pattern_len
    wl.total_queries = wl.nq * D.world
    wl.first = wl.nq * D.rank
    seed = 0x6C5A0012 + 0x1000 * D.rank
    t = time.time()
    pats = patterns.walk_patterns(graph, wl.nq, wl.m, seed) if args.set == "S" else patterns.uniform_patterns(wl.nq, wl.m, seed)
    flat, off = patterns.as_batch(pats)
    wl.d_pat = padded_bytes(torch.from_numpy(flat).to(dev))
    wl.d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    log(f"patterns: {wl.nq} x {wl.m} set {args.set} ({time.time() - t:.1f} s)")
    wl.label = (f"chr22-like SNP graph 2^{log2_bases} bases, order-{args.order} GCSA, {wl.nq} x {wl.m}-mer find() per GPU, "
                f"pattern set {args.set}")
    return wl


def setup_linear(args, D, dev, local_rank):
    import torch
    from workload import linear_torch, patterns
    from gcsa2_amd.binding import GCSA
    wl = Workload()
    log2_bases = args.log2_bases or 30
    t = time.time()
    ix = linear_torch.build_linear(1 << log2_bases, LINEAR_SEED, order=args.order, with_lcp=False, with_samples=False, verbose=log)
    torch.cuda.empty_cache()
    log(f"linear index built on the GPU: n={ix.n} ({time.time() - t:.1f} s)")
    wl.gpu = GCSA(ix, device=local_rank, with_samples=False, with_counters=False, with_lcp=False)
    wl.ix = ix
    wl.nq = args.queries or 10_000_000
    wl.m = args.pattern_len
    wl.total_queries = wl.nq * D.world
    wl.first = wl.nq * D.rank
    seed = 0x6C5A0012 + 0x1000 * D.rank
    if args.set == "S":
        pats = linear_torch.substring_patterns_torch(1 << log2_bases, LINEAR_SEED, wl.nq, wl.m, seed, dev)
    else:
        pats = patterns.uniform_patterns(wl.nq, wl.m, seed)
    flat, off = patterns.as_batch(pats)
    wl.d_pat = padded_bytes(torch.from_numpy(flat).to(dev))
    wl.d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    wl.label = (f"linear graph 2^{log2_bases} bases (FM-index shaped GCSA, built on the GPU), {wl.nq} x {wl.m}-mer find() per GPU, "
                f"pattern set {args.set}")
    return wl


# ---- the timed loop ------------------------------------------------------------------------------------------

def gather_via_host(D, mine, shard_bytes):
    """gloo control-flow check only: torch's gather wants equal sizes, so pad to the largest shard."""
    import torch
    width = max(shard_bytes)
    padded = torch.zeros(width, dtype=torch.uint8)
    padded[: mine.numel()] = mine
    tmp = [torch.zeros(width, dtype=torch.uint8) for _ in shard_bytes] if D.rank == 0 else None
    D.dist.gather(padded, tmp, dst=0)
    if D.rank != 0:
        return None
    return torch.cat([tmp[r][:size] for r, size in enumerate(shard_bytes)])


def measure(args, D, dev, wl, steps, warmup):
    """Warm-up, then `steps` timed passes: find() over the shard (+ the RCCL gather of the ranges on rank 0 when
    distributed, overlapped with the next pass on a second stream).  Returns timings, the device result tensor and
    the algorithmic traffic of one launch."""
    import torch
    from gcsa2_amd import binding
    gpu, nq, m = wl.gpu, wl.nq, wl.m
    stream = torch.cuda.current_stream()
    comm_stream = torch.cuda.Stream(device=dev) if D.active else None
    nbuf = 2 if D.active else 1
    outs = [torch.zeros((nq, 2), dtype=torch.int64, device=dev) for _ in range(nbuf)]
    bounds = shard_bounds(wl.total_queries, D.world) if wl.scaling == "strong" else [(r * nq, (r + 1) * nq) for r in range(D.world)]
    counts = [e - b for b, e in bounds]
    total = sum(counts)
    # wire format (round 6): below 2^40 path nodes and edges six bytes per range -- sp in 40 bits, the length in one byte, the few
    # ranges of 255 and more path nodes in a fixed-capacity list behind the shard's ranges (gcsa2_pack_ranges48_device): 75 MB per
    # peer and step at N = 8 for the headline batch instead of the 125 MB of 40-bit pairs (10 bytes), which stay as the fallback
    # when a batch has more long ranges than the list holds; u64 pairs beyond 2^40.  GCSA2_BENCH_WIRE = 32 / 40 / 64 forces the
    # (sp, len) u32 pairs (indexes below 2^32), the 40-bit pairs or the u64 pairs (tests).
    top = max(int(wl.ix.n), int(wl.ix.e))
    wire_env = os.environ.get("GCSA2_BENCH_WIRE", "")
    pack48 = D.active and top < (1 << 40) and wire_env in ("", "48")
    pack32 = D.active and top < (1 << 32) and wire_env == "32"
    pack40 = D.active and not pack48 and not pack32 and top < (1 << 40) and wire_env != "64"
    packed = pack48 or pack32 or pack40
    wire_bytes = 6 if pack48 else (8 if pack32 else (10 if pack40 else 16))
    cap48 = [c // 64 + 64 for c in counts]                    # entries of a shard's overflow list
    shard_bytes = [binding.wire48_bytes(c, cap) for c, cap in zip(counts, cap48)] if pack48 else [c * wire_bytes for c in counts]
    shard_at = [sum(shard_bytes[:r]) for r in range(D.world)]
    wire = [torch.zeros(shard_bytes[D.rank] + 16, dtype=torch.uint8, device=dev) for _ in outs] if packed else outs
    root = D.active and D.rank == 0
    recv = [torch.zeros(sum(shard_bytes) + 16, dtype=torch.uint8, device=dev) for _ in outs] if root else [None] * nbuf
    gathered = torch.zeros((total, 2), dtype=torch.int64, device=dev) if (root and packed) else None
    overflow48 = torch.zeros(D.world, dtype=torch.int64, device=dev) if (root and pack48) else None      # long ranges per shard, as the root's unpack saw them
    free_ev = [None] * nbuf                  # the gather of the buffer's previous contents has completed
    # the root widens the gathered pairs on a THIRD stream: at N = 8 the unpack of 100 M pairs (0.45 ms) would otherwise sit
    # between two gathers on the gather stream, which is the slowest stage of the step (seven shards into the root)
    unpack_stream = torch.cuda.Stream(device=dev) if (root and packed) else None
    unpacked_ev = [None] * nbuf              # the unpack that read recv[b] has completed

    def gather_call(b):
        """The single collective of the path -- one gather of the shards' wire blocks into the root -- enqueued on the gather stream."""
        if D.comm is not None:               # the library's grouped send / recv over xGMI (or the host transport of the rehearsals)
            D.comm.gather(wire[b].data_ptr(), shard_bytes, recv[b].data_ptr() if root else 0, 0, comm_stream.cuda_stream)
        elif D.backend == "nccl":            # fallback (see Dist.make_comm): torch's RCCL gather, shards padded to one size
            with torch.cuda.stream(comm_stream):
                width = max(shard_bytes)
                mine = torch.zeros(width, dtype=torch.uint8, device=dev)
                mine[: shard_bytes[D.rank]] = wire[b].view(torch.uint8).reshape(-1)[: shard_bytes[D.rank]]
                parts = [torch.zeros(width, dtype=torch.uint8, device=dev) for _ in counts] if root else None
                D.dist.gather(mine, parts, dst=0)
                if root:
                    for p_, at, size in zip(parts, shard_at, shard_bytes):
                        recv[b][at: at + size] = p_[:size]
        else:                                # gloo control-flow check: through host memory
            comm_stream.synchronize()
            parts = gather_via_host(D, wire[b].view(torch.uint8).reshape(-1)[: shard_bytes[D.rank]].cpu(), shard_bytes)
            if root:
                with torch.cuda.stream(comm_stream):
                    recv[b][: sum(shard_bytes)].copy_(parts)

    def step(k, record=None):
        b = k % nbuf
        if free_ev[b] is not None:
            stream.wait_event(free_ev[b])
        if record is not None:
            record[0].record(stream)
        gpu.find_device_variant(args.variant, wl.d_pat.data_ptr(), wl.d_off.data_ptr(), nq, outs[b].data_ptr(), stream.cuda_stream)
        if record is not None:
            record[1].record(stream)
        if not D.active:
            return
        if pack48:
            binding.pack_ranges48_device(outs[b].data_ptr(), nq, wire[b].data_ptr(), cap48[D.rank], stream.cuda_stream)
        elif pack32:
            binding.pack_ranges32_device(outs[b].data_ptr(), nq, wire[b].data_ptr(), stream.cuda_stream)
        elif pack40:
            binding.pack_ranges40_device(outs[b].data_ptr(), nq, wire[b].data_ptr(), stream.cuda_stream)
        ready = torch.cuda.Event(enable_timing=record is not None)
        ready.record(stream)
        comm_stream.wait_event(ready)
        if record is not None:               # per-rank breakdown: pack = record[1]..record[2], gather (+ unpack) = record[3]..record[4]
            record[2] = ready
            record[3].record(comm_stream)
        if unpack_stream is not None and unpacked_ev[b] is not None:
            comm_stream.wait_event(unpacked_ev[b])                 # recv[b] is free again
        gather_call(b)
        last_stream = comm_stream
        if unpack_stream is not None:
            arrived = torch.cuda.Event()
            arrived.record(comm_stream)
            unpack_stream.wait_event(arrived)
            if pack48:                       # a block per shard: its ranges, then its list of long ranges
                for r_, (b0, _) in enumerate(bounds):
                    binding.unpack_ranges48_device(recv[b].data_ptr() + shard_at[r_], counts[r_], cap48[r_], gathered.data_ptr() + 16 * (b0 - bounds[0][0]),
                                                   overflow48.data_ptr() + 8 * r_, unpack_stream.cuda_stream)
            elif pack32:
                binding.unpack_ranges32_device(recv[b].data_ptr(), total, gathered.data_ptr(), unpack_stream.cuda_stream)
            else:
                binding.unpack_ranges40_device(recv[b].data_ptr(), total, gathered.data_ptr(), unpack_stream.cuda_stream)
            last_stream = unpack_stream
        done = record[4] if record is not None else torch.cuda.Event()
        done.record(last_stream)
        free_ev[b] = done
        if unpack_stream is not None:
            unpacked_ev[b] = done

    def drain():
        if comm_stream is not None:
            comm_stream.synchronize()
        if unpack_stream is not None:
            unpack_stream.synchronize()
        transport = getattr(D, "transport", None)
        if transport is not None and hasattr(transport, "check"):
            transport.check()                # (a host-memory transport whose helper thread failed says so here, not at the next call)

    for k in range(warmup):
        step(k)
    drain()
    if pack48:
        # did every shard's long ranges fit its list?  (The root's unpack reports the counts.)  If not, every rank switches to
        # the 40-bit pairs together and starts over: nothing of a truncated block is ever timed or verified.
        fits = True
        if root and warmup > 0:
            fits = all(int(n_long) <= cap for n_long, cap in zip(overflow48.cpu().tolist(), cap48))
        if not D.all_true(fits):
            log("the six-byte wire format's overflow lists are too short for this batch: falling back to 40-bit pairs")
            os.environ["GCSA2_BENCH_WIRE"] = "40"
            del wire, recv, gathered, outs
            return measure(args, D, dev, wl, steps, warmup)
    events = [[torch.cuda.Event(enable_timing=True) for _ in range(5)] for _ in range(steps)]
    D.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        step(k, events[k])
    drain()
    torch.cuda.synchronize()
    local_elapsed = time.perf_counter() - t0
    D.barrier()
    elapsed = D.max(time.perf_counter() - t0)
    last = (steps - 1) % nbuf if steps > 0 else 0
    d_out = outs[last]
    kernel_ms = float(np.mean([e[0].elapsed_time(e[1]) for e in events])) if steps > 0 else 0.0
    per_rank = None
    if D.active and steps > 0:
        # What each rank spent per step, on its own clock: the find kernel, the wire packing, the gather as its stream saw it
        # (on the root: receiving 7 shards + unpacking; on a peer: its send, which waits for the root to post the receive), and
        # from kernel start of step k to kernel start of step k + 1 (the pace the rank actually kept).  The gather of step k runs
        # on the second stream under the kernel of step k + 1: `gather_hidden_frac` = the share of gather time that did NOT
        # lengthen the step, 1 - (pace - kernel - pack) / gather.
        mine = dict(rank=D.rank, device=torch.cuda.current_device(), queries=nq,
                    kernel_ms=kernel_ms,
                    pack_ms=float(np.mean([e[1].elapsed_time(e[2]) for e in events])),
                    gather_ms=float(np.mean([e[3].elapsed_time(e[4]) for e in events])),
                    pace_ms=(float(np.mean([events[k][0].elapsed_time(events[k + 1][0]) for k in range(steps - 1)])) if steps > 1 else None),
                    wall_ms_per_step=local_elapsed / steps * 1e3)
        exposed = max(0.0, (mine["pace_ms"] if mine["pace_ms"] is not None else mine["wall_ms_per_step"]) - mine["kernel_ms"] - mine["pack_ms"])
        mine["gather_hidden_frac"] = max(0.0, min(1.0, 1.0 - exposed / mine["gather_ms"])) if mine["gather_ms"] > 0 else None
        mine["wire_bytes_sent"] = 0 if D.rank == 0 else shard_bytes[D.rank]
        transport = getattr(D, "transport", None)
        if transport is not None:            # (host-memory transports of the one-GPU rehearsals: how many gather calls returned before their bytes had moved)
            mine["transport_calls"] = transport.calls
            mine["transport_early_returns"] = getattr(transport, "early_returns", 0)
        mine["rccl_ranks"] = D.comm.rccl_ranks() if D.comm is not None else None
        # (what this rank computed in the last step, for the root to hold against what arrived: sums of sp and ep, mod 2^63)
        mine["shard_checksum"] = [int(d_out[:, 0].sum().item()), int(d_out[:, 1].sum().item())]
        everyone = [None] * D.world
        D.dist.all_gather_object(everyone, mine)
        per_rank = everyone
    gather_only = None
    if D.active and steps > 0 and args.full:
        # The gather ALONE -- no kernel, no packing, no unpack: the blocks of the last steps once more --, back to back on the gather
        # stream: what the root's links take in per second, next to `gather_hidden_frac` (VERDICT r05 #6 ii).  Every rank takes part.
        reps = max(steps, 4)
        g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        drain()
        D.barrier()
        torch.cuda.synchronize()
        t_g = time.perf_counter()
        g0.record(comm_stream)
        for k in range(reps):
            gather_call(k % nbuf)
        g1.record(comm_stream)
        comm_stream.synchronize()
        wall = D.max(time.perf_counter() - t_g)
        into_root = sum(shard_bytes[1:])
        gather_only = {"reps": reps, "ms_per_gather_root_stream": g0.elapsed_time(g1) / reps, "ms_per_gather_wall_max_over_ranks": wall / reps * 1e3,
                       "bytes_into_root_per_gather": into_root, "root_ingest_GBps": into_root / (wall / reps) / 1e9 if wall > 0 else None}
    result = dict(elapsed=elapsed, kernel_ms=kernel_ms, d_out=d_out, gathered=None, pack32=pack32, pack40=pack40, pack48=pack48, gather_only=gather_only,
                  gather=(("gcsa2_comm_gather (library RCCL communicator)" if D.backend == "nccl" else
                           "gcsa2_comm_gather over a host-memory transport (gcsa2_comm_create_custom; control-flow check; "
                           + ("blocking" if os.environ.get("GCSA2_BENCH_TRANSPORT", "async") == "blocking" else "asynchronous: enqueued on the gather stream") + ")") if D.comm is not None else
                          ("torch.distributed.gather (fallback)" if D.active and D.backend == "nccl" else
                           ("host copies (gloo control-flow check)" if D.active else "none (one GPU)"))))
    result["per_rank"] = per_rank
    result["wire_bytes_per_query"] = wire_bytes if D.active else None
    if root and steps > 0:
        result["gathered"] = gathered if packed else recv[last][: total * 16].view(torch.int64).view(total, 2)
        mine = result["gathered"][bounds[0][0]:bounds[0][1]]
        assert torch.equal(mine, d_out), "gathered shard differs from the computed ranges"
        for r, (b0, e0) in enumerate(bounds):                 # every other shard: the checksums its rank computed on its own GPU
            part = result["gathered"][b0:e0]
            got = [int(part[:, 0].sum().item()), int(part[:, 1].sum().item())]
            assert got == per_rank[r]["shard_checksum"], f"the shard gathered from rank {r} differs from what that rank computed"
        result["gathered_shards_verified"] = len(bounds)
    if not args.full:
        return result

    # algorithmic traffic of one launch (instrumented kernel, outside the timed region)
    d_stats = torch.zeros(8, dtype=torch.int64, device=dev)
    d_out2 = torch.zeros_like(d_out)
    # the twin also marks every block it fetches in a bitmap over the image's blocks (d_stats[7]): the distinct blocks are
    # the batch's working set -- what decides whether a leg is served by HBM or partly by L2 / the Infinity Cache
    n_blocks = int(wl.ix.sigma) * (int(wl.ix.n) // 384 + 1) + 16 * (int(wl.ix.n) // 192 + 1)
    d_touched = torch.zeros(n_blocks // 32 + 2, dtype=torch.int32, device=dev)
    d_stats[7] = d_touched.data_ptr()
    gpu.find_stats_device(wl.d_pat.data_ptr(), wl.d_off.data_ptr(), nq, d_out2.data_ptr(), d_stats.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(d_out, d_out2), "instrumented and timed kernels disagree"
    blocks, lf_steps, lookups, jumps, fetch_steps, second_fetches, wide_seeds, _ = (int(x) for x in d_stats.cpu())
    bits = torch.tensor([bin(b).count("1") for b in range(256)], dtype=torch.int64, device=dev)
    distinct_blocks = 0
    as_bytes = d_touched.view(torch.uint8)
    for a in range(0, as_bytes.shape[0], 1 << 26):
        distinct_blocks += int(bits[as_bytes[a: a + (1 << 26)].to(torch.int64)].sum().item())
    del d_touched, as_bytes
    result.update(blocks=blocks, lf_steps=lf_steps, lookups=lookups, jumps=jumps, fetch_steps=fetch_steps, second_fetches=second_fetches,
                  wide_seeds=wide_seeds, distinct_blocks=distinct_blocks,
                  algo_bytes=blocks * gpu.find_block_bytes() + lookups * 8 + jumps * 16 + nq * (m + 16),
                  found=int((d_out[:, 0] <= d_out[:, 1]).sum().item()))
    return result


DUMP_SEED = 0x6C5A0060
DUMP_MAX_QUERIES = 1 << 21          # 48 MB of float64: (sp, ep) and the query id


def dump_outputs(out_dir, d_ranges):
    """What the timed path hands its caller -- the (sp, ep) range of every query of the batch (on the root at N > 1: the gathered
    ranges) -- from the last timed step, as float64 (exact: every value is below 2^53).  A batch of more than DUMP_MAX_QUERIES
    queries is sampled: the same seeded choice of query ids for the same batch size, so two builds compare query for query."""
    import torch
    n = int(d_ranges.shape[0])
    if n > DUMP_MAX_QUERIES:
        ids = np.sort(np.random.default_rng(DUMP_SEED).choice(n, DUMP_MAX_QUERIES, replace=False))
    else:
        ids = np.arange(n)
    ranges = d_ranges[torch.from_numpy(ids).to(d_ranges.device)].cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "find_ranges.npy"), ranges.astype(np.float64))
    np.save(os.path.join(out_dir, "find_query_ids.npy"), ids.astype(np.float64))
    log(f"dumped the ranges of {len(ids)} of {n} queries to {out_dir}")


def timed_calls(call, warm=3, warm_seconds=0.5, timed=6):
    """Best wall-clock time of `timed` calls after at least `warm` untimed ones and `warm_seconds` of them.  The host legs need
    the warm-up: after a pause the first calls of a 10 M-pattern batch run 30-40 % below the steady state on these boxes (same
    shape of the pipeline, same arrays, same process: profiles/r04_host.md), and a caller that streams batches sees the steady
    state."""
    t_end = time.perf_counter() + warm_seconds
    done = 0
    while done < warm or time.perf_counter() < t_end:
        call()
        done += 1
    best = None
    for _ in range(timed):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def host_batch_rate(wl, d_out, nq=10_000_000, sweep=None, default_shape=(6, 18)):
    """The PCIe-inclusive rate (never `value`): the first `nq` patterns of the batch in host memory through gcsa2_find_batch
    -- chunked and double-buffered on several streams (csrc: find_pipelined) -- results back in host memory; checked against
    the device-resident run.  Twice: from pageable memory (the lanes copy through their pinned staging sets) and from
    page-locked memory (the copy engines read and write the caller's arrays in place)."""
    import torch
    nq = min(nq, wl.nq)
    m = wl.m
    want = d_out[:nq].cpu().numpy().view(np.uint64)

    def run(flat, offsets, got):
        wl.gpu.find_batch(flat[: 1_000_000 * m], offsets[:1_000_001])         # first call: the pipeline's pinned and device buffers
        got[:] = 1                                                             # touched: no page faults inside the timed calls
        best = timed_calls(lambda: wl.gpu.find_batch(flat, offsets, out=got))
        return best, bool(np.array_equal(got, want))

    flat = wl.d_pat[: nq * m].cpu().numpy().copy()
    offsets = np.arange(nq + 1, dtype=np.uint64) * np.uint64(m)
    best, same = run(flat, offsets, np.zeros((nq, 2), dtype=np.uint64))
    out = {"workload": f"{nq} x {m}-mers in pageable host memory -> gcsa2_find_batch -> ranges in host memory (best of 6 after half a second of untimed calls)",
           "value": nq / best, "unit": "queries/s", "ms": best * 1e3, "bytes_per_query_over_pcie": m + 8 + 16,
           "GB_per_s_end_to_end": nq * (m + 24) / best / 1e9, "equals_device_resident_run": same}
    try:
        p_flat = torch.empty(nq * m, dtype=torch.uint8).pin_memory()
        p_off = torch.empty(nq + 1, dtype=torch.int64).pin_memory()
        p_got = torch.empty((nq, 2), dtype=torch.int64).pin_memory()
        p_flat.numpy()[:] = flat
        p_off.numpy().view(np.uint64)[:] = offsets
        best, same = run(p_flat.numpy(), p_off.numpy().view(np.uint64), p_got.numpy().view(np.uint64))
        out["page_locked"] = {"workload": "the same batch with patterns, offsets and ranges in page-locked host memory (no staging copies)",
                              "value": nq / best, "unit": "queries/s", "ms": best * 1e3,
                              "GB_per_s_end_to_end": nq * (m + 24) / best / 1e9, "equals_device_resident_run": same}
    except Exception as e:           # the secondary never takes the line down
        out["page_locked"] = {"error": str(e)[:200]}
    # the same patterns handed over as 2-bit codes (gcsa2_find_batch_packed): 8 + 16 bytes per 32-mer over the link.  The
    # packing is the caller's (done here outside the timed calls, on the device, with the layout of include/gcsa2_hip.h).
    try:
        if m <= 32 and bool((wl.d_pat[: nq * m] != ord("N")).all()):
            lut = torch.full((256,), 0, dtype=torch.int64, device=wl.d_pat.device)
            for ch, c in zip(b"ACGT", range(4)):
                lut[ch] = c
            comps = lut[wl.d_pat[: nq * m].view(nq, m).to(torch.int64)]
            code = torch.zeros(nq, dtype=torch.int64, device=wl.d_pat.device)
            for t in range(m):                                       # distance t from the end -> bits [2t, 2t + 2)
                code |= comps[:, m - 1 - t] << (2 * t)
            codes = code.cpu().numpy().view(np.uint64).reshape(nq, 1).copy()
            del comps, code
            got = np.ones((nq, 2), dtype=np.uint64)
            wl.gpu.find_batch_packed(codes[:1_000_000], m)
            best = timed_calls(lambda: wl.gpu.find_batch_packed(codes, m, out=got))
            out["packed"] = {"workload": f"the same {nq} x {m}-mers as 2-bit codes (8 bytes each) in pageable host memory -> gcsa2_find_batch_packed "
                                         "-> ranges in host memory (best of 6 after half a second of untimed calls; packing not timed: the caller's)",
                             "value": nq / best, "unit": "queries/s", "ms": best * 1e3, "bytes_per_query_over_pcie": 8 + 16,
                             "GB_per_s_end_to_end": nq * 24 / best / 1e9, "equals_device_resident_run": bool(np.array_equal(got, want))}
            p_codes = torch.empty((nq, 1), dtype=torch.int64).pin_memory()
            p_got = torch.empty((nq, 2), dtype=torch.int64).pin_memory()
            p_codes.numpy().view(np.uint64)[:] = codes
            best = timed_calls(lambda: wl.gpu.find_batch_packed(p_codes.numpy().view(np.uint64), m, out=p_got.numpy().view(np.uint64)))
            out["packed"]["page_locked"] = {"value": nq / best, "unit": "queries/s", "ms": best * 1e3,
                                            "equals_device_resident_run": bool(np.array_equal(p_got.numpy().view(np.uint64), want))}
            if sweep:                    # diagnostic (--pipeline-sweep): the pipeline's shape on this host, one live image
                rows = []
                for lanes, chunk, *rest in sweep:
                    blocking = rest[0] if rest else 0
                    if lanes >= 0:                  # -1: the shape and the buffers stay as they are
                        wl.gpu.set_pipeline(lanes, chunk, blocking)
                    row = {"lanes": lanes, "chunk_log2": chunk, "blocking": blocking}
                    for name, call in (("packed", lambda: wl.gpu.find_batch_packed(codes, m, out=got)),
                                       ("packed_page_locked", lambda: wl.gpu.find_batch_packed(p_codes.numpy().view(np.uint64), m, out=p_got.numpy().view(np.uint64))),
                                       ("bytes", lambda: wl.gpu.find_batch(flat, offsets, out=got))):
                        call()
                        times = []
                        for _ in range(4):
                            t0 = time.perf_counter()
                            call()
                            times.append(time.perf_counter() - t0)
                        row[name + "_Gqps"] = round(nq / min(times) / 1e9, 3)
                        row[name + "_median_Gqps"] = round(nq / sorted(times)[len(times) // 2] / 1e9, 3)
                    row["same"] = bool(np.array_equal(got, want))
                    rows.append(row)
                    log(f"pipeline sweep: {row}")
                out["sweep"] = rows
                wl.gpu.set_pipeline(*default_shape, 0)
    except Exception as e:
        out["packed"] = {"error": str(e)[:200]}
    return out


def measure_locate(gpu, d_ranges, dev, steps):
    """Secondary figure (BASELINE configs[2]): locate() of the ranges the timed find() returned, into
    caller-owned device buffers (gcsa2_locate_into); reported beside the headline, never part of `value`."""
    import torch
    nq = int(d_ranges.shape[0])
    stream = torch.cuda.current_stream()
    d_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    d_val = torch.zeros(1, dtype=torch.int64, device=dev)
    try:
        total = gpu.locate_into(d_ranges.data_ptr(), nq, d_off.data_ptr(), d_val.data_ptr(), 1, stream.cuda_stream)
    except Exception as e:           # BUFFER_TOO_SMALL carries the size needed
        total = getattr(e, "needed", 0)
    d_val = torch.zeros(max(total, 1), dtype=torch.int64, device=dev)
    gpu.locate_into(d_ranges.data_ptr(), nq, d_off.data_ptr(), d_val.data_ptr(), d_val.shape[0], stream.cuda_stream)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        gpu.locate_into(d_ranges.data_ptr(), nq, d_off.data_ptr(), d_val.data_ptr(), d_val.shape[0], stream.cuda_stream)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    # size-independent check (the query_gcsa consistency test, benchmark/query_gcsa.cpp:160-179): per range,
    # the number of located values equals count()
    d_cnt = torch.zeros(nq, dtype=torch.int64, device=dev)
    gpu.count_device(d_ranges.data_ptr(), nq, d_cnt.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    consistent = bool(torch.equal(d_off[1:] - d_off[:-1], d_cnt)) and int(d_off[-1]) == int(total)
    out = {"count_equals_located": consistent,
           "workload": f"locate() of the {nq} ranges found above, sorted distinct values per range, results into caller-owned HBM buffers",
           "value": nq / (ms * 1e-3), "unit": "queries/s", "ms_per_step": ms, "values": int(total),
           "values_per_s": int(total) / (ms * 1e-3), "locate_table_bytes": gpu.locate_table_bytes()}
    out["roofline"] = locate_roofline(gpu, d_ranges, nq, int(total), ms)
    return out, d_off, d_val


def locate_roofline(gpu, d_ranges, nq, total, ms):
    """What locate() must move at least, against the call's whole duration on the stream (several kernels and, in the general
    pipeline, two host polls: `call_ms` is the caller's time, not a kernel time).  Path nodes = sum of the range widths; with the
    locate table every path node costs one 8-byte table entry -- a RANDOM 128-byte line when the range is one node, consecutive
    entries of a line when it is wide -- and every value 8 bytes out; ranges and offsets are streamed.  A batch of one-node
    ranges is a pure gather: its request rate against the box's ceiling is the figure of merit.  Wide ranges pay for
    removeDuplicates (sort + compaction), which no byte count of the INPUT bounds: their `frac` is reported, not argued."""
    import torch
    width = (d_ranges[:, 1] - d_ranges[:, 0] + 1).clamp(min=0)
    nodes = int(width.sum().item())
    singles = int((width == 1).sum().item())
    lines = singles + int(torch.div(width[width > 1] + 15, 16, rounding_mode="floor").sum().item())      # 16 entries per 128-byte line
    algo = 16 * nq + 8 * nodes + 8 * total + 8 * (nq + 1)
    limit = MEASURED_CEILING or REQUEST_CEILING_GPS
    rate = lines / (ms * 1e-3) / 1e9
    achieved = algo / (ms * 1e-3) / 1e9
    out = {"bound": "hbm", "kernel": "k_locate_single" if (singles == nq and total == nq and gpu.locate_table_bytes()) else "locate pipeline (walk / table, sorts, compaction)",
           "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": None,
           "algorithmic_bytes_per_call": algo, "call_ms": ms, "path_nodes": nodes, "one_node_ranges": singles,
           "request_rate": {"table_lines_per_call": lines, "achieved_G_per_s": rate, "ceiling_G_per_s": limit, "frac_of_ceiling": rate / limit}}
    seen = locate_traffic(nq, nodes, total)
    if seen:               # (reads by request size; writes as 64- and 32-byte requests, which the microarchitecture guide leaves uncalibrated)
        out["traffic"] = seen["read_bytes_per_call"] + seen["write_bytes_per_call"]
        out["traffic_read"], out["traffic_write"] = seen["read_bytes_per_call"], seen["write_bytes_per_call"]
        out["traffic_over_algorithmic"] = out["traffic"] / algo
        out["traffic_GBps"] = out["traffic"] / (ms * 1e-3) / 1e9
        out["traffic_source"] = seen.get("source")
    return out


def locate_traffic(nq, nodes, total):
    """Memory-side bytes of one locate() call from the committed counter passes of this exact batch (profiles/traffic.json,
    "locate": tools/pmc_locate.sh + tools/pmc_locate_summary.py); the batch is identified by its ranges, path nodes and values."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            return json.load(f).get("locate", {}).get(f"{nq}_{nodes}_{total}")
    except (OSError, ValueError):
        return None


def pmc_traffic(args, key, gpu, nq, m):
    """Memory-side read bytes of one launch from the committed rocprofv3 --pmc pass of this exact
    workload (profiles/traffic.json).  PMC counters cannot be read from inside the timed process, so this is
    looked up, never estimated: any mismatch in workload, batch shape, seed table or kernel yields None."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            entry = json.load(f).get(key)
    except (OSError, ValueError):
        return None
    if not entry or args.variant != 2 or entry["queries"] != nq or entry["pattern_len"] != m:
        return None
    if entry.get("kmer_table_k") != gpu.kmer_table_k() or entry.get("pair_blocks") != bool(gpu.pair_block_bytes()):
        return None
    return entry["read_bytes_per_launch"]


TIMED_FIND = re.compile(r"k_find2<false, false, (true|false)(, (true|false))?>")


def measured_traffic(args, nq):
    """Memory-side read bytes of ONE launch of the timed find kernel, MEASURED: this command's headline again (index, batch, two
    launches; no secondaries) as a child process under `rocprofv3 --pmc TCC_EA0_RDREQ_{32B,64B,128B}_sum` -- counters cannot be
    read from inside the timed process, and a counter pass slows the kernel, so it runs after every leg, when this process has
    given its image back.  128 x RDREQ_128B + 64 x RDREQ_64B + 32 x RDREQ_32B per dispatch (MI355X_MICROARCH.md, HBM section),
    mean over the dispatches of the timed instantiation.  None when there is no profiler or the pass fails (the line then keeps
    the committed lookup and says so)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if prof is None:
        return None
    out_dir = tempfile.mkdtemp(prefix="gcsa2_pmc_", dir="/tmp")
    cmd = [prof, "--kernel-include-regex", "k_find2", "--pmc", "TCC_EA0_RDREQ_32B_sum", "TCC_EA0_RDREQ_64B_sum", "TCC_EA0_RDREQ_128B_sum",
           "--output-format", "csv", "-d", out_dir, "-o", "x", "--",
           sys.executable, os.path.abspath(__file__), "--full", "--workload", args.workload, "--steps", "2", "--warmup", "1", "--no-cpu", "--no-secondary",
           "--no-extras", "--full-json", "", "--set", args.set, "--pattern-len", str(args.pattern_len), "--variant", str(args.variant),
           "--junctions", str(args.junctions), "--snp-period", str(args.snp_period), "--order", str(args.order), "--cache-dir", args.cache_dir]
    for flag, value in (("--degree", args.degree), ("--log2-bases", args.log2_bases), ("--queries", args.queries)):
        if value:
            cmd += [flag, str(value)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "GCSA2_BENCH_SELF_LAUNCHED", "GCSA2_BENCH_FAIL_LEG")}
    env["TMPDIR"] = "/tmp"
    try:
        done = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=float(os.environ.get("GCSA2_BENCH_PMC_TIMEOUT", "600")))
        per = {}
        for path in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if TIMED_FIND.search(row["Kernel_Name"]):
                        per.setdefault(row["Dispatch_Id"], {}).setdefault(row["Counter_Name"], 0.0)
                        per[row["Dispatch_Id"]][row["Counter_Name"]] += float(row["Counter_Value"])
        if not per:
            log(f"measured traffic: no counters of the timed kernel in {out_dir} (rocprofv3 rc {done.returncode}): {done.stderr.decode(errors='replace')[-400:]}")
            return None
        launches = [128 * c.get("TCC_EA0_RDREQ_128B_sum", 0) + 64 * c.get("TCC_EA0_RDREQ_64B_sum", 0) + 32 * c.get("TCC_EA0_RDREQ_32B_sum", 0) for c in per.values()]
        child = None
        for text in reversed(done.stdout.decode(errors="replace").strip().splitlines()):
            if text.startswith("{"):
                child = json.loads(text)
                break
        if child is None or child.get("config", {}).get("queries_per_gpu") != nq:
            log("measured traffic: the child's line is missing or describes another batch")
            return None
        return {"read_bytes_per_launch": sum(launches) / len(launches), "launches": len(launches),
                "requests_128B_per_launch": sum(c.get("TCC_EA0_RDREQ_128B_sum", 0) for c in per.values()) / len(per),
                "kernel_ms_under_counters": child["roofline"]["kernel_ms"]}
    except (subprocess.TimeoutExpired, OSError, ValueError, KeyError) as e:
        log(f"measured traffic: {type(e).__name__}: {e}")
        return None
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def apply_measured_traffic(result, seen):
    """The headline's roofline object with the bytes of this run's own counter pass (the committed lookup stays beside them)."""
    rf = result["roofline"]
    rf["traffic_lookup"] = rf.get("traffic")
    rf["traffic"] = seen["read_bytes_per_launch"]
    rf["traffic_source"] = "measured"
    rf["traffic_source_note"] = (f"this run: the headline again as a child process under rocprofv3 --pmc TCC_EA0_RDREQ_*_sum after the legs, mean of "
                                 f"{seen['launches']} launches of the timed kernel ({seen['kernel_ms_under_counters']:.3f} ms under the counters); "
                                 "128 B x RDREQ_128B + 64 B x RDREQ_64B + 32 B x RDREQ_32B")
    rf["traffic_over_algorithmic"] = rf["traffic"] / rf["algorithmic_bytes_per_launch"]
    rf["traffic_GBps"] = rf["traffic"] / (rf["kernel_ms"] * 1e-3) / 1e9
    rf["traffic_frac_of_measured_hbm_rate"] = rf["traffic_GBps"] / HBM_MEASURED_GBS
    rf["request_rate"]["memory_requests_per_query"] = seen["requests_128B_per_launch"] / result["config"]["queries_per_gpu"]
    return {"read_bytes_per_launch": seen["read_bytes_per_launch"], "launches": seen["launches"], "lookup_read_bytes_per_launch": rf["traffic_lookup"]}


def working_set(gpu, r, nq):
    """Bytes a launch gathers from: the DISTINCT blocks it fetched (the instrumented twin's bitmap) and the lines of the seed
    table its lookups fall into (expected number for uniformly spread indices: L (1 - exp(-lookups / L)) of L lines of 16 entries)."""
    k = gpu.kmer_table_k()
    lines = float(1 << (2 * k)) / 16.0 if k else 0.0
    seed_lines = lines * (1.0 - float(np.exp(-r["lookups"] / lines))) if lines >= 1.0 and r["lookups"] else 0.0
    return int(r["distinct_blocks"] * gpu.find_block_bytes() + seed_lines * 128)


CACHE_BYTES = 256 << 20          # Infinity Cache (MALL) of an MI355X; the eight L2s add 32 MB


def roofline(args, r, wl, key, ceiling=None):
    gpu, nq, m = wl.gpu, wl.nq, wl.m
    achieved = r["algo_bytes"] / (r["kernel_ms"] * 1e-3) / 1e9
    traffic = pmc_traffic(args, key, gpu, nq, m)
    ws = working_set(gpu, r, nq)
    requests = r["blocks"] + r["lookups"] + r["jumps"]
    req_rate = requests / (r["kernel_ms"] * 1e-3) / 1e9
    limit = ceiling or MEASURED_CEILING or REQUEST_CEILING_GPS
    # Who serves the launch.  A batch whose working set is many times the on-die caches AND whose request rate stays below what
    # HBM delivers for dependent random 128-byte fetches (gather_bench) is served by HBM: `frac` is then an HBM fraction.
    # Anything else -- a working set within a few multiples of the Infinity Cache, a request rate above the HBM ceiling (ranges
    # that share their upper levels: the same blocks again and again), memory-side traffic (PMC pass) below the algorithmic
    # bytes -- is served partly on-die, and `achieved` / `frac` are ALGORITHMIC rates, not memory-side ones.
    reuse = requests / max(1.0, ws / 128.0)          # (information: requests per distinct line; a 60 GB working set touched twice by
    #                                                    # different queries at random times is still served by HBM)
    # (the ceiling is this box's probe of a few seconds before the index was loaded: 47.1 - 48.6 G/s over the round's boxes and
    # +-2 % from probe to probe, so a rate within 3 % above it is the ceiling, not evidence of on-die service)
    on_die = ws < 8 * CACHE_BYTES or req_rate > 1.03 * limit or achieved > HBM_PEAK_GBS or (traffic is not None and traffic < 0.9 * r["algo_bytes"])
    out = {"bound": "hbm", "kernel": "k_find2<pair>" if gpu.pair_block_bytes() else "k_find2",
           "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
           "algorithmic_bytes_per_launch": r["algo_bytes"], "kernel_ms": r["kernel_ms"], "working_set_bytes": ws,
           "requests_per_distinct_line": reuse,
           "served": "L2 / Infinity Cache (partly)" if on_die else "HBM",
           "working_set_note": ("distinct blocks fetched (bitmap of the instrumented twin) + seed-table lines: "
                                + ("partly served on-die, `achieved` and `frac` are algorithmic rates, not HBM fractions" if on_die
                                   else "far beyond the 256 MiB Infinity Cache, one request per line: served by HBM"))}
    # what bounds a random-gather kernel beyond L2 is requests per second (profiles/r01_gather_bench.md:
    # ~50 G dependent random 128-byte fetches/s at HBM footprints); reported beside the byte roofline
    # (on a partly cached launch the fraction may exceed 1: it is then part of the evidence for the label, not an HBM figure)
    out["request_rate"] = {"achieved_G_per_s": req_rate, "ceiling_G_per_s": limit, "requests_per_query": requests / nq, "frac_of_ceiling": req_rate / limit}
    if traffic is not None:
        out["traffic_source"] = "lookup"               # ("measured" once this run's own counter pass has replaced it: apply_measured_traffic)
        out["traffic_source_note"] = ("profiles/traffic.json (the committed rocprofv3 --pmc TCC_EA0_RDREQ_*_sum pass of this workload; "
                                      "128 B x RDREQ_128B + 64 B x RDREQ_64B + 32 B x RDREQ_32B)")
        out["traffic_over_algorithmic"] = traffic / r["algo_bytes"]
        out["traffic_GBps"] = traffic / (r["kernel_ms"] * 1e-3) / 1e9
        # the guide's measured streaming rate (MI355X_MICROARCH.md: 6.29 TB/s float4 copy = 79 % of the 8 TB/s spec): how close the
        # launch's memory-side traffic is to what HBM delivers at all
        out["traffic_frac_of_measured_hbm_rate"] = out["traffic_GBps"] / HBM_MEASURED_GBS
    return out


def find_config(wl, r, world):
    gpu = wl.gpu
    cfg = {"workload": wl.label, "path_nodes": int(wl.ix.n), "edges": int(wl.ix.e), "queries_total": wl.total_queries,
           "queries_per_gpu": wl.nq, "pattern_len": wl.m, "index_bytes_hbm": gpu.device_bytes(),
           "pair_block_bytes": gpu.pair_block_bytes(), "single_block_bytes": int(wl.ix.sigma) * (int(wl.ix.n) // 384 + 1) * 128,
           "kmer_table_k": gpu.kmer_table_k(), "block_bytes": gpu.find_block_bytes(),
           "parallelism": f"replicated index, contiguous query shards x{world}, one gather of ranges per step: {r['gather']}"
                          + (" as 40-bit sp + length byte, 6 bytes (+ a list of the long ranges)" if r.get("pack48") else
                             (" as (sp, len) u32 pairs" if r["pack32"] else (" as (sp, len) 40-bit pairs, 10 bytes" if r.get("pack40") else "")))}
    if "blocks" in r:                       # the instrumented twin ran (--full)
        cfg.update({"found": r["found"], "lf_steps_per_query": r["lf_steps"] / wl.nq,
                    "second_fetch_fraction_of_steps": r["second_fetches"] / max(r["fetch_steps"], 1), "wide_seed_entries_hit": r["wide_seeds"],
                    "blocks_per_query": r["blocks"] / wl.nq})
    return cfg


# ---- N = 1 secondaries ---------------------------------------------------------------------------------------

def config5(args, wl, dev):
    """BASELINE configs[4] on one GPU: 1 M 256-bp walks through the index of the headline, every second one with a
    substitution every 41 bp.  Backward search with parent() on failure (k_match_stats2: LF + LCPArray::parent fused, the
    MEM-finder interplay of SURVEY.md 8(f)-2), plain find(), then -- when the index carries samples -- locate() and
    parent() of the final ranges.  Closed forms for the unmodified half, the CPU oracle on a sample of everything."""
    import torch
    from workload import mseq_torch
    gpu, ix = wl.gpu, wl.ix
    nq, m = 1_000_000, 256
    stream = torch.cuda.current_stream()
    pats, start, expected = wl.long_patterns(0, nq, m, CONFIG5_SEED)
    nxt = torch.zeros(256, dtype=torch.uint8, device=dev)
    for a, b in zip(b"ACGT", b"CGTA"):
        nxt[a] = b
    for col in range(37, m, 41):
        pats[1::2, col] = nxt[pats[1::2, col].to(torch.int64)]
    d_pat = padded_bytes(pats)
    del pats
    d_off = torch.arange(nq + 1, dtype=torch.int64, device=dev) * m
    d_ms = torch.zeros(nq * m + 8, dtype=torch.int16, device=dev)
    d_rng = torch.zeros((nq, 2), dtype=torch.int64, device=dev)
    d_fb = torch.zeros(nq, dtype=torch.int64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 5

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    ms_time = timed(lambda: gpu.match_stats_device(d_pat.data_ptr(), d_off.data_ptr(), nq, d_ms.data_ptr(), d_rng.data_ptr(),
                                                   d_fb.data_ptr(), stream.cuda_stream, total_bytes=nq * m))
    # closed form for the unmodified half: the walk matches to full depth, so no parent() call, the match starting at
    # byte i has length 256 - i, and the final range is the single node of the walk's first k characters
    exp = expected[0::2]
    ms2d = d_ms[: nq * m].view(nq, m)
    want_ms = (m - torch.arange(m, device=dev)).to(torch.int16).view(1, m)
    exact_ok = bool(torch.equal(d_rng[0::2, 0], exp)) and bool(torch.equal(d_rng[0::2, 1], exp)) and \
        bool((d_fb[0::2] == 0).all()) and bool((ms2d[0::2] == want_ms).all())
    out = {"workload": f"{nq} x {m}-bp walks through the same index, every second one with a substitution every 41 bp: "
                       "backward search with parent() on failure (k_match_stats2), find(), then locate() and parent() of the final ranges",
           "path_nodes": int(ix.n), "edges": int(ix.e),
           "match_stats_ms": ms_time, "patterns_per_s": nq / (ms_time * 1e-3), "bases_per_s": nq * m / (ms_time * 1e-3),
           "parent_calls_per_pattern": float(d_fb.to(torch.float64).mean().item()),
           "unmodified_half_equals_closed_form": exact_ok}
    try:
        out["roofline"] = match_stats_roofline(gpu, d_pat, d_off, nq, m, d_ms, d_rng, d_fb, ms_time, dev, records=None)
    except Exception as e:               # (the twin needs the pair blocks: absent on an image made under a tight memory budget)
        out["roofline"] = {"error": str(e)[:200]}
    out["match_breaks"] = match_breaks_leg(gpu, d_pat, d_off, nq, m, d_ms, d_rng, d_fb, exp, timed, dev)
    if "error" not in out["roofline"]:
        mb = out["match_breaks"]
        mb["roofline"] = match_stats_roofline(gpu, d_pat, d_off, nq, m, d_ms, d_rng, d_fb, mb["ms"], dev, records=mb["records"], events=out["roofline"]["events"])
    # plain find() of the same batch (a substituted pattern usually empties at its first substitution)
    d_find = torch.zeros((nq, 2), dtype=torch.int64, device=dev)
    out["find_ms"] = timed(lambda: gpu.find_device(d_pat.data_ptr(), d_off.data_ptr(), nq, d_find.data_ptr(), stream.cuda_stream))
    out["find_patterns_per_s"] = nq / (out["find_ms"] * 1e-3)
    out["find_unmodified_half_equals_closed_form"] = bool(torch.equal(d_find[0::2, 0], exp)) and bool(torch.equal(d_find[0::2, 1], exp))
    if gpu.sampleCount() > 0:
        loc, d_loff, d_lval = measure_locate(gpu, d_rng, dev, 3)
        out["locate"] = loc
        if start is not None:
            vals = mseq_torch.node_values(start[0::2].cpu().numpy())
            out["locate_unmodified_half_equals_closed_form"] = bool(np.array_equal(d_lval[d_loff[:-1][0::2]].cpu().numpy().view(np.uint64), vals))
    d_nodes = torch.zeros((nq, 5), dtype=torch.int64, device=dev)
    t_parent = timed(lambda: gpu.parent_device(d_rng.data_ptr(), nq, d_nodes.data_ptr(), stream.cuda_stream))
    out["parent_queries_per_s"] = nq / (t_parent * 1e-3)
    if not args.no_cpu:
        out["cpu_baseline"] = cpu_baseline_match_stats(ix, d_pat, d_ms, d_rng, d_fb, m)
    if "error" not in out.get("roofline", {}):
        del d_ms, d_find, d_nodes
        torch.cuda.empty_cache()
        out["four_times_the_batch"] = config5_large_batch(wl, dev, nxt, out["roofline"], 4 * nq, m)
    return out


def config5_large_batch(wl, dev, nxt, small_roofline, nq, m):
    """The same workload with FOUR times the patterns (4 M x 256 bp, dense statistics only): the persistent lanes of the kernel hold
    262 144 patterns at a time, so a batch of 1 M is four patterns per lane and its last patterns -- a pattern with mismatches
    takes a fifth of the whole launch -- drain a machine that has nothing else to run; at 4 M the drain is a twentieth.  The
    steady-state rate, with the requests per pattern of the 1 M batch's instrumented twin against the request ceiling."""
    import torch
    gpu = wl.gpu
    stream = torch.cuda.current_stream()
    pats, _, expected = wl.long_patterns(0, nq, m, CONFIG5_SEED + 1)
    for col in range(37, m, 41):
        pats[1::2, col] = nxt[pats[1::2, col].to(torch.int64)]
    d_pat = padded_bytes(pats)
    del pats
    d_off = torch.arange(nq + 1, dtype=torch.int64, device=dev) * m
    d_ms = torch.zeros(nq * m + 8, dtype=torch.int16, device=dev)
    d_rng = torch.zeros((nq, 2), dtype=torch.int64, device=dev)
    d_fb = torch.zeros(nq, dtype=torch.int64, device=dev)
    run = lambda: gpu.match_stats_device(d_pat.data_ptr(), d_off.data_ptr(), nq, d_ms.data_ptr(), d_rng.data_ptr(), d_fb.data_ptr(), stream.cuda_stream, total_bytes=nq * m)
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(3):
        run()
    e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 3
    exp = expected[0::2]
    want_ms = (m - torch.arange(m, device=dev)).to(torch.int16).view(1, m)
    ok = bool(torch.equal(d_rng[0::2, 0], exp)) and bool(torch.equal(d_rng[0::2, 1], exp)) and bool((d_fb[0::2] == 0).all()) and \
        bool((d_ms[: nq * m].view(nq, m)[0:200_000:2] == want_ms).all())
    per_pattern = small_roofline["requests_per_pattern"]
    rate = per_pattern * nq / (ms * 1e-3) / 1e9
    limit = small_roofline["request_rate"]["ceiling_G_per_s"]
    return {"patterns": nq, "match_stats_ms": ms, "patterns_per_s": nq / (ms * 1e-3), "parent_calls_per_pattern": float(d_fb.to(torch.float64).mean().item()),
            "unmodified_half_equals_closed_form": ok, "requests_per_pattern": per_pattern,
            "request_rate": {"achieved_G_per_s": rate, "ceiling_G_per_s": limit, "frac_of_ceiling": rate / limit}}


def match_stats_roofline(gpu, d_pat, d_off, nq, m, d_ms, d_rng, d_fb, kernel_ms, dev, records=None, events=None):
    """Memory requests of one launch of the matching-statistics kernel from its instrumented twin (gcsa2_match_stats_profile_device:
    same results, event counts), against the box's request ceiling -- the kernel is a gather like find(): blocks requested first
    (one per lane step or pair attempt), second blocks (endpoints in different blocks), LCP windows (parent()), all 128-byte
    lines; one 16-byte pattern record per 32 characters, the seed entry, the pattern's offsets; the statistics go out as 32-byte
    sectors (16 positions), break points as 32-byte records.  `kernel_ms` is the timed launch (pre-pass included)."""
    import torch
    if events is None:
        d_prof = torch.zeros(16, dtype=torch.int64, device=dev)
        keep = (d_ms.clone(), d_rng.clone(), d_fb.clone())
        gpu.match_stats_profile_device(d_pat.data_ptr(), d_off.data_ptr(), nq, nq * m, d_ms.data_ptr(), d_rng.data_ptr(), d_fb.data_ptr(), d_prof.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(keep[0], d_ms) and torch.equal(keep[1], d_rng) and torch.equal(keep[2], d_fb), "instrumented and timed kernels disagree"
        prof = [int(x) for x in d_prof.cpu()]
        # k_match_stats2's twin: one window per parent() call, every retry a block request (a lane step)
        names = ["rounds", "rounds_with_second_fetch", "lane_steps", "pair_attempts", "failed_pair_attempts", "parent_calls", "tree_walks", "second_fetches"]
        events = dict(zip(names, prof[8:16]))
        events["lcp_windows"] = events["parent_calls"]
        del keep
    lines = events["lane_steps"] + events["second_fetches"] + events["lcp_windows"]
    records_in = nq * ((m + 31) // 32 + 2)
    small = records_in + 2 * nq                                   # pattern records, seed entry, offsets
    writes = nq * ((m + 15) // 16) if records is None else records + nq
    algo = 128 * lines + 16 * records_in + 24 * nq + 32 * writes + 24 * nq
    requests = lines + small + writes
    limit = MEASURED_CEILING or REQUEST_CEILING_GPS
    rate = requests / (kernel_ms * 1e-3) / 1e9
    achieved = algo / (kernel_ms * 1e-3) / 1e9
    return {"bound": "hbm", "kernel": "k_match_stats2" + ("<breaks>" if records is not None else ""), "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS, "traffic": None, "algorithmic_bytes_per_launch": algo, "kernel_ms": kernel_ms,
            "events": events, "requests_per_pattern": requests / nq, "line_requests_per_pattern": lines / nq,
            "request_rate": {"achieved_G_per_s": rate, "ceiling_G_per_s": limit, "frac_of_ceiling": rate / limit},
            "frac_of_request_ceiling": rate / limit}


def match_breaks_leg(gpu, d_pat, d_off, nq, m, d_ms, d_rng, d_fb, exp, timed, dev):
    """The same batch through gcsa2_match_breaks_device: the break points (left-maximal matches {position, length, sp, ep}) as a
    CSR instead of 2 bytes per pattern position -- what a MEM finder consumes (src/algorithms.cpp:146-167 is the reference's
    caller of this interplay).  Checks: the unmodified half has exactly one record each, (0, 256, r, r) with r the closed form;
    the records of the first 200 k patterns expand to exactly the dense statistics of the timed dense run; final ranges and
    parent() counts equal the dense kernel's.  Also the unmodified patterns alone (a clean batch), dense and as break points."""
    import torch
    stream = torch.cuda.current_stream()
    d_boff = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    d_rng2 = torch.zeros((nq, 2), dtype=torch.int64, device=dev)
    d_fb2 = torch.zeros(nq, dtype=torch.int64, device=dev)
    from gcsa2_amd.binding import Gcsa2Error
    cap = 16 * nq
    d_brk = torch.zeros((cap, 4), dtype=torch.int64, device=dev)
    total = [0]

    def run():
        total[0] = gpu.match_breaks_device(d_pat.data_ptr(), d_off.data_ptr(), nq, nq * m, d_boff.data_ptr(), d_brk.data_ptr(), cap,
                                           d_rng2.data_ptr(), d_fb2.data_ptr(), stream.cuda_stream)
    try:
        run()
    except Gcsa2Error as e:              # the refusal carries the number of records needed (a small index breaks far more often)
        if e.code != -6:
            raise
        cap = int(e.needed)
        d_brk = torch.zeros((cap, 4), dtype=torch.int64, device=dev)
    t = timed(run)
    n = total[0]
    counts = d_boff[1:] - d_boff[:-1]
    first = d_brk[d_boff[:-1][0::2]]
    one_each = bool((counts[0::2] == 1).all()) and bool((first[:, 0] == 0).all()) and bool((first[:, 1] == m).all()) and \
        bool(torch.equal(first[:, 2], exp)) and bool(torch.equal(first[:, 3], exp))
    same_tail = bool(torch.equal(d_rng2, d_rng)) and bool(torch.equal(d_fb2, d_fb))
    # expansion of the first patterns' records: record j of a pattern covers [p_j, p_(j-1)) (m for its first record)
    ns = min(nq, 200_000)
    r0, r1 = 0, int(d_boff[ns].item())
    rec = d_brk[r0:r1]
    owner = torch.repeat_interleave(torch.arange(ns, device=dev), counts[:ns])
    is_first = torch.ones(r1 - r0, dtype=torch.bool, device=dev)
    is_first[1:] = owner[1:] != owner[:-1]
    right = torch.where(is_first, torch.full_like(rec[:, 0], m), torch.cat([rec[:1, 0], rec[:-1, 0]]))
    span = right - rec[:, 0]
    covers = bool((span > 0).all()) and int(span.sum().item()) == ns * m
    dense_ok = False
    if covers:
        ridx = torch.repeat_interleave(torch.arange(r1 - r0, device=dev), span)
        begin = torch.cumsum(span, 0) - span
        within = torch.arange(ns * m, device=dev) - begin[ridx]                  # i - p, in the order records arrive (descending p per pattern)
        pos = rec[ridx, 0] + within
        val = torch.clamp(rec[ridx, 1] - within, max=65535)
        rebuilt = torch.zeros(ns * m, dtype=torch.int64, device=dev)
        rebuilt[owner[ridx] * m + pos] = val
        dense_ok = bool(torch.equal(rebuilt, d_ms[: ns * m].to(torch.int64) & 0xFFFF))
        del ridx, within, pos, val, rebuilt
    # a MEM finder's view: only matches of at least 20 bp (right after a mismatch a match is as short as any string of
    # log4(n) = 16 characters and every position breaks: those records outnumber the bytes of the dense statistics)
    min_mem = 20
    t_mem = timed(lambda: total.__setitem__(0, gpu.match_breaks_device(d_pat.data_ptr(), d_off.data_ptr(), nq, nq * m, d_boff.data_ptr(), d_brk.data_ptr(),
                                                                         cap, d_rng2.data_ptr(), d_fb2.data_ptr(), stream.cuda_stream, min_length=min_mem)))
    n_mem = total[0]
    long_enough = bool((d_brk[:n_mem, 1] >= min_mem).all()) if n_mem else True
    # diagnostic: a minimum length no match reaches -- the kernel finds every break and writes none (what the record stores cost)
    t_none = timed(lambda: gpu.match_breaks_device(d_pat.data_ptr(), d_off.data_ptr(), nq, nq * m, d_boff.data_ptr(), d_brk.data_ptr(), cap,
                                                   d_rng2.data_ptr(), d_fb2.data_ptr(), stream.cuda_stream, min_length=1 << 30))
    out = {"ms": t, "patterns_per_s": nq / (t * 1e-3), "records": n, "records_per_pattern": n / nq, "bytes_out_per_pattern": 32 * n / nq + 8,
           "no_records_ms": t_none,
           "min_length_20": {"ms": t_mem, "patterns_per_s": nq / (t_mem * 1e-3), "records": n_mem, "records_per_pattern": n_mem / nq,
                             "bytes_out_per_pattern": 32 * n_mem / nq + 8, "every_record_long_enough": long_enough,
                             "unmodified_half_still_one_record_each": bool((d_boff[1:][0::2] - d_boff[:-1][0::2] == 1).all())},
           "unmodified_half_has_one_record_in_closed_form": one_each, "expands_to_the_dense_statistics_on_the_first_patterns": dense_ok,
           "final_ranges_and_parent_counts_equal_dense": same_tail}
    # a clean batch: the unmodified patterns alone
    nc = nq // 2
    d_clean = padded_bytes(d_pat[: nq * m].view(nq, m)[0::2].contiguous())
    d_coff = torch.arange(nc + 1, dtype=torch.int64, device=dev) * m
    d_ms2 = torch.zeros(nc * m + 8, dtype=torch.int16, device=dev)
    t_dense = timed(lambda: gpu.match_stats_device(d_clean.data_ptr(), d_coff.data_ptr(), nc, d_ms2.data_ptr(), d_rng2.data_ptr(), d_fb2.data_ptr(),
                                                   stream.cuda_stream, total_bytes=nc * m))
    t_brk = timed(lambda: gpu.match_breaks_device(d_clean.data_ptr(), d_coff.data_ptr(), nc, nc * m, d_boff.data_ptr(), d_brk.data_ptr(), cap,
                                                  d_rng2.data_ptr(), d_fb2.data_ptr(), stream.cuda_stream))
    out["clean_batch"] = {"patterns": nc, "dense_patterns_per_s": nc / (t_dense * 1e-3), "breaks_patterns_per_s": nc / (t_brk * 1e-3)}
    # where a MEM finder's reads actually live: the batch in pageable HOST memory -> gcsa2_match_breaks_batch (pieces of 16 MB of
    # pattern bytes on four streams, records committed in piece order) -> CSR, final ranges and parent() counts in host memory
    try:
        h_pat = d_pat[: nq * m].cpu().numpy().copy()
        h_off = np.arange(nq + 1, dtype=np.uint64) * np.uint64(m)
        bufs = (np.ones(nq + 1, dtype=np.uint64), np.ones((max(n_mem, 1) + 16, 4), dtype=np.uint64), np.ones((nq, 2), dtype=np.uint64), np.ones(nq, dtype=np.uint64))
        best = timed_calls(lambda: gpu.match_breaks_batch(h_pat, h_off, min_length=min_mem, out=bufs), warm=2, warm_seconds=0.3, timed=4)
        hb, hr, hrng, hfb = gpu.match_breaks_batch(h_pat, h_off, min_length=min_mem, out=bufs)
        assert gpu.match_breaks_device(d_pat.data_ptr(), d_off.data_ptr(), nq, nq * m, d_boff.data_ptr(), d_brk.data_ptr(), cap, d_rng2.data_ptr(),
                                       d_fb2.data_ptr(), stream.cuda_stream, min_length=min_mem) == n_mem       # the device-resident run to compare with
        torch.cuda.synchronize()
        same = bool(np.array_equal(hb, d_boff.cpu().numpy().view(np.uint64))) and hr.shape[0] == n_mem and \
            bool(np.array_equal(hr, d_brk[:n_mem].cpu().numpy().view(np.uint64))) and bool(np.array_equal(hrng, d_rng2.cpu().numpy().view(np.uint64))) and \
            bool(np.array_equal(hfb, d_fb2.cpu().numpy().view(np.uint64)))
        out["host_batch_min_length_20"] = {"workload": f"the same {nq} x {m}-bp patterns in pageable host memory -> gcsa2_match_breaks_batch (min_length {min_mem}) -> "
                                                       "break points, final ranges and parent() counts in host memory (best of 4 after warm-up)",
                                           "ms": best * 1e3, "patterns_per_s": nq / best, "bytes_per_pattern_over_pcie": m + 8 + 32 * n_mem / nq + 8 + 24,
                                           "GB_per_s_end_to_end": nq * (m + 40 + 32 * n_mem / nq) / best / 1e9, "equals_device_resident_run": same}
        # the same with every array of the caller page-locked (the copy engines read and write them in place)
        pin = lambda a: torch.from_numpy(a).pin_memory().numpy()
        p_pat, p_off = pin(h_pat), pin(h_off.view(np.int64)).view(np.uint64)
        p_bufs = tuple(pin(b.view(np.int64)).view(np.uint64) for b in bufs)
        best = timed_calls(lambda: gpu.match_breaks_batch(p_pat, p_off, min_length=min_mem, out=p_bufs), warm=2, warm_seconds=0.3, timed=4)
        pb_, pr_, _, _ = gpu.match_breaks_batch(p_pat, p_off, min_length=min_mem, out=p_bufs)
        out["host_batch_min_length_20"]["page_locked"] = {"ms": best * 1e3, "patterns_per_s": nq / best,
                                                          "equals_pageable_run": bool(np.array_equal(pb_, hb) and np.array_equal(pr_, hr))}
    except Exception as e:
        out["host_batch_min_length_20"] = dict(out.get("host_batch_min_length_20", {}), error=str(e)[:200])
    return out


def config5_sharded(args, D, wl, dev):
    """BASELINE configs[4] as written: the 1 M 256-bp batch sharded contiguously over the ranks (index replicated), every rank
    runs the fused LF + parent kernel and locate() on its shard, the root receives the matching statistics, ranges, parent()
    counts and the CSR of located values in query order (gcsa2_comm_match_stats / gcsa2_comm_locate: per-rank totals, then
    offsets and values through the grouped send / recv gather).  The root checks the gathered batch: closed
    form for the unmodified half, count() == located values for every range (benchmark/query_gcsa.cpp:171-179)."""
    import torch
    from workload import mseq_torch
    from gcsa2_amd import shard
    gpu, ix = wl.gpu, wl.ix
    nq_total, m = 1_000_000, 256
    bounds = shard_bounds(nq_total, D.world)
    b, e = bounds[D.rank]
    nq = e - b
    counts = [hi - lo for lo, hi in bounds]
    stream = torch.cuda.current_stream()
    pats, start, expected = wl.long_patterns(b, nq, m, CONFIG5_SEED)
    nxt = torch.zeros(256, dtype=torch.uint8, device=dev)
    for a_, b_ in zip(b"ACGT", b"CGTA"):
        nxt[a_] = b_
    odd = (torch.arange(b, e, device=dev) % 2) == 1                # global parity: the batch is the same for every N
    for col in range(37, m, 41):
        pats[odd, col] = nxt[pats[odd, col].to(torch.int64)]
    d_pat = padded_bytes(pats)
    del pats
    d_off = torch.arange(nq + 1, dtype=torch.int64, device=dev) * m
    root = D.rank == 0
    d_ms = torch.zeros((nq_total if root else 1) * m + 8, dtype=torch.int16, device=dev)
    d_rng = torch.zeros((nq_total if root else 1, 2), dtype=torch.int64, device=dev)
    d_fb = torch.zeros(nq_total if root else 1, dtype=torch.int64, device=dev)
    use_comm = D.comm is not None

    def run_match_stats():
        if use_comm:
            D.comm.match_stats(gpu, d_pat.data_ptr(), d_off.data_ptr(), counts, [c * m for c in counts], d_ms.data_ptr(), d_rng.data_ptr(),
                               d_fb.data_ptr(), 0, stream.cuda_stream)
            return
        # control-flow check without the library communicator (gloo, or the torch fallback): through host memory
        l_ms = torch.zeros(nq * m + 8, dtype=torch.int16, device=dev)
        l_rng = torch.zeros((max(nq, 1), 2), dtype=torch.int64, device=dev)
        l_fb = torch.zeros(max(nq, 1), dtype=torch.int64, device=dev)
        gpu.match_stats_device(d_pat.data_ptr(), d_off.data_ptr(), nq, l_ms.data_ptr(), l_rng.data_ptr(), l_fb.data_ptr(), stream.cuda_stream,
                               total_bytes=nq * m)
        torch.cuda.synchronize()
        g_ms = shard.gather_variable(l_ms[: nq * m].cpu().numpy().view(np.uint16), [c * m for c in counts])
        g_rng = shard.gather_variable(l_rng[:nq].cpu().numpy().view(np.uint64).reshape(-1), [2 * c for c in counts])
        g_fb = shard.gather_variable(l_fb[:nq].cpu().numpy().view(np.uint64), counts)
        if root:
            d_ms[: nq_total * m] = torch.from_numpy(g_ms.view(np.int16)).to(dev)
            d_rng.copy_(torch.from_numpy(g_rng.view(np.int64).reshape(-1, 2)).to(dev))
            d_fb.copy_(torch.from_numpy(g_fb.view(np.int64)).to(dev))

    run_match_stats()
    torch.cuda.synchronize()
    reps = 5
    D.barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        run_match_stats()
    torch.cuda.synchronize()
    D.barrier()
    ms_time = D.max(time.perf_counter() - t0) / reps * 1e3
    # locate() of the final ranges of every shard, CSR gathered on the root
    if root:
        my_rng = d_rng[b:e].contiguous()
    else:
        my_rng = torch.zeros((max(nq, 1), 2), dtype=torch.int64, device=dev)
        l_ms = torch.zeros(nq * m + 8, dtype=torch.int16, device=dev)
        gpu.match_stats_device(d_pat.data_ptr(), d_off.data_ptr(), nq, l_ms.data_ptr(), my_rng.data_ptr(), 0, stream.cuda_stream, total_bytes=nq * m)
        torch.cuda.synchronize()
        del l_ms
    d_loff = torch.zeros((nq_total if root else 1) + 1, dtype=torch.int64, device=dev)
    loc_total, loc_vals = 0, None

    def run_locate():
        nonlocal loc_total, loc_vals
        if use_comm:
            res = D.comm.locate(gpu, my_rng.data_ptr(), counts, d_loff.data_ptr(), 0, stream.cuda_stream)
            if root:
                job, d_val, loc_total = res
                from gcsa2_amd.binding import fetch_job
                loc_vals = fetch_job(job, loc_total) if loc_vals is None else (gpu.locate_discard(job) or loc_vals)
            return
        job, d_o, d_v, tot = gpu.locate_device(my_rng.data_ptr(), nq, stream.cuda_stream)
        l_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        l_val = torch.zeros(max(tot, 1), dtype=torch.int64, device=dev)
        gpu.locate_discard(job)
        gpu.locate_into(my_rng.data_ptr(), nq, l_off.data_ptr(), l_val.data_ptr(), max(tot, 1), stream.cuda_stream)
        torch.cuda.synchronize()
        res = shard.locate_sharded(lambda r: (l_off.cpu().numpy().view(np.uint64), l_val[:tot].cpu().numpy().view(np.uint64)),
                                   np.zeros((nq_total, 2), dtype=np.uint64))
        if root:
            d_loff.copy_(torch.from_numpy(res[0].view(np.int64)).to(dev))
            loc_total, loc_vals = int(res[0][-1]), res[1]

    run_locate()
    D.barrier()
    t0 = time.perf_counter()
    for _ in range(3):
        run_locate()
    torch.cuda.synchronize()
    D.barrier()
    loc_ms = D.max(time.perf_counter() - t0) / 3 * 1e3
    out = None
    if root:
        pats_all, start_all, exp_all = wl.long_patterns(0, nq_total, m, CONFIG5_SEED)
        del pats_all
        exp = exp_all[0::2]
        ms2d = d_ms[: nq_total * m].view(nq_total, m)
        want_ms = (m - torch.arange(m, device=dev)).to(torch.int16).view(1, m)
        exact_ok = bool(torch.equal(d_rng[0::2, 0], exp)) and bool(torch.equal(d_rng[0::2, 1], exp)) and \
            bool((d_fb[0::2] == 0).all()) and bool((ms2d[0::2] == want_ms).all())
        d_cnt = torch.zeros(nq_total, dtype=torch.int64, device=dev)
        gpu.count_device(d_rng.data_ptr(), nq_total, d_cnt.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        consistent = bool(torch.equal(d_loff[1:] - d_loff[:-1], d_cnt)) and int(d_loff[-1]) == loc_total
        first_vals = loc_vals[d_loff[:-1][0::2].cpu().numpy()]
        located_ok = bool(np.array_equal(first_vals, mseq_torch.node_values(start_all[0::2].cpu().numpy()))) if start_all is not None else None
        out = {"workload": f"{nq_total} x {m}-bp walks, every second one with a substitution every 41 bp, sharded contiguously over {D.world} GPU(s): "
                           "backward search with parent() on failure + locate() of the final ranges on every shard, results gathered on the root "
                           + (("(gcsa2_comm_match_stats / gcsa2_comm_locate: grouped RCCL send / recv)" if D.backend == "nccl" else
                              "(gcsa2_comm_match_stats / gcsa2_comm_locate over a host-memory transport: control-flow check)") if use_comm
                              else "(through host memory, Python mirror of the sharding: control-flow check)"),
               "n_gpus": D.world, "match_stats_ms": ms_time, "patterns_per_s": nq_total / (ms_time * 1e-3), "bases_per_s": nq_total * m / (ms_time * 1e-3),
               "parent_calls_per_pattern": float(d_fb.to(torch.float64).mean().item()), "unmodified_half_equals_closed_form": exact_ok,
               "locate": {"ms_per_step": loc_ms, "value": nq_total / (loc_ms * 1e-3), "unit": "queries/s", "values": loc_total,
                          "count_equals_located": consistent, "unmodified_half_equals_closed_form": located_ok}}
    return out


def setup_repeats(args, D, dev, local_rank, nq=None, m=None):
    """A repeat-rich index: the chr22-like SNP graph over a backbone with planted repeat families (an Alu-like family in every
    600-bp block at 7 % divergence, a younger 600-bp family, short tandem arrays; workload/graphs.py::repeat_bases), so that
    found 32-mers match hundreds of path nodes on average and 16-mers thousands, as on the paper's human indexes
    (paper.tex:403,408) -- the other workloads have unique seed-length k-mers, i.e. singleton ranges."""
    import torch
    from workload import graphs, builder, cache, patterns
    from gcsa2_amd.binding import GCSA
    wl = Workload()
    log2_bases = args.log2_bases or 23
    path = os.path.join(args.cache_dir, f"repeats_{log2_bases}_{args.order}_v1.npz")
    t = time.time()
    graph = graphs.repeat_graph(1 << log2_bases, 0x6C5A0020, 0x6C5A0021)
    ix = None
    if D.rank == 0 and not os.path.exists(path):
        os.makedirs(args.cache_dir, exist_ok=True)
        ix = builder.build(graph, args.order, keep_table=False)
        cache.save(path + ".tmp.npz", ix)
        os.replace(path + ".tmp.npz", path)
    D.barrier()
    if ix is None:
        ix = cache.load(path)
    log(f"repeat-rich index: n={ix.n} e={ix.e} samples={ix.sample_count} ({time.time() - t:.1f} s)")
    wl.gpu = GCSA(ix, device=local_rank)
    wl.ix, wl.graph = ix, graph
    wl.nq = nq or args.queries or 4_000_000
    wl.m = m or args.pattern_len
    wl.total_queries = wl.nq * D.world
    wl.first = wl.nq * D.rank
    pats = patterns.walk_patterns(graph, wl.nq, wl.m, 0x6C5A0022 + wl.m + 0x1000 * D.rank)
    flat, off = patterns.as_batch(pats)
    wl.d_pat = padded_bytes(torch.from_numpy(flat).to(dev))
    wl.d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    wl.label = (f"repeat-rich SNP graph 2^{log2_bases} bases (planted interspersed and tandem repeats), order-{args.order} GCSA, "
                f"{wl.nq} x {wl.m}-mer find() per GPU, walks through the graph")
    return wl


def repeats_secondary(args, D, dev, local_rank):
    """The hot path on WIDE ranges: find() of 32-mers and 16-mers on the repeat-rich index, with the share of steps that need a
    second block, the seed-table entries marked wide, and locate() of the ranges with its segment-size classes."""
    import torch
    out = {}
    for m in (32, 16):
        wl = setup_repeats(args, D, dev, local_rank, nq=4_000_000, m=m)
        r = measure(args, D, dev, wl, max(5, args.steps), 2)
        d_out = r["d_out"]
        width = (d_out[:, 1] - d_out[:, 0] + 1).to(torch.float64)
        leg = {"workload": wl.label, "value": wl.nq / (r["kernel_ms"] * 1e-3), "unit": "queries/s", "kernel_ms": r["kernel_ms"],
               "mean_range_width_path_nodes": float(width.mean().item()), "ranges_wider_than_one": float((width > 1).to(torch.float64).mean().item()),
               "config": find_config(wl, r, 1), "roofline": roofline(args, r, wl, f"repeats_{args.log2_bases or 23}_{m}_S")}
        if not args.no_cpu:
            leg["cpu_baseline"] = cpu_baseline(args, wl, d_out, args.cpu_seconds / 4)
        # locate() of the first ranges (the whole batch would be billions of values), with the sizes the sort has to handle
        nloc = 400_000 if m == 32 else 100_000
        loc, d_loff, _ = measure_locate(wl.gpu, d_out[:nloc].contiguous(), dev, 3)
        sizes = d_loff[1:] - d_loff[:-1]
        loc["segments"] = {"one value": int((sizes == 1).sum().item()), "2..16": int(((sizes >= 2) & (sizes <= 16)).sum().item()),
                           "17..1024": int(((sizes >= 17) & (sizes <= 1024)).sum().item()), "more than 1024": int((sizes > 1024).sum().item()),
                           "largest": int(sizes.max().item())}
        leg["locate"] = loc
        out[f"{m}-mers"] = leg
        del r, d_out
        release(wl)
    return out


# ---- wide ranges and the memory ladder on the headline index ---------------------------------

class Leg(Workload):
    """The headline's image with another batch of patterns: what measure() / roofline() / find_config() read."""

    def __init__(self, wl, d_pat, nq, m, label):
        import torch
        super().__init__()
        self.gpu, self.ix, self.scaling = wl.gpu, wl.ix, "strong"
        self.d_pat, self.nq, self.m, self.total_queries, self.first = d_pat, nq, m, nq, 0
        self.d_off = torch.arange(nq + 1, dtype=torch.int64, device=d_pat.device) * m
        self.label = label


def find_leg(args, D, dev, leg, steps, expect=None, key="unprofiled"):
    """One find() measurement as a compact object: rate, requests per query, share of steps that fetch a second block
    (a range whose ends lie in different blocks), mean range width, roofline, and the closed-form check."""
    import torch
    r = measure(args, D, dev, leg, steps, 1)
    d_out = r["d_out"]
    width = (d_out[:, 1] - d_out[:, 0] + 1).to(torch.float64)
    rf = roofline(args, r, leg, key)
    out = {"workload": leg.label, "value": leg.nq / (r["kernel_ms"] * 1e-3), "unit": "queries/s", "kernel_ms": r["kernel_ms"], "queries": leg.nq,
           "pattern_len": leg.m, "kmer_table_k": leg.gpu.kmer_table_k(), "pair_blocks": bool(leg.gpu.pair_block_bytes()),
           "mean_range_width_path_nodes": float(width.mean().item()), "ranges_wider_than_one": float((width > 1).to(torch.float64).mean().item()),
           "lf_steps_per_query": r["lf_steps"] / leg.nq, "blocks_per_query": r["blocks"] / leg.nq,
           "requests_per_query": rf["request_rate"]["requests_per_query"], "requests_G_per_s": rf["request_rate"]["achieved_G_per_s"],
           "second_fetch_fraction_of_steps": r["second_fetches"] / max(r["fetch_steps"], 1), "wide_seed_entries_hit": r["wide_seeds"],
           "algorithmic_bytes_per_launch": r["algo_bytes"], "achieved_GBps": rf["achieved"], "frac": rf["frac"],
           "served": rf["served"], "working_set_bytes": rf["working_set_bytes"], "requests_per_distinct_line": rf["requests_per_distinct_line"],
           "image_bytes_hbm": leg.gpu.device_bytes()}
    if rf["served"] != "HBM":
        out["frac_is"] = "algorithmic bytes / kernel time / 8 TB/s: the launch is partly served on-die, this is NOT an HBM fraction"
    out["frac_of_request_ceiling"] = rf["request_rate"].get("frac_of_ceiling")
    for name in ("traffic", "traffic_over_algorithmic", "traffic_GBps", "traffic_frac_of_measured_hbm_rate"):
        if rf.get(name) is not None:
            out[name] = rf[name]
    if expect is not None:
        out["all_ranges_equal_closed_form"] = bool(expect(d_out))
    return out, d_out


def wide_ranges_secondary(args, D, dev, wl):
    """The hot path on WIDE ranges at HBM footprint, on the headline index itself.  (i) 12-, 14- and 16-mers: prefixes of
    path labels, whose ranges are intervals of the k-mer bitmap's ranks (workload/dbg_torch.py::prefix_patterns_device):
    ~341 / 21 / 1.3 path nodes per range at 5.73 G nodes; shorter than the seed table's k, the 12- and 14-mers are searched
    from charRange on, every step on a range of thousands to millions of path nodes (sp and ep + 1 in different blocks: two
    memory requests per step).  (ii) The headline's 32-mers with the seed table cut to k = 8 (gcsa2_index_set_tables): 24
    steps per query, the first nine of them on wide ranges (4^9 = 262 144 -> 1 path nodes).  Every range is checked against
    its closed form.  The headline's own batch (k = 16) meets no wide range after its seed entry."""
    import torch
    from workload import dbg_torch
    out = {}
    k_full = wl.gpu.kmer_table_k()
    nq = min(25_000_000, max(100_000, wl.total_queries // 4))
    k = wl.dbg.k
    for m in ((12, 14, 16) if k == 17 else sorted({max(1, k - 5), max(1, k - 3), k - 1})):       # (small test indexes: scaled with k)
        pats, sp, ep = dbg_torch.prefix_patterns_device(wl.dbg, 0, nq, m, HUMAN_PATTERN_SEED + 0x100 + m)
        leg = Leg(wl, padded_bytes(pats), nq, m, f"{nq} x {m}-mers, prefixes of path labels of the headline index (closed form: rank interval of the k-mer bitmap)")
        del pats
        out[f"{m}-mers"], _ = find_leg(args, D, dev, leg, 5, expect=lambda d: torch.equal(d[:, 0], sp) and torch.equal(d[:, 1], ep),
                                       key=f"pangenome_{wl.degree}_{m}_prefix")
        del leg, sp, ep
    k_cut = min(8, max(1, wl.dbg.k // 2))
    if k_full > k_cut:
        wl.gpu.set_tables(kmer_k=k_cut)
        leg = Leg(wl, wl.d_pat, wl.nq, wl.m, f"the headline batch ({wl.nq} x {wl.m}-mers) with the seed table cut to k = {k_cut}")
        out[f"{wl.m}-mers, seed table k = {k_cut}"], _ = find_leg(args, D, dev, leg, 3, expect=lambda d: wl.verify(d, wl.first, wl.nq),
                                                               key=f"pangenome_{wl.degree}_{wl.m}_S_k{k_cut}")
        wl.gpu.set_tables(kmer_k=k_full)
    return out


def memory_ladder(args, D, dev, wl, headline):
    """What each optional table buys per gigabyte, at HBM scale: the headline batch and locate() of its first 10 M ranges on the
    same image re-shaped rung by rung with gcsa2_index_set_tables (no re-creation).  Every rung is checked bit for bit against
    the closed form (find) and count() (locate).  The rungs go down in the order that loses least find() throughput per
    gigabyte freed (round 4's ladder gave up the 61 GB pair blocks before a 26 GB seed level worth a ninth of them, VERDICT r04
    #4): locate table, then seed-table levels (each quarters the table and costs one LF step per query), and only then the pair
    blocks; the second half shows the seed table's value without pair blocks.  The last rung is the image north_star's "~30 GB"
    had in mind (paper.tex:380: 14.6 GB for the reference's encoding) -- its rate goes into the line as
    `value_at_reference_footprint`.  GCSA2_MEMORY_BUDGET_MB at create time takes the same decisions from a cap
    (tests/test_gpu_parity.py::test_memory_ladder)."""
    import torch
    gpu = wl.gpu
    k_full = gpu.kmer_table_k()
    has_samples = gpu.sampleCount() > 0
    has_pairs = gpu.pair_block_bytes() > 0
    nloc = min(10_000_000, wl.nq)
    rungs = []

    def rung(name, first=False):
        leg = Leg(wl, wl.d_pat, wl.nq, wl.m, name)
        if first:
            o = {"workload": name, "value": headline["value"], "kernel_ms": headline["roofline"]["kernel_ms"],
                 "requests_per_query": headline["roofline"]["request_rate"]["requests_per_query"], "frac": headline["roofline"]["frac"],
                 "frac_of_request_ceiling": headline["roofline"]["request_rate"].get("frac_of_ceiling"), "served": headline["roofline"]["served"],
                 "all_ranges_equal_closed_form": headline["config"]["all_ranges_equal_closed_form"], "from": "the headline measurement above"}
            d_out = torch.zeros((wl.nq, 2), dtype=torch.int64, device=dev)
            gpu.find_device(wl.d_pat.data_ptr(), wl.d_off.data_ptr(), wl.nq, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        else:
            o, d_out = find_leg(args, D, dev, leg, 3, expect=lambda d: wl.verify(d, wl.first, wl.nq))
            o = {key: o.get(key) for key in ("workload", "value", "kernel_ms", "requests_per_query", "lf_steps_per_query", "frac", "frac_of_request_ceiling",
                                             "served", "all_ranges_equal_closed_form")}
        o.update(image_bytes_hbm=gpu.device_bytes(), pair_block_bytes=gpu.pair_block_bytes(), kmer_table_k=gpu.kmer_table_k(),
                 locate_table_bytes=gpu.locate_table_bytes())
        if rungs:
            freed = (rungs[-1]["image_bytes_hbm"] - o["image_bytes_hbm"]) / 1e9
            if freed > 0:
                o["queries_per_s_lost_per_GB_freed"] = (rungs[-1]["value"] - o["value"]) / freed
        if has_samples:
            loc, _, _ = measure_locate(gpu, d_out[:nloc].contiguous(), dev, 2)
            o["locate"] = {key: loc[key] for key in ("value", "unit", "ms_per_step", "values", "count_equals_located")}
        del d_out
        torch.cuda.empty_cache()
        rungs.append(o)

    rung("everything: pair blocks, seed table, locate table", first=True)
    if gpu.locate_table_bytes() > 0:
        gpu.set_tables(locate_table=0)
        rung("without the locate table")
    seen = {k_full}
    for k in (k_full - 1, k_full - 2, k_full - 3):
        if k >= 1 and k not in seen:
            seen.add(k)
            gpu.set_tables(kmer_k=k)
            rung(f"... seed table at k = {k}" + (" (pair blocks kept)" if has_pairs else ""))
    if has_pairs:
        seen = set()
        for k in (k_full, k_full - 1, k_full - 3):
            if k >= 1 and k not in seen:
                seen.add(k)
                gpu.set_tables(pair_blocks=0, kmer_k=k)
                rung(f"no pair blocks, seed table at k = {k}")
    out = {"note": "one image re-shaped with gcsa2_index_set_tables; find() = the headline batch, locate() = its first "
                   f"{nloc} ranges; results identical on every rung", "rungs": rungs}
    last = rungs[-1]
    headline["value_at_reference_footprint"] = {
        "value": last["value"], "unit": "queries/s", "image_GB": round(last["image_bytes_hbm"] / 1e9, 1), "frac": last["frac"],
        "frac_of_request_ceiling": last.get("frac_of_request_ceiling"), "served": last.get("served"), "requests_per_query": last["requests_per_query"],
        "tables": last["workload"], "note": "the headline batch on the smallest image of the memory ladder (north_star: ~30 GB)"}
    return out


# ---- a repeat-rich text at HBM footprint: wide ranges as real genomes have them (VERDICT r03 #2 ii) ----------------

REPEATS30_SEED = 0x6C5A0060


def setup_repeats30(args, D, dev, local_rank, log2_bases=30):
    """The repeat-rich text as a primary workload (`--workload repeats30`; profiler passes): 20 M patterns per GPU."""
    import torch
    from workload import linear_torch, repeats_torch
    from gcsa2_amd.binding import GCSA
    n = 1 << log2_bases
    t = time.time()
    seq = repeats_torch.repeat_bases_torch(n, REPEATS30_SEED, dev)
    ix = linear_torch.build_linear(n, REPEATS30_SEED, order=256, device=dev, with_lcp=False, verbose=log, sequence=seq)
    torch.cuda.empty_cache()
    log(f"repeat-rich text: 2^{log2_bases} bases, n = {ix.n} path nodes ({time.time() - t:.1f} s)")
    t = time.time()
    wl = Workload()
    wl.gpu = GCSA(ix, device=local_rank, with_lcp=False)
    wl.ix, wl.scaling, wl.seq, wl.log2_bases = ix, "weak", seq, log2_bases
    log(f"device image: {wl.gpu.device_bytes() / 1e9:.2f} GB, seed table k = {wl.gpu.kmer_table_k()} ({time.time() - t:.1f} s)")
    wl.nq = args.queries or (20_000_000 if log2_bases >= 28 else 2_000_000)
    wl.m = args.pattern_len
    wl.total_queries, wl.first = wl.nq * D.world, wl.nq * D.rank
    pats, _ = repeats_torch.substring_patterns_device(seq, wl.nq, wl.m, REPEATS30_SEED + wl.m, first=wl.first)
    wl.d_pat = padded_bytes(pats)
    wl.d_off = torch.arange(wl.nq + 1, dtype=torch.int64, device=dev) * wl.m
    wl.label = (f"repeat-rich text of 2^{log2_bases} bases (families of interspersed repeats at 7 % divergence, a young family at 6 %, tandem "
                f"arrays; workload/repeats_torch.py) as a linear graph: {ix.n} path nodes, order 256; {wl.nq} x {wl.m}-mer find() per GPU, "
                f"substrings of the text")

    def verify(d_ranges, first, count):
        # the definition on a sample: range width == number of occurrences of the pattern in the text
        if first != wl.first:
            return None
        ns = 48
        occ = repeats_torch.count_occurrences_device(seq, pats[:ns])
        return bool(torch.equal(d_ranges[:ns, 1] - d_ranges[:ns, 0] + 1, occ))
    wl.verify = verify
    return wl


def repeats_hbm_secondary(args, D, dev, local_rank, log2_bases=30):
    """2^30 bases with planted repeat families (workload/repeats_torch.py: interspersed copies at 7 % divergence in families
    of 115 k, a young family, tandem arrays) as a linear graph (workload/linear_torch.py: prefix doubling on the GPU, one
    path node per position): found 32-mers match hundreds of path nodes on average and 16-mers thousands, like the paper's
    human indexes (paper.tex:403,408), on an image of tens of gigabytes.  find() of 20 M 32-mers and 16-mers, locate() of
    400 k / 100 k ranges; checks: range width == number of occurrences in the text for a sample (the definition, by comparing
    windows of the text), the oracle on a sample, count() == located values for every range."""
    import torch
    from workload import repeats_torch
    wl = setup_repeats30(args, D, dev, local_rank, log2_bases=log2_bases)
    ix, seq = wl.ix, wl.seq
    out = {"workload": f"repeat-rich text of 2^{log2_bases} bases (families of interspersed repeats at 7 % divergence, a young family at 6 %, "
                       f"tandem arrays) as a linear graph: {ix.n} path nodes, order 256", "image_bytes_hbm": wl.gpu.device_bytes()}
    nq = args.queries or (20_000_000 if log2_bases >= 28 else 2_000_000)
    cpu = None if args.no_cpu else cpu_open(ix)
    for m in (32, 16):
        pats, _ = repeats_torch.substring_patterns_device(seq, nq, m, REPEATS30_SEED + m)
        leg = Leg(wl, padded_bytes(pats), nq, m, f"{nq} x {m}-mers, substrings of the text at SplitMix64 positions")
        o, d_out = find_leg(args, D, dev, leg, 5, key=f"repeats30_{log2_bases}_{m}_S")
        ns = 64
        occ = repeats_torch.count_occurrences_device(seq, pats[:ns])
        o["range_width_equals_occurrences_in_text_on_sample"] = bool(torch.equal(d_out[:ns, 1] - d_out[:ns, 0] + 1, occ))
        if cpu is not None:
            o["cpu_baseline"] = cpu_baseline_sample(cpu, leg, d_out, min(nq, 200_000))
        nloc = min(nq, 400_000 if m == 32 else 100_000)
        loc, d_loff, d_val = measure_locate(wl.gpu, d_out[:nloc].contiguous(), dev, 3)
        sizes = d_loff[1:] - d_loff[:-1]
        loc["segments"] = {"one value": int((sizes == 1).sum().item()), "2..16": int(((sizes >= 2) & (sizes <= 16)).sum().item()),
                           "17..1024": int(((sizes >= 17) & (sizes <= 1024)).sum().item()), "more than 1024": int((sizes > 1024).sum().item()),
                           "largest": int(sizes.max().item())}
        # a linear graph: every path node has one value, the start position of its suffix; locate() of a pattern = its occurrences
        first_vals = d_val[: int(d_loff[1].item())]
        loc["sorted_distinct_first_range"] = bool((first_vals[1:] > first_vals[:-1]).all().item()) if first_vals.numel() > 1 else True
        # ... of EVERY range (the split + register sort of segments beyond 8192 values, round 5, at full size): values rise strictly
        # inside a range; only across a range boundary may a value be followed by a smaller or equal one
        total_vals = int(d_loff[-1].item())
        if total_vals > 1:
            rises = d_val[1:total_vals] > d_val[: total_vals - 1]
            inner = d_loff[1:-1]
            rises[inner[(inner > 0) & (inner < total_vals)] - 1] = True
            loc["sorted_distinct_every_range"] = bool(rises.all().item())
            del rises
        # ... and the DEFINITION on the widest ranges of the first few thousand: on this linear graph locate() of a pattern's range
        # is the sorted list of its occurrences in the text (as node values), found by comparing windows of the text
        order = torch.argsort(sizes[:4000], descending=True)[:4].cpu().numpy()
        same, checked = True, 0
        for q in order:
            a, e = int(d_loff[q].item()), int(d_loff[q + 1].item())
            want_vals = repeats_torch.occurrence_values_device(seq, pats[int(q)])
            same = same and bool(torch.equal(d_val[a:e], want_vals))
            checked += e - a
        loc["widest_ranges_equal_occurrences_in_text"] = {"ranges": len(order), "values": checked, "equal": same}
        o["locate"] = loc
        out[f"{m}-mers"] = o
        del pats, leg, d_out, d_loff, d_val, sizes
    if cpu is not None:
        cpu.close()
    release(wl)
    return out


def chr22_secondary(args, D, dev, local_rank):
    """BASELINE configs[1] and [2] on one GPU."""
    wl = setup_chr22(args, D, dev, local_rank, nq=10_000_000)
    r = measure(args, D, dev, wl, max(5, args.steps), 2)
    out = {"workload": wl.label, "value": wl.nq / (r["kernel_ms"] * 1e-3), "unit": "queries/s", "kernel_ms": r["kernel_ms"],
           "config": find_config(wl, r, 1), "roofline": roofline(args, r, wl, f"chr22_{args.log2_bases or 25}_{wl.m}_{args.set}")}
    if not args.no_cpu:
        out["cpu_baseline"] = cpu_baseline(args, wl, r["d_out"], args.cpu_seconds / 2)
    out["locate"], _, _ = measure_locate(wl.gpu, r["d_out"], dev, 3)
    del r
    release(wl)
    return out


def release(wl):
    """Free a workload's device image and tensors now (its `verify` closure refers back to it, so dropping the last
    name would leave that to the cycle collector)."""
    import gc
    import torch
    if wl.gpu is not None:
        wl.gpu.close()
    for name in list(vars(wl)):
        setattr(wl, name, None)
    gc.collect()
    torch.cuda.empty_cache()


def human32_secondary(args, D, dev, local_rank):
    """Rounds 1-2's headline, for continuity: the 2^32 - 1 node index of the degree-32 m-sequence text (e = n), find() only."""
    saved = (args.degree, args.no_secondary)
    args.degree, args.no_secondary = 32, True              # no samples / LCP: the find() leg only
    wl = setup_human(args, D, dev, local_rank, total_queries=args.queries or 100_000_000)
    args.degree, args.no_secondary = saved
    r = measure(args, D, dev, wl, max(5, args.steps // 2), 2)
    ok = wl.verify(r["d_out"], wl.first, wl.nq)
    out = {"workload": wl.label, "value": wl.nq / (r["kernel_ms"] * 1e-3), "unit": "queries/s", "kernel_ms": r["kernel_ms"],
           "all_ranges_equal_closed_form": ok, "config": find_config(wl, r, 1),
           "roofline": roofline(args, r, wl, f"human_{wl.degree}_{wl.m}_{args.set}")}
    del r
    release(wl)
    return out


def human_snp_secondary(args, D, dev, local_rank):
    """The headline workload on a BRANCHING index of the same footprint (e = 1.08 n: out- and in-degrees above one wherever a
    bubble opens, closes or an alternative k-mer lands), every range checked against its closed form."""
    import torch
    wl = setup_human(args, D, dev, local_rank, branching=True, total_queries=args.queries or 100_000_000)
    r = measure(args, D, dev, wl, max(5, args.steps // 2), 2)
    ok = wl.verify(r["d_out"], wl.first, wl.nq)
    out = {"workload": wl.label, "value": wl.nq / (r["kernel_ms"] * 1e-3), "unit": "queries/s", "kernel_ms": r["kernel_ms"],
           "all_ranges_equal_closed_form": ok, "config": find_config(wl, r, 1),
           "roofline": roofline(args, r, wl, f"human_snp_{wl.degree}_{wl.m}_{args.set}")}
    del r
    if wl.ix.lcp_size > 0:
        out["config5"] = config5(args, wl, dev)
    release(wl)
    return out


def cpu_baseline(args, wl, d_out, seconds):
    """The oracle (CPU restatement of the reference path) timed on this host: a bounded sample of
    the same patterns, all cores with the verifyIndex-style static split, plus one thread."""
    from oracle.oracle import OracleIndex, max_threads
    t = time.time()
    cpu = OracleIndex(wl.ix, with_samples=False, with_counters=False, with_lcp=False)
    build_s = time.time() - t
    cores = max_threads()
    m = wl.m
    cap = min(wl.nq, 40_000_000)
    flat = wl.d_pat[: cap * m].cpu().numpy()
    offsets = np.arange(cap + 1, dtype=np.uint64) * np.uint64(m)
    probe = min(cap, 20000)
    cpu.find_batch(flat, offsets[:probe + 1], threads=1)
    per_query = cpu.last_seconds / probe
    n1 = int(min(cap, max(probe, 0.25 * seconds / per_query)))
    r1 = cpu.find_batch(flat, offsets[:n1 + 1], threads=1)
    t1 = cpu.last_seconds
    nall = int(min(cap, max(n1, 0.75 * seconds * cores / per_query * 0.5)))
    rall = cpu.find_batch(flat, offsets[:nall + 1], threads=cores)
    tall = cpu.last_seconds
    got = d_out[:nall].cpu().numpy().view(np.uint64)
    parity = bool(np.array_equal(got, rall)) and bool(np.array_equal(got[:n1], r1))
    cpu.close()
    return {"value": nall / tall, "unit": "queries/s", "cores": cores, "kind": "port",
            "sample": f"first {nall} of the {wl.nq} patterns, {m}-mers, OpenMP static split over {cores} threads "
                      f"= the CPUs this container may use (affinity / cgroup quota; {os.cpu_count()} logical CPUs visible) "
                      f"({tall:.1f} s); single thread: first {n1} patterns ({t1:.1f} s); oracle index built in {build_s:.1f} s",
            "single_thread_value": n1 / t1, "single_thread_us_per_query": t1 / n1 * 1e6,
            "gpu_matches_cpu_on_sample": parity}


def cpu_open(ix):
    """The oracle over the find() part of an index (for legs that time it on several batches)."""
    from oracle.oracle import OracleIndex
    return OracleIndex(ix, with_samples=False, with_counters=False, with_lcp=False)


def cpu_baseline_sample(cpu, leg, d_out, nc):
    """The oracle on the first `nc` patterns of a leg, all cores; checks the GPU ranges of the sample."""
    from oracle.oracle import max_threads
    cores = max_threads()
    flat = leg.d_pat[: nc * leg.m].cpu().numpy()
    want = cpu.find_batch(flat, np.arange(nc + 1, dtype=np.uint64) * np.uint64(leg.m), threads=cores)
    return {"value": nc / cpu.last_seconds, "unit": "queries/s", "cores": cores, "kind": "port",
            "sample": f"first {nc} of the {leg.nq} patterns, {leg.m}-mers, OpenMP static split over {cores} threads ({cpu.last_seconds:.1f} s)",
            "gpu_matches_cpu_on_sample": bool(np.array_equal(d_out[:nc].cpu().numpy().view(np.uint64), want))}


def cpu_baseline_match_stats(ix, d_pat, d_ms, d_rng, d_fb, m, ns=4000):
    """config 5's CPU leg: the oracle's LF + parent loop on the first `ns` patterns, timed on all cores, and the
    GPU results of those patterns checked against it."""
    from oracle.oracle import OracleIndex, max_threads
    t = time.time()
    cpu = OracleIndex(ix, with_samples=False, with_counters=False)
    build_s = time.time() - t
    cores = max_threads()
    flat = d_pat[: ns * m].cpu().numpy()
    off = np.arange(ns + 1, dtype=np.uint64) * np.uint64(m)
    cm, cr, cf = cpu.match_stats_batch(flat, off, threads=cores)
    seconds = cpu.last_seconds
    got_ms = d_ms[: ns * m].cpu().numpy().view(np.uint16)
    parity = bool(np.array_equal(got_ms, cm)) and bool(np.array_equal(d_rng[:ns].cpu().numpy().view(np.uint64), cr)) \
        and bool(np.array_equal(d_fb[:ns].cpu().numpy().view(np.uint64), cf))
    cpu.close()
    return {"value": ns / seconds, "unit": "patterns/s", "cores": cores, "kind": "port",
            "sample": f"first {ns} of the patterns, {m} bp, OpenMP static split over {cores} threads ({seconds:.2f} s); "
                      f"oracle index built in {build_s:.1f} s",
            "gpu_matches_cpu_on_sample": parity}


# ---- the line -------------------------------------------------------------------------------------------------

LINE_LIMIT = 4096        # the driver keeps the tail of stdout; round 4's 23 KB line could not be parsed from it


def pick(d, *keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def short(text, n=240):
    return text if not isinstance(text, str) or len(text) <= n else text[: n - 3] + "..."


def one_number(key, leg):
    """A secondary leg in the compact line: its rate (and request-rate fraction where it has one), or its error."""
    if not isinstance(leg, dict):
        return leg
    if "error" in leg:
        return {"error": short(leg["error"], 120)}
    if key == "config5":
        out = pick(leg, "patterns_per_s", "find_patterns_per_s", "n_gpus")
        out["match_stats_frac_of_request_ceiling"] = leg.get("roofline", {}).get("frac_of_request_ceiling")
        out["match_breaks_patterns_per_s"] = leg.get("match_breaks", {}).get("patterns_per_s")
        out["patterns_per_s_at_4x_the_batch"] = leg.get("four_times_the_batch", {}).get("patterns_per_s")
        out["locate_values_per_s"] = leg.get("locate", {}).get("values_per_s")
        out["locate_frac_of_request_ceiling"] = leg.get("locate", {}).get("roofline", {}).get("request_rate", {}).get("frac_of_ceiling")
        return out
    if key == "host_batch":
        return {"queries_per_s": leg.get("value"), "packed_queries_per_s": leg.get("packed", {}).get("value")}
    if key == "memory_ladder":
        rungs = leg.get("rungs", [])       # (image GB, G queries/s) rung by rung; the tables of each rung are in bench_full.json
        return {"image_GB": [round(x["image_bytes_hbm"] / 1e9, 1) for x in rungs], "G_queries_per_s": [round(x["value"] / 1e9, 3) for x in rungs]}
    if key == "locate":
        out = pick(leg, "values_per_s", "ms_per_step")
        out["frac"] = leg.get("roofline", {}).get("frac")
        return out
    if key == "traffic_measured":
        return pick(leg, "source")
    if "value" in leg:                      # chr22, human32, human_branching
        out = {"queries_per_s": leg["value"], "frac": leg.get("roofline", {}).get("frac")}
        if "locate" in leg:
            out["locate_values_per_s"] = leg["locate"].get("values_per_s")
            out["locate_frac_of_request_ceiling"] = leg["locate"].get("roofline", {}).get("request_rate", {}).get("frac_of_ceiling")
        return out
    # wide_ranges, repeats, repeats_hbm: one object per pattern length
    out = {}
    for k, v in leg.items():
        if isinstance(v, dict) and "value" in v:
            out[short(k, 40)] = {"queries_per_s": v["value"], "served": v.get("served", v.get("roofline", {}).get("served"))}
            if isinstance(v.get("locate"), dict) and "ms_per_step" in v["locate"]:       # locate() of the leg's ranges: call time, algorithmic fraction of 8 TB/s
                out[short(k, 40)].update(locate_ms=v["locate"]["ms_per_step"], locate_frac=v["locate"].get("roofline", {}).get("frac"))
    return out


def compact_line(full):
    """The stdout line: the contract's keys and, from a --full run, `roofline`, `cpu_baseline` and one number per secondary; everything
    else lives in bench_full.json (and on stderr).  Kept under LINE_LIMIT bytes by construction, and by dropping secondaries if it is not."""
    out = pick(full, "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    cfg = dict(full["config"])
    for k in ("single_block_bytes", "block_bytes", "wide_seed_entries_hit", "found"):        # (in bench_full.json)
        cfg.pop(k, None)
    cfg["workload"] = short(cfg["workload"], 250)
    cfg["parallelism"] = short(cfg.get("parallelism", ""), 160)
    out["config"] = cfg
    if "roofline" in full:                  # (--full runs)
        rf = dict(full["roofline"])
        for k in ("working_set_note", "traffic_source_note", "traffic_GBps", "traffic_frac_of_measured_hbm_rate", "traffic_lookup", "requests_per_distinct_line"):
            rf.pop(k, None)
        if "request_rate" in rf:
            rf["request_rate"] = {k: v for k, v in rf["request_rate"].items() if k != "ceiling_source"}
        out["roofline"] = rf
    if "value_at_reference_footprint" in full:
        out["value_at_reference_footprint"] = {k: v for k, v in full["value_at_reference_footprint"].items() if k != "note"}
    if "cpu_baseline" in full:
        cb = dict(full["cpu_baseline"])
        if "sample" in cb:
            cb["sample"] = short(cb["sample"], 110)
        if "error" in cb:
            cb["error"] = short(cb["error"], 200)
        out["cpu_baseline"] = cb
    if "multi_gpu" in full:
        mg = full["multi_gpu"]
        out["multi_gpu"] = pick(mg, "backend", "wire_bytes_per_query", "bytes_into_root_per_step", "rccl_ranks", "gathered_shards_verified", "slowest_kernel_ms",
                                "root_gather_ms", "root_gather_hidden_frac", "root_ingest_GBps", "asserted")
        if mg.get("problems"):
            out["multi_gpu"]["problems"] = [short(x, 140) for x in mg["problems"]]
        out["multi_gpu"]["gather"] = short(mg.get("gather", ""), 100)
        out["multi_gpu"]["kernel_ms_per_rank"] = [round(x["kernel_ms"], 3) for x in mg.get("per_rank", [])]
    out["full"] = os.path.basename(full.get("full_json") or "")
    sec = {}
    for key, leg in full.items():
        if key in out or key in ("device", "full_json", "errors"):
            continue
        sec[key] = one_number(key, leg)
    if full.get("errors"):
        sec["errors"] = [short(e, 100) for e in full["errors"]][:4]
    out["secondary"] = sec
    out = rounded(out, keep=("value", "ms_per_step"))
    line = json.dumps(out, allow_nan=False)
    while len(line) >= LINE_LIMIT and out["secondary"]:
        out["secondary"].pop(max(out["secondary"], key=lambda k: len(json.dumps(out["secondary"][k]))))
        out["secondary_dropped_for_size"] = True
        line = json.dumps(out, allow_nan=False)
    return line


def rounded(o, keep=()):
    """Six significant digits for everything but the keys named (the line is for reading; bench_full.json keeps full precision)."""
    if isinstance(o, float):
        return float(f"{o:.6g}")
    if isinstance(o, dict):
        return {k: (v if k in keep else rounded(v)) for k, v in o.items()}
    if isinstance(o, list):
        return [rounded(v) for v in o]
    return o


def finite(o):
    """NaN / inf never reach the line (strict JSON): replaced by None."""
    if isinstance(o, float):
        return o if o == o and o not in (float("inf"), float("-inf")) else None
    if isinstance(o, dict):
        return {str(k): finite(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [finite(v) for v in o]
    if isinstance(o, np.generic):
        return finite(o.item())
    return o


class Emitter:
    """Owns the result object from the moment the headline exists.  Every later leg runs under leg(): an exception becomes
    {"error": ...} under the leg's key; after each leg the full object is checkpointed to --full-json.  emit() prints the
    compact line exactly once -- at the normal end, from main()'s `finally` on any exception after the headline, or from the
    SIGTERM watcher thread (a launcher tearing the job down while the main thread sits in a collective)."""

    def __init__(self, args, rank):
        import threading
        self.args, self.rank, self.result, self.done, self.current = args, rank, None, False, None
        self.exit_code = 0                  # set by a check that must fail the run AFTER the line has been printed
        self.lock = threading.Lock()
        if rank == 0:
            self._watch_sigterm()

    def _watch_sigterm(self):
        import signal
        import socket
        import threading
        try:
            rd, wr = socket.socketpair()
            wr.setblocking(False)
            # (the wake-up fd is written at C level, whatever the main thread is blocked in.  SIGSEGV / SIGBUS / SIGFPE / SIGABRT too: a
            # crash inside a library call -- which runs without the interpreter lock -- leaves the watcher thread free to print the
            # line before the process dies; a crash that holds the lock still loses it)
            fatal = [signal.SIGSEGV, signal.SIGBUS, signal.SIGFPE, signal.SIGABRT]
            for sig in [signal.SIGTERM] + fatal:
                signal.signal(sig, lambda *_: None)
            signal.set_wakeup_fd(wr.fileno(), warn_on_full_buffer=False)
        except (ValueError, OSError):
            return
        self._sockets = (rd, wr)

        def watch():
            while True:
                data = rd.recv(16)
                if not data:
                    return
                hit = [sig for sig in (signal.SIGTERM, signal.SIGSEGV, signal.SIGBUS, signal.SIGFPE, signal.SIGABRT) if int(sig) in data]
                if hit:
                    if self.result is not None:
                        self.result.setdefault("errors", []).append(f"{hit[0].name} in leg {self.current or '?'}: the legs after it did not run")
                        if self.current and self.current not in self.result:
                            self.result[self.current] = {"error": f"{hit[0].name} (the process was ended by the signal)"}
                    self.emit()
                    os._exit(128 + int(hit[0]))
        threading.Thread(target=watch, daemon=True).start()

    def headline(self, result):
        self.result = result
        if result is not None:
            result["full_json"] = self.args.full_json
            self.checkpoint()

    def checkpoint(self):
        if self.result is None or not self.args.full_json:
            return
        try:
            tmp = self.args.full_json + ".tmp"
            with open(tmp, "w") as f:
                json.dump(finite(self.result), f, allow_nan=False)
            os.replace(tmp, self.args.full_json)
        except OSError as e:
            log(f"could not write {self.args.full_json}: {e}")

    def leg(self, key, fn, keep=True):
        t = time.time()
        self.current = key
        fail = os.environ.get("GCSA2_BENCH_FAIL_LEG", "")           # tests: a leg that raises must not cost the line
        try:
            if fail and fail == key:
                raise RuntimeError(f"GCSA2_BENCH_FAIL_LEG={key}")
            value = fn()
        except Exception as e:
            import traceback
            log(f"leg {key} failed: {traceback.format_exc()}")
            value = {"error": f"{type(e).__name__}: {e}"[:400]}
            if self.result is None:
                raise                                   # not the root: the launcher ends the job, the root's watcher prints the line
            if self.args.gpus > 1:
                self.result[key] = value                # the other ranks are inside this leg's collectives: print what exists, then fail
                self.emit()
                raise
            try:
                import torch
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
            except Exception:
                pass
        if self.result is not None and (keep or (isinstance(value, dict) and "error" in value)):
            self.result[key] = value
            log(f"leg {key}: {time.time() - t:.1f} s")
            self.checkpoint()

    def emit(self):
        with self.lock:
            if self.done or self.result is None:
                return
            self.done = True
            full = finite(self.result)
            self.checkpoint()
            print(json.dumps(full), file=sys.stderr, flush=True)
            line = json.dumps(full, allow_nan=False) if self.args.full_line else compact_line(full)
            print(line, flush=True)


def main():
    args = parse()
    if args.gather_only:
        args.no_secondary = True
    launch_ranks(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (torch.cuda.is_available() is False)")
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("GCSA2_BENCH_BACKEND", "nccl") != "nccl":
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    D = Dist(dev)
    rank, world = D.rank, D.world
    if world != args.gpus:
        raise SystemExit(f"bench.py: world size {world} but --gpus {args.gpus}")
    from gcsa2_amd import binding
    D.make_comm(binding, local_rank)
    D.probe_comm()
    global MEASURED_CEILING
    ceiling = measured_request_ceiling() if (rank == 0 and world == 1 and not args.no_extras) else None
    MEASURED_CEILING = ceiling
    if ceiling is not None:
        log(f"request-rate ceiling of this box: {ceiling:.1f} G dependent random 128-byte fetches/s (gather_bench lds128, 32 GB)")

    if args.workload.startswith("pangenome"):
        wl = setup_pangenome(args, D, dev, local_rank)
    elif args.workload in ("human", "human_snp"):
        wl = setup_human(args, D, dev, local_rank, branching=(args.workload == "human_snp"))
    elif args.workload == "chr22":
        wl = setup_chr22(args, D, dev, local_rank)
    elif args.workload == "repeats":
        wl = setup_repeats(args, D, dev, local_rank)
    elif args.workload == "repeats30":
        wl = setup_repeats30(args, D, dev, local_rank, log2_bases=args.log2_bases or 30)
    else:
        wl = setup_linear(args, D, dev, local_rank)

    emitter = Emitter(args, rank)
    try:
        run_legs(args, D, dev, local_rank, wl, ceiling, emitter)
    finally:
        emitter.emit()
    D.barrier()
    D.close()
    if emitter.exit_code:
        log(f"bench.py: ending with exit code {emitter.exit_code}: {emitter.result.get('multi_gpu', {}).get('problems') if emitter.result else ''}")
        sys.exit(emitter.exit_code)


def run_legs(args, D, dev, local_rank, wl, ceiling, emitter):
    """The headline first -- from then on the line exists and only grows: every other leg runs under emitter.leg(), which
    turns an exception into {"error": ...} under that leg's key and checkpoints bench_full.json."""
    import torch
    rank, world = D.rank, D.world
    r = measure(args, D, dev, wl, args.steps, args.warmup)
    checked = None
    if args.full:
        # every rank checks its own shard; the root also checks everything it gathered
        ok = wl.verify(r["d_out"], wl.first, wl.nq)
        if rank == 0 and r["gathered"] is not None and ok is not None:
            ok = ok and wl.verify(r["gathered"], 0, wl.total_queries)
        checked = None if ok is None else D.all_true(ok)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, r["gathered"] if r["gathered"] is not None else r["d_out"])

    result = None
    if rank == 0:
        size = {"chr22": args.log2_bases or 25, "repeats": args.log2_bases or 23, "repeats30": args.log2_bases or 30, "linear": args.log2_bases or 30}.get(args.workload, getattr(wl, "degree", args.degree))
        result = {
            "metric": "kmer_find_queries_per_sec", "value": wl.total_queries * args.steps / r["elapsed"], "unit": "queries/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": r["elapsed"] / args.steps * 1e3, "higher_is_better": True, "scaling": wl.scaling,
            "vs_baseline": None, "dtype": "u64", "data": "synthetic",
            "config": find_config(wl, r, world),
        }
        if args.full:
            result["roofline"] = roofline(args, r, wl, f"{args.workload}_{size}_{wl.m}_{args.set}")
        result["config"]["pattern_set"] = args.set
        if r["per_rank"] is not None:
            ranks = r["per_rank"]
            result["multi_gpu"] = {
                "launched_by": "bench.py itself (torch.distributed.run child process)" if os.environ.get("GCSA2_BENCH_SELF_LAUNCHED") else "external launcher",
                "backend": D.backend, "gather": r["gather"], "wire_bytes_per_query": r["wire_bytes_per_query"],
                "bytes_into_root_per_step": sum(x["wire_bytes_sent"] for x in ranks),
                "rccl_ranks": ranks[0]["rccl_ranks"],
                "slowest_kernel_ms": max(x["kernel_ms"] for x in ranks), "root_gather_ms": ranks[0]["gather_ms"],
                "root_gather_hidden_frac": ranks[0]["gather_hidden_frac"],
                "gathered_shards_verified": r.get("gathered_shards_verified"),
                "note": "per rank and step, HIP events on the rank's own streams: kernel = k_find2 over the shard; pack = wire format; "
                        "gather = the grouped send / recv (+ unpack on the root) on the second stream, overlapping the next kernel; "
                        "pace = kernel start to kernel start; gather_hidden_frac = 1 - (pace - kernel - pack) / gather",
                "per_rank": ranks}
            mg = result["multi_gpu"]
            mg["gather_only"] = r.get("gather_only")
            if r.get("gather_only"):
                mg["root_ingest_GBps"] = r["gather_only"]["root_ingest_GBps"]
            # The first real N > 1 run explains itself (VERDICT r05 #6 i): the line is printed whatever happens, and the process ends
            # with a non-zero code when the root did not verify every gathered shard, or -- under RCCL -- when the gather did not
            # run through the library's communicator with one rank per GPU (the fallback path is timed and labelled, not passed off).
            problems = []
            if r.get("gathered_shards_verified") != world:
                problems.append(f"gathered_shards_verified = {r.get('gathered_shards_verified')}, expected {world}")
            if D.backend == "nccl" and ranks[0]["rccl_ranks"] != world and not os.environ.get("GCSA2_BENCH_NO_COMM"):      # (the knob asks for the fallback: tests)
                problems.append(f"rccl_ranks = {ranks[0]['rccl_ranks']}, expected {world}: the gather ran as `{r['gather']}`")
            mg["asserted"] = not problems
            if problems:
                mg["problems"] = problems
                emitter.exit_code = 3
        if args.full:
            result["config"]["all_ranges_equal_closed_form"] = checked
        if ceiling is not None:
            result["roofline"]["request_rate"]["ceiling_source"] = "gather_bench --mode lds128 35 on this box, before the index was loaded"
    emitter.headline(result)
    leg = emitter.leg
    if rank == 0 and not args.no_cpu and world == 1:
        leg("cpu_baseline", lambda: cpu_baseline(args, wl, r["d_out"], args.cpu_seconds))
    if rank == 0 and world == 1 and not args.no_extras:
        st = torch.cuda.current_stream()

        def under_load():
            d_tmp = torch.zeros((wl.nq, 2), dtype=torch.int64, device=dev)
            for _ in range(max(1, int(1000 / max(r["kernel_ms"], 0.1)))):
                wl.gpu.find_device(wl.d_pat.data_ptr(), wl.d_off.data_ptr(), wl.nq, d_tmp.data_ptr(), st.cuda_stream)
        leg("device", lambda: device_telemetry(under_load))
        sweep = [tuple(int(x) for x in c.split(":")) for c in args.pipeline_sweep.split(",")] if args.pipeline_sweep else None
        leg("host_batch", lambda: host_batch_rate(wl, r["d_out"], sweep=sweep))
    if rank == 0 and world == 1 and args.workload in ("repeats", "repeats30", "chr22") and wl.gpu.sampleCount() > 0 and (args.locate or not args.no_extras):
        nloc = min(wl.nq, args.locate_ranges or (400_000 if args.workload.startswith("repeats") else wl.nq))
        leg("locate", lambda: measure_locate(wl.gpu, r["d_out"][:nloc].contiguous(), dev, 3)[0])
    secondary = args.workload in ("pangenome", "pangenome_plain", "human") and world == 1 and not args.no_secondary
    if secondary and args.secondary in ("all", "config5") and wl.ix.lcp_size > 0:
        leg("config5", lambda: config5(args, wl, dev))
    if secondary and args.secondary in ("all", "wide") and args.workload.startswith("pangenome") and args.set == "S":
        leg("wide_ranges", lambda: wide_ranges_secondary(args, D, dev, wl))
    if secondary and args.secondary in ("all", "ladder") and args.workload.startswith("pangenome") and args.set == "S":
        leg("memory_ladder", lambda: memory_ladder(args, D, dev, wl, result))        # re-shapes the image: the last user of the headline index
    if world > 1 and not args.no_secondary and args.secondary in ("all", "config5") and D.all_true(wl.ix.lcp_size > 0 and wl.gpu.sampleCount() > 0):
        # (every rank enters the leg; an exception on one rank alone ends the job through the launcher -- the root's line is
        # already safe with the emitter's SIGTERM watcher)
        leg("config5", lambda: config5_sharded(args, D, wl, dev))
    del r
    full_size = getattr(wl, "degree", 0) >= 32
    if secondary:
        leg("release", lambda: release(wl), keep=False)
        del wl
    if secondary and args.secondary in ("all", "chr22"):
        leg("chr22", lambda: chr22_secondary(args, D, dev, local_rank))
    if secondary and args.secondary in ("all", "repeats"):
        leg("repeats", lambda: repeats_secondary(args, D, dev, local_rank))
    if secondary and args.secondary in ("all", "repeats30"):
        # the repeat-rich text at HBM footprint; scaled down with the headline index in small runs (tests)
        leg("repeats_hbm", lambda: repeats_hbm_secondary(args, D, dev, local_rank, log2_bases=(30 if full_size else 22)))
    if secondary and args.workload != "human" and args.secondary == "human32" and full_size:       # rounds 1-2's headline, on request only
        leg("human32", lambda: human32_secondary(args, D, dev, local_rank))
    if secondary and args.secondary == "human_snp":
        leg("human_branching", lambda: human_snp_secondary(args, D, dev, local_rank))
    if rank == 0 and world == 1 and not args.no_extras and not args.no_measured_traffic and result is not None:
        # roofline.traffic MEASURED in this run when the box has a profiler; the last leg: the child builds the
        # index again, so this process gives its own image back first
        if not secondary:
            leg("release", lambda: release(wl), keep=False)
        nq_headline = result["config"]["queries_per_gpu"]

        def traffic_leg():
            seen = measured_traffic(args, nq_headline)
            if seen is None:
                return {"source": "lookup", "note": "no rocprofv3 on this box, or the counter pass failed: roofline.traffic is the committed lookup"}
            return dict(apply_measured_traffic(result, seen), source="measured")
        leg("traffic_measured", traffic_leg)


if __name__ == "__main__":
    main()
