"""The jump table (memoised forced LF chains, 16 bytes per path node) on find-only images: built by default there and
nowhere else, by either of two builders with identical output, last in the order under a memory budget; find() returns
exactly the oracle's ranges through every entry point that reaches k_find2."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from workload import graphs
from workload.brute_builder import build
from workload.rng import SplitMix64
from gcsa2_amd.hostview import concat_patterns
from test_oracle import CASES, random_patterns, truncate_at_sink

FIND_ONLY = dict(with_samples=False, with_counters=False, with_lcp=False)
ENV = ("GCSA2_JUMP_TABLE", "GCSA2_JUMP_BUILD", "GCSA2_KMER_TABLE", "GCSA2_PAIR_BLOCKS", "GCSA2_MEMORY_BUDGET_MB")


@pytest.fixture(scope="module")
def engine():
    from gcsa2_amd import binding
    assert binding.device_count() >= 1, "no MI355X visible"
    return binding


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def chain_patterns(cpu, walks, seed):
    """The pattern set of the parity tests.  The backward search reads a pattern from its end; `s` below is the number of
    characters after which the range of a walk is a single node, the point from which forced chains can be followed."""
    rng = SplitMix64(seed)
    walks = [w for w in walks if len(w) > 0]
    pats = list(walks)
    # s of every walk: the ranges of all its suffixes, in one oracle batch
    suffixes = [w[len(w) - s:] for w in walks for s in range(1, len(w) + 1)]
    data, off = concat_patterns(suffixes)
    ranges = cpu.find_batch(data, off)
    at = 0
    for w in walks:
        single = [s for s in range(1, len(w) + 1) if ranges[at + s - 1][0] == ranges[at + s - 1][1]]
        at += len(w)
        if not single:
            continue
        s = single[0]
        for d in range(10):
            k = len(w) - 1 - s - d                      # the character read d steps after the range became one node
            if k >= 0:
                other = bytes(c for c in b"ACGT" if c != w[k])
                pats.append(w[:k] + bytes([other[rng.below(len(other))]]) + w[k + 1:])      # leaves the chain after d labels
                pats.append(w[k:])                                                          # ends d + 1 characters into it
        if len(w) > 2:
            k = rng.below(len(w))
            pats.append(w[:k] + b"N" + w[k + 1:])
    pats += [bytes(b"ACGTN"[rng.below(5)] for _ in range(1 + rng.below(20))) for _ in range(300)]
    return pats + [b"", b"N", b"A"]


def graph_cases():
    """(name, index arrays, walks of 1..3 x the order): the small definitional graphs, the SNP graph of test_memory_ladder and
    an order-10 de Bruijn graph with junction edges."""
    import torch
    from workload import builder, dbg_torch
    out = []
    for name, g, K in CASES:
        ix = build(g, K, sample_period=8, branching=4)
        out.append((name, ix, [truncate_at_sink(p) for p in random_patterns(g, 3 * K - 2, 0x4A0, 160)]))
    g = graphs.snp_graph(40000, 0xB1, 0xB2, snp_period=12, node_len=16)
    out.append(("snp40000", builder.build(g, 16, sample_period=16, branching=8),
                [truncate_at_sink(p) for p in random_patterns(g, 46, 0x4A1, 240)]))
    ix, dbg = dbg_torch.build_dbg(20, junctions=80, device=torch.device("cuda", 0))
    walks = []
    for m in (10, 13, 20, 30):
        pats = dbg_torch.walk_patterns_device(dbg, 0, 40, m, 0x4A2 + m)[0]
        walks += [bytes(row) for row in pats.cpu().numpy()]
    out.append(("dbg20", ix, walks))
    return out


@pytest.fixture(scope="module")
def prepared(engine):
    """Per graph: the index arrays, the pattern batch and the oracle's ranges, computed once and left unchanged."""
    from oracle.oracle import OracleIndex
    out = []
    for name, ix, walks in graph_cases():
        cpu = OracleIndex(ix, **FIND_ONLY)
        pats = chain_patterns(cpu, walks, 0x4B0 + len(out))
        data, off = concat_patterns(pats)
        out.append((name, ix, data, off, cpu.find_batch(data, off)))
    return out


class DeviceBatch:
    def __init__(self, data, off):
        import torch
        dev = torch.device("cuda", 0)
        self.nq = len(off) - 1
        self.d_pat = torch.zeros(int(off[-1]) + 16, dtype=torch.uint8, device=dev)
        self.d_pat[: int(off[-1])] = torch.from_numpy(np.ascontiguousarray(data[: int(off[-1])])).to(dev)
        self.d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
        self.d_out = torch.zeros((self.nq, 2), dtype=torch.int64, device=dev)
        self.d_stats = torch.zeros(8, dtype=torch.int64, device=dev)

    def run(self, call):
        import torch
        self.d_out.fill_(-7)
        call(self.d_pat.data_ptr(), self.d_off.data_ptr(), self.nq, self.d_out.data_ptr())
        torch.cuda.synchronize()
        return self.d_out.cpu().numpy().view(np.uint64)

    def stats(self, gpu):
        """(ranges, [blocks, steps, lookups, jumps, fetch_steps, second_fetches]) of the instrumented kernel"""
        self.d_stats.zero_()
        got = self.run(lambda p, o, n, r: gpu.find_stats_device(p, o, n, r, self.d_stats.data_ptr(), 0))
        return got, [int(x) for x in self.d_stats.cpu()[:6]]


def test_default_rule(engine, prepared, monkeypatch):
    for name, ix, data, off, want in prepared[:-1]:
        gpu = engine.GCSA(ix, **FIND_ONLY)
        assert gpu.jump_table_bytes() == 16 * ix.n, name
        gpu.close()
        monkeypatch.setenv("GCSA2_JUMP_TABLE", "0")
        off_image = engine.GCSA(ix, **FIND_ONLY)
        sampled_off = engine.GCSA(ix)
        monkeypatch.delenv("GCSA2_JUMP_TABLE")
        assert off_image.jump_table_bytes() == 0, name
        sampled = engine.GCSA(ix)                       # an image with samples: as before
        assert sampled.jump_table_bytes() == 0 and sampled.device_bytes() == sampled_off.device_bytes(), name
        assert sampled.locate_table_bytes() == sampled_off.locate_table_bytes(), name
        for g_ in (off_image, sampled_off, sampled):
            g_.close()
    name, ix, data, off, want = prepared[-1]            # (its arrays hold no samples: the find-only half alone)
    gpu = engine.GCSA(ix, **FIND_ONLY)
    assert gpu.jump_table_bytes() == 16 * ix.n, name
    gpu.close()


@pytest.mark.parametrize("pairs", [None, "0"], ids=["pair-blocks", "single-blocks"])
@pytest.mark.parametrize("kmer", [None, "0"], ids=["seed-table", "no-seed-table"])
def test_parity_on_the_default_image(engine, prepared, monkeypatch, kmer, pairs):
    if kmer is not None:
        monkeypatch.setenv("GCSA2_KMER_TABLE", kmer)
    if pairs is not None:
        monkeypatch.setenv("GCSA2_PAIR_BLOCKS", pairs)
    jumps = 0
    for name, ix, data, off, want in prepared:
        gpu = engine.GCSA(ix, **FIND_ONLY)
        assert gpu.jump_table_bytes() == 16 * ix.n and (gpu.pair_block_bytes() > 0) == (pairs is None), name
        assert kmer is None or gpu.kmer_table_k() == 0, name
        assert np.array_equal(gpu.find_batch(data, off), want), name                       # the host batch path
        batch = DeviceBatch(data, off)
        assert np.array_equal(batch.run(lambda p, o, n, r: gpu.find_device(p, o, n, r, 0)), want), name
        for variant in (2, 4):
            assert np.array_equal(batch.run(lambda p, o, n, r: gpu.find_device_variant(variant, p, o, n, r, 0)), want), (name, variant)
        got, counters = batch.stats(gpu)
        assert np.array_equal(got, want), name
        jumps += counters[3]
        gpu.close()
    assert jumps > 0                                    # the table was consulted


def test_builders_agree(engine, prepared, monkeypatch):
    for name, ix, data, off, want in prepared:
        batch = DeviceBatch(data, off)
        seen = []
        for how in ("double", "walk"):
            monkeypatch.setenv("GCSA2_JUMP_BUILD", how)
            gpu = engine.GCSA(ix, **FIND_ONLY)
            assert gpu.jump_table_bytes() == 16 * ix.n, (name, how)
            assert np.array_equal(gpu.find_batch(data, off), want), (name, how)
            got, counters = batch.stats(gpu)
            assert np.array_equal(got, want), (name, how)
            seen.append(counters)
            gpu.close()
        blocks, steps, lookups, jumps, fetch_steps, second = seen[0]
        assert seen[0] == seen[1], (name, seen)
        assert blocks == fetch_steps + second, (name, seen)


def test_budget(engine, prepared, monkeypatch):
    name, ix, data, off, want = [p for p in prepared if p[0] == "snp40000"][0]
    gpu = engine.GCSA(ix, **FIND_ONLY)
    full, jump_bytes = gpu.device_bytes(), 16 * ix.n
    assert gpu.jump_table_bytes() == jump_bytes and gpu.pair_block_bytes() > 0 and gpu.kmer_table_k() > 0
    gpu.set_tables(pair_blocks=0, kmer_k=0)
    bare = gpu.device_bytes() - jump_bytes
    gpu.close()
    mb = 1048576.0
    seen = []
    for budget in (full + 1, full - jump_bytes // 2, bare // 2):
        monkeypatch.setenv("GCSA2_MEMORY_BUDGET_MB", repr(budget / mb))
        capped = engine.GCSA(ix, **FIND_ONLY)
        monkeypatch.setenv("GCSA2_JUMP_TABLE", "0")
        before = engine.GCSA(ix, **FIND_ONLY)          # what the same cap gave without the table
        monkeypatch.delenv("GCSA2_JUMP_TABLE")
        assert capped.device_bytes() <= max(budget, bare), budget
        assert capped.pair_block_bytes() == before.pair_block_bytes() and capped.kmer_table_k() == before.kmer_table_k(), budget
        assert before.jump_table_bytes() == 0 and capped.device_bytes() == before.device_bytes() + capped.jump_table_bytes(), budget
        assert np.array_equal(capped.find_batch(data, off), want), budget
        seen.append((capped.jump_table_bytes(), capped.pair_block_bytes() > 0, capped.kmer_table_k()))
        capped.close()
        before.close()
    assert seen[0][0] == jump_bytes and seen[0][1] and seen[0][2] > 0, seen
    assert seen[1][0] == 0 and seen[1][1] and seen[1][2] > 0, seen          # the jump table is the first to go
    assert seen[2] == (0, False, 0), seen                                   # below the image itself: no table at all
