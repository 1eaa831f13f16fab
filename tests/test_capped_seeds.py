"""Batched capped seeds (gcsa2_capped_seeds_device / gcsa2_capped_seeds_batch, kernels_seeds.hpp + kernels_mem.hpp): from the
end of every read the match is extended until it has min_length characters and occurs at most max_count times, emitted as a
seed record {position, length, sp, ep, count}, and the search starts again behind it; hits by the rules of the MEM hits.  The
expectation is a Python restatement of the contract's walk (include/gcsa2_hip.h) over the CPU oracle's LF, count and locate
(locate(range, max_positions) above the cap under SAMPLE), cached per distinct range and left unchanged."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from gcsa2_amd.hostview import concat_patterns
from test_oracle import CASES
from test_mem_hits import EDGE, SENTINEL
from test_extend import GRAPHS, BIG, indexed, is_empty
from test_kmer_windows import reads_of
from test_locate_max_batch import reference_spins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
INVALID, MISSING, TOO_SMALL = -1, -5, -6
SKIP, SAMPLE = 0, 1                                     # GCSA2_MEM_OVER_SKIP, GCSA2_MEM_OVER_SAMPLE
HIT_MAX = (0, 1, 3, 64, U64)
GUARD = 64
WORKGROUP = 128                                         # reads per workgroup of the walk
FIXED = ((1, 0, 1), (1, 0, 3), (4, 0, 3), (8, 0, 1), (8, 16, 1), (8, 16, 3), (12, 0, 64), (16, 16, 1), (3, 5, 1), (20, 0, 2))


def grid_of(which):
    """(min_length, max_length, max_count) of the parity grid for one graph: the fixed cases and (K, K, 1) at its order."""
    K = GRAPHS[which][2]
    return FIXED + (((K, K, 1),) if (K, K, 1) not in FIXED else ())


class Spins(Exception):
    """The reference never returns for some sampled seed (count() overstates its distinct values)."""


class Walks:
    """The contract's walk for one batch of reads over the oracle.  LF() per (range, character), count() and the hits per
    range are asked once per index: batches of the same index share them through `like`."""

    def __init__(self, cpu, reads, like=None):
        self.cpu, self.reads = cpu, reads
        self.lf, self.cnt, self.full, self.maxed = (like.lf, like.cnt, like.full, like.maxed) if like is not None else ({}, {}, {}, {})
        self.walked = {}

    def LF(self, r, comp):
        key = (r, comp)
        if key not in self.lf:
            self.lf[key] = self.cpu.LF(r, comp)
        return self.lf[key]

    def count(self, r):
        if r not in self.cnt:
            self.cnt[r] = self.cpu.count(r)
        return self.cnt[r]

    def walk(self, P, min_length, max_length, max_count):
        """One read: (seeds as (position, length, sp, ep, count), LF steps, attempts ended by {empty step, start, cut})."""
        n = self.cpu.n
        seeds, steps, ends = [], 0, {"empty": 0, "start": 0, "cut": 0}
        e = len(P) if n > 0 else 0
        while e > 0:
            r, i, fail, emitted = (0, n - 1), e, None, False
            while True:
                if i == 0:
                    fail = -1
                    ends["start"] += 1
                    break
                if max_length != 0 and e - i == max_length:
                    fail = i - 1
                    ends["cut"] += 1
                    break
                r2 = self.LF(r, int(self.cpu.char2comp[P[i - 1]]))
                steps += 1
                if is_empty(r2):
                    fail = i - 1
                    ends["empty"] += 1
                    break
                i, r = i - 1, r2
                if e - i >= min_length:
                    c = self.count(r)
                    if c <= max_count:
                        seeds.append((i, e - i, r[0], r[1], c))
                        emitted = True
                        break
            e = i if emitted else max(0, min(e - 1, fail + 1))
        return seeds, steps, ends

    def walks(self, params):
        """Per read (seeds, steps, ends) for params = (min_length, max_length, max_count)."""
        if params not in self.walked:
            self.walked[params] = [self.walk(P, *params) for P in self.reads]
        return self.walked[params]

    def seeds(self, params):
        """(seed_offsets, seeds (m, 5))."""
        per_read = [w[0] for w in self.walks(params)]
        soff = np.concatenate([[0], np.cumsum([len(s) for s in per_read])]).astype(np.uint64)
        flat = [s for seeds in per_read for s in seeds]
        return soff, np.asarray(flat, dtype=np.uint64).reshape(-1, 5)

    def hits(self, r, c, hit_max, sample):
        if c == 0:
            return []
        if hit_max == 0 or c <= hit_max:
            if r not in self.full:
                self.full[r] = [int(v) for v in self.cpu.locate(r)]
            return self.full[r]
        if not sample:
            return []
        if (r, hit_max) not in self.maxed:
            if reference_spins(self.cpu, r, hit_max):
                raise Spins(r)
            self.maxed[(r, hit_max)] = [int(v) for v in self.cpu.locate(r, max_positions=hit_max)]
        return self.maxed[(r, hit_max)]

    def want(self, params, hit_max, sample):
        """(seed_offsets, seeds, hit_offsets, hits)."""
        soff, seeds = self.seeds(params)
        per_seed = [self.hits((int(sp), int(ep)), int(c), hit_max, sample) for _, _, sp, ep, c in seeds.tolist()]
        hoff = np.concatenate([[0], np.cumsum([len(h) for h in per_seed])]).astype(np.uint64)
        hits = np.asarray([v for h in per_seed for v in h], dtype=np.uint64)
        return soff, seeds, hoff, hits


@functools.lru_cache(maxsize=None)
def oracle_of(which):
    return Walks(indexed(which)[1], reads_of(which))


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_library_exports_capped_seeds_and_refuses_a_null_index():
    """1. The built library exports both calls and binding.EXPORTS lists them; each refuses a NULL index with INVALID_ARGUMENT
    without a device, names the index and writes nothing."""
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    assert "gcsa2_capped_seeds_device" in binding.EXPORTS and "gcsa2_capped_seeds_batch" in binding.EXPORTS
    for name in ("gcsa2_capped_seeds_device", "gcsa2_capped_seeds_batch"):
        assert hasattr(ctypes.CDLL(binding.LIB_PATH), name), name
    lib = binding.load_library()
    off = (ctypes.c_uint64 * 2)(0, 8)
    pat = (ctypes.c_uint8 * 8)(*b"ACGTACGT")
    soff = (ctypes.c_uint64 * 2)(7, 7)
    seeds = (ctypes.c_uint64 * 25)(*([7] * 25))
    hoff = (ctypes.c_uint64 * 6)(*([7] * 6))
    hits = (ctypes.c_uint64 * 8)(*([7] * 8))
    total_seeds, total_hits = ctypes.c_uint64(7), ctypes.c_uint64(7)
    outputs = (ctypes.addressof(soff), ctypes.addressof(seeds), 5, ctypes.byref(total_seeds), ctypes.addressof(hoff), ctypes.addressof(hits), 8,
               ctypes.byref(total_hits))
    rc = lib.gcsa2_capped_seeds_device(None, ctypes.addressof(pat), ctypes.addressof(off), 1, 4, 0, 1, 0, SKIP, *outputs, None)
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    rc = lib.gcsa2_capped_seeds_batch(None, pat, off, 1, 4, 0, 1, 0, SKIP, *outputs)
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    assert list(soff) == [7, 7] and list(seeds) == [7] * 25 and list(hoff) == [7] * 6 and list(hits) == [7] * 8
    assert total_seeds.value == 7 and total_hits.value == 7


@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_the_restatement_holds_the_contract(which):
    """2. What the header says follows from the walk, on every graph and for the whole grid: each seed's range is find() of
    its substring (non-empty) and its count count() of that range; the seeds of a read do not overlap and come in descending
    position; a read takes at most 2 L LF steps; no seed is shorter than min_length or longer than a non-zero max_length, and
    none is above max_count."""
    oracle = oracle_of(which)
    cpu = oracle.cpu
    found = {}
    for params in grid_of(which):
        min_length, max_length, max_count = params
        for P, (seeds, steps, _) in zip(oracle.reads, oracle.walks(params)):
            assert steps <= 2 * len(P), (params, P, steps)
            end = len(P)
            for position, length, sp, ep, count in seeds:
                assert position + length <= end, (params, P, seeds)                   # below the seed before it: no overlap
                end = position
                assert length >= min_length and (max_length == 0 or length <= max_length) and count <= max_count, (params, P, seeds)
                sub = P[position:position + length]
                if sub not in found:
                    found[sub] = cpu.find(sub)
                assert (sp, ep) == found[sub] and not is_empty((sp, ep)) and count == cpu.count((sp, ep)), (params, P, position, length)
            if len(P) < min_length:
                assert not seeds


def classes(oracle, params):
    """The figures of test 3 for one batch and one grid point."""
    walks = oracle.walks(params)
    seeds = [s for w in walks for s in w[0]]
    return {
        "seeds": len(seeds),
        "at min_length": sum(1 for s in seeds if s[1] == params[0]),
        "longer": sum(1 for s in seeds if s[1] > params[0]),
        "count above 1": sum(1 for s in seeds if s[4] > 1),
        "ended by an empty step": sum(w[2]["empty"] for w in walks),
        "ended at the start": sum(w[2]["start"] for w in walks),
        "cut": sum(w[2]["cut"] for w in walks),
        "long enough without a seed": sum(1 for P, w in zip(oracle.reads, walks) if len(P) >= params[0] and not w[0]),
        "without a seed": sum(1 for w in walks if not w[0]),
        "shorter": sum(1 for P in oracle.reads if len(P) < params[0]),
        "two or more seeds": sum(1 for w in walks if len(w[0]) >= 2),
        "seed at 0": sum(1 for w in walks if w[0] and w[0][-1][0] == 0),
    }


def over_cap(oracle, params, hit_max):
    """The seeds of a grid point above a cap: (how many, their distinct (sp, ep))."""
    seeds = [s for w in oracle.walks(params) for s in w[0] if s[4] > hit_max]
    return len(seeds), sorted({(s[2], s[3]) for s in seeds})


def test_the_batches_are_not_vacuous():
    """3. The batch the GPU tests run on the 6000-base graph holds every class of event the walk has: seeds at exactly
    min_length and longer ones, attempts ended by an empty step, at the read's start and by max_length, reads long enough that
    have no seed, reads that are too short, reads with several seeds and with a seed at position 0, seeds with count > 1, and
    seeds above hit_max for SKIP and SAMPLE to act on -- none of them on a range the reference's sampler would draw forever
    on, so SAMPLE has an expectation everywhere.  The small graphs hold the classes that their 60 reads can."""
    big = oracle_of(BIG)
    got = classes(big, (8, 0, 1))
    print("snp6000 (8,0,1):", got)
    for name in ("seeds", "at min_length", "longer", "ended by an empty step", "ended at the start", "long enough without a seed", "shorter",
                 "two or more seeds", "seed at 0"):
        assert got[name] > 0, name
    got = classes(big, (8, 16, 3))
    print("snp6000 (8,16,3):", got)
    assert got["count above 1"] > 0
    got = classes(big, (3, 5, 1))
    print("snp6000 (3,5,1):", got)
    assert got["cut"] > 0 and got["seeds"] > 0 and got["without a seed"] > 0
    many, distinct = over_cap(big, (1, 0, 3), 1)
    print("snp6000 (1,0,3) above 1:", many, len(distinct))
    assert many > 0 and len(distinct) > 0
    many, _ = over_cap(big, (1, 0, 64), 3)
    print("snp6000 (1,0,64) above 3:", many)
    assert many > 0
    spinning = []
    for params in grid_of(BIG) + ((1, 0, 64), (4, 0, 64)):
        for hit_max in (1, 3):
            spinning += [(params, hit_max, r) for r in over_cap(big, params, hit_max)[1] if reference_spins(big.cpu, r, hit_max)]
    assert len(spinning) == 0, spinning[:3]
    for which in range(len(CASES)):
        small = oracle_of(which)
        got = classes(small, (1, 0, 3))
        print(GRAPHS[which][0], "(1,0,3):", got)
        assert got["seeds"] > 0 and got["two or more seeds"] > 0 and got["ended by an empty step"] > 0 and got["without a seed"] > 0, GRAPHS[which][0]
        K = GRAPHS[which][2]
        got = classes(small, (K, K, 1))
        print(GRAPHS[which][0], (K, K, 1), got)
        assert got["shorter"] > 0 and got["without a seed"] > 0, GRAPHS[which][0]


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine():
    from gcsa2_amd import binding
    assert binding.device_count() >= 1, "no MI355X visible"
    return binding


@pytest.fixture(scope="module")
def big(engine):
    gpu, _ = engine.open_index(indexed(BIG)[0], device=0)
    yield gpu
    gpu.close()


class DeviceReads:
    """A batch of reads in device memory: `lead` bytes of 0xFF, the reads, 8 spare bytes of 0xFF; the offsets start at `lead`."""

    def __init__(self, reads, lead=0):
        import torch
        self.dev = torch.device("cuda", 0)
        data, off = concat_patterns(reads)
        self.n, self.total = len(reads), int(off[-1]) if len(reads) else 0
        self.d_pat = torch.full((lead + self.total + 8,), 0xFF, dtype=torch.uint8, device=self.dev)
        if self.total:
            self.d_pat[lead:lead + self.total] = torch.from_numpy(np.array(data[:self.total], dtype=np.uint8)).to(self.dev)
        self.d_off = torch.from_numpy((np.ascontiguousarray(off).astype(np.uint64) + np.uint64(lead)).view(np.int64).copy()).to(self.dev)

    def seeds(self, gpu, params, hit_max, over, seed_capacity, hit_capacity, null_buffers=False):
        """gcsa2_capped_seeds_device on sentinel-filled buffers with GUARD entries behind every one: (result or Gcsa2Error,
        seed_offsets, seeds, hit_offsets, hits) as numpy, whole buffers (guards included)."""
        import torch
        from gcsa2_amd.binding import Gcsa2Error
        s = np.uint64(SENTINEL).view(np.int64).item()
        d_soff = torch.full((self.n + 1 + GUARD,), s, dtype=torch.int64, device=self.dev)
        d_seeds = torch.full((seed_capacity + GUARD, 5), s, dtype=torch.int64, device=self.dev)
        d_hoff = torch.full((seed_capacity + 1 + GUARD,), s, dtype=torch.int64, device=self.dev)
        d_hits = torch.full((hit_capacity + GUARD,), s, dtype=torch.int64, device=self.dev)
        try:
            res = gpu.capped_seeds_device(self.d_pat.data_ptr(), self.d_off.data_ptr(), self.n, params[0], params[1], params[2], hit_max, over,
                                          d_soff.data_ptr(), 0 if null_buffers else d_seeds.data_ptr(), seed_capacity, d_hoff.data_ptr(),
                                          0 if null_buffers else d_hits.data_ptr(), hit_capacity)
        except Gcsa2Error as e:
            res = e
        torch.cuda.synchronize()
        return (res,) + tuple(t.cpu().numpy().view(np.uint64) for t in (d_soff, d_seeds, d_hoff, d_hits))


def untouched(arrays):
    return all((a == np.uint64(SENTINEL)).all() for a in arrays)


def assert_device(got, want, n, what):
    """A device call's whole buffers against (seed_offsets, seeds, hit_offsets, hits); the guards are intact."""
    res, soff, seeds, hoff, hits = got
    w_soff, w_seeds, w_hoff, w_hits = want
    m, h = w_seeds.shape[0], w_hits.shape[0]
    assert res == (m, h), (what, res, (m, h))
    sentinel = np.uint64(SENTINEL)
    assert np.array_equal(soff[:n + 1], w_soff) and (soff[n + 1:] == sentinel).all(), (what, "seed_offsets")
    bad = np.nonzero((seeds[:m] != w_seeds).any(axis=1))[0]
    assert bad.size == 0, (what, "seeds", int(bad.size), int(bad[0]), seeds[bad[0]].tolist(), w_seeds[bad[0]].tolist())
    assert (seeds[m:] == sentinel).all(), (what, "behind the seeds")
    assert np.array_equal(hoff[:m + 1], w_hoff) and (hoff[m + 1:] == sentinel).all(), (what, "hit_offsets")
    assert np.array_equal(hits[:h], w_hits) and (hits[h:] == sentinel).all(), (what, "hits")


def assert_host(got, want, what):
    for name, a, b in zip(("seed_offsets", "seeds", "hit_offsets", "hits"), got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name, a.shape, b.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_parity_with_the_restatement(engine, which):
    """4. Device form and host form equal the restatement's four arrays and both totals exactly, for the whole grid, every
    cap and both policies.  Where the reference's sampler would draw forever the call passes its refusal through."""
    from gcsa2_amd.binding import Gcsa2Error
    oracle = oracle_of(which)
    reads = oracle.reads
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    seen = 0
    for params in grid_of(which):
        for hit_max in HIT_MAX:
            for sample in (False, True):
                what = (GRAPHS[which][0], params, hit_max, sample)
                try:
                    want = oracle.want(params, hit_max, sample)
                except Spins:
                    assert which != BIG, what
                    with pytest.raises(Gcsa2Error) as err:
                        gpu.capped_seeds_batch(flat, off, *params, hit_max, sample)
                    assert err.value.code == INVALID and "max_positions" in str(err.value), what
                    continue
                m, h = want[1].shape[0], want[3].shape[0]
                seen += m
                assert_device(batch.seeds(gpu, params, hit_max, int(sample), m, h), want, len(reads), what + ("device",))
                assert_host(gpu.capped_seeds_batch(flat, off, *params, hit_max, sample), want, what + ("host",))
    assert seen > 0
    gpu.close()


@pytest.mark.gpu
def test_order_across_wavefronts_and_workgroups(big):
    """5. More than two workgroups' worth of reads whose seed counts differ from read to read, mixed with 200 empty and
    too-short reads: the persistent lanes draw them in whatever order, the records land at their CSR slots, and the guard
    regions behind every buffer stay intact."""
    base = reads_of(BIG)
    filler = [b"", b"ACG", b"A", b"ACGTACG"]
    reads = []
    for q, r in enumerate(base):
        reads.append(r)
        if q < 200:
            reads.append(filler[q % 4])
    params = (8, 0, 1)
    oracle = Walks(indexed(BIG)[1], reads, like=oracle_of(BIG))
    want = oracle.want(params, 1, False)
    per_read = np.diff(want[0].astype(np.int64))
    assert len(reads) > 2 * WORKGROUP and len(set(per_read.tolist())) >= 4 and int((per_read == 0).sum()) >= 200
    assert (per_read[:WORKGROUP].sum() != per_read[WORKGROUP:2 * WORKGROUP].sum())
    m, h = want[1].shape[0], want[3].shape[0]
    assert m > 1000 and h > 0
    assert_device(DeviceReads(reads).seeds(big, params, 1, SKIP, m, h), want, len(reads), "mixed batch")


@pytest.mark.gpu
def test_every_table_shape(engine, big, monkeypatch):
    """6. With and without pair blocks, with the seed table at 0 and its default, and on images made with the jump table asked
    for and not (both without an LCP array): byte for byte the seeds and hits of the default image.  An image without samples
    and counters is refused with nothing written."""
    reads = reads_of(BIG)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    default_k = big.kmer_table_k()
    assert default_k > 1 and big.pair_block_bytes() > 0
    cases = [(params, hit_max, sample) for params in ((8, 0, 1), (1, 0, 3), (16, 16, 1)) for hit_max, sample in ((0, False), (1, True))]
    base = {c: big.capped_seeds_batch(flat, off, *c[0], c[1], c[2]) for c in cases}
    assert all(v[1].shape[0] > 0 and v[3].shape[0] > 0 for v in base.values())

    def compare(gpu, what):
        for c, want in base.items():
            m, h = want[1].shape[0], want[3].shape[0]
            assert_device(batch.seeds(gpu, c[0], c[1], int(c[2]), m, h), want, len(reads), (what, c))

    try:
        for pair_blocks in (1, 0):
            for kmer_k in (0, default_k):
                big.set_tables(pair_blocks=pair_blocks, kmer_k=kmer_k)
                assert (big.pair_block_bytes() > 0) == bool(pair_blocks) and big.kmer_table_k() == kmer_k
                compare(big, (pair_blocks, kmer_k))
    finally:
        big.set_tables(pair_blocks=1, kmer_k=default_k)
    monkeypatch.setenv("GCSA2_JUMP_TABLE", "1")
    jumping = engine.GCSA(indexed(BIG)[0], with_lcp=False)
    find_only = engine.GCSA(indexed(BIG)[0], with_samples=False, with_counters=False, with_lcp=False)
    monkeypatch.setenv("GCSA2_JUMP_TABLE", "0")
    plain = engine.GCSA(indexed(BIG)[0], with_lcp=False)
    monkeypatch.delenv("GCSA2_JUMP_TABLE")
    assert jumping.jump_table_bytes() > 0 and find_only.jump_table_bytes() > 0 and plain.jump_table_bytes() == 0
    compare(jumping, "jump table, no LCP array")
    compare(plain, "no jump table, no LCP array")
    got = batch.seeds(find_only, (8, 0, 1), 0, SKIP, 64, 64)
    assert got[0].code == MISSING and untouched(got[1:]), got[0]
    for gpu in (jumping, plain, find_only):
        gpu.close()


@pytest.mark.gpu
def test_read_edges(big):
    """7. Reads of length 0, 1, min_length - 1, min_length and min_length + 1; a read of only N; a read whose last character is
    not in the index; a read that matches whole and stays above max_count, which ends at the read's start without a seed;
    max_length == min_length; and, in the device form, a pattern buffer whose first offset is not 0."""
    cpu = indexed(BIG)[1]
    walk = next(r for r in reads_of(BIG)[:100] if len(r) >= 40)
    frequent = walk[10:14]
    reads = [b"", walk[:1], walk[:7], walk[:8], walk[:9], walk[-7:], walk[-8:], walk[-9:], b"N" * 20, walk[:30] + b"X", walk[:30] + b"N", frequent, walk]
    oracle = Walks(cpu, reads, like=oracle_of(BIG))
    assert not is_empty(cpu.find(frequent)) and cpu.count(cpu.find(frequent)) > 1
    seeds, _, ends = oracle.walk(frequent, 2, 0, 1)
    assert not seeds and ends == {"empty": 0, "start": 1, "cut": 0}                 # one attempt, which runs into the read's start
    assert oracle.walk(walk[:30] + b"X", 8, 0, 1)[2]["empty"] > 0 and not oracle.walk(b"N" * 20, 8, 0, 1)[0]
    assert oracle.walk(walk[:8], 8, 0, 64)[0] and not oracle.walk(walk[:7], 8, 0, 64)[0]
    flat, off = concat_patterns(reads)
    for lead in (0, 37):
        batch = DeviceReads(reads, lead=lead)
        for params in ((8, 0, 1), (8, 0, 64), (8, 8, 1), (2, 0, 1), (1, 1, 64), (9, 0, 3)):
            for hit_max, over in ((0, SKIP), (1, SAMPLE)):
                want = oracle.want(params, hit_max, bool(over))
                m, h = want[1].shape[0], want[3].shape[0]
                assert_device(batch.seeds(big, params, hit_max, over, m, h), want, len(reads), (lead, params, hit_max, over))
                if lead == 0:
                    assert_host(big.capped_seeds_batch(flat, off, *params, hit_max, bool(over)), want, (params, hit_max, over, "host"))
    assert all(s[1] == 8 for s in oracle.seeds((8, 8, 1))[1].tolist()) and oracle.seeds((8, 8, 1))[1].shape[0] > 0


def host_call(gpu, reads, params, hit_max, over, seed_capacity, hit_capacity, null_index=False, null_totals=False):
    """gcsa2_capped_seeds_batch on sentinel-filled numpy buffers: (status, (seeds, hits), seed_offsets, seeds, hit_offsets,
    hits)."""
    data, off = concat_patterns(reads)
    data, off = np.ascontiguousarray(data, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64)
    n = len(reads)

    def buf(*shape):
        return np.full(shape, SENTINEL, dtype=np.uint64)

    soff, seeds, hoff, hits = buf(n + 1 + GUARD), buf(seed_capacity + GUARD, 5), buf(seed_capacity + 1 + GUARD), buf(hit_capacity + GUARD)
    total_seeds, total_hits = ctypes.c_uint64(SENTINEL), ctypes.c_uint64(SENTINEL)
    rc = gpu._L.gcsa2_capped_seeds_batch(None if null_index else gpu._h, data.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                         off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n, params[0], params[1], params[2], hit_max, over,
                                         soff.ctypes.data, seeds.ctypes.data, seed_capacity, None if null_totals else ctypes.byref(total_seeds),
                                         hoff.ctypes.data, hits.ctypes.data, hit_capacity, ctypes.byref(total_hits))
    return rc, (total_seeds.value, total_hits.value), soff, seeds, hoff, hits


@pytest.mark.gpu
def test_capacities_and_nulls(engine, big):
    """8. Exact capacities are filled and nothing lies behind them; the sizing call with NULL buffers, and one record or one hit
    short, are refused with both totals and nothing written; empty batches and batches without a seed are fine; every invalid
    argument is refused with nothing written, the totals included; an image without samples is refused, one without the LCP
    array answers."""
    reads = reads_of(BIG)[90:130] + EDGE
    n = len(reads)
    oracle = Walks(indexed(BIG)[1], reads, like=oracle_of(BIG))
    batch = DeviceReads(reads)
    for params, hit_max, over in (((8, 0, 1), 0, SKIP), ((1, 0, 3), 1, SAMPLE)):
        want = oracle.want(params, hit_max, bool(over))
        m, h = want[1].shape[0], want[3].shape[0]
        assert m > 0 and h > 0
        what = (params, hit_max, over)
        assert_device(batch.seeds(big, params, hit_max, over, m, h), want, n, what + ("exact",))
        rc, totals, *arrays = host_call(big, reads, params, hit_max, over, m, h)
        assert rc == 0
        assert_device(((totals[0], totals[1]),) + tuple(arrays), want, n, what + ("exact, host",))
        got = batch.seeds(big, params, hit_max, over, 0, 0, null_buffers=True)
        assert got[0].code == TOO_SMALL and got[0].needed == (m, h) and untouched(got[1:]), what + ("sizing",)
        for mcap, hcap in ((m - 1, h), (m, h - 1), (m - 1, h - 1), (0, 0)):
            got = batch.seeds(big, params, hit_max, over, mcap, hcap)
            assert got[0].code == TOO_SMALL and got[0].needed == (m, h), what + (mcap, hcap)
            assert untouched(got[1:]), what + (mcap, hcap)
            rc, totals, *arrays = host_call(big, reads, params, hit_max, over, mcap, hcap)
            assert rc == TOO_SMALL and totals == (m, h) and untouched(arrays), what + (mcap, hcap, "host")
    # no reads at all; reads all shorter than min_length; reads without any seed
    sentinel = np.uint64(SENTINEL)
    for some, params in (([], (16, 0, 1)), ([b"ACGT", b"", b"ACGTACG", b"A"], (8, 0, 1)), ([b"NNNN", b"XYZ", b"NNNN", b""], (2, 0, 1)), ([b"NNNN", b"XYZ"], (1, 1, 64))):
        nn = len(some)
        res, soff, seeds, hoff, hits = DeviceReads(some).seeds(big, params, 3, SAMPLE, 4, 4)
        assert res == (0, 0), (some, params)
        assert (soff[:nn + 1] == 0).all() and (soff[nn + 1:] == sentinel).all() and int(hoff[0]) == 0 and (hoff[1:] == sentinel).all()
        assert untouched([seeds, hits])
        rc, totals, soff, seeds, hoff, hits = host_call(big, some, params, 3, SAMPLE, 4, 4)
        assert rc == 0 and totals == (0, 0), (some, params)
        assert (soff[:nn + 1] == 0).all() and (soff[nn + 1:] == sentinel).all() and int(hoff[0]) == 0 and (hoff[1:] == sentinel).all()
        assert untouched([seeds, hits])
        got = big.capped_seeds_batch(*concat_patterns(some), *params, 3, True)
        assert got[0].tolist() == [0] * (nn + 1) and got[1].shape == (0, 5) and got[2].tolist() == [0] and got[3].shape == (0,)
    # invalid arguments: min_length 0, max_count 0, min_length above max_length, an unknown policy
    for params, over in (((0, 0, 1), SKIP), ((4, 0, 0), SKIP), ((9, 8, 1), SKIP), ((4, 0, 1), 7)):
        got = batch.seeds(big, params, 0, over, 64, 64)
        assert got[0].code == INVALID and got[0].needed == (0, 0) and untouched(got[1:]), (params, over)
        rc, totals, *arrays = host_call(big, reads, params, 0, over, 64, 64)
        assert rc == INVALID and totals == (SENTINEL, SENTINEL) and untouched(arrays), (params, over)
    rc, totals, *arrays = host_call(big, reads, (4, 0, 1), 0, SKIP, 64, 64, null_index=True)
    assert rc == INVALID and totals == (SENTINEL, SENTINEL) and untouched(arrays)
    rc, totals, *arrays = host_call(big, reads, (4, 0, 1), 0, SKIP, 64, 64, null_totals=True)
    assert rc == INVALID and totals[1] == SENTINEL and untouched(arrays)
    # the host form refuses offsets that do not start at 0 or decrease
    for bad in ([1, 20, 40], [0, 40, 20]):
        off = np.asarray(bad, dtype=np.uint64)
        out = np.full(64, SENTINEL, dtype=np.uint64)
        totals = (ctypes.c_uint64(SENTINEL), ctypes.c_uint64(SENTINEL))
        rc = big._L.gcsa2_capped_seeds_batch(big._h, np.zeros(64, dtype=np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                             off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 2, 4, 0, 1, 0, SKIP, out.ctypes.data,
                                             out[8:].ctypes.data, 1, ctypes.byref(totals[0]), out[16:].ctypes.data, out[24:].ctypes.data, 1,
                                             ctypes.byref(totals[1]))
        assert rc == INVALID and untouched([out]), bad
    # components: no samples -> refused; no LCP array -> the same answer
    want = oracle.want((8, 0, 1), 0, False)
    m, h = want[1].shape[0], want[3].shape[0]
    bare = engine.GCSA(indexed(BIG)[0], with_samples=False, with_lcp=False)
    got = batch.seeds(bare, (8, 0, 1), 0, SKIP, m, h)
    assert got[0].code == MISSING and untouched(got[1:]), got[0]
    bare.close()
    no_lcp = engine.GCSA(indexed(BIG)[0], with_lcp=False)
    assert_device(batch.seeds(no_lcp, (8, 0, 1), 0, SKIP, m, h), want, n, "no LCP array")
    no_lcp.close()


@pytest.mark.gpu
def test_composition(big):
    """9. For 200 seeds: find() of the substring gives the range; extend_batch from the root over [position, position + length)
    matches every character and ends with the same range; count_batch gives the count; locate_batch gives the hits of the seeds
    under the cap.  The seed CSR goes into sub_mem_hits_batch as it is and gives what the same records built by hand give."""
    import torch
    reads = reads_of(BIG)
    flat, off = concat_patterns(reads)
    params, hit_max = (8, 0, 3), 2
    soff, seeds, hoff, hits = big.capped_seeds_batch(flat, off, *params, hit_max, False)
    owner = np.repeat(np.arange(len(reads)), np.diff(soff.astype(np.int64)))
    over = seeds[:, 4] > np.uint64(hit_max)
    some_over, all_under = np.nonzero(over)[0][:40], np.nonzero(~over)[0]
    pick = np.sort(np.concatenate([some_over, all_under[np.linspace(0, all_under.size - 1, 200 - some_over.size).astype(np.int64)]]))
    assert seeds.shape[0] > 200 and len(set(pick.tolist())) == 200
    subs = [reads[owner[i]][int(seeds[i, 0]):int(seeds[i, 0] + seeds[i, 1])] for i in pick]
    assert all(len(s) == int(seeds[i, 1]) for s, i in zip(subs, pick))
    batch = DeviceReads(subs)
    d_ranges = torch.zeros((len(subs), 2), dtype=torch.int64, device=batch.dev)
    big.find_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), len(subs), d_ranges.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_ranges.cpu().numpy().view(np.uint64), seeds[pick, 2:4])
    n = indexed(BIG)[0].n
    states = np.asarray([(owner[i], seeds[i, 0], seeds[i, 0] + seeds[i, 1], 0, n - 1) for i in pick], dtype=np.uint64)
    ext = big.extend_batch(flat, off, states)
    assert np.array_equal(ext[:, 0], seeds[pick, 1]) and np.array_equal(ext[:, 1:3], seeds[pick, 2:4]) and np.array_equal(ext[:, 3:5], seeds[pick, 2:4])
    assert np.array_equal(big.count_batch(seeds[pick, 2:4].copy()), seeds[pick, 4])
    under = pick[seeds[pick, 4] <= np.uint64(hit_max)]
    above = pick[seeds[pick, 4] > np.uint64(hit_max)]
    assert under.size > 0 and above.size > 0
    lo, lv = big.locate_batch(seeds[under, 2:4].copy())
    for j, i in enumerate(under.tolist()):
        assert np.array_equal(hits[int(hoff[i]):int(hoff[i + 1])], lv[int(lo[j]):int(lo[j + 1])]), i
    assert all(int(hoff[i + 1]) == int(hoff[i]) for i in above.tolist())
    hand = np.zeros((seeds.shape[0], 5), dtype=np.uint64)
    every = [reads[owner[i]][int(seeds[i, 0]):int(seeds[i, 0] + seeds[i, 1])] for i in range(seeds.shape[0])]
    hand[:, 0], hand[:, 1] = seeds[:, 0], [len(s) for s in every]
    hand[:, 2:4] = big.find_batch(*concat_patterns(every))
    hand[:, 4] = big.count_batch(hand[:, 2:4].copy())
    hand_off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=len(reads)))]).astype(np.uint64)
    assert np.array_equal(hand, seeds) and np.array_equal(hand_off, soff)
    got = big.sub_mem_hits_batch(flat, off, soff, seeds, 4, 8, 0, False)
    want = big.sub_mem_hits_batch(flat, off, hand_off, hand, 4, 8, 0, False)
    assert got[1].shape[0] > 0 and got[3].shape[0] > 0
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_host_form_in_pieces(engine, monkeypatch):
    """10. The batch of the 6000-base graph, repeated until it is 3 MB of reads (the smallest piece is 1 MB), in 1 MB pieces
    equals the same batch in one piece, and its first repetition the batch alone -- which test 4 holds against the device form
    and the restatement.  Library against library."""
    ix = indexed(BIG)[0]
    whole, _ = engine.open_index(ix, device=0)
    monkeypatch.setenv("GCSA2_MS_PIECE_MB", "1")
    pieced, _ = engine.open_index(ix, device=0)
    once = reads_of(BIG)
    repeats = (3 << 20) // sum(len(r) for r in once) + 1
    reads = once * repeats
    flat, off = concat_patterns(reads)
    assert int(off[-1]) >= 3 << 20                      # a piece holds at most 1 MB of reads, so cut_pieces yields at least 3
    alone = whole.capped_seeds_batch(*concat_patterns(once), 8, 0, 3, 2, True)
    for params, hit_max, sample in (((8, 0, 3), 2, True), ((12, 16, 1), 0, False)):
        a = pieced.capped_seeds_batch(flat, off, *params, hit_max, sample)
        b = whole.capped_seeds_batch(flat, off, *params, hit_max, sample)
        assert_host(a, b, (params, hit_max, sample))
        assert a[1].shape[0] > 0 and a[3].shape[0] > 0
    a = pieced.capped_seeds_batch(flat, off, 8, 0, 3, 2, True)
    m, h, n = alone[1].shape[0], alone[3].shape[0], len(once)
    assert a[1].shape[0] == repeats * m and a[3].shape[0] == repeats * h
    assert_host((a[0][:n + 1], a[1][:m], a[2][:m + 1], a[3][:h]), alone, "first repetition")
    # too small in pieces: refused with both totals
    from gcsa2_amd.binding import Gcsa2Error
    with pytest.raises(Gcsa2Error) as err:
        pieced.capped_seeds_batch(flat, off, 8, 0, 3, 2, True, out=(np.zeros(len(reads) + 1, dtype=np.uint64), np.zeros((repeats * m - 1, 5), dtype=np.uint64),
                                                                   np.zeros(repeats * m, dtype=np.uint64), np.zeros(repeats * h, dtype=np.uint64)))
    assert err.value.code == TOO_SMALL and err.value.needed == (repeats * m, repeats * h)
    pieced.close()
    whole.close()


@pytest.mark.gpu
def test_facade_capped_seeds(engine, tmp_path):
    """11. GCSA::capped_seeds_batch from a C++ client (tests/cpp/capped_seeds_client.cpp) prints what GCSA.capped_seeds_batch
    returns."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    which = len(CASES) - 1
    reads = reads_of(which)
    assert all(b"\n" not in r for r in reads)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    save_host_view(indexed(which)[0], str(tmp_path / "index.g2hv"))
    (tmp_path / "reads.txt").write_bytes(b"".join(r + b"\n" for r in reads))
    exe = compile_client(str(tmp_path / "capped_seeds_client"), os.path.join(ROOT, "tests", "cpp", "capped_seeds_client.cpp"))
    data, off = concat_patterns(reads)
    for min_length, max_length, max_count, hit_max, sample in ((1, 0, 3, 0, 0), (3, 5, 1, 0, 0), (1, 0, 3, 1, 1)):
        out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "reads.txt"), str(min_length), str(max_length), str(max_count),
                              str(hit_max), str(sample)], capture_output=True, text=True, env=_run_env(), timeout=300)
        assert out.returncode == 0, out.stderr
        soff, seeds, hoff, hits = gpu.capped_seeds_batch(data, off, min_length, max_length, max_count, hit_max, bool(sample))
        want = [f"read {q} {int(soff[q + 1] - soff[q])}" for q in range(len(reads))]
        want += [f"seed {i} " + " ".join(str(int(x)) for x in seeds[i]) for i in range(seeds.shape[0])]
        want += [" ".join(["hits", str(i), str(int(hoff[i + 1] - hoff[i]))] + [str(int(v)) for v in hits[int(hoff[i]):int(hoff[i + 1])]])
                 for i in range(seeds.shape[0])]
        assert out.stdout.strip().split("\n") == want, (min_length, max_length, max_count, hit_max, sample)
        assert seeds.shape[0] > 0 and hits.shape[0] > 0
    gpu.close()
