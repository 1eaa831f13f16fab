"""Batched k-mer hits (gcsa2_kmer_hits_device / gcsa2_kmer_hits_batch, kernels_windows.hpp + kernels_mem.hpp): the windows
P_q[j stride, j stride + k) of every read that find() finds, compacted in read order as seed records {position, length, sp, ep,
count}, with their hits by the rules of the MEM hits.  The expectations are the CPU oracle's alone: find() and count() of every
materialised window (test_kmer_windows.Expected, once per graph and window length), locate(range) up to the cap and
locate(range, max_positions) above it under SAMPLE, cached per distinct range and left unchanged."""
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
from test_kmer_windows import reads_of, Expected, window_count
from test_locate_max_batch import reference_spins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
INVALID, MISSING, TOO_SMALL = -1, -5, -6
SKIP, SAMPLE = 0, 1                                     # GCSA2_MEM_OVER_SKIP, GCSA2_MEM_OVER_SAMPLE
SHORT_K = (1, 2, 3, 4, 6, 8)
LONG_K = (12, 16, 24, 32, 33)
HIT_MAX = (0, 1, 3, 64, U64)
GUARD = 64
WAVE, WORKGROUP = 64, 128                               # windows per wavefront and per workgroup of the search kernel


def all_k(kmer_k):
    """The window lengths of the parity grid for an image whose seed table has kmer_k."""
    return sorted(set(SHORT_K) | set(LONG_K) | {k for k in (kmer_k - 1, kmer_k, kmer_k + 1) if k >= 1})


class Spins(Exception):
    """The reference never returns for some sampled seed (count() overstates its distinct values)."""


class Seeds:
    """The contract's four arrays (and the profiles) for one batch of reads, from the oracle."""

    def __init__(self, cpu, reads):
        self.cpu, self.reads = cpu, reads
        self.exp = Expected(cpu, reads)
        self.full, self.maxed, self.cut = {}, {}, {}

    def windows(self, k, stride):
        """Of the (k, stride) windows: profiles, the seed records, the seed offsets, and per seed the index of its range among
        the distinct ones."""
        if (k, stride) not in self.cut:
            woff, prof, rng, cnt = self.exp.want(k, stride)
            per_read = np.diff(woff.astype(np.int64))
            position = (np.arange(int(woff[-1]), dtype=np.int64) - np.repeat(woff[:-1].astype(np.int64), per_read)) * stride
            nonempty = ((rng[:, 0] + np.uint64(1)) <= (rng[:, 1] + np.uint64(1))) if rng.shape[0] else np.zeros(0, dtype=bool)
            assert [bool(x) for x in nonempty[:64]] == [not is_empty((int(a), int(b))) for a, b in rng[:64].tolist()]
            seeds = np.zeros((int(nonempty.sum()), 5), dtype=np.uint64)
            seeds[:, 0] = position[nonempty]
            seeds[:, 1] = k
            seeds[:, 2:4] = rng[nonempty]
            seeds[:, 4] = cnt[nonempty]
            soff = np.concatenate([[0], np.cumsum(prof[:, 1].astype(np.int64))]).astype(np.uint64)
            assert int(soff[-1]) == seeds.shape[0]
            distinct, inverse = (np.unique(seeds[:, 2:5], axis=0, return_inverse=True) if seeds.shape[0]
                                 else (np.zeros((0, 3), dtype=np.uint64), np.zeros(0, dtype=np.int64)))
            self.cut[(k, stride)] = (prof, seeds, soff, distinct, np.asarray(inverse).reshape(-1))
        return self.cut[(k, stride)]

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

    def want(self, k, stride, hit_max, sample):
        """(seed_offsets, seeds, hit_offsets, hits, profiles)."""
        prof, seeds, soff, distinct, inverse = self.windows(k, stride)
        per_range = [np.asarray(self.hits((int(sp), int(ep)), int(c), hit_max, sample), dtype=np.uint64) for sp, ep, c in distinct.tolist()]
        sizes = np.asarray([a.shape[0] for a in per_range], dtype=np.int64)[inverse] if seeds.shape[0] else np.zeros(0, dtype=np.int64)
        hoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        hits = np.concatenate([per_range[i] for i in inverse.tolist()] + [np.zeros(0, dtype=np.uint64)]).astype(np.uint64)
        return soff, seeds, hoff, hits, prof


@functools.lru_cache(maxsize=None)
def oracle_of(which):
    return Seeds(indexed(which)[1], reads_of(which))


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_library_exports_kmer_hits_and_refuses_a_null_index():
    """1. The built library exports both calls; each refuses a NULL index with INVALID_ARGUMENT without a device, names the
    index and writes nothing."""
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    assert "gcsa2_kmer_hits_device" in binding.EXPORTS and "gcsa2_kmer_hits_batch" in binding.EXPORTS
    for name in ("gcsa2_kmer_hits_device", "gcsa2_kmer_hits_batch"):
        assert hasattr(ctypes.CDLL(binding.LIB_PATH), name), name
    lib = binding.load_library()
    off = (ctypes.c_uint64 * 2)(0, 8)
    pat = (ctypes.c_uint8 * 8)(*b"ACGTACGT")
    prof = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    soff = (ctypes.c_uint64 * 2)(7, 7)
    seeds = (ctypes.c_uint64 * 25)(*([7] * 25))
    hoff = (ctypes.c_uint64 * 6)(*([7] * 6))
    hits = (ctypes.c_uint64 * 8)(*([7] * 8))
    total_seeds, total_hits = ctypes.c_uint64(7), ctypes.c_uint64(7)
    outputs = (ctypes.addressof(prof), ctypes.addressof(soff), ctypes.addressof(seeds), 5, ctypes.byref(total_seeds), ctypes.addressof(hoff),
               ctypes.addressof(hits), 8, ctypes.byref(total_hits))
    rc = lib.gcsa2_kmer_hits_device(None, ctypes.addressof(pat), ctypes.addressof(off), 1, 4, 1, 0, SKIP, *outputs, None)
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    rc = lib.gcsa2_kmer_hits_batch(None, pat, off, 1, 4, 1, 0, SKIP, *outputs)
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    assert list(prof) == [7] * 4 and list(soff) == [7, 7] and list(seeds) == [7] * 25 and list(hoff) == [7] * 6 and list(hits) == [7] * 8
    assert total_seeds.value == 7 and total_hits.value == 7


def test_the_batches_are_not_vacuous():
    """2. The batch the GPU tests run on the 6000-base graph holds, at stride 1: for every k up to 8, seeds at or below and
    above the caps 1 and 3 (above 64 for k <= 3), windows that are not found, reads of at least k characters without any seed
    and reads shorter than k; for the longer k, found and not found windows.  On every graph no range above a cap of 1, 3 or
    64 is one the reference would draw forever on, so SAMPLE has an expectation everywhere."""
    big = oracle_of(BIG)
    reads = reads_of(BIG)
    for k in SHORT_K + LONG_K:
        prof, seeds, soff, _, _ = big.windows(k, 1)
        windows, found = int(prof[:, 0].sum()), seeds.shape[0]
        assert 0 < found < windows, (k, found, windows)
        if k in SHORT_K:
            counts = seeds[:, 4]
            for hit_max in (1, 3):
                assert int((counts <= np.uint64(hit_max)).sum()) > 0 and int((counts > np.uint64(hit_max)).sum()) > 0, (k, hit_max)
            assert int((counts <= np.uint64(64)).sum()) > 0 and (k > 3 or int((counts > np.uint64(64)).sum()) > 0), k
            per_read = np.diff(soff.astype(np.int64))
            assert any(len(r) >= k and per_read[q] == 0 for q, r in enumerate(reads)), k
            assert any(len(r) < k for r in reads), k
    for which in range(len(GRAPHS)):
        seeds_of = oracle_of(which)
        for k in SHORT_K + LONG_K:
            distinct = seeds_of.windows(k, 1)[3]
            for hit_max in (1, 3, 64):
                spinning = [r for r in distinct.tolist() if r[2] > hit_max and reference_spins(seeds_of.cpu, (r[0], r[1]), hit_max)]
                assert not spinning, (GRAPHS[which][0], k, hit_max, spinning[:3])


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
    """A batch of reads in device memory: the pattern buffer is exactly total + 8 bytes, the spare ones filled with 0xFF."""

    def __init__(self, reads):
        import torch
        self.dev = torch.device("cuda", 0)
        data, off = concat_patterns(reads)
        self.n, self.total = len(reads), int(off[-1]) if len(reads) else 0
        self.d_pat = torch.full((self.total + 8,), 0xFF, dtype=torch.uint8, device=self.dev)
        if self.total:
            self.d_pat[:self.total] = torch.from_numpy(np.ascontiguousarray(data[:self.total])).to(self.dev)
        self.d_off = torch.from_numpy(np.ascontiguousarray(off).view(np.int64).copy()).to(self.dev)

    def hits(self, gpu, k, stride, hit_max, over, seed_capacity, hit_capacity, profiles=True):
        """gcsa2_kmer_hits_device on sentinel-filled buffers with GUARD entries behind every one: (result or Gcsa2Error,
        seed_offsets, seeds, hit_offsets, hits, profiles) as numpy, whole buffers (guards included)."""
        import torch
        from gcsa2_amd.binding import Gcsa2Error
        s = np.uint64(SENTINEL).view(np.int64).item()
        d_prof = torch.full((self.n + GUARD, 4), s, dtype=torch.int64, device=self.dev) if profiles else None
        d_soff = torch.full((self.n + 1 + GUARD,), s, dtype=torch.int64, device=self.dev)
        d_seeds = torch.full((seed_capacity + GUARD, 5), s, dtype=torch.int64, device=self.dev)
        d_hoff = torch.full((seed_capacity + 1 + GUARD,), s, dtype=torch.int64, device=self.dev)
        d_hits = torch.full((hit_capacity + GUARD,), s, dtype=torch.int64, device=self.dev)
        try:
            res = gpu.kmer_hits_device(self.d_pat.data_ptr(), self.d_off.data_ptr(), self.n, k, stride, hit_max, over,
                                       0 if d_prof is None else d_prof.data_ptr(), d_soff.data_ptr(), d_seeds.data_ptr(), seed_capacity,
                                       d_hoff.data_ptr(), d_hits.data_ptr(), hit_capacity)
        except Gcsa2Error as e:
            res = e
        torch.cuda.synchronize()
        return (res,) + tuple(None if t is None else t.cpu().numpy().view(np.uint64) for t in (d_soff, d_seeds, d_hoff, d_hits, d_prof))

    def windows(self, gpu, k, stride):
        """gcsa2_kmer_windows_device with ranges and counts: (window_offsets, profiles, ranges, counts)."""
        import torch
        d_woff = torch.zeros(self.n + 1, dtype=torch.int64, device=self.dev)
        d_prof = torch.zeros((self.n, 4), dtype=torch.int64, device=self.dev)
        total = gpu.kmer_windows_device(self.d_pat.data_ptr(), self.d_off.data_ptr(), self.n, k, stride, 1, d_woff.data_ptr(), 0, 0, 0, 0)
        d_rng = torch.zeros((total, 2), dtype=torch.int64, device=self.dev)
        d_cnt = torch.zeros(total, dtype=torch.int64, device=self.dev)
        assert gpu.kmer_windows_device(self.d_pat.data_ptr(), self.d_off.data_ptr(), self.n, k, stride, 1, 0, d_prof.data_ptr(), d_rng.data_ptr(),
                                       d_cnt.data_ptr(), total) == total
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy().view(np.uint64) for t in (d_woff, d_prof, d_rng, d_cnt))


def untouched(arrays):
    return all((a == np.uint64(SENTINEL)).all() for a in arrays if a is not None)


def assert_device(got, want, n, what):
    """A device call's whole buffers against (seed_offsets, seeds, hit_offsets, hits, profiles); the guards are intact."""
    res, soff, seeds, hoff, hits, prof = got
    w_soff, w_seeds, w_hoff, w_hits, w_prof = want
    m, h = w_seeds.shape[0], w_hits.shape[0]
    assert res == (m, h), (what, res, (m, h))
    sentinel = np.uint64(SENTINEL)
    assert np.array_equal(soff[:n + 1], w_soff) and (soff[n + 1:] == sentinel).all(), (what, "seed_offsets")
    bad = np.nonzero((seeds[:m] != w_seeds).any(axis=1))[0]
    assert bad.size == 0, (what, "seeds", int(bad.size), int(bad[0]), seeds[bad[0]].tolist(), w_seeds[bad[0]].tolist())
    assert (seeds[m:] == sentinel).all(), (what, "behind the seeds")
    assert np.array_equal(hoff[:m + 1], w_hoff) and (hoff[m + 1:] == sentinel).all(), (what, "hit_offsets")
    assert np.array_equal(hits[:h], w_hits) and (hits[h:] == sentinel).all(), (what, "hits")
    if prof is not None:
        bad = np.nonzero((prof[:n] != w_prof).any(axis=1))[0]
        assert bad.size == 0, (what, "profiles", int(bad.size), int(bad[0]), prof[bad[0]].tolist(), w_prof[bad[0]].tolist())
        assert (prof[n:] == sentinel).all(), (what, "behind the profiles")


def assert_host(got, want, what):
    for name, a, b in zip(("seed_offsets", "seeds", "hit_offsets", "hits", "profiles"), got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name, a.shape, b.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_parity_with_the_oracle(engine, which):
    """3. Device form and host form equal the oracle's four arrays exactly, and the profiles those of the k-mer windows, for
    every k, cap and policy at stride 1, and for strides 3 and k + 5 at k = 4 and 16."""
    from gcsa2_amd.binding import Gcsa2Error
    oracle = oracle_of(which)
    reads = reads_of(which)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    if which == BIG:
        assert gpu.kmer_table_k() > 1 and gpu.pair_block_bytes() > 0
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    grid = [(k, 1) for k in all_k(gpu.kmer_table_k())] + [(k, s) for k in (4, 16) for s in (3, k + 5)]
    spun = 0
    for k, stride in grid:
        for hit_max in HIT_MAX:
            for sample in (False, True):
                what = (GRAPHS[which][0], k, stride, hit_max, sample)
                try:
                    want = oracle.want(k, stride, hit_max, sample)
                except Spins:
                    spun += 1
                    assert hit_max not in (1, 3, 64), what
                    with pytest.raises(Gcsa2Error) as err:
                        gpu.kmer_hits_batch(flat, off, k, stride, hit_max, sample)
                    assert err.value.code == INVALID and "max_positions" in str(err.value), what
                    continue
                m, h = want[1].shape[0], want[3].shape[0]
                assert_device(batch.hits(gpu, k, stride, hit_max, int(sample), m, h), want, len(reads), what + ("device",))
                assert_host(gpu.kmer_hits_batch(flat, off, k, stride, hit_max, sample, profiles=True), want, what + ("host",))
    assert spun <= 10, spun
    gpu.close()


@pytest.mark.gpu
def test_order_across_wavefronts_and_workgroups(big):
    """4. The seeds are, record for record, the non-empty windows of gcsa2_kmer_windows_device in window order, and the seed
    offsets the exclusive sum of profile.found, on a batch of many workgroups whose reads straddle wavefront and workgroup
    boundaries -- so that the order in which wavefronts reserve their records can differ from window order."""
    reads = reads_of(BIG)
    k, stride = 8, 1
    batch = DeviceReads(reads)
    woff, prof, rng, cnt = batch.windows(big, k, stride)
    total = int(woff[-1])
    first, last = woff[:-1].astype(np.int64), woff[1:].astype(np.int64) - 1
    has = last >= first
    assert total > 8 * WORKGROUP
    assert int((has & (first // WAVE != last // WAVE)).sum()) > 10 and int((has & (first // WORKGROUP != last // WORKGROUP)).sum()) > 10
    nonempty = (rng[:, 0] + np.uint64(1)) <= (rng[:, 1] + np.uint64(1))
    position = (np.arange(total, dtype=np.int64) - np.repeat(first, np.diff(woff.astype(np.int64)))) * stride
    want = np.zeros((int(nonempty.sum()), 5), dtype=np.uint64)
    want[:, 0], want[:, 1], want[:, 2:4], want[:, 4] = position[nonempty], k, rng[nonempty], cnt[nonempty]
    m = want.shape[0]
    assert 0 < m < total
    res, soff, seeds, hoff, hits, got_prof = batch.hits(big, k, stride, 3, SKIP, m, total * 3)
    assert res[0] == m
    assert np.array_equal(seeds[:m], want)
    assert np.array_equal(soff[:len(reads) + 1], np.concatenate([[0], np.cumsum(prof[:, 1].astype(np.int64))]).astype(np.uint64))
    assert np.array_equal(got_prof[:len(reads)], prof)


@pytest.mark.gpu
def test_every_table_shape(engine, big, monkeypatch):
    """5. With and without pair blocks, with the seed table at 0 and its default, and on an image that has a jump table (asked
    for, and without an LCP array): the same seeds and hits as the default image.  A find-only image is refused."""
    reads = reads_of(BIG)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    default_k = big.kmer_table_k()
    cases = [(k, stride, hit_max, sample) for k, stride in ((8, 1), (16, 1), (33, 3)) for hit_max, sample in ((0, False), (3, True))]
    base = {c: big.kmer_hits_batch(flat, off, *c, profiles=True) for c in cases}
    assert all(v[1].shape[0] > 0 and v[3].shape[0] > 0 for v in base.values())

    def compare(gpu, what):
        for c, want in base.items():
            m, h = want[1].shape[0], want[3].shape[0]
            assert_device(batch.hits(gpu, c[0], c[1], c[2], int(c[3]), m, h), want, len(reads), (what, c))

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
    monkeypatch.delenv("GCSA2_JUMP_TABLE")
    assert jumping.jump_table_bytes() > 0 and find_only.jump_table_bytes() > 0
    compare(jumping, "jump table, no LCP array")
    got = batch.hits(find_only, 16, 1, 0, SKIP, 64, 64)
    assert got[0].code == MISSING and untouched(got[1:]), got[0]
    jumping.close()
    find_only.close()


def host_call(gpu, reads, k, stride, hit_max, over, seed_capacity, hit_capacity, profiles=True, null_index=False):
    """gcsa2_kmer_hits_batch on sentinel-filled numpy buffers: (status, (seeds, hits), seed_offsets, seeds, hit_offsets, hits,
    profiles)."""
    data, off = concat_patterns(reads)
    data, off = np.ascontiguousarray(data, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64)
    n = len(reads)

    def buf(*shape):
        return np.full(shape, SENTINEL, dtype=np.uint64)

    prof = buf(n + GUARD, 4) if profiles else None
    soff, seeds, hoff, hits = buf(n + 1 + GUARD), buf(seed_capacity + GUARD, 5), buf(seed_capacity + 1 + GUARD), buf(hit_capacity + GUARD)
    total_seeds, total_hits = ctypes.c_uint64(SENTINEL), ctypes.c_uint64(SENTINEL)
    rc = gpu._L.gcsa2_kmer_hits_batch(None if null_index else gpu._h, data.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                      off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n, k, stride, hit_max, over,
                                      None if prof is None else prof.ctypes.data, soff.ctypes.data, seeds.ctypes.data, seed_capacity,
                                      ctypes.byref(total_seeds), hoff.ctypes.data, hits.ctypes.data, hit_capacity, ctypes.byref(total_hits))
    return rc, (total_seeds.value, total_hits.value), soff, seeds, hoff, hits, prof


@pytest.mark.gpu
def test_capacities_and_nulls(big):
    """6. Exact capacities are filled and nothing lies behind them; one record or one hit short is refused with both totals and
    nothing written; the profiles may be NULL; empty batches, batches without windows and without found windows are fine; the
    invalid arguments are refused with nothing written, the totals included."""
    reads = reads_of(BIG)[90:130] + EDGE
    n = len(reads)
    oracle = Seeds(indexed(BIG)[1], reads)
    batch = DeviceReads(reads)
    for k, stride, hit_max, over in ((12, 2, 0, SKIP), (6, 1, 3, SAMPLE)):
        want = oracle.want(k, stride, hit_max, bool(over))
        m, h = want[1].shape[0], want[3].shape[0]
        assert m > 0 and h > 0
        what = (k, stride, hit_max, over)
        assert_device(batch.hits(big, k, stride, hit_max, over, m, h), want, n, what + ("exact",))
        assert_device(batch.hits(big, k, stride, hit_max, over, m, h, profiles=False), want, n, what + ("no profiles",))
        rc, totals, *arrays = host_call(big, reads, k, stride, hit_max, over, m, h)
        assert rc == 0
        assert_device(((totals[0], totals[1]),) + tuple(arrays), want, n, what + ("exact, host",))
        rc, totals, *arrays = host_call(big, reads, k, stride, hit_max, over, m, h, profiles=False)
        assert rc == 0
        assert_device(((totals[0], totals[1]),) + tuple(arrays), want, n, what + ("no profiles, host",))
        for mcap, hcap in ((m - 1, h), (m, h - 1), (m - 1, h - 1), (0, 0)):
            got = batch.hits(big, k, stride, hit_max, over, mcap, hcap)
            assert got[0].code == TOO_SMALL and got[0].needed == (m, h), what + (mcap, hcap)
            assert untouched(got[1:]), what + (mcap, hcap)
            rc, totals, *arrays = host_call(big, reads, k, stride, hit_max, over, mcap, hcap)
            assert rc == TOO_SMALL and totals == (m, h) and untouched(arrays), what + (mcap, hcap, "host")
    # no reads at all; reads all shorter than k; reads without any found window
    sentinel = np.uint64(SENTINEL)
    for some, k in (([], 16), ([b"ACGT", b"", b"ACGTACG", b"A"], 8), ([b"NNNN", b"XYZ", b"NNNN", b""], 2), ([b"NNNN", b"XYZ"], 3)):
        nn = len(some)
        res, soff, seeds, hoff, hits, prof = DeviceReads(some).hits(big, k, 1, 3, SAMPLE, 4, 4)
        assert res == (0, 0), (some, k)
        assert (soff[:nn + 1] == 0).all() and (soff[nn + 1:] == sentinel).all() and int(hoff[0]) == 0 and (hoff[1:] == sentinel).all()
        assert untouched([seeds, hits, prof[nn:]])
        assert prof[:nn].tolist() == [[window_count(len(r), k, 1), 0, 0, 0] for r in some], (some, k)
        rc, totals, soff, seeds, hoff, hits, prof = host_call(big, some, k, 1, 3, SAMPLE, 4, 4)
        assert rc == 0 and totals == (0, 0), (some, k)
        assert (soff[:nn + 1] == 0).all() and (soff[nn + 1:] == sentinel).all() and int(hoff[0]) == 0 and (hoff[1:] == sentinel).all()
        assert untouched([seeds, hits, prof[nn:]])
        if nn:
            assert prof[:nn].tolist() == [[window_count(len(r), k, 1), 0, 0, 0] for r in some], (some, k)
        got = big.kmer_hits_batch(*concat_patterns(some), k, 1, 3, True)
        assert got[0].tolist() == [0] * (nn + 1) and got[1].shape == (0, 5) and got[2].tolist() == [0] and got[3].shape == (0,)
    # invalid arguments
    for kk, ss, over in ((0, 1, SKIP), (4, 0, SKIP), (4, 1, 7)):
        got = batch.hits(big, kk, ss, 0, over, 64, 64)
        assert got[0].code == INVALID and got[0].needed == (0, 0) and untouched(got[1:]), (kk, ss, over)
        rc, totals, *arrays = host_call(big, reads, kk, ss, 0, over, 64, 64)
        assert rc == INVALID and totals == (SENTINEL, SENTINEL) and untouched(arrays), (kk, ss, over)
    rc, totals, *arrays = host_call(big, reads, 4, 1, 0, SKIP, 64, 64, null_index=True)
    assert rc == INVALID and totals == (SENTINEL, SENTINEL) and untouched(arrays)
    # the host form refuses offsets that do not start at 0 or decrease
    for bad in ([1, 20, 40], [0, 40, 20]):
        off = np.asarray(bad, dtype=np.uint64)
        out = np.full(64, SENTINEL, dtype=np.uint64)
        totals = (ctypes.c_uint64(SENTINEL), ctypes.c_uint64(SENTINEL))
        rc = big._L.gcsa2_kmer_hits_batch(big._h, np.zeros(64, dtype=np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                          off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 2, 4, 1, 0, SKIP, None, out.ctypes.data,
                                          out[8:].ctypes.data, 1, ctypes.byref(totals[0]), out[16:].ctypes.data, out[24:].ctypes.data, 1,
                                          ctypes.byref(totals[1]))
        assert rc == INVALID and untouched([out]), bad


@pytest.mark.gpu
def test_the_cap_bites(engine):
    """7. Seeds whose counts are far above hit_max, with a hit_max above 1024: SAMPLE equals locate_max_batch value for value,
    SKIP leaves those seeds without hits and with their true counts, and the other seeds have the same hits under both."""
    from workload import patterns
    from test_mem_hits import cap_index
    g, ix, gpu = cap_index(engine)
    reads = [bytes(p) for p in patterns.walk_patterns(g, 48, 30, 0x6B1)]
    flat, off = concat_patterns(reads)
    for k in (1, 2, 3, 6):
        for hit_max in (1, 8, 64, 1100):
            soff, seeds, hoff, hits = gpu.kmer_hits_batch(flat, off, k, 1, hit_max, True)
            s_soff, s_seeds, s_hoff, s_hits = gpu.kmer_hits_batch(flat, off, k, 1, hit_max, False)
            assert np.array_equal(soff, s_soff) and np.array_equal(seeds, s_seeds)
            assert seeds.shape[0] == sum(window_count(len(r), k, 1) for r in reads)          # walks: every window is found
            counts = seeds[:, 4].astype(np.uint64)
            over = counts > np.uint64(hit_max)
            if k >= 3 and hit_max == 1100:              # 3-mers and 6-mers of this graph occur fewer than 1100 times: all located in full
                assert not over.any() and int(counts.max()) > 64, (k, hit_max, int(counts.max()))
            else:
                assert int(over.sum()) >= 4 and int(counts.max()) > 2 * hit_max, (k, hit_max, int(over.sum()), int(counts.max()))
            assert np.array_equal(gpu.count_batch(seeds[:, 2:4].copy()), counts)
            lo, lv = gpu.locate_max_batch(seeds[over][:, 2:4].copy(), hit_max)
            sizes = np.diff(hoff.astype(np.int64))
            assert (sizes[over] == hit_max).all(), (k, hit_max)
            assert np.array_equal(hits[np.repeat(over, sizes)], lv) and np.array_equal(np.diff(lo.astype(np.int64)), sizes[over]), (k, hit_max)
            s_sizes = np.diff(s_hoff.astype(np.int64))
            assert (s_sizes[over] == 0).all() and np.array_equal(s_sizes[~over], sizes[~over])
            assert np.array_equal(s_hits, hits[np.repeat(~over, sizes)])
    gpu.close()


@pytest.mark.gpu
def test_feeds_reseeding(big):
    """8. The seed CSR of a k = 16 call goes into sub_mem_hits_batch as it is and gives what the same records give when they
    are put together by hand from find() and count() of the materialised windows."""
    reads = reads_of(BIG)
    flat, off = concat_patterns(reads)
    k = 16
    soff, seeds, _, _ = big.kmer_hits_batch(flat, off, k, 1, 0, False)
    wins = [r[j:j + k] for r in reads for j in range(window_count(len(r), k, 1))]
    owner = np.repeat(np.arange(len(reads)), [window_count(len(r), k, 1) for r in reads])
    position = np.concatenate([np.arange(window_count(len(r), k, 1)) for r in reads])
    ranges = big.find_batch(*concat_patterns(wins))
    keep = (ranges[:, 0] + np.uint64(1)) <= (ranges[:, 1] + np.uint64(1))
    hand = np.zeros((int(keep.sum()), 5), dtype=np.uint64)
    hand[:, 0], hand[:, 1], hand[:, 2:4], hand[:, 4] = position[keep], k, ranges[keep], big.count_batch(ranges[keep].copy())
    hand_off = np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=len(reads)))]).astype(np.uint64)
    assert np.array_equal(hand, seeds) and np.array_equal(hand_off, soff)
    got = big.sub_mem_hits_batch(flat, off, soff, seeds, 6, 16, 8, True)
    want = big.sub_mem_hits_batch(flat, off, hand_off, hand, 6, 16, 8, True)
    assert got[1].shape[0] > 0 and got[3].shape[0] > 0
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_host_form_in_pieces(engine, monkeypatch):
    """9. The batch of the 6000-base graph, repeated until it is 3 MB of reads (the smallest piece is 1 MB), in 1 MB pieces
    equals the same batch in one piece, and its first repetition the batch alone.  Library against library."""
    ix = indexed(BIG)[0]
    whole, _ = engine.open_index(ix, device=0)
    monkeypatch.setenv("GCSA2_MS_PIECE_MB", "1")
    pieced, _ = engine.open_index(ix, device=0)
    once = reads_of(BIG)
    repeats = (3 << 20) // sum(len(r) for r in once) + 1
    reads = once * repeats
    flat, off = concat_patterns(reads)
    assert int(off[-1]) >= 3 << 20                      # a piece holds at most 1 MB of reads, so cut_pieces yields at least 3
    alone = whole.kmer_hits_batch(*concat_patterns(once), 32, 1, 4, True, profiles=True)
    for k, stride, hit_max, sample in ((32, 1, 4, True), (24, 5, 0, False)):
        a = pieced.kmer_hits_batch(flat, off, k, stride, hit_max, sample, profiles=True)
        b = whole.kmer_hits_batch(flat, off, k, stride, hit_max, sample, profiles=True)
        assert_host(a, b, (k, stride, hit_max, sample))
        assert 0 < a[1].shape[0] < sum(window_count(len(r), k, stride) for r in reads) and a[3].shape[0] > 0
    a = pieced.kmer_hits_batch(flat, off, 32, 1, 4, True, profiles=True)
    m, h, n = alone[1].shape[0], alone[3].shape[0], len(once)
    assert a[1].shape[0] == repeats * m and a[3].shape[0] == repeats * h
    assert_host((a[0][:n + 1], a[1][:m], a[2][:m + 1], a[3][:h], a[4][:n]), alone, "first repetition")
    # too small in pieces: refused with both totals
    from gcsa2_amd.binding import Gcsa2Error
    with pytest.raises(Gcsa2Error) as err:
        pieced.kmer_hits_batch(flat, off, 32, 1, 4, True, out=(np.zeros(len(reads) + 1, dtype=np.uint64), np.zeros((repeats * m - 1, 5), dtype=np.uint64),
                                                              np.zeros(repeats * m, dtype=np.uint64), np.zeros(repeats * h, dtype=np.uint64)))
    assert err.value.code == TOO_SMALL and err.value.needed == (repeats * m, repeats * h)
    pieced.close()
    whole.close()


@pytest.mark.gpu
def test_facade_kmer_hits(engine, tmp_path):
    """10. GCSA::kmer_hits_batch from a C++ client (tests/cpp/kmer_hits_client.cpp) prints what GCSA.kmer_hits_batch returns."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    which = len(CASES) - 1
    reads = reads_of(which)
    assert all(b"\n" not in r for r in reads)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    save_host_view(indexed(which)[0], str(tmp_path / "index.g2hv"))
    (tmp_path / "reads.txt").write_bytes(b"".join(r + b"\n" for r in reads))
    exe = compile_client(str(tmp_path / "kmer_hits_client"), os.path.join(ROOT, "tests", "cpp", "kmer_hits_client.cpp"))
    data, off = concat_patterns(reads)
    for k, stride, hit_max, sample in ((5, 1, 0, 0), (3, 1, 3, 1), (7, 3, 2, 0)):
        out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "reads.txt"), str(k), str(stride), str(hit_max), str(sample)],
                             capture_output=True, text=True, env=_run_env(), timeout=300)
        assert out.returncode == 0, out.stderr
        soff, seeds, hoff, hits = gpu.kmer_hits_batch(data, off, k, stride, hit_max, bool(sample))
        want = [f"read {q} {int(soff[q + 1] - soff[q])}" for q in range(len(reads))]
        want += [f"seed {i} " + " ".join(str(int(x)) for x in seeds[i]) for i in range(seeds.shape[0])]
        want += [" ".join(["hits", str(i), str(int(hoff[i + 1] - hoff[i]))] + [str(int(v)) for v in hits[int(hoff[i]):int(hoff[i + 1])]])
                 for i in range(seeds.shape[0])]
        assert out.stdout.strip().split("\n") == want, (k, stride, hit_max, sample)
        assert seeds.shape[0] > 0 and hits.shape[0] > 0
    gpu.close()
