"""A maximum match length for the break records and the MEM hits (gcsa2_match_breaks_bounded_* / gcsa2_mem_hits_bounded_*,
k_match_stats2<.., CAP>): a match that has reached max_length characters is cut as if the next character had failed and the
search goes on from parent().  Against a Python restatement of the contract's walk (include/gcsa2_hip.h) over the CPU
oracle's LF / parent, against the unbounded entry points where the cap cannot bite, and against the composition of the
library's own public calls."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from workload import graphs
from workload.brute_builder import build
from gcsa2_amd.hostview import concat_patterns
from test_oracle import CASES, random_patterns
from test_gpu_parity import breaks_from_dense
from test_mem_hits import substituted, assert_same, composition, SENTINEL, EDGE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
S = np.uint64(SENTINEL)


def is_empty(r):
    """range_empty of the reference (utils.h): sp + 1 > ep + 1 in 64-bit arithmetic."""
    return ((r[0] + 1) & U64) > ((r[1] + 1) & U64)


def walk(cpu, pattern, max_length):
    """The contract's walk (include/gcsa2_hip.h) over the oracle's LF and parent: ([(position, length, sp, ep)] in the order
    of discovery, final range, parent() calls)."""
    n = cpu.n
    root = (0, n - 1)
    i, r, depth, last, parents = len(pattern), root, 0, None, 0
    out = []
    while i > 0:
        if not (max_length > 0 and depth >= max_length):
            r2 = cpu.LF(r, int(cpu.char2comp[pattern[i - 1]]))
            if not is_empty(r2):
                r, depth, i = r2, depth + 1, i - 1
                continue
        if r == root:
            depth, i = 0, i - 1
            if i + 1 < len(pattern) and last != i + 1:
                out.append((i + 1, 0, 0, n - 1))
                last = i + 1
            continue
        if last != i:
            out.append((i, depth, r[0], r[1]))
            last = i
        p = cpu.parent(r)
        r, depth, parents = (p[0], p[1]), p[4], parents + 1
    if len(pattern) > 0 and last != 0:
        out.append((0, depth, r[0], r[1]))
    return out, r, parents


class Walked:
    """The walk of every pattern of a batch under one max_length, unfiltered; expected() applies a minimum length."""
    def __init__(self, cpu, pats, max_length):
        self.records, self.ranges, self.parents = [], [], []
        for p in pats:
            rec, r, calls = walk(cpu, p, max_length)
            self.records.append(rec)
            self.ranges.append(r)
            self.parents.append(calls)

    def expected(self, min_length):
        off, rows = [0], []
        for rec in self.records:
            rows += [x for x in rec if x[1] >= min_length]
            off.append(len(rows))
        return (np.asarray(off, dtype=np.uint64), np.asarray(rows, dtype=np.uint64).reshape(-1, 4),
                np.asarray(self.ranges, dtype=np.uint64).reshape(-1, 2), np.asarray(self.parents, dtype=np.uint64))

    def longest(self):
        return max([x[1] for rec in self.records for x in rec] + [0])


def case_patterns(which):
    name, g, K = CASES[which]
    return random_patterns(g, 3 * K, 0x7E0 + which, 300) + EDGE


def assert_breaks(got, want, what):
    for name, a, b in zip(("break_offsets", "breaks", "ranges", "fallbacks"), got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name, a.shape, b.shape)


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_library_exports_the_bounded_calls_and_refuses_a_null_index():
    """The built library exports the four bounded calls; each refuses a NULL index with INVALID_ARGUMENT before touching a
    device."""
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    for name in ("gcsa2_match_breaks_bounded_device", "gcsa2_match_breaks_bounded_batch", "gcsa2_mem_hits_bounded_device",
                 "gcsa2_mem_hits_bounded_batch"):
        assert hasattr(ctypes.CDLL(binding.LIB_PATH), name), name
    lib = binding.load_library()
    total_a, total_b = ctypes.c_uint64(7), ctypes.c_uint64(7)
    buf = (ctypes.c_uint64 * 16)()
    at = ctypes.addressof(buf)
    rc = lib.gcsa2_match_breaks_bounded_device(None, None, None, 0, 0, 0, 1, 4, at, None, 0, ctypes.byref(total_a), None, None, None)
    assert rc == -1 and "index" in lib.gcsa2_last_error().decode()
    rc = lib.gcsa2_match_breaks_bounded_batch(None, None, buf, 0, 1, 4, buf, None, 0, ctypes.byref(total_a), None, None)
    assert rc == -1 and "index" in lib.gcsa2_last_error().decode()
    rc = lib.gcsa2_mem_hits_bounded_device(None, None, None, 0, 0, 1, 4, 0, 0, at, None, 0, ctypes.byref(total_a), at, None, 0,
                                           ctypes.byref(total_b), None)
    assert rc == -1 and "index" in lib.gcsa2_last_error().decode()
    rc = lib.gcsa2_mem_hits_bounded_batch(None, None, buf, 0, 1, 4, 0, 0, at, None, 0, ctypes.byref(total_a), at, None, 0, ctypes.byref(total_b))
    assert rc == -1 and "index" in lib.gcsa2_last_error().decode()
    assert total_a.value == 7 and total_b.value == 7 and all(v == 0 for v in buf)


@pytest.mark.parametrize("which", range(len(CASES)), ids=[c[0] for c in CASES])
def test_walk_restates_the_contract(which):
    """The restatement itself, on the CPU: without a cap it gives the records the dense statistics imply and the oracle's
    final ranges and parent() counts; with a cap every record is at most that long and carries find() of its substring, and a
    pattern changes exactly when it has a record longer than the cap."""
    from oracle.oracle import OracleIndex
    name, g, K = CASES[which]
    ix = build(g, K, sample_period=8, branching=4)
    cpu = OracleIndex(ix)
    pats = case_patterns(which)
    data, off = concat_patterns(pats)
    cm, cr, cf = cpu.match_stats_batch(data, off, threads=2)
    free = Walked(cpu, pats, 0)
    assert_breaks(free.expected(0), breaks_from_dense(cpu, pats, cm, off) + (cr.reshape(-1, 2), cf), (name, "uncapped"))
    for cap in (1, K, K + 1):
        capped = Walked(cpu, pats, cap)
        for q, p in enumerate(pats):
            for pos, ln, sp, ep in capped.records[q]:
                assert ln <= cap and (ln == 0 or (sp, ep) == cpu.find(p[pos:pos + ln])), (name, cap, p, pos, ln)
            has_long = any(x[1] > cap for x in free.records[q])
            assert (capped.records[q] != free.records[q]) == has_long, (name, cap, p)


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine():
    from gcsa2_amd import binding
    assert binding.device_count() >= 1, "no MI355X visible"
    return binding


class DeviceBatch:
    """A batch in device memory with sentinel-filled result buffers of `capacity` records and `guard` more behind them."""
    def __init__(self, pats, capacity, guard=16):
        import torch
        self.torch = torch
        data, off = concat_patterns(pats)
        dev = torch.device("cuda", 0)
        self.nq, self.total, self.capacity = len(pats), int(off[-1]), capacity
        self.d_pat = torch.zeros(self.total + 16, dtype=torch.uint8, device=dev)
        self.d_pat[:self.total] = torch.from_numpy(data[:self.total].copy()).to(dev)
        self.d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
        s = S.view(np.int64).item()
        self.d_boff = torch.full((self.nq + 1,), s, dtype=torch.int64, device=dev)
        self.d_brk = torch.full((capacity + guard, 4), s, dtype=torch.int64, device=dev)
        self.d_rng = torch.full((max(self.nq, 1), 2), s, dtype=torch.int64, device=dev)
        self.d_fb = torch.full((max(self.nq, 1),), s, dtype=torch.int64, device=dev)
        self.s = s

    def call(self, gpu, min_length, max_length, variant=0, capacity=None, bounded=True):
        """(records or Gcsa2Error, break_offsets, breaks (whole buffer), ranges, fallbacks); bounded=False: the C entry point
        without a cap, gcsa2_match_breaks_device, called as it was before the cap existed."""
        from gcsa2_amd.binding import Gcsa2Error
        for t in (self.d_boff, self.d_brk, self.d_rng, self.d_fb):
            t.fill_(self.s)
        cap = self.capacity if capacity is None else capacity
        try:
            if bounded:
                res = gpu.match_breaks_device(self.d_pat.data_ptr(), self.d_off.data_ptr(), self.nq, self.total, self.d_boff.data_ptr(),
                                              self.d_brk.data_ptr(), cap, self.d_rng.data_ptr(), self.d_fb.data_ptr(), 0, variant=variant,
                                              min_length=min_length, max_length=max_length)
            else:
                total = ctypes.c_uint64()
                rc = gpu._L.gcsa2_match_breaks_device(gpu._h, self.d_pat.data_ptr(), self.d_off.data_ptr(), self.nq, self.total, variant, min_length,
                                                      self.d_boff.data_ptr(), self.d_brk.data_ptr(), cap, ctypes.byref(total),
                                                      self.d_rng.data_ptr(), self.d_fb.data_ptr(), None)
                assert rc == 0, rc
                res = total.value
        except Gcsa2Error as e:
            res = e
        self.torch.cuda.synchronize()
        return tuple([res] + [t.cpu().numpy().view(np.uint64) for t in (self.d_boff, self.d_brk, self.d_rng, self.d_fb)])


def uncapped_host(gpu, flat, off, min_length):
    """gcsa2_match_breaks_batch, the C entry point without a cap: (break_offsets, breaks, ranges, fallbacks)."""
    flat = np.ascontiguousarray(flat, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    nq = off.shape[0] - 1
    cap = int(off[-1]) + nq + 1
    boff, brk = np.zeros(nq + 1, dtype=np.uint64), np.zeros((cap, 4), dtype=np.uint64)
    rng, fb = np.zeros((nq, 2), dtype=np.uint64), np.zeros(nq, dtype=np.uint64)
    total = ctypes.c_uint64()
    from gcsa2_amd.binding import u8p, u64p
    rc = gpu._L.gcsa2_match_breaks_batch(gpu._h, flat.ctypes.data_as(u8p), off.ctypes.data_as(u64p), nq, min_length, boff.ctypes.data_as(u64p),
                                         brk.ctypes.data, cap, ctypes.byref(total), rng.ctypes.data, fb.ctypes.data)
    assert rc == 0, rc
    return boff, brk[:total.value], rng, fb


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(CASES)), ids=[c[0] for c in CASES])
def test_oracle_parity(engine, which):
    """Every graph of test_oracle.CASES, random patterns up to 3 x the order long and the edge patterns; max_length 1, 2, K - 1,
    K, K + 1, the longest unbounded record and 0; min_length 1, 2, K: the device form in its three launch shapes and the host
    form give the walk's break_offsets, breaks, ranges and fallbacks exactly.  The cap K changes the records of at least 50
    patterns; no cap and a cap that is never reached equal the unbounded entry points."""
    from oracle.oracle import OracleIndex
    name, g, K = CASES[which]
    ix = build(g, K, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    cpu = OracleIndex(ix)
    pats = case_patterns(which)
    flat, off = concat_patterns(pats)
    free = Walked(cpu, pats, 0)
    longest = free.longest()
    assert longest > K, (name, longest)
    batch = DeviceBatch(pats, int(off[-1]) + len(pats))
    caps = []
    for cap in (1, 2, K - 1, K, K + 1, longest, 0):
        if cap not in caps:
            caps.append(cap)
    for cap in caps:
        walked = free if cap == 0 else Walked(cpu, pats, cap)
        if cap == K:
            changed = sum(1 for a, b in zip(walked.records, free.records) if a != b)
            assert changed >= 50, (name, changed)
        for min_length in (1, 2, K):
            if cap != 0 and min_length > cap:
                continue
            what = (name, cap, min_length)
            want = walked.expected(min_length)
            n = want[1].shape[0]
            for variant in (0, 2, 5):
                res, boff, brk, rng, fb = batch.call(gpu, min_length, cap, variant)
                assert res == n, (what, variant, res, n)
                assert_breaks((boff, brk[:n], rng, fb), want, what + ("device", variant))
                assert (brk[n:] == S).all(), what
            assert_breaks(gpu.match_breaks_batch(flat, off, min_length, max_length=cap), want, what + ("host",))
            if cap in (0, longest):
                for variant in (0, 2, 5):
                    res, boff, brk, rng, fb = batch.call(gpu, min_length, 0, variant, bounded=False)
                    assert res == n, (what, variant)
                    assert_breaks((boff, brk[:n], rng, fb), want, what + ("unbounded device", variant))
                assert_breaks(uncapped_host(gpu, flat, off, min_length), want, what + ("unbounded host",))
    gpu.close()


LARGE_CAPS = (5, 16, 31, 32, 33, 64)


@pytest.fixture(scope="module")
def large(engine):
    """The snp graph of 2^16 bases of test_mem_hits.test_composition_larger_index (order 32) and substituted walk patterns of
    100 to 120 bp, which cross the 32-character pattern records of k_pack_records; the walk of a fixed sample of 300 of them
    under every cap, computed once."""
    from oracle.oracle import OracleIndex
    from workload import builder, patterns
    g = graphs.snp_graph(1 << 16, 0x4E1, 0x4E2, snp_period=16, node_len=16)
    ix = builder.build(g, 32, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    pats = []
    for k, length in enumerate((100, 107, 113, 120)):
        pats += substituted([bytes(p) for p in patterns.walk_patterns(g, 1000, length, 0x6A0 + k)], 0x6B0 + k, period=40)
    sample = list(range(0, len(pats), len(pats) // 300))[:300]
    cpu = OracleIndex(ix)
    walked = {cap: Walked(cpu, [pats[q] for q in sample], cap) for cap in LARGE_CAPS}
    return g, ix, gpu, pats, sample, walked


def per_pattern(boff, brk):
    return [brk[int(boff[q]):int(boff[q + 1])] for q in range(boff.shape[0] - 1)]


@pytest.mark.gpu
def test_kernel_corners_on_a_larger_index(engine, large):
    """Order 32, 100 to 120 bp patterns, max_length 5, 16, 31, 32, 33 and 64, with and without pair blocks, with a k-mer seed
    table shorter than the cap, as long as it and longer: the same records in every configuration, the walk's on the sample;
    for the whole batch every length is at most the cap, every range is find() of its substring, the MEM counts are count(),
    and a pattern whose unbounded records all fit under the cap keeps them."""
    g, ix, gpu, pats, sample, walked = large
    flat, off = concat_patterns(pats)
    nq = len(pats)
    free = gpu.match_breaks_batch(flat, off, 0)
    free_rows = per_pattern(free[0], free[1])
    results, relations = {}, set()
    for pair_blocks in (1, 0):
        for kmer_k in (4, 5, 8):
            gpu.set_tables(pair_blocks=pair_blocks, kmer_k=kmer_k)
            k = gpu.kmer_table_k()
            assert k == kmer_k and (gpu.pair_block_bytes() > 0) == bool(pair_blocks)
            for cap in LARGE_CAPS:
                relations.add("below" if k < cap else "equal" if k == cap else "above")
                got = gpu.match_breaks_batch(flat, off, 0, max_length=cap)
                if cap not in results:
                    results[cap] = got
                else:
                    assert_breaks(got, results[cap], (cap, pair_blocks, kmer_k))
    assert relations == {"below", "equal", "above"}, relations
    for cap in LARGE_CAPS:
        boff, brk, rng, fb = results[cap]
        rows = per_pattern(boff, brk)
        want = walked[cap].expected(0)
        got_rows = [rows[q] for q in sample]
        assert np.array_equal(np.concatenate(got_rows), want[1]) and [r.shape[0] for r in got_rows] == np.diff(want[0]).tolist(), cap
        assert np.array_equal(rng[sample], want[2]) and np.array_equal(fb[sample], want[3]), cap
        # the whole batch
        assert int(brk[:, 1].max()) <= cap and int(brk[:, 1].max()) == min(cap, int(free[1][:, 1].max())), cap
        owner = np.repeat(np.arange(nq), np.diff(boff).astype(np.int64))
        subs = [pats[int(q)][int(p):int(p) + int(ln)] for q, (p, ln) in zip(owner, brk[:, :2].tolist())]
        sflat, soff = concat_patterns(subs)
        found = gpu.find_batch(sflat, soff)
        nonempty = brk[:, 1] > 0
        assert np.array_equal(found[nonempty], brk[nonempty][:, 2:4]), cap
        assert (brk[~nonempty][:, 2] == 0).all() and (brk[~nonempty][:, 3] == np.uint64(ix.n - 1)).all(), cap
        moff, mems, hoff, hits = gpu.mem_hits_batch(flat, off, 1, 1, False, max_length=cap)
        assert np.array_equal(mems[:, :4], brk[nonempty]) and np.array_equal(mems[:, 4], gpu.count_batch(mems[:, 2:4].copy())), cap
        fits = 0
        for q in range(nq):
            if free_rows[q].shape[0] == 0 or int(free_rows[q][:, 1].max()) <= cap:
                fits += 1
                assert np.array_equal(rows[q], free_rows[q]) and np.array_equal(rng[q], free[2][q]) and fb[q] == free[3][q], (cap, q)
        assert fits > 0 or cap < 64, (cap, fits)       # (not vacuous: a substitution in its middle keeps a pattern's matches under 64)
    # the cap bites: a pattern changes when it has a record longer than the cap, and with a substitution in one character of 40
    # most of these patterns have a match of more than 32
    at_order = per_pattern(*results[32][:2])
    assert sum(1 for q in range(nq) if not np.array_equal(at_order[q], free_rows[q])) > nq // 4


class Capped:
    """An index whose match_breaks_batch runs under a maximum match length: for test_mem_hits.composition."""
    def __init__(self, gpu, max_length):
        self.gpu, self.max_length = gpu, max_length

    def match_breaks_batch(self, flat, off, min_length):
        return self.gpu.match_breaks_batch(flat, off, min_length, max_length=self.max_length)

    def __getattr__(self, name):
        return getattr(self.gpu, name)


COMBOS = ((0, False), (0, True), (2, False), (2, True), (64, False), (64, True))


@pytest.mark.gpu
def test_mem_hits_under_the_cap(engine, large):
    """mem_hits_batch(max_length=L) equals match_breaks_batch(max_length=L) -> count_batch -> locate_batch / locate_max_batch
    for hit_max 0, 2 and 64 and both over-cap policies; the sub-MEMs of the capped MEMs are at most L long."""
    g, ix, gpu, pats, sample, walked = large
    gpu.set_tables(pair_blocks=1, kmer_k=8)
    flat, off = concat_patterns(pats)
    for L, min_length in ((32, 12), (16, 16)):
        for hit_max, sampled in COMBOS:
            want = composition(Capped(gpu, L), flat, off, min_length, hit_max, sampled)
            got = gpu.mem_hits_batch(flat, off, min_length, hit_max, sampled, max_length=L)
            assert_same(got, want, (L, min_length, hit_max, sampled))
            assert got[1].shape[0] > len(pats) and int(got[1][:, 1].max()) == L
        moff, mems, _, _ = gpu.mem_hits_batch(flat, off, min_length, 0, False, max_length=L)
        # (every MEM is reseeded: reseed_length is the minimum MEM length, which is at most L)
        soff, subs, shoff, shits = gpu.sub_mem_hits_batch(flat, off, moff, mems, 6, min_length, 0, False)
        assert subs.shape[0] > 0 and int(subs[:, 1].max()) <= L, (L, subs.shape)
    assert not np.array_equal(gpu.mem_hits_batch(flat, off, 12, 2, False, max_length=32)[1], gpu.mem_hits_batch(flat, off, 12, 2, False)[1])


@pytest.mark.gpu
def test_mem_hits_under_the_cap_in_pieces(engine, large, monkeypatch):
    """The same on a host batch of 3 MB that goes in 1 MB pieces: every piece runs under the cap."""
    from workload import patterns
    g, ix, gpu, pats, sample, walked = large
    gpu.set_tables(pair_blocks=1, kmer_k=8)
    monkeypatch.setenv("GCSA2_MS_PIECE_MB", "1")
    pieced, _ = engine.open_index(ix, device=0)
    big = substituted([bytes(p) for p in patterns.walk_patterns(g, 32_000, 100, 0x6C5)], 0x6C6, period=40)
    flat, off = concat_patterns(big)
    assert int(off[-1]) >= 3 << 20
    L, min_length = 32, 20
    assert_breaks(pieced.match_breaks_batch(flat, off, min_length, max_length=L), gpu.match_breaks_batch(flat, off, min_length, max_length=L), "pieces")
    for hit_max, sampled in COMBOS:
        want = composition(Capped(gpu, L), flat, off, min_length, hit_max, sampled)
        got = pieced.mem_hits_batch(flat, off, min_length, hit_max, sampled, max_length=L)
        assert_same(got, want, (hit_max, sampled))
        assert got[1].shape[0] > 30_000 and int(got[1][:, 1].max()) == L
    pieced.close()


def mem_device_call(gpu, pats, min_length, max_length, hit_max, over, mem_capacity, hit_capacity, guard=64):
    """gcsa2_mem_hits_bounded_device on sentinel-filled torch buffers with `guard` entries behind the capacities: (result or
    Gcsa2Error, mem_offsets, mems, hit_offsets, hits), whole buffers."""
    import torch
    from gcsa2_amd.binding import Gcsa2Error
    data, off = concat_patterns(pats)
    dev = torch.device("cuda", 0)
    nq, total = len(pats), int(off[-1])
    d_pat = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
    d_pat[:total] = torch.from_numpy(data[:total].copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    s = S.view(np.int64).item()
    d_moff = torch.full((nq + 1,), s, dtype=torch.int64, device=dev)
    d_mems = torch.full((mem_capacity + guard, 5), s, dtype=torch.int64, device=dev)
    d_hoff = torch.full((mem_capacity + 1 + guard,), s, dtype=torch.int64, device=dev)
    d_hits = torch.full((hit_capacity + guard,), s, dtype=torch.int64, device=dev)
    try:
        res = gpu.mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, min_length, hit_max, over, d_moff.data_ptr(), d_mems.data_ptr(),
                                  mem_capacity, d_hoff.data_ptr(), d_hits.data_ptr(), hit_capacity, max_length=max_length)
    except Gcsa2Error as e:
        res = e
    torch.cuda.synchronize()
    return tuple([res] + [t.cpu().numpy().view(np.uint64) for t in (d_moff, d_mems, d_hoff, d_hits)])


@pytest.mark.gpu
def test_contract(engine):
    """min_length > max_length > 0: INVALID_ARGUMENT from all four calls with the sentinel-filled buffers untouched; too small
    a buffer: BUFFER_TOO_SMALL with the capped totals and nothing written; nothing behind the capacities of a fitting call; an
    index without its LCP array: MISSING_COMPONENT; an empty batch: zero offsets; a cap of 2^32 or more: no cap."""
    from gcsa2_amd.binding import Gcsa2Error
    name, g, K = CASES[-1]
    ix = build(g, K, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    pats = case_patterns(len(CASES) - 1)
    flat, off = concat_patterns(pats)
    nq = len(pats)
    batch = DeviceBatch(pats, int(off[-1]) + nq)
    # min_length > max_length > 0
    for min_length, cap in ((K + 1, K), (2, 1), (1 << 33, 5)):
        res, boff, brk, rng, fb = batch.call(gpu, min_length, cap)
        assert isinstance(res, Gcsa2Error) and res.code == -1 and "max_length" in str(res), (min_length, cap)
        assert (boff == S).all() and (brk == S).all() and (rng == S).all() and (fb == S).all()
        out = (np.full(nq + 1, S), np.full((64, 4), S), np.full((nq, 2), S), np.full(nq, S))
        with pytest.raises(Gcsa2Error) as err:
            gpu.match_breaks_batch(flat, off, min_length, out=out, max_length=cap)
        assert err.value.code == -1 and all((a == S).all() for a in out)
        res, moff, mems, hoff, hits = mem_device_call(gpu, pats, min_length, cap, 0, 0, 64, 64)
        assert isinstance(res, Gcsa2Error) and res.code == -1 and res.needed == (0, 0)
        assert (moff == S).all() and (mems == S).all() and (hoff == S).all() and (hits == S).all()
        out = (np.full(nq + 1, S), np.full((64, 5), S), np.full(65, S), np.full(64, S))
        with pytest.raises(Gcsa2Error) as err:
            gpu.mem_hits_batch(flat, off, min_length, 0, False, out=out, max_length=cap)
        assert err.value.code == -1 and all((a == S).all() for a in out)
    # min_length == max_length is a valid call; so is any min_length without a cap
    assert batch.call(gpu, K, K)[0] > 0 and batch.call(gpu, K + 1, 0)[0] > 0
    # BUFFER_TOO_SMALL: the capped totals, nothing written
    free_n = batch.call(gpu, 1, 0)[0]
    n = batch.call(gpu, 1, K)[0]
    assert n != free_n
    res, boff, brk, rng, fb = batch.call(gpu, 1, K, capacity=n - 1)
    assert isinstance(res, Gcsa2Error) and res.code == -6 and res.needed == n and (brk == S).all()
    with pytest.raises(Gcsa2Error) as err:
        gpu.match_breaks_batch(flat, off, 1, out=(np.zeros(nq + 1, dtype=np.uint64), np.zeros((n - 1, 4), dtype=np.uint64),
                                                  np.zeros((nq, 2), dtype=np.uint64), np.zeros(nq, dtype=np.uint64)), max_length=K)
    assert err.value.code == -6 and err.value.needed == n
    res, boff, brk, rng, fb = batch.call(gpu, 1, K, capacity=n)
    assert res == n and (brk[n:] == S).all() and not (brk[:n] == S).any()
    for hit_max, over in ((0, 0), (2, 1)):
        want = gpu.mem_hits_batch(flat, off, 1, hit_max, bool(over), max_length=K)
        m, h = want[1].shape[0], want[3].shape[0]
        assert m == n and h > 0 and m != gpu.mem_hits_batch(flat, off, 1, hit_max, bool(over))[1].shape[0]
        for mcap, hcap in ((m - 1, h), (m, h - 1), (0, 0)):
            res, moff, mems, hoff, hits = mem_device_call(gpu, pats, 1, K, hit_max, over, mcap, hcap)
            assert isinstance(res, Gcsa2Error) and res.code == -6 and res.needed == (m, h), (hit_max, over, mcap, hcap)
            assert (mems == S).all() and (hoff == S).all() and (hits == S).all()
        res, moff, mems, hoff, hits = mem_device_call(gpu, pats, 1, K, hit_max, over, m, h)
        assert res == (m, h)
        assert (mems[m:] == S).all() and (hoff[m + 1:] == S).all() and (hits[h:] == S).all()
        assert_same((moff, mems[:m], hoff[:m + 1], hits[:h]), want, (hit_max, over))
    # a cap that no pattern can reach is no cap
    assert_breaks(gpu.match_breaks_batch(flat, off, 1, max_length=1 << 32), gpu.match_breaks_batch(flat, off, 1), "2^32")
    assert_breaks(gpu.match_breaks_batch(flat, off, 1, max_length=U64), gpu.match_breaks_batch(flat, off, 1), "2^64 - 1")
    # without the LCP array
    bare = engine.GCSA(ix, device=0, with_lcp=False)
    with pytest.raises(Gcsa2Error) as err:
        bare.match_breaks_batch(flat, off, 1, max_length=K)
    assert err.value.code == -5
    with pytest.raises(Gcsa2Error) as err:
        bare.mem_hits_batch(flat, off, 1, 0, False, max_length=K)
    assert err.value.code == -5
    res, *_ = batch.call(bare, 1, K)
    assert isinstance(res, Gcsa2Error) and res.code == -5
    res, *_ = mem_device_call(bare, pats, 1, K, 0, 0, 64, 64)
    assert isinstance(res, Gcsa2Error) and res.code == -5
    bare.close()
    # an empty batch
    none, one = np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64)
    boff, brk, rng, fb = gpu.match_breaks_batch(none, one, 1, max_length=K)
    assert boff.tolist() == [0] and brk.shape[0] == 0
    moff, mems, hoff, hits = gpu.mem_hits_batch(none, one, 1, 0, True, max_length=K)
    assert moff.tolist() == [0] and mems.shape == (0, 5) and hoff.tolist() == [0] and hits.shape[0] == 0
    empty = DeviceBatch([], 4)
    res, boff, *_ = empty.call(gpu, 1, K)
    assert res == 0 and boff.tolist() == [0]
    res, moff, mems, hoff, hits = mem_device_call(gpu, [], 1, K, 0, 0, 4, 4)
    assert res == (0, 0) and moff.tolist() == [0] and int(hoff[0]) == 0
    gpu.close()


@pytest.mark.gpu
def test_facade_bounded_overloads(engine, tmp_path):
    """GCSA::match_breaks_batch and GCSA::mem_hits_batch with max_length = order() from a C++ client
    (tests/cpp/bounded_mems_client.cpp) equal the Python calls."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    g = graphs.snp_graph(3000, 0x5F1, 0x5F2, snp_period=12, node_len=16)
    K = 8
    ix = build(g, K, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    save_host_view(ix, str(tmp_path / "index.g2hv"))
    pats = random_patterns(g, 40, 0x5F3, 200)
    pats = [p for p in pats if b"\n" not in p] + [b"", b"ACGTACGT"]
    (tmp_path / "patterns.txt").write_bytes(b"".join(p + b"\n" for p in pats))
    flat, off = concat_patterns(pats)
    exe = compile_client(str(tmp_path / "bounded_mems_client"), os.path.join(ROOT, "tests", "cpp", "bounded_mems_client.cpp"))
    for min_length, hit_max, sample in ((4, 0, 0), (4, 3, 1), (8, 64, 1)):
        out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "patterns.txt"), str(min_length), str(hit_max), str(sample)],
                             capture_output=True, text=True, env=_run_env(), timeout=300)
        assert out.returncode == 0, out.stderr
        boff, brk, _, _ = gpu.match_breaks_batch(flat, off, min_length, max_length=K)
        moff, mems, hoff, hits = gpu.mem_hits_batch(flat, off, min_length, hit_max, bool(sample), max_length=K)
        want = [f"order {K}"]
        want += [f"breaks {q} {int(boff[q + 1] - boff[q])}" for q in range(len(pats))]
        want += [f"break {i} " + " ".join(str(int(x)) for x in brk[i]) for i in range(brk.shape[0])]
        want += [f"pattern {q} {int(moff[q + 1] - moff[q])}" for q in range(len(pats))]
        want += [f"mem {i} " + " ".join(str(int(x)) for x in mems[i]) for i in range(mems.shape[0])]
        want += [" ".join(["hits", str(i), str(int(hoff[i + 1] - hoff[i]))] + [str(int(v)) for v in hits[int(hoff[i]):int(hoff[i + 1])]])
                 for i in range(mems.shape[0])]
        assert out.stdout.strip().split("\n") == want, (min_length, hit_max, sample)
        assert mems.shape[0] > 0 and hits.shape[0] > 0 and int(mems[:, 1].max()) == K
        assert not np.array_equal(brk, gpu.match_breaks_batch(flat, off, min_length)[1])
    gpu.close()
