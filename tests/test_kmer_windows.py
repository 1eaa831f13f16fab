"""Batched k-mer windows (gcsa2_kmer_windows_device / gcsa2_kmer_windows_batch, kernels_windows.hpp): find() and count() of
every window P_q[j stride, j stride + k) of every read, with per-read profiles.  The expectations are the CPU oracle's find()
and count() of each window handed over as a pattern of its own (the contract in include/gcsa2_hip.h), computed once per graph
and window length at stride 1 -- the windows of any other stride are a subset of those -- and left unchanged."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from workload.rng import SplitMix64
from gcsa2_amd.hostview import concat_patterns
from test_oracle import CASES, COMP2CHAR
from test_mem_hits import EDGE, SENTINEL, substituted
from test_extend import GRAPHS, BIG, indexed, is_empty

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
COUNTS = 1                          # GCSA2_KMER_COUNTS
INVALID, MISSING, TOO_SMALL = -1, -5, -6
FIXED_K = (1, 2, 3, 16, 23, 24, 25, 26, 31, 32, 33)      # plus kmer_k - 1, kmer_k, kmer_k + 1 of the image


def all_k(kmer_k):
    """The window lengths of the issue for an image whose seed table has kmer_k (gcsa2_kmer_table_k)."""
    return sorted(set(FIXED_K) | {k for k in (kmer_k - 1, kmer_k, kmer_k + 1) if k >= 1})


def strides(k):
    return sorted({1, 3, k, k + 5})


def walks(g, seed, count, lo=40, hi=63):
    """Walks through the graph of lo .. hi characters."""
    rng = SplitMix64(seed)
    out = []
    for _ in range(count):
        v = rng.below(g.size)
        s = []
        for _ in range(lo + rng.below(hi - lo + 1)):
            s.append(COMP2CHAR[int(g.comp[v])])
            succ = g.successors(v)
            v = int(succ[rng.below(len(succ))])
        out.append("".join(s).encode())
    return out


def with_n(pats, seed):
    """Each pattern with one base replaced by N."""
    rng = SplitMix64(seed)
    out = []
    for p in pats:
        j = rng.below(len(p))
        out.append(p[:j] + b"N" + p[j + 1:])
    return out


@functools.lru_cache(maxsize=None)
def reads_of(which):
    """The reads of tests 1, 2 and 5 for one graph: walks of 40..63 characters, the same with a substitution about every 12
    characters, the walks with one N, and the edge patterns."""
    g = GRAPHS[which][1]
    base = walks(g, 0x4B10 + which, 100 if which == BIG else 16)
    return base + substituted(base, 0x4B20 + which, period=12) + with_n(base, 0x4B30 + which) + EDGE


def window_count(length, k, stride):
    return 0 if length < k else (length - k) // stride + 1


class Expected:
    """The oracle's answers for one batch of reads: per k the ranges and counts of every stride-1 window, in read order."""

    def __init__(self, cpu, reads):
        self.cpu, self.reads = cpu, reads
        self.by_k = {}

    def stride1(self, k):
        if k not in self.by_k:
            wins = [r[j:j + k] for r in self.reads for j in range(window_count(len(r), k, 1))]
            starts = np.cumsum([0] + [window_count(len(r), k, 1) for r in self.reads])
            if wins:
                data, off = concat_patterns(wins)
                ranges = self.cpu.find_batch(data, off, threads=2)
                counts = self.cpu.count_batch(ranges, threads=2)
            else:
                ranges, counts = np.zeros((0, 2), dtype=np.uint64), np.zeros(0, dtype=np.uint64)
            self.by_k[k] = (starts, ranges, counts, wins)
        return self.by_k[k]

    def want(self, k, stride, counts=True):
        """(window_offsets, profiles, ranges, counts) of the contract."""
        starts, ranges, cnt, _ = self.stride1(k)
        pick, woff = [], [0]
        for q, r in enumerate(self.reads):
            w = window_count(len(r), k, stride)
            pick += [int(starts[q]) + j * stride for j in range(w)]
            woff.append(woff[-1] + w)
        pick = np.asarray(pick, dtype=np.int64)
        rng, c = ranges[pick], cnt[pick]
        nonempty = ((rng[:, 0] + np.uint64(1)) <= (rng[:, 1] + np.uint64(1))) if len(pick) else np.zeros(0, dtype=bool)
        assert [bool(x) for x in nonempty[:50]] == [not is_empty((int(a), int(b))) for a, b in rng[:50].tolist()]
        length = np.where(nonempty, rng[:, 1] + np.uint64(1) - rng[:, 0], np.uint64(0)).astype(np.uint64)
        prof = np.zeros((len(self.reads), 4), dtype=np.uint64)
        for q in range(len(self.reads)):
            a, b = woff[q], woff[q + 1]
            prof[q] = (b - a, int(nonempty[a:b].sum()), int(length[a:b].sum()), int(c[a:b].sum()) if counts else 0)
        return np.asarray(woff, dtype=np.uint64), prof, rng, c

    def classes(self, k):
        """(found, emptied by an LF step, emptied by charRange) among the stride-1 windows."""
        _, ranges, _, wins = self.stride1(k)
        last_empty = {c: is_empty(self.cpu.find(bytes([c]))) for c in {w[-1] for w in wins}}
        found = lf = cr = 0
        for w, (a, b) in zip(wins, ranges.tolist()):
            if not is_empty((a, b)):
                found += 1
            elif last_empty[w[-1]]:
                cr += 1
            else:
                lf += 1
        return found, lf, cr


@functools.lru_cache(maxsize=None)
def expected(which):
    return Expected(indexed(which)[1], reads_of(which))


def assert_not_vacuous(exp, ks):
    """At stride 1 every k <= 32 meets found windows, windows emptied by a failed LF step and windows emptied by charRange.
    (k = 1 takes no LF step at all -- find() of one character IS its charRange -- so it cannot hold the second class; there
    the empties must all be charRange's.)"""
    counted = {k: exp.classes(k) for k in ks if k <= 32}
    for k, (found, lf, cr) in counted.items():
        assert found >= 50 and cr >= 5, (k, found, lf, cr)
        assert lf >= 50 if k >= 2 else lf == 0, (k, found, lf, cr)
    _, _, counts, _ = exp.stride1(4)
    assert int(counts.max()) > 1                        # count() is not the range length everywhere


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_library_exports_kmer_windows_and_refuses_a_null_index():
    """The built library exports both calls; each refuses a NULL index with INVALID_ARGUMENT without a device, names the index
    and writes nothing."""
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    assert "gcsa2_kmer_windows_device" in binding.EXPORTS and "gcsa2_kmer_windows_batch" in binding.EXPORTS
    for name in ("gcsa2_kmer_windows_device", "gcsa2_kmer_windows_batch"):
        assert hasattr(ctypes.CDLL(binding.LIB_PATH), name), name
    lib = binding.load_library()
    off = (ctypes.c_uint64 * 2)(0, 8)
    pat = (ctypes.c_uint8 * 8)(*b"ACGTACGT")
    woff = (ctypes.c_uint64 * 2)(7, 7)
    prof = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    rng = (ctypes.c_uint64 * 10)(*([7] * 10))
    total = ctypes.c_uint64(7)
    rc = lib.gcsa2_kmer_windows_device(None, ctypes.addressof(pat), ctypes.addressof(off), 1, 4, 1, 0, ctypes.addressof(woff), ctypes.addressof(prof),
                                       ctypes.addressof(rng), None, 5, ctypes.byref(total), None)
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    rc = lib.gcsa2_kmer_windows_batch(None, pat, off, 1, 4, 1, 0, ctypes.addressof(woff), ctypes.addressof(prof), ctypes.addressof(rng), None, 5,
                                      ctypes.byref(total))
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    assert list(woff) == [7, 7] and list(prof) == [7] * 4 and list(rng) == [7] * 10 and total.value == 7


def test_the_large_batch_holds_every_class():
    """The batch the GPU tests run on the 6000-base graph meets the conditions they rely on (asserted there again for the
    window lengths the image's seed table adds), whatever the seed table's k is."""
    assert_not_vacuous(expected(BIG), range(1, 34))


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

    def windows(self, gpu, k, stride, flags=0, offsets=True, profiles=True, ranges=True, counts=False, capacity=0, guard=8):
        """gcsa2_kmer_windows_device on sentinel-filled buffers with `guard` windows behind the capacity: (total or Gcsa2Error,
        window_offsets, profiles, ranges, counts) as numpy, whole buffers (guards included), None for what was not passed."""
        import torch
        from gcsa2_amd.binding import Gcsa2Error
        s = np.uint64(SENTINEL).view(np.int64).item()

        def buf(wanted, *shape):
            return torch.full(shape, s, dtype=torch.int64, device=self.dev) if wanted else None

        d_woff, d_prof = buf(offsets, self.n + 1 + guard), buf(profiles, self.n + guard, 4)
        d_rng, d_cnt = buf(ranges, capacity + guard, 2), buf(counts, capacity + guard)
        ptr = [0 if t is None else t.data_ptr() for t in (d_woff, d_prof, d_rng, d_cnt)]
        try:
            result = gpu.kmer_windows_device(self.d_pat.data_ptr(), self.d_off.data_ptr(), self.n, k, stride, flags, ptr[0], ptr[1], ptr[2], ptr[3], capacity, 0)
        except Gcsa2Error as e:
            result = e
        torch.cuda.synchronize()
        return (result,) + tuple(None if t is None else t.cpu().numpy().view(np.uint64) for t in (d_woff, d_prof, d_rng, d_cnt))


def assert_windows(got, want, n, what, counts=True):
    """A device call's buffers against the contract's (window_offsets, profiles, ranges, counts); the guards are intact."""
    total, woff, prof, rng, cnt = got
    w_off, w_prof, w_rng, w_cnt = want
    t = int(w_off[-1])
    assert total == t, (what, total, t)
    sentinel = np.uint64(SENTINEL)
    if woff is not None:
        assert np.array_equal(woff[:n + 1], w_off) and (woff[n + 1:] == sentinel).all(), what
    if rng is not None:
        bad = np.nonzero((rng[:t] != w_rng).any(axis=1))[0]
        assert bad.size == 0, (what, int(bad.size), int(bad[0]), rng[bad[0]].tolist(), w_rng[bad[0]].tolist())
        assert (rng[t:] == sentinel).all(), what
    if cnt is not None:
        assert np.array_equal(cnt[:t], w_cnt) and (cnt[t:] == sentinel).all(), what
    if prof is not None:
        w = w_prof if counts else np.concatenate([w_prof[:, :3], np.zeros((n, 1), dtype=np.uint64)], axis=1)
        bad = np.nonzero((prof[:n] != w).any(axis=1))[0]
        assert bad.size == 0, (what, int(bad.size), int(bad[0]), prof[bad[0]].tolist(), w[bad[0]].tolist())
        assert (prof[n:] == sentinel).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_parity_with_the_oracle(engine, which):
    """1. Every range bit for bit, every count, every profile and the window offsets, for every k and stride of the issue."""
    exp = expected(which)
    reads = reads_of(which)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    ks = all_k(gpu.kmer_table_k())
    if which == BIG:
        assert gpu.kmer_table_k() > 1 and gpu.pair_block_bytes() > 0
        assert_not_vacuous(exp, ks)
    batch = DeviceReads(reads)
    for k in ks:
        for stride in strides(k):
            want = exp.want(k, stride)
            t = int(want[0][-1])
            got = batch.windows(gpu, k, stride, COUNTS, counts=True, capacity=t)
            assert_windows(got, want, len(reads), (GRAPHS[which][0], k, stride))
    gpu.close()


def find_device(gpu, reads):
    """gcsa2_find_device of `reads` as patterns of their own."""
    import torch
    b = DeviceReads(reads)
    out = torch.zeros((max(b.n, 1), 2), dtype=torch.int64, device=b.dev)
    gpu.find_device(b.d_pat.data_ptr(), b.d_off.data_ptr(), b.n, out.data_ptr(), 0)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)[:b.n]


def materialised(reads, k, stride):
    return [r[j * stride:j * stride + k] for r in reads for j in range(window_count(len(r), k, stride))]


@pytest.mark.gpu
def test_every_table_shape(engine, big, monkeypatch):
    """2. The ranges are gcsa2_find_device's on the materialised windows with and without pair blocks, with the seed table
    at 0, 4 and its default, and on a find-only image that has a jump table; counts on that image are refused."""
    reads = reads_of(BIG)
    batch = DeviceReads(reads)
    default_k = big.kmer_table_k()
    ks = all_k(default_k)
    wins = {(k, s): materialised(reads, k, s) for k in ks for s in (1, 3)}

    def compare(gpu, what):
        for (k, s), w in wins.items():
            want = find_device(gpu, w)
            total, _, prof, rng, _ = batch.windows(gpu, k, s, 0, capacity=len(w))
            assert total == len(w) and np.array_equal(rng[:total], want), (what, k, s)
            assert int(prof[:len(reads), 0].sum()) == total, (what, k, s)

    try:
        for pair_blocks in (1, 0):
            for kmer_k in (0, 4, default_k):
                big.set_tables(pair_blocks=pair_blocks, kmer_k=kmer_k)
                assert (big.pair_block_bytes() > 0) == bool(pair_blocks) and big.kmer_table_k() == kmer_k
                compare(big, (pair_blocks, kmer_k))
    finally:
        big.set_tables(pair_blocks=1, kmer_k=default_k)
    monkeypatch.setenv("GCSA2_JUMP_TABLE", "1")
    find_only = engine.GCSA(indexed(BIG)[0], with_samples=False, with_counters=False, with_lcp=False)
    monkeypatch.delenv("GCSA2_JUMP_TABLE")
    assert find_only.jump_table_bytes() > 0
    compare(find_only, "find-only")
    for counts in (False, True):
        got = batch.windows(find_only, 16, 1, COUNTS, counts=counts, capacity=len(wins[(16, 1)]))
        assert got[0].code == MISSING, got[0]
        assert all((a == np.uint64(SENTINEL)).all() for a in got[1:] if a is not None)
    find_only.close()


@functools.lru_cache(maxsize=None)
def edge_reads():
    """3. The reads of the edge test: for (k, stride) = (16, 3), lengths 0, k - 1, k, k + 1, k + stride - 1, k + stride; 200
    reads of one window each; one read of 1000 windows; reads of 33..40 characters, so that reads start at every byte residue;
    a last read that ends the buffer."""
    g = GRAPHS[BIG][1]
    k, stride = 16, 3
    rng = SplitMix64(0x4B40)

    def walk_from(v, length):                           # from the first half of the backbone: never reaches the sink
        s = []
        for _ in range(length):
            s.append(COMP2CHAR[int(g.comp[v])])
            succ = g.successors(v)
            v = int(succ[rng.below(len(succ))])
        assert "$" not in s and "#" not in s
        return "".join(s).encode()

    pool = [walk_from(1 + rng.below(2500), 64) for _ in range(260)]
    reads = [pool[i][:n] for i, n in enumerate((0, k - 1, k, k + 1, k + stride - 1, k + stride))]
    reads += [pool[10 + i][i % 40:i % 40 + k + (i % stride)] for i in range(200)]            # one window each
    reads += [walk_from(1 + rng.below(2500), 1000 * stride + k - stride)]                    # 1000 windows
    reads += [pool[230 + i][:33 + i] for i in range(8)] + substituted([pool[240 + i][:33 + i] for i in range(8)], 0x4B41, period=12)
    reads += [pool[250][:47]]
    return k, stride, reads


@pytest.mark.gpu
def test_read_edges(big):
    k, stride, reads = edge_reads()
    _, off = concat_patterns(reads)
    assert {int(o) % 8 for o in off[:-1]} == set(range(8))
    assert [window_count(len(r), k, stride) for r in reads[:6]] == [0, 0, 1, 1, 1, 2]
    assert all(window_count(len(r), k, stride) == 1 for r in reads[6:206]) and window_count(len(reads[206]), k, stride) == 1000
    exp = Expected(indexed(BIG)[1], reads)
    batch = DeviceReads(reads)
    assert batch.d_pat.shape[0] == int(off[-1]) + 8
    for kk, ss in ((k, stride), (k, 1), (1, 1), (33, 7), (40, 1)):
        want = exp.want(kk, ss)
        got = batch.windows(big, kk, ss, COUNTS, counts=True, capacity=int(want[0][-1]))
        assert_windows(got, want, len(reads), (kk, ss))
        host = big.kmer_windows_batch(*concat_patterns(reads), kk, ss, counts=True)
        for a, b in zip(host, want):
            assert np.array_equal(a, b), (kk, ss)
    found = exp.want(k, stride)[1][:, 1]
    assert int(found[206]) == 1000 and int(found[6:206].sum()) == 200                      # walks: every window is found
    # no reads at all
    empty = DeviceReads([])
    got = empty.windows(big, 16, 1, 0, capacity=0)
    assert got[0] == 0 and int(got[1][0]) == 0 and (got[1][1:] == np.uint64(SENTINEL)).all()
    assert all((a == np.uint64(SENTINEL)).all() for a in got[2:] if a is not None)
    woff, prof, rng, cnt = big.kmer_windows_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 16, 1, counts=True)
    assert woff.tolist() == [0] and prof.shape == (0, 4) and rng.shape == (0, 2) and cnt.shape == (0,)


def host_call(gpu, reads, k, stride, flags, offsets=True, profiles=True, ranges=True, counts=False, capacity=0, guard=8, null_index=False):
    """gcsa2_kmer_windows_batch on sentinel-filled numpy buffers: (status, total, window_offsets, profiles, ranges, counts)."""
    data, off = concat_patterns(reads)
    data, off = np.ascontiguousarray(data, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64)
    n = len(reads)

    def buf(wanted, *shape):
        return np.full(shape, SENTINEL, dtype=np.uint64) if wanted else None

    arrays = (buf(offsets, n + 1 + guard), buf(profiles, n + guard, 4), buf(ranges, capacity + guard, 2), buf(counts, capacity + guard))
    total = ctypes.c_uint64(SENTINEL)
    rc = gpu._L.gcsa2_kmer_windows_batch(None if null_index else gpu._h, data.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                         off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n, k, stride, flags,
                                         *[None if a is None else a.ctypes.data for a in arrays], capacity, ctypes.byref(total))
    return (rc, total.value) + arrays


def untouched(arrays):
    return all((a == np.uint64(SENTINEL)).all() for a in arrays if a is not None)


@pytest.mark.gpu
def test_capacities_and_nulls(big):
    """4. A short buffer is refused with the total and nothing written (the device form completes the window offsets), an
    exact one is filled and nothing lies behind it, every output may be NULL, and every invalid argument is refused."""
    reads = reads_of(BIG)[90:130] + EDGE
    n = len(reads)
    exp = Expected(indexed(BIG)[1], reads)
    k, stride = 12, 2
    want = exp.want(k, stride)
    t = int(want[0][-1])
    batch = DeviceReads(reads)
    # one window short
    got = batch.windows(big, k, stride, COUNTS, counts=True, capacity=t - 1)
    assert got[0].code == TOO_SMALL and got[0].needed == t
    assert np.array_equal(got[1][:n + 1], want[0]) and untouched(got[2:])
    rc, total, *arrays = host_call(big, reads, k, stride, COUNTS, counts=True, capacity=t - 1)
    assert rc == TOO_SMALL and total == t and untouched(arrays)
    # exactly enough
    assert_windows(batch.windows(big, k, stride, COUNTS, counts=True, capacity=t), want, n, "exact")
    rc, total, woff, prof, rng, cnt = host_call(big, reads, k, stride, COUNTS, counts=True, capacity=t)
    assert rc == 0
    assert_windows((total, woff, prof, rng, cnt), want, n, "exact, host")
    # subsets of the outputs; the capacity is ignored without ranges and counts
    no_counts = exp.want(k, stride, counts=False)
    for form in ("device", "host"):
        for kw, flags in ((dict(offsets=False, ranges=False), 0), (dict(offsets=False, ranges=False), COUNTS),
                          (dict(offsets=False, profiles=False), 0), (dict(profiles=False, ranges=False, counts=True), COUNTS),
                          (dict(profiles=False, ranges=False), 0), (dict(offsets=False, profiles=False, ranges=False), COUNTS)):
            cap = t if kw.get("ranges", True) or kw.get("counts") else 0
            if form == "device":
                got = batch.windows(big, k, stride, flags, capacity=cap, **kw)
            else:
                rc, *got = host_call(big, reads, k, stride, flags, capacity=cap, **kw)
                assert rc == 0
            assert_windows(tuple(got), want if flags else no_counts, n, (form, kw, flags), counts=bool(flags))
    # invalid arguments: nothing is written, the total included
    for kk, ss, flags, counts in ((0, 1, 0, False), (4, 0, 0, False), (4, 1, 0, True), (4, 1, 2, False), (4, 1, COUNTS | 4, True)):
        got = batch.windows(big, kk, ss, flags, counts=counts, capacity=t)
        assert got[0].code == INVALID and untouched(got[1:]), (kk, ss, flags, counts)
        rc, total, *arrays = host_call(big, reads, kk, ss, flags, counts=counts, capacity=t)
        assert rc == INVALID and total == SENTINEL and untouched(arrays), (kk, ss, flags, counts)
    rc, total, *arrays = host_call(big, reads, k, stride, 0, capacity=t, null_index=True)
    assert rc == INVALID and total == SENTINEL and untouched(arrays)
    # the host form refuses offsets that do not start at 0 or decrease
    for bad in ([1, 20, 40], [0, 40, 20]):
        off = np.asarray(bad, dtype=np.uint64)
        total = ctypes.c_uint64(SENTINEL)
        out = np.full(8, SENTINEL, dtype=np.uint64)
        rc = big._L.gcsa2_kmer_windows_batch(big._h, np.zeros(64, dtype=np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                             off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 2, 4, 1, 0, out.ctypes.data, None, None, None, 0,
                                             ctypes.byref(total))
        assert rc == INVALID and untouched([out]), bad


@pytest.mark.gpu
def test_host_form_equals_the_device_form(big):
    """5a. On the batch of test 1."""
    reads = reads_of(BIG)
    data, off = concat_patterns(reads)
    batch = DeviceReads(reads)
    for k in all_k(big.kmer_table_k()):
        for stride in strides(k):
            woff, prof, rng, cnt = big.kmer_windows_batch(data, off, k, stride, counts=True)
            t = int(woff[-1])
            got = batch.windows(big, k, stride, COUNTS, counts=True, capacity=t)
            assert_windows(got, (woff, prof, rng, cnt), len(reads), (k, stride))


@pytest.mark.gpu
def test_host_form_in_pieces(engine, monkeypatch):
    """5b. About 3 MB of 100-base walks of the 2^16-base SNP graph in 1 MB pieces equal the same batch in one piece, in every
    output.  Library against library."""
    from workload import builder, graphs, patterns
    g = graphs.snp_graph(1 << 16, 0x4E1, 0x4E2, snp_period=16, node_len=16)
    ix = builder.build(g, 32, sample_period=8, branching=4)
    whole, _ = engine.open_index(ix, device=0)
    monkeypatch.setenv("GCSA2_MS_PIECE_MB", "1")
    pieced, _ = engine.open_index(ix, device=0)
    reads = substituted([bytes(p) for p in patterns.walk_patterns(g, 32_000, 100, 0x4E5)], 0x4E6, period=40)
    reads[5] = reads[5][:20]                            # a read without windows in the first piece
    flat, off = concat_patterns(reads)
    assert int(off[-1]) >= 3 << 20
    for k, stride, counts in ((32, 1, True), (21, 4, False)):
        a = pieced.kmer_windows_batch(flat, off, k, stride, counts=counts)
        b = whole.kmer_windows_batch(flat, off, k, stride, counts=counts)
        assert int(a[0][-1]) == sum(window_count(len(r), k, stride) for r in reads) > 500_000
        for x, y in zip(a, b):
            assert (x is None and y is None) or np.array_equal(x, y), (k, stride)
        assert 0 < int(a[1][:, 1].sum()) < int(a[0][-1])                  # found and not found windows
        only = pieced.kmer_windows_batch(flat, off, k, stride, ranges=False, occurrences=counts)
        assert only[2] is None and only[3] is None and np.array_equal(only[1], a[1]), (k, stride)
    pieced.close()
    whole.close()


@pytest.mark.gpu
def test_facade_kmer_windows(engine, tmp_path):
    """6. GCSA::kmer_windows_batch from a C++ client (tests/cpp/kmer_windows_client.cpp) prints what GCSA.kmer_windows_batch
    returns."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    which = len(CASES) - 1
    reads = reads_of(which)
    assert all(b"\n" not in r for r in reads)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    save_host_view(indexed(which)[0], str(tmp_path / "index.g2hv"))
    (tmp_path / "reads.txt").write_bytes(b"".join(r + b"\n" for r in reads))
    exe = compile_client(str(tmp_path / "kmer_windows_client"), os.path.join(ROOT, "tests", "cpp", "kmer_windows_client.cpp"))
    data, off = concat_patterns(reads)
    for k, stride, counts in ((5, 1, 1), (7, 3, 0)):
        out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "reads.txt"), str(k), str(stride), str(counts)],
                             capture_output=True, text=True, env=_run_env(), timeout=300)
        assert out.returncode == 0, out.stderr
        woff, prof, rng, cnt = gpu.kmer_windows_batch(data, off, k, stride, counts=bool(counts))
        lines = [f"read {q} " + " ".join(str(int(x)) for x in row) for q, row in enumerate(prof)]
        lines += [f"window {w} {int(r[0])} {int(r[1])} {int(cnt[w]) if counts else 0}" for w, r in enumerate(rng)]
        assert int(woff[-1]) == len(rng) > 0 and out.stdout.strip().split("\n") == lines
    gpu.close()
