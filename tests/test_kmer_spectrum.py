"""Index k-mer spectrum (gcsa2_kmer_spectrum / gcsa2_list_kmers / gcsa2_index_kmer_support_device, kernels_kmers.hpp): the
k-mers of the index itself, binned by value, listed, or summed per bin of located values.  The expectations are the CPU
oracle's alone: a Python walk over OracleIndex.LF_fast / LF_all from the root gives the states of depth k and their keys,
count_batch their values, and the Folded / tally helpers of test_kmer_support (locate_batch once per distinct range) the
support."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from workload import graphs
from gcsa2_amd.hostview import concat_patterns
from test_mem_hits import SENTINEL
from test_oracle import COMP2CHAR
from test_extend import GRAPHS as SMALL_GRAPHS, BIG, indexed as small_indexed, is_empty
from test_kmer_support import Oracle, FIELDS, START, fresh_support, assert_support, full_bins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
INVALID, MISSING, TOO_SMALL = -1, -5, -6
COUNTS = 1                                              # GCSA2_SPECTRUM_COUNTS
PER_BIN = 1                                             # GCSA2_SUPPORT_PER_BIN
NODE_SHIFT = 11
STATS = ("kmers", "nodes", "occurrences", "unique", "max_value")
GUARD = 16
N_HIST = (0, 1, 2, 64, 4096)
WINDOWS = ((0, 0), (1, 1), (2, 0), (64, 0))
REPEAT = len(SMALL_GRAPHS)                              # index of the repeat-rich graph in GRAPHS
GRAPHS = SMALL_GRAPHS + [("repeat", graphs.repeat_graph(16384, 0xB7, 0xB8, snp_period=24, node_len=16), 16)]
NAMES = [c[0] for c in GRAPHS]


@functools.lru_cache(maxsize=None)
def indexed(which):
    if which != REPEAT:
        return small_indexed(which)
    from oracle.oracle import OracleIndex
    from workload import builder
    ix = builder.build(GRAPHS[which][1], GRAPHS[which][2], sample_period=8, branching=4)
    return ix, OracleIndex(ix)


def depths(which):
    K = GRAPHS[which][2]
    return sorted({1, 2, 3, K // 2, K, K + 2})


class Levels:
    """The search tree of countKMers for one (graph, include_Ns), level by level and kept: (ranges, keys) per depth, the key an
    int with the comp of extension step i at bits [3i, 3i + 3)."""

    def __init__(self, which, ns):
        self.ix, self.cpu = indexed(which)
        self.ns = ns
        self.limit = int(self.ix.sigma) - 2 if ns else int(self.ix.fast_chars)
        self.levels = [[((0, self.cpu.n - 1), 0)] if self.cpu.n > 0 else []]

    def at(self, k):
        while len(self.levels) <= k:
            d = len(self.levels) - 1
            step = self.cpu.LF_all if self.ns else self.cpu.LF_fast
            nxt = []
            for r, key in self.levels[d]:
                children = step(r)
                for c in range(1, self.limit + 1):
                    if not is_empty(children[c]):
                        nxt.append((children[c], key | (c << (3 * d))))
            self.levels.append(nxt)
        return self.levels[k]


@functools.lru_cache(maxsize=None)
def levels_of(which, ns):
    return Levels(which, bool(ns))


class Expected:
    """K(k, include_Ns) of one graph: ranges (m, 2), keys (m, 3), count() and Range::length per state."""

    def __init__(self, which, k, ns):
        self.which, self.k = which, k
        self.cpu = indexed(which)[1]
        states = levels_of(which, ns).at(k)
        self.m = len(states)
        self.ranges = np.asarray([s[0] for s in states], dtype=np.uint64).reshape(-1, 2)
        self.keys = np.asarray([[(s[1] >> (64 * w)) & U64 for w in range(3)] for s in states], dtype=np.uint64).reshape(-1, 3)
        self.ints = [s[1] for s in states]
        self.nodes = (self.ranges[:, 1] + np.uint64(1) - self.ranges[:, 0]).astype(np.uint64)
        self.counts = self.cpu.count_batch(self.ranges, threads=2).astype(np.uint64) if self.m else np.zeros(0, dtype=np.uint64)

    def values(self, flags):
        return self.counts if flags & COUNTS else self.nodes

    def stats(self, flags):
        v = self.values(flags)
        return dict(kmers=self.m, nodes=int(self.nodes.sum()), occurrences=int(self.counts.sum()) if flags & COUNTS else 0,
                    unique=int((v == 1).sum()), max_value=int(v.max()) if self.m else 0)

    def histogram(self, flags, n_hist):
        if n_hist == 0:
            return np.zeros(0, dtype=np.uint64)
        v = np.minimum(self.values(flags), np.uint64(n_hist - 1)).astype(np.int64)
        return np.bincount(v, minlength=n_hist).astype(np.uint64)

    def records(self, flags, lo, hi):
        """The (m', 8) records of gcsa2_list_kmers for the window [lo, hi], as sorted tuples."""
        v = self.values(flags)
        keep = (v >= np.uint64(lo)) & (np.ones(self.m, dtype=bool) if hi == 0 else v <= np.uint64(hi))
        count = self.counts if flags & COUNTS else np.zeros(self.m, dtype=np.uint64)
        rows = np.column_stack([self.ranges, count, self.nodes, np.full(self.m, self.k, dtype=np.uint64), self.keys]) if self.m \
            else np.zeros((0, 8), dtype=np.uint64)
        return sorted(map(tuple, rows[keep].tolist()))

    def strings(self):
        return [decode(key, self.k) for key in self.ints]


def decode(key, k):
    """The k-mer of a key: step 0 is its LAST character."""
    return bytes(ord(COMP2CHAR[(key >> (3 * i)) & 7]) for i in range(k))[::-1]


def key_int(row):
    return int(row[5]) | (int(row[6]) << 64) | (int(row[7]) << 128)


@functools.lru_cache(maxsize=None)
def expected(which, k, ns):
    return Expected(which, k, bool(ns))


@functools.lru_cache(maxsize=None)
def fold_of(which, k, ns, hit_max):
    """The support expectation: the records {0, k, sp, ep} of K, weight 1 each, folded by test_kmer_support.Oracle."""
    exp = expected(which, k, ns)
    return support_oracle(which).fold(exp.ranges, exp.counts, None, hit_max)


@functools.lru_cache(maxsize=None)
def support_oracle(which):
    return Oracle(indexed(which)[1])


# ---- CPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    return binding.load_library()


def test_library_exports_the_spectrum_calls(lib):
    """1. The built library exports the three calls, binding.EXPORTS lists them, and each refuses a NULL index with
    GCSA2_ERR_INVALID_ARGUMENT, leaving sentinel-filled outputs as they were."""
    from gcsa2_amd import binding
    for name in ("gcsa2_kmer_spectrum", "gcsa2_list_kmers", "gcsa2_index_kmer_support_device"):
        assert name in binding.EXPORTS, name
        assert hasattr(ctypes.CDLL(binding.LIB_PATH), name), name
    assert binding.SPECTRUM_COUNTS == COUNTS and binding.SPECTRUM_STATS == STATS
    hist = (ctypes.c_uint64 * 8)(*([SENTINEL] * 8))
    stats = (ctypes.c_uint64 * 7)(*([SENTINEL] * 7))
    recs = (ctypes.c_uint64 * 16)(*([SENTINEL] * 16))
    total = ctypes.c_uint64(SENTINEL)
    assert lib.gcsa2_kmer_spectrum(None, 4, 0, 0, COUNTS, ctypes.addressof(hist), 8, ctypes.addressof(stats)) == INVALID
    assert lib.gcsa2_list_kmers(None, 4, 0, 0, COUNTS, 0, 0, ctypes.addressof(recs), 2, ctypes.byref(total)) == INVALID
    assert lib.gcsa2_index_kmer_support_device(None, 4, 0, 0, 0, NODE_SHIFT, 0, ctypes.addressof(hist), 8, ctypes.addressof(stats), None) == INVALID
    assert "index" in lib.gcsa2_last_error().decode()
    assert list(hist) == [SENTINEL] * 8 and list(stats) == [SENTINEL] * 7 and list(recs) == [SENTINEL] * 16 and total.value == SENTINEL


@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=NAMES)
def test_the_expectation_walk_is_count_kmers(which):
    """2. The test's own yardstick: the Python walk has as many states as the oracle's countKMers at every depth used below,
    for both alphabets, and every key decodes to a string whose oracle find() is the state's range."""
    cpu = indexed(which)[1]
    for ns in (False, True):
        for k in depths(which):
            exp = expected(which, k, ns)
            assert exp.m == cpu.count_kmers(k, ns, force=True), (NAMES[which], k, ns)
            if exp.m:
                strings = exp.strings()
                assert len(set(strings)) == exp.m, (NAMES[which], k, ns)
                found = cpu.find_batch(*concat_patterns(strings), threads=2)
                assert np.array_equal(found, exp.ranges), (NAMES[which], k, ns)


def test_the_graphs_are_not_vacuous():
    """What the cases below rely on: the repeat graph's spectrum at k = 8 reaches beyond 63 (n_hist = 64 has an overflow bin)
    and stays below 4095; distinct k-mers share ranges on the 6000-base graph at k = 16; rand7 has no 16-mer."""
    rep = expected(REPEAT, 8, False)
    assert rep.m == 15075 and int(rep.counts.max()) == 73 and int((rep.counts > 63).sum()) == 9
    assert np.count_nonzero(rep.histogram(COUNTS, 64)) == 22 and rep.histogram(COUNTS, 64)[63] == 9 and rep.histogram(COUNTS, 4096)[4095] == 0
    assert expected(REPEAT, 16, False).m == 28506 and int((expected(REPEAT, 16, False).counts > 63).sum()) == 4
    big = expected(BIG, 16, False)
    assert big.m == 27650 and np.unique(big.ranges, axis=0).shape[0] == 12566
    assert int(expected(BIG, 2, False).counts.max()) == 472 and int(expected(BIG, 3, False).counts.max()) == 149
    assert expected(BIG, 18, False).m == 33358
    assert expected(NAMES.index("rand7"), 16, False).m == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine():
    from gcsa2_amd import binding
    assert binding.device_count() >= 1, "no MI355X visible"
    return binding


def raw_spectrum(engine, gpu, k, ns, force, flags, n_hist, null_stats=False):
    """gcsa2_kmer_spectrum into n_hist words of garbage with GUARD sentinel words behind them: (rc, histogram, guard, stats)."""
    L = engine.load_library()
    buf = np.full(n_hist + GUARD, SENTINEL, dtype=np.uint64)
    buf[:n_hist] = 0x77
    stats = (ctypes.c_uint64 * 5)(*([SENTINEL] * 5))
    rc = L.gcsa2_kmer_spectrum(gpu.handle, k, int(ns), int(force), flags, buf.ctypes.data if n_hist else None, n_hist,
                               None if null_stats else ctypes.addressof(stats))
    return rc, buf[:n_hist].copy(), buf[n_hist:].copy(), dict(zip(STATS, (int(x) for x in stats)))


def raw_list(engine, gpu, k, ns, force, flags, lo, hi, capacity, null=False):
    """gcsa2_list_kmers into capacity records with GUARD sentinel records behind them: (rc, records, guard, total)."""
    L = engine.load_library()
    buf = np.full((capacity + GUARD, 8), SENTINEL, dtype=np.uint64)
    total = ctypes.c_uint64(SENTINEL)
    rc = L.gcsa2_list_kmers(gpu.handle, k, int(ns), int(force), flags, lo, hi, None if null else buf.ctypes.data, capacity, ctypes.byref(total))
    return rc, buf[:capacity], buf[capacity:], total.value


def index_support(gpu, k, ns, force, hit_max, shift, flags, n_bins):
    """gcsa2_index_kmer_support_device into n_bins words of START with sentinel words behind them: (stats, the whole buffer)."""
    import torch
    d = fresh_support(n_bins, torch.device("cuda", 0))
    stats = gpu.index_kmer_support_device(k, hit_max, shift, flags, d.data_ptr() if n_bins else 0, n_bins, include_Ns=ns, force=force)
    torch.cuda.synchronize()
    return stats, d.cpu().numpy().view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=NAMES)
def test_spectrum_parity(engine, which):
    """3. The histogram and every field of stats equal the oracle's for both alphabets, every depth (K + 2 with force), with and
    without GCSA2_SPECTRUM_COUNTS and for every n_hist; stats.kmers is count_kmers; the bins sum to it; the words behind n_hist
    are untouched; k > order without force gives zeros."""
    K = GRAPHS[which][2]
    gpu = engine.GCSA(indexed(which)[0])
    kmers = 0
    for ns in (False, True):
        for k in depths(which):
            exp = expected(which, k, ns)
            assert gpu.count_kmers(k, include_Ns=ns, force=True) == exp.m
            for flags in (0, COUNTS):
                want = exp.stats(flags)
                for n_hist in N_HIST:
                    what = (NAMES[which], ns, k, flags, n_hist)
                    rc, hist, guard, stats = raw_spectrum(engine, gpu, k, ns, k > K, flags, n_hist)
                    assert rc == 0 and stats == want, (what, rc, stats, want)
                    assert np.array_equal(hist, exp.histogram(flags, n_hist)), what
                    assert (n_hist == 0 or int(hist.sum()) == stats["kmers"]) and (guard == np.uint64(SENTINEL)).all(), what
                kmers += want["kmers"]
        rc, hist, guard, stats = raw_spectrum(engine, gpu, K + 2, ns, False, COUNTS, 64)
        assert rc == 0 and stats == dict.fromkeys(STATS, 0) and not hist.any() and (guard == np.uint64(SENTINEL)).all()
        assert raw_spectrum(engine, gpu, K, ns, False, COUNTS, 64, null_stats=True)[0] == 0
    if NAMES[which] == "rand7":
        rc, hist, _, stats = raw_spectrum(engine, gpu, 16, False, False, COUNTS, 64)
        assert rc == 0 and stats == dict.fromkeys(STATS, 0) and not hist.any()
    assert kmers > 0
    # the Python form
    k = min(3, K)
    hist, stats = gpu.kmer_spectrum(k, n_hist=64)
    assert stats == expected(which, k, False).stats(COUNTS) and np.array_equal(hist, expected(which, k, False).histogram(COUNTS, 64))
    gpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which,k", [(REPEAT, 8), (BIG, 3), (BIG, 16)], ids=["repeat-8", "snp6000-3", "snp6000-16"])
def test_list_parity(engine, which, k):
    """4. The records of every window, sorted, equal the oracle's; find_batch of the decoded keys returns the records' ranges;
    capacity == total succeeds, capacity == total - 1 is refused with *total exact and nothing written behind capacity; a
    sizing call with NULL works; k = 65 is refused."""
    gpu = engine.GCSA(indexed(which)[0])
    exp = expected(which, k, False)
    for flags in (COUNTS, 0):
        for lo, hi in WINDOWS:
            what = (NAMES[which], k, flags, lo, hi)
            want = exp.records(flags, lo, hi)
            rc, _, _, total = raw_list(engine, gpu, k, False, False, flags, lo, hi, 0, null=True)
            assert total == len(want) and rc == (TOO_SMALL if want else 0), (what, rc, total, len(want))
            rc, recs, guard, total = raw_list(engine, gpu, k, False, False, flags, lo, hi, len(want))
            assert rc == 0 and total == len(want) and (guard == np.uint64(SENTINEL)).all(), (what, rc, total)
            assert sorted(map(tuple, recs.tolist())) == want, what
            if want:
                rc, _, guard, total = raw_list(engine, gpu, k, False, False, flags, lo, hi, len(want) - 1)
                assert rc == TOO_SMALL and total == len(want) and (guard == np.uint64(SENTINEL)).all(), (what, rc, total)
                assert "capacity" in engine.load_library().gcsa2_last_error().decode()
    assert len(exp.records(COUNTS, 2, 0)) > 0 and (which != REPEAT or len(exp.records(COUNTS, 64, 0)) == 9)
    recs = gpu.list_kmers(k)
    assert sorted(map(tuple, recs.tolist())) == exp.records(COUNTS, 0, 0)
    strings = [decode(key_int(row), k) for row in recs.tolist()]
    assert np.array_equal(gpu.find_batch(*concat_patterns(strings)), recs[:, 0:2])
    sentinel = np.uint64(SENTINEL)
    rc, recs, guard, total = raw_list(engine, gpu, 65, False, True, 0, 0, 0, 4)
    assert rc == INVALID and total == SENTINEL and (recs == sentinel).all() and (guard == sentinel).all()
    gpu.close()


def seed_records(rows):
    """gcsa2_mem records {position 0, length k, sp, ep, count} of list_kmers rows."""
    return np.ascontiguousarray(np.column_stack([np.zeros(rows.shape[0], dtype=np.uint64), rows[:, 4], rows[:, 0], rows[:, 1], rows[:, 2]]))


@pytest.mark.gpu
@pytest.mark.parametrize("which,k", [(REPEAT, 8), (BIG, 16), (NAMES.index("snp"), 6)], ids=["repeat-8", "snp6000-16", "snp-6"])
def test_index_support_parity(engine, which, k):
    """5. d_support -- pre-filled, because the call adds -- and all seven stats fields equal tally() of the records {0, k, sp, ep}
    of K for every cap, shift and flag, with n_bins once holding every bin and once so small that dropped > 0; windows == found ==
    the spectrum's kmers; and the array equals gcsa2_seed_support_device on the uploaded records of list_kmers."""
    import torch
    gpu = engine.GCSA(indexed(which)[0])
    exp = expected(which, k, False)
    rows = gpu.list_kmers(k)
    d_seeds = torch.from_numpy(seed_records(rows).view(np.int64)).to(torch.device("cuda", 0))
    dropped = 0
    for hit_max in (0, 1, 3):
        fold = fold_of(which, k, False, hit_max)
        for shift in (0, NODE_SHIFT):
            full = full_bins(fold, shift)
            for flags in (0, PER_BIN):
                for n_bins in (full, full // 2):
                    what = (NAMES[which], k, hit_max, shift, flags, n_bins)
                    want = fold.tally(shift, bool(flags), n_bins)
                    got = index_support(gpu, k, False, False, hit_max, shift, flags, n_bins)
                    assert_support(got, want, n_bins, what)
                    assert got[0]["windows"] == got[0]["found"] == exp.m, what
                    dropped += want[1]["dropped"]
                    d = fresh_support(n_bins, d_seeds.device)
                    composed = gpu.seed_support_device(d_seeds.data_ptr(), rows.shape[0], 0, hit_max, shift, flags, d.data_ptr() if n_bins else 0, n_bins)
                    torch.cuda.synchronize()
                    assert composed == got[0] and np.array_equal(d.cpu().numpy().view(np.uint64), got[1]), what
    assert dropped > 0
    if which == BIG:
        support, stats = gpu.index_kmer_support(k, full_bins(fold_of(which, k, False, 3), NODE_SHIFT), hit_max=3)
        add, want = fold_of(which, k, False, 3).tally(NODE_SHIFT, False, support.shape[0])
        assert stats == want and np.array_equal(support, add)
    gpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("piece", ["4", "50"])
def test_pieces_change_nothing(engine, monkeypatch, piece):
    """6. With GCSA2_KMER_PIECE at 4 and 50 states (set before the index is created) every level is walked in many pieces: the
    histogram, the stats, the record set and the support array are those of the default piece -- and the oracle's --; of the
    support stats, distinct and values are per-piece sums, at least the one-piece figures."""
    k = 8
    for name in ("rand4", "snp", "snp6000"):
        which = NAMES.index(name)
        force = k > GRAPHS[which][2]
        exp = expected(which, k, False)
        plain = engine.GCSA(indexed(which)[0])
        monkeypatch.setenv("GCSA2_KMER_PIECE", piece)
        cut = engine.GCSA(indexed(which)[0])
        monkeypatch.delenv("GCSA2_KMER_PIECE")
        fold = fold_of(which, k, False, 3)
        n_bins = full_bins(fold, NODE_SHIFT) - 1
        results = []
        for gpu in (plain, cut):
            hist, stats = gpu.kmer_spectrum(k, n_hist=64, force=force)
            recs = sorted(map(tuple, gpu.list_kmers(k, force=force).tolist()))
            results.append((hist, stats, recs, index_support(gpu, k, False, force, 3, NODE_SHIFT, 0, n_bins)))
            assert gpu.count_kmers(k, force=force) == exp.m
        (hist_a, stats_a, recs_a, sup_a), (hist_b, stats_b, recs_b, sup_b) = results
        assert stats_a == stats_b == exp.stats(COUNTS) and np.array_equal(hist_a, hist_b) and np.array_equal(hist_a, exp.histogram(COUNTS, 64)), name
        assert recs_a == recs_b == exp.records(COUNTS, 0, 0), name
        assert expected(which, k - 1, False).m * levels_of(which, False).limit > 2 * int(piece), (name, "the last level is cut")
        want = fold.tally(NODE_SHIFT, False, n_bins)
        assert_support(sup_a, want, n_bins, (name, "one piece"))
        for f in FIELDS:
            if f in ("distinct", "values"):
                assert sup_b[0][f] >= sup_a[0][f], (name, f)
            else:
                assert sup_b[0][f] == sup_a[0][f], (name, f)
        assert np.array_equal(sup_a[1], sup_b[1]), name
        plain.close()
        cut.close()


@pytest.mark.gpu
@pytest.mark.parametrize("groups", ["1", "3"])
def test_leaf_groups_change_nothing(engine, monkeypatch, groups):
    """6b. The last level's kernel runs a bounded number of workgroups, each over every gridDim.x-th tile of 256 states; the
    graphs here have fewer tiles than the default holds workgroups.  With GCSA2_SPECTRUM_GROUPS (read per call) at 1 and 3 a
    workgroup walks 8 to 100 tiles, the last of them partly filled: histogram, stats, records and support are the oracle's."""
    monkeypatch.setenv("GCSA2_SPECTRUM_GROUPS", groups)
    for which, k in ((BIG, 8), (REPEAT, 16)):
        exp = expected(which, k, False)
        assert expected(which, k - 1, False).m > 8 * 256 * int(groups) and expected(which, k - 1, False).m % 256 != 0
        gpu = engine.GCSA(indexed(which)[0])
        for flags in (0, COUNTS):
            rc, hist, guard, stats = raw_spectrum(engine, gpu, k, False, False, flags, 64)
            assert rc == 0 and stats == exp.stats(flags) and np.array_equal(hist, exp.histogram(flags, 64)), (NAMES[which], flags)
            assert (guard == np.uint64(SENTINEL)).all()
        assert sorted(map(tuple, gpu.list_kmers(k, min_value=2).tolist())) == exp.records(COUNTS, 2, 0), NAMES[which]
        fold = fold_of(which, k, False, 3)
        n_bins = full_bins(fold, NODE_SHIFT)
        assert_support(index_support(gpu, k, False, False, 3, NODE_SHIFT, PER_BIN, n_bins), fold.tally(NODE_SHIFT, True, n_bins), n_bins, NAMES[which])
        gpu.close()


@pytest.mark.gpu
def test_components_and_refusals(engine):
    """7. An image without samples answers the spectrum and the list exactly -- with GCSA2_SPECTRUM_COUNTS too, because it keeps
    its counters -- and refuses the support call; one without counters answers them without the flag and refuses the flag; every
    other refusal of the contract, one by one, with sentinel-filled outputs left as they were."""
    import torch
    which, k = BIG, 8
    ix = indexed(which)[0]
    exp = expected(which, k, False)
    L = engine.load_library()
    d = fresh_support(8, torch.device("cuda", 0))
    sentinel = np.uint64(SENTINEL)

    def support_refused(gpu, code, **change):
        arg = dict(k=k, hit_max=0, shift=NODE_SHIFT, flags=0, support=d.data_ptr(), n_bins=8)
        arg.update(change)
        stats = (ctypes.c_uint64 * 7)(*([SENTINEL] * 7))
        rc = L.gcsa2_index_kmer_support_device(gpu.handle, arg["k"], 0, 0, arg["hit_max"], arg["shift"], arg["flags"], arg["support"], arg["n_bins"],
                                               ctypes.addressof(stats), None)
        torch.cuda.synchronize()
        buf = d.cpu().numpy().view(np.uint64)
        assert rc == code and list(stats) == [SENTINEL] * 7 and (buf[:8] == np.uint64(START)).all() and (buf[8:] == sentinel).all(), (change, rc)

    find_only = engine.GCSA(ix, with_samples=False)
    bare = engine.GCSA(ix, with_samples=False, with_counters=False)
    for gpu, flag_sets in ((find_only, (0, COUNTS)), (bare, (0,))):
        for flags in flag_sets:
            rc, hist, guard, stats = raw_spectrum(engine, gpu, k, False, False, flags, 64)
            assert rc == 0 and stats == exp.stats(flags) and np.array_equal(hist, exp.histogram(flags, 64)) and (guard == sentinel).all()
            want = exp.records(flags, 2, 0)
            rc, recs, guard, total = raw_list(engine, gpu, k, False, False, flags, 2, 0, len(want))
            assert rc == 0 and total == len(want) and sorted(map(tuple, recs.tolist())) == want and (guard == sentinel).all()
        support_refused(gpu, MISSING)
    rc, hist, guard, stats = raw_spectrum(engine, bare, k, False, False, COUNTS, 64)
    assert rc == MISSING and (hist == np.uint64(0x77)).all() and (guard == sentinel).all() and set(stats.values()) == {SENTINEL}
    rc, recs, guard, total = raw_list(engine, bare, k, False, False, COUNTS, 0, 0, 4)
    assert rc == MISSING and total == SENTINEL and (recs == sentinel).all()
    find_only.close()
    bare.close()

    gpu = engine.GCSA(ix)
    for change in (dict(k=0), dict(flags=2), dict(flags=-1)):
        arg = dict(k=k, flags=COUNTS)
        arg.update(change)
        rc, hist, guard, stats = raw_spectrum(engine, gpu, arg["k"], False, False, arg["flags"], 64)
        assert rc == INVALID and (hist == np.uint64(0x77)).all() and (guard == sentinel).all() and set(stats.values()) == {SENTINEL}, change
        rc, recs, guard, total = raw_list(engine, gpu, arg["k"], False, False, arg["flags"], 0, 0, 4)
        assert rc == INVALID and total == SENTINEL and (recs == sentinel).all() and (guard == sentinel).all(), change
    stats = (ctypes.c_uint64 * 5)(*([SENTINEL] * 5))
    assert L.gcsa2_kmer_spectrum(gpu.handle, k, 0, 0, 0, None, 8, ctypes.addressof(stats)) == INVALID and list(stats) == [SENTINEL] * 5
    rc, recs, guard, total = raw_list(engine, gpu, k, False, False, COUNTS, 3, 2, 4)                  # min_value > max_value != 0
    assert rc == INVALID and total == SENTINEL and (recs == sentinel).all()
    rc, _, _, total = raw_list(engine, gpu, k, False, False, COUNTS, 0, 0, 4, null=True)               # NULL records with capacity > 0
    assert rc == INVALID and total == SENTINEL
    buf = np.full((4, 8), SENTINEL, dtype=np.uint64)
    assert L.gcsa2_list_kmers(gpu.handle, k, 0, 0, COUNTS, 0, 0, buf.ctypes.data, 4, None) == INVALID and (buf == sentinel).all()   # NULL total
    for change in (dict(k=0), dict(shift=64), dict(shift=U64), dict(flags=2), dict(flags=-1), dict(support=None)):
        support_refused(gpu, INVALID, **change)
    gpu.close()


@pytest.mark.gpu
def test_facade(engine, tmp_path):
    """8. kmerSpectrum and listKMers of the C++ facade on the paper's example (tests/cpp/kmer_spectrum_client.cpp): the
    printed statistics, histogram bins and list sums are the oracle's."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    which = NAMES.index("paper")
    K = GRAPHS[which][2]
    save_host_view(indexed(which)[0], str(tmp_path / "index.g2hv"))
    exe = compile_client(str(tmp_path / "kmer_spectrum_client"), os.path.join(ROOT, "tests", "cpp", "kmer_spectrum_client.cpp"))
    for k, ns, force, n_hist, counts, lo, hi in ((K, 0, 0, 8, 1, 2, 0), (2, 1, 0, 2, 0, 1, 1), (K + 2, 0, 1, 0, 1, 0, 0)):
        exp = expected(which, k, bool(ns))
        flags = COUNTS if counts else 0
        stats, hist = exp.stats(flags), exp.histogram(flags, n_hist)
        listed = exp.records(flags, lo, hi)
        want = ["stats " + " ".join(str(stats[f]) for f in STATS)] + [f"bin {i} {int(hist[i])}" for i in np.nonzero(hist)[0].tolist()]
        want.append(f"listed {len(listed)} {sum(r[3] for r in listed)} {sum(r[2] for r in listed)}")
        out = subprocess.run([exe, str(tmp_path / "index.g2hv")] + [str(x) for x in (k, ns, force, n_hist, counts, lo, hi)],
                             capture_output=True, text=True, env=_run_env(), timeout=300)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip().split("\n") == want, (k, ns, force)
        assert stats["kmers"] > 0
