"""Batched k-mer support (gcsa2_kmer_support_device / gcsa2_kmer_support_batch / gcsa2_seed_support_device,
kernels_support.hpp): the k-mers of every read -- or any seed records -- summed per bin of located values (value >> shift; node
ids at shift 11).  The expectations are the CPU oracle's alone: find() and count() of every materialised window
(test_kmer_windows.Expected), locate(range) once per distinct counted range, np.add.at for the array and the contract's words
(include/gcsa2_hip.h) for the stats."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from gcsa2_amd.hostview import concat_patterns
from test_mem_hits import SENTINEL
from test_extend import GRAPHS, BIG, indexed
from test_kmer_windows import reads_of, Expected, window_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
INVALID, MISSING = -1, -5
PER_BIN = 1                                             # GCSA2_SUPPORT_PER_BIN
NODE_SHIFT = 11                                         # Node::ID_OFFSET
FIELDS = ("windows", "found", "counted", "distinct", "values", "added", "dropped")
GRID_K, GRID_STRIDE, GRID_HIT_MAX, GRID_SHIFT = (1, 3, 8, 16, 33), (1, 3), (0, 1, 3, 64), (0, 11, 13)
GUARD = 64
START = 0x0101010101010101                              # what a support array holds before a call: the call adds


def nonempty_of(ranges):
    return ((ranges[:, 0] + np.uint64(1)) <= (ranges[:, 1] + np.uint64(1))) if ranges.shape[0] else np.zeros(0, dtype=bool)


class Folded:
    """The counted records of one call, folded: the distinct ranges, their summed weights and the CSR of their located values."""

    def __init__(self, records, found, counted, ranges, mult, offsets, values):
        self.records, self.found, self.counted = records, found, counted
        self.ranges, self.mult, self.offsets, self.values = ranges, mult, offsets, values
        sizes = np.diff(offsets)
        self.owner = np.repeat(np.arange(ranges.shape[0]), sizes)
        self.first = np.zeros(values.shape[0], dtype=bool)
        self.first[offsets[:-1][sizes > 0]] = True

    def tally(self, shift, per_bin, n_bins):
        """(what the call adds to a support array of n_bins, the stats)."""
        bins = self.values >> np.uint64(shift)
        keep = np.ones(bins.shape[0], dtype=bool)
        if per_bin and bins.shape[0]:
            keep[1:] = self.first[1:] | (bins[1:] != bins[:-1])         # the values of a range are sorted: equal bins are neighbours
        weight = self.mult[self.owner][keep]
        bins = bins[keep]
        inside = bins < np.uint64(n_bins)
        add = np.zeros(n_bins, dtype=np.uint64)
        np.add.at(add, bins[inside].astype(np.int64), weight[inside])
        stats = dict(windows=self.records, found=self.found, counted=self.counted, distinct=self.ranges.shape[0],
                     values=self.values.shape[0], added=int(weight[inside].sum()), dropped=int(weight[~inside].sum()))
        return add, stats


class Oracle:
    """The contract for one index, from the oracle: locate() once per distinct range, kept."""

    def __init__(self, cpu, reads=()):
        self.cpu, self.reads = cpu, list(reads)
        self.exp = Expected(cpu, self.reads)
        self.located, self.folds = {}, {}

    def locate(self, ranges):
        """The CSR of locate(range) -- sorted distinct values -- for (d, 2) ranges."""
        missing = [r for r in map(tuple, ranges.tolist()) if r not in self.located]
        if missing:
            off, val = self.cpu.locate_batch(np.asarray(missing, dtype=np.uint64), threads=2)
            for i, r in enumerate(missing):
                self.located[r] = val[int(off[i]):int(off[i + 1])].astype(np.uint64)
            for r in missing[:3]:
                direct = np.asarray(self.cpu.locate(r), dtype=np.uint64)
                assert np.array_equal(self.located[r], direct) and (np.diff(direct.astype(np.int64)) > 0).all()
        per = [self.located[r] for r in map(tuple, ranges.tolist())]
        offsets = np.concatenate([[0], np.cumsum([a.shape[0] for a in per])]).astype(np.int64)
        return offsets, np.concatenate(per + [np.zeros(0, dtype=np.uint64)]).astype(np.uint64)

    def fold(self, ranges, counts, weights, hit_max):
        """Records (m, 2) with their count()s and weights (None: 1 each) under the cap."""
        found = nonempty_of(ranges)
        counted = found & (counts > 0) & (np.ones(counts.shape[0], dtype=bool) if hit_max == 0 else counts <= np.uint64(hit_max))
        assert bool((found == (found & (counts > 0))).all())      # count() of a non-empty range of find() is at least 1
        weights = np.ones(ranges.shape[0], dtype=np.uint64) if weights is None else np.asarray(weights, dtype=np.uint64)
        if counted.any():
            distinct, inverse = np.unique(ranges[counted], axis=0, return_inverse=True)
            mult = np.zeros(distinct.shape[0], dtype=np.uint64)
            np.add.at(mult, np.asarray(inverse).reshape(-1), weights[counted])
        else:
            distinct, mult = np.zeros((0, 2), dtype=np.uint64), np.zeros(0, dtype=np.uint64)
        offsets, values = self.locate(distinct)
        return Folded(ranges.shape[0], int(found.sum()), int(counted.sum()), distinct, mult, offsets, values)

    def kmers(self, k, stride, hit_max):
        key = (k, stride, hit_max)
        if key not in self.folds:
            _, _, ranges, counts = self.exp.want(k, stride)
            self.folds[key] = self.fold(ranges, counts, None, hit_max)
        return self.folds[key]

    def seeds(self, seeds, weights, hit_max):
        """Seed records (m, 5): only sp, ep are read; count() is the oracle's."""
        ranges = np.ascontiguousarray(seeds[:, 2:4], dtype=np.uint64)
        counts = self.cpu.count_batch(ranges) if ranges.shape[0] else np.zeros(0, dtype=np.uint64)
        return self.fold(ranges, counts, weights, hit_max)


@functools.lru_cache(maxsize=None)
def oracle_of(which):
    return Oracle(indexed(which)[1], reads_of(which))


def full_bins(fold, shift):
    """A support array that holds every bin of the call: the largest bin + 1 (1 when there is none)."""
    return int(fold.values.max() >> np.uint64(shift)) + 1 if fold.values.shape[0] else 1


def every_kmer_count(k):
    """count() of every k-mer that the 6000-base graph spells (a walk from every vertex)."""
    from test_kmer_windows import COMP2CHAR
    g, cpu = GRAPHS[BIG][1], indexed(BIG)[1]
    kmers = set()

    def walk(v, s):
        s += COMP2CHAR[int(g.comp[v])]
        if len(s) == k:
            kmers.add(s)
            return
        for w in g.successors(v):
            walk(int(w), s)

    for v in range(g.size):
        walk(v, "")
    ranges = cpu.find_batch(*concat_patterns([x.encode() for x in sorted(kmers)]), threads=2)
    assert nonempty_of(ranges).all()
    return cpu.count_batch(ranges, threads=2)


# ---- CPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    return binding.load_library()


def test_library_exports_the_support_calls(lib):
    """1. The built library exports the three calls and binding.EXPORTS lists them."""
    from gcsa2_amd import binding
    for name in ("gcsa2_kmer_support_device", "gcsa2_kmer_support_batch", "gcsa2_seed_support_device"):
        assert name in binding.EXPORTS, name
        assert hasattr(ctypes.CDLL(binding.LIB_PATH), name), name
    assert binding.SUPPORT_PER_BIN == PER_BIN and binding.SUPPORT_STATS == FIELDS


def refusal_cases(index):
    """(argument the message names, keyword changes) of every refusal of the contract, for a handle `index` (any non-NULL
    pointer does for the checks in front of it)."""
    return [("index", dict(index=None)), ("k must", dict(k=0)), ("stride must", dict(stride=0)), ("shift must", dict(shift=64)),
            ("shift must", dict(shift=U64)), ("unknown flags", dict(flags=2)), ("unknown flags", dict(flags=-1)),
            ("support is NULL", dict(support=False))]


def refuse(lib, handle, form, **change):
    """One refused call on sentinel-filled host arrays (no device is touched before the refusal, so host pointers do for the
    device forms): (status, message, support and stats afterwards)."""
    arg = dict(index=handle, k=4, stride=1, shift=NODE_SHIFT, flags=0, support=True)
    arg.update(change)
    off = (ctypes.c_uint64 * 2)(0, 8)
    pat = (ctypes.c_uint8 * 8)(*b"ACGTACGT")
    seeds = (ctypes.c_uint64 * 5)(0, 4, 1, 2, 2)
    support = (ctypes.c_uint64 * 8)(*([SENTINEL] * 8))
    stats = (ctypes.c_uint64 * 7)(*([SENTINEL] * 7))
    sup = ctypes.addressof(support) if arg["support"] else None
    if form == "kmer_device":
        rc = lib.gcsa2_kmer_support_device(arg["index"], ctypes.addressof(pat), ctypes.addressof(off), 1, arg["k"], arg["stride"], 0, arg["shift"],
                                           arg["flags"], sup, 8, ctypes.addressof(stats), None)
    elif form == "kmer_batch":
        rc = lib.gcsa2_kmer_support_batch(arg["index"], pat, off, 1, arg["k"], arg["stride"], 0, arg["shift"], arg["flags"], sup, 8,
                                          ctypes.addressof(stats))
    else:
        rc = lib.gcsa2_seed_support_device(arg["index"], ctypes.addressof(seeds), 1, None, 0, arg["shift"], arg["flags"], sup, 8,
                                           ctypes.addressof(stats), None)
    return rc, lib.gcsa2_last_error().decode(), list(support), list(stats)


def test_refusals_need_no_device(lib):
    """2. Every refusal of the contract happens without a device -- the handle is a pointer to nothing that the checks never
    follow -- names its argument and leaves sentinel-filled support and stats untouched."""
    nothing = ctypes.create_string_buffer(64)
    index = ctypes.addressof(nothing)
    for form in ("kmer_device", "kmer_batch", "seed_device"):
        for names, change in refusal_cases(index):
            if form == "seed_device" and names in ("k must", "stride must"):
                continue
            rc, message, support, stats = refuse(lib, index, form, **change)
            assert rc == INVALID and names in message, (form, change, rc, message)
            assert support == [SENTINEL] * 8 and stats == [SENTINEL] * 7, (form, change)


def test_the_batches_are_not_vacuous():
    """3. On the 6000-base graph, at stride 1, the oracle shows: counted and skipped windows for k in (3, 8, 16) under the caps
    1 and 3 -- but for k = 16 under the cap 3, which no read can show on this graph (see below); a counted range with fewer distinct values than path nodes (the duplicate removal at work); distinct < counted
    (repeated k-mers); at shift 11 a range with two values in one bin, so that PER_BIN changes the result; and with n_bins at
    half of the largest bin + 1 both added > 0 and dropped > 0."""
    big = oracle_of(BIG)
    for k in (3, 8, 16):
        for hit_max in (1, 3):
            fold = big.kmers(k, 1, hit_max)
            assert 0 < fold.counted <= fold.found < fold.records, (k, hit_max, fold.counted, fold.found, fold.records)
            assert fold.ranges.shape[0] < fold.counted, (k, hit_max)
            if (k, hit_max) == (16, 3):
                # No read can show a skipped window here: of all the 16-mers the graph spells none occurs more than twice
                # (counted below, exhaustively), so the cap of 3 never bites at k = 16 on this graph.  The cap of 1 does.
                assert fold.counted == fold.found and every_kmer_count(16).max() <= 2
            else:
                assert fold.counted < fold.found, (k, hit_max, fold.counted, fold.found)
    deduplicated, per_bin_matters = [], []
    for k in (3, 8, 16):
        fold = big.kmers(k, 1, 0)
        nodes = (fold.ranges[:, 1] + np.uint64(1) - fold.ranges[:, 0]).astype(np.int64)
        if int((np.diff(fold.offsets) < nodes).sum()) > 0:
            deduplicated.append(k)
        full = full_bins(fold, NODE_SHIFT)
        plain, s_plain = fold.tally(NODE_SHIFT, False, full)
        once, s_once = fold.tally(NODE_SHIFT, True, full)
        if s_once["added"] < s_plain["added"] and not np.array_equal(plain, once):
            per_bin_matters.append(k)
        assert s_plain["added"] == int(np.diff(fold.offsets).astype(np.uint64).dot(fold.mult)) and s_plain["dropped"] == 0
        _, s_half = fold.tally(NODE_SHIFT, False, full // 2)
        assert s_half["added"] > 0 and s_half["dropped"] > 0 and s_half["added"] + s_half["dropped"] == s_plain["added"], k
    assert deduplicated and per_bin_matters, (deduplicated, per_bin_matters)


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
            self.d_pat[:self.total] = torch.from_numpy(np.array(data[:self.total], dtype=np.uint8)).to(self.dev)
        self.d_off = torch.from_numpy(np.ascontiguousarray(off).view(np.int64).copy()).to(self.dev)

    def support(self, gpu, k, stride, hit_max, shift, flags, n_bins, d_support=None):
        """gcsa2_kmer_support_device into a buffer of n_bins words of START and GUARD sentinel words behind them (or the
        caller's tensor): (stats, the whole buffer as numpy)."""
        import torch
        if d_support is None:
            d_support = fresh_support(n_bins, self.dev)
        stats = gpu.kmer_support_device(self.d_pat.data_ptr(), self.d_off.data_ptr(), self.n, k, stride, hit_max, shift, flags,
                                        d_support.data_ptr() if n_bins else 0, n_bins)
        torch.cuda.synchronize()
        return stats, d_support.cpu().numpy().view(np.uint64)


def fresh_support(n_bins, dev):
    import torch
    d = torch.full((n_bins + GUARD,), np.uint64(SENTINEL).view(np.int64).item(), dtype=torch.int64, device=dev)
    d[:n_bins] = START
    return d


def assert_support(got, want, n_bins, what, start=START):
    stats, buf = got
    add, want_stats = want
    assert stats == want_stats, (what, stats, want_stats)
    bad = np.nonzero(buf[:n_bins] != add + np.uint64(start))[0]
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), int(buf[bad[0]]) - start, int(add[bad[0]]))
    assert (buf[n_bins:] == np.uint64(SENTINEL)).all(), (what, "behind n_bins")


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_parity_with_the_oracle(engine, which):
    """4. d_support and every field of stats equal the oracle's exactly over the whole grid; the buffer starts from a non-zero
    pattern (the call adds) and the 64 sentinel words behind n_bins are unchanged."""
    oracle = oracle_of(which)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    batch = DeviceReads(reads_of(which))
    added = 0
    for k in GRID_K:
        for stride in GRID_STRIDE:
            for hit_max in GRID_HIT_MAX:
                fold = oracle.kmers(k, stride, hit_max)
                for shift in GRID_SHIFT:
                    full = full_bins(fold, shift)
                    for flags in (0, PER_BIN):
                        for n_bins in (full, full // 2):
                            what = (GRAPHS[which][0], k, stride, hit_max, shift, flags, n_bins)
                            want = fold.tally(shift, bool(flags), n_bins)
                            assert_support(batch.support(gpu, k, stride, hit_max, shift, flags, n_bins), want, n_bins, what)
                            added += want[1]["added"]
    assert added > 0
    gpu.close()


@pytest.mark.gpu
def test_accumulation_over_calls(big):
    """5. Two calls on two halves of the reads into one array equal one call on all reads, and so do windows, found, counted,
    added and dropped.  distinct and values do NOT add up: a k-mer that both halves carry is one distinct range of the whole
    batch and one of each half, so the halves' sums are larger -- ranges fold within a call only."""
    reads = reads_of(BIG)
    half = len(reads) // 2
    oracle = oracle_of(BIG)
    for k, hit_max, shift, flags in ((8, 3, NODE_SHIFT, 0), (16, 0, 0, PER_BIN)):
        fold = oracle.kmers(k, 1, hit_max)
        n_bins = full_bins(fold, shift) - 3
        want = fold.tally(shift, bool(flags), n_bins)
        d = fresh_support(n_bins, DeviceReads([]).dev)
        a, _ = DeviceReads(reads[:half]).support(big, k, 1, hit_max, shift, flags, n_bins, d_support=d)
        b, buf = DeviceReads(reads[half:]).support(big, k, 1, hit_max, shift, flags, n_bins, d_support=d)
        both = {f: a[f] + b[f] for f in FIELDS}
        for f in ("windows", "found", "counted", "added", "dropped"):
            assert both[f] == want[1][f], (k, f)
        assert both["distinct"] > want[1]["distinct"] and both["values"] > want[1]["values"], k
        for part, some in ((a, reads[:half]), (b, reads[half:])):
            assert part == Oracle(oracle.cpu, some).kmers(k, 1, hit_max).tally(shift, bool(flags), n_bins)[1], k
        assert_support((want[1], buf), want, n_bins, (k, "two halves"))


def client_lines(add, stats):
    return ["stats " + " ".join(str(stats[f]) for f in FIELDS)] + [f"bin {i} {int(add[i]) + 5}" for i in np.nonzero(add)[0].tolist()]


@pytest.fixture(scope="module")
def client(engine, tmp_path_factory):
    """tests/cpp/kmer_support_client.cpp, the 6000-base index as a host-view file and its reads, one per line."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client
    tmp = tmp_path_factory.mktemp("kmer_support")
    reads = reads_of(BIG)
    assert all(b"\n" not in r for r in reads)
    save_host_view(indexed(BIG)[0], str(tmp / "index.g2hv"))
    (tmp / "reads.txt").write_bytes(b"".join(r + b"\n" for r in reads))
    exe = compile_client(str(tmp / "kmer_support_client"), os.path.join(ROOT, "tests", "cpp", "kmer_support_client.cpp"))

    def run(k, stride, hit_max, shift, per_bin, n_bins, **env):
        from test_facade import _run_env
        full = _run_env()
        full.pop("GCSA2_SUPPORT_CHUNK", None)
        full.update(env)
        out = subprocess.run([exe, str(tmp / "index.g2hv"), str(tmp / "reads.txt")] + [str(int(x)) for x in (k, stride, hit_max, shift, per_bin, n_bins)],
                             capture_output=True, text=True, env=full, timeout=300)
        assert out.returncode == 0, out.stderr
        return out.stdout.strip().split("\n")
    return run


@pytest.mark.gpu
def test_chunking_changes_nothing(client):
    """6. The 6000-base batch with GCSA2_SUPPORT_CHUNK at 1, 64 and the default, each in a fresh process (the facade's client):
    identical support and stats, the oracle's.  Both small budgets are below the count() of some range -- the largest exceeds
    64 -- which is the 'at least one range' rule; 64 also makes chunks of several small ranges."""
    oracle = oracle_of(BIG)
    k, hit_max = 3, 0
    fold = oracle.kmers(k, 1, hit_max)
    counts = oracle.cpu.count_batch(fold.ranges)
    assert int(counts.max()) > 64 and int(np.sort(counts)[:2].sum()) <= 64 and fold.ranges.shape[0] > 8
    n_bins = full_bins(fold, NODE_SHIFT) - 1
    want = client_lines(*fold.tally(NODE_SHIFT, False, n_bins))
    for env in (dict(GCSA2_SUPPORT_CHUNK="1"), dict(GCSA2_SUPPORT_CHUNK="64"), dict()):
        assert client(k, 1, hit_max, NODE_SHIFT, 0, n_bins, **env) == want, env


@pytest.mark.gpu
def test_edges(engine, big, monkeypatch):
    """7. Reads shorter than k, no reads, nothing found, n_bins == 0, one read of 1000 windows of one repeated k-mer, exactly
    64, 65 and 128 found windows, and an image without pair blocks."""
    cpu = indexed(BIG)[1]
    zero = dict.fromkeys(FIELDS, 0)
    # reads shorter than k; no reads; nothing found
    for some, k in (([b"ACGT", b"", b"ACGTACG", b"A"], 8), ([], 16), ([b"NNNN", b"XYZ", b"NNNN", b""], 2)):
        stats, buf = DeviceReads(some).support(big, k, 1, 3, NODE_SHIFT, 0, 16)
        assert stats == dict(zero, windows=sum(window_count(len(r), k, 1) for r in some)), (some, k)
        assert (buf[:16] == np.uint64(START)).all() and (buf[16:] == np.uint64(SENTINEL)).all(), (some, k)
    # n_bins == 0: a statistics run, with a NULL array
    oracle = oracle_of(BIG)
    fold = oracle.kmers(8, 1, 3)
    stats, buf = DeviceReads(reads_of(BIG)).support(big, 8, 1, 3, NODE_SHIFT, 0, 0)
    want = fold.tally(NODE_SHIFT, False, 0)
    assert stats == want[1] and stats["added"] == 0 and stats["dropped"] > 0 and (buf == np.uint64(SENTINEL)).all()
    # one k-mer 1000 times in one read: a homopolymer, or a tandem repeat of two bases, that the graph holds
    k = 4
    units = [u for u in (b"A", b"C", b"G", b"T", b"AC", b"AG", b"AT", b"CA", b"CT", b"GA", b"GT", b"TA", b"TC", b"TG", b"CG", b"GC")
             if nonempty_of(np.asarray([cpu.find((u * k)[:k])], dtype=np.uint64))[0]]
    assert units
    unit = units[0]
    stride = len(unit)
    read = (unit * (k + 1000 * stride))[:k + 999 * stride]
    assert window_count(len(read), k, stride) == 1000 and len({read[j:j + k] for j in range(0, 1000 * stride, stride)}) == 1
    fold = Oracle(cpu, [read]).kmers(k, stride, 0)
    assert fold.counted == 1000 and fold.ranges.shape[0] == 1 and int(fold.mult[0]) == 1000
    n_bins = full_bins(fold, NODE_SHIFT)
    assert_support(DeviceReads([read]).support(big, k, stride, 0, NODE_SHIFT, 0, n_bins), fold.tally(NODE_SHIFT, False, n_bins), n_bins, "1000 windows")
    # exactly 64, 65 and 128 found windows (and five that are not): the wavefront and workgroup edges of the search and of the
    # run kernel
    k = 16
    walk = reads_of(BIG)[0]
    assert len(walk) >= k + 31
    for found in (64, 65, 128):
        some = [b"N" * (k + 4)] + [walk[:k + 31]] * (found // 32) + ([walk[:k + found % 32 - 1]] if found % 32 else [])
        fold = Oracle(cpu, some).kmers(k, 1, 0)
        assert fold.found == found and fold.counted == found and fold.records == found + 5, (found, fold.found, fold.records)
        n_bins = full_bins(fold, 0)
        assert_support(DeviceReads(some).support(big, k, 1, 0, 0, PER_BIN, n_bins), fold.tally(0, True, n_bins), n_bins, ("found", found))
    # an image without pair blocks
    monkeypatch.setenv("GCSA2_PAIR_BLOCKS", "0")
    plain = engine.GCSA(indexed(BIG)[0])
    monkeypatch.delenv("GCSA2_PAIR_BLOCKS")
    assert plain.pair_block_bytes() == 0 and big.pair_block_bytes() > 0
    batch = DeviceReads(reads_of(BIG))
    for k, hit_max in ((8, 3), (33, 0)):
        fold = oracle.kmers(k, 1, hit_max)
        n_bins = full_bins(fold, NODE_SHIFT)
        assert_support(batch.support(plain, k, 1, hit_max, NODE_SHIFT, 0, n_bins), fold.tally(NODE_SHIFT, False, n_bins), n_bins, ("no pair blocks", k))
    plain.close()
    # a find-only image is refused, with nothing written
    find_only = engine.GCSA(indexed(BIG)[0], with_samples=False, with_counters=False, with_lcp=False)
    with pytest.raises(engine.Gcsa2Error) as err:
        batch.support(find_only, 8, 1, 0, NODE_SHIFT, 0, 16)
    assert err.value.code == MISSING
    find_only.close()


def seed_support(gpu, seeds, weights, hit_max, shift, flags, n_bins):
    """gcsa2_seed_support_device on records and weights copied to the device: (stats, the whole buffer)."""
    import torch
    dev = torch.device("cuda", 0)
    d_seeds = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_weights = None if weights is None else torch.from_numpy(np.ascontiguousarray(weights, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_support = fresh_support(n_bins, dev)
    stats = gpu.seed_support_device(d_seeds.data_ptr() if seeds.shape[0] else 0, seeds.shape[0], 0 if d_weights is None else d_weights.data_ptr(),
                                    hit_max, shift, flags, d_support.data_ptr(), n_bins)
    torch.cuda.synchronize()
    return stats, d_support.cpu().numpy().view(np.uint64)


def device_records(gpu, batch, call, sized, *args):
    """The seed records of a *_device call (`call`, whose host form `sized` gives the sizes), as they lie in device memory."""
    import torch
    m, h = sized[1].shape[0], sized[3].shape[0]
    d_soff = torch.zeros(batch.n + 1, dtype=torch.int64, device=batch.dev)
    d_seeds = torch.zeros((m, 5), dtype=torch.int64, device=batch.dev)
    d_hoff = torch.zeros(m + 1, dtype=torch.int64, device=batch.dev)
    d_hits = torch.zeros(max(h, 1), dtype=torch.int64, device=batch.dev)
    assert call(d_soff, d_seeds, d_hoff, d_hits, m, h) == (m, h)
    torch.cuda.synchronize()
    got = d_seeds.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, sized[1])
    return got


@pytest.mark.gpu
def test_seed_form(big):
    """8. The records of kmer_hits_device, mem_hits_device and capped_seeds_device on the same reads, fed to
    gcsa2_seed_support_device, give the oracle's sum over those records; the k-mer seeds with NULL weights give the array of the
    k-mer form; weights 0, 1, 7 scale as defined; a garbage count field changes nothing; records with an empty range of either
    form are ignored."""
    reads = reads_of(BIG)
    oracle = oracle_of(BIG)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    p, o = batch.d_pat.data_ptr(), batch.d_off.data_ptr()
    kmer = device_records(big, batch, lambda so, se, ho, hi, m, h: big.kmer_hits_device(p, o, batch.n, 8, 1, 3, 0, 0, so.data_ptr(), se.data_ptr(), m,
                                                                                        ho.data_ptr(), hi.data_ptr(), h),
                          big.kmer_hits_batch(flat, off, 8, 1, 3, False))
    mems = device_records(big, batch, lambda so, se, ho, hi, m, h: big.mem_hits_device(p, o, batch.n, None, 6, 3, 0, so.data_ptr(), se.data_ptr(), m,
                                                                                       ho.data_ptr(), hi.data_ptr(), h),
                          big.mem_hits_batch(flat, off, 6, 3, False))
    capped = device_records(big, batch, lambda so, se, ho, hi, m, h: big.capped_seeds_device(p, o, batch.n, 4, 0, 3, 0, 0, so.data_ptr(), se.data_ptr(), m,
                                                                                             ho.data_ptr(), hi.data_ptr(), h),
                            big.capped_seeds_batch(flat, off, 4, 0, 3, 0, False))
    for name, seeds in (("kmer", kmer), ("mem", mems), ("capped", capped)):
        assert seeds.shape[0] > 64, name
        for hit_max, shift, flags in ((3, NODE_SHIFT, 0), (0, 0, PER_BIN), (1, 13, PER_BIN)):
            fold = oracle.seeds(seeds, None, hit_max)
            n_bins = full_bins(fold, shift) - 1
            assert fold.counted > 0
            assert_support(seed_support(big, seeds, None, hit_max, shift, flags, n_bins), fold.tally(shift, bool(flags), n_bins), n_bins,
                           (name, hit_max, shift, flags))
    # the k-mer seeds are the found windows: the same array and stats as the k-mer form, but for `windows`
    fold = oracle.kmers(8, 1, 3)
    n_bins = full_bins(fold, NODE_SHIFT)
    add, stats = fold.tally(NODE_SHIFT, False, n_bins)
    got = seed_support(big, kmer, None, 3, NODE_SHIFT, 0, n_bins)
    assert_support(got, (add, dict(stats, windows=kmer.shape[0])), n_bins, "k-mer seeds")
    assert kmer.shape[0] == stats["found"]
    assert_support(batch.support(big, 8, 1, 3, NODE_SHIFT, 0, n_bins), (add, stats), n_bins, "k-mer form")
    # weights; a garbage count field; empty records of both forms in between
    weights = np.asarray([(0, 1, 7)[i % 3] for i in range(mems.shape[0])], dtype=np.uint64)
    fold = oracle.seeds(mems, weights, 3)
    plain = oracle.seeds(mems, None, 3)
    n_bins = full_bins(fold, NODE_SHIFT)
    want = fold.tally(NODE_SHIFT, False, n_bins)
    assert 0 < want[1]["added"] != plain.tally(NODE_SHIFT, False, n_bins)[1]["added"] and want[1]["counted"] == plain.counted
    assert_support(seed_support(big, mems, weights, 3, NODE_SHIFT, 0, n_bins), want, n_bins, "weights")
    garbage = mems.copy()
    garbage[:, 4] = np.uint64(SENTINEL)
    garbage[::2, 4] = 0
    assert_support(seed_support(big, garbage, weights, 3, NODE_SHIFT, 0, n_bins), want, n_bins, "garbage counts")
    n = indexed(BIG)[1].n
    empties = np.asarray([[0, 5, 1, 0, 9], [0, 5, n + 3, n + 2, 1], [0, 0, 0, U64, 0], [3, 3, 7, 6, 1]], dtype=np.uint64)
    assert not nonempty_of(empties[:, 2:4]).any()
    mixed = np.concatenate([empties[:2], mems[:70], empties[2:], mems[70:], empties])
    mixed_weights = np.concatenate([[5, 5], weights[:70], [5, 5], weights[70:], [5, 5, 5, 5]]).astype(np.uint64)
    assert_support(seed_support(big, mixed, mixed_weights, 3, NODE_SHIFT, 0, n_bins),
                   (want[0], dict(want[1], windows=mixed.shape[0])), n_bins, "empty records")
    only = seed_support(big, empties, None, 0, NODE_SHIFT, 0, 8)
    assert only[0] == dict(dict.fromkeys(FIELDS, 0), windows=4) and (only[1][:8] == np.uint64(START)).all()
    none = seed_support(big, np.zeros((0, 5), dtype=np.uint64), None, 0, NODE_SHIFT, 0, 8)
    assert none[0] == dict.fromkeys(FIELDS, 0) and (none[1][:8] == np.uint64(START)).all()


@pytest.mark.gpu
def test_host_form(engine, big, client, monkeypatch):
    """9. gcsa2_kmer_support_batch equals the device form in one piece; with GCSA2_MS_PIECE_MB forcing several pieces distinct
    (and values) are at least the one-piece figures and everything else is equal; the facade and GCSA.kmer_support_batch
    agree with it."""
    oracle = oracle_of(BIG)
    once = reads_of(BIG)
    flat, off = concat_patterns(once)
    for k, stride, hit_max, shift, per_bin in ((8, 1, 3, NODE_SHIFT, False), (16, 3, 0, 0, True)):
        fold = oracle.kmers(k, stride, hit_max)
        n_bins = full_bins(fold, shift) - 2
        add, stats = fold.tally(shift, per_bin, n_bins)
        support, got = big.kmer_support_batch(flat, off, k, stride, hit_max, shift, n_bins=n_bins, per_bin=per_bin)
        assert got == stats and np.array_equal(support, add), (k, "fresh array")
        mine = np.full(n_bins, START, dtype=np.uint64)
        support, got = big.kmer_support_batch(flat, off, k, stride, hit_max, shift, per_bin=per_bin, support=mine)
        assert support is mine and got == stats and np.array_equal(mine, add + np.uint64(START)), (k, "adds")
        assert client(k, stride, hit_max, shift, per_bin, n_bins) == client_lines(add, stats), (k, "facade")
    with pytest.raises(ValueError):
        big.kmer_support_batch(flat, off, 8)
    # several pieces: the batch repeated until it is 3 MB of reads, in 1 MB pieces, against the same batch in one piece
    monkeypatch.setenv("GCSA2_MS_PIECE_MB", "1")
    pieced, _ = engine.open_index(indexed(BIG)[0], device=0)
    monkeypatch.delenv("GCSA2_MS_PIECE_MB")
    repeats = (3 << 20) // sum(len(r) for r in once) + 1
    flat, off = concat_patterns(once * repeats)
    assert int(off[-1]) >= 3 << 20
    fold = oracle.kmers(16, 1, 3)
    n_bins = full_bins(fold, NODE_SHIFT) - 2
    add, stats = fold.tally(NODE_SHIFT, False, n_bins)
    whole_support, whole = big.kmer_support_batch(flat, off, 16, 1, 3, NODE_SHIFT, n_bins=n_bins)
    piece_support, piece = pieced.kmer_support_batch(flat, off, 16, 1, 3, NODE_SHIFT, n_bins=n_bins)
    assert np.array_equal(whole_support, add * np.uint64(repeats)) and np.array_equal(piece_support, whole_support)
    assert whole == dict({f: stats[f] * repeats for f in FIELDS}, distinct=stats["distinct"], values=stats["values"])
    assert piece["distinct"] > whole["distinct"] and piece["values"] > whole["values"]
    assert {f: piece[f] for f in FIELDS if f not in ("distinct", "values")} == {f: whole[f] for f in FIELDS if f not in ("distinct", "values")}
    pieced.close()
