"""Batched k-mer classes (gcsa2_kmer_classes_device / gcsa2_kmer_classes_batch / gcsa2_seed_classes_device,
kernels_classes.hpp): per read -- or group of seed records -- the votes of its counted records over classes of bins of located
values.  The expectations are the CPU oracle's alone: find() and count() of every materialised window
(test_kmer_windows.Expected), locate(range) once per distinct counted range (test_kmer_support.Oracle) and `restate`, the
DEFINITION of include/gcsa2_hip.h in numpy.  Every comparison is exact.

The parity grid: (k, stride, hit_max, shift) -- what decides the fold and the located values -- is the full product of the
contract's lists on every graph; each of its 80 points runs 8 of the 80 combinations of (flags, n_classes, map), taken in turn
so that over a graph every combination runs 8 times, with different points.  (The full product of all seven lists would be
6400 calls on each of 11 graphs.)"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from gcsa2_amd.hostview import concat_patterns
from test_mem_hits import SENTINEL
from test_extend import GRAPHS, BIG, indexed
from test_kmer_windows import reads_of, window_count
from test_kmer_support import Oracle, oracle_of, nonempty_of, DeviceReads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
UNKNOWN = U64
INVALID, MISSING = -1, -5
NONE = 0xFFFFFFFF                                       # GCSA2_CLASS_NONE
LIMIT = 4096                                            # GCSA2_CLASS_LIMIT
PER_WINDOW, UNAMBIGUOUS = 1, 2
NODE_SHIFT = 11
FIELDS = ("windows", "found", "counted", "distinct", "values", "votes", "unclassified", "ambiguous")
CALL = ("best", "best_votes", "second", "second_votes", "total", "counted")
GRID_K, GRID_STRIDE, GRID_HIT_MAX, GRID_SHIFT = (1, 3, 8, 16, 33), (1, 3), (0, 1, 3, 64), (0, 11)
GRID_FLAGS, GRID_CLASSES = (0, PER_WINDOW, UNAMBIGUOUS, PER_WINDOW | UNAMBIGUOUS), (1, 5, 64, 4096)
MAPS = ("interleaved", "blocked", "holes", "beyond", "short")
GUARD = 64


def class_map(kind, n_bins, n_classes):
    """The maps of the contract's test list over n_bins bins (n_bins = the largest bin + 1), made once and left unchanged."""
    out = make_class_map(kind, int(n_bins), int(n_classes))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=64)
def make_class_map(kind, n_bins, n_classes):
    bins = np.arange(n_bins, dtype=np.uint64)
    if kind == "interleaved":
        return (bins % np.uint64(n_classes)).astype(np.uint32)
    if kind == "blocked":
        return (bins * np.uint64(n_classes) // np.uint64(max(n_bins, 1))).astype(np.uint32)
    if kind == "holes":                                  # interleaved, bin % 7 == 3 -> no class
        out = (bins % np.uint64(n_classes)).astype(np.uint32)
        out[bins % np.uint64(7) == 3] = NONE
        return out
    if kind == "beyond":                                 # interleaved over n_classes + 3 ids: some are >= n_classes
        return (bins % np.uint64(n_classes + 3)).astype(np.uint32)
    if kind == "short":                                  # shorter than the largest bin
        return (bins[:n_bins // 2] % np.uint64(n_classes)).astype(np.uint32)
    if kind == "one":
        return np.zeros(n_bins, dtype=np.uint32)
    raise ValueError(kind)


class Records:
    """Seed records of one call, folded under the cap: per record its run (distinct range) or -1, the runs' located values."""

    def __init__(self, oracle, ranges, counts, hit_max, windows=None):
        self.m = ranges.shape[0]
        self.windows = self.m if windows is None else windows
        found = nonempty_of(ranges)
        counted = found & (counts > 0) & (np.ones(self.m, dtype=bool) if hit_max == 0 else counts <= np.uint64(hit_max))
        self.found, self.counted = int(found.sum()), int(counted.sum())
        self.run_of = np.full(self.m, -1, dtype=np.int64)
        if counted.any():
            self.ranges, inverse = np.unique(ranges[counted], axis=0, return_inverse=True)
            self.run_of[counted] = np.asarray(inverse).reshape(-1)
        else:
            self.ranges = np.zeros((0, 2), dtype=np.uint64)
        self.offsets, self.values = oracle.locate(self.ranges)
        self.owner = np.repeat(np.arange(self.ranges.shape[0]), np.diff(self.offsets))

    def largest_bin(self, shift):
        return int(self.values.max() >> np.uint64(shift)) if self.values.shape[0] else 0

    def signatures(self, shift, cmap, n_classes):
        """Per run: (entry offsets, entry classes, entry n_c) of the classes with n_c > 0, none(R), classes(R), and the class
        of every value in value order (n_classes = no class)."""
        d, C = self.ranges.shape[0], n_classes
        bins = self.values >> np.uint64(shift)
        inside = bins < np.uint64(cmap.shape[0])
        ids = np.full(bins.shape[0], NONE, dtype=np.uint64)
        ids[inside] = cmap[bins[inside].astype(np.int64)]
        cls = np.where(ids < np.uint64(C), ids, np.uint64(C)).astype(np.int64)
        uniq, n = np.unique(self.owner * (C + 1) + cls, return_counts=True)
        e_run, e_cls = uniq // (C + 1), uniq % (C + 1)
        real = e_cls < C
        none_of = np.zeros(d, dtype=np.uint64)
        none_of[e_run[~real]] = n[~real].astype(np.uint64)
        classes_of = np.bincount(e_run[real], minlength=d).astype(np.int64)
        e_off = np.concatenate([[0], np.cumsum(classes_of)]).astype(np.int64)
        return e_off, e_cls[real], n[real].astype(np.uint64), none_of, classes_of, cls


def restate(rec, owner, index, n_groups, weights, shift, cmap, n_classes, flags):
    """The DEFINITION: (votes (n_groups, n_classes), calls (n_groups, 6), stats).  Group owner[i] owns record index[i] (a record
    may be owned more than once, or not at all); weights per record or None."""
    C = n_classes
    e_off, e_cls, e_n, none_of, classes_of, _ = rec.signatures(shift, cmap, C)
    weights = np.ones(rec.m, dtype=np.uint64) if weights is None else np.asarray(weights, dtype=np.uint64)
    keep = rec.run_of[index] >= 0
    g, r, w = owner[keep].astype(np.int64), rec.run_of[index[keep]], weights[index[keep]]
    counted_of = np.bincount(g, minlength=n_groups).astype(np.uint64)
    stats = dict(windows=rec.windows, found=rec.found, counted=rec.counted, distinct=rec.ranges.shape[0], values=rec.values.shape[0],
                 unclassified=int(none_of[r].sum()), ambiguous=int((classes_of[r] >= 2).sum()))
    if flags & UNAMBIGUOUS:
        ok = classes_of[r] == 1
        g, r, w = g[ok], r[ok], w[ok]
    votes = np.zeros(n_groups * C, dtype=np.uint64)
    d = max(rec.ranges.shape[0], 1)
    if g.shape[0]:
        # the records of a group on one run first (their weights add), then every (group, run) pair times the run's entries
        pair = g * d + r
        order = np.argsort(pair, kind="stable")
        pair, w = pair[order], w[order]
        starts = np.nonzero(np.concatenate([[True], pair[1:] != pair[:-1]]))[0]
        pw = np.add.reduceat(w, starts)
        pg, pr = pair[starts] // d, pair[starts] % d
        cnt = classes_of[pr]
        rep = np.repeat(np.arange(pr.shape[0]), cnt)
        within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        e = e_off[pr][rep] + within
        x = pw[rep] if flags & PER_WINDOW else pw[rep] * e_n[e]
        flat = pg[rep] * C + e_cls[e]
        order = np.argsort(flat, kind="stable")
        flat, x = flat[order], x[order]
        if flat.shape[0]:
            starts = np.nonzero(np.concatenate([[True], flat[1:] != flat[:-1]]))[0]
            votes[flat[starts]] = np.add.reduceat(x, starts)
    votes = votes.reshape(n_groups, C)
    rows = np.arange(n_groups)
    calls = np.zeros((n_groups, 6), dtype=np.uint64)
    if n_groups:
        best = votes.argmax(axis=1)                       # the first of the largest: the lowest id on a tie
        best_votes = votes[rows, best]
        rest = votes.copy()
        rest[rows, best] = 0
        second = rest.argmax(axis=1)
        second_votes = rest[rows, second]
        calls[:, 0] = np.where(best_votes > 0, best.astype(np.uint64), np.uint64(UNKNOWN))
        calls[:, 1] = best_votes
        calls[:, 2] = np.where(second_votes > 0, second.astype(np.uint64), np.uint64(UNKNOWN))
        calls[:, 3] = second_votes
        calls[:, 4] = votes.sum(axis=1, dtype=np.uint64)
        calls[:, 5] = counted_of
    stats["votes"] = int(calls[:, 4].sum(dtype=np.uint64))
    return votes, calls, {f: stats[f] for f in FIELDS}


class Kmers:
    """The k-mer form for one oracle (test_kmer_support.Oracle): the folded records of (k, stride, hit_max), kept."""

    def __init__(self, oracle):
        self.oracle, self.kept = oracle, {}

    def records(self, k, stride, hit_max):
        key = (k, stride, hit_max)
        if key not in self.kept:
            woff, _, ranges, counts = self.oracle.exp.want(k, stride)
            rec = Records(self.oracle, ranges, counts, hit_max)
            owner = np.repeat(np.arange(len(self.oracle.reads)), np.diff(woff.astype(np.int64)))
            self.kept[key] = (rec, owner)
        return self.kept[key]

    def want(self, k, stride, hit_max, shift, cmap, n_classes, flags):
        rec, owner = self.records(k, stride, hit_max)
        return restate(rec, owner, np.arange(rec.m), len(self.oracle.reads), None, shift, cmap, n_classes, flags)


@functools.lru_cache(maxsize=None)
def kmers_of(which):
    return Kmers(oracle_of(which))


@functools.lru_cache(maxsize=None)
def bins_of(which, shift):
    """The largest bin of any value of the graph's index + 1: one map size per graph and shift, so that the maps are made once."""
    cpu = indexed(which)[1]
    return (int(np.asarray(cpu.locate((0, cpu.n - 1)), dtype=np.uint64).max()) >> shift) + 1


def grid_points():
    return [(k, stride, hit_max, shift) for k in GRID_K for stride in GRID_STRIDE for hit_max in GRID_HIT_MAX for shift in GRID_SHIFT]


def grid_combinations(point):
    """The 8 of the 80 (flags, n_classes, map) that grid point number `point` runs: 21 is coprime to 80, so the 640 calls of a
    graph visit every combination 8 times, and the 8 of one point hold every flag combination twice."""
    out = []
    for i in range(8):
        j = (21 * (8 * point + i)) % 80
        out.append((GRID_FLAGS[j % 4], GRID_CLASSES[(j // 4) % 4], MAPS[j // 16]))
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    return binding.load_library()


def test_library_exports_the_classes_calls(lib):
    """1. The header declares the three calls, the built library exports them and binding.EXPORTS lists them."""
    from gcsa2_amd import binding
    header = open(os.path.join(ROOT, "include", "gcsa2_hip.h")).read()
    for name in ("gcsa2_kmer_classes_device", "gcsa2_kmer_classes_batch", "gcsa2_seed_classes_device"):
        assert ("int " + name + "(") in header, name
        assert name in binding.EXPORTS, name
        assert hasattr(ctypes.CDLL(binding.LIB_PATH), name), name
    assert (binding.CLASS_NONE, binding.CLASS_LIMIT, binding.CLASS_PER_WINDOW, binding.CLASS_UNAMBIGUOUS) == (NONE, LIMIT, PER_WINDOW, UNAMBIGUOUS)
    assert binding.CLASS_STATS == FIELDS and binding.CLASS_CALL == CALL
    for text in ("#define GCSA2_CLASS_NONE        0xFFFFFFFFu", "#define GCSA2_CLASS_LIMIT       4096", "#define GCSA2_CLASS_PER_WINDOW  1",
                 "#define GCSA2_CLASS_UNAMBIGUOUS 2"):
        assert text in header, text


def test_the_grid_covers_every_combination():
    points = grid_points()
    assert len(points) == 80
    seen = {}
    for p in range(len(points)):
        combos = grid_combinations(p)
        assert sorted(c[0] for c in combos) == sorted(GRID_FLAGS * 2)
        for c in combos:
            seen[c] = seen.get(c, 0) + 1
    assert len(seen) == 80 and set(seen.values()) == {8}


def refusal_cases(index):
    """(what the message names, keyword changes) of every refusal of the contract in front of the device."""
    return [("index", dict(index=None)), ("k must", dict(k=0)), ("stride must", dict(stride=0)), ("shift must", dict(shift=64)),
            ("shift must", dict(shift=U64)), ("unknown flags", dict(flags=4)), ("unknown flags", dict(flags=-1)), ("unknown flags", dict(flags=8 | 1)),
            ("n_classes must", dict(n_classes=0)), ("n_classes must", dict(n_classes=LIMIT + 1)), ("n_classes must", dict(n_classes=U64)),
            ("is NULL with n_bins", dict(cmap=False))]


def refuse(lib, form, **change):
    """One refused call on sentinel-filled host arrays (no device is touched before the refusal, so host pointers do for the
    device forms): (status, message, votes, calls and stats afterwards)."""
    arg = dict(index=None, k=4, stride=1, shift=NODE_SHIFT, flags=0, n_classes=2, cmap=True)
    arg.update(change)
    off = (ctypes.c_uint64 * 2)(0, 8)
    pat = (ctypes.c_uint8 * 8)(*b"ACGTACGT")
    seeds = (ctypes.c_uint64 * 5)(0, 4, 1, 2, 2)
    cmap = (ctypes.c_uint32 * 8)(0, 1, 0, 1, 0, 1, 0, 1)
    votes = (ctypes.c_uint64 * 16)(*([SENTINEL] * 16))
    calls = (ctypes.c_uint64 * 12)(*([SENTINEL] * 12))
    stats = (ctypes.c_uint64 * 8)(*([SENTINEL] * 8))
    pm = ctypes.addressof(cmap) if arg["cmap"] else None
    pv, pc, ps = ctypes.addressof(votes), ctypes.addressof(calls), ctypes.addressof(stats)
    if form == "kmer_device":
        rc = lib.gcsa2_kmer_classes_device(arg["index"], ctypes.addressof(pat), ctypes.addressof(off), 1, arg["k"], arg["stride"], 0, arg["shift"],
                                           arg["flags"], pm, 8, arg["n_classes"], pv, pc, ps, None)
    elif form == "kmer_batch":
        rc = lib.gcsa2_kmer_classes_batch(arg["index"], pat, off, 1, arg["k"], arg["stride"], 0, arg["shift"], arg["flags"], pm, 8, arg["n_classes"],
                                          pv, pc, ps)
    else:
        rc = lib.gcsa2_seed_classes_device(arg["index"], ctypes.addressof(off), 1, ctypes.addressof(seeds), 1, None, 0, arg["shift"], arg["flags"],
                                           pm, 8, arg["n_classes"], pv, pc, ps, None)
    return rc, lib.gcsa2_last_error().decode(), list(votes), list(calls), list(stats)


def test_refusals_need_no_device(lib):
    """10. Every INVALID_ARGUMENT of the contract happens without a device -- the handle is a pointer to nothing that the checks
    never follow -- names its argument and leaves sentinel-filled votes, calls and stats untouched; n_classes = 4097 among them."""
    nothing = ctypes.create_string_buffer(64)
    index = ctypes.addressof(nothing)
    for form in ("kmer_device", "kmer_batch", "seed_device"):
        for names, change in refusal_cases(index):
            if form == "seed_device" and names in ("k must", "stride must"):
                continue
            rc, message, votes, calls, stats = refuse(lib, form, **dict(dict(index=index), **change))
            assert rc == INVALID and names in message, (form, change, rc, message)
            assert votes == [SENTINEL] * 16 and calls == [SENTINEL] * 12 and stats == [SENTINEL] * 8, (form, change)


def class_sequences(rec, shift, cmap, n_classes):
    """Per run the classes of its values in value order (n_classes = no class)."""
    cls = rec.signatures(shift, cmap, n_classes)[5]
    return [cls[int(a):int(b)] for a, b in zip(rec.offsets[:-1], rec.offsets[1:])]


def returns_to_a_class(seq):
    """A, B, A: some class comes again after another one."""
    change = np.nonzero(np.diff(seq) != 0)[0]
    heads = np.concatenate([seq[:1], seq[change + 1]])
    return len(set(heads.tolist())) < heads.shape[0]


def test_the_batches_are_not_vacuous():
    """3. On the 6000-base graph at hit_max = 0, shift = 11, n_classes = 5, from the oracle alone: under the interleaved map
    ranges whose classes in value order come back to a class after another one (64 of 68 ranges at k = 3, 9 at k = 8) and
    ranges with classes(R) >= 2 (64 and 481); under the map with holes unclassified values (1073 and 598) and counted ranges
    all of whose values are unclassified (2 and 454).  The grid holds a read with a tie for best, a read with exactly one
    voted class and a read with total == 0 but counted > 0."""
    kmers = kmers_of(BIG)
    figures = {}
    for k in (3, 8):
        rec, _ = kmers.records(k, 1, 0)
        n_bins = rec.largest_bin(NODE_SHIFT) + 1
        inter, holes = class_map("interleaved", n_bins, 5), class_map("holes", n_bins, 5)
        back = sum(returns_to_a_class(s) for s in class_sequences(rec, NODE_SHIFT, inter, 5))
        _, _, _, none_of, classes_of, _ = rec.signatures(NODE_SHIFT, inter, 5)
        assert int(none_of.sum()) == 0
        several = int((classes_of >= 2).sum())
        _, _, _, none_of, classes_of, _ = rec.signatures(NODE_SHIFT, holes, 5)
        figures[k] = (rec.ranges.shape[0], back, several, int(none_of.sum()), int(((classes_of == 0) & (none_of > 0)).sum()))
    print(figures)
    assert figures[3] == (68, 64, 64, 1073, 2), figures
    assert figures[8][1:] == (9, 481, 598, 454), figures
    # ties, single-class reads, reads whose counted records all fall into no class
    tie = single = silent = 0
    for k, hit_max, kind, C in ((8, 3, "interleaved", 5), (16, 0, "blocked", 5), (8, 0, "holes", 64), (16, 0, "holes", 5)):
        rec, _ = kmers.records(k, 1, hit_max)
        cmap = class_map(kind, rec.largest_bin(NODE_SHIFT) + 1, C)
        votes, calls, _ = kmers.want(k, 1, hit_max, NODE_SHIFT, cmap, C, 0)
        tie += int(((votes == calls[:, 1:2]).sum(axis=1)[calls[:, 1] > 0] >= 2).sum())
        single += int(((calls[:, 0] != np.uint64(UNKNOWN)) & (calls[:, 2] == np.uint64(UNKNOWN))).sum())
        silent += int(((calls[:, 4] == 0) & (calls[:, 5] > 0)).sum())
    print(tie, single, silent)
    assert tie > 0 and single > 0 and silent > 0, (tie, single, silent)


def test_restate_on_a_hand_made_case():
    """The restatement itself on values written down by hand: two runs, a map under which run 0 goes A, B, A."""
    class Fixed(Oracle):
        def __init__(self):
            self.table = {(1, 2): [0 << 11, 1 << 11, 2 << 11, (2 << 11) + 5], (4, 4): [3 << 11], (7, 9): [9 << 11]}

        def locate(self, ranges):
            per = [np.asarray(self.table[tuple(r)], dtype=np.uint64) for r in ranges.tolist()]
            return np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64), np.concatenate(per + [np.zeros(0, dtype=np.uint64)]).astype(np.uint64)

    ranges = np.asarray([[1, 2], [4, 4], [1, 2], [5, 4], [7, 9], [4, 4]], dtype=np.uint64)
    counts = np.asarray([4, 1, 4, 0, 1, 1], dtype=np.uint64)
    rec = Records(Fixed(), ranges, counts, 0)
    cmap = np.asarray([0, 1, 0, NONE], dtype=np.uint32)            # bins 0, 2 -> class 0; 1 -> class 1; 3 none; 9 beyond the map
    owner, index = np.asarray([0, 0, 1, 1, 1, 2]), np.arange(6)
    votes, calls, stats = restate(rec, owner, index, 4, np.asarray([1, 1, 2, 9, 1, 1 << 40], dtype=np.uint64), NODE_SHIFT, cmap, 2, 0)
    assert votes.tolist() == [[3, 1], [6, 2], [0, 0], [0, 0]]
    assert calls.tolist() == [[0, 3, 1, 1, 4, 2], [0, 6, 1, 2, 8, 2], [UNKNOWN, 0, UNKNOWN, 0, 0, 1], [UNKNOWN, 0, UNKNOWN, 0, 0, 0]]
    assert stats == dict(windows=6, found=5, counted=5, distinct=3, values=6, votes=12, unclassified=3, ambiguous=2)
    votes, calls, stats = restate(rec, owner, index, 4, None, NODE_SHIFT, cmap, 2, PER_WINDOW)
    assert votes.tolist() == [[1, 1], [1, 1], [0, 0], [0, 0]] and calls[0].tolist() == [0, 1, 1, 1, 2, 2]
    votes, calls, stats = restate(rec, owner, index, 4, None, NODE_SHIFT, cmap, 2, UNAMBIGUOUS)
    assert votes.tolist() == [[0, 0]] * 4 and stats["ambiguous"] == 2 and stats["votes"] == 0
    cmap = cmap.copy()
    cmap[1] = 0                                                   # now run 0 has one class
    votes, calls, stats = restate(rec, owner, index, 4, None, NODE_SHIFT, cmap, 2, UNAMBIGUOUS)
    assert votes.tolist() == [[4, 0], [4, 0], [0, 0], [0, 0]] and stats["ambiguous"] == 0 and calls[0].tolist() == [0, 4, UNKNOWN, 0, 4, 2]


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


def to_device(a, dtype=np.int64):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dtype).copy()).to(torch.device("cuda", 0))


class Outputs:
    """Sentinel-filled device buffers of one call with GUARD sentinel words behind them; each may be absent."""

    def __init__(self, n, n_classes, votes=True, calls=True, stats=True):
        import torch
        dev = torch.device("cuda", 0)
        fill = np.uint64(SENTINEL).view(np.int64).item()
        self.n, self.C, self.stats = n, n_classes, stats
        self.votes = torch.full((n * n_classes + GUARD,), fill, dtype=torch.int64, device=dev) if votes else None
        self.calls = torch.full((n * 6 + GUARD,), fill, dtype=torch.int64, device=dev) if calls else None

    def pointers(self):
        return (self.votes.data_ptr() if self.votes is not None else 0, self.calls.data_ptr() if self.calls is not None else 0)

    def check(self, got_stats, want, what):
        """Rows and calls fully overwritten with the expected, the guards untouched, every stats field equal."""
        import torch
        votes, calls, stats = want
        torch.cuda.synchronize()
        fill = np.uint64(SENTINEL).view(np.int64).item()
        if self.votes is not None:
            n = self.n * self.C
            if not torch.equal(self.votes[:n], to_device(votes.reshape(-1))):
                got = self.votes[:n].cpu().numpy().view(np.uint64).reshape(self.n, self.C)
                bad = np.argwhere(got != votes)
                raise AssertionError((what, "votes", len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(votes[tuple(bad[0])])))
            assert bool((self.votes[n:] == fill).all()), (what, "behind the votes")
        if self.calls is not None:
            got = self.calls.cpu().numpy().view(np.uint64)
            bad = np.nonzero((got[:self.n * 6].reshape(self.n, 6) != calls).any(axis=1))[0]
            assert bad.size == 0, (what, "calls", int(bad.size), int(bad[0]), got[:self.n * 6].reshape(self.n, 6)[bad[0]].tolist(), calls[bad[0]].tolist())
            assert (got[self.n * 6:] == np.uint64(SENTINEL)).all(), (what, "behind the calls")
        if self.stats:
            assert got_stats == stats, (what, got_stats, stats)
        else:
            assert got_stats is None


DEVICE_MAPS = {}


def device_map(cmap):
    """The map in device memory (None for an empty one); the copies of the cached maps are kept, a few dozen at most."""
    if cmap.shape[0] == 0:
        return None
    if cmap.flags.writeable:
        return to_device(cmap, np.int32)
    if id(cmap) not in DEVICE_MAPS:
        if len(DEVICE_MAPS) >= 48:
            DEVICE_MAPS.clear()
        DEVICE_MAPS[id(cmap)] = (cmap, to_device(cmap, np.int32))
    return DEVICE_MAPS[id(cmap)][1]


def kmer_call(gpu, batch, k, stride, hit_max, shift, flags, cmap, n_classes, out):
    d_map = device_map(cmap)
    pv, pc = out.pointers()
    return gpu.kmer_classes_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, k, stride, hit_max, shift, flags,
                                   d_map.data_ptr() if d_map is not None else 0, cmap.shape[0], n_classes, pv, pc, want_stats=out.stats)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_parity_with_the_oracle(engine, which):
    """2. Rows, calls and every field of stats equal the restatement exactly over the grid (see the module's text); the buffers
    are prefilled with a sentinel, rows and calls are fully overwritten and the 64 words behind them unchanged.  On four points
    per graph each of d_votes / d_calls / stats is absent in turn, and all three.  The calls that ran on the 6000-base graph hold
    reads with a tie for best, reads with exactly one voted class and reads with counted records but no vote."""
    kmers = kmers_of(which)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    batch = DeviceReads(reads_of(which))
    voted = beyond = 0
    seen = [0, 0, 0]                                             # reads with a tie for best, with one voted class, silent though counted
    for p, (k, stride, hit_max, shift) in enumerate(grid_points()):
        rec, _ = kmers.records(k, stride, hit_max)
        n_bins = bins_of(which, shift)
        for i, (flags, C, kind) in enumerate(grid_combinations(p)):
            cmap = class_map(kind, n_bins, C)
            beyond += int(kind == "short" and rec.largest_bin(shift) >= cmap.shape[0])
            what = (GRAPHS[which][0], k, stride, hit_max, shift, flags, C, kind)
            want = kmers.want(k, stride, hit_max, shift, cmap, C, flags)
            out = Outputs(batch.n, C)
            out.check(kmer_call(gpu, batch, k, stride, hit_max, shift, flags, cmap, C, out), want, what)
            voted += want[2]["votes"]
            if which == BIG:
                votes, calls = want[0], want[1]
                seen[0] += int(((votes == calls[:, 1:2]).sum(axis=1)[calls[:, 1] > 0] >= 2).sum())
                seen[1] += int(((calls[:, 0] != np.uint64(UNKNOWN)) & (calls[:, 2] == np.uint64(UNKNOWN))).sum())
                seen[2] += int(((calls[:, 4] == 0) & (calls[:, 5] > 0)).sum())
            if p % 20 == 7 and i == 0:
                for absent in (dict(votes=False), dict(calls=False), dict(stats=False), dict(votes=False, calls=False, stats=False)):
                    out = Outputs(batch.n, C, **absent)
                    out.check(kmer_call(gpu, batch, k, stride, hit_max, shift, flags, cmap, C, out), want, what + (tuple(absent),))
    assert voted > 0 and beyond > 0                              # the short map is shorter than the largest bin of some call
    assert which != BIG or min(seen) > 0, seen
    gpu.close()


@pytest.mark.gpu
def test_shapes_across_wavefront_and_workgroup_edges(big):
    """4. 1, 63, 64 and 65 reads; empty reads and reads shorter than k; no read at all; one read of 1000 windows of one k-mer
    beside 200 reads of one window each; a read with more records than one pass of its wavefront (64)."""
    cpu = indexed(BIG)[1]
    reads = reads_of(BIG)
    for n in (1, 63, 64, 65):
        some = reads[:n]
        kmers = Kmers(Oracle(cpu, some))
        for k, hit_max, C, kind, flags in ((8, 0, 5, "interleaved", 0), (3, 0, 64, "holes", PER_WINDOW)):
            rec, _ = kmers.records(k, 1, hit_max)
            cmap = class_map(kind, rec.largest_bin(NODE_SHIFT) + 1, C)
            out = Outputs(n, C)
            out.check(kmer_call(big, DeviceReads(some), k, 1, hit_max, NODE_SHIFT, flags, cmap, C, out),
                      kmers.want(k, 1, hit_max, NODE_SHIFT, cmap, C, flags), ("reads", n, k))
    # empty reads, reads shorter than k, nothing found
    for some, k in (([b"ACGT", b"", b"ACGTACG", b"A"], 8), ([b"NNNN", b"XYZ", b"NNNN", b""], 2), ([b"", b""], 1)):
        kmers = Kmers(Oracle(cpu, some))
        cmap = class_map("interleaved", 16, 5)
        want = kmers.want(k, 1, 3, NODE_SHIFT, cmap, 5, 0)
        assert want[2] == dict(dict.fromkeys(FIELDS, 0), windows=sum(window_count(len(r), k, 1) for r in some))
        assert (want[1] == np.asarray([UNKNOWN, 0, UNKNOWN, 0, 0, 0], dtype=np.uint64)).all()
        out = Outputs(len(some), 5)
        out.check(kmer_call(big, DeviceReads(some), k, 1, 3, NODE_SHIFT, 0, cmap, 5, out), want, ("nothing", some, k))
    # no read: nothing is written, the stats are zero
    out = Outputs(0, 5)
    stats = kmer_call(big, DeviceReads([]), 8, 1, 0, NODE_SHIFT, 0, class_map("interleaved", 16, 5), 5, out)
    out.check(stats, (np.zeros((0, 5), dtype=np.uint64), np.zeros((0, 6), dtype=np.uint64), dict.fromkeys(FIELDS, 0)), "no read")
    # one k-mer 1000 times in one read beside 200 reads of one window each
    k = 4
    units = [u for u in (b"A", b"C", b"G", b"T", b"AC", b"AG", b"AT", b"CA", b"CT", b"GA", b"GT", b"TA", b"TC", b"TG", b"CG", b"GC")
             if nonempty_of(np.asarray([cpu.find((u * k)[:k])], dtype=np.uint64))[0]]
    unit = units[0]
    stride = len(unit)
    long_read = (unit * (k + 1000 * stride))[:k + 999 * stride]
    assert window_count(len(long_read), k, stride) == 1000
    singles = [reads[i % 100][j:j + k] for i in range(200) for j in (i // 100 * 7,)]
    some = singles[:100] + [long_read] + singles[100:]
    assert all(window_count(len(r), k, stride) == 1 for r in singles)
    kmers = Kmers(Oracle(cpu, some))
    rec, owner = kmers.records(k, stride, 0)
    assert int((owner == 100).sum()) == 1000 and len(set(rec.run_of[owner == 100].tolist())) == 1 and rec.run_of[owner == 100][0] >= 0
    for C, kind, flags in ((5, "interleaved", 0), (4096, "blocked", UNAMBIGUOUS), (64, "holes", PER_WINDOW)):
        cmap = class_map(kind, rec.largest_bin(NODE_SHIFT) + 1, C)
        out = Outputs(len(some), C)
        out.check(kmer_call(big, DeviceReads(some), k, stride, 0, NODE_SHIFT, flags, cmap, C, out),
                  kmers.want(k, stride, 0, NODE_SHIFT, cmap, C, flags), ("1000 windows", C, kind))
    # reads with more than 64 counted records: several passes of the wavefront, across the 64-window spans of the search
    walk = reads[0]
    some = [b"N" * 9, walk[:40] * 5, walk[:33], walk[3:50] * 3]
    kmers = Kmers(Oracle(cpu, some))
    rec, owner = kmers.records(8, 1, 0)
    assert int(((owner == 1) & (rec.run_of >= 0)).sum()) > 128 and int(((owner == 3) & (rec.run_of >= 0)).sum()) > 64
    for C, kind in ((5, "interleaved"), (64, "beyond")):
        cmap = class_map(kind, rec.largest_bin(NODE_SHIFT) + 1, C)
        out = Outputs(len(some), C)
        out.check(kmer_call(big, DeviceReads(some), 8, 1, 0, NODE_SHIFT, 0, cmap, C, out), kmers.want(8, 1, 0, NODE_SHIFT, cmap, C, 0), ("long reads", C))


def seed_call(gpu, d_goff, n_groups, d_seeds, n_seeds, d_weights, hit_max, shift, flags, cmap, n_classes, out):
    d_map = device_map(cmap)
    pv, pc = out.pointers()
    return gpu.seed_classes_device(d_goff.data_ptr() if d_goff is not None else 0, n_groups, d_seeds.data_ptr() if n_seeds else 0, n_seeds,
                                   d_weights.data_ptr() if d_weights is not None else 0, hit_max, shift, flags,
                                   d_map.data_ptr() if d_map is not None else 0, cmap.shape[0], n_classes, pv, pc, want_stats=out.stats)


def seeds_want(oracle, goff, seeds, weights, hit_max, shift, cmap, n_classes, flags):
    """The restatement for a seed call: the groups whose offsets decrease or reach beyond the records own nothing."""
    ranges = np.ascontiguousarray(seeds[:, 2:4], dtype=np.uint64)
    counts = oracle.cpu.count_batch(ranges) if ranges.shape[0] else np.zeros(0, dtype=np.uint64)
    rec = Records(oracle, ranges, counts, hit_max)
    owner, index = [], []
    for g in range(len(goff) - 1):
        a, b = int(goff[g]), int(goff[g + 1])
        if a <= b <= seeds.shape[0]:
            owner += [g] * (b - a)
            index += list(range(a, b))
    return restate(rec, np.asarray(owner, dtype=np.int64), np.asarray(index, dtype=np.int64), len(goff) - 1, weights, shift, cmap, n_classes, flags), rec


@pytest.mark.gpu
def test_seed_form(big):
    """5. The records and seed offsets of kmer_hits_device, mem_hits_device and capped_seeds_device, as they lie in device
    memory, voted per read; weights 0, 1, 7 and 2^40; the k-mer seeds give the rows of the k-mer form; empty groups, records
    with an empty range of both forms and one that reaches beyond the index; groups with decreasing offsets and offsets beyond
    n_seeds own nothing and disturb nothing."""
    import torch
    reads = reads_of(BIG)
    oracle = oracle_of(BIG)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    p, o = batch.d_pat.data_ptr(), batch.d_off.data_ptr()

    def on_device(call, sized):
        m, h = sized[1].shape[0], sized[3].shape[0]
        d_soff = torch.zeros(batch.n + 1, dtype=torch.int64, device=batch.dev)
        d_seeds = torch.zeros((max(m, 1), 5), dtype=torch.int64, device=batch.dev)
        d_hoff = torch.zeros(m + 1, dtype=torch.int64, device=batch.dev)
        d_hits = torch.zeros(max(h, 1), dtype=torch.int64, device=batch.dev)
        assert call(d_soff, d_seeds, d_hoff, d_hits, m, h) == (m, h)
        torch.cuda.synchronize()
        return d_soff, d_seeds, d_soff.cpu().numpy().view(np.uint64), d_seeds.cpu().numpy().view(np.uint64)[:m]

    kmer = on_device(lambda so, se, ho, hi, m, h: big.kmer_hits_device(p, o, batch.n, 8, 1, 3, 0, 0, so.data_ptr(), se.data_ptr(), m, ho.data_ptr(), hi.data_ptr(), h),
                     big.kmer_hits_batch(flat, off, 8, 1, 3, False))
    mems = on_device(lambda so, se, ho, hi, m, h: big.mem_hits_device(p, o, batch.n, None, 6, 3, 0, so.data_ptr(), se.data_ptr(), m, ho.data_ptr(), hi.data_ptr(), h),
                     big.mem_hits_batch(flat, off, 6, 3, False))
    capped = on_device(lambda so, se, ho, hi, m, h: big.capped_seeds_device(p, o, batch.n, 4, 0, 3, 0, 0, so.data_ptr(), se.data_ptr(), m, ho.data_ptr(), hi.data_ptr(), h),
                       big.capped_seeds_batch(flat, off, 4, 0, 3, 0, False))
    big_weight = 0
    for name, (d_soff, d_seeds, soff, seeds) in (("kmer", kmer), ("mem", mems), ("capped", capped)):
        m = seeds.shape[0]
        assert m > 64 and int(soff[-1]) == m and (np.diff(soff.astype(np.int64)) == 0).any(), name          # empty groups among them
        weights = np.asarray([(0, 1, 7, 1 << 40)[i % 4] for i in range(m)], dtype=np.uint64)
        d_weights = to_device(weights)
        for hit_max, shift, flags, C, kind in ((3, NODE_SHIFT, 0, 5, "interleaved"), (0, 0, PER_WINDOW, 64, "holes"), (1, NODE_SHIFT, UNAMBIGUOUS, 4096, "blocked"),
                                               (0, NODE_SHIFT, 0, 5, "short")):
            for w, d_w in ((None, None), (weights, d_weights)):
                want, rec = seeds_want(oracle, soff, seeds, w, hit_max, shift, class_map(kind, 1, C), C, flags)
                cmap = class_map(kind, rec.largest_bin(shift) + 1, C)
                want, rec = seeds_want(oracle, soff, seeds, w, hit_max, shift, cmap, C, flags)
                assert rec.counted > 0
                out = Outputs(batch.n, C)
                out.check(seed_call(big, d_soff, batch.n, d_seeds, m, d_w, hit_max, shift, flags, cmap, C, out), want, (name, hit_max, shift, flags, C, kind, w is not None))
                if w is not None:
                    big_weight = max(big_weight, int(want[0].max()))
    assert big_weight > 1 << 41                                   # sums that need more than 32 bits, of weights that do
    # the k-mer seeds under SKIP are the found windows: the rows, calls and stats of the k-mer form, but for `windows`
    d_soff, d_seeds, soff, seeds = kmer
    kmers = kmers_of(BIG)
    for flags, C, kind in ((0, 5, "interleaved"), (PER_WINDOW | UNAMBIGUOUS, 64, "holes")):
        rec, _ = kmers.records(8, 1, 3)
        cmap = class_map(kind, rec.largest_bin(NODE_SHIFT) + 1, C)
        want = kmers.want(8, 1, 3, NODE_SHIFT, cmap, C, flags)
        out = Outputs(batch.n, C)
        out.check(kmer_call(big, batch, 8, 1, 3, NODE_SHIFT, flags, cmap, C, out), want, ("k-mer form", flags))
        out = Outputs(batch.n, C)
        out.check(seed_call(big, d_soff, batch.n, d_seeds, seeds.shape[0], None, 3, NODE_SHIFT, flags, cmap, C, out),
                  (want[0], want[1], dict(want[2], windows=seeds.shape[0])), ("k-mer seeds", flags))
    # empty records of both forms, one beyond the index, a garbage count field; bad groups
    d_soff, d_seeds, soff, seeds = mems
    n = indexed(BIG)[1].n
    odd = np.asarray([[0, 5, 1, 0, 9], [0, 5, n + 3, n + 2, 1], [0, 0, 0, U64, 0], [3, 3, 7, 6, 1], [0, 4, n - 2, n + 5, 3]], dtype=np.uint64)
    assert not nonempty_of(odd[:4, 2:4]).any() and nonempty_of(odd[4:, 2:4]).all()
    mixed = np.concatenate([odd[:2], seeds[:70], odd[2:], seeds[70:], odd])
    mixed[::2, 4] = np.uint64(SENTINEL)
    m = mixed.shape[0]
    weights = np.asarray([(3, 0, 1 << 40)[i % 3] for i in range(m)], dtype=np.uint64)
    goff = np.asarray([0, 40, 40, 90, 60, 80, m + 1, 100, 100, m, m, 5, U64, 0, m], dtype=np.uint64)
    bad = [g for g in range(len(goff) - 1) if not int(goff[g]) <= int(goff[g + 1]) <= m]
    assert len(bad) >= 5 and any(int(goff[g + 1]) > m for g in bad) and any(int(goff[g]) > int(goff[g + 1]) for g in bad)
    for flags, C, kind in ((0, 5, "interleaved"), (PER_WINDOW, 64, "holes")):
        want, rec = seeds_want(oracle, goff, mixed, weights, 3, NODE_SHIFT, class_map(kind, 1, C), C, flags)
        cmap = class_map(kind, rec.largest_bin(NODE_SHIFT) + 1, C)
        want, rec = seeds_want(oracle, goff, mixed, weights, 3, NODE_SHIFT, cmap, C, flags)
        assert (want[1][bad] == np.asarray([UNKNOWN, 0, UNKNOWN, 0, 0, 0], dtype=np.uint64)).all() and want[2]["votes"] > 0 and want[2]["windows"] == m
        out = Outputs(len(goff) - 1, C)
        out.check(seed_call(big, to_device(goff), len(goff) - 1, to_device(mixed), m, to_device(weights), 3, NODE_SHIFT, flags, cmap, C, out), want, ("bad groups", flags))
    # no seeds but groups; no groups
    cmap = class_map("interleaved", 8, 5)
    none = np.zeros((0, 5), dtype=np.uint64)
    goff = np.asarray([0, 0, 0, 1], dtype=np.uint64)
    want, _ = seeds_want(oracle, goff, none, None, 0, NODE_SHIFT, cmap, 5, 0)
    out = Outputs(3, 5)
    out.check(seed_call(big, to_device(goff), 3, None, 0, None, 0, NODE_SHIFT, 0, cmap, 5, out), want, "no seeds")
    out = Outputs(0, 5)
    out.check(seed_call(big, None, 0, to_device(mixed), m, None, 0, NODE_SHIFT, 0, cmap, 5, out),
              (np.zeros((0, 5), dtype=np.uint64), np.zeros((0, 6), dtype=np.uint64), dict.fromkeys(FIELDS, 0)), "no groups")


@pytest.mark.gpu
def test_consistency_with_kmer_support(big):
    """6. With every bin in class 0 and no flags the rows' sum equals added + dropped of gcsa2_kmer_support_device at the same
    parameters with n_bins = the map's size; stats.votes equals added and stats.unclassified equals dropped (weights 1)."""
    import torch
    batch = DeviceReads(reads_of(BIG))
    kmers = kmers_of(BIG)
    for k, stride, hit_max, shift in ((8, 1, 3, NODE_SHIFT), (3, 1, 0, NODE_SHIFT), (16, 3, 0, 0)):
        rec, _ = kmers.records(k, stride, hit_max)
        for n_bins in (rec.largest_bin(shift) + 1, (rec.largest_bin(shift) + 1) // 2):
            cmap = class_map("one", n_bins, 1)
            out = Outputs(batch.n, 1)
            stats = kmer_call(big, batch, k, stride, hit_max, shift, 0, cmap, 1, out)
            d_support = torch.zeros(n_bins + 1, dtype=torch.int64, device=batch.dev)
            sup = big.kmer_support_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, k, stride, hit_max, shift, 0, d_support.data_ptr(), n_bins)
            torch.cuda.synchronize()
            rows = int(out.votes[:batch.n].sum().item())
            assert rows == sup["added"] == stats["votes"] and stats["unclassified"] == sup["dropped"], (k, n_bins, rows, stats, sup)
            assert rows + stats["unclassified"] == sup["added"] + sup["dropped"] and sup["added"] > 0
            assert {f: stats[f] for f in FIELDS[:5]} == {f: sup[f] for f in FIELDS[:5]}
            if n_bins <= rec.largest_bin(shift):
                assert sup["dropped"] > 0


def client_lines(votes, calls, stats):
    lines = ["stats " + " ".join(str(stats[f]) for f in FIELDS)]
    lines += ["call %d %s" % (q, " ".join(str(int(x)) for x in calls[q])) for q in range(calls.shape[0])]
    lines += ["vote %d %d %d" % (q, c, int(votes[q, c])) for q, c in np.argwhere(votes != 0).tolist()]
    return lines


@pytest.fixture(scope="module")
def client(engine, tmp_path_factory):
    """tests/cpp/kmer_classes_client.cpp, the 6000-base index as a host-view file and its reads, one per line; the client's map
    is bin % modulus over n_bins bins."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    tmp = tmp_path_factory.mktemp("kmer_classes")
    reads = reads_of(BIG)
    assert all(b"\n" not in r for r in reads)
    save_host_view(indexed(BIG)[0], str(tmp / "index.g2hv"))
    (tmp / "reads.txt").write_bytes(b"".join(r + b"\n" for r in reads))
    exe = compile_client(str(tmp / "kmer_classes_client"), os.path.join(ROOT, "tests", "cpp", "kmer_classes_client.cpp"))

    def run(k, stride, hit_max, shift, flags, n_bins, modulus, n_classes, **env):
        full = _run_env()
        full.pop("GCSA2_SUPPORT_CHUNK", None)
        full.update(env)
        out = subprocess.run([exe, str(tmp / "index.g2hv"), str(tmp / "reads.txt")] + [str(int(x)) for x in (k, stride, hit_max, shift, flags, n_bins, modulus, n_classes)],
                             capture_output=True, text=True, env=full, timeout=300)
        assert out.returncode == 0, out.stderr
        return out.stdout.strip().split("\n")
    return run


@pytest.mark.gpu
def test_chunking_changes_nothing(client):
    """7. GCSA2_SUPPORT_CHUNK at 1, 64 and the default, each in a fresh process (the facade's client): identical rows, calls and
    stats, the restatement's.  Both small budgets are below the count() of some range; 64 also makes chunks of several small
    ranges, and at 1 every range is a chunk of its own, so that the signatures of many chunks lie behind one another."""
    kmers = kmers_of(BIG)
    counts = kmers.oracle.cpu.count_batch(kmers.records(3, 1, 0)[0].ranges)
    assert int(counts.max()) > 64 and int(np.sort(counts)[:2].sum()) <= 64 and counts.shape[0] > 8
    for k, hit_max, C, kind, flags in ((3, 0, 5, "interleaved", 0), (8, 0, 64, "beyond", PER_WINDOW)):
        n_bins = bins_of(BIG, NODE_SHIFT)
        want = client_lines(*kmers.want(k, 1, hit_max, NODE_SHIFT, class_map(kind, n_bins, C), C, flags))
        for env in (dict(GCSA2_SUPPORT_CHUNK="1"), dict(GCSA2_SUPPORT_CHUNK="64"), dict()):
            assert client(k, 1, hit_max, NODE_SHIFT, flags, n_bins, C + 3 if kind == "beyond" else C, C, **env) == want, (k, env)


@pytest.mark.gpu
def test_wide_values(engine):
    """8. The linear index whose values lie across 2^63 (tests/test_locate_wide_values.py), shift = 53: the bins are taken
    unsigned -- the values at and above 2^63 fall into bin 1024 and above, never below bin 1023."""
    from test_locate_wide_values import linear_index, text_read
    g, ix, cpu = linear_index("across-2^63")
    reads = [text_read(g, 31000, 40), text_read(g, 40000, 60), b"ACGT", b""]
    kmers = Kmers(Oracle(cpu, reads))
    gpu, _ = engine.open_index(ix)
    batch = DeviceReads(reads)
    for k, hit_max in ((1, 0), (2, 0), (12, 0)):
        rec, _ = kmers.records(k, 1, hit_max)
        bins = rec.values >> np.uint64(53)
        assert int(bins.min()) == 1023 and int(bins.max()) == 1024 and rec.counted > 0, (k, int(bins.min()), int(bins.max()))
        for cmap in (np.asarray([NONE] * 1023 + [0, 1], dtype=np.uint32), np.asarray([NONE] * 1023 + [2], dtype=np.uint32)):
            want = kmers.want(k, 1, hit_max, 53, cmap, 3, 0)
            assert want[2]["votes"] > 0
            out = Outputs(len(reads), 3)
            out.check(kmer_call(gpu, batch, k, 1, hit_max, 53, 0, cmap, 3, out), want, ("wide", k, cmap.shape[0]))
    gpu.close()


@pytest.mark.gpu
def test_host_form_and_facade(engine, big, client, monkeypatch):
    """9, 11. gcsa2_kmer_classes_batch equals the restatement in one piece, with each output absent; the facade's client
    (tests/cpp/kmer_classes_client.cpp) prints the same rows, calls and stats; the batch tiled to 3 MB under GCSA2_MS_PIECE_MB=1
    equals the device form row for row -- distinct and values are then per-piece sums; offsets[0] != 0 and decreasing offsets
    are refused with nothing written."""
    import torch
    kmers = kmers_of(BIG)
    once = reads_of(BIG)
    flat, off = concat_patterns(once)
    for k, stride, hit_max, shift, flags, C in ((8, 1, 3, NODE_SHIFT, 0, 5), (16, 3, 0, NODE_SHIFT, PER_WINDOW | UNAMBIGUOUS, 64)):
        rec, _ = kmers.records(k, stride, hit_max)
        n_bins = rec.largest_bin(shift) + 1
        cmap = class_map("beyond", n_bins, C)
        want = kmers.want(k, stride, hit_max, shift, cmap, C, flags)
        votes, calls, stats = big.kmer_classes_batch(flat, off, k, cmap, C, stride, hit_max, shift, bool(flags & PER_WINDOW), bool(flags & UNAMBIGUOUS))
        assert np.array_equal(votes, want[0]) and np.array_equal(calls, want[1]) and stats == want[2], (k, "host form")
        votes, calls, stats = big.kmer_classes_batch(flat, off, k, cmap, C, stride, hit_max, shift, bool(flags & PER_WINDOW), bool(flags & UNAMBIGUOUS), votes=False)
        assert votes is None and np.array_equal(calls, want[1]) and stats == want[2]
        votes, calls, stats = big.kmer_classes_batch(flat, off, k, cmap, C, stride, hit_max, shift, bool(flags & PER_WINDOW), bool(flags & UNAMBIGUOUS), calls=False)
        assert calls is None and np.array_equal(votes, want[0]) and stats == want[2]
        assert client(k, stride, hit_max, shift, flags, n_bins, C + 3, C) == client_lines(*want), (k, "facade")
    # refused offsets: nothing is written
    lib = engine.load_library()
    pat = (ctypes.c_uint8 * 16)(*b"ACGTACGTACGTACGT")
    cmap8 = (ctypes.c_uint32 * 8)(0, 1, 0, 1, 0, 1, 0, 1)
    for offsets in ((1, 8, 16), (0, 9, 8)):
        c_off = (ctypes.c_uint64 * 3)(*offsets)
        votes = (ctypes.c_uint64 * 4)(*([SENTINEL] * 4))
        calls = (ctypes.c_uint64 * 12)(*([SENTINEL] * 12))
        stats = (ctypes.c_uint64 * 8)(*([SENTINEL] * 8))
        rc = lib.gcsa2_kmer_classes_batch(big._h, pat, c_off, 2, 4, 1, 0, NODE_SHIFT, 0, ctypes.addressof(cmap8), 8, 2, ctypes.addressof(votes),
                                          ctypes.addressof(calls), ctypes.addressof(stats))
        assert rc == INVALID and "offsets" in lib.gcsa2_last_error().decode(), offsets
        assert list(votes) == [SENTINEL] * 4 and list(calls) == [SENTINEL] * 12 and list(stats) == [SENTINEL] * 8
    # several pieces: the batch repeated until it is 3 MB of reads, in 1 MB pieces, against the device form on the same batch
    monkeypatch.setenv("GCSA2_MS_PIECE_MB", "1")
    pieced, _ = engine.open_index(indexed(BIG)[0], device=0)
    monkeypatch.delenv("GCSA2_MS_PIECE_MB")
    repeats = (3 << 20) // sum(len(r) for r in once) + 1
    tiled = once * repeats
    flat, off = concat_patterns(tiled)
    assert int(off[-1]) >= 3 << 20
    k, hit_max, C = 16, 3, 5
    rec, _ = kmers.records(k, 1, hit_max)
    cmap = class_map("interleaved", rec.largest_bin(NODE_SHIFT) + 1, C)
    want = kmers.want(k, 1, hit_max, NODE_SHIFT, cmap, C, 0)
    batch = DeviceReads(tiled)
    out = Outputs(batch.n, C)
    whole = kmer_call(big, batch, k, 1, hit_max, NODE_SHIFT, 0, cmap, C, out)
    torch.cuda.synchronize()
    d_votes = out.votes[:batch.n * C].cpu().numpy().view(np.uint64).reshape(batch.n, C)
    d_calls = out.calls[:batch.n * 6].cpu().numpy().view(np.uint64).reshape(batch.n, 6)
    assert np.array_equal(d_votes, np.tile(want[0], (repeats, 1))) and np.array_equal(d_calls, np.tile(want[1], (repeats, 1)))
    assert whole == dict({f: want[2][f] * repeats for f in FIELDS}, distinct=want[2]["distinct"], values=want[2]["values"])
    votes, calls, piece = pieced.kmer_classes_batch(flat, off, k, cmap, C, 1, hit_max, NODE_SHIFT)
    assert np.array_equal(votes, d_votes) and np.array_equal(calls, d_calls)
    assert piece["distinct"] > whole["distinct"] and piece["values"] > whole["values"]
    assert {f: piece[f] for f in FIELDS if f not in ("distinct", "values")} == {f: whole[f] for f in FIELDS if f not in ("distinct", "values")}
    pieced.close()


@pytest.mark.gpu
def test_refusals_on_a_device(engine, big):
    """10. With a real handle: every INVALID_ARGUMENT again through the binding, nothing written; n_bins == 0 is valid and
    leaves everything unclassified; an image without samples or counters is MISSING_COMPONENT, nothing written."""
    batch = DeviceReads(reads_of(BIG))
    cmap = class_map("interleaved", 2000, 5)
    untouched = (np.full((batch.n, 5), SENTINEL, dtype=np.uint64), np.full((batch.n, 6), SENTINEL, dtype=np.uint64), None)
    for change in (dict(k=0), dict(stride=0), dict(shift=64), dict(flags=4), dict(C=0), dict(C=LIMIT + 1)):
        arg = dict(dict(k=8, stride=1, shift=NODE_SHIFT, flags=0, C=5), **change)
        out = Outputs(batch.n, 5)
        with pytest.raises(engine.Gcsa2Error) as err:
            kmer_call(big, batch, arg["k"], arg["stride"], 0, arg["shift"], arg["flags"], cmap, arg["C"], out)
        assert err.value.code == INVALID, change
        out.stats = False
        out.check(None, untouched, change)
    out = Outputs(batch.n, 5)
    with pytest.raises(engine.Gcsa2Error) as err:
        big.kmer_classes_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, 8, 1, 0, NODE_SHIFT, 0, 0, 2000, 5, *out.pointers())
    assert err.value.code == INVALID
    out.stats = False
    out.check(None, untouched, "NULL map")
    # n_bins == 0: everything is unclassified
    kmers = kmers_of(BIG)
    want = kmers.want(8, 1, 3, NODE_SHIFT, np.zeros(0, dtype=np.uint32), 5, 0)
    assert want[2]["votes"] == 0 and want[2]["unclassified"] > 0 and want[2]["ambiguous"] == 0
    out = Outputs(batch.n, 5)
    out.check(kmer_call(big, batch, 8, 1, 3, NODE_SHIFT, 0, np.zeros(0, dtype=np.uint32), 5, out), want, "n_bins == 0")
    for missing in (dict(with_samples=False), dict(with_counters=False), dict(with_samples=False, with_counters=False)):
        lame = engine.GCSA(indexed(BIG)[0], with_lcp=False, **missing)
        for form in ("kmer", "seed"):
            out = Outputs(batch.n, 5)
            with pytest.raises(engine.Gcsa2Error) as err:
                if form == "kmer":
                    kmer_call(lame, batch, 8, 1, 0, NODE_SHIFT, 0, cmap, 5, out)
                else:
                    seed_call(lame, to_device(np.asarray([0, 1], dtype=np.uint64)), 1, to_device(np.asarray([[0, 4, 1, 2, 2]], dtype=np.uint64)), 1, None, 0,
                              NODE_SHIFT, 0, cmap, 5, Outputs(1, 5))
            assert err.value.code == MISSING, (missing, form)
        out.stats = False
        out.check(None, untouched, missing)
        lame.close()
