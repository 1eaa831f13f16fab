"""Batched k-mer top classes (gcsa2_kmer_top_classes_device / gcsa2_kmer_top_classes_batch / gcsa2_seed_top_classes_device,
k_classes_top of kernels_classes.hpp): per read -- or group of seed records -- the top_n classes with the most votes and
{voted, total, counted}, for up to 0xFFFFFFFF classes.  The expectations are the CPU oracle's alone: `Records` / `Kmers` of
test_kmer_classes.py and `sparse_restate`, the DEFINITION of include/gcsa2_hip.h in numpy as per (group, class) sums over
sorted keys -- no n_groups x n_classes array exists.  Every comparison is exact.

The parity grid: (k, stride, hit_max, shift) is the full product of the reduced lists on every graph; each of its 60 points
runs 4 of the 336 combinations of (top_n, flags, map and C), taken in turn with a step coprime to 336 and a start that moves
with the graph, so that the 11 graphs together visit every combination several times."""
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
from test_kmer_classes import (Records, Kmers, kmers_of, bins_of, class_map, to_device, device_map, FIELDS, PER_WINDOW, UNAMBIGUOUS, NODE_SHIFT, UNKNOWN,
                               U64, INVALID, MISSING, GUARD)
import test_kmer_classes as dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP_LIMIT = 64                                          # GCSA2_TOP_LIMIT
WIDE = 0xFFFFFFFF                                       # the largest n_classes
GRID_K, GRID_STRIDE, GRID_HIT_MAX, GRID_SHIFT = (1, 3, 8, 16, 33), (1, 3), (0, 3, 64), (0, 11)
GRID_TOP, GRID_FLAGS = (1, 2, 5, 64), (0, PER_WINDOW, UNAMBIGUOUS, PER_WINDOW | UNAMBIGUOUS)
GRID_MAPS = [(kind, C) for kind in ("interleaved", "holes", "beyond", "short") for C in (1, 5, 4096, 4097, 100003)] + [("identity", 0)]
COMBINATIONS = len(GRID_TOP) * len(GRID_FLAGS) * len(GRID_MAPS)     # 336
STEP = 47                                               # coprime to 336


def sparse_restate(rec, owner, index, n_groups, weights, shift, cmap, n_classes, flags, top_n):
    """The DEFINITION, sparse: (top (n_groups, top_n, 2), summaries (n_groups, 3), stats, tie) with tie[q] = the class behind
    the row's last entry has the same votes as that entry.  Group owner[i] owns record index[i]; weights per record or None.
    One entry per (owned record, class of its signature), sorted by (group, class) and summed; then sorted by (group, votes
    descending, class) and cut."""
    C = n_classes
    e_off, e_cls, e_n, none_of, classes_of, _ = rec.signatures(shift, cmap, C)
    weights = np.ones(rec.m, dtype=np.uint64) if weights is None else np.asarray(weights, dtype=np.uint64)
    keep = rec.run_of[index] >= 0
    g, r, w = owner[keep].astype(np.int64), rec.run_of[index[keep]], weights[index[keep]]
    stats = dict(windows=rec.windows, found=rec.found, counted=rec.counted, distinct=rec.ranges.shape[0], values=rec.values.shape[0],
                 unclassified=int(none_of[r].sum()), ambiguous=int((classes_of[r] >= 2).sum()))
    sums = np.zeros((n_groups, 3), dtype=np.uint64)
    sums[:, 2] = np.bincount(g, minlength=n_groups).astype(np.uint64)
    if flags & UNAMBIGUOUS:
        ok = classes_of[r] == 1
        g, r, w = g[ok], r[ok], w[ok]
    full = np.zeros((n_groups, top_n + 1, 2), dtype=np.uint64)
    full[:, :, 0] = np.uint64(UNKNOWN)
    cnt = classes_of[r] if g.shape[0] else np.zeros(0, dtype=np.int64)
    if int(cnt.sum()):
        rep = np.repeat(np.arange(r.shape[0]), cnt)
        e = e_off[r][rep] + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        x = w[rep] if flags & PER_WINDOW else w[rep] * e_n[e]
        eg, ec = g[rep], e_cls[e].astype(np.int64)
        order = np.lexsort((ec, eg))
        eg, ec, x = eg[order], ec[order], x[order]
        starts = np.nonzero(np.concatenate([[True], (eg[1:] != eg[:-1]) | (ec[1:] != ec[:-1])]))[0]
        v = np.add.reduceat(x, starts)                     # 64-bit sums
        sg, sc = eg[starts], ec[starts]
        live = v > 0                                       # a class of zero-weight records only has no vote
        sg, sc, v = sg[live], sc[live], v[live]
        sums[:, 0] = np.bincount(sg, minlength=n_groups).astype(np.uint64)
        np.add.at(sums[:, 1], sg, v)
        order = np.lexsort((sc, np.uint64(U64) - v, sg))
        sg, sc, v = sg[order], sc[order], v[order]
        rank = np.arange(sg.shape[0]) - np.searchsorted(sg, sg, side="left")
        sel = rank <= top_n
        full[sg[sel], rank[sel], 0] = sc[sel].astype(np.uint64)
        full[sg[sel], rank[sel], 1] = v[sel]
    stats["votes"] = int(sums[:, 1].sum(dtype=np.uint64))
    tie = (full[:, top_n, 1] > 0) & (full[:, top_n, 1] == full[:, top_n - 1, 1])
    return np.ascontiguousarray(full[:, :top_n]), sums, {f: stats[f] for f in FIELDS}, tie


def top_of_dense(votes, calls, top_n):
    """(top, summaries) from the dense row and calls of test_kmer_classes.restate: the non-zero entries, more votes first and
    the lower id on a tie."""
    n = votes.shape[0]
    top = np.zeros((n, top_n, 2), dtype=np.uint64)
    top[:, :, 0] = np.uint64(UNKNOWN)
    sums = np.zeros((n, 3), dtype=np.uint64)
    for q in range(n):
        ids = np.nonzero(votes[q])[0]
        ids = ids[np.lexsort((ids, np.uint64(U64) - votes[q][ids]))][:top_n]
        top[q, :ids.shape[0], 0] = ids.astype(np.uint64)
        top[q, :ids.shape[0], 1] = votes[q][ids]
        sums[q] = (np.count_nonzero(votes[q]), calls[q, 4], calls[q, 5])
    return top, sums


def kmers_want(kmers, k, stride, hit_max, shift, cmap, n_classes, flags, top_n):
    rec, owner = kmers.records(k, stride, hit_max)
    return sparse_restate(rec, owner, np.arange(rec.m), len(kmers.oracle.reads), None, shift, cmap, n_classes, flags, top_n)


@functools.lru_cache(maxsize=4)
def identity_map(n_bins):
    out = np.arange(n_bins, dtype=np.uint32)
    out.setflags(write=False)
    return out


def grid_map(kind, C, n_bins):
    """(map, n_classes) of one entry of GRID_MAPS."""
    if kind == "identity":
        return identity_map(n_bins), n_bins
    return class_map(kind, n_bins, C), C


def grid_points():
    return [(k, stride, hit_max, shift) for k in GRID_K for stride in GRID_STRIDE for hit_max in GRID_HIT_MAX for shift in GRID_SHIFT]


def grid_combinations(which, point):
    out = []
    for i in range(4):
        j = (STEP * (240 * which + 4 * point + i)) % COMBINATIONS
        out.append((GRID_TOP[j % 4], GRID_FLAGS[(j // 4) % 4]) + GRID_MAPS[j // 16])
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    return binding.load_library()


def test_library_exports_the_top_classes_calls(lib):
    """1. The header declares the three calls, the two structures and GCSA2_TOP_LIMIT; the built library exports the calls and
    the binding mirrors all of it."""
    from gcsa2_amd import binding
    header = open(os.path.join(ROOT, "include", "gcsa2_hip.h")).read()
    for name in ("gcsa2_kmer_top_classes_device", "gcsa2_kmer_top_classes_batch", "gcsa2_seed_top_classes_device"):
        assert ("int " + name + "(") in header, name
        assert name in binding.EXPORTS, name
        assert hasattr(ctypes.CDLL(binding.LIB_PATH), name), name
    for text in ("#define GCSA2_TOP_LIMIT 64", "typedef struct gcsa2_class_vote  { uint64_t class_id, votes; } gcsa2_class_vote;",
                 "typedef struct gcsa2_top_summary { uint64_t voted, total, counted; } gcsa2_top_summary;"):
        assert text in header, text
    assert binding.TOP_LIMIT == TOP_LIMIT
    assert binding.CLASS_VOTE.names == ("class_id", "votes") and binding.CLASS_VOTE.itemsize == 16
    assert binding.TOP_SUMMARY.names == ("voted", "total", "counted") and binding.TOP_SUMMARY.itemsize == 24
    for name in ("kmer_top_classes_batch", "kmer_top_classes_device", "seed_top_classes_device"):
        assert callable(getattr(binding.GCSA, name)), name
    facade = open(os.path.join(ROOT, "include", "gcsa", "gcsa.h")).read()
    assert "void kmer_top_classes_batch(" in facade
    assert 64 <= binding.TOP_SLOTS_DEFAULT <= 4096 and binding.TOP_SLOTS_DEFAULT & (binding.TOP_SLOTS_DEFAULT - 1) == 0


def test_the_grid_covers_every_combination():
    assert len(grid_points()) == 60 and COMBINATIONS == 336
    seen = {}
    for which in range(len(GRAPHS)):
        for p in range(60):
            for c in grid_combinations(which, p):
                seen[c] = seen.get(c, 0) + 1
    assert len(seen) == COMBINATIONS and min(seen.values()) >= 4
    for which in range(len(GRAPHS)):
        assert any(c[2] == "identity" for p in range(60) for c in grid_combinations(which, p)), which
    on_big = {c for p in range(60) for c in grid_combinations(BIG, p)}
    assert {c[0] for c in on_big} == set(GRID_TOP) and {c[2:] for c in on_big} == set(GRID_MAPS)


def refusal_cases():
    """(what the message names, keyword changes) of every refusal of the contract in front of the device."""
    return [("index", dict(index=None)), ("k must", dict(k=0)), ("stride must", dict(stride=0)), ("shift must", dict(shift=64)),
            ("shift must", dict(shift=U64)), ("unknown flags", dict(flags=4)), ("unknown flags", dict(flags=-1)), ("unknown flags", dict(flags=8 | 1)),
            ("n_classes must", dict(n_classes=0)), ("n_classes must", dict(n_classes=1 << 32)), ("n_classes must", dict(n_classes=U64)),
            ("top_n must", dict(top_n=0)), ("top_n must", dict(top_n=TOP_LIMIT + 1)), ("top_n must", dict(top_n=U64)),
            ("is NULL with n_bins", dict(cmap=False))]


def refuse(lib, form, **change):
    """One refused call on sentinel-filled host arrays (no device is touched before the refusal, so host pointers do for the
    device forms): (status, message, top, summaries and stats afterwards)."""
    arg = dict(index=None, k=4, stride=1, shift=NODE_SHIFT, flags=0, n_classes=2, top_n=2, cmap=True)
    arg.update(change)
    off = (ctypes.c_uint64 * 2)(0, 8)
    pat = (ctypes.c_uint8 * 8)(*b"ACGTACGT")
    seeds = (ctypes.c_uint64 * 5)(0, 4, 1, 2, 2)
    cmap = (ctypes.c_uint32 * 8)(0, 1, 0, 1, 0, 1, 0, 1)
    top = (ctypes.c_uint64 * 16)(*([SENTINEL] * 16))
    sums = (ctypes.c_uint64 * 12)(*([SENTINEL] * 12))
    stats = (ctypes.c_uint64 * 8)(*([SENTINEL] * 8))
    pm = ctypes.addressof(cmap) if arg["cmap"] else None
    pt, ps, pst = ctypes.addressof(top), ctypes.addressof(sums), ctypes.addressof(stats)
    if form == "kmer_device":
        rc = lib.gcsa2_kmer_top_classes_device(arg["index"], ctypes.addressof(pat), ctypes.addressof(off), 1, arg["k"], arg["stride"], 0, arg["shift"],
                                               arg["flags"], pm, 8, arg["n_classes"], arg["top_n"], pt, ps, pst, None)
    elif form == "kmer_batch":
        rc = lib.gcsa2_kmer_top_classes_batch(arg["index"], pat, off, 1, arg["k"], arg["stride"], 0, arg["shift"], arg["flags"], pm, 8, arg["n_classes"],
                                              arg["top_n"], pt, ps, pst)
    else:
        rc = lib.gcsa2_seed_top_classes_device(arg["index"], ctypes.addressof(off), 1, ctypes.addressof(seeds), 1, None, 0, arg["shift"], arg["flags"],
                                               pm, 8, arg["n_classes"], arg["top_n"], pt, ps, pst, None)
    return rc, lib.gcsa2_last_error().decode(), list(top), list(sums), list(stats)


def test_refusals_need_no_device(lib):
    """2. Every INVALID_ARGUMENT of the contract happens without a device -- the handle is a pointer to nothing that the checks
    never follow -- names its argument and leaves sentinel-filled rows, summaries and stats untouched; top_n = 0 and 65,
    n_classes = 0 and 2^32 among them.  n_classes = 4097 and 0xFFFFFFFF pass these checks (the missing device is what fails)."""
    nothing = ctypes.create_string_buffer(64)
    index = ctypes.addressof(nothing)
    for form in ("kmer_device", "kmer_batch", "seed_device"):
        for names, change in refusal_cases():
            if form == "seed_device" and names in ("k must", "stride must"):
                continue
            rc, message, top, sums, stats = refuse(lib, form, **dict(dict(index=index), **change))
            assert rc == INVALID and names in message, (form, change, rc, message)
            assert top == [SENTINEL] * 16 and sums == [SENTINEL] * 12 and stats == [SENTINEL] * 8, (form, change)


@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_sparse_restatement_equals_the_dense_one(which):
    """3. For C in (1, 5, 64, 4096) the sparse restatement equals the top rows, summaries and stats derived from the dense
    restatement of test_kmer_classes.py, over maps, flags and top_n in turn."""
    kmers = kmers_of(which)
    voted = 0
    for i, C in enumerate((1, 5, 64, 4096)):
        for j, (k, stride, hit_max, shift) in enumerate(((3, 1, 0, 0), (8, 1, 3, NODE_SHIFT), (16, 3, 64, NODE_SHIFT))):
            kind, flags, top_n = dense.MAPS[(i + j) % 5], GRID_FLAGS[(i + 2 * j) % 4], GRID_TOP[(i + j) % 4]
            cmap = class_map(kind, bins_of(which, shift), C)
            votes, calls, stats = kmers.want(k, stride, hit_max, shift, cmap, C, flags)
            top, sums, sparse_stats, _ = kmers_want(kmers, k, stride, hit_max, shift, cmap, C, flags, top_n)
            want_top, want_sums = top_of_dense(votes, calls, top_n)
            what = (GRAPHS[which][0], C, k, kind, flags, top_n)
            assert np.array_equal(top, want_top) and np.array_equal(sums, want_sums) and sparse_stats == stats, what
            voted += int(sums[:, 0].sum())
    assert voted > 0


def test_sparse_restatement_on_a_hand_made_case():
    """4. Values written down by hand: a tie at the cut (classes 1 and 100000 of group 1 at top_n = 2: the lower id is in the
    row), a tie inside the row, and a class that only a zero-weight record reaches (class 3 in group 2), which is not voted."""
    class Fixed(Oracle):
        def __init__(self):
            self.table = {(1, 2): [0 << 11, 1 << 11, 2 << 11, (2 << 11) + 5], (4, 4): [3 << 11], (7, 9): [9 << 11]}

        def locate(self, ranges):
            per = [np.asarray(self.table[tuple(r)], dtype=np.uint64) for r in ranges.tolist()]
            return np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64), np.concatenate(per + [np.zeros(0, dtype=np.uint64)]).astype(np.uint64)

    ranges = np.asarray([[1, 2], [4, 4], [1, 2], [5, 4], [7, 9], [4, 4]], dtype=np.uint64)
    counts = np.asarray([4, 1, 4, 0, 1, 1], dtype=np.uint64)
    rec = Records(Fixed(), ranges, counts, 0)
    big_id = 100000
    cmap = np.asarray([big_id, 1, 2, 3], dtype=np.uint32)         # run (1, 2): classes big_id, 1, 2 (two values); (4, 4): class 3; (7, 9): beyond the map
    owner, index = np.asarray([0, 0, 1, 1, 1, 2]), np.arange(6)
    weights = np.asarray([1, 2, 3, 9, 1, 0], dtype=np.uint64)
    # group 0: record 0 (w 1) -> {big_id: 1, 1: 1, 2: 2}, record 1 (w 2) -> {3: 2}: votes 2 -> 2, 3 -> 2, 1 -> 1, big_id -> 1
    # group 1: record 2 (w 3) -> {big_id: 3, 1: 3, 2: 6}; record 3 is empty; record 4 has no class
    # group 2: record 5 (w 0) -> class 3 with 0 votes: not voted;  group 3 owns nothing
    top, sums, stats, tie = sparse_restate(rec, owner, index, 4, weights, NODE_SHIFT, cmap, big_id + 1, 0, 2)
    assert top.tolist() == [[[2, 2], [3, 2]], [[2, 6], [1, 3]], [[UNKNOWN, 0]] * 2, [[UNKNOWN, 0]] * 2]
    assert sums.tolist() == [[4, 6, 2], [3, 12, 2], [0, 0, 1], [0, 0, 0]]
    assert tie.tolist() == [False, True, False, False]
    assert stats == dict(windows=6, found=5, counted=5, distinct=3, values=6, votes=18, unclassified=1, ambiguous=2)
    top, sums, _, tie = sparse_restate(rec, owner, index, 4, weights, NODE_SHIFT, cmap, big_id + 1, 0, 3)
    assert top[0].tolist() == [[2, 2], [3, 2], [1, 1]] and top[1].tolist() == [[2, 6], [1, 3], [big_id, 3]] and tie.tolist() == [True, False, False, False]
    top, sums, _, _ = sparse_restate(rec, owner, index, 4, None, NODE_SHIFT, cmap, big_id, PER_WINDOW, 5)     # big_id is now no class
    assert top[0].tolist() == [[1, 1], [2, 1], [3, 1], [UNKNOWN, 0], [UNKNOWN, 0]] and sums.tolist() == [[3, 3, 2], [2, 2, 2], [1, 1, 1], [0, 0, 0]]
    top, sums, stats, _ = sparse_restate(rec, owner, index, 4, None, NODE_SHIFT, cmap, big_id + 1, UNAMBIGUOUS, 1)
    assert top[:, 0].tolist() == [[3, 1], [UNKNOWN, 0], [3, 1], [UNKNOWN, 0]] and stats["ambiguous"] == 2 and stats["votes"] == 2


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


class Outputs:
    """Sentinel-filled device buffers of one call with GUARD sentinel words behind them; each may be absent."""

    def __init__(self, n, top_n, top=True, summaries=True, stats=True):
        import torch
        dev = torch.device("cuda", 0)
        fill = np.uint64(SENTINEL).view(np.int64).item()
        self.n, self.top_n, self.stats = n, top_n, stats
        self.top = torch.full((n * top_n * 2 + GUARD,), fill, dtype=torch.int64, device=dev) if top else None
        self.sums = torch.full((n * 3 + GUARD,), fill, dtype=torch.int64, device=dev) if summaries else None

    def pointers(self):
        return (self.top.data_ptr() if self.top is not None else 0, self.sums.data_ptr() if self.sums is not None else 0)

    def rows(self):
        import torch
        torch.cuda.synchronize()
        return self.top.cpu().numpy().view(np.uint64)[:self.n * self.top_n * 2].reshape(self.n, self.top_n, 2)

    def check(self, got_stats, want, what):
        """Rows and summaries fully overwritten with the expected, the guards untouched, every stats field equal."""
        import torch
        top, sums, stats = want[:3]
        torch.cuda.synchronize()
        if self.top is not None:
            got = self.top.cpu().numpy().view(np.uint64)
            n = self.n * self.top_n * 2
            rows = got[:n].reshape(self.n, self.top_n, 2)
            bad = np.nonzero((rows != top).any(axis=(1, 2)))[0]
            assert bad.size == 0, (what, "top", int(bad.size), int(bad[0]), rows[bad[0]].tolist()[:8], top[bad[0]].tolist()[:8])
            assert (got[n:] == np.uint64(SENTINEL)).all(), (what, "behind the top rows")
        if self.sums is not None:
            got = self.sums.cpu().numpy().view(np.uint64)
            rows = got[:self.n * 3].reshape(self.n, 3)
            bad = np.nonzero((rows != sums).any(axis=1))[0]
            assert bad.size == 0, (what, "summaries", int(bad.size), int(bad[0]), rows[bad[0]].tolist(), sums[bad[0]].tolist())
            assert (got[self.n * 3:] == np.uint64(SENTINEL)).all(), (what, "behind the summaries")
        if self.stats:
            assert got_stats == stats, (what, got_stats, stats)
        else:
            assert got_stats is None


def kmer_call(gpu, batch, k, stride, hit_max, shift, flags, cmap, n_classes, top_n, out):
    d_map = device_map(cmap)
    pt, ps = out.pointers()
    return gpu.kmer_top_classes_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, k, stride, hit_max, shift, flags,
                                       d_map.data_ptr() if d_map is not None else 0, cmap.shape[0], n_classes, top_n, pt, ps, want_stats=out.stats)


def seed_call(gpu, d_goff, n_groups, d_seeds, n_seeds, d_weights, hit_max, shift, flags, cmap, n_classes, top_n, out):
    d_map = device_map(cmap)
    pt, ps = out.pointers()
    return gpu.seed_top_classes_device(d_goff.data_ptr() if d_goff is not None else 0, n_groups, d_seeds.data_ptr() if n_seeds else 0, n_seeds,
                                       d_weights.data_ptr() if d_weights is not None else 0, hit_max, shift, flags,
                                       d_map.data_ptr() if d_map is not None else 0, cmap.shape[0], n_classes, top_n, pt, ps, want_stats=out.stats)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_parity_with_the_oracle(engine, which):
    """5. Top rows, summaries and every field of stats equal the sparse restatement exactly over the grid (see the module's
    text), the identity map among the maps (on the 6000-base graph at shift 0: 3 938 305 classes); the buffers are prefilled
    with a sentinel, fully overwritten and the 64 words behind them unchanged.  On three points per graph each of d_top /
    d_summaries / stats is absent in turn, and all three.  The calls on the 6000-base graph hold rows that are cut
    (voted > top_n), rows shorter than top_n and reads with a tie exactly at the cut."""
    kmers = kmers_of(which)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    batch = DeviceReads(reads_of(which))
    voted = beyond = identity = 0
    seen = [0, 0, 0]                                             # rows cut, rows shorter than top_n, ties at the cut
    for p, (k, stride, hit_max, shift) in enumerate(grid_points()):
        rec, _ = kmers.records(k, stride, hit_max)
        n_bins = bins_of(which, shift)
        for i, (top_n, flags, kind, C) in enumerate(grid_combinations(which, p)):
            cmap, C = grid_map(kind, C, n_bins)
            beyond += int(kind == "short" and rec.largest_bin(shift) >= cmap.shape[0])
            identity += int(kind == "identity")
            what = (GRAPHS[which][0], k, stride, hit_max, shift, top_n, flags, kind, C)
            want = kmers_want(kmers, k, stride, hit_max, shift, cmap, C, flags, top_n)
            out = Outputs(batch.n, top_n)
            out.check(kmer_call(gpu, batch, k, stride, hit_max, shift, flags, cmap, C, top_n, out), want, what)
            voted += want[2]["votes"]
            seen[0] += int((want[1][:, 0] > top_n).sum())
            seen[1] += int((want[1][:, 0] < top_n).sum())
            seen[2] += int(want[3].sum())
            if p % 20 == 7 and i == 0:
                for absent in (dict(top=False), dict(summaries=False), dict(stats=False), dict(top=False, summaries=False, stats=False)):
                    out = Outputs(batch.n, top_n, **absent)
                    out.check(kmer_call(gpu, batch, k, stride, hit_max, shift, flags, cmap, C, top_n, out), want, what + (tuple(absent),))
    assert voted > 0 and identity > 0
    if which == BIG:
        assert bins_of(BIG, 0) == 3938305 and beyond > 0
        assert min(seen) > 0, seen
    gpu.close()


def dense_outputs(gpu, call, n, C):
    """(votes (n, C), calls (n, 6), stats) of a dense call into fresh device buffers."""
    import torch
    out = dense.Outputs(n, C)
    stats = call(out)
    torch.cuda.synchronize()
    return (out.votes[:n * C].cpu().numpy().view(np.uint64).reshape(n, C), out.calls[:n * 6].cpu().numpy().view(np.uint64).reshape(n, 6), stats)


@pytest.mark.gpu
def test_the_law_against_the_dense_calls(big):
    """6. On the GPU, for C in (1, 5, 64, 4096) and equal arguments: the first two entries of the top row are the dense call's
    best and second, total, counted and every field of stats are equal, and the whole top row is the sorted non-zero entries
    of the dense row -- for the k-mer form and for the seed form over the records of kmer_hits_device with weights."""
    import torch
    reads = reads_of(BIG)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    soff_h, seeds_h, _, _ = big.kmer_hits_batch(flat, off, 8, 1, 3, False)
    m = seeds_h.shape[0]
    d_soff, d_seeds = to_device(np.asarray(soff_h, dtype=np.uint64)), to_device(np.asarray(seeds_h, dtype=np.uint64))
    weights = np.asarray([(0, 1, 7, 1 << 40)[i % 4] for i in range(m)], dtype=np.uint64)
    d_weights = to_device(weights)
    for i, C in enumerate((1, 5, 64, 4096)):
        kind, flags = ("interleaved", "holes", "beyond", "blocked")[i], GRID_FLAGS[i]
        for k, hit_max, shift in ((3, 0, 0), (8, 3, NODE_SHIFT)):
            cmap = class_map(kind, bins_of(BIG, shift), C)
            for form in ("kmer", "seed"):
                if form == "kmer":
                    votes, calls, stats = dense_outputs(big, lambda o: dense.kmer_call(big, batch, k, 1, hit_max, shift, flags, cmap, C, o), batch.n, C)
                else:
                    votes, calls, stats = dense_outputs(big, lambda o: dense.seed_call(big, d_soff, batch.n, d_seeds, m, d_weights, hit_max, shift, flags, cmap, C, o), batch.n, C)
                for top_n in (2, 64):
                    out = Outputs(batch.n, top_n)
                    if form == "kmer":
                        got = kmer_call(big, batch, k, 1, hit_max, shift, flags, cmap, C, top_n, out)
                    else:
                        got = seed_call(big, d_soff, batch.n, d_seeds, m, d_weights, hit_max, shift, flags, cmap, C, top_n, out)
                    top, sums = top_of_dense(votes, calls, top_n)
                    out.check(got, (top, sums, stats), ("law", form, C, k, top_n))
                    if C >= 2:
                        rows = out.rows()
                        assert np.array_equal(rows[:, :2].reshape(batch.n, 4), calls[:, :4]), ("law", form, C, k, "best and second")
            assert stats["votes"] > 0


@pytest.mark.gpu
def test_more_classes_than_the_table_holds(engine, big, monkeypatch):
    """7. The identity map at shift 0 and hit_max = 0 on the 6000-base graph: at k = 3 a read votes for up to 5008 classes (300
    of 312 reads for more than 2048), at k = 4 for up to 1973, at k = 8 for up to 79.  k = 3 and k = 4 with the default table,
    k = 8 with 64 and with 128 slots, k = 3 with 64 slots: always the restatement's rows; where the test says so the most
    voted read exceeds the slots in force."""
    kmers = kmers_of(BIG)
    batch = DeviceReads(reads_of(BIG))
    n_bins = bins_of(BIG, 0)
    cmap = identity_map(n_bins)
    default = engine.TOP_SLOTS_DEFAULT
    most = {}
    for k, slots, overflows in ((3, None, True), (4, None, None), (8, 64, True), (8, 128, False), (3, 64, True)):
        if slots is None:
            monkeypatch.delenv("GCSA2_TOP_SLOTS", raising=False)
        else:
            monkeypatch.setenv("GCSA2_TOP_SLOTS", str(slots))
        for top_n, flags in ((64, 0), (5, PER_WINDOW)):
            want = kmers_want(kmers, k, 1, 0, 0, cmap, n_bins, flags, top_n)
            most[k] = int(want[1][:, 0].max())
            in_force = default if slots is None else slots
            if overflows is not None:
                assert (most[k] > in_force) == overflows, (k, slots, most[k], in_force)
            out = Outputs(batch.n, top_n)
            out.check(kmer_call(big, batch, k, 1, 0, 0, flags, cmap, n_bins, top_n, out), want, ("overflow", k, slots, top_n))
    monkeypatch.delenv("GCSA2_TOP_SLOTS", raising=False)
    assert most == {3: 5008, 4: 1973, 8: 79}, most
    # values below 64 are clamped: the same result
    monkeypatch.setenv("GCSA2_TOP_SLOTS", "1")
    want = kmers_want(kmers, 8, 1, 0, 0, cmap, n_bins, 0, 5)
    out = Outputs(batch.n, 5)
    out.check(kmer_call(big, batch, 8, 1, 0, 0, 0, cmap, n_bins, 5, out), want, "clamped")


@pytest.mark.gpu
def test_shapes_across_wavefront_and_workgroup_edges(big):
    """8. 1, 63, 64 and 65 reads; empty reads, reads shorter than k, nothing found; no read at all; one read of 1000 windows of
    one k-mer beside 200 reads of one window each; reads with more than 128 counted records."""
    cpu = indexed(BIG)[1]
    reads = reads_of(BIG)
    for n in (1, 63, 64, 65):
        some = reads[:n]
        kmers = Kmers(Oracle(cpu, some))
        for k, hit_max, C, kind, flags, top_n in ((8, 0, 100003, "interleaved", 0, 5), (3, 0, 4097, "holes", PER_WINDOW, 64)):
            rec, _ = kmers.records(k, 1, hit_max)
            cmap = class_map(kind, rec.largest_bin(NODE_SHIFT) + 1, C)
            out = Outputs(n, top_n)
            out.check(kmer_call(big, DeviceReads(some), k, 1, hit_max, NODE_SHIFT, flags, cmap, C, top_n, out),
                      kmers_want(kmers, k, 1, hit_max, NODE_SHIFT, cmap, C, flags, top_n), ("reads", n, k))
    for some, k in (([b"ACGT", b"", b"ACGTACG", b"A"], 8), ([b"NNNN", b"XYZ", b"NNNN", b""], 2), ([b"", b""], 1)):
        kmers = Kmers(Oracle(cpu, some))
        cmap = class_map("interleaved", 16, 5)
        want = kmers_want(kmers, k, 1, 3, NODE_SHIFT, cmap, 5, 0, 3)
        assert want[2] == dict(dict.fromkeys(FIELDS, 0), windows=sum(window_count(len(r), k, 1) for r in some))
        assert (want[0] == np.asarray([UNKNOWN, 0], dtype=np.uint64)).all() and not want[1].any()
        out = Outputs(len(some), 3)
        out.check(kmer_call(big, DeviceReads(some), k, 1, 3, NODE_SHIFT, 0, cmap, 5, 3, out), want, ("nothing", some, k))
    out = Outputs(0, 5)
    stats = kmer_call(big, DeviceReads([]), 8, 1, 0, NODE_SHIFT, 0, class_map("interleaved", 16, 5), 5, 5, out)
    out.check(stats, (np.zeros((0, 5, 2), dtype=np.uint64), np.zeros((0, 3), dtype=np.uint64), dict.fromkeys(FIELDS, 0)), "no read")
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
    kmers = Kmers(Oracle(cpu, some))
    rec, owner = kmers.records(k, stride, 0)
    assert int((owner == 100).sum()) == 1000 and len(set(rec.run_of[owner == 100].tolist())) == 1 and rec.run_of[owner == 100][0] >= 0
    for C, kind, flags, top_n, shift in ((5, "interleaved", 0, 2, NODE_SHIFT), (0, "identity", UNAMBIGUOUS, 64, 0), (4097, "holes", PER_WINDOW, 5, NODE_SHIFT)):
        cmap, C = grid_map(kind, C, rec.largest_bin(shift) + 1)
        out = Outputs(len(some), top_n)
        out.check(kmer_call(big, DeviceReads(some), k, stride, 0, shift, flags, cmap, C, top_n, out),
                  kmers_want(kmers, k, stride, 0, shift, cmap, C, flags, top_n), ("1000 windows", C, kind))
    # reads with more than 128 counted records
    walk = reads[0]
    some = [b"N" * 9, walk[:40] * 5, walk[:33], walk[3:50] * 3]
    kmers = Kmers(Oracle(cpu, some))
    rec, owner = kmers.records(8, 1, 0)
    assert int(((owner == 1) & (rec.run_of >= 0)).sum()) > 128 and int(((owner == 3) & (rec.run_of >= 0)).sum()) > 64
    for C, kind, top_n, shift in ((5, "interleaved", 5, NODE_SHIFT), (0, "identity", 64, 0)):
        cmap, C = grid_map(kind, C, rec.largest_bin(shift) + 1)
        out = Outputs(len(some), top_n)
        out.check(kmer_call(big, DeviceReads(some), 8, 1, 0, shift, 0, cmap, C, top_n, out), kmers_want(kmers, 8, 1, 0, shift, cmap, C, 0, top_n), ("long reads", C))


def seeds_want(oracle, goff, seeds, weights, hit_max, shift, cmap, n_classes, flags, top_n):
    """The sparse restatement for a seed call: the groups whose offsets decrease or reach beyond the records own nothing."""
    ranges = np.ascontiguousarray(seeds[:, 2:4], dtype=np.uint64)
    counts = oracle.cpu.count_batch(ranges) if ranges.shape[0] else np.zeros(0, dtype=np.uint64)
    rec = Records(oracle, ranges, counts, hit_max)
    owner, index = [], []
    for g in range(len(goff) - 1):
        a, b = int(goff[g]), int(goff[g + 1])
        if a <= b <= seeds.shape[0]:
            owner += [g] * (b - a)
            index += list(range(a, b))
    want = sparse_restate(rec, np.asarray(owner, dtype=np.int64), np.asarray(index, dtype=np.int64), len(goff) - 1, weights, shift, cmap, n_classes, flags, top_n)
    return want, rec


@pytest.mark.gpu
def test_seed_form(big):
    """9. A CSR over the records of kmer_hits_device and capped_seeds_device, as they lie in device memory; weights 0, 1, 7 and
    2^40 -- some class is reached by zero-weight records only and is not voted; records owned by two groups; groups with
    decreasing offsets or offsets beyond n_seeds: the row all {UNKNOWN, 0}, the summary zero, nothing read; n_groups = 0."""
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
    capped = on_device(lambda so, se, ho, hi, m, h: big.capped_seeds_device(p, o, batch.n, 4, 0, 3, 0, 0, so.data_ptr(), se.data_ptr(), m, ho.data_ptr(), hi.data_ptr(), h),
                       big.capped_seeds_batch(flat, off, 4, 0, 3, 0, False))
    silent = 0                                                    # classes that only zero-weight records reach
    for name, (d_soff, d_seeds, soff, seeds) in (("kmer", kmer), ("capped", capped)):
        m = seeds.shape[0]
        assert m > 64 and int(soff[-1]) == m, name
        weights = np.asarray([(0, 1, 7, 1 << 40)[i % 4] for i in range(m)], dtype=np.uint64)
        d_weights = to_device(weights)
        for hit_max, shift, flags, kind, C, top_n in ((3, NODE_SHIFT, 0, "interleaved", 5, 2), (0, 0, PER_WINDOW, "identity", 0, 64),
                                                      (1, NODE_SHIFT, UNAMBIGUOUS, "holes", 100003, 5), (0, NODE_SHIFT, 0, "short", 4097, 1)):
            cmap, C = grid_map(kind, C, bins_of(BIG, shift))
            for w, d_w in ((None, None), (weights, d_weights)):
                want, rec = seeds_want(oracle, soff, seeds, w, hit_max, shift, cmap, C, flags, top_n)
                assert rec.counted > 0
                out = Outputs(batch.n, top_n)
                out.check(seed_call(big, d_soff, batch.n, d_seeds, m, d_w, hit_max, shift, flags, cmap, C, top_n, out), want, (name, hit_max, shift, flags, C, kind, w is not None))
                if w is not None:
                    plain, _ = seeds_want(oracle, soff, seeds, None, hit_max, shift, cmap, C, flags, top_n)
                    silent += int((plain[1][:, 0] > want[1][:, 0]).sum())
    assert silent > 0
    # the k-mer seeds under SKIP are the found windows: the rows, summaries and stats of the k-mer form, but for `windows`
    d_soff, d_seeds, soff, seeds = kmer
    kmers = kmers_of(BIG)
    cmap = identity_map(bins_of(BIG, 0))
    want = kmers_want(kmers, 8, 1, 3, 0, cmap, cmap.shape[0], 0, 5)
    out = Outputs(batch.n, 5)
    out.check(seed_call(big, d_soff, batch.n, d_seeds, seeds.shape[0], None, 3, 0, 0, cmap, cmap.shape[0], 5, out),
              (want[0], want[1], dict(want[2], windows=seeds.shape[0])), "k-mer seeds")
    # records owned by two groups; bad groups; empty records and one beyond the index
    n = indexed(BIG)[1].n
    odd = np.asarray([[0, 5, 1, 0, 9], [0, 5, n + 3, n + 2, 1], [0, 0, 0, U64, 0], [3, 3, 7, 6, 1], [0, 4, n - 2, n + 5, 3]], dtype=np.uint64)
    mixed = np.concatenate([odd[:2], seeds[:70], odd[2:], seeds[70:], odd])
    m = mixed.shape[0]
    weights = np.asarray([(3, 0, 1 << 40)[i % 3] for i in range(m)], dtype=np.uint64)
    goff = np.asarray([0, 40, 40, 90, 60, 80, m + 1, 100, 100, m, m, 5, U64, 0, m], dtype=np.uint64)
    bad = [g for g in range(len(goff) - 1) if not int(goff[g]) <= int(goff[g + 1]) <= m]
    assert len(bad) >= 5 and any(int(goff[g + 1]) > m for g in bad) and any(int(goff[g]) > int(goff[g + 1]) for g in bad)
    for flags, kind, C, top_n in ((0, "interleaved", 5, 3), (PER_WINDOW, "holes", 100003, 64)):
        cmap = class_map(kind, bins_of(BIG, NODE_SHIFT), C)
        want, rec = seeds_want(oracle, goff, mixed, weights, 3, NODE_SHIFT, cmap, C, flags, top_n)
        assert (want[0][bad] == np.asarray([UNKNOWN, 0], dtype=np.uint64)).all() and not want[1][bad].any() and want[2]["votes"] > 0 and want[2]["windows"] == m
        out = Outputs(len(goff) - 1, top_n)
        out.check(seed_call(big, to_device(goff), len(goff) - 1, to_device(mixed), m, to_device(weights), 3, NODE_SHIFT, flags, cmap, C, top_n, out), want, ("bad groups", flags))
    # no seeds but groups; no groups
    cmap = class_map("interleaved", 8, 5)
    goff = np.asarray([0, 0, 0, 1], dtype=np.uint64)
    want, _ = seeds_want(oracle, goff, np.zeros((0, 5), dtype=np.uint64), None, 0, NODE_SHIFT, cmap, 5, 0, 2)
    out = Outputs(3, 2)
    out.check(seed_call(big, to_device(goff), 3, None, 0, None, 0, NODE_SHIFT, 0, cmap, 5, 2, out), want, "no seeds")
    out = Outputs(0, 2)
    out.check(seed_call(big, None, 0, to_device(mixed), m, None, 0, NODE_SHIFT, 0, cmap, 5, 2, out),
              (np.zeros((0, 2, 2), dtype=np.uint64), np.zeros((0, 3), dtype=np.uint64), dict.fromkeys(FIELDS, 0)), "no groups")


@pytest.mark.gpu
def test_wide_ids(big):
    """10. Class ids in [2^31 - 2, 2^31 + 2] and 0xFFFFFFFE with n_classes = 0xFFFFFFFF; the id 0xFFFFFFFF is no class."""
    kmers = kmers_of(BIG)
    batch = DeviceReads(reads_of(BIG))
    ids = np.asarray([(1 << 31) - 2, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 31) + 2, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    for k, hit_max, shift, flags, top_n in ((8, 0, NODE_SHIFT, 0, 5), (3, 0, 0, PER_WINDOW, 64), (16, 3, NODE_SHIFT, UNAMBIGUOUS, 2)):
        n_bins = bins_of(BIG, shift)
        cmap = ids[np.arange(n_bins) % 7]
        want = kmers_want(kmers, k, 1, hit_max, shift, cmap, WIDE, flags, top_n)
        assert want[2]["unclassified"] > 0 and want[2]["votes"] > 0
        seen = set(want[0][:, :, 0].reshape(-1).tolist()) - {UNKNOWN}
        assert seen <= set(ids[:6].tolist()) and (top_n < 5 or seen == set(ids[:6].tolist())), seen
        out = Outputs(batch.n, top_n)
        out.check(kmer_call(big, batch, k, 1, hit_max, shift, flags, cmap, WIDE, top_n, out), want, ("wide ids", k))


def client_lines(top, sums, stats):
    lines = ["stats " + " ".join(str(stats[f]) for f in FIELDS)]
    lines += ["summary %d %s" % (q, " ".join(str(int(x)) for x in sums[q])) for q in range(sums.shape[0])]
    lines += ["top %d %d %d %d" % (q, j, int(top[q, j, 0]), int(top[q, j, 1])) for q in range(top.shape[0]) for j in range(top.shape[1])]
    return lines


@pytest.fixture(scope="module")
def client(engine, tmp_path_factory):
    """tests/cpp/kmer_top_classes_client.cpp, the 6000-base index as a host-view file and its reads, one per line; the client's
    map is bin % modulus over n_bins bins."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    tmp = tmp_path_factory.mktemp("kmer_top_classes")
    reads = reads_of(BIG)
    assert all(b"\n" not in r for r in reads)
    save_host_view(indexed(BIG)[0], str(tmp / "index.g2hv"))
    (tmp / "reads.txt").write_bytes(b"".join(r + b"\n" for r in reads))
    exe = compile_client(str(tmp / "kmer_top_classes_client"), os.path.join(ROOT, "tests", "cpp", "kmer_top_classes_client.cpp"))

    def run(k, stride, hit_max, shift, flags, n_bins, modulus, n_classes, top_n, **env):
        full = _run_env()
        full.pop("GCSA2_SUPPORT_CHUNK", None)
        full.pop("GCSA2_TOP_SLOTS", None)
        full.update(env)
        out = subprocess.run([exe, str(tmp / "index.g2hv"), str(tmp / "reads.txt")] + [str(int(x)) for x in (k, stride, hit_max, shift, flags, n_bins, modulus, n_classes, top_n)],
                             capture_output=True, text=True, env=full, timeout=300)
        assert out.returncode == 0, out.stderr
        return out.stdout.strip().split("\n")
    return run


@pytest.mark.gpu
def test_chunking_changes_nothing(client):
    """11. GCSA2_SUPPORT_CHUNK at 1, 64 and the default, each in a fresh process (the facade's client): identical rows,
    summaries and stats, the restatement's.  Both small budgets are below the count() of some range."""
    kmers = kmers_of(BIG)
    counts = kmers.oracle.cpu.count_batch(kmers.records(3, 1, 0)[0].ranges)
    assert int(counts.max()) > 64 and counts.shape[0] > 8
    n_bins = bins_of(BIG, NODE_SHIFT)
    C = n_bins + 7                                               # more classes than bins: the map is bin % C = the identity
    want = client_lines(*kmers_want(kmers, 3, 1, 0, NODE_SHIFT, identity_map(n_bins), C, 0, 5)[:3])
    for env in (dict(GCSA2_SUPPORT_CHUNK="1"), dict(GCSA2_SUPPORT_CHUNK="64"), dict()):
        assert client(3, 1, 0, NODE_SHIFT, 0, n_bins, C, C, 5, **env) == want, env


@pytest.mark.gpu
def test_host_form_and_facade(engine, big, client, monkeypatch):
    """12. gcsa2_kmer_top_classes_batch equals the restatement in one piece, with each output absent; the facade's client prints
    the same rows; the batch tiled to 3 MB under GCSA2_MS_PIECE_MB=1 equals the device form row for row -- distinct and values
    are then per-piece sums; offsets[0] != 0 and decreasing offsets are refused with nothing written."""
    import torch
    kmers = kmers_of(BIG)
    once = reads_of(BIG)
    flat, off = concat_patterns(once)

    def as_arrays(top, sums):
        return (np.stack([top["class_id"], top["votes"]], axis=2) if top is not None else None,
                np.stack([sums["voted"], sums["total"], sums["counted"]], axis=1) if sums is not None else None)

    for k, stride, hit_max, shift, flags, C, top_n in ((8, 1, 3, NODE_SHIFT, 0, 100003, 5), (16, 3, 0, NODE_SHIFT, PER_WINDOW | UNAMBIGUOUS, 4097, 64)):
        n_bins = bins_of(BIG, shift)
        cmap = class_map("beyond", n_bins, C)
        want = kmers_want(kmers, k, stride, hit_max, shift, cmap, C, flags, top_n)
        args = (flat, off, k, cmap, C, top_n, stride, hit_max, shift, bool(flags & PER_WINDOW), bool(flags & UNAMBIGUOUS))
        top, sums, stats = big.kmer_top_classes_batch(*args)
        assert top.dtype == engine.CLASS_VOTE and sums.dtype == engine.TOP_SUMMARY
        top, sums = as_arrays(top, sums)
        assert np.array_equal(top, want[0]) and np.array_equal(sums, want[1]) and stats == want[2], (k, "host form")
        top, sums, stats = big.kmer_top_classes_batch(*args, top=False)
        assert top is None and np.array_equal(as_arrays(None, sums)[1], want[1]) and stats == want[2]
        top, sums, stats = big.kmer_top_classes_batch(*args, summaries=False)
        assert sums is None and np.array_equal(as_arrays(top, None)[0], want[0]) and stats == want[2]
        assert client(k, stride, hit_max, shift, flags, n_bins, C + 3, C, top_n) == client_lines(*want[:3]), (k, "facade")
    # refused offsets: nothing is written
    lib = engine.load_library()
    pat = (ctypes.c_uint8 * 16)(*b"ACGTACGTACGTACGT")
    cmap8 = (ctypes.c_uint32 * 8)(0, 1, 0, 1, 0, 1, 0, 1)
    for offsets in ((1, 8, 16), (0, 9, 8)):
        c_off = (ctypes.c_uint64 * 3)(*offsets)
        top = (ctypes.c_uint64 * 8)(*([SENTINEL] * 8))
        sums = (ctypes.c_uint64 * 6)(*([SENTINEL] * 6))
        stats = (ctypes.c_uint64 * 8)(*([SENTINEL] * 8))
        rc = lib.gcsa2_kmer_top_classes_batch(big._h, pat, c_off, 2, 4, 1, 0, NODE_SHIFT, 0, ctypes.addressof(cmap8), 8, 2, 2, ctypes.addressof(top),
                                              ctypes.addressof(sums), ctypes.addressof(stats))
        assert rc == INVALID and "offsets" in lib.gcsa2_last_error().decode(), offsets
        assert list(top) == [SENTINEL] * 8 and list(sums) == [SENTINEL] * 6 and list(stats) == [SENTINEL] * 8
    # several pieces: the batch repeated until it is 3 MB of reads, in 1 MB pieces, against the device form on the same batch
    monkeypatch.setenv("GCSA2_MS_PIECE_MB", "1")
    pieced, _ = engine.open_index(indexed(BIG)[0], device=0)
    monkeypatch.delenv("GCSA2_MS_PIECE_MB")
    repeats = (3 << 20) // sum(len(r) for r in once) + 1
    tiled = once * repeats
    flat, off = concat_patterns(tiled)
    assert int(off[-1]) >= 3 << 20
    k, hit_max, C, top_n = 16, 3, 100003, 5
    cmap = class_map("interleaved", bins_of(BIG, NODE_SHIFT), C)
    want = kmers_want(kmers, k, 1, hit_max, NODE_SHIFT, cmap, C, 0, top_n)
    batch = DeviceReads(tiled)
    out = Outputs(batch.n, top_n)
    whole = kmer_call(big, batch, k, 1, hit_max, NODE_SHIFT, 0, cmap, C, top_n, out)
    tiled_want = (np.tile(want[0], (repeats, 1, 1)), np.tile(want[1], (repeats, 1)),
                  dict({f: want[2][f] * repeats for f in FIELDS}, distinct=want[2]["distinct"], values=want[2]["values"]))
    out.check(whole, tiled_want, "tiled, device form")
    top, sums, piece = pieced.kmer_top_classes_batch(flat, off, k, cmap, C, top_n, 1, hit_max, NODE_SHIFT)
    top, sums = as_arrays(top, sums)
    assert np.array_equal(top, tiled_want[0]) and np.array_equal(sums, tiled_want[1])
    assert piece["distinct"] > whole["distinct"] and piece["values"] > whole["values"]
    assert {f: piece[f] for f in FIELDS if f not in ("distinct", "values")} == {f: whole[f] for f in FIELDS if f not in ("distinct", "values")}
    pieced.close()


@pytest.mark.gpu
def test_refusals_on_a_device(engine, big):
    """13. With a real handle: every INVALID_ARGUMENT again through the binding, nothing written; n_bins == 0 is valid and
    leaves everything unclassified; an image without samples or counters is MISSING_COMPONENT, nothing written."""
    batch = DeviceReads(reads_of(BIG))
    cmap = class_map("interleaved", 2000, 5)
    untouched = (np.full((batch.n, 5, 2), SENTINEL, dtype=np.uint64), np.full((batch.n, 3), SENTINEL, dtype=np.uint64), None)
    for change in (dict(k=0), dict(stride=0), dict(shift=64), dict(flags=4), dict(C=0), dict(C=1 << 32), dict(top_n=0), dict(top_n=TOP_LIMIT + 1)):
        arg = dict(dict(k=8, stride=1, shift=NODE_SHIFT, flags=0, C=5, top_n=5), **change)
        out = Outputs(batch.n, 5)
        with pytest.raises(engine.Gcsa2Error) as err:
            kmer_call(big, batch, arg["k"], arg["stride"], 0, arg["shift"], arg["flags"], cmap, arg["C"], arg["top_n"], out)
        assert err.value.code == INVALID, change
        out.stats = False
        out.check(None, untouched, change)
    out = Outputs(batch.n, 5)
    with pytest.raises(engine.Gcsa2Error) as err:
        big.kmer_top_classes_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, 8, 1, 0, NODE_SHIFT, 0, 0, 2000, 5, 5, *out.pointers())
    assert err.value.code == INVALID
    out.stats = False
    out.check(None, untouched, "NULL map")
    kmers = kmers_of(BIG)
    want = kmers_want(kmers, 8, 1, 3, NODE_SHIFT, np.zeros(0, dtype=np.uint32), WIDE, 0, 5)
    assert want[2]["votes"] == 0 and want[2]["unclassified"] > 0 and want[2]["ambiguous"] == 0
    out = Outputs(batch.n, 5)
    out.check(kmer_call(big, batch, 8, 1, 3, NODE_SHIFT, 0, np.zeros(0, dtype=np.uint32), WIDE, 5, out), want, "n_bins == 0")
    for missing in (dict(with_samples=False), dict(with_counters=False), dict(with_samples=False, with_counters=False)):
        lame = engine.GCSA(indexed(BIG)[0], with_lcp=False, **missing)
        for form in ("kmer", "seed"):
            out = Outputs(batch.n, 5)
            with pytest.raises(engine.Gcsa2Error) as err:
                if form == "kmer":
                    kmer_call(lame, batch, 8, 1, 0, NODE_SHIFT, 0, cmap, 5, 5, out)
                else:
                    seed_call(lame, to_device(np.asarray([0, 1], dtype=np.uint64)), 1, to_device(np.asarray([[0, 4, 1, 2, 2]], dtype=np.uint64)), 1, None, 0,
                              NODE_SHIFT, 0, cmap, 5, 5, Outputs(1, 5))
            assert err.value.code == MISSING, (missing, form)
        out.stats = False
        out.check(None, untouched, missing)
        lame.close()
