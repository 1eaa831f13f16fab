"""Batched seed clusters (gcsa2_seed_clusters_device, gcsa2_kmer_clusters_device / _batch, gcsa2_minimizer_clusters_device /
_batch; kernels_clusters.hpp): per read -- or group of seed records -- the top_n diagonal bands of its anchors and
{anchors, unplaced, clusters}.  Every expectation is `restate`, the DEFINITION of include/gcsa2_hip.h in numpy, over seeds
and hits computed by the CPU oracle (test_kmer_hits.Seeds, test_minimizer_hits.MinSeeds) or made by hand; none comes from
the GPU.  Every comparison is exact.

The parity grid: (k, (hit_max, over), shift) is the full product of the lists on every graph; each of its 24 points runs 3
of the 100 combinations of (band, top_n, map), taken in turn with a step coprime to 100 and a start that moves with the
graph, so that the 11 graphs together visit every combination several times."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from gcsa2_amd.hostview import concat_patterns
from test_mem_hits import SENTINEL
from test_extend import GRAPHS, BIG, indexed
from test_kmer_windows import reads_of
from test_kmer_support import Oracle, DeviceReads, GUARD
from test_kmer_hits import oracle_of as seeds_of, Spins
from test_minimizer_hits import minimizers_of
from test_kmer_classes import bins_of, to_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
UNKNOWN = U64
INVALID, MISSING = -1, -5
TOP_LIMIT = 64                                          # GCSA2_CLUSTER_TOP_LIMIT
LDS_DEFAULT = 4096                                      # the default of GCSA2_CLUSTER_LDS
BIAS = np.uint64(1 << 63)
LIMIT = 1 << 32
NAMES = ("gcsa2_seed_clusters_device", "gcsa2_kmer_clusters_device", "gcsa2_minimizer_clusters_device", "gcsa2_kmer_clusters_batch",
         "gcsa2_minimizer_clusters_batch")
FIELDS = ("groups", "invalid_groups", "seeds", "anchors", "unplaced", "clusters")     # `spilled` depends on the knob
GRID_K, GRID_CAP, GRID_SHIFT = (8, 16), ((0, 0), (3, 0), (3, 1), (64, 0)), (0, 10, 11)
GRID_BAND, GRID_TOP, GRID_MAPS = (0, 1, 7, 1 << 20, U64), (1, 2, 5, 64), ("linear", "holes", "short", "shuffled", "collapsed")
COMBINATIONS = len(GRID_BAND) * len(GRID_TOP) * len(GRID_MAPS)     # 100
STEP = 37                                               # coprime to 100
PARITY = dict(k=16, hit_max=64, over=0, shift=10, band=7, top_n=5)     # the batch of the coverage conditions, on BIG


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def restate(goff, seeds, hoff, hits, shift, cmap, band, top_n):
    """The DEFINITION: (top (n_groups, top_n, 8), summaries (n_groups, 3), stats without `spilled`, full) over a seed CSR with
    hits; full[g] = every cluster of group g in rank order as rows of eight."""
    goff, seeds, hoff, hits, cmap = u64(goff), u64(seeds).reshape(-1, 5), u64(hoff), u64(hits), u64(cmap)
    n_groups, n_seeds, n_hits = goff.shape[0] - 1, seeds.shape[0], hits.shape[0]
    top = np.zeros((n_groups, top_n, 8), dtype=np.uint64)
    sums = np.zeros((n_groups, 3), dtype=np.uint64)
    stats = dict(groups=n_groups, invalid_groups=0, seeds=0, anchors=0, unplaced=0, clusters=0)
    full = [np.zeros((0, 8), dtype=np.uint64)] * n_groups
    # the valid groups and their anchors (group, seed, hit)
    a_group, a_seed, a_hit = [], [], []
    for g in range(n_groups):
        first, last = int(goff[g]), int(goff[g + 1])
        ok = first <= last <= n_seeds
        if ok and first < last:
            span = hoff[first:last + 1].astype(object)
            ok = all(span[i] <= span[i + 1] for i in range(last - first)) and span[-1] <= n_hits
        if not ok:
            stats["invalid_groups"] += 1
            continue
        stats["seeds"] += last - first
        if first < last:
            sizes = np.diff(hoff[first:last + 1].astype(np.int64))
            a_seed.append(np.repeat(np.arange(first, last), sizes))
            a_hit.append(np.arange(int(hoff[first]), int(hoff[last])))
            a_group.append(np.full(int(sizes.sum()), g))
    if not a_group or sum(a.shape[0] for a in a_group) == 0:
        return top, sums, stats, full
    grp, sd, ht = (np.concatenate(a).astype(np.int64) for a in (a_group, a_seed, a_hit))
    pos, length, v = seeds[sd, 0], seeds[sd, 1], hits[ht]
    bins = v >> np.uint64(shift)
    known = bins < np.uint64(cmap.shape[0])
    coord = np.where(known, cmap[np.where(known, bins, 0).astype(np.int64)], np.uint64(UNKNOWN))
    fits = (pos < LIMIT) & (length < LIMIT) & ((pos % LIMIT) + (length % LIMIT) < LIMIT)
    placed = known & (coord != np.uint64(UNKNOWN)) & fits
    sums[:, 1] = np.bincount(grp[~placed], minlength=n_groups).astype(np.uint64)
    grp, pos, length, v, coord = grp[placed], pos[placed], length[placed], v[placed], coord[placed]
    sums[:, 0] = np.bincount(grp, minlength=n_groups).astype(np.uint64)
    stats["anchors"], stats["unplaced"] = int(sums[:, 0].sum()), int(sums[:, 1].sum())
    if grp.shape[0] == 0:
        return top, sums, stats, full
    with np.errstate(over="ignore"):
        x = coord + (v & np.uint64((1 << shift) - 1))
        key = (x - pos) ^ BIAS                            # diag in signed order
    end = pos + length
    order = np.lexsort((key, grp))
    grp, pos, end, x, key = grp[order], pos[order], end[order], x[order], key[order]
    head = np.ones(grp.shape[0], dtype=bool)
    head[1:] = (grp[1:] != grp[:-1]) | ((key[1:] - key[:-1]) > np.uint64(band))
    cid = np.cumsum(head) - 1
    starts_at = np.nonzero(head)[0]
    n_clusters = starts_at.shape[0]
    c_group = grp[starts_at]
    rec = np.zeros((n_clusters, 8), dtype=np.uint64)
    rec[:, 0] = key[starts_at] ^ BIAS
    rec[:, 1] = key[np.concatenate([starts_at[1:], [grp.shape[0]]]) - 1] ^ BIAS
    rec[:, 2] = np.bincount(cid, minlength=n_clusters)
    rec[:, 5] = np.minimum.reduceat(pos, starts_at)
    rec[:, 6] = np.maximum.reduceat(end, starts_at)
    rec[:, 7] = np.minimum.reduceat(x, starts_at)
    # starts and covered: per cluster the anchors by position, the union of [position, end) along the running end
    by = np.lexsort((pos, cid))
    c2, p2, e2 = cid[by], pos[by].astype(np.int64), end[by].astype(np.int64)
    fresh = np.ones(c2.shape[0], dtype=bool)
    fresh[1:] = (c2[1:] != c2[:-1]) | (p2[1:] != p2[:-1])
    rec[:, 3] = np.bincount(c2[fresh], minlength=n_clusters)
    reach = np.maximum.accumulate(c2 * LIMIT + e2)        # inside a cluster: the running end
    before = np.concatenate([[-1], reach[:-1]])
    reached = np.where(before // LIMIT == c2, before % LIMIT, 0)
    lo = np.maximum(p2, reached)
    rec[:, 4] = np.bincount(c2, weights=None, minlength=n_clusters) * 0
    np.add.at(rec[:, 4], c2, np.where(e2 > lo, e2 - lo, 0).astype(np.uint64))
    sums[:, 2] = np.bincount(c_group, minlength=n_groups).astype(np.uint64)
    stats["clusters"] = n_clusters
    rank = np.lexsort((key[starts_at], np.uint64(U64) - rec[:, 2], np.uint64(U64) - rec[:, 4], c_group))
    rec, c_group = rec[rank], c_group[rank]
    place = np.arange(n_clusters) - np.searchsorted(c_group, c_group, side="left")
    sel = place < top_n
    top[c_group[sel], place[sel]] = rec[sel]
    cut = np.searchsorted(c_group, np.arange(n_groups + 1), side="left")
    full = [rec[cut[g]:cut[g + 1]] for g in range(n_groups)]
    return top, sums, stats, full


def signed(d):
    return d - (1 << 64) if d >= (1 << 63) else d


def brute_force(goff, seeds, hoff, hits, shift, cmap, band, top_n):
    """Independent of `restate`: the anchors one by one in Python integers, single linkage on the diagonals by comparing every
    pair (O(n^2)), the covered bases counted with a set.  Valid groups only.  (top rows as lists, summaries)."""
    tops, sums = [], []
    for g in range(len(goff) - 1):
        anchors, unplaced = [], 0
        for i in range(int(goff[g]), int(goff[g + 1])):
            pos, length = int(seeds[i][0]), int(seeds[i][1])
            for h in range(int(hoff[i]), int(hoff[i + 1])):
                v = int(hits[h])
                b = v >> shift
                if b >= len(cmap) or int(cmap[b]) == UNKNOWN or pos >= LIMIT or length >= LIMIT or pos + length >= LIMIT:
                    unplaced += 1
                    continue
                x = (int(cmap[b]) + (v & ((1 << shift) - 1))) & U64
                anchors.append((signed((x - pos) & U64), pos, length, x))
        label = list(range(len(anchors)))

        def find(a):
            while label[a] != a:
                label[a] = label[label[a]]
                a = label[a]
            return a

        for a in range(len(anchors)):
            for b in range(a + 1, len(anchors)):
                if abs(anchors[a][0] - anchors[b][0]) <= band:
                    label[find(a)] = find(b)
        clusters = {}
        for a in range(len(anchors)):
            clusters.setdefault(find(a), []).append(anchors[a])
        rows = []
        for members in clusters.values():
            bases = set()
            for _, pos, length, _ in members:
                bases.update(range(pos, pos + length))
            diags = [m[0] for m in members]
            rows.append((len(bases), len(members), min(diags), max(diags), len({m[1] for m in members}), min(m[1] for m in members),
                         max(m[1] + m[2] for m in members), min(m[3] for m in members)))
        rows.sort(key=lambda r: (-r[0], -r[1], r[2]))
        tops.append([[r[2] & U64, r[3] & U64, r[1], r[4], r[0], r[5], r[6], r[7]] for r in rows[:top_n]] + [[0] * 8] * max(0, top_n - len(rows)))
        sums.append([len(anchors), unplaced, len(rows)])
    return tops, sums


@functools.lru_cache(maxsize=None)
def coord_map(kind, which, shift):
    """One of GRID_MAPS for a graph's bins: linear (coord = bin << shift), holes (every 7th bin unknown), short (half of the
    bins), shuffled (a seeded permutation of the bin order: wide and negative diagonals), collapsed (every bin at 0)."""
    n_bins = bins_of(which, shift)
    out = np.arange(n_bins, dtype=np.uint64) << np.uint64(shift)
    if kind == "holes":
        out[::7] = np.uint64(UNKNOWN)
    elif kind == "short":
        out = out[:max(1, n_bins // 2)].copy()
    elif kind == "shuffled":
        out = np.random.default_rng(0xC0 + which).permutation(n_bins).astype(np.uint64) << np.uint64(shift)
    elif kind == "collapsed":
        out[:] = 0
    else:
        assert kind == "linear"
    out.setflags(write=False)
    return out


def grid_points():
    return [(k, cap, shift) for k in GRID_K for cap in GRID_CAP for shift in GRID_SHIFT]


def grid_combinations(which, point):
    out = []
    for i in range(3):
        j = (STEP * (72 * which + 3 * point + i)) % COMBINATIONS
        out.append((GRID_BAND[j % 5], GRID_TOP[(j // 5) % 4], GRID_MAPS[j // 20]))
    return out


def oracle_csr(which, k, hit_max, over, stride=1):
    """(seed_offsets, seeds, hit_offsets, hits) of the graph's reads from the CPU oracle."""
    return seeds_of(which).want(k, stride, hit_max, bool(over))[:4]


# ---- CPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    return binding.load_library()


def test_library_exports_the_cluster_calls(lib):
    """1. The header declares the five calls, the three structures and GCSA2_CLUSTER_TOP_LIMIT; the built library exports the
    calls and the binding mirrors all of it."""
    from gcsa2_amd import binding
    header = open(os.path.join(ROOT, "include", "gcsa2_hip.h")).read()
    exported = ctypes.CDLL(binding.LIB_PATH)
    for name in NAMES:
        assert ("int " + name + "(") in header, name
        assert name in binding.EXPORTS, name
        assert hasattr(exported, name), name
    for text in ("#define GCSA2_CLUSTER_TOP_LIMIT 64",
                 "typedef struct gcsa2_cluster { uint64_t diag_min, diag_max, anchors, starts, covered, read_begin, read_end, ref_begin; } gcsa2_cluster;",
                 "typedef struct gcsa2_cluster_summary { uint64_t anchors, unplaced, clusters; } gcsa2_cluster_summary;",
                 "typedef struct gcsa2_cluster_stats { uint64_t groups, invalid_groups, seeds, anchors, unplaced, clusters, spilled; } gcsa2_cluster_stats;"):
        assert text in header, text
    assert binding.CLUSTER_TOP_LIMIT == TOP_LIMIT and binding.CLUSTER_LDS_DEFAULT == LDS_DEFAULT
    assert binding.CLUSTER_STATS == FIELDS + ("spilled",) and len(binding.CLUSTER) == 8 and binding.CLUSTER_SUMMARY == ("anchors", "unplaced", "clusters")
    for name in ("seed_clusters_device", "kmer_clusters_device", "minimizer_clusters_device", "kmer_clusters_batch", "minimizer_clusters_batch"):
        assert callable(getattr(binding.GCSA, name)), name
    facade = open(os.path.join(ROOT, "include", "gcsa", "gcsa.h")).read()
    for name in ("seed_clusters_device", "kmer_clusters_batch", "minimizer_clusters_batch"):
        assert ("void " + name + "(") in facade, name


def test_the_grid_covers_every_combination():
    assert len(grid_points()) == 24 and COMBINATIONS == 100
    seen = {}
    for which in range(len(GRAPHS)):
        for p in range(24):
            for c in grid_combinations(which, p):
                seen[c] = seen.get(c, 0) + 1
    assert len(seen) == COMBINATIONS and min(seen.values()) >= 4
    on_big = {c for p in range(24) for c in grid_combinations(BIG, p)}
    assert {c[0] for c in on_big} == set(GRID_BAND) and {c[1] for c in on_big} == set(GRID_TOP) and {c[2] for c in on_big} == set(GRID_MAPS)


def refusal_cases():
    """(what the message names, keyword changes, the forms it applies to) of every refusal in front of the device."""
    every, seed = ("seed", "kmer_device", "kmer_batch", "mini_device", "mini_batch"), ("seed",)
    return [("index", dict(index=None), every), ("top_n must", dict(top_n=0), every), ("top_n must", dict(top_n=TOP_LIMIT + 1), every),
            ("top_n must", dict(top_n=U64), every), ("shift must", dict(shift=64), every), ("shift must", dict(shift=U64), every),
            ("n_bins must", dict(n_bins=0), every), ("is NULL", dict(cmap=False), every),
            ("d_group_offsets is NULL", dict(goff=False), seed), ("d_seeds is NULL", dict(seeds=False), seed),
            ("d_hit_offsets is NULL", dict(hoff=False), seed), ("d_hits is NULL", dict(hits=False), seed),
            ("or more groups", dict(n_groups=1 << 32), seed), ("or more seeds", dict(n_seeds=1 << 32), seed), ("or more hits", dict(n_hits=1 << 32), seed),
            ("k must", dict(k=0), every[1:]), ("stride must", dict(stride=0), ("kmer_device", "kmer_batch")),
            ("w must", dict(w=0), ("mini_device", "mini_batch")), ("w must", dict(w=65), ("mini_device", "mini_batch")),
            ("k must", dict(k=33), ("mini_device", "mini_batch")), ("over-cap policy", dict(over=2), every[1:])]


def refuse(lib, form, **change):
    """One refused call on sentinel-filled host arrays (no device is touched before the refusal, so host pointers do for the
    device forms): (status, message, top, summaries and stats afterwards)."""
    arg = dict(index=None, k=4, stride=1, w=2, over=0, shift=10, top_n=2, n_bins=8, cmap=True, goff=True, seeds=True, hoff=True, hits=True,
               n_groups=1, n_seeds=1, n_hits=2)
    arg.update(change)
    off = (ctypes.c_uint64 * 2)(0, 8)
    goff = (ctypes.c_uint64 * 2)(0, 1)
    pat = (ctypes.c_uint8 * 8)(*b"ACGTACGT")
    seeds = (ctypes.c_uint64 * 5)(0, 4, 1, 2, 2)
    hoff = (ctypes.c_uint64 * 2)(0, 2)
    hits = (ctypes.c_uint64 * 2)(1 << 11, 2 << 11)
    cmap = (ctypes.c_uint64 * 8)(*range(8))
    top = (ctypes.c_uint64 * 16)(*([SENTINEL] * 16))
    sums = (ctypes.c_uint64 * 3)(*([SENTINEL] * 3))
    stats = (ctypes.c_uint64 * 7)(*([SENTINEL] * 7))
    at = ctypes.addressof
    pm = at(cmap) if arg["cmap"] else None
    tail = (arg["shift"], pm, arg["n_bins"], 0, arg["top_n"], at(top), at(sums), at(stats))
    if form == "seed":
        rc = lib.gcsa2_seed_clusters_device(arg["index"], at(goff) if arg["goff"] else None, arg["n_groups"], at(seeds) if arg["seeds"] else None, arg["n_seeds"],
                                            at(hoff) if arg["hoff"] else None, at(hits) if arg["hits"] else None, arg["n_hits"], *tail, None)
    elif form == "kmer_device":
        rc = lib.gcsa2_kmer_clusters_device(arg["index"], at(pat), at(off), 1, arg["k"], arg["stride"], 0, arg["over"], *tail, None)
    elif form == "kmer_batch":
        rc = lib.gcsa2_kmer_clusters_batch(arg["index"], pat, off, 1, arg["k"], arg["stride"], 0, arg["over"], *tail)
    elif form == "mini_device":
        rc = lib.gcsa2_minimizer_clusters_device(arg["index"], at(pat), at(off), 1, arg["k"], arg["w"], 0, 0, arg["over"], *tail, None)
    else:
        rc = lib.gcsa2_minimizer_clusters_batch(arg["index"], pat, off, 1, arg["k"], arg["w"], 0, 0, arg["over"], *tail)
    return rc, lib.gcsa2_last_error().decode(), list(top), list(sums), list(stats)


def test_refusals_need_no_device(lib):
    """2. Every INVALID_ARGUMENT of the contract happens without a device -- the handle is a pointer to nothing that the checks
    never follow --, names its argument and leaves sentinel-filled rows, summaries and stats untouched."""
    nothing = ctypes.create_string_buffer(64)
    index = ctypes.addressof(nothing)
    for names, change, forms in refusal_cases():
        for form in forms:
            rc, message, top, sums, stats = refuse(lib, form, **dict(dict(index=index), **change))
            assert rc == INVALID and names in message, (form, change, rc, message)
            assert top == [SENTINEL] * 16 and sums == [SENTINEL] * 3 and stats == [SENTINEL] * 7, (form, change)


def hand_made():
    """Twelve anchors of one group, shift = 4 (bin = value >> 4, sixteen values per bin), band = 3, and an empty group.
    coord_of_bin = [100, 1000, UNKNOWN, 0]; a value of bin 0 is at x = 100 + (value & 15).
      seed 0: position 10, length 5, hits 0, 3, 3     diag 90, 93, 93 (a repeated anchor)
      seed 1: position 12, length 5, hits 8, 9        diag 96 (gap of exactly band = 3 to 93: same cluster), 97
      seed 2: position 0, length 4, hit 4             diag 104 -- no: see below
      seed 3: position 50, length 0, hit 16 + 1       x = 1001, diag 951 (a zero-length seed)
      seed 4: position 7, length 3, hit 3 * 16 + 2    x = 2, diag -5 (a negative diagonal)
      seed 5: position 2^32 - 1, length 1, hit 0      unplaced: position + length reaches 2^32
      seed 6: position 3, length 2, hits 2 * 16 (an unknown bin), 4 * 16 (beyond the map)   both unplaced
      seed 7: position 20, length 10, hit 1           x = 101: diag 81
      seed 8: position 30, length 10, hit 15          x = 115: diag 85 (gap of band + 1 = 4 to 81 and 5 to 90: alone)"""
    seeds = [[10, 5, 0, 0, 0], [12, 5, 0, 0, 0], [0, 4, 0, 0, 0], [50, 0, 0, 0, 0], [7, 3, 0, 0, 0], [LIMIT - 1, 1, 0, 0, 0], [3, 2, 0, 0, 0],
             [20, 10, 0, 0, 0], [30, 10, 0, 0, 0]]
    hits = [0, 3, 3, 8, 9, 4, 17, 50, 0, 32, 64, 1, 15]
    hoff = [0, 3, 5, 6, 7, 8, 9, 11, 12, 13]
    goff = [0, 9, 9]
    cmap = [100, 1000, UNKNOWN, 0]
    return goff, seeds, hoff, hits, 4, cmap, 3


def test_restate_on_a_hand_made_case():
    """3. Rows typed in by hand.  Seed 2 (position 0, length 4, value 4) is at x = 104, diag 104: alone (the gap to 97 is 7).
    Clusters at band 3, as (diag_min .. diag_max): A = 90 .. 97 (five anchors: 90, 93, 93, 96, 97; positions 10 and 12: covered
    [10, 17) = 7, starts 2, ref_begin = 100), B = 81 (covered 10), C = 85 (covered 10), D = 104 (covered 4), E = -5 (covered 3),
    F = 951 (covered 0).  B and C tie on covered AND anchors: the smaller diag_min, B, is first.  With the band at 4 instead, B
    and C join ((81 .. 85), covered 20, two anchors) and stay in front of A."""
    goff, seeds, hoff, hits, shift, cmap, band = hand_made()
    top, sums, stats, full = restate(goff, seeds, hoff, hits, shift, cmap, band, 4)
    A = [90, 97, 5, 2, 7, 10, 17, 100]
    B = [81, 81, 1, 1, 10, 20, 30, 101]
    C = [85, 85, 1, 1, 10, 30, 40, 115]
    D = [104, 104, 1, 1, 4, 0, 4, 104]
    E = [U64 - 4, U64 - 4, 1, 1, 3, 7, 10, 2]
    F = [951, 951, 1, 1, 0, 50, 50, 1001]
    assert top[0].tolist() == [B, C, A, D]                       # top_n = 4 of six clusters
    assert top[1].tolist() == [[0] * 8] * 4
    assert sums.tolist() == [[10, 3, 6], [0, 0, 0]]
    assert stats == dict(groups=2, invalid_groups=0, seeds=9, anchors=10, unplaced=3, clusters=6)
    assert full[0].tolist() == [B, C, A, D, E, F] and full[1].shape == (0, 8)
    # equal covered, separated by anchors: a second anchor on diag 85 (seed 8 again, one more hit of value 15)
    more_hits, more_hoff = hits + [15], hoff[:-1] + [14]
    top, sums, _, _ = restate(goff, seeds, more_hoff, more_hits, shift, cmap, band, 2)
    assert top[0].tolist() == [[85, 85, 2, 1, 10, 30, 40, 115], B] and sums[0].tolist() == [11, 3, 6]
    top, _, _, _ = restate(goff, seeds, hoff, hits, shift, cmap, 4, 3)
    assert top[0].tolist() == [[81, 85, 2, 2, 20, 20, 40, 101], A, D]
    top, sums, _, _ = restate(goff, seeds, hoff, hits, shift, cmap, U64, 2)
    assert top[0].tolist() == [[U64 - 4, 951, 10, 7, 34, 0, 50, 2], [0] * 8]       # the seven placed seeds, [0, 4) + [7, 17) + [20, 40) and sums[0].tolist() == [10, 3, 1]
    want_top, want_sums = brute_force(goff, seeds, hoff, hits, shift, cmap, band, 4)
    assert want_top[0] == [B, C, A, D] and want_sums == [[10, 3, 6], [0, 0, 0]]


@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_restate_equals_the_brute_force(which):
    """4. `restate` equals an independent O(n^2) brute force (single linkage on the diagonals, covered bases counted with a set)
    on the oracle's seeds and hits of every graph, over maps, bands and shifts in turn."""
    clusters = 0
    for i, (k, hit_max, over, shift) in enumerate(((8, 3, 1, 0), (16, 64, 0, 10), (8, 64, 0, 11))):
        soff, seeds, hoff, hits = oracle_csr(which, k, hit_max, over)
        if which == BIG:                                          # the first 60 reads: the brute force is quadratic
            soff = soff[:61]
        for j, kind in enumerate(GRID_MAPS):
            band, top_n = GRID_BAND[(i + j) % 5], GRID_TOP[(i + 2 * j) % 4]
            cmap = coord_map(kind, which, shift)
            top, sums, _, _ = restate(soff, seeds, hoff, hits, shift, cmap, band, top_n)
            want_top, want_sums = brute_force(soff.tolist(), seeds.tolist(), hoff.tolist(), hits.tolist(), shift, cmap.tolist() if cmap.shape[0] < 100000 else cmap,
                                              band, top_n)
            assert top.tolist() == want_top and sums.tolist() == want_sums, (GRAPHS[which][0], k, hit_max, shift, kind, band, top_n)
            clusters += int(sums[:, 2].sum())
    assert clusters > 0


def test_the_parity_batch_covers_the_conditions():
    """5. The parity batch of the 6000-base graph holds, under the grid's maps: a group with more clusters than top_n = 5, a tie
    on covered inside a group, a group with unplaced anchors, and a group with seeds and hits but no placed anchor."""
    p = PARITY
    soff, seeds, hoff, hits = oracle_csr(BIG, p["k"], p["hit_max"], p["over"])
    more = tie = unplaced = nothing = 0
    for kind in GRID_MAPS:
        top, sums, stats, full = restate(soff, seeds, hoff, hits, p["shift"], coord_map(kind, BIG, p["shift"]), p["band"], p["top_n"])
        more += int((sums[:, 2] > p["top_n"]).sum())
        tie += sum(1 for rows in full if rows.shape[0] >= 2 and (rows[1:, 4] == rows[:-1, 4]).any())
        unplaced += int((sums[:, 1] > 0).sum())
        nothing += int(((sums[:, 0] == 0) & (sums[:, 1] > 0)).sum())
    assert more > 0 and tie > 0 and unplaced > 0 and nothing > 0, (more, tie, unplaced, nothing)


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
        self.top = torch.full((n * top_n * 8 + GUARD,), fill, dtype=torch.int64, device=dev) if top else None
        self.sums = torch.full((n * 3 + GUARD,), fill, dtype=torch.int64, device=dev) if summaries else None

    def pointers(self):
        return (self.top.data_ptr() if self.top is not None else 0, self.sums.data_ptr() if self.sums is not None else 0)

    def arrays(self):
        import torch
        torch.cuda.synchronize()
        top = self.top.cpu().numpy().view(np.uint64)[:self.n * self.top_n * 8].reshape(self.n, self.top_n, 8) if self.top is not None else None
        sums = self.sums.cpu().numpy().view(np.uint64)[:self.n * 3].reshape(self.n, 3) if self.sums is not None else None
        return top, sums

    def check(self, got_stats, want, what, spilled=None):
        """Rows and summaries fully overwritten with the expected, the guards untouched, every stats field equal."""
        import torch
        top, sums, stats = want[:3]
        torch.cuda.synchronize()
        if self.top is not None:
            got = self.top.cpu().numpy().view(np.uint64)
            n = self.n * self.top_n * 8
            rows = got[:n].reshape(self.n, self.top_n, 8)
            bad = np.nonzero((rows != top).any(axis=(1, 2)))[0]
            assert bad.size == 0, (what, "top", int(bad.size), int(bad[0]), rows[bad[0]].tolist()[:3], top[bad[0]].tolist()[:3])
            assert (got[n:] == np.uint64(SENTINEL)).all(), (what, "behind the top rows")
        if self.sums is not None:
            got = self.sums.cpu().numpy().view(np.uint64)
            rows = got[:self.n * 3].reshape(self.n, 3)
            bad = np.nonzero((rows != sums).any(axis=1))[0]
            assert bad.size == 0, (what, "summaries", int(bad.size), int(bad[0]), rows[bad[0]].tolist(), sums[bad[0]].tolist())
            assert (got[self.n * 3:] == np.uint64(SENTINEL)).all(), (what, "behind the summaries")
        if self.stats:
            assert {f: got_stats[f] for f in FIELDS} == stats, (what, got_stats, stats)
            if spilled is not None:
                assert got_stats["spilled"] == spilled, (what, got_stats, spilled)
        else:
            assert got_stats is None


DEVICE_MAPS = {}


def device_map(cmap):
    """The map in device memory, exactly n_bins words; the copies of the cached maps are kept."""
    if cmap.flags.writeable:
        return to_device(cmap)
    if id(cmap) not in DEVICE_MAPS:
        if len(DEVICE_MAPS) >= 24:
            DEVICE_MAPS.clear()
        DEVICE_MAPS[id(cmap)] = (cmap, to_device(cmap))
    return DEVICE_MAPS[id(cmap)][1]


class DeviceCsr:
    """A seed CSR with its hits in device memory, every buffer exactly to size (an empty one is absent)."""

    def __init__(self, goff, seeds, hoff, hits):
        self.goff, self.seeds, self.hoff, self.hits = u64(goff), u64(seeds).reshape(-1, 5), u64(hoff), u64(hits)
        self.n_groups, self.n_seeds, self.n_hits = self.goff.shape[0] - 1, self.seeds.shape[0], self.hits.shape[0]
        self.d_goff = to_device(self.goff)
        self.d_seeds = to_device(self.seeds) if self.n_seeds else None
        self.d_hoff = to_device(self.hoff) if self.hoff.shape[0] else None
        self.d_hits = to_device(self.hits) if self.n_hits else None

    def call(self, gpu, shift, cmap, band, top_n, out, n_seeds=None, n_hits=None):
        d_map = device_map(cmap)
        pt, ps = out.pointers()
        return gpu.seed_clusters_device(self.d_goff.data_ptr(), self.n_groups, self.d_seeds.data_ptr() if self.d_seeds is not None else 0,
                                        self.n_seeds if n_seeds is None else n_seeds, self.d_hoff.data_ptr() if self.d_hoff is not None else 0,
                                        self.d_hits.data_ptr() if self.d_hits is not None else 0, self.n_hits if n_hits is None else n_hits,
                                        shift, d_map.data_ptr(), cmap.shape[0], band, top_n, pt, ps, want_stats=out.stats)

    def want(self, shift, cmap, band, top_n):
        return restate(self.goff, self.seeds, self.hoff, self.hits, shift, cmap, band, top_n)

    def run(self, gpu, shift, cmap, band, top_n, what, spilled=None, want=None, **absent):
        out = Outputs(self.n_groups, top_n, **absent)
        want = self.want(shift, cmap, band, top_n) if want is None else want
        out.check(self.call(gpu, shift, cmap, band, top_n, out), want, what, spilled)
        return want


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_parity_with_the_oracle(engine, which):
    """6. The seed form over the oracle's seeds and hits of every graph: rows, summaries and every field of stats equal the
    restatement over the grid (see the module's text); the buffers are prefilled with a sentinel, fully overwritten and the 64
    words behind them unchanged.  On two points per graph each of d_top / d_summaries / stats is absent in turn, and all three."""
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    clusters = cut = spun = 0
    for p, (k, (hit_max, over), shift) in enumerate(grid_points()):
        try:
            csr = DeviceCsr(*oracle_csr(which, k, hit_max, over))
        except Spins:
            spun += 1
            continue
        for i, (band, top_n, kind) in enumerate(grid_combinations(which, p)):
            cmap = coord_map(kind, which, shift)
            what = (GRAPHS[which][0], k, hit_max, over, shift, band, top_n, kind)
            want = csr.run(gpu, shift, cmap, band, top_n, what, spilled=0)
            clusters += want[2]["clusters"]
            cut += int((want[1][:, 2] > top_n).sum())
            if p % 12 == 5 and i == 0:
                for absent in (dict(top=False), dict(summaries=False), dict(stats=False), dict(top=False, summaries=False, stats=False)):
                    csr.run(gpu, shift, cmap, band, top_n, what + (tuple(absent),), want=want, **absent)
    assert clusters > 0 and spun < len(grid_points()) // 2
    if which == BIG:
        assert cut > 0
    gpu.close()


def synthetic(rng, sizes, spread=6, jitter=40, coords=1 << 16):
    """A seed CSR whose group g has sizes[g] anchors: a few seeds per group (some without a hit) at random positions and
    lengths (0 among them), the hits around `spread` places of [0, coords) with a jitter, so that bands join some of them."""
    goff, seeds, hoff, hits = [0], [], [0], []
    for size in sizes:
        n_seeds = int(rng.integers(1, 9)) if size else int(rng.integers(0, 3))
        cuts = np.sort(rng.integers(0, size + 1, n_seeds - 1)) if n_seeds > 1 else np.zeros(0, dtype=np.int64)
        per = np.diff(np.concatenate([[0], cuts, [size]])) if n_seeds else np.zeros(0, dtype=np.int64)
        centres = rng.integers(1000, coords - 1000, spread)
        for s in range(n_seeds):
            seeds.append([int(rng.integers(0, 200)), int(rng.integers(0, 31)), 0, 0, 0])
            values = centres[rng.integers(0, spread, int(per[s]))] + rng.integers(0, jitter, int(per[s]))
            hits.extend(int(v) for v in values)
            hoff.append(len(hits))
        goff.append(len(seeds))
    return u64(goff), u64(seeds).reshape(-1, 5), u64(hoff), u64(hits)


@functools.lru_cache(maxsize=None)
def identity_map(n):
    out = np.arange(n, dtype=np.uint64)
    out.setflags(write=False)
    return out


@pytest.mark.gpu
def test_synthetic_shapes(big, monkeypatch):
    """7. The seed form on caller-made hits, shift 0 and the identity map: groups of 0 .. 257 anchors around the wavefront and
    workgroup sizes; groups around the capacity under GCSA2_CLUSTER_LDS=64 (rows equal to the default knob's run -- both equal
    the restatement --, stats.spilled counted); one group of the default capacity + 1; 1, 3, 64 and 1000 groups with empty
    ones at the front, in the middle and at the end; diagonals next to -2^63, 2^63 - 1 and 0; one diagonal; every anchor alone."""
    rng = np.random.default_rng(0x5EED)
    cmap = identity_map(1 << 16)
    sizes = [0, 1, 63, 64, 65, 255, 256, 257]
    csr = DeviceCsr(*synthetic(rng, sizes))
    for band, top_n in ((0, 1), (7, 5), (40, 64), (1 << 20, 2)):
        csr.run(big, 0, cmap, band, top_n, ("edges", band, top_n), spilled=0)
    # around the capacity of a small knob
    sizes = [63, 64, 65, 4 * 64 + 3, 0, 64]
    csr = DeviceCsr(*synthetic(rng, sizes))
    for band, top_n in ((0, 5), (7, 64), (40, 2)):
        want = csr.run(big, 0, cmap, band, top_n, ("default knob", band, top_n), spilled=0)
        monkeypatch.setenv("GCSA2_CLUSTER_LDS", "64")
        csr.run(big, 0, cmap, band, top_n, ("knob 64", band, top_n), spilled=2, want=want)
        monkeypatch.setenv("GCSA2_CLUSTER_LDS", "100")             # not a power of two: ignored
        csr.run(big, 0, cmap, band, top_n, ("knob 100", band, top_n), spilled=0, want=want)
        monkeypatch.delenv("GCSA2_CLUSTER_LDS")
    # the default capacity and one beyond it
    csr = DeviceCsr(*synthetic(rng, [LDS_DEFAULT, LDS_DEFAULT + 1, 5], spread=40))
    for band, top_n in ((0, 64), (3, 5), (U64, 1)):
        csr.run(big, 0, cmap, band, top_n, ("capacity", band, top_n), spilled=1)
    # many groups, empty ones at the front, in the middle and at the end
    for n in (1, 3, 64, 1000):
        sizes = rng.integers(0, 90, n)
        sizes[0] = 0 if n > 1 else 17
        sizes[n // 2] = 0 if n > 1 else sizes[n // 2]
        sizes[-1] = 0 if n > 1 else sizes[-1]
        csr = DeviceCsr(*synthetic(rng, [int(s) for s in sizes]))
        csr.run(big, 0, cmap, 7, 5, ("groups", n), spilled=0)
        if n == 1000:
            monkeypatch.setenv("GCSA2_CLUSTER_LDS", "64")
            csr.run(big, 0, cmap, 7, 5, ("groups", n, "knob 64"), spilled=int((sizes > 64).sum()))
            monkeypatch.delenv("GCSA2_CLUSTER_LDS")
    # the ends of the signed range and 0: a map of a few bins at extreme coordinates, positions 0 .. 3
    extreme = u64([0, 1, 2, (1 << 63) - 2, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, U64 - 1, U64, 3])
    extreme[8] = np.uint64(U64 - 2)                               # U64 itself is GCSA2_UNKNOWN
    seeds = u64([[p, 4, 0, 0, 0] for p in (0, 1, 2, 3)])
    hits = u64(list(range(10)) * 4)
    csr = DeviceCsr(u64([0, 4, 4, 2]), seeds, u64([0, 10, 20, 30, 40]), hits)     # the last group is invalid: it decreases
    for knob in (None, "64"):
        for band, top_n in ((0, 64), (1, 64), (2, 5), (U64 - 1, 3), (U64, 1)):
            if knob is not None:
                monkeypatch.setenv("GCSA2_CLUSTER_LDS", knob)
            csr.run(big, 0, extreme, band, top_n, ("extremes", band, top_n, knob))
            monkeypatch.delenv("GCSA2_CLUSTER_LDS", raising=False)
    # one diagonal; every anchor a cluster of its own
    n = 700
    seeds = u64([[i % 150, 20, 0, 0, 0] for i in range(n)])
    one = DeviceCsr(u64([0, n]), seeds, u64(np.arange(n + 1)), u64([5000 + i % 150 for i in range(n)]))
    want = one.run(big, 0, cmap, 0, 3, "one diagonal", spilled=0)
    assert want[1].tolist() == [[n, 0, 1]] and want[0][0, 0].tolist() == [5000, 5000, n, 150, 169, 0, 169, 5000]
    alone = DeviceCsr(u64([0, n]), seeds, u64(np.arange(n + 1)), u64([9000 + 3 * i + i % 150 for i in range(n)]))
    want = alone.run(big, 0, cmap, 2, 64, "every anchor alone", spilled=0)
    assert want[1].tolist() == [[n, 0, n]]
    for knob in ("64", "256"):
        monkeypatch.setenv("GCSA2_CLUSTER_LDS", knob)
        one.run(big, 0, cmap, 0, 3, ("one diagonal", knob), spilled=1)
        alone.run(big, 0, cmap, 2, 64, ("every anchor alone", knob), spilled=1)
        monkeypatch.delenv("GCSA2_CLUSTER_LDS")


@pytest.mark.gpu
def test_invalid_groups_and_cursors(big, monkeypatch):
    """8. Decreasing group offsets, offsets beyond n_seeds, hit offsets decreasing inside a group and hit offsets beyond n_hits:
    a zero row and summary for each, the neighbouring groups unaffected, invalid_groups counted -- in both paths.  Every
    buffer is allocated exactly to size and the expectation is the restatement: nothing here relies on a fault."""
    rng = np.random.default_rng(0xBAD)
    cmap = identity_map(1 << 16)
    goff, seeds, hoff, hits = synthetic(rng, [30, 70, 0, 110, 45, 80, 20, 300])
    n_seeds, n_hits = seeds.shape[0], hits.shape[0]
    cases = []
    g = goff.copy(); g[5], g[6] = g[6], g[5]                      # groups 4 .. 6: [a, c), [c, b) decreasing, [b, d)
    cases.append(("decreasing group offsets", g, hoff, n_seeds, n_hits, None))
    g = goff.copy(); g[-1] = n_seeds + 7
    cases.append(("group offsets beyond n_seeds", g, hoff, n_seeds, n_hits, 1))
    cases.append(("fewer seeds than the offsets say", goff, hoff, int(goff[6]), n_hits, None))
    h = hoff.copy(); at = int(goff[3]) + 1; h[at] = h[at + 1] + np.uint64(5)
    cases.append(("hit offsets decrease inside a group", goff, h, n_seeds, n_hits, None))
    cases.append(("hit offsets beyond n_hits", goff, hoff, n_seeds, int(hoff[int(goff[5])]) + 3, None))
    h = hoff.copy(); h[-1] = n_hits + 1000
    cases.append(("the last hit offset beyond n_hits", goff, h, n_seeds, n_hits, 1))
    for name, g, h, ns, nh, invalid in cases:
        # the restatement sees what the call is told: n_seeds seeds and n_hits hits
        want = restate(g, seeds[:ns], h[:ns + 1] if ns < n_seeds else h, hits[:nh], 0, cmap, 7, 5)
        assert want[2]["invalid_groups"] >= 1 and want[2]["invalid_groups"] < 8, (name, want[2])
        if invalid is not None:
            assert want[2]["invalid_groups"] == invalid, (name, want[2])
        csr = DeviceCsr(g, seeds[:ns], h[:ns + 1] if ns < n_seeds else h, hits[:nh])
        for knob in (None, "64"):
            if knob is not None:
                monkeypatch.setenv("GCSA2_CLUSTER_LDS", knob)
            csr.run(big, 0, cmap, 7, 5, (name, knob), want=want)
            monkeypatch.delenv("GCSA2_CLUSTER_LDS", raising=False)
        bad = np.nonzero([not (g[i] <= g[i + 1] <= ns) for i in range(8)])[0]
        assert (want[0][bad] == 0).all() and (want[1][bad] == 0).all()


def fused_outputs(call, n, top_n, **absent):
    out = Outputs(n, top_n, **absent)
    stats = call(out)
    return out.arrays() + (stats, out)


@pytest.mark.gpu
def test_the_law(big, monkeypatch):
    """9. LAW: gcsa2_kmer_clusters_device and gcsa2_minimizer_clusters_device equal the hits call followed by the seed form, word
    for word -- and both equal the restatement over the oracle's seeds --, on the 6000-base graph; all three outputs NULL
    return the same stats.  Under GCSA2_CLUSTER_LDS=64 nothing but `spilled` changes."""
    reads = reads_of(BIG)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    shift, band, top_n = 10, 16, 4
    cmap = coord_map("linear", BIG, shift)
    d_map = device_map(cmap)
    for form, a, b in (("kmer", 16, 1), ("kmer", 16, 3), ("mini", 16, 5), ("mini", 16, 11)):
        for hit_max, over in ((0, 0), (64, 0), (64, 1)):
            what = (form, a, b, hit_max, over)
            if form == "kmer":
                soff, seeds, hoff, hits = big.kmer_hits_batch(flat, off, a, b, hit_max, bool(over))[:4]
                oracle = seeds_of(BIG).want(a, b, hit_max, bool(over))[:4]
                call = lambda o: big.kmer_clusters_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, a, b, hit_max, over, shift,
                                                          d_map.data_ptr(), cmap.shape[0], band, top_n, *o.pointers(), want_stats=o.stats)
            else:
                soff, seeds, hoff, hits = big.minimizer_hits_batch(flat, off, a, b, 0, hit_max, bool(over))[:4]
                oracle = minimizers_of(BIG).want(a, b, 0, hit_max, bool(over))[:4]
                call = lambda o: big.minimizer_clusters_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, a, b, 0, hit_max, over, shift,
                                                               d_map.data_ptr(), cmap.shape[0], band, top_n, *o.pointers(), want_stats=o.stats)
            want = restate(*oracle, shift, cmap, band, top_n)
            csr = DeviceCsr(soff, seeds, hoff, hits)
            two = Outputs(batch.n, top_n)
            two_stats = csr.call(big, shift, cmap, band, top_n, two)
            two.check(two_stats, want, what + ("hits, then the seed form",), spilled=0)
            top, sums, stats, out = fused_outputs(call, batch.n, top_n)
            out.check(stats, want, what + ("fused",), spilled=0)
            two_top, two_sums = two.arrays()
            assert np.array_equal(top, two_top) and np.array_equal(sums, two_sums) and stats == two_stats, what
            _, _, none_stats, _ = fused_outputs(call, batch.n, top_n, top=False, summaries=False)
            assert none_stats == stats, what
            if hit_max == 64 and over == 0:
                monkeypatch.setenv("GCSA2_CLUSTER_LDS", "64")
                _, _, small, out = fused_outputs(call, batch.n, top_n)
                monkeypatch.delenv("GCSA2_CLUSTER_LDS")
                out.check(small, want, what + ("knob 64",))
                assert small["spilled"] == int((want[1][:, :2].sum(axis=1) > 64).sum()), what


@pytest.mark.gpu
def test_host_forms(engine, big, monkeypatch):
    """10. The Python batch calls agree with the restatement (and so with the device form), and pieces of whole reads
    (GCSA2_MS_PIECE_MB) change no row and no stats field."""
    reads = reads_of(BIG)
    flat, off = concat_patterns(reads)
    shift, band, top_n = 11, 7, 5
    cmap = coord_map("holes", BIG, shift)
    want_k = restate(*seeds_of(BIG).want(16, 3, 64, False)[:4], shift, cmap, band, top_n)
    want_m = restate(*minimizers_of(BIG).want(16, 5, 0, 64, False)[:4], shift, cmap, band, top_n)
    for pieces in (None, "0.002"):
        if pieces is not None:
            monkeypatch.setenv("GCSA2_MS_PIECE_MB", pieces)
        top, sums, stats = big.kmer_clusters_batch(flat, off, 16, cmap, top_n, stride=3, hit_max=64, shift=shift, band=band)
        assert np.array_equal(top, want_k[0]) and np.array_equal(sums, want_k[1]) and {f: stats[f] for f in FIELDS} == want_k[2], pieces
        top, sums, stats = big.minimizer_clusters_batch(flat, off, 16, 5, cmap, top_n, hit_max=64, shift=shift, band=band)
        assert np.array_equal(top, want_m[0]) and np.array_equal(sums, want_m[1]) and {f: stats[f] for f in FIELDS} == want_m[2], pieces
        top, sums, stats = big.kmer_clusters_batch(flat, off, 16, cmap, top_n, stride=3, hit_max=64, shift=shift, band=band, top=False, summaries=False)
        assert top is None and sums is None and {f: stats[f] for f in FIELDS} == want_k[2]
        monkeypatch.delenv("GCSA2_MS_PIECE_MB", raising=False)
    top, sums, stats = big.kmer_clusters_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 16, cmap, top_n)
    assert top.shape == (0, top_n, 8) and sums.shape == (0, 3) and set(stats.values()) == {0}


def client_lines(top, sums, stats):
    lines = ["top %d %d %s" % (q, j, " ".join(str(int(x)) for x in top[q, j])) for q in range(top.shape[0]) for j in range(top.shape[1])]
    lines += ["summary %d %s" % (q, " ".join(str(int(x)) for x in sums[q])) for q in range(sums.shape[0])]
    return lines + ["stats " + " ".join(str(int(stats[f])) for f in FIELDS)]


@pytest.mark.gpu
def test_facade_client(engine, tmp_path):
    """11. tests/cpp/seed_clusters_client.cpp, a client of the C++ facade (kmer_clusters_batch and minimizer_clusters_batch),
    prints the rows, summaries and stats that the restatement expects."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    reads = reads_of(BIG)
    assert all(b"\n" not in r for r in reads)
    save_host_view(indexed(BIG)[0], str(tmp_path / "index.g2hv"))
    (tmp_path / "reads.txt").write_bytes(b"".join(r + b"\n" for r in reads))
    exe = compile_client(str(tmp_path / "seed_clusters_client"), os.path.join(ROOT, "tests", "cpp", "seed_clusters_client.cpp"))
    shift, band, top_n = 10, 7, 5
    cmap = coord_map("holes", BIG, shift)                          # the client makes the same map: linear, every 7th bin unknown
    for form, a, b, oracle in (("kmer", 16, 3, seeds_of(BIG).want(16, 3, 64, False)), ("mini", 16, 5, minimizers_of(BIG).want(16, 5, 0, 64, False))):
        want = restate(*oracle[:4], shift, cmap, band, top_n)
        out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "reads.txt"), form] + [str(int(x)) for x in (a, b, 64, shift, cmap.shape[0], band, top_n)],
                             capture_output=True, text=True, env=_run_env(), timeout=300)
        assert out.returncode == 0, out.stderr
        got = out.stdout.strip().split("\n")
        assert got == client_lines(*want[:3]), (form, got[:3])


@pytest.mark.gpu
def test_refusals_on_a_device(engine, big):
    """12. The fused forms need the samples and the counters (MISSING_COMPONENT on a find-only image, nothing written); the seed
    form needs no component and runs on the same image."""
    Gcsa2Error = engine.Gcsa2Error
    bare = engine.GCSA(indexed(BIG)[0], with_lcp=False, with_samples=False, with_counters=False)
    reads = reads_of(BIG)
    batch = DeviceReads(reads)
    shift, band, top_n = 10, 7, 2
    cmap = coord_map("linear", BIG, shift)
    d_map = device_map(cmap)
    for form in ("kmer", "mini"):
        out = Outputs(batch.n, top_n)
        with pytest.raises(Gcsa2Error) as err:
            if form == "kmer":
                bare.kmer_clusters_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, 16, 1, 0, 0, shift, d_map.data_ptr(), cmap.shape[0],
                                          band, top_n, *out.pointers())
            else:
                bare.minimizer_clusters_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, 16, 5, 0, 0, 0, shift, d_map.data_ptr(),
                                               cmap.shape[0], band, top_n, *out.pointers())
        assert err.value.code == MISSING, (form, err.value)
        import torch
        torch.cuda.synchronize()
        assert (out.top.cpu().numpy().view(np.uint64) == np.uint64(SENTINEL)).all() and (out.sums.cpu().numpy().view(np.uint64) == np.uint64(SENTINEL)).all()
    flat, off = concat_patterns(reads)
    with pytest.raises(Gcsa2Error) as err:
        bare.kmer_clusters_batch(flat, off, 16, cmap, top_n)
    assert err.value.code == MISSING
    csr = DeviceCsr(*oracle_csr(BIG, 16, 64, 0))
    csr.run(bare, shift, cmap, band, top_n, "the seed form on a find-only image", spilled=0)
    bare.close()
