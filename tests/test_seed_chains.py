"""Batched seed chains (gcsa2_seed_chains_device, gcsa2_kmer_chains_device / _batch, gcsa2_minimizer_chains_device / _batch;
kernels_chains.hpp): per read -- or group of seed records -- the top_n colinear chains of its anchors, their members from the end
backwards and {anchors, unplaced, chains}.  Every expectation is `restate`, the DEFINITION of include/gcsa2_hip_chains.h in plain
Python integers, over seeds and hits made by hand, by a generator, or located by the hits calls (which their own tests pin to
the CPU oracle); no expected chain comes from the chain kernels.  Every comparison is exact.

The census and the stream-contract rows of the new header are at the end: tests/test_stream_contract.py reads include/gcsa2_hip.h
only, and the two tables are to be merged when that file is next open for change."""
import ctypes
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import streams
from streams import Case, COMPLETE
from gcsa2_amd.hostview import concat_patterns
from test_mem_hits import SENTINEL
from test_extend import GRAPHS, BIG, indexed
from test_kmer_windows import reads_of, walks
from test_kmer_support import DeviceReads, GUARD
from test_kmer_classes import bins_of, to_device
from test_seed_clusters import identity_map, device_map, coord_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
UNKNOWN = U64
INVALID, MISSING = -1, -5
LIMIT = 1 << 32
X_LIMIT = 1 << 62
NAMES = ("gcsa2_seed_chains_device", "gcsa2_kmer_chains_device", "gcsa2_minimizer_chains_device", "gcsa2_kmer_chains_batch",
         "gcsa2_minimizer_chains_batch")
FIELDS = ("groups", "invalid_groups", "seeds", "anchors", "unplaced", "chains")     # `spilled` depends on the knob
PARAMS = ("band", "max_gap", "lookback", "match", "gap", "min_score", "top_n", "member_cap")     # gcsa2_chain_params, in order
BASE = dict(band=7, max_gap=200, lookback=16, match=3, gap=1, min_score=0, top_n=5, member_cap=3)     # what the GPU sweeps vary


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def params(**change):
    out = dict(BASE)
    out.update(change)
    assert set(out) == set(PARAMS)
    return out


# ---- the DEFINITION ------------------------------------------------------------------------------------------------------

def link(P, a, b):
    """(gain, drift) of the link a -> b of two placed anchors (x, q, l) but for the distance of their places, or None."""
    (xj, qj, lj), (xi, qi, li) = a, b
    dq, dx = (qi + li) - (qj + lj), (xi + li) - (xj + lj)
    if not (qj < qi and xj < xi and 1 <= dq <= P["max_gap"] and 1 <= dx <= P["max_gap"] and abs(dx - dq) <= P["band"]):
        return None
    return min(li, dq, dx), abs(dx - dq)


def scores(P, anchors):
    """f and pred of the sorted anchors."""
    f, pred = [], []
    for i, b in enumerate(anchors):
        best, at = P["match"] * b[2], None
        for j in range(max(0, i - P["lookback"]), i):           # ascending: `>=` lets the largest j win among equal values
            got = link(P, anchors[j], b)
            if got is not None:
                value = f[j] + P["match"] * got[0] - P["gap"] * got[1]
                if value > P["match"] * b[2] and value >= best:
                    best, at = value, j
        f.append(best)
        pred.append(at)
    return f, pred


def chains_of(P, anchors):
    """The kept chains of one group's placed anchors (any order), ranked: [(row of eight, members from the end backwards)]."""
    anchors = sorted(anchors)
    f, pred = scores(P, anchors)
    assert all(v >= 0 for v in f)
    used, kept = [None] * len(anchors), []
    for e in sorted(range(len(anchors)), key=lambda i: (-f[i], i)):
        if used[e] is not None:
            continue
        i, walked, matched, drift = e, [], 0, 0
        while True:
            used[i] = e
            walked.append(i)
            j = pred[i]
            if j is None:
                matched += anchors[i][2]
                break
            gain, d = link(P, anchors[j], anchors[i])
            matched, drift = matched + gain, drift + d
            if used[j] is not None:
                break
            i = j
        score = P["match"] * matched - P["gap"] * drift
        assert score == f[e] - (f[pred[i]] if pred[i] is not None else 0)
        if score >= P["min_score"]:
            (xe, qe, le), (xb, qb, _) = anchors[e], anchors[i]
            kept.append((score, len(walked), e, [score, len(walked), matched, drift, qb, qe + le, xb, xe + le], [anchors[a] for a in walked]))
    kept.sort(key=lambda c: (-c[0], -c[1], c[2]))
    return [(c[3], c[4]) for c in kept]


def restate(goff, seeds, hoff, hits, shift, cmap, P):
    """The DEFINITION: (top (n_groups, top_n, 8), members (n_groups, top_n, member_cap, 2) as x and position | length << 32,
    summaries (n_groups, 3), stats without `spilled`, full); full[g] = every kept chain of group g in rank order."""
    goff, seeds, hoff, hits, cmap = (np.asarray(a, dtype=np.uint64).tolist() for a in (goff, np.asarray(seeds, dtype=np.uint64).reshape(-1, 5), hoff, hits, cmap))
    n_groups, n_seeds, n_hits, top_n, cap = len(goff) - 1, len(seeds), len(hits), P["top_n"], P["member_cap"]
    top = np.zeros((n_groups, top_n, 8), dtype=np.uint64)
    members = np.zeros((n_groups, top_n, cap, 2), dtype=np.uint64)
    sums = np.zeros((n_groups, 3), dtype=np.uint64)
    stats = dict(groups=n_groups, invalid_groups=0, seeds=0, anchors=0, unplaced=0, chains=0)
    full = [[] for _ in range(n_groups)]
    for g in range(n_groups):
        first, last = goff[g], goff[g + 1]
        ok = first <= last <= n_seeds
        if ok and first < last:
            span = hoff[first:last + 1]
            ok = all(span[i] <= span[i + 1] for i in range(last - first)) and span[-1] <= n_hits
        if not ok:
            stats["invalid_groups"] += 1
            continue
        stats["seeds"] += last - first
        placed, unplaced = [], 0
        for i in range(first, last):
            q, l = seeds[i][0], seeds[i][1]
            for h in range(hoff[i], hoff[i + 1]):
                v = hits[h]
                b = v >> shift
                x = ((cmap[b] if b < len(cmap) else 0) + (v & ((1 << shift) - 1))) & U64
                if b >= len(cmap) or cmap[b] == UNKNOWN or q >= LIMIT or l >= LIMIT or q + l >= LIMIT or x >= X_LIMIT:
                    unplaced += 1
                else:
                    placed.append((x, q, l))
        full[g] = chains_of(P, placed)
        for j, (row, walked) in enumerate(full[g][:top_n]):
            top[g, j] = row
            for m, (x, q, l) in enumerate(walked[:cap]):
                members[g, j, m] = (x, q | (l << 32))
        sums[g] = (len(placed), unplaced, len(full[g]))
        stats["anchors"] += len(placed)
        stats["unplaced"] += unplaced
        stats["chains"] += len(full[g])
    return top, members, sums, stats, full


def brute_force(P, anchors):
    """Independent of `scores`: for every anchor the best score over all explicitly enumerated link sequences that end there."""
    anchors = sorted(anchors)
    n = len(anchors)
    step = {}
    for j, i in itertools.combinations(range(n), 2):
        got = link(P, anchors[j], anchors[i]) if i - j <= P["lookback"] else None
        if got is not None:
            step[(j, i)] = P["match"] * got[0] - P["gap"] * got[1]
    best = [None] * n

    def extend(path, score):
        i = path[-1]
        best[i] = score if best[i] is None else max(best[i], score)
        for k in range(i + 1, n):
            if (i, k) in step:
                extend(path + [k], score + step[(i, k)])

    for i in range(n):
        extend([i], P["match"] * anchors[i][2])
    return best


# ---- CPU -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    return binding.load_library()


def test_library_exports_the_chain_calls(lib):
    """1. The new header declares the five calls, the structures and the limits; the built library exports the calls, the binding
    mirrors all of it (the structures are 64, 64, 16, 24 and 56 bytes) and the facade has its three methods."""
    from gcsa2_amd import binding
    header = open(os.path.join(ROOT, "include", "gcsa2_hip_chains.h")).read()
    exported = ctypes.CDLL(binding.LIB_PATH)
    for name in NAMES:
        assert ("int " + name + "(") in header, name
        assert name in binding.CHAIN_EXPORTS, name
        assert hasattr(exported, name), name
    for text in ("#define GCSA2_CHAIN_TOP_LIMIT 64", "#define GCSA2_CHAIN_LOOKBACK_LIMIT 64", '#include "gcsa2_hip.h"',
                 "uint64_t band, max_gap, lookback, match, gap, min_score, top_n, member_cap;",
                 "uint64_t score, anchors, matched, drift, read_begin, read_end, ref_begin, ref_end;",
                 "typedef struct gcsa2_chain_anchor { uint64_t x; uint32_t position, length; } gcsa2_chain_anchor;",
                 "typedef struct gcsa2_chain_summary { uint64_t anchors, unplaced, chains; } gcsa2_chain_summary;",
                 "typedef struct gcsa2_chain_stats { uint64_t groups, invalid_groups, seeds, anchors, unplaced, chains, spilled; } gcsa2_chain_stats;"):
        assert text in header, text
    assert ctypes.sizeof(binding.ChainParams) == 64 and tuple(n for n, _ in binding.ChainParams._fields_) == PARAMS
    assert binding.CHAIN.itemsize == 64 and binding.CHAIN_ANCHOR.itemsize == 16 and binding.CHAIN_SUMMARY.itemsize == 24
    assert 8 * len(binding.CHAIN_STATS) == 56 and binding.CHAIN_STATS == FIELDS + ("spilled",)
    assert binding.CHAIN.names == ("score", "anchors", "matched", "drift", "read_begin", "read_end", "ref_begin", "ref_end")
    assert binding.CHAIN_ANCHOR.names == ("x", "position", "length") and binding.CHAIN_SUMMARY.names == ("anchors", "unplaced", "chains")
    assert binding.CHAIN_TOP_LIMIT == 64 and binding.CHAIN_LOOKBACK_LIMIT == 64 and binding.CHAIN_LDS_DEFAULT == 4096
    assert tuple(binding.CHAIN_DEFAULTS) == PARAMS
    for name in ("seed_chains_device", "kmer_chains_device", "minimizer_chains_device", "kmer_chains_batch", "minimizer_chains_batch"):
        assert callable(getattr(binding.GCSA, name)), name
    # one binding module per header: what gcsa2_amd/binding_chains.py calls through the library is what CHAIN_EXPORTS lists
    import inspect
    import re
    from gcsa2_amd import binding_chains
    called = set(re.findall(r"\b_?L\.(gcsa2_\w+)", inspect.getsource(binding_chains)))
    assert called == set(NAMES) | {"gcsa2_last_error"} and set(binding.CHAIN_EXPORTS) == set(NAMES) and not set(NAMES) & set(binding.EXPORTS)
    assert binding.CHAIN_EXPORTS is binding_chains.CHAIN_EXPORTS and issubclass(binding.GCSA, binding_chains.ChainCalls)
    facade = open(os.path.join(ROOT, "include", "gcsa", "gcsa.h")).read()
    for name in ("seed_chains_device", "kmer_chains_batch", "minimizer_chains_batch"):
        assert ("void " + name + "(") in facade, name
    assert '#include "../gcsa2_hip_chains.h"' in facade and "struct ChainParameters" in facade
    assert '#include "../gcsa2_hip_chains.h"' in open(os.path.join(ROOT, "include", "gcsa2_hip", "gcsa.hpp")).read()


def refusal_cases():
    """(what the message names, keyword changes, the forms it applies to): one per line of the refusal list."""
    every, seed = ("seed", "kmer_device", "kmer_batch", "mini_device", "mini_batch"), ("seed",)
    fused = every[1:]
    return [("index", dict(index=None), every), ("top_n must", dict(top_n=0), every), ("top_n must", dict(top_n=65), every),
            ("top_n must", dict(top_n=U64), every), ("shift must", dict(shift=64), every), ("n_bins must", dict(n_bins=0), every),
            ("is NULL", dict(cmap=False), every),
            ("d_group_offsets is NULL", dict(goff=False), seed), ("d_seeds is NULL", dict(seeds=False), seed),
            ("d_hit_offsets is NULL", dict(hoff=False), seed), ("d_hits is NULL", dict(hits=False), seed),
            ("or more groups", dict(n_groups=1 << 32), seed), ("or more seeds", dict(n_seeds=1 << 32), seed), ("or more hits", dict(n_hits=1 << 32), seed),
            ("k must", dict(k=0), fused), ("stride must", dict(stride=0), ("kmer_device", "kmer_batch")),
            ("w must", dict(w=0), ("mini_device", "mini_batch")), ("over-cap policy", dict(over=2), fused),
            ("params is NULL", dict(params=False), every),
            ("lookback must", dict(lookback=0), every), ("lookback must", dict(lookback=65), every),
            ("match must", dict(match=0), every), ("match must", dict(match=65537), every),
            ("gap must", dict(gap=65537), every),
            ("max_gap must", dict(max_gap=0), every), ("max_gap must", dict(max_gap=1 << 32), every),
            ("min_score must", dict(min_score=1 << 62), every),
            ("member_cap", dict(member_cap=1 << 31, top_n=2), every), ("member_cap", dict(member_cap=U64, top_n=1), every),
            ("member_cap", dict(member_cap=1, n_groups=(1 << 32) - 1, top_n=2), seed)]


def refuse(lib, form, **change):
    """One refused call on sentinel-filled host arrays (no device is touched before the refusal, so host pointers do for the
    device forms): (status, message, every output word afterwards)."""
    from gcsa2_amd.binding import ChainParams
    arg = dict(index=None, k=4, stride=1, w=2, over=0, shift=10, n_bins=8, cmap=True, goff=True, seeds=True, hoff=True, hits=True,
               n_groups=1, n_seeds=1, n_hits=2, params=True, band=3, max_gap=10, lookback=4, match=1, gap=1, min_score=0, top_n=2, member_cap=2)
    arg.update(change)
    off = (ctypes.c_uint64 * 2)(0, 8)
    goff = (ctypes.c_uint64 * 2)(0, 1)
    pat = (ctypes.c_uint8 * 8)(*b"ACGTACGT")
    seeds = (ctypes.c_uint64 * 5)(0, 4, 1, 2, 2)
    hoff = (ctypes.c_uint64 * 2)(0, 2)
    hits = (ctypes.c_uint64 * 2)(1 << 11, 2 << 11)
    cmap = (ctypes.c_uint64 * 8)(*range(8))
    top = (ctypes.c_uint64 * 16)(*([SENTINEL] * 16))
    mem = (ctypes.c_uint64 * 8)(*([SENTINEL] * 8))
    sums = (ctypes.c_uint64 * 3)(*([SENTINEL] * 3))
    stats = (ctypes.c_uint64 * 7)(*([SENTINEL] * 7))
    p = ChainParams(*(arg[name] for name in PARAMS))
    at = ctypes.addressof
    tail = (arg["shift"], at(cmap) if arg["cmap"] else None, arg["n_bins"], at(p) if arg["params"] else None, at(top), at(mem), at(sums), at(stats))
    if form == "seed":
        rc = lib.gcsa2_seed_chains_device(arg["index"], at(goff) if arg["goff"] else None, arg["n_groups"], at(seeds) if arg["seeds"] else None, arg["n_seeds"],
                                          at(hoff) if arg["hoff"] else None, at(hits) if arg["hits"] else None, arg["n_hits"], *tail, None)
    elif form == "kmer_device":
        rc = lib.gcsa2_kmer_chains_device(arg["index"], at(pat), at(off), 1, arg["k"], arg["stride"], 0, arg["over"], *tail, None)
    elif form == "kmer_batch":
        rc = lib.gcsa2_kmer_chains_batch(arg["index"], pat, off, 1, arg["k"], arg["stride"], 0, arg["over"], *tail)
    elif form == "mini_device":
        rc = lib.gcsa2_minimizer_chains_device(arg["index"], at(pat), at(off), 1, arg["k"], arg["w"], 0, 0, arg["over"], *tail, None)
    else:
        rc = lib.gcsa2_minimizer_chains_batch(arg["index"], pat, off, 1, arg["k"], arg["w"], 0, 0, arg["over"], *tail)
    return rc, lib.gcsa2_last_error().decode(), list(top) + list(mem) + list(sums) + list(stats)


def test_refusals_need_no_device(lib):
    """2. Every INVALID_ARGUMENT of the contract happens without a device -- the handle is a pointer to nothing that the checks
    never follow --, names its argument and leaves sentinel-filled rows, member rows, summaries and stats untouched.  The
    largest accepted value of every limit gets past the checks of the parameters (the refusal then names something else)."""
    nothing = ctypes.create_string_buffer(64)
    index = ctypes.addressof(nothing)
    for names, change, forms in refusal_cases():
        for form in forms:
            rc, message, words = refuse(lib, form, **dict(dict(index=index), **change))
            assert rc == INVALID and names in message, (form, change, rc, message)
            assert words == [SENTINEL] * 34, (form, change)
    for change in (dict(top_n=64), dict(lookback=64), dict(match=65536), dict(gap=65536), dict(gap=0), dict(max_gap=LIMIT - 1), dict(min_score=X_LIMIT - 1),
                   dict(band=U64), dict(member_cap=(1 << 31) - 1, top_n=2)):
        rc, message, words = refuse(lib, "seed", **dict(dict(index=index, goff=False), **change))
        assert rc == INVALID and "d_group_offsets is NULL" in message and words == [SENTINEL] * 34, (change, message)


HAND = dict(band=3, max_gap=20, lookback=3, match=2, gap=2, min_score=3, top_n=4, member_cap=2)


def hand_made():
    """One group of ten placed and six unplaced anchors (sixteen in all: the ten are the group that is chained by hand, the six
    stand beside them, one per placement rule), and an empty group.  shift = 6 (bin = value >> 6),
    coord_of_bin = [100, 1000, UNKNOWN, 2^62 - 8]; match = gap = 2, band = 3, max_gap = 20, lookback = 3, min_score = 3.
    The placed anchors in (x, q, l) order, with f and pred:
      0 j1 (100, 0, 3)    f 6            seed 0 has the hit 0 twice (an over-sample hit list): a pair of identical anchors
      1 j1'(100, 0, 3)    f 6            no link from 0: q is not smaller
      2 j2 (102, 1, 2)    f 4            dq = 0 from 0 and 1: no link
      3 i  (111, 10, 2)   f 8, pred 2    from 2: 4 + 2 2 = 8; from 1 and 0: dq 9, dx 10, drift 1: 6 + 4 - 2 = 8: a tie of three, the
                                         nearest wins
      4 a0 (1000, 20, 4)  f 8            (dx from 3 is 891 > max_gap)
      5 a1 (1005, 25, 4)  f 16, pred 4
      6 b1 (1011, 28, 2)  f 12, pred 5   dq 1, dx 4, drift 3, gain 1: 16 + 2 - 6 (from 4: 8 + 4 - 6 = 6)
      7 ec (1014, 31, 2)  f 16, pred 6   dq 3, dx 3, gain 2: 12 + 4 (from 5: 16 + 4 - 6 = 14)
      8 e' (1015, 31, 3)  f 16, pred 6   dq 4, dx 5, drift 1, gain 3: 12 + 6 - 2 (no link from 7: q is not smaller; from 5 the drift is 4)
      9 z  (1060, 50, 0)  f 0            a zero-length seed, beyond max_gap of everything
    The visit: 5, 7, 8 (f 16, by place), 6, 3, 4 (f 8, by place), 0, 1, 2, 9.
      5: a1, a0: matched 4 + 4, score 16                                     A, kept
      7: ec, b1, stops at the used a1: matched 2 + 1, drift 0 + 3, score 0   dropped (0 < 3); ec and b1 stay marked
      8: e', stops at b1, which the dropped chain marked: matched 3, drift 1, score 4 = f(e') - f(b1)   E, kept -- had the marks
         gone, or had 8 been visited before 7, the walk e', b1 would have stopped at a1 with score 0
      3: i, j2: matched 2 + 2, score 8                                       X, kept
      0, 1: j1 alone, twice: score 6                                         Y, Y
      9: score 0                                                             dropped
    Unplaced: value 128 (bin 2 is unknown), 256 (bin 4 is beyond the map), 200 (bin 3: x = 2^62), and a hit of value 0 for the
    seeds (2^32 - 1, 1) (position + length reaches 2^32), (2^32, 0) and (0, 2^32)."""
    seeds = [[0, 3], [1, 2], [10, 2], [20, 4], [25, 4], [28, 2], [31, 2], [31, 3], [50, 0], [5, 2], [LIMIT - 1, 1], [LIMIT, 0], [0, LIMIT]]
    per_seed = [[0, 0], [2], [11], [64], [69], [75], [78], [79], [124], [128, 256, 200], [0], [0], [0]]
    hits = [v for h in per_seed for v in h]
    hoff = [0] + list(np.cumsum([len(h) for h in per_seed]))
    return [0, 13, 13], [s + [0, 0, 0] for s in seeds], hoff, hits, 6, [100, 1000, UNKNOWN, X_LIMIT - 8]


def identity_holds(P, full):
    """score == match matched - gap drift for every kept chain."""
    n = 0
    for rows in full:
        for row, walked in rows:
            assert row[0] == P["match"] * row[2] - P["gap"] * row[3] and row[1] == len(walked), row
            n += 1
    return n


def test_restate_on_a_hand_made_case():
    """3. Rows, members and summary typed in by hand (the derivation is hand_made's text): a chain cut at a used anchor, a dropped
    chain whose marks stay, a tie in f decided by place, a tie between predecessors decided by the nearest, a pair of identical
    anchors, a zero-length seed and an unplaced anchor by every placement rule."""
    goff, seeds, hoff, hits, shift, cmap = hand_made()
    top, members, sums, stats, full = restate(goff, seeds, hoff, hits, shift, cmap, HAND)
    A = [16, 2, 8, 0, 20, 29, 1000, 1009]
    X = [8, 2, 4, 0, 1, 12, 102, 113]
    Y = [6, 1, 3, 0, 0, 3, 100, 103]
    E = [4, 1, 3, 1, 31, 34, 1015, 1018]
    anchor = lambda x, q, l: [x, q | (l << 32)]
    assert top[0].tolist() == [A, X, Y, Y] and top[1].tolist() == [[0] * 8] * 4
    assert members[0].tolist() == [[anchor(1005, 25, 4), anchor(1000, 20, 4)], [anchor(111, 10, 2), anchor(102, 1, 2)],
                                   [anchor(100, 0, 3), [0, 0]], [anchor(100, 0, 3), [0, 0]]]
    assert not members[1].any()
    assert sums.tolist() == [[10, 6, 5], [0, 0, 0]]
    assert stats == dict(groups=2, invalid_groups=0, seeds=13, anchors=10, unplaced=6, chains=5)
    assert [row for row, _ in full[0]] == [A, X, Y, Y, E] and full[0][4][1] == [(1015, 31, 3)] and full[1] == []
    placed = [(100, 0, 3), (100, 0, 3), (102, 1, 2), (111, 10, 2), (1000, 20, 4), (1005, 25, 4), (1011, 28, 2), (1014, 31, 2), (1015, 31, 3), (1060, 50, 0)]
    assert scores(HAND, placed) == ([6, 6, 4, 8, 8, 16, 12, 16, 16, 0], [None, None, None, 2, None, 4, 5, 6, 6, None])
    assert brute_force(HAND, placed) == [6, 6, 4, 8, 8, 16, 12, 16, 16, 0]
    # min_score 0 keeps the cut chain (score 0, two anchors: in front of z by its anchors) and the zero-length seed
    C = [0, 2, 3, 3, 28, 33, 1011, 1016]
    Z = [0, 1, 0, 0, 50, 50, 1060, 1060]
    low = dict(HAND, min_score=0, top_n=8, member_cap=1)
    top, members, sums, _, full_low = restate(goff, seeds, hoff, hits, shift, cmap, low)
    assert top[0].tolist() == [A, X, Y, Y, E, C, Z, [0] * 8] and sums[0].tolist() == [10, 6, 7]
    assert members[0, :, 0].tolist() == [anchor(1005, 25, 4), anchor(111, 10, 2), anchor(100, 0, 3), anchor(100, 0, 3), anchor(1015, 31, 3), anchor(1014, 31, 2),
                                         anchor(1060, 50, 0), [0, 0]]
    # lookback 2: j1 is out of i's reach, j1' and j2 still tie; band 0 cuts b1 off a1 (drift 3) and e' off b1 (drift 1)
    assert scores(dict(HAND, lookback=2), placed) == scores(HAND, placed)
    assert scores(dict(HAND, band=0), placed) == ([6, 6, 4, 8, 8, 16, 4, 8, 6, 0], [None, None, None, 2, None, 4, None, 6, None, None])
    assert identity_holds(HAND, full) == 5 and identity_holds(low, full_low) == 7


def random_group(rng, n):
    """n anchors close together: two loci, small positions and lengths, so that links, ties and drifts are frequent."""
    out = []
    for _ in range(n):
        q, l = int(rng.integers(0, 12)), int(rng.integers(0, 4))
        out.append((int(rng.choice([50, 58])) + q + int(rng.integers(-2, 3)), q, l))
    return out


def test_restate_equals_the_brute_force():
    """4. For random groups of at most nine anchors f(i) equals the best score over all explicitly enumerated link sequences
    that end at i, over lookbacks, bands, gap costs and gap limits; and every kept chain of every case satisfies
    score == match matched - gap drift."""
    rng = np.random.default_rng(0xC4A1)
    linked = checked = 0
    for trial in range(600):
        P = dict(band=int(rng.choice([0, 1, 3, U64])), max_gap=int(rng.choice([2, 5, 40])), lookback=int(rng.choice([1, 2, 3, 64])),
                 match=int(rng.choice([1, 2, 65536])), gap=int(rng.choice([0, 1, 5, 65536])), min_score=int(rng.choice([0, 3])), top_n=3, member_cap=2)
        anchors = random_group(rng, int(rng.integers(0, 10)))
        f, pred = scores(P, sorted(anchors))
        assert f == brute_force(P, anchors), (P, anchors)
        linked += sum(p is not None for p in pred)
        checked += identity_holds(P, [chains_of(P, anchors)])
    assert linked > 300 and checked > 300


# ---- GPU -----------------------------------------------------------------------------------------------------------------

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

    def __init__(self, n, P, top=True, members=True, summaries=True, stats=True):
        import torch
        dev = torch.device("cuda", 0)
        fill = np.uint64(SENTINEL).view(np.int64).item()
        self.n, self.P, self.stats = n, P, stats
        self.sizes = dict(top=n * P["top_n"] * 8, members=n * P["top_n"] * P["member_cap"] * 2, sums=n * 3)
        wanted = dict(top=top, members=members, sums=summaries)
        self.bufs = {key: (torch.full((size + GUARD,), fill, dtype=torch.int64, device=dev) if wanted[key] else None) for key, size in self.sizes.items()}

    def pointers(self):
        return tuple(self.bufs[key].data_ptr() if self.bufs[key] is not None else 0 for key in ("top", "members", "sums"))

    def arrays(self):
        import torch
        torch.cuda.synchronize()
        return {key: (t.cpu().numpy().view(np.uint64) if t is not None else None) for key, t in self.bufs.items()}

    def check(self, got_stats, want, what, spilled=None):
        """Rows, member rows and summaries fully overwritten with the expected, the guards untouched, every stats field equal."""
        got = self.arrays()
        for key, expected in zip(("top", "members", "sums"), want[:3]):
            if got[key] is None:
                continue
            size = self.sizes[key]
            a, b = got[key][:size], expected.reshape(-1)
            bad = np.nonzero(a != b)[0]
            assert bad.size == 0, (what, key, int(bad.size), int(bad[0]), a[bad[0]:bad[0] + 8].tolist(), b[bad[0]:bad[0] + 8].tolist())
            assert (got[key][size:] == np.uint64(SENTINEL)).all(), (what, "behind", key)
        if self.stats:
            assert {f: got_stats[f] for f in FIELDS} == want[3], (what, got_stats, want[3])
            if spilled is not None:
                assert got_stats["spilled"] == spilled, (what, got_stats, spilled)
        else:
            assert got_stats is None


class DeviceCsr:
    """A seed CSR with its hits in device memory, every buffer exactly to size (an empty one is absent)."""

    def __init__(self, goff, seeds, hoff, hits):
        self.goff, self.seeds, self.hoff, self.hits = u64(goff), u64(seeds).reshape(-1, 5), u64(hoff), u64(hits)
        self.n_groups, self.n_seeds, self.n_hits = self.goff.shape[0] - 1, self.seeds.shape[0], self.hits.shape[0]
        self.d_goff = to_device(self.goff)
        self.d_seeds = to_device(self.seeds) if self.n_seeds else None
        self.d_hoff = to_device(self.hoff) if self.hoff.shape[0] else None
        self.d_hits = to_device(self.hits) if self.n_hits else None
        self.wanted = {}

    def call(self, gpu, shift, cmap, P, out):
        d_map = device_map(cmap)
        return gpu.seed_chains_device(self.d_goff.data_ptr(), self.n_groups, self.d_seeds.data_ptr() if self.d_seeds is not None else 0, self.n_seeds,
                                      self.d_hoff.data_ptr() if self.d_hoff is not None else 0, self.d_hits.data_ptr() if self.d_hits is not None else 0,
                                      self.n_hits, shift, d_map.data_ptr(), cmap.shape[0], *out.pointers(), want_stats=out.stats, **P)

    def want(self, shift, cmap, P):
        """The restatement, computed once per parameter set and left unchanged."""
        key = (shift, id(cmap)) + tuple(P[name] for name in PARAMS)
        if key not in self.wanted:
            self.wanted[key] = restate(self.goff, self.seeds, self.hoff, self.hits, shift, cmap, P)
        return self.wanted[key]

    def run(self, gpu, shift, cmap, P, what, spilled=None, **absent):
        out = Outputs(self.n_groups, P, **absent)
        want = self.want(shift, cmap, P)
        out.check(self.call(gpu, shift, cmap, P, out), want, what, spilled)
        return want


def chained(rng, sizes, loci=3, noise=3, coords=1 << 16, repeat=0.1):
    """A seed CSR whose group g has sizes[g] anchors: seeds at rising and repeating positions with lengths 0 .. 20 (some without
    a hit), every hit on one of `loci` diagonals of [0, coords) with a little noise, some hits repeated: colinear runs with
    gaps, drifts, branches and duplicates."""
    goff, seeds, hoff, hits = [0], [], [0], []
    for size in sizes:
        base = rng.integers(2000, coords - 2000, loci)
        left, spare = size, (int(rng.integers(0, 3)) if size == 0 else 0)      # a group without an anchor has 0 .. 2 seeds
        while left > 0 or spare > 0:
            q, l = int(rng.integers(0, 400)), int(rng.integers(0, 21))
            take = min(left, int(rng.integers(0, 4)))
            spare = max(spare - 1, 0)
            seeds.append([q, l, 0, 0, 0])
            for _ in range(take):
                if hits and len(hits) > hoff[-1] and rng.random() < repeat:
                    hits.append(hits[-1])
                else:
                    hits.append(int(base[rng.integers(0, loci)]) + q + int(rng.integers(-noise, noise + 1)))
            left -= take
            hoff.append(len(hits))
        goff.append(len(seeds))
    return u64(goff), u64(seeds).reshape(-1, 5), u64(hoff), u64(hits)


SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 600]
SPILLED_AT_64 = sum(s > 64 for s in SIZES)


@pytest.fixture(scope="module")
def shapes():
    return DeviceCsr(*chained(np.random.default_rng(0xC4A2), SIZES))


def with_knob(monkeypatch, value, run):
    monkeypatch.setenv("GCSA2_CHAIN_LDS", value)
    try:
        return run()
    finally:
        monkeypatch.delenv("GCSA2_CHAIN_LDS")


SWEEP = [("base", params()), ("lookback 64", params(lookback=64)), ("lookback 1", params(lookback=1)), ("band 0", params(band=0)),
         ("band any", params(band=U64, gap=0)), ("max_gap cuts", params(max_gap=12)), ("gap 0", params(gap=0)),
         ("gap large", params(gap=65536, match=65536, band=U64)), ("min_score", params(min_score=60)),
         ("top_n 1", params(top_n=1, member_cap=5)), ("top_n 64", params(top_n=64, member_cap=1, lookback=3)), ("top_n 3, no members", params(top_n=3, member_cap=0))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [name for name, _ in SWEEP])
def test_group_sizes_and_parameters(big, shapes, monkeypatch, name):
    """5. The seed form on groups of 0, 1, 2, 63, 64, 65, 255, 256, 257 and 600 anchors in one call (shift 0, the identity map):
    rows, member rows, summaries and stats equal the restatement, the guards behind every output are intact -- at the default
    capacity (no group spills) and under GCSA2_CHAIN_LDS=64, where the groups of 65 to 600 anchors take the large path, the
    results are the same and `spilled` is 5; a knob that is no power of two is ignored.  The parameter sets: lookback 1, 16 and
    64, band 0, 7 and 2^64 - 1, a max_gap that cuts chains, gap 0 and a gap large enough for negative walk scores, min_score 0
    and above some chains, top_n 1, 3, 5 and 64 with more kept chains than top_n, member_cap 0, 1, 3 and 5 with longer chains."""
    P = dict(SWEEP)[name]
    cmap = identity_map(1 << 16)
    want = shapes.run(big, 0, cmap, P, (name, "default"), spilled=0)
    with_knob(monkeypatch, "64", lambda: shapes.run(big, 0, cmap, P, (name, "knob 64"), spilled=SPILLED_AT_64))
    if name == "base":
        with_knob(monkeypatch, "100", lambda: shapes.run(big, 0, cmap, P, (name, "knob 100"), spilled=0))
        with_knob(monkeypatch, "256", lambda: shapes.run(big, 0, cmap, P, (name, "knob 256"), spilled=2))
    top, members, sums, stats, full = want
    kept, longest = max(len(rows) for rows in full), max((row[1] for rows in full for row, _ in rows), default=0)
    assert identity_holds(P, full) == stats["chains"] > 0
    assert kept > P["top_n"] and longest > P["member_cap"], (name, kept, longest)
    if name == "base":                                            # duplicate anchors: a seed whose hit list repeats a value
        csr = shapes
        assert sum(len(set(csr.hits[int(csr.hoff[i]):int(csr.hoff[i + 1])].tolist())) < int(csr.hoff[i + 1] - csr.hoff[i]) for i in range(csr.n_seeds)) > 20
    if name == "gap large":
        assert any(f < 0 for f in walk_scores(P, shapes)), "no negative walk score"
    if name == "min_score":
        assert 0 < stats["chains"] < shapes.want(0, cmap, params())[3]["chains"]
    if name == "max_gap cuts":
        assert stats["chains"] > shapes.want(0, cmap, params())[3]["chains"]


def walk_scores(P, csr):
    """The scores of every walk of the group of 600 anchors, dropped ones included (min_score below every score)."""
    g = csr.n_groups - 1
    placed = [(int(csr.hits[h]), int(csr.seeds[i, 0]), int(csr.seeds[i, 1])) for i in range(int(csr.goff[g]), int(csr.goff[g + 1]))
              for h in range(int(csr.hoff[i]), int(csr.hoff[i + 1]))]
    anchors = sorted(placed)
    f, pred = scores(P, anchors)
    used, out = set(), []
    for e in sorted(range(len(anchors)), key=lambda i: (-f[i], i)):
        if e in used:
            continue
        i = e
        while True:
            used.add(i)
            if pred[i] is None or pred[i] in used:
                break
            i = pred[i]
        out.append(f[e] - (f[pred[i]] if pred[i] is not None else 0))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("lookback", (1, 3, 64))
def test_lookback_reaches_exactly_that_far(big, monkeypatch, lookback):
    """6. Two groups per lookback: the best (and only) predecessor of the last anchor lies exactly `lookback` places back, and
    lookback + 1 places back; the identical anchors between them link to neither (their q is larger than its, and they end
    in front of the first one's end).  One chain of two anchors in the first group, none in the second -- in LDS and in the
    large path."""
    P = params(lookback=lookback, max_gap=400, band=U64, gap=0, top_n=2, member_cap=2)
    goff, seeds, hoff, hits = [0], [], [0], []
    for distance in (lookback, lookback + 1):
        for q, l, x in [(10, 10, 1000)] + [(300, 1, 1001)] * (distance - 1) + [(30, 10, 1100)]:
            seeds.append([q, l, 0, 0, 0])
            hits.append(x)
            hoff.append(len(hits))
        goff.append(len(seeds))
    csr = DeviceCsr(goff, seeds, hoff, hits)
    cmap = identity_map(1 << 16)
    want = csr.run(big, 0, cmap, P, ("lookback", lookback), spilled=0)
    assert want[0][0, 0].tolist() == [P["match"] * 20, 2, 20, 80, 10, 40, 1000, 1110] and want[0][1, :, 1].tolist() == [1, 1]
    assert want[2].tolist() == [[lookback + 1, 0, lookback], [lookback + 2, 0, lookback + 2]]
    if lookback == 64:
        with_knob(monkeypatch, "64", lambda: csr.run(big, 0, cmap, P, ("lookback", lookback, "knob 64"), spilled=2))


@pytest.mark.gpu
def test_the_hand_made_case_and_absent_outputs(big, monkeypatch):
    """7. The hand-made group on the device (every placement rule, the map with a coordinate next to 2^62), in LDS and in the
    large path (the knob cannot go below 64: the group is repeated five times in one group of 80 anchors for that); and each of
    d_top, d_members, d_summaries and stats absent in turn, and all four: the others are the same."""
    goff, seeds, hoff, hits, shift, cmap = hand_made()
    cmap = u64(cmap)
    csr = DeviceCsr(goff, seeds, hoff, hits)
    for P in (HAND, dict(HAND, min_score=0, top_n=8, member_cap=1), dict(HAND, band=0), dict(HAND, member_cap=0)):
        csr.run(big, shift, cmap, P, ("hand-made", tuple(P.values())), spilled=0)
    for absent in (dict(top=False), dict(members=False), dict(summaries=False), dict(stats=False), dict(top=False, members=False, summaries=False, stats=False)):
        csr.run(big, shift, cmap, HAND, ("hand-made", tuple(absent)), **absent)
    more = DeviceCsr([0, 65, 65], [s for _ in range(5) for s in seeds], [0] + list(np.cumsum([b - a for _ in range(5) for a, b in zip(hoff, hoff[1:])])), hits * 5)
    want = more.run(big, shift, cmap, dict(HAND, lookback=64), "hand-made, five times", spilled=0)
    assert want[2][:, :2].tolist() == [[50, 30], [0, 0]]
    for absent in (dict(), dict(top=False), dict(members=False), dict(summaries=False), dict(stats=False), dict(top=False, members=False, summaries=False)):
        with_knob(monkeypatch, "64", lambda: more.run(big, shift, cmap, dict(HAND, lookback=64), ("five times, knob 64", tuple(absent)),
                                                      spilled=1 if absent.get("stats", True) else None, **absent))


@pytest.mark.gpu
def test_invalid_groups(big, monkeypatch):
    """8. Decreasing group offsets, offsets beyond n_seeds, hit offsets decreasing inside a group and hit offsets beyond n_hits, as
    in the cluster test: a zero row, zero member rows and a zero summary for each, the neighbouring groups unaffected,
    invalid_groups counted -- in both paths.  Every buffer is allocated exactly to size: nothing here relies on a fault."""
    rng = np.random.default_rng(0xBAD2)
    cmap = identity_map(1 << 16)
    goff, seeds, hoff, hits = chained(rng, [30, 70, 0, 110, 45, 80, 20, 300])
    n_seeds, n_hits = seeds.shape[0], hits.shape[0]
    cases = []
    g = goff.copy(); g[5], g[6] = g[6], g[5]
    cases.append(("decreasing group offsets", g, hoff, n_seeds, n_hits))
    g = goff.copy(); g[-1] = n_seeds + 7
    cases.append(("group offsets beyond n_seeds", g, hoff, n_seeds, n_hits))
    cases.append(("fewer seeds than the offsets say", goff, hoff, int(goff[6]), n_hits))
    h = hoff.copy(); at = int(goff[3]) + 1; h[at] = h[at + 1] + np.uint64(5)
    cases.append(("hit offsets decrease inside a group", goff, h, n_seeds, n_hits))
    cases.append(("hit offsets beyond n_hits", goff, hoff, n_seeds, int(hoff[int(goff[5])]) + 3))
    P = params()
    for name, g, h, ns, nh in cases:
        csr = DeviceCsr(g, seeds[:ns], h[:ns + 1] if ns < n_seeds else h, hits[:nh])
        want = csr.want(0, cmap, P)
        assert 1 <= want[3]["invalid_groups"] < 8, (name, want[3])
        csr.run(big, 0, cmap, P, (name, None))
        with_knob(monkeypatch, "64", lambda: csr.run(big, 0, cmap, P, (name, "64")))
        bad = np.nonzero([not (g[i] <= g[i + 1] <= ns) for i in range(8)])[0]
        assert not want[0][bad].any() and not want[1][bad].any() and not want[2][bad].any()


@functools.lru_cache(maxsize=None)
def small_graph():
    """The 3000-base graph: (index, reads)."""
    from workload import builder, graphs
    g = graphs.snp_graph(3000, 0x81, 0x82, snp_period=12, node_len=16)
    return builder.build(g, 16, sample_period=8, branching=4), walks(g, 0xC4A3, 60)


def fused_call(gpu, form, batch, a, b, hit_max, over, shift, d_map, n_bins, P):
    if form == "kmer":
        return lambda o: gpu.kmer_chains_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, a, b, hit_max, over, shift, d_map.data_ptr(), n_bins,
                                                *o.pointers(), want_stats=o.stats, **P)
    return lambda o: gpu.minimizer_chains_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, a, b, 0, hit_max, over, shift, d_map.data_ptr(), n_bins,
                                                 *o.pointers(), want_stats=o.stats, **P)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", ("snp3000", "snp6000"))
def test_the_law(engine, big, monkeypatch, graph):
    """9. LAW: gcsa2_kmer_chains_device and gcsa2_minimizer_chains_device equal the hits call followed by the seed form, word for
    word -- and both equal the restatement over the located seeds and hits --, on the 3000-base and the 6000-base graph, SKIP
    and SAMPLE hit lists; all outputs NULL return the same stats.  Under GCSA2_CHAIN_LDS=64 nothing but `spilled` changes.
    (No sampled hit list of these graphs repeats a value; the hit lists that do, as an over-sample list may, are those of
    `chained` in test 5 and of the hand-made group.)"""
    if graph == "snp6000":
        gpu, reads, shift = big, reads_of(BIG), 10
        n_bins = bins_of(BIG, shift)
    else:
        ix, reads = small_graph()
        gpu, _ = engine.open_index(ix, device=0)
        shift = 10
        n_bins = (int(gpu.locate_batch(np.array([[0, ix.n - 1]], dtype=np.uint64))[1].max()) >> shift) + 1
    cmap = np.arange(n_bins, dtype=np.uint64) << np.uint64(shift)
    cmap[::11] = np.uint64(UNKNOWN)
    d_map = to_device(cmap)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    P = params(band=16, top_n=4, member_cap=4, lookback=32)
    chains = 0
    for form, a, b in (("kmer", 16, 1), ("kmer", 12, 3), ("mini", 16, 5), ("mini", 12, 11)):
        for hit_max, over in ((0, 0), (8, 1)):
            what = (graph, form, a, b, hit_max, over)
            if form == "kmer":
                soff, seeds, hoff, hits = gpu.kmer_hits_batch(flat, off, a, b, hit_max, bool(over))[:4]
            else:
                soff, seeds, hoff, hits = gpu.minimizer_hits_batch(flat, off, a, b, 0, hit_max, bool(over))[:4]
            call = fused_call(gpu, form, batch, a, b, hit_max, over, shift, d_map, n_bins, P)
            csr = DeviceCsr(soff, seeds, hoff, hits)
            want = restate(soff, seeds, hoff, hits, shift, cmap, P)
            two = Outputs(batch.n, P)
            two_stats = gpu.seed_chains_device(csr.d_goff.data_ptr(), csr.n_groups, csr.d_seeds.data_ptr(), csr.n_seeds, csr.d_hoff.data_ptr(),
                                               csr.d_hits.data_ptr(), csr.n_hits, shift, d_map.data_ptr(), n_bins, *two.pointers(), **P)
            two.check(two_stats, want, what + ("hits, then the seed form",), spilled=0)
            one = Outputs(batch.n, P)
            stats = call(one)
            one.check(stats, want, what + ("fused",), spilled=0)
            assert stats == two_stats and all(np.array_equal(x, y) for x, y in zip(one.arrays().values(), two.arrays().values())), what
            none = Outputs(batch.n, P, top=False, members=False, summaries=False)
            assert call(none) == stats, what
            if over:
                small = Outputs(batch.n, P)
                small_stats = with_knob(monkeypatch, "64", lambda: call(small))
                small.check(small_stats, want, what + ("knob 64",), spilled=int((want[2][:, :2].sum(axis=1) > 64).sum()))
            chains += want[3]["chains"]
            assert identity_holds(P, want[4]) == want[3]["chains"]
    assert chains > 0
    if graph != "snp6000":
        gpu.close()


def as_words(top, members, sums):
    """The binding's structured arrays as the restatement's words."""
    n, top_n = top.shape
    return (top.view(np.uint64).reshape(n, top_n, 8), members.view(np.uint64).reshape(n, top_n, -1, 2) if members is not None else None,
            sums.view(np.uint64).reshape(n, 3))


@pytest.mark.gpu
def test_host_forms(big, monkeypatch):
    """10. The Python batch calls return structured arrays equal to the restatement over the located hits (and so to the device
    forms), and pieces of whole reads (GCSA2_MS_PIECE_MB) change no row, no member row and no stats field."""
    from gcsa2_amd import binding
    reads = reads_of(BIG)
    flat, off = concat_patterns(reads)
    shift = 11
    cmap = coord_map("holes", BIG, shift)
    P = params(top_n=3, member_cap=2)
    want_k = restate(*big.kmer_hits_batch(flat, off, 16, 3, 64, False)[:4], shift, cmap, P)
    want_m = restate(*big.minimizer_hits_batch(flat, off, 16, 5, 0, 64, False)[:4], shift, cmap, P)
    for pieces in (None, "0.002"):
        if pieces is not None:
            monkeypatch.setenv("GCSA2_MS_PIECE_MB", pieces)
        for want, got in ((want_k, big.kmer_chains_batch(flat, off, 16, cmap, stride=3, hit_max=64, shift=shift, **P)),
                          (want_m, big.minimizer_chains_batch(flat, off, 16, 5, cmap, hit_max=64, shift=shift, **P))):
            top, members, sums, stats = got
            assert top.dtype == binding.CHAIN and members.dtype == binding.CHAIN_ANCHOR and sums.dtype == binding.CHAIN_SUMMARY
            assert top.shape == (len(reads), 3) and members.shape == (len(reads), 3, 2) and sums.shape == (len(reads),)
            assert all(np.array_equal(a, b) for a, b in zip(as_words(top, members, sums), want[:3])) and {f: stats[f] for f in FIELDS} == want[3], pieces
            assert np.array_equal(members["position"].astype(np.uint64) | (members["length"].astype(np.uint64) << np.uint64(32)), want[1][..., 1])
        top, members, sums, stats = big.kmer_chains_batch(flat, off, 16, cmap, stride=3, hit_max=64, shift=shift, top=False, members=False, summaries=False, **P)
        assert top is None and members is None and sums is None and {f: stats[f] for f in FIELDS} == want_k[3]
        monkeypatch.delenv("GCSA2_MS_PIECE_MB", raising=False)
    top, members, sums, stats = big.kmer_chains_batch(flat, off, 16, cmap, stride=3, hit_max=64, shift=shift, **dict(P, member_cap=0))
    assert members is None and np.array_equal(as_words(top, None, sums)[0], want_k[0])
    top, members, sums, stats = big.kmer_chains_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 16, cmap, **P)
    assert top.shape == (0, 3) and members.shape == (0, 3, 2) and sums.shape == (0,) and set(stats.values()) == {0}
    with pytest.raises(TypeError):
        big.kmer_chains_batch(flat, off, 16, cmap, bandwidth=3)
    assert want_k[3]["chains"] > 0 and want_m[3]["chains"] > 0


def client_lines(top, members, sums, stats):
    lines = ["top %d %d %s" % (q, j, " ".join(str(int(x)) for x in top[q, j])) for q in range(top.shape[0]) for j in range(top.shape[1])]
    lines += ["member %d %d %d %d %d %d" % (q, j, m, int(members[q, j, m, 0]), int(members[q, j, m, 1]) & 0xFFFFFFFF, int(members[q, j, m, 1]) >> 32)
              for q in range(members.shape[0]) for j in range(members.shape[1]) for m in range(members.shape[2])]
    lines += ["summary %d %s" % (q, " ".join(str(int(x)) for x in sums[q])) for q in range(sums.shape[0])]
    return lines + ["stats " + " ".join(str(int(stats[f])) for f in FIELDS)]


@pytest.mark.gpu
def test_facade_client(big, tmp_path):
    """11. tests/cpp/seed_chains_client.cpp, a client of the C++ facade (kmer_chains_batch and minimizer_chains_batch), prints the
    rows, member rows, summaries and stats that the binding returns."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    reads = reads_of(BIG)
    assert all(b"\n" not in r for r in reads)
    flat, off = concat_patterns(reads)
    save_host_view(indexed(BIG)[0], str(tmp_path / "index.g2hv"))
    (tmp_path / "reads.txt").write_bytes(b"".join(r + b"\n" for r in reads))
    exe = compile_client(str(tmp_path / "seed_chains_client"), os.path.join(ROOT, "tests", "cpp", "seed_chains_client.cpp"))
    shift = 10
    cmap = coord_map("holes", BIG, shift)                          # the client makes the same map: linear, every 7th bin unknown
    P = params(top_n=3, member_cap=2)
    for form, a, b in (("kmer", 16, 3), ("mini", 16, 5)):
        if form == "kmer":
            top, members, sums, stats = big.kmer_chains_batch(flat, off, a, cmap, stride=b, hit_max=64, shift=shift, **P)
        else:
            top, members, sums, stats = big.minimizer_chains_batch(flat, off, a, b, cmap, hit_max=64, shift=shift, **P)
        out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "reads.txt"), form] +
                             [str(int(x)) for x in (a, b, 64, shift, cmap.shape[0]) + tuple(P[name] for name in PARAMS)],
                             capture_output=True, text=True, env=_run_env(), timeout=300)
        assert out.returncode == 0, out.stderr
        got = out.stdout.strip().split("\n")
        assert stats["chains"] > 0 and got == client_lines(*as_words(top, members, sums), stats), (form, got[:3])


@pytest.mark.gpu
def test_refusals_on_a_device(engine, big):
    """12. The fused forms need the samples and the counters (MISSING_COMPONENT on a find-only image, nothing written); the seed
    form needs no component and runs on the same image."""
    bare = engine.GCSA(indexed(BIG)[0], with_lcp=False, with_samples=False, with_counters=False)
    reads = reads_of(BIG)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    shift, P = 10, params(top_n=2)
    cmap = coord_map("linear", BIG, shift)
    d_map = device_map(cmap)
    for form in ("kmer", "mini"):
        out = Outputs(batch.n, P)
        with pytest.raises(engine.Gcsa2Error) as err:
            fused_call(bare, form, batch, 16, 1 if form == "kmer" else 5, 0, 0, shift, d_map, cmap.shape[0], P)(out)
        assert err.value.code == MISSING, (form, err.value)
        assert all((a == np.uint64(SENTINEL)).all() for a in out.arrays().values())
    with pytest.raises(engine.Gcsa2Error) as err:
        bare.kmer_chains_batch(flat, off, 16, cmap, **P)
    assert err.value.code == MISSING
    csr = DeviceCsr(*big.kmer_hits_batch(flat, off, 16, 1, 64, False)[:4])
    csr.run(bare, shift, cmap, P, "the seed form on a find-only image", spilled=0)
    bare.close()


# ---- the stream contract of the new header -------------------------------------------------------------------------------------
# One row per binding method (or per form of one): the C entry point it reaches and its contract class, in the header's words.
TABLE = {
    "seed_chains_device":         ("gcsa2_seed_chains_device", COMPLETE),
    "seed_chains_device-lds64":   ("gcsa2_seed_chains_device", COMPLETE),
    "kmer_chains_device":         ("gcsa2_kmer_chains_device", COMPLETE),
    "minimizer_chains_device":    ("gcsa2_minimizer_chains_device", COMPLETE),
}
BUILDERS = {}


def test_every_stream_entry_point_of_the_chain_header_has_a_row():
    """A declaration of include/gcsa2_hip_chains.h with a `void* stream` parameter (found with the regular expression of
    tests/test_stream_contract.py) has a row in TABLE; every row names a declaration and its binding method exists."""
    import test_stream_contract as contract
    from gcsa2_amd import binding
    with open(os.path.join(ROOT, "include", "gcsa2_hip_chains.h")) as f:
        declared = contract.declarations_with_a_stream(f.read())
    assert declared == {"gcsa2_seed_chains_device", "gcsa2_kmer_chains_device", "gcsa2_minimizer_chains_device"}
    assert {c for c, _ in TABLE.values()} == declared
    assert all(hasattr(binding.GCSA, row.split("-")[0]) for row in TABLE)
    assert set(TABLE) == set(BUILDERS)


def seed_chains_row(sizes, knob):
    """One group per tier.  The decoy keeps every offset and moves the hits and the seeds' positions."""
    def build(env, name):
        goff, seeds, hoff, hits = chained(np.random.default_rng(0x57E6), sizes)
        other = np.random.default_rng(0x57E7)
        decoy_seeds = seeds.copy()
        decoy_seeds[:, 0] = u64(other.integers(0, 400, seeds.shape[0]))
        decoy_hits = u64(other.integers(2000, (1 << 16) - 2000, hits.shape[0]))
        cmap = identity_map(1 << 16)
        n_groups, P = goff.shape[0] - 1, params(top_n=3, member_cap=2)
        ins = {"goff": (goff, goff), "seeds": (seeds, decoy_seeds), "hoff": (hoff, hoff), "hits": (hits, decoy_hits), "cmap": (cmap, cmap)}

        def call(p, s):
            before = os.environ.get("GCSA2_CHAIN_LDS")
            if knob is not None:
                os.environ["GCSA2_CHAIN_LDS"] = knob
            try:
                stats = env.gpu.seed_chains_device(p["goff"], n_groups, p["seeds"], seeds.shape[0], p["hoff"], p["hits"], hits.shape[0], 0, p["cmap"],
                                                   cmap.shape[0], p["top"], p["members"], p["sums"], s, **P)
            finally:
                if knob is not None:
                    if before is None:
                        del os.environ["GCSA2_CHAIN_LDS"]
                    else:
                        os.environ["GCSA2_CHAIN_LDS"] = before
            assert (stats["spilled"] > 0) == (knob is not None), stats
            return tuple(sorted(stats.items()))

        return Case(name, COMPLETE, ins, {"top": 64 * n_groups * 3, "members": 16 * n_groups * 3 * 2, "sums": 24 * n_groups}, call)
    return build


BUILDERS["seed_chains_device"] = seed_chains_row([200, 3000, 0, 30], None)            # at most 256 anchors, at most 4096
BUILDERS["seed_chains_device-lds64"] = seed_chains_row([200, 40, 70], "64")           # above GCSA2_CHAIN_LDS=64: the large path


def fused_row(form):
    def build(env, name):
        import test_stream_contract as contract
        ins, n, total = contract.reads_input()
        ins["cmap"] = contract.coord_table(env)
        P = params(top_n=2, member_cap=2)
        sizes = {"top": 64 * n * 2, "members": 16 * n * 2 * 2, "sums": 24 * n}
        if form == "kmer":
            return Case(name, COMPLETE, ins, sizes,
                        lambda p, s: contract.frozen(env.gpu.kmer_chains_device(p["pat"], p["off"], n, 8, 1, contract.HIT_MAX, contract.SAMPLE, contract.SHIFT,
                                                                                p["cmap"], env.n_bins(), p["top"], p["members"], p["sums"], s, **P)))
        return Case(name, COMPLETE, ins, sizes,
                    lambda p, s: contract.frozen(env.gpu.minimizer_chains_device(p["pat"], p["off"], n, 16, 5, 7, contract.HIT_MAX, contract.SAMPLE, contract.SHIFT,
                                                                                 p["cmap"], env.n_bins(), p["top"], p["members"], p["sums"], s, **P)))
    return build


BUILDERS["kmer_chains_device"] = fused_row("kmer")
BUILDERS["minimizer_chains_device"] = fused_row("mini")


@pytest.fixture(scope="module")
def env(engine, big):
    import test_stream_contract as contract
    return contract.Env(engine, big, None, None, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLE))
def test_entry_point_on_a_caller_stream(env, name):
    """Both probes of tests/streams.py, and nothing left on the stream when the call returns, for one row."""
    case = BUILDERS[name](env, name)
    assert case.contract == TABLE[name][1]
    ms = case.time_ms()
    print(f"stream_contract timing: {name} {ms:.3f} ms (delay {streams.DELAY_MS:.0f} ms)")
    assert ms < streams.DELAY_MS, (name, ms, "the delay no longer outlasts the call: a smaller row, or a longer delay")
    streams.probe_delayed_inputs(case)
    streams.probe_busy_null_stream(case)
