"""Batched chain pairs (gcsa2_chain_pairs_device, gcsa2_minimizer_chain_pairs_device / _batch; kernels_pairs.hpp): per pair of
interleaved mates the top_n placements of a chain of one mate and a chain of the other under a fragment model, and {candidates,
proper, kept, ignored, the best chain of each mate}.  Every expectation is `restate`, the DEFINITION of include/gcsa2_hip_pairs.h
in plain Python integers, over chain rows made by hand, by a generator, or restated (test_seed_chains.restate) from the seeds and
hits that the stranded hits call located; no expected placement comes from the pair kernel.  Every comparison is exact.

The census and the stream-contract rows of the new header are at the end, as in tests/test_seed_chains.py."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import streams
from streams import Case, COMPLETE
from gcsa2_amd.hostview import concat_patterns
from test_mem_hits import SENTINEL
from test_extend import GRAPHS, BIG, indexed
from test_kmer_windows import walks
from test_kmer_support import DeviceReads, GUARD
from test_kmer_classes import to_device
from test_seed_clusters import coord_map
import test_seed_chains as chains

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
UNKNOWN = U64
INVALID, MISSING = -1, -5
LIMIT = 1 << 32
X_LIMIT = 1 << 62
FR, RF, FF = 0, 1, 2
NAMES = ("gcsa2_chain_pairs_device", "gcsa2_minimizer_chain_pairs_device", "gcsa2_minimizer_chain_pairs_batch")
PARAMS = ("orientation", "min_fragment", "max_fragment", "mean_fragment", "unit", "cost", "min_score", "top_n")     # gcsa2_pair_params, in order
STATS = ("pairs", "candidates", "proper", "kept", "ignored", "paired", "unique", "unique_fragment_sum")           # gcsa2_pair_stats
# left and right group (m, s) of combination c = 0, 1 of every orientation
COMBINATIONS = {FR: (((0, 0), (1, 1)), ((1, 0), (0, 1))), RF: (((0, 1), (1, 0)), ((1, 1), (0, 0))), FF: (((0, 0), (1, 0)), ((1, 1), (0, 1)))}
SCORE, ANCHORS, REF_BEGIN, REF_END = 0, 1, 6, 7             # the words of a chain that are read


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def pair_params(**change):
    out = dict(orientation=FR, min_fragment=100, max_fragment=500, mean_fragment=300, unit=16, cost=1, min_score=0, top_n=4)
    out.update(change)
    assert set(out) == set(PARAMS)
    return out


# ---- the DEFINITION ------------------------------------------------------------------------------------------------------

def pair_of(groups, P):
    """One pair: `groups` = four rows (lists of eight-word lists).  (every kept candidate in rank order as (row of eight,
    deviation, (c, i, j)), candidates, proper, ignored, [mate1_score, mate1_at, mate2_score, mate2_at])."""
    valid, ignored = [], 0
    for row in groups:
        ok = []
        for e, entry in enumerate(row):
            if entry[ANCHORS] == 0:
                continue
            if entry[SCORE] < X_LIMIT and entry[REF_BEGIN] < entry[REF_END] < X_LIMIT:
                ok.append(e)
            else:
                ignored += 1
        valid.append(ok)
    candidates = proper = 0
    kept = []
    for c, ((lm, ls), (rm, rs)) in enumerate(COMBINATIONS[P["orientation"]]):
        lg, rg = 2 * lm + ls, 2 * rm + rs
        for i in valid[lg]:
            L = groups[lg][i]
            for j in valid[rg]:
                R = groups[rg][j]
                candidates += 1
                if not (L[REF_BEGIN] <= R[REF_BEGIN] and L[REF_END] <= R[REF_END]):
                    continue
                fragment = R[REF_END] - L[REF_BEGIN]
                if not P["min_fragment"] <= fragment <= P["max_fragment"]:
                    continue
                assert fragment >= 1
                proper += 1
                deviation = abs(fragment - P["mean_fragment"])
                penalty = P["cost"] * (deviation // P["unit"])
                chain_score = L[SCORE] + R[SCORE]
                score = chain_score - min(penalty, chain_score)
                assert max(penalty, chain_score, score) <= U64
                if score >= P["min_score"]:
                    kept.append(([score, fragment, penalty, chain_score, lg, i, rg, j], deviation, (c, i, j)))
    kept.sort(key=lambda k: (-k[0][0], k[1], k[2]))
    mates = []
    for m in (0, 1):
        best = [(groups[g][e][SCORE], (g << 32) | e) for g in (2 * m, 2 * m + 1) for e in valid[g]]
        mates += list(min(best, key=lambda b: (-b[0], b[1]))) if best else [0, UNKNOWN]
    return kept, candidates, proper, ignored, mates


def restate(rows, n_pairs, chain_top_n, P, cache=None):
    """The DEFINITION: (top (n_pairs, top_n, 8), summaries (n_pairs, 8), stats, full); full[p] = every kept candidate of pair p in
    rank order.  `rows`: the 4 n_pairs chain rows, (4 n_pairs, chain_top_n, 8) words.  `cache` (a dict, for one `rows`): the
    pairs already restated under the same parameters but for top_n, which only cuts the ranked list."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(4 * n_pairs, chain_top_n, 8)
    top_n = P["top_n"]
    top = np.zeros((n_pairs, top_n, 8), dtype=np.uint64)
    sums = np.zeros((n_pairs, 8), dtype=np.uint64)
    stats = dict.fromkeys(STATS, 0)
    stats["pairs"] = n_pairs
    full = []
    key = tuple(P[name] for name in PARAMS if name != "top_n")
    for p in range(n_pairs):
        if cache is not None and (p, key) in cache:
            got = cache[(p, key)]
        else:
            got = pair_of(rows[4 * p:4 * p + 4].tolist(), P)
            if cache is not None:
                cache[(p, key)] = got
        kept, candidates, proper, ignored, mates = got
        for r, (row, _, _) in enumerate(kept[:top_n]):
            top[p, r] = row
        sums[p] = [candidates, proper, len(kept), ignored] + mates
        full.append(kept)
        for name, value in (("candidates", candidates), ("proper", proper), ("kept", len(kept)), ("ignored", ignored), ("paired", int(len(kept) >= 1)),
                            ("unique", int(len(kept) == 1)), ("unique_fragment_sum", kept[0][0][1] if len(kept) == 1 else 0)):
            stats[name] += value
    return top, sums, stats, full


# ---- CPU -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    return binding.load_library()


def test_library_exports_the_pair_calls(lib):
    """1. The new header declares the three calls, the four structures and the three orientation constants; the built library
    exports the calls; PAIR_EXPORTS lists exactly them and none is in EXPORTS, CHAIN_EXPORTS or STRAND_EXPORTS; the four
    structures are 64 bytes in the binding; the facade has its two methods."""
    from gcsa2_amd import binding, binding_pairs
    header = open(os.path.join(ROOT, "include", "gcsa2_hip_pairs.h")).read()
    exported = ctypes.CDLL(binding.LIB_PATH)
    for name in NAMES:
        assert ("int " + name + "(") in header, name
        assert hasattr(exported, name), name
        assert name not in binding.EXPORTS and name not in binding.CHAIN_EXPORTS and name not in binding.STRAND_EXPORTS, name
    assert sorted(binding.PAIR_EXPORTS) == sorted(NAMES) and binding.PAIR_EXPORTS is binding_pairs.PAIR_EXPORTS
    for text in ('#include "gcsa2_hip_chains.h"', '#include "gcsa2_hip_strands.h"', "#define GCSA2_PAIR_TOP_LIMIT 64", "#define GCSA2_PAIR_FR 0",
                 "#define GCSA2_PAIR_RF 1", "#define GCSA2_PAIR_FF 2",
                 "typedef struct gcsa2_pair_params  { uint64_t orientation, min_fragment, max_fragment, mean_fragment, unit, cost, min_score, top_n; } gcsa2_pair_params;",
                 "typedef struct gcsa2_chain_pair   { uint64_t score, fragment, penalty, chain_score, left_group, left_chain, right_group, right_chain; } gcsa2_chain_pair;",
                 "typedef struct gcsa2_pair_summary { uint64_t candidates, proper, kept, ignored, mate1_score, mate1_at, mate2_score, mate2_at; } gcsa2_pair_summary;",
                 "typedef struct gcsa2_pair_stats   { uint64_t pairs, candidates, proper, kept, ignored, paired, unique, unique_fragment_sum; } gcsa2_pair_stats;"):
        assert text in header, text
    assert ctypes.sizeof(binding.PairParams) == 64 and tuple(n for n, _ in binding.PairParams._fields_) == PARAMS
    assert binding.CHAIN_PAIR.itemsize == 64 and binding.PAIR_SUMMARY.itemsize == 64 and 8 * len(binding.PAIR_STATS) == 64
    assert binding.CHAIN_PAIR.names == ("score", "fragment", "penalty", "chain_score", "left_group", "left_chain", "right_group", "right_chain")
    assert binding.PAIR_SUMMARY.names == ("candidates", "proper", "kept", "ignored", "mate1_score", "mate1_at", "mate2_score", "mate2_at")
    assert binding.PAIR_STATS == STATS and (binding.PAIR_FR, binding.PAIR_RF, binding.PAIR_FF, binding.PAIR_TOP_LIMIT) == (0, 1, 2, 64)
    assert binding.PAIR_DEFAULTS == dict(orientation=0, min_fragment=0, max_fragment=1000, mean_fragment=400, unit=16, cost=1, min_score=0, top_n=2)
    assert tuple(binding.PAIR_DEFAULTS) == PARAMS
    with pytest.raises(TypeError):
        binding.pair_params(fragment=3)
    for name in ("chain_pairs_device", "minimizer_chain_pairs_device", "minimizer_chain_pairs_batch"):
        assert callable(getattr(binding.GCSA, name)), name
    import inspect
    import re
    called = set(re.findall(r"\b_?L\.(gcsa2_\w+)", inspect.getsource(binding_pairs)))
    assert called == set(NAMES) | {"gcsa2_last_error"} and issubclass(binding.GCSA, binding_pairs.PairCalls)
    facade = open(os.path.join(ROOT, "include", "gcsa", "gcsa.h")).read()
    for name in ("chain_pairs_device", "minimizer_chain_pairs_batch"):
        assert ("void " + name + "(") in facade, name
    assert '#include "../gcsa2_hip_pairs.h"' in facade and "struct PairParameters" in facade
    assert '#include "../gcsa2_hip_pairs.h"' in open(os.path.join(ROOT, "include", "gcsa2_hip", "gcsa.hpp")).read()
    assert '#include "kernels_pairs.hpp"' in open(os.path.join(ROOT, "gcsa2_amd", "csrc", "gcsa2_hip.hip")).read()


FORMS = ("seed", "fused_device", "fused_batch")


def refusal_cases():
    """(what the message names, keyword changes, the forms it applies to): one per refusal of the header, and the odd batch."""
    seed, fused = ("seed",), FORMS[1:]
    return [("index", dict(index=None), FORMS), ("params is NULL", dict(params=False), FORMS),
            ("orientation must", dict(orientation=3), FORMS), ("orientation must", dict(orientation=U64), FORMS),
            ("top_n must", dict(top_n=0), FORMS), ("top_n must", dict(top_n=65), FORMS),
            ("chain_top_n must", dict(chain_top_n=0), seed), ("chain_top_n must", dict(chain_top_n=65), seed),
            ("top_n must", dict(chain_top_n=0), fused), ("top_n must", dict(chain_top_n=65), fused),
            ("min_fragment exceeds", dict(min_fragment=11, max_fragment=10), FORMS),
            ("max_fragment must", dict(max_fragment=LIMIT), FORMS), ("mean_fragment must", dict(mean_fragment=LIMIT), FORMS),
            ("unit must", dict(unit=0), FORMS), ("cost must", dict(cost=65537), FORMS), ("min_score must", dict(min_score=X_LIMIT), FORMS),
            ("or more pairs", dict(n_pairs=1 << 30), seed), ("d_chains is NULL", dict(chains=False), seed),
            ("n_patterns must be even", dict(n_patterns=1), fused), ("n_patterns must be even", dict(n_patterns=3), fused),
            ("params is NULL", dict(chain_params=False), fused), ("lookback must", dict(lookback=0), fused), ("k must", dict(k=0), fused),
            ("w must", dict(w=0), fused), ("is NULL", dict(cmap=False), fused)]


WORDS = 32 + 8 + 8 + 64 + 16 + 12 + 7                       # every output word of `refuse`


def refuse(lib, form, **change):
    """One refused call on sentinel-filled host arrays (no device is touched before the refusal, so host pointers do for the
    device forms): (status, message, every output word afterwards)."""
    from gcsa2_amd.binding import ChainParams, PairParams
    arg = dict(index=None, params=True, chain_params=True, chains=True, cmap=True, n_pairs=1, n_patterns=2, chain_top_n=2, k=4, w=2, lookback=4,
               orientation=FR, min_fragment=0, max_fragment=100, mean_fragment=50, unit=4, cost=1, min_score=0, top_n=4)
    arg.update(change)
    at = ctypes.addressof
    fill = lambda n: (ctypes.c_uint64 * n)(*([SENTINEL] * n))
    off = (ctypes.c_uint64 * 4)(0, 8, 16, 24)
    pat = (ctypes.c_uint8 * 24)(*(b"ACGTACGT" * 3))
    cmap = (ctypes.c_uint64 * 8)(*range(8))
    rows = (ctypes.c_uint64 * 64)(*([1] * 64))
    top, sums, stats = fill(32), fill(8), fill(8)
    chain_rows, members, chain_sums, chain_stats = fill(64), fill(16), fill(12), fill(7)
    pp = PairParams(*(arg[name] for name in PARAMS))
    cp = ChainParams(3, 10, arg["lookback"], 1, 1, 0, arg["chain_top_n"], 1)
    p = at(pp) if arg["params"] else None
    if form == "seed":
        rc = lib.gcsa2_chain_pairs_device(arg["index"], at(rows) if arg["chains"] else None, arg["n_pairs"], arg["chain_top_n"], p, at(top), at(sums), at(stats), None)
    else:
        tail = (10, at(cmap) if arg["cmap"] else None, 8, at(cp) if arg["chain_params"] else None, p, at(chain_rows), at(members), at(chain_sums), at(top), at(sums),
                at(chain_stats), at(stats))
        if form == "fused_device":
            rc = lib.gcsa2_minimizer_chain_pairs_device(arg["index"], at(pat), at(off), arg["n_patterns"], arg["k"], arg["w"], 0, 0, 0, *tail, None)
        else:
            rc = lib.gcsa2_minimizer_chain_pairs_batch(arg["index"], pat, off, arg["n_patterns"], arg["k"], arg["w"], 0, 0, 0, *tail)
    words = list(top) + list(sums) + list(stats) + list(chain_rows) + list(members) + list(chain_sums) + list(chain_stats)
    return rc, lib.gcsa2_last_error().decode(), words


def test_refusals_need_no_device(lib):
    """2. Every INVALID_ARGUMENT of the header, and the odd n_patterns of the fused forms, happens without a device -- the handle is
    a pointer to nothing that the checks never follow --, names its argument and leaves sentinel-filled outputs and stats
    untouched.  The largest accepted value of every limit gets past the checks of the parameters (the refusal then names
    something else)."""
    nothing = ctypes.create_string_buffer(64)
    index = ctypes.addressof(nothing)
    for names, change, forms in refusal_cases():
        for form in forms:
            rc, message, words = refuse(lib, form, **dict(dict(index=index), **change))
            assert rc == INVALID and names in message, (form, change, rc, message)
            assert words == [SENTINEL] * WORDS, (form, change)
    for change in (dict(orientation=2), dict(top_n=64), dict(chain_top_n=64), dict(min_fragment=10, max_fragment=10), dict(max_fragment=LIMIT - 1),
                   dict(mean_fragment=LIMIT - 1), dict(unit=U64), dict(cost=65536), dict(cost=0), dict(min_score=X_LIMIT - 1), dict(n_pairs=(1 << 30) - 1)):
        rc, message, words = refuse(lib, "seed", **dict(dict(index=index, chains=False), **change))
        assert rc == INVALID and "d_chains is NULL" in message and words == [SENTINEL] * WORDS, (change, message)
    # no pair is no work: zero stats, nothing else written, whatever the row pointer
    rc, message, words = refuse(lib, "seed", index=index, n_pairs=0, chains=False)
    assert rc == 0 and words[:40] == [SENTINEL] * 40 and words[40:48] == [0] * 8 and words[48:] == [SENTINEL] * (WORDS - 48)


def chain(score, begin, end, anchors=1, junk=0):
    """A chain row entry with the four words that are read, and `junk` in the four that are not."""
    return [score, anchors, junk, junk, junk, junk, begin, end]


EMPTY = chain(0, 0, 0, anchors=0)
HAND = dict(orientation=FR, min_fragment=100, max_fragment=200, mean_fragment=150, unit=10, cost=5, min_score=0, top_n=8)


def hand_made():
    """Three pairs, chain_top_n = 5, FR with fragments 100 .. 200 around 150, unit 10, cost 5: penalty = 5 (|fragment - 150| / 10).
    Pair 0.  Group 0 (mate 1 forward; the left group of c = 0):
        0 (50, 1000, 1040)   1 (30, 1010, 1050)   2 empty   3 ignored: score 2^62   4 (20, 1050, 1120)
      group 3 (mate 2 reverse; the right group of c = 0):
        0 (40, 1060, 1100)   1 (40, 1160, 1200)   2 (10, 1059, 1099)   3 (10, 1161, 1201)   4 ignored: ref_begin == ref_end
      c = 0, 3 x 4 candidates:
        (0, 0) fragment 100 = min_fragment: deviation 50, penalty 25, 90 - 25 = 65
        (0, 1) fragment 200 = max_fragment: deviation 50, penalty 25, 65: equal to (0, 0) in score and deviation, behind it by (c, i, j)
        (0, 2) fragment 99, one below;  (0, 3) fragment 201, one above: not proper
        (1, 0) fragment 90, (1, 2) fragment 89: not proper
        (1, 1) fragment 190: deviation 40, penalty 20, 70 - 20 = 50
        (1, 3) fragment 191: deviation 41, penalty 20, 40 - 20 = 20
        (4, 0), (4, 2): the left chain ends behind the right one (1120 > 1100, 1099): not proper
        (4, 1) fragment 150: penalty 0, 60;  (4, 3) fragment 151: deviation 1, penalty 0, 30
      group 2 (mate 2 forward; the left group of c = 1):  0 (3, 2000, 2030)   1 (25, 2000, 2040)   2 empty   3 empty with a score   4 empty
      group 1 (mate 1 reverse; the right group of c = 1): 0 (4, 2070, 2100)   1 (30, 2110, 2160)   2 ignored: ref_end 2^62   3, 4 empty
      c = 1, 2 x 2 candidates:
        (0, 0) fragment 100: penalty 25 above chain_score 7: score 0
        (0, 1) fragment 160: deviation 10, penalty 5, 33 - 5 = 28
        (1, 0) fragment 100: penalty 25, 29 - 25 = 4
        (1, 1) fragment 160: penalty 5, 55 - 5 = 50: equal to c = 0 (1, 1) in score, ahead of it by its deviation (10 < 40)
      16 candidates, 10 proper, 10 kept, 3 ignored; mate 1: 50 at group 0 entry 0; mate 2: 40 at group 3 entry 0 (entry 1 has 40 too).
    Pair 1: one chain each, (10, 500, 530) in group 0 and (10, 600, 650) in group 3: fragment 150, score 20: the unique pair.
    Pair 2: mate 1 has one chain, (7, 10, 20) at group 1 entry 1; mate 2 has none."""
    g0 = [chain(50, 1000, 1040, 3, 7), chain(30, 1010, 1050), EMPTY, chain(X_LIMIT, 1000, 1040), chain(20, 1050, 1120, 9, U64)]
    g3 = [chain(40, 1060, 1100), chain(40, 1160, 1200, 2, 5), chain(10, 1059, 1099), chain(10, 1161, 1201), chain(5, 1100, 1100)]
    g2 = [chain(3, 2000, 2030), chain(25, 2000, 2040), EMPTY, chain(99, 2000, 2040, anchors=0), EMPTY]
    g1 = [chain(4, 2070, 2100), chain(30, 2110, 2160), chain(5, 10, X_LIMIT), EMPTY, EMPTY]
    none = [EMPTY] * 5
    one = [[chain(10, 500, 530)] + [EMPTY] * 4, none, none, [chain(10, 600, 650)] + [EMPTY] * 4]
    lone = [none, [EMPTY, chain(7, 10, 20)] + [EMPTY] * 3, none, none]
    return u64([g0, g1, g2, g3] + one + lone)


HAND_TOP = [[65, 100, 25, 90, 0, 0, 3, 0], [65, 200, 25, 90, 0, 0, 3, 1], [60, 150, 0, 60, 0, 4, 3, 1], [50, 160, 5, 55, 2, 1, 1, 1],
            [50, 190, 20, 70, 0, 1, 3, 1], [30, 151, 0, 30, 0, 4, 3, 3], [28, 160, 5, 33, 2, 0, 1, 1], [20, 191, 20, 40, 0, 1, 3, 3]]
HAND_REST = [[4, 100, 25, 29, 2, 1, 1, 0], [0, 100, 25, 7, 2, 0, 1, 0]]
HAND_SUMS = [[16, 10, 10, 3, 50, 0, 40, 3 << 32], [1, 1, 1, 0, 10, 0, 10, 3 << 32], [0, 0, 0, 0, 7, (1 << 32) | 1, 0, UNKNOWN]]
HAND_STATS = dict(pairs=3, candidates=17, proper=11, kept=11, ignored=3, paired=2, unique=1, unique_fragment_sum=150)


def test_restate_on_a_hand_made_case():
    """3. Rows, summaries and stats typed in by hand (the derivation is hand_made's text): fragments exactly on min_fragment and
    max_fragment and one beyond each, a penalty above chain_score, two candidates equal in score that differ in deviation, two
    equal in both where (c, i, j) decides, the three kinds of ignored entry, an empty entry between valid ones, a unique pair
    and a mate without a chain."""
    from gcsa2_amd import binding_pairs
    assert tuple(HAND_STATS) == binding_pairs.PAIR_STATS and HAND["orientation"] == binding_pairs.PAIR_FR
    packed = binding_pairs.pair_params(**HAND)                  # the restatement's parameters are the structure's, name for name
    assert {name: getattr(packed, name) for name, _ in packed._fields_} == HAND
    rows = hand_made()
    top, sums, stats, full = restate(rows, 3, 5, HAND)
    zero = [0] * 8
    assert top[0].tolist() == HAND_TOP and [k[0] for k in full[0]] == HAND_TOP + HAND_REST
    assert top[1].tolist() == [[20, 150, 0, 20, 0, 0, 3, 0]] + [zero] * 7 and top[2].tolist() == [zero] * 8
    assert sums.tolist() == HAND_SUMS and stats == HAND_STATS
    # min_score 1 drops the candidate whose penalty ate its score; top_n 2 cuts the row, not the counts
    top, sums, stats, _ = restate(rows, 3, 5, dict(HAND, min_score=1, top_n=2))
    assert top[0].tolist() == HAND_TOP[:2] and sums[0].tolist() == [16, 10, 9, 3, 50, 0, 40, 3 << 32] and stats == dict(HAND_STATS, kept=10)
    # cost 0: the chain scores alone, then the deviation
    top, _, _, _ = restate(rows, 3, 5, dict(HAND, cost=0, top_n=3))
    assert top[0].tolist() == [[90, 100, 0, 90, 0, 0, 3, 0], [90, 200, 0, 90, 0, 0, 3, 1], [70, 190, 0, 70, 0, 1, 3, 1]]


def generated(rng, n_pairs, chain_top_n, fill=0.6, ignored=0.05, span=600):
    """Chain rows of n_pairs pairs: an entry is empty with probability 1 - fill (a few of those with words in every field but
    `anchors`), else a chain of 20 .. 150 reference bases at 1000 .. 1000 + span with a score of 0 .. 300, or -- with probability
    `ignored` -- an entry of one of the three ignored kinds.  The four words that are not read hold anything."""
    rows = np.zeros((4 * n_pairs, chain_top_n, 8), dtype=np.uint64)
    for g in range(4 * n_pairs):
        for e in range(chain_top_n):
            draw = rng.random()
            junk = [int(x) for x in rng.integers(0, 1 << 62, 4)]
            begin = 1000 + int(rng.integers(0, span))
            end = begin + int(rng.integers(20, 151))
            entry = [int(rng.integers(0, 301)), int(rng.integers(1, 10))] + junk + [begin, end]
            if draw >= fill:
                entry = [0] * 8 if rng.random() < 0.8 else [entry[0], 0] + entry[2:]
            elif draw < ignored:
                kind = int(rng.integers(0, 3))
                if kind == 0:
                    entry[SCORE] = X_LIMIT + int(rng.integers(0, 5))
                elif kind == 1:
                    entry[REF_END] = entry[REF_BEGIN] - int(rng.integers(0, 2))
                else:
                    entry[REF_END] = X_LIMIT + int(rng.integers(0, 5))
            rows[g, e] = entry
    return rows


def swapped(rows, n_pairs):
    """The mates of every pair swapped: group (m, s) becomes group (1 - m, s)."""
    rows = rows.reshape(n_pairs, 4, -1, 8)
    return np.ascontiguousarray(rows[:, [2, 3, 0, 1]]).reshape(4 * n_pairs, -1, 8)


def test_swapping_the_mates():
    """4. Swapping the mates of every pair maps the FR and RF results onto themselves with c -> 1 - c: the same rows in the same
    order but for the mate bit of left_group and right_group; the counts stay and the two mates' best chains change places with
    the mate bit of their group flipped.  On inputs with kept <= top_n (4 x 4 x 2 <= 64) and without two kept candidates equal
    in score and deviation, where (c, i, j) would decide."""
    from gcsa2_amd import binding_pairs
    assert (FR, RF, FF) == (binding_pairs.PAIR_FR, binding_pairs.PAIR_RF, binding_pairs.PAIR_FF) and 4 * 4 * 2 <= binding_pairs.PAIR_TOP_LIMIT
    rng = np.random.default_rng(0x9A12)
    rows = generated(rng, 40, 4, fill=0.8)
    rows[:, :, SCORE] = np.where(rows[:, :, SCORE] < np.uint64(X_LIMIT), u64(rng.integers(0, 1 << 40, rows.shape[:2])), rows[:, :, SCORE])
    other = swapped(rows, 40)
    assert np.array_equal(swapped(other, 40), rows)
    flip = lambda at: at if at == UNKNOWN else at ^ (2 << 32)
    checked = 0
    for orientation in (FR, RF):
        P = pair_params(orientation=orientation, top_n=64, unit=1, cost=3)
        top, sums, stats, full = restate(rows, 40, 4, P)
        top2, sums2, stats2, full2 = restate(other, 40, 4, P)
        assert stats2 == stats and stats["kept"] > 100
        for p in range(40):
            ranks = [(k[0][0], k[1]) for k in full[p]]
            assert len(set(ranks)) == len(ranks) <= 64, "a full tie: choose another seed"
            assert [(1 - k[2][0],) + k[2][1:] for k in full[p]] == [k[2] for k in full2[p]]
            want = top[p].copy()
            want[:len(ranks), 4] ^= np.uint64(2)
            want[:len(ranks), 6] ^= np.uint64(2)
            assert np.array_equal(top2[p], want), (orientation, p)
            a, b = sums[p].tolist(), sums2[p].tolist()
            assert b == a[:4] + [a[6], flip(a[7]), a[4], flip(a[5])], (orientation, p)
            checked += len(ranks)
    assert checked > 200


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


def sentinels(words):
    import torch
    return torch.full((words + GUARD,), np.uint64(SENTINEL).view(np.int64).item(), dtype=torch.int64, device=torch.device("cuda", 0))


class Outputs:
    """Sentinel-filled device buffers of one pair call with GUARD sentinel words behind them; each may be absent."""

    def __init__(self, n_pairs, top_n, top=True, summaries=True, stats=True):
        self.stats = stats
        self.sizes = dict(top=n_pairs * top_n * 8, sums=n_pairs * 8)
        wanted = dict(top=top, sums=summaries)
        self.bufs = {key: (sentinels(size) if wanted[key] else None) for key, size in self.sizes.items()}

    def pointers(self):
        return tuple(self.bufs[key].data_ptr() if self.bufs[key] is not None else 0 for key in ("top", "sums"))

    def arrays(self):
        import torch
        torch.cuda.synchronize()
        return {key: (t.cpu().numpy().view(np.uint64) if t is not None else None) for key, t in self.bufs.items()}

    def check(self, got_stats, want, what):
        """Rows and summaries fully overwritten with the expected, the guards untouched, every stats field equal."""
        got = self.arrays()
        for key, expected in zip(("top", "sums"), want[:2]):
            if got[key] is None:
                continue
            size = self.sizes[key]
            a, b = got[key][:size], expected.reshape(-1)
            bad = np.nonzero(a != b)[0]
            assert bad.size == 0, (what, key, int(bad.size), int(bad[0]), a[bad[0] - bad[0] % 8:][:8].tolist(), b[bad[0] - bad[0] % 8:][:8].tolist())
            assert (got[key][size:] == np.uint64(SENTINEL)).all(), (what, "behind", key)
        if self.stats:
            assert got_stats == want[2], (what, got_stats, want[2])
        else:
            assert got_stats is None


def run_rows(gpu, d_rows, rows, n_pairs, chain_top_n, P, what, cache=None, **absent):
    """The seed form on the first n_pairs pairs of `rows` (in device memory as d_rows) against the restatement."""
    want = restate(rows[:4 * n_pairs], n_pairs, chain_top_n, P, cache)
    out = Outputs(n_pairs, P["top_n"], **absent)
    out.check(gpu.chain_pairs_device(d_rows.data_ptr(), n_pairs, chain_top_n, *out.pointers(), want_stats=out.stats, **P), want, what)
    return want


SWEEP_FILL = {1: 0.8, 5: 0.6, 64: 0.25}


@functools.lru_cache(maxsize=None)
def sweep_rows(chain_top_n):
    """The 257 pairs of the sweep at one chain_top_n, generated once and left unchanged."""
    rows = generated(np.random.default_rng(0x9A20 + chain_top_n), 257, chain_top_n, fill=SWEEP_FILL[chain_top_n])
    rows.setflags(write=False)
    return rows


def test_the_sweep_sees_every_count():
    """5, the expectation's side, on the CPU: over the rows and the orientations of the sweep of test_generated_rows, `kept`,
    `ignored`, `unique` and `paired` of the expectation are each greater than 0 -- at every chain_top_n for the first, second and
    last, and `unique` where rows are short enough for a pair to have one placement."""
    from gcsa2_amd import binding_pairs
    seen = dict.fromkeys(("kept", "ignored", "unique", "paired"), 0)
    for chain_top_n in SWEEP_FILL:
        for orientation in (binding_pairs.PAIR_FR, binding_pairs.PAIR_RF, binding_pairs.PAIR_FF):
            stats = restate(sweep_rows(chain_top_n), 257, chain_top_n, pair_params(orientation=orientation))[2]
            assert stats["kept"] > 0 and stats["ignored"] > 0 and stats["paired"] > 0, (chain_top_n, orientation, stats)
            for name in seen:
                seen[name] += stats[name]
    assert all(seen[name] > 0 for name in seen), seen
    assert restate(sweep_rows(1), 257, 1, pair_params())[2]["unique"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("orientation", (FR, RF, FF))
@pytest.mark.parametrize("chain_top_n", (1, 5, 64))
def test_generated_rows(big, chain_top_n, orientation):
    """5. The seed form against the restatement on generated rows: 1, 4, 5 and 257 pairs (one wavefront, a full workgroup, one past
    it, 65 workgroups; the grid's stride is test_more_pairs_than_the_grid's), chain_top_n 1, 5 and 64, top_n 1, 4 and 64, the
    three orientations; rows with empty entries between valid ones and the three kinds of ignored entry; and, on the first
    orientation, cost 0, a min_score that cuts part of the proper candidates, a unit above every deviation and deviations next to
    2^32."""
    rows = sweep_rows(chain_top_n)
    d_rows = to_device(rows)
    cache = {}
    sets = [pair_params(orientation=orientation)]
    if orientation == FR:
        sets += [pair_params(cost=0), pair_params(min_score=250, cost=7, unit=3), pair_params(unit=1 << 20, cost=65536), pair_params(unit=U64),
                 pair_params(min_fragment=0, max_fragment=LIMIT - 1, mean_fragment=LIMIT - 1, unit=1 << 20, cost=1)]
    for P in sets:
        for n_pairs in (1, 4, 5, 257):
            for top_n in (1, 4, 64):
                want = run_rows(big, d_rows, rows, n_pairs, chain_top_n, dict(P, top_n=top_n), (chain_top_n, n_pairs, tuple(P.values()), top_n), cache)
        top, sums, stats, full = want
        assert stats["candidates"] > stats["proper"] > 0 and stats["ignored"] > 0 and stats["paired"] > 0
        if P.get("min_score"):
            assert 0 < stats["kept"] < stats["proper"]
        if P["unit"] >= 1 << 20 and P["mean_fragment"] < LIMIT - 1:
            assert all(k[0][2] == 0 for kept in full for k in kept)
    if chain_top_n > 1:
        assert max(len(kept) for kept in full) > 4, "no pair with more kept candidates than top_n = 4"
    assert any(any(rows[g, e, ANCHORS] == 0 and rows[g, e + 1:, ANCHORS].any() for e in range(chain_top_n - 1)) for g in range(rows.shape[0])) or chain_top_n == 1


@pytest.mark.gpu
def test_every_candidate_proper(big):
    """5, continued.  chain_top_n = 64 with all 2 x 64 x 64 = 8192 candidates proper and kept, top_n = 64: every left chain lies in
    front of every right chain and every fragment is inside the window; with scores that repeat, so that deviation and (c, i, j)
    order most of the row."""
    rng = np.random.default_rng(0x9A30)
    rows = np.zeros((8, 64, 8), dtype=np.uint64)
    for p in range(2):
        for g in range(4):
            left = g in (0, 2)                                 # FR: the forward groups are the left ones
            for e in range(64):
                begin = (1000 if left else 1400) + int(rng.integers(0, 100))
                rows[4 * p + g, e] = chain(int(rng.integers(0, 4 if p else 300)), begin, begin + int(rng.integers(30, 100)), 2, int(rng.integers(0, 1 << 63)))
    d_rows = to_device(rows)
    for P in (pair_params(top_n=64, min_fragment=300, max_fragment=700, mean_fragment=480, unit=7, cost=2), pair_params(top_n=64, cost=0, max_fragment=700)):
        top, sums, stats, full = run_rows(big, d_rows, rows, 2, 64, P, ("all proper", tuple(P.values())))
        assert stats["candidates"] == stats["proper"] == stats["kept"] == 2 * 8192 and stats["paired"] == 2 and stats["unique"] == 0
        assert top[:, :, 1].all()
    assert len({tuple(k[0][:1]) for k in full[1][:64]}) < 8          # the last row is ordered by deviation and (c, i, j)


@pytest.mark.gpu
def test_more_pairs_than_the_grid(big):
    """5, continued.  The grid is capped at eight workgroups of four pairs per compute unit and the pairs are strided: 4 x 8 x 320 + 3
    pairs are more than one pass of it on a device of up to 320 compute units (an MI355X has 256).  Two entries a row keep the
    restatement short."""
    n_pairs = 4 * 8 * 320 + 3
    rows = generated(np.random.default_rng(0x9A35), n_pairs, 2, fill=0.7)
    top, sums, stats, full = run_rows(big, to_device(rows), rows, n_pairs, 2, pair_params(top_n=2), "the grid's stride")
    assert stats["unique"] > 100 and stats["paired"] > stats["unique"] and sums[-3:, 0].any()


@pytest.mark.gpu
def test_the_hand_made_case_and_absent_outputs(big):
    """3 on the device, and 6: each of d_top, d_summaries and stats NULL in turn, and all three -- the others are the same, the
    stats equal those of the full call, and no word of a guard region is touched.  Rows that start at an address that is no
    multiple of 16 take the kernel's 8-byte loads and stores."""
    rows = hand_made()
    d_rows = to_device(rows)
    want = run_rows(big, d_rows, rows, 3, 5, HAND, "hand-made")
    assert want[0][0].tolist() == HAND_TOP and want[1].tolist() == HAND_SUMS and want[2] == HAND_STATS
    for absent in (dict(top=False), dict(summaries=False), dict(stats=False), dict(top=False, summaries=False), dict(top=False, summaries=False, stats=False)):
        run_rows(big, d_rows, rows, 3, 5, HAND, ("hand-made", tuple(absent)), **absent)
    big_rows = generated(np.random.default_rng(0x9A40), 9, 64, fill=0.3)
    for absent in (dict(), dict(top=False), dict(summaries=False), dict(stats=False), dict(top=False, summaries=False)):
        run_rows(big, to_device(big_rows), big_rows, 9, 64, pair_params(top_n=5), ("64 entries", tuple(absent)), **absent)
    # one word further: the rows are 8-byte aligned only
    shifted = to_device(np.concatenate([u64([SENTINEL]), rows.reshape(-1)]))
    P = HAND
    out = Outputs(3, P["top_n"])
    stats = big.chain_pairs_device(shifted.data_ptr() + 8, 3, 5, *out.pointers(), **P)
    out.check(stats, want, "rows at an odd word")


# ---- the LAW ---------------------------------------------------------------------------------------------------------------

READ = 50                                                   # the length of a mate
COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def reverse_complement(read):
    return bytes(c if c in b"ACGT" else ord("N") for c in read.translate(COMPLEMENT)[::-1])


def paired_reads(g, seed, count):
    """Interleaved mates of `count` fragments: walks of 2 READ + 20 .. 4 READ characters; mate 1 is the first READ characters of
    the fragment, mate 2 the reverse complement of its last READ; every second fragment is reverse-complemented first (a pair
    from the other strand: its mate 2 is the one that lies forward, upstream)."""
    reads = []
    for p, fragment in enumerate(walks(g, seed, count, lo=2 * READ + 20, hi=4 * READ)):
        if p % 2:
            fragment = reverse_complement(fragment)
        reads += [fragment[:READ], reverse_complement(fragment[-READ:])]
    return reads


def backbone_map(g, shift):
    """coord_of_bin over the node ids of an SNP graph (shift = the bits below the id of a located value): the backbone position
    of the node's first base, an alternative allele at the position of its site -- coordinates in which a walk is contiguous,
    so that the chains of two mates lie a fragment length apart.  (The `linear` map of test_seed_clusters.coord_map, x = the
    located value, puts 2^shift between two nodes; the 6000-base graph runs under it as well.)"""
    from workload.graphs import ID_OFFSET
    assert shift == ID_OFFSET
    n = int(np.nonzero(g.comp == 0)[0][0]) - 1                  # positions 1 .. n are the backbone, n + 1 is the sink
    value = np.asarray(g.value, dtype=np.uint64)
    bins = (value >> np.uint64(shift)).astype(np.int64)
    cmap = np.full(int(bins.max()) + 1, UNKNOWN, dtype=np.uint64)
    offset = (value & np.uint64((1 << shift) - 1)).astype(np.int64)
    position = np.arange(1, n + 1)
    cmap[bins[1:n + 1]] = (position - offset[1:n + 1]).astype(np.uint64)
    for b in bins[n + 2:]:                                      # an alternative allele's id follows its reference allele's
        cmap[b] = cmap[b - 1]
    return cmap


@functools.lru_cache(maxsize=None)
def pair_case(graph):
    """(the graph, its index, the interleaved reads) of the 3000-base graph of test_seed_chains and of the 6000-base BIG."""
    if graph == "snp6000":
        g, ix = GRAPHS[BIG][1], indexed(BIG)[0]
    else:
        from workload import graphs
        g, ix = graphs.snp_graph(3000, 0x81, 0x82, snp_period=12, node_len=16), chains.small_graph()[0]
    return g, ix, paired_reads(g, 0x9A50 + len(graph), 40)


CHAINS = chains.params(band=16, top_n=4, member_cap=2, lookback=32, max_gap=200)
# The fragment window.  A fragment here is between chain extents: from the first seed of the upstream mate's chain to the end of
# the last seed of the downstream mate's, so somewhat shorter than the walk of 2 READ + 20 .. 4 READ = 120 .. 200 characters.
# The expectation's own best fragments under an open window (test_the_law prints them) are 108 .. 195 on both graphs, every one
# of the 40 pairs placed; the window 115 .. 190 around 150 keeps most of them and leaves a few pairs at either end unplaced.
WINDOW = dict(min_fragment=115, max_fragment=190, mean_fragment=150, unit=8, cost=2)
OPEN = dict(min_fragment=0, max_fragment=LIMIT - 1, mean_fragment=150, unit=8, cost=0)


class ChainOutputs(chains.Outputs):
    """The chain outputs of a fused call, and the pair outputs beside them."""

    def __init__(self, n_reads, P, PP, **absent):
        super().__init__(2 * n_reads, P, **{k: v for k, v in absent.items() if k in ("top", "members", "summaries")})
        self.pairs = Outputs(n_reads // 2, PP["top_n"], top=absent.get("pair_top", True), summaries=absent.get("pair_summaries", True))

    def every(self):
        return tuple(self.pointers()) + tuple(self.pairs.pointers())


def fused(gpu, batch, k, w, hit_max, over, shift, d_map, n_bins, P, PP, out, want_stats=True):
    return gpu.minimizer_chain_pairs_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, k, w, 0, hit_max, over, shift, d_map.data_ptr(), n_bins,
                                            *out.every(), want_stats=want_stats, pair=PP, **P)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", ("snp3000", "snp6000"))
def test_the_law(engine, big, monkeypatch, graph):
    """7. LAW: gcsa2_minimizer_chain_pairs_device equals gcsa2_stranded_minimizer_hits_device (both strands, exact buffers), then
    gcsa2_seed_chains_device over the 2 n groups, then gcsa2_chain_pairs_device over the n / 2 pairs, word for word -- and both
    equal the pair restatement over the chain restatement over the located CSR --, at (k, w) = (16, 5) and (12, 11), SKIP and
    SAMPLE hit lists, under the backbone map (and, on the 6000-base graph, the linear map of test_seed_clusters).  With chain rows
    that stay in scratch (d_chains NULL) and all outputs NULL the stats are the same.  Under GCSA2_CHAIN_LDS=64 nothing changes
    but chain_stats.spilled.  Pairs of both strands of origin are placed: the even pairs by c = 0, the odd ones by c = 1."""
    g, ix, reads = pair_case(graph)
    gpu = big if graph == "snp6000" else engine.open_index(ix, device=0)[0]
    shift = 11
    maps = [("backbone", backbone_map(g, shift))] + ([("linear", coord_map("linear", BIG, shift))] if graph == "snp6000" else [])
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    n, n_pairs = len(reads), len(reads) // 2
    placed = {0: 0, 1: 0}
    for name, cmap in maps:
        d_map = to_device(cmap)
        n_bins = cmap.shape[0]
        P = CHAINS if name == "backbone" else dict(CHAINS, band=U64, gap=0, max_gap=LIMIT - 1)
        for (k, w), (hit_max, over) in (((16, 5), (0, 0)), ((12, 11), (8, 1))) if name == "linear" else [(kw, ho) for kw in ((16, 5), (12, 11)) for ho in ((0, 0), (8, 1))]:
            what = (graph, name, k, w, hit_max, over)
            soff, seeds, hoff, hits = gpu.stranded_minimizer_hits_batch(flat, off, k, w, hit_max=hit_max, sample=bool(over))[:4]
            chain_want = chains.restate(soff, seeds, hoff, hits, shift, cmap, P)
            if name == "backbone":
                fragments = sorted(k[0][1] for kept in restate(chain_want[0], n_pairs, P["top_n"], dict(pair_params(**OPEN), top_n=1))[3] for k in kept[:1])
                print("chain_pairs fragments under an open window:", what, fragments)
            for PP in (pair_params(**WINDOW, top_n=3), pair_params(**OPEN, orientation=FF, top_n=2)) if name == "backbone" else (pair_params(**OPEN, top_n=3),):
                want = restate(chain_want[0], n_pairs, P["top_n"], PP)
                # the composition, every buffer exactly to size
                d_soff, d_seeds, d_hoff, d_hits = (to_device(a) for a in (np.zeros(2 * n + 1, np.uint64), np.zeros((max(len(seeds), 1), 5), np.uint64),
                                                                          np.zeros(len(seeds) + 1, np.uint64), np.zeros(max(len(hits), 1), np.uint64)))
                assert gpu.stranded_minimizer_hits_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), n, k, w, 0, engine.STRAND_BOTH, hit_max, over, 0,
                                                          d_soff.data_ptr(), d_seeds.data_ptr(), len(seeds), d_hoff.data_ptr(), d_hits.data_ptr(), len(hits)) == (len(seeds), len(hits))
                three = ChainOutputs(n, P, PP)
                chain_stats = gpu.seed_chains_device(d_soff.data_ptr(), 2 * n, d_seeds.data_ptr(), len(seeds), d_hoff.data_ptr(), d_hits.data_ptr(), len(hits),
                                                     shift, d_map.data_ptr(), n_bins, *three.pointers(), **P)
                pair_stats = gpu.chain_pairs_device(three.bufs["top"].data_ptr(), n_pairs, P["top_n"], *three.pairs.pointers(), **PP)
                three.check(chain_stats, chain_want, what + ("composition: chains",), spilled=0)
                three.pairs.check(pair_stats, want, what + ("composition: pairs",))
                one = ChainOutputs(n, P, PP)
                got = fused(gpu, batch, k, w, hit_max, over, shift, d_map, n_bins, P, PP, one)
                one.check(got[0], chain_want, what + ("fused: chains",), spilled=0)
                one.pairs.check(got[1], want, what + ("fused: pairs",))
                assert got == (chain_stats, pair_stats), what
                assert all(np.array_equal(x, y) for o in ((one, three), (one.pairs, three.pairs)) for x, y in zip(o[0].arrays().values(), o[1].arrays().values())), what
                none = ChainOutputs(n, P, PP, top=False, members=False, summaries=False, pair_top=False, pair_summaries=False)
                assert fused(gpu, batch, k, w, hit_max, over, shift, d_map, n_bins, P, PP, none) == got, what
                assert fused(gpu, batch, k, w, hit_max, over, shift, d_map, n_bins, P, PP, none, want_stats=False) == (None, None)
                scratch_rows = ChainOutputs(n, P, PP, top=False)
                assert fused(gpu, batch, k, w, hit_max, over, shift, d_map, n_bins, P, PP, scratch_rows) == got, what
                scratch_rows.pairs.check(got[1], want, what + ("chain rows in scratch",))
                small = ChainOutputs(n, P, PP)
                small_got = chains.with_knob(monkeypatch, "64", lambda: fused(gpu, batch, k, w, hit_max, over, shift, d_map, n_bins, P, PP, small))
                small.check(small_got[0], chain_want, what + ("knob 64",), spilled=int((chain_want[2][:, :2].sum(axis=1) > 64).sum()))
                small.pairs.check(small_got[1], want, what + ("knob 64: pairs",))
                if PP["orientation"] == FR and name == "backbone":
                    for p in range(n_pairs):
                        if want[1][p, 2] > 0:
                            placed[p % 2] += 1
                            assert int(want[0][p, 0, 4]) == (0 if p % 2 == 0 else 2), (what, p, want[0][p, 0].tolist())
    assert placed[0] > 10 and placed[1] > 10, placed
    if graph != "snp6000":
        gpu.close()


def as_words(got):
    """The binding's structured arrays of the host form as the restatements' words."""
    rows, members, chain_sums, top, sums = got[:5]
    n2, chain_top_n = rows.shape
    return (rows.view(np.uint64).reshape(n2, chain_top_n, 8), members.view(np.uint64).reshape(n2, chain_top_n, -1, 2), chain_sums.view(np.uint64).reshape(n2, 3),
            top.view(np.uint64).reshape(top.shape[0], -1, 8), sums.view(np.uint64).reshape(-1, 8))


@pytest.mark.gpu
def test_host_form(engine, big, monkeypatch):
    """8. minimizer_chain_pairs_batch returns structured arrays equal to the restatement (and so to the device form); an odd number
    of reads is refused with nothing written; and a batch in pieces gives the same.  The piece size is read when an index is
    opened and is at least 1 MB, so the pieces are those of a second handle opened under GCSA2_MS_PIECE_MB=1 and of a batch of
    more than 3 MB: the reads of the small case over and over, so that its expectation, tiled, is the expectation."""
    g, ix, reads = pair_case("snp6000")
    flat, off = concat_patterns(reads)
    shift = 11
    cmap = backbone_map(g, shift)
    P, PP = CHAINS, pair_params(**WINDOW, top_n=3)
    soff, seeds, hoff, hits = big.stranded_minimizer_hits_batch(flat, off, 16, 5, hit_max=64)[:4]
    chain_want = chains.restate(soff, seeds, hoff, hits, shift, cmap, P)
    want = restate(chain_want[0], len(reads) // 2, P["top_n"], PP)
    got = big.minimizer_chain_pairs_batch(flat, off, 16, 5, cmap, hit_max=64, shift=shift, pair=PP, **P)
    assert got[0].dtype == engine.CHAIN and got[1].dtype == engine.CHAIN_ANCHOR and got[2].dtype == engine.CHAIN_SUMMARY
    assert got[3].dtype == engine.CHAIN_PAIR and got[4].dtype == engine.PAIR_SUMMARY
    assert got[0].shape == (2 * len(reads), 4) and got[1].shape == (2 * len(reads), 4, 2) and got[3].shape == (len(reads) // 2, 3) and got[4].shape == (len(reads) // 2,)
    words = as_words(got)
    assert all(np.array_equal(a, b) for a, b in zip(words, chain_want[:3] + want[:2]))
    assert {f: got[5][f] for f in chains.FIELDS} == chain_want[3] and got[6] == want[2] and want[2]["paired"] > 20
    absent = big.minimizer_chain_pairs_batch(flat, off, 16, 5, cmap, hit_max=64, shift=shift, chains=False, members=False, chain_summaries=False, top=False,
                                             summaries=False, pair=PP, **P)
    assert absent[:5] == (None,) * 5 and absent[5:] == got[5:]
    empty = big.minimizer_chain_pairs_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 16, 5, cmap, pair=PP, **P)
    assert empty[0].shape == (0, 4) and empty[3].shape == (0, 3) and set(empty[5].values()) == {0} and set(empty[6].values()) == {0}
    # an odd number of reads: refused, and nothing written to the caller's arrays
    from gcsa2_amd.binding import ChainParams, PairParams
    cp, pp = ChainParams(*(P[name] for name in chains.PARAMS)), PairParams(*(PP[name] for name in PARAMS))
    fill = lambda n: (ctypes.c_uint64 * n)(*([SENTINEL] * n))
    outs = [fill(2 * 3 * 4 * 8), fill(2 * 3 * 4 * 2 * 2), fill(2 * 3 * 3), fill(3 * 8), fill(8), fill(7), fill(8)]
    three, off3 = concat_patterns(reads[:3])
    rc = big._L.gcsa2_minimizer_chain_pairs_batch(big._h, engine._p8(three), engine._p64(off3), 3, 16, 5, 0, 64, 0, shift, cmap.ctypes.data, cmap.shape[0],
                                                  ctypes.addressof(cp), ctypes.addressof(pp), *(ctypes.addressof(o) for o in outs))
    assert rc == INVALID and "n_patterns must be even" in big._L.gcsa2_last_error().decode() and all(list(o) == [SENTINEL] * len(o) for o in outs)
    # pieces
    times = (3 << 20) // int(off[-1]) + 2
    many = reads * times
    flat_many, off_many = concat_patterns(many)
    assert int(off_many[-1]) > 3 << 20
    monkeypatch.setenv("GCSA2_MS_PIECE_MB", "1")
    cut, _ = engine.open_index(ix, device=0)
    monkeypatch.delenv("GCSA2_MS_PIECE_MB")
    in_pieces = cut.minimizer_chain_pairs_batch(flat_many, off_many, 16, 5, cmap, hit_max=64, shift=shift, pair=PP, **P)
    cut.close()
    whole = big.minimizer_chain_pairs_batch(flat_many, off_many, 16, 5, cmap, hit_max=64, shift=shift, pair=PP, **P)
    for a, b, c in zip(as_words(in_pieces), as_words(whole), words):
        assert np.array_equal(a, b) and np.array_equal(a, np.concatenate([c] * times))
    assert in_pieces[5] == whole[5] and in_pieces[6] == whole[6] == {f: v * times for f, v in got[6].items()}


def client_lines(rows, top, sums, stats):
    lines = ["chain %d %d %s" % (q, j, " ".join(str(int(x)) for x in rows[q, j])) for q in range(rows.shape[0]) for j in range(rows.shape[1])]
    lines += ["pair %d %d %s" % (p, r, " ".join(str(int(x)) for x in top[p, r])) for p in range(top.shape[0]) for r in range(top.shape[1])]
    lines += ["summary %d %s" % (p, " ".join(str(int(x)) for x in sums[p])) for p in range(sums.shape[0])]
    return lines + ["stats " + " ".join(str(int(stats[f])) for f in STATS)]


@pytest.mark.gpu
def test_facade_client(big, tmp_path):
    """9. tests/cpp/chain_pairs_client.cpp, a client of the C++ facade (minimizer_chain_pairs_batch), prints the chain rows, pair
    rows, summaries and stats that the binding returns."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    g, ix, reads = pair_case("snp6000")
    assert all(b"\n" not in r for r in reads)
    flat, off = concat_patterns(reads)
    save_host_view(ix, str(tmp_path / "index.g2hv"))
    (tmp_path / "reads.txt").write_bytes(b"".join(r + b"\n" for r in reads))
    exe = compile_client(str(tmp_path / "chain_pairs_client"), os.path.join(ROOT, "tests", "cpp", "chain_pairs_client.cpp"))
    shift = 11
    cmap = coord_map("linear", BIG, shift)                         # the client makes the same map
    P, PP = dict(CHAINS, band=U64, gap=0, max_gap=LIMIT - 1), pair_params(**OPEN, top_n=3)
    got = big.minimizer_chain_pairs_batch(flat, off, 16, 5, cmap, hit_max=64, shift=shift, pair=PP, **P)
    out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "reads.txt")] +
                         [str(int(x)) for x in (16, 5, 64, shift, cmap.shape[0]) + tuple(P[name] for name in chains.PARAMS) + tuple(PP[name] for name in PARAMS)],
                         capture_output=True, text=True, env=_run_env(), timeout=300)
    assert out.returncode == 0, out.stderr
    words = as_words(got)
    assert got[6]["paired"] > 0 and out.stdout.strip().split("\n") == client_lines(words[0], words[3], words[4], got[6])


@pytest.mark.gpu
def test_refusals_on_a_device(engine, big):
    """10. The fused forms need the samples and the counters (MISSING_COMPONENT on a find-only image, nothing written); the seed
    form needs no component and runs on the same image.  The limits are those of the stranded hits call: 2^31 reads or more are
    BUFFER_TOO_SMALL before any read is looked at."""
    g, ix, reads = pair_case("snp6000")
    bare = engine.GCSA(ix, with_lcp=False, with_samples=False, with_counters=False)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    shift, P, PP = 11, CHAINS, pair_params(**WINDOW)
    cmap = backbone_map(g, shift)
    d_map = to_device(cmap)
    out = ChainOutputs(batch.n, P, PP)
    with pytest.raises(engine.Gcsa2Error) as err:
        fused(bare, batch, 16, 5, 0, 0, shift, d_map, cmap.shape[0], P, PP, out)
    assert err.value.code == MISSING, err.value
    assert all((a == np.uint64(SENTINEL)).all() for o in (out, out.pairs) for a in o.arrays().values())
    with pytest.raises(engine.Gcsa2Error) as err:
        bare.minimizer_chain_pairs_batch(flat, off, 16, 5, cmap, shift=shift, pair=PP, **P)
    assert err.value.code == MISSING
    rows = hand_made()
    run_rows(bare, to_device(rows), rows, 3, 5, HAND, "the seed form on a find-only image")
    bare.close()
    with pytest.raises(engine.Gcsa2Error) as err:
        big.minimizer_chain_pairs_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), 1 << 31, 16, 5, 0, 0, 0, shift, d_map.data_ptr(), cmap.shape[0],
                                         *out.every(), pair=PP, **dict(P, member_cap=0))
    assert err.value.code == -6 and "2^31 or more reads" in str(err.value)
    assert all((a == np.uint64(SENTINEL)).all() for o in (out, out.pairs) for a in o.arrays().values())


# ---- the stream contract of the new header -------------------------------------------------------------------------------------
# One row per binding method (or per form of one): the C entry point it reaches and its contract class, in the header's words.
TABLE = {
    "chain_pairs_device":             ("gcsa2_chain_pairs_device", COMPLETE),
    "chain_pairs_device-64":          ("gcsa2_chain_pairs_device", COMPLETE),
    "minimizer_chain_pairs_device":   ("gcsa2_minimizer_chain_pairs_device", COMPLETE),
}
BUILDERS = {}


def test_every_stream_entry_point_of_the_pair_header_has_a_row():
    """11. A declaration of include/gcsa2_hip_pairs.h with a `void* stream` parameter (found with the regular expression of
    tests/test_stream_contract.py) has a row in TABLE; every row names a declaration and its binding method exists."""
    import test_stream_contract as contract
    from gcsa2_amd import binding
    with open(os.path.join(ROOT, "include", "gcsa2_hip_pairs.h")) as f:
        declared = contract.declarations_with_a_stream(f.read())
    assert declared == {"gcsa2_chain_pairs_device", "gcsa2_minimizer_chain_pairs_device"}
    assert {c for c, _ in TABLE.values()} == declared
    assert all(hasattr(binding.GCSA, row.split("-")[0]) for row in TABLE)
    assert set(TABLE) == set(BUILDERS)


def chain_pairs_row(n_pairs, chain_top_n, top_n):
    """Generated rows; the decoy's are other rows of the same shape."""
    def build(env, name):
        rows = generated(np.random.default_rng(0x57F0), n_pairs, chain_top_n)
        decoy = generated(np.random.default_rng(0x57F1), n_pairs, chain_top_n)
        P = pair_params(top_n=top_n)
        return Case(name, COMPLETE, {"rows": (rows, decoy)}, {"top": 64 * n_pairs * top_n, "sums": 64 * n_pairs},
                    lambda p, s: tuple(sorted(env.gpu.chain_pairs_device(p["rows"], n_pairs, chain_top_n, p["top"], p["sums"], s, **P).items())))
    return build


BUILDERS["chain_pairs_device"] = chain_pairs_row(3000, 5, 2)
BUILDERS["chain_pairs_device-64"] = chain_pairs_row(300, 64, 64)


def fused_row(env, name):
    """The reads of the stream-contract tests as if they were interleaved mates: they all lie forward, so FF places them."""
    import test_stream_contract as contract
    ins, n, total = contract.reads_input()
    n -= n % 2
    ins["cmap"] = contract.coord_table(env)
    P, PP = chains.params(top_n=2, member_cap=2, band=U64, gap=0, max_gap=LIMIT - 1), pair_params(**OPEN, orientation=FF, top_n=2)
    sizes = {"rows": 64 * 2 * n * 2, "members": 16 * 2 * n * 2 * 2, "chain_sums": 24 * 2 * n, "top": 64 * (n // 2) * 2, "sums": 64 * (n // 2)}

    def call(p, s):
        chain_stats, stats = env.gpu.minimizer_chain_pairs_device(p["pat"], p["off"], n, 16, 5, 7, contract.HIT_MAX, contract.SAMPLE, contract.SHIFT, p["cmap"],
                                                                  env.n_bins(), p["rows"], p["members"], p["chain_sums"], p["top"], p["sums"], s, pair=PP, **P)
        assert stats["paired"] > 0, stats
        return contract.frozen(chain_stats), contract.frozen(stats)

    return Case(name, COMPLETE, ins, sizes, call)


BUILDERS["minimizer_chain_pairs_device"] = fused_row


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
