"""k_find2 on jump-table images fetches its blocks straight into LDS and evaluates them there (kernels_find.hpp).  The
shapes at which a slot assignment or a round count of that path can go wrong: every count of stepping lanes in a wave,
second fetches in most lanes of a wave, iterations that mix jumping, stepping and finished lanes, partial last waves and
workgroups.  Every range is the oracle's, the instrumented twin returns the same ranges, the image without the table (the
register form) agrees, and the STATS counters -- functions of the batch, not of the schedule -- are those of the kernel
before the change."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gcsa2_amd.hostview import concat_patterns
from test_find_only_jump import FIND_ONLY, DeviceBatch, chain_patterns, graph_cases

ENV = ("GCSA2_JUMP_TABLE", "GCSA2_JUMP_BUILD", "GCSA2_KMER_TABLE", "GCSA2_PAIR_BLOCKS", "GCSA2_MEMORY_BUDGET_MB")
LIVE_COUNTS = (0, 1, 31, 32, 33, 47, 48, 49, 63, 64)        # around every stage size a build can have (32, 48, 64)
PLACEMENTS = ("first", "last", "alternating")
MIXED_SIZES = (63, 64, 65, 129)
WIDE_SIZES = (64, 130)

# [blocks, LF steps, seed lookups, jumps, fetch_steps, second_fetches] of every batch below from the kernel before this
# change (register staging, one slot per lane), one find_stats_device call each on the default find-only image.
PARENT_COUNTERS = {
    ("paper", "lanes-first"): [427, 743, 134, 235, 427, 0],
    ("paper", "lanes-last"): [421, 721, 146, 229, 421, 0],
    ("paper", "lanes-alternating"): [432, 746, 133, 240, 432, 0],
    ("paper", "wide-64"): [86, 92, 0, 0, 86, 0],
    ("paper", "wide-130"): [175, 187, 0, 0, 175, 0],
    ("paper", "mixed-63"): [50, 84, 29, 29, 50, 0],
    ("paper", "mixed-64"): [50, 84, 30, 29, 50, 0],
    ("paper", "mixed-65"): [50, 84, 31, 29, 50, 0],
    ("paper", "mixed-129"): [112, 194, 41, 67, 112, 0],
    ("rand1", "lanes-first"): [746, 1517, 137, 493, 746, 0],
    ("rand1", "lanes-last"): [757, 1623, 138, 508, 757, 0],
    ("rand1", "lanes-alternating"): [748, 1541, 138, 488, 748, 0],
    ("rand1", "wide-64"): [57, 76, 0, 0, 57, 0],
    ("rand1", "wide-130"): [116, 154, 0, 0, 116, 0],
    ("rand1", "mixed-63"): [96, 183, 17, 50, 96, 0],
    ("rand1", "mixed-64"): [98, 187, 17, 51, 98, 0],
    ("rand1", "mixed-65"): [102, 197, 17, 56, 102, 0],
    ("rand1", "mixed-129"): [225, 410, 37, 126, 225, 0],
    ("rand2", "lanes-first"): [725, 1695, 234, 509, 725, 0],
    ("rand2", "lanes-last"): [805, 2018, 228, 621, 805, 0],
    ("rand2", "lanes-alternating"): [731, 1779, 241, 538, 731, 0],
    ("rand2", "wide-64"): [67, 111, 0, 0, 67, 0],
    ("rand2", "wide-130"): [136, 226, 0, 0, 136, 0],
    ("rand2", "mixed-63"): [120, 210, 46, 80, 120, 0],
    ("rand2", "mixed-64"): [121, 211, 47, 80, 121, 0],
    ("rand2", "mixed-65"): [123, 217, 47, 83, 123, 0],
    ("rand2", "mixed-129"): [203, 335, 89, 129, 203, 0],
    ("rand3", "lanes-first"): [500, 767, 200, 295, 500, 0],
    ("rand3", "lanes-last"): [575, 966, 184, 379, 575, 0],
    ("rand3", "lanes-alternating"): [523, 816, 194, 317, 523, 0],
    ("rand3", "wide-64"): [44, 44, 0, 0, 44, 0],
    ("rand3", "wide-130"): [90, 90, 0, 0, 90, 0],
    ("rand3", "mixed-63"): [102, 140, 10, 53, 102, 0],
    ("rand3", "mixed-64"): [105, 143, 10, 54, 105, 0],
    ("rand3", "mixed-65"): [105, 143, 11, 54, 105, 0],
    ("rand3", "mixed-129"): [187, 242, 38, 93, 187, 0],
    ("rand4", "lanes-first"): [780, 1986, 195, 515, 780, 0],
    ("rand4", "lanes-last"): [842, 2435, 244, 624, 842, 0],
    ("rand4", "lanes-alternating"): [798, 2084, 205, 541, 798, 0],
    ("rand4", "wide-64"): [57, 76, 0, 0, 57, 0],
    ("rand4", "wide-130"): [116, 154, 0, 0, 116, 0],
    ("rand4", "mixed-63"): [107, 189, 18, 43, 107, 0],
    ("rand4", "mixed-64"): [109, 196, 18, 44, 109, 0],
    ("rand4", "mixed-65"): [110, 208, 19, 46, 110, 0],
    ("rand4", "mixed-129"): [249, 533, 37, 114, 249, 0],
    ("rand5", "lanes-first"): [777, 2346, 195, 608, 777, 0],
    ("rand5", "lanes-last"): [827, 2515, 192, 658, 827, 0],
    ("rand5", "lanes-alternating"): [773, 2339, 197, 604, 773, 0],
    ("rand5", "wide-64"): [71, 107, 0, 0, 71, 0],
    ("rand5", "wide-130"): [144, 218, 0, 0, 144, 0],
    ("rand5", "mixed-63"): [110, 252, 25, 76, 110, 0],
    ("rand5", "mixed-64"): [111, 258, 26, 78, 111, 0],
    ("rand5", "mixed-65"): [112, 259, 27, 78, 112, 0],
    ("rand5", "mixed-129"): [219, 514, 54, 160, 219, 0],
    ("rand6", "lanes-first"): [303, 327, 244, 126, 303, 0],
    ("rand6", "lanes-last"): [332, 385, 234, 161, 332, 0],
    ("rand6", "lanes-alternating"): [316, 346, 241, 141, 316, 0],
    ("rand6", "wide-64"): [44, 44, 0, 0, 44, 0],
    ("rand6", "wide-130"): [90, 90, 0, 0, 90, 0],
    ("rand6", "mixed-63"): [44, 57, 36, 11, 44, 0],
    ("rand6", "mixed-64"): [45, 59, 37, 12, 45, 0],
    ("rand6", "mixed-65"): [46, 61, 37, 12, 46, 0],
    ("rand6", "mixed-129"): [135, 144, 48, 42, 135, 0],
    ("rand7", "lanes-first"): [341, 462, 136, 231, 341, 0],
    ("rand7", "lanes-last"): [307, 336, 135, 201, 307, 0],
    ("rand7", "lanes-alternating"): [344, 455, 134, 232, 344, 0],
    ("rand7", "wide-64"): [66, 67, 0, 12, 66, 0],
    ("rand7", "wide-130"): [134, 135, 0, 25, 134, 0],
    ("rand7", "mixed-63"): [117, 174, 9, 91, 117, 0],
    ("rand7", "mixed-64"): [119, 175, 9, 92, 119, 0],
    ("rand7", "mixed-65"): [123, 186, 9, 95, 123, 0],
    ("rand7", "mixed-129"): [255, 405, 16, 204, 255, 0],
    ("linear", "lanes-first"): [264, 2089, 237, 351, 256, 8],
    ("linear", "lanes-last"): [237, 2421, 284, 415, 235, 2],
    ("linear", "lanes-alternating"): [260, 2167, 245, 365, 253, 7],
    ("linear", "wide-64"): [77, 114, 0, 0, 64, 13],
    ("linear", "wide-130"): [156, 232, 0, 0, 130, 26],
    ("linear", "mixed-63"): [54, 214, 46, 54, 52, 2],
    ("linear", "mixed-64"): [55, 215, 47, 54, 53, 2],
    ("linear", "mixed-65"): [56, 226, 48, 56, 54, 2],
    ("linear", "mixed-129"): [107, 421, 91, 100, 102, 5],
    ("snp", "lanes-first"): [510, 1998, 234, 428, 502, 8],
    ("snp", "lanes-last"): [533, 2312, 272, 500, 531, 2],
    ("snp", "lanes-alternating"): [532, 2060, 241, 446, 526, 6],
    ("snp", "wide-64"): [77, 114, 0, 0, 64, 13],
    ("snp", "wide-130"): [156, 232, 0, 0, 130, 26],
    ("snp", "mixed-63"): [80, 222, 43, 54, 78, 2],
    ("snp", "mixed-64"): [81, 223, 44, 54, 79, 2],
    ("snp", "mixed-65"): [83, 234, 45, 57, 81, 2],
    ("snp", "mixed-129"): [161, 436, 85, 120, 158, 3],
    ("snp40000", "lanes-first"): [1237, 5855, 187, 896, 933, 304],
    ("snp40000", "lanes-last"): [1336, 6090, 180, 933, 997, 339],
    ("snp40000", "lanes-alternating"): [1260, 6045, 186, 928, 953, 307],
    ("snp40000", "wide-64"): [128, 114, 0, 0, 64, 64],
    ("snp40000", "wide-130"): [260, 232, 0, 0, 130, 130],
    ("snp40000", "mixed-63"): [114, 383, 45, 77, 93, 21],
    ("snp40000", "mixed-64"): [117, 391, 46, 79, 96, 21],
    ("snp40000", "mixed-65"): [118, 423, 47, 84, 97, 21],
    ("snp40000", "mixed-129"): [250, 810, 93, 161, 203, 47],
    ("dbg20", "lanes-first"): [685, 5710, 368, 1072, 685, 0],
    ("dbg20", "lanes-last"): [788, 6650, 368, 1217, 788, 0],
    ("dbg20", "lanes-alternating"): [722, 5940, 368, 1112, 722, 0],
    ("dbg20", "wide-64"): [128, 114, 0, 0, 64, 64],
    ("dbg20", "wide-130"): [260, 232, 0, 0, 130, 130],
    ("dbg20", "mixed-63"): [118, 102, 40, 0, 65, 53],
    ("dbg20", "mixed-64"): [125, 108, 40, 0, 69, 56],
    ("dbg20", "mixed-65"): [125, 108, 41, 0, 69, 56],
    ("dbg20", "mixed-129"): [248, 261, 89, 26, 152, 96],
}


@pytest.fixture(scope="module")
def engine():
    from gcsa2_amd import binding
    assert binding.device_count() >= 1, "no MI355X visible"
    return binding


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def live_lanes(t, placement):
    """Which of the 64 lanes of a wave get a live pattern."""
    if placement == "first":
        return set(range(t))
    if placement == "last":
        return set(range(64 - t, 64))
    order = list(range(0, 64, 2)) + list(range(1, 64, 2))       # every second lane, then the lanes between them
    return set(order[:t])


def batches_of(cpu, walks, seed):
    """(name, patterns) of every batch of one graph."""
    walks = [w for w in walks if len(w) > 0]
    longest = sorted(walks, key=len, reverse=True)[:64]          # patterns that still have characters left after their seed
    out = []
    # 1. stepping-lane counts: one wave per count, the other lanes hold empty patterns (done at the start)
    for placement in PLACEMENTS:
        pats = []
        for t in LIVE_COUNTS:
            live = live_lanes(t, placement)
            assert len(live) == t
            pats += [longest[(lane + t) % len(longest)] if lane in live else b"" for lane in range(64)]
        out.append(("lanes-" + placement, pats))
    # 2. wide ranges: every 2-mer and 3-mer over ACGT; sp and ep + 1 of such a range lie in different blocks
    short = [bytes([a, b]) for a in b"ACGT" for b in b"ACGT"] + [bytes([a, b, c]) for a in b"ACGT" for b in b"ACGT" for c in b"ACGT"]
    for nq in WIDE_SIZES:
        out.append((f"wide-{nq}", [short[(7 * q) % len(short)] for q in range(nq)]))
    # 3. walks interleaved lane by lane with patterns that leave their chain after 0..9 labels
    chained = chain_patterns(cpu, walks, seed)
    leaving = chained[len(walks):]
    for nq in MIXED_SIZES:
        out.append((f"mixed-{nq}", [walks[(q // 2) % len(walks)] if q % 2 == 0 else leaving[(q // 2) % len(leaving)] for q in range(nq)]))
    return out


@pytest.fixture(scope="module")
def prepared(engine):
    """Per graph: the index arrays and, per batch, the concatenated patterns and the oracle's ranges; computed once."""
    from oracle.oracle import OracleIndex
    out = []
    for name, ix, walks in graph_cases():
        cpu = OracleIndex(ix, **FIND_ONLY)
        batches = []
        for bname, pats in batches_of(cpu, walks, 0x5D0 + len(out)):
            data, off = concat_patterns(pats)
            batches.append((bname, data, off, cpu.find_batch(data, off)))
        out.append((name, ix, batches))
    return out


def run_image(gpu, batches, label):
    """find_device equals the oracle and the instrumented twin equals find_device; returns the counters per batch."""
    counters = {}
    for bname, data, off, want in batches:
        batch = DeviceBatch(data, off)
        got = batch.run(lambda p, o, n, r: gpu.find_device(p, o, n, r, 0))
        assert np.array_equal(got, want), (label, bname)
        twin, counters[bname] = batch.stats(gpu)
        assert np.array_equal(twin, got), (label, bname)
    return counters


def test_staged_path(engine, prepared):
    most_second = 0
    for name, ix, batches in prepared:
        gpu = engine.GCSA(ix, **FIND_ONLY)
        assert gpu.jump_table_bytes() == 16 * ix.n, name
        counters = run_image(gpu, batches, name)
        gpu.close()
        for bname, seen in counters.items():
            print(f'    ("{name}", "{bname}"): {seen},')
            blocks, steps, lookups, jumps, fetch_steps, second = seen
            assert blocks == fetch_steps + second, (name, bname, seen)
        most_second = max(most_second, counters["wide-64"][5])
        for bname, seen in counters.items():
            assert seen == PARENT_COUNTERS[(name, bname)], (name, bname, seen, PARENT_COUNTERS[(name, bname)])
    assert most_second > 32, most_second                # a second round with more needing lanes than the smallest stage has slots


def test_without_the_table(engine, prepared, monkeypatch):
    monkeypatch.setenv("GCSA2_JUMP_TABLE", "0")
    for name, ix, batches in prepared:
        gpu = engine.GCSA(ix, **FIND_ONLY)
        assert gpu.jump_table_bytes() == 0, name
        counters = run_image(gpu, batches, name)
        gpu.close()
        assert all(seen[3] == 0 for seen in counters.values()), (name, counters)
