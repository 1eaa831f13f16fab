"""locate() on node_type values of 62 to 64 bits, through every path of the sorted pipeline.

A node_type is 64 bits (a node id shifted left, OR-ed with an offset), and an index is accepted with a sample_width up
to 64.  The locate pipeline has branches of its own for the widest values: bit 63 is the flag of a direct entry of the
locate table (a value >= 2^63 is an indirect entry), fusion is off and the second table pass is forced from 63 bits on,
the device-wide radix sort gives way to the library's segmented sort when a value and a segment rank do not share a
key, and the value 2^64 - 1 is what every sort pads with and what the duplicate filter calls an empty slot.

Four placements of the same graphs' values (m = the graph's largest value before the shift):

    top-of-62    + 2^62 - 1 - m    sample_width 62   the widest index on which fusion still runs
    across-2^62  + 2^62 - m // 2   sample_width 63   direct entries only, but none of the 62-bit shortcuts
    across-2^63  + 2^63 - m // 2   sample_width 64   direct and indirect entries mixed
    top-of-64    + 2^64 - 1 - m    sample_width 64   indirect entries only; the largest value is 2^64 - 1

The CPU tests pin the oracle at these widths against the two naive references; the GPU tests then compare with the
oracle bit for bit (offsets and values, no tolerance)."""
import functools

import numpy as np
import pytest

from workload import graphs
from workload.rng import SplitMix64
from gcsa2_amd.hostview import concat_patterns
from naive import NaiveIndex, GraphBrute
from test_gpu_parity import engine, all_ranges        # noqa: F401  (engine: the fixture)

gpu_test = pytest.mark.gpu

COMP2CHAR = b"$ACGTN#"
ONES = (1 << 64) - 1
PLACEMENTS = {"top-of-62": (lambda m: (1 << 62) - 1 - m, 62),
              "across-2^62": (lambda m: (1 << 62) - m // 2, 63),
              "across-2^63": (lambda m: (1 << 63) - m // 2, 64),
              "top-of-64": (lambda m: (1 << 64) - 1 - m, 64)}
NAMES = list(PLACEMENTS)
BIG = 8192                                           # values the LDS hash set and the workgroup sort hold


def shifted(g, placement):
    shift = PLACEMENTS[placement][0](int(g.value.max()))
    g.value += np.uint64(shift)
    return g


def shuffled(ranges, rng):
    order = list(range(len(ranges)))
    for k in range(len(order) - 1, 0, -1):
        j = rng.below(k + 1)
        order[k], order[j] = order[j], order[k]
    return np.array([ranges[k] for k in order], dtype=np.uint64)


def unsorted_csr(cpu, arr):
    """The oracle's locate(range, sort=False) of every range, as one CSR."""
    parts = [np.asarray(cpu.locate((int(a), int(b)), sort=False), dtype=np.uint64) for a, b in arr]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    return off, (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64))


# ---- the indexes and what the oracle says about them: made once per placement, never changed afterwards ----------------

@functools.lru_cache(maxsize=None)
def linear_index(placement):
    """The index of test_locate_many_large_distinct_segments (a linear text: one value per path node), values shifted."""
    from oracle.oracle import OracleIndex
    from workload import builder
    g = shifted(graphs.linear_graph(70000, 0x4E1, node_len=32), placement)
    ix = builder.build(g, 16, sample_period=32)
    return g, ix, OracleIndex(ix)


@functools.lru_cache(maxsize=None)
def linear_segments(placement):
    """The 67 ranges of test_locate_many_large_distinct_segments (same widths, seeds and shuffle) with the oracle's sorted and
    unsorted results."""
    g, ix, cpu = linear_index(placement)
    rng = SplitMix64(0x4E2)
    ranges = []
    for width in (8193, 8500, 9000, 12000, 16384, 20000, 33000, 50000, 3, 1, 700, 4097, 5000):
        for _ in range(5):
            a = rng.below(ix.n - width)
            ranges.append((a, a + width - 1))
    ranges += [(0, ix.n - 1), (9, 8)]
    arr = shuffled(ranges, rng)
    co, cv = cpu.locate_batch(arr, threads=8)
    uo, uv = unsorted_csr(cpu, arr)
    for a in (arr, co, cv, uo, uv):
        a.setflags(write=False)
    return arr, co, cv, uo, uv


@functools.lru_cache(maxsize=None)
def linear_node_values(placement):
    """The value of every path node of the linear index: one oracle batch over all n one-node ranges."""
    g, ix, cpu = linear_index(placement)
    nodes = np.arange(ix.n, dtype=np.uint64)
    off, values = cpu.locate_batch(np.stack([nodes, nodes], axis=1), threads=8)
    assert np.array_equal(off, np.arange(ix.n + 1, dtype=np.uint64)), "a linear text: one value per path node"
    values.setflags(write=False)
    return values


@functools.lru_cache(maxsize=None)
def snp_index(placement):
    """The duplicate-rich index of test_locate_segment_sizes, values shifted."""
    from oracle.oracle import OracleIndex
    from workload import builder
    g = shifted(graphs.snp_graph(30000, 0x4D1, 0x4D2, snp_period=5, node_len=16), placement)
    ix = builder.build(g, 16, sample_period=16)
    return g, ix, OracleIndex(ix)


@functools.lru_cache(maxsize=None)
def snp_segments(placement):
    """The ranges of test_locate_segment_sizes (same widths, seeds and shuffle) with the oracle's results."""
    g, ix, cpu = snp_index(placement)
    rng = SplitMix64(0x4D3)
    ranges = []
    for width in (1, 2, 3, 8, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 150, 191, 192, 193, 200, 257, 300, 383, 384, 385, 511, 512, 513, 900, 1023, 1024, 1025, 1500, 2047, 2048, 2049, 3000,
                  4096, 4097, 7000, 8191, 8192, 8193, 9000, 20000):
        for _ in range(6):
            a = rng.below(ix.n - width)
            ranges.append((a, a + width - 1))
    ranges += [(0, ix.n - 1), (5, 4), (ix.n, ix.n + 3)]
    arr = shuffled(ranges, rng)
    co, cv = cpu.locate_batch(arr, threads=8)
    uo, uv = unsorted_csr(cpu, arr)
    counts = cpu.count_batch(arr)
    modest = arr[(arr[:, 1] - arr[:, 0] < 5000) | (arr[:, 0] > arr[:, 1])]
    mo, mv = cpu.locate_batch(modest, threads=8)
    for a in (arr, co, cv, uo, uv, counts, modest, mo, mv):
        a.setflags(write=False)
    return arr, co, cv, uo, uv, counts, modest, mo, mv


def text_read(g, start, length):
    """`length` bases of the linear graph's text (position 0 is the source marker)."""
    return bytes(COMP2CHAR[int(c)] for c in g.comp[1 + start:1 + start + length])


def sides_of(values, bit):
    """(some value below 2^bit, some value at or above it)"""
    high = (values >> np.uint64(bit)) != 0
    return bool((~high).any()), bool(high.any())


# ---- CPU: the oracle is right at these widths ---------------------------------------------------------------------------

@pytest.mark.parametrize("placement", NAMES)
def test_oracle_equals_the_graph_at_wide_values(placement):
    """locate(find(p)) of the oracle on the shifted linear graph is what the graph itself says (GraphBrute: the values of
    the positions at which a path labelled p starts), for patterns with 17572, 4407 and 1129 occurrences and two 16-mers cut
    from the text; the stored samples have the width the placement is named for."""
    g, ix, cpu = linear_index(placement)
    width = PLACEMENTS[placement][1]
    assert ix.n == 70002 and ix.sample_width == width
    assert int(g.value.max()).bit_length() == width
    brute = GraphBrute(g)
    pats = [b"A", b"AC", b"GAT", text_read(g, 1234, 16), text_read(g, 65000, 16)]
    for p, most in zip(pats, (None, None, None, 2, 2)):
        comps = [int(ix.char2comp[b]) for b in p]
        want = brute.occurrences(comps)
        got = [int(v) for v in cpu.locate(cpu.find(p))]
        assert got == want and len(got) > 0, (placement, p)
        assert most is None or len(got) <= most, (placement, p)
    if placement == "top-of-64":
        assert int(g.value.max()) == ONES
    # every path node on its own: the oracle's values are values of the graph
    assert set(int(v) for v in linear_node_values(placement)) <= set(int(v) for v in g.value)


@pytest.mark.parametrize("placement", NAMES)
def test_oracle_equals_the_naive_index_at_wide_values(placement):
    """On a 300-base SNP graph (the index of smoke(), values shifted) the oracle's locate() equals the pseudocode evaluated with
    plain scans (NaiveIndex, Python integers: no 64-bit arithmetic to get wrong), for every one-node range, the whole index
    and 200 short ranges, sorted and in path order."""
    from oracle.oracle import OracleIndex
    from workload.brute_builder import build as brute_build
    g = shifted(graphs.snp_graph(300, 0x51, 0x52, snp_period=8, node_len=8), placement)
    ix = brute_build(g, 8, sample_period=8, branching=4)
    assert ix.sample_width == PLACEMENTS[placement][1]
    cpu, naive = OracleIndex(ix), NaiveIndex(ix)
    several = 0
    for r in all_ranges(ix, 0x3E1):
        for sort in (True, False):
            want = naive.locate(r, sort=sort)
            got = [int(v) for v in cpu.locate(r, sort=sort)]
            assert got == want, (placement, r, sort)
        several += int(r[0] == r[1] and len(want) > 1)
    assert several > 0, "the graph has path nodes with several values"
    # (the graph is small: its values lie on both sides of the placement's power of two, or all in the top bit of the width)
    lo, hi = sides_of(np.asarray(cpu.locate((0, ix.n - 1))), PLACEMENTS[placement][1] - 1)
    assert hi and lo == placement.startswith("across")


def linear_preconditions(placement):
    """What test_large_distinct_segments rests on, said of the oracle's output alone."""
    g, ix, cpu = linear_index(placement)
    arr, co, cv, uo, uv = linear_segments(placement)
    assert ix.sample_width == PLACEMENTS[placement][1]
    assert int((np.diff(co) > BIG).sum()) >= 40 and int(np.diff(co).max()) == ix.n
    assert np.array_equal(uo, co), "a linear text: nothing to deduplicate"
    for q in np.flatnonzero(np.diff(co) > BIG):
        seg = cv[int(co[q]):int(co[q + 1])]
        assert bool((seg[1:] > seg[:-1]).all()), "strictly increasing"
        if placement == "across-2^63":
            assert int(seg[0]) >> 63 == 0 and int(seg[-1]) >> 63 == 1
        if placement == "top-of-62":
            assert int(seg[-1]) >> 62 == 0
    if placement == "top-of-64":
        assert int(cv.max()) == ONES and int(cv.min()) >> 63 == 1


def snp_preconditions(placement):
    """What test_every_segment_size_class_with_duplicates rests on."""
    g, ix, cpu = snp_index(placement)
    arr, co, cv, uo, uv, counts, modest, mo, mv = snp_segments(placement)
    assert ix.sample_width == PLACEMENTS[placement][1]
    # the whole-index range overflows the duplicate filter, the modest batch stays within the LDS sorts, and most raw values
    # are duplicates
    assert int(np.diff(co).max()) > 4 * BIG and 1024 < int(np.diff(mo).max()) <= BIG and int(uo[-1]) > 2 * int(co[-1])
    if placement == "top-of-64":
        assert int(cv.max()) == ONES and int(cv.min()) >> 63 == 1
    if placement == "across-2^63":
        assert sides_of(cv, 63) == (True, True)


@functools.lru_cache(maxsize=None)
def padding_value_batch():
    """Ranges of every size class around the path node whose value is 2^64 - 1 (linear graph, top-of-64; at a seeded position
    inside the range), each followed by a range of the same width without it: (ranges, which hold it, sorted CSR, unsorted
    CSR)."""
    g, ix, cpu = linear_index("top-of-64")
    values = linear_node_values("top-of-64")
    assert len(values) == 70002
    at = np.flatnonzero(values == np.uint64(ONES))
    assert len(at) == 1
    p, n = int(at[0]), ix.n
    rng = SplitMix64(0x4E7)
    ranges, holds = [], []
    for width in (1, 2, 16, 17, 64, 65, 512, 513, 1024, 1025, 4096, 4097, 8192, 8193, 20000):
        a = min(max(p - rng.below(width), 0), n - width)
        assert 0 <= a <= p <= a + width - 1 <= n - 1
        ranges.append((a, a + width - 1)); holds.append(True)
        while True:
            a = rng.below(n - width + 1)
            if not a <= p <= a + width - 1:
                break
        ranges.append((a, a + width - 1)); holds.append(False)
    arr = np.array(ranges, dtype=np.uint64)
    co, cv = cpu.locate_batch(arr, threads=8)
    uo, uv = unsorted_csr(cpu, arr)
    assert np.array_equal(np.diff(co), arr[:, 1] - arr[:, 0] + np.uint64(1))
    for q, with_p in enumerate(holds):
        assert (int(cv[int(co[q + 1]) - 1]) == ONES) == with_p, arr[q]
    for a in (arr, co, cv, uo, uv):
        a.setflags(write=False)
    return arr, holds, co, cv, uo, uv


@functools.lru_cache(maxsize=None)
def one_value_batch(placement):
    """20 000 one-node ranges of the linear index and the oracle's CSR."""
    g, ix, cpu = linear_index(placement)
    rng = SplitMix64(0x4E9)
    pick = np.array([rng.below(ix.n) for _ in range(20000)], dtype=np.uint64)
    arr = np.stack([pick, pick], axis=1)
    co, cv = cpu.locate_batch(arr, threads=8)
    assert np.array_equal(co, np.arange(len(arr) + 1, dtype=np.uint64)) and np.array_equal(cv, linear_node_values(placement)[pick])
    if placement == "across-2^63":
        assert sides_of(cv, 63) == (True, True)                 # direct and indirect table entries
    if placement == "top-of-64":
        assert sides_of(cv, 63) == (False, True)                # no direct entry
    for a in (arr, co, cv):
        a.setflags(write=False)
    return arr, co, cv


@pytest.mark.parametrize("placement", NAMES)
def test_gpu_cases_rest_on_what_they_claim(placement):
    """Everything the GPU tests below assume of their inputs, checked on the oracle's output alone (the GPU tests assert the
    same again, so that a changed generator cannot turn one of them into a test of nothing)."""
    linear_preconditions(placement)
    snp_preconditions(placement)
    one_value_batch(placement)
    g, ix, cpu = snp_index(placement)
    assert ix.n == 175249
    whole = np.asarray(cpu.locate((0, ix.n - 1)))
    assert len(whole) == 36031 and bool((whole[1:] > whole[:-1]).all())
    if placement == "across-2^63":
        assert 0.45 < float((whole >> np.uint64(63)).mean()) < 0.55
    if placement == "top-of-64":
        assert int(whole[-1]) == ONES and int(whole[0]) >> 63 == 1
        arr, holds, co, cv, uo, uv = padding_value_batch()
        assert sum(holds) == 15 and len(arr) == 30


# ---- GPU ----------------------------------------------------------------------------------------------------------------

KNOBS = [{}, {"GCSA2_SPLIT_TARGET": "24"}, {"GCSA2_SPLIT_TARGET": "1500", "GCSA2_SPLIT_SKEW": "700"}, {"GCSA2_SPLIT_SKEW": "16"},
         {"GCSA2_LOCATE_FUSED_COMPACT": "0"}, {"GCSA2_LOCATE_IN_PLACE": "0"}, {"GCSA2_LOCATE_FUSE_ABOVE": "600"}, {"walk": "1"}]
KNOB_IDS = ["split-with-listed-buckets", "split-with-runs", "split-with-listed-and-skewed-buckets", "split-with-skewed-buckets",
            "four-kernel-compaction", "sorts-in-scratch", "fused-from-600-nodes", "walk-without-table"]


def assert_unsorted(go, gv, uo, uv, arr):
    assert np.array_equal(go, uo)
    for q in range(len(arr)):
        assert np.array_equal(gv[int(go[q]):int(go[q + 1])], uv[int(uo[q]):int(uo[q + 1])]), arr[q]


@gpu_test
@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
@pytest.mark.parametrize("placement", NAMES)
def test_large_distinct_segments(engine, placement, knobs, monkeypatch):
    """Dozens of segments of more than 8192 DISTINCT values each (k_over_split and what it lists: the bucket sorts, the
    workgroup sort, and -- with the skew knobs, at 63 and 64 bits -- the library's segmented sort, since a value of 64 or 65
    key bits leaves no room for the segment's rank), read from the raw values (fusion is off from 63 bits on) or from the
    locate table (top-of-62), sorted in the caller's buffer or in scratch, compacted by either compaction, with and without
    the locate table: sorted and unsorted, through the job interface and into a caller's buffer."""
    import torch
    knobs = dict(knobs)
    walk = knobs.pop("walk", None)
    for key, value in knobs.items():
        monkeypatch.setenv(key, value)
    g, ix, cpu = linear_index(placement)
    arr, co, cv, uo, uv = linear_segments(placement)
    linear_preconditions(placement)
    gpu, lcp = engine.open_index(ix)
    assert gpu.sampleBits() == PLACEMENTS[placement][1]
    if walk:
        gpu.set_tables(locate_table=0)
        assert gpu.locate_table_bytes() == 0
    go, gv = gpu.locate_batch(arr)
    assert np.array_equal(go, co) and np.array_equal(gv, cv)
    go, gv = gpu.locate_batch(arr, sort=False)
    assert_unsorted(go, gv, uo, uv, arr)
    dev = torch.device("cuda", 0)
    d_r = torch.from_numpy(arr.view(np.int64).copy()).to(dev)
    d_o = torch.full((len(arr) + 1,), -1, dtype=torch.int64, device=dev)
    d_v = torch.full((len(cv) + 7,), -1, dtype=torch.int64, device=dev)
    total = gpu.locate_into(d_r.data_ptr(), len(arr), d_o.data_ptr(), d_v.data_ptr(), d_v.shape[0])
    torch.cuda.synchronize()
    assert total == len(cv) and np.array_equal(d_o.cpu().numpy().view(np.uint64), co)
    # (the values are all distinct, so nothing lies between the total and the capacity: the seven words behind are the caller's)
    assert np.array_equal(d_v.cpu().numpy().view(np.uint64)[:total], cv) and bool((d_v[total:] == -1).all())
    gpu.close()


@gpu_test
@pytest.mark.parametrize("placement", NAMES)
def test_every_segment_size_class_with_duplicates(engine, placement):
    """removeDuplicates at every segment size class (test_locate_segment_sizes' ranges: 1 value, registers, one wavefront,
    one workgroup, the duplicate filter, the split sort) on a repetitive SNP graph.  across-2^63: the filter's 64-bit table
    takes a mix of direct and indirect table entries; top-of-64: indirect entries only, and 2^64 - 1 -- the filter's mark of
    an empty slot -- is a value of the whole-index range.  And the sub-batch without a segment beyond 8192 values."""
    g, ix, cpu = snp_index(placement)
    arr, co, cv, uo, uv, counts, modest, mo, mv = snp_segments(placement)
    snp_preconditions(placement)
    gpu, lcp = engine.open_index(ix)
    assert gpu.sampleBits() == PLACEMENTS[placement][1]
    go, gv = gpu.locate_batch(arr)
    assert np.array_equal(go, co) and np.array_equal(gv, cv)
    assert np.array_equal(gpu.count_batch(arr), counts)
    go, gv = gpu.locate_batch(arr, sort=False)
    assert_unsorted(go, gv, uo, uv, arr)
    go, gv = gpu.locate_batch(modest)
    assert np.array_equal(go, mo) and np.array_equal(gv, mv)
    gpu.close()


@gpu_test
def test_the_padding_value_in_every_size_class(engine):
    """Every sort pads a short segment with 2^64 - 1.  Here that is a real value: ranges of every size class around the one
    path node that has it, each next to a range of the same width without it."""
    g, ix, cpu = linear_index("top-of-64")
    arr, holds, co, cv, uo, uv = padding_value_batch()
    gpu, lcp = engine.open_index(ix)
    go, gv = gpu.locate_batch(arr)
    assert np.array_equal(go, co) and np.array_equal(gv, cv)
    for q, with_p in enumerate(holds):
        assert (int(gv[int(go[q + 1]) - 1]) == ONES) == with_p, arr[q]
    go, gv = gpu.locate_batch(arr, sort=False)
    assert_unsorted(go, gv, uo, uv, arr)
    gpu.close()


@gpu_test
@pytest.mark.parametrize("single", ["1", "0"], ids=["one-kernel-path", "general-pipeline"])
@pytest.mark.parametrize("placement", NAMES)
def test_one_value_batches(engine, placement, single, monkeypatch):
    """20 000 one-node ranges.  The one-kernel path (k_locate_single) answers from direct table entries only: across-2^63
    every other entry is indirect, so it meets a misfit and the handle backs off for the next calls; top-of-64 no entry is
    direct.  Three calls on one handle cross the back-off counter."""
    monkeypatch.setenv("GCSA2_LOCATE_SINGLE", single)
    g, ix, cpu = linear_index(placement)
    arr, co, cv = one_value_batch(placement)
    gpu, lcp = engine.open_index(ix)
    assert gpu.sampleBits() == PLACEMENTS[placement][1]
    for call in range(3):
        go, gv = gpu.locate_batch(arr)
        assert np.array_equal(go, co) and np.array_equal(gv, cv), call
    go, gv = gpu.locate_batch(arr, sort=False)
    assert np.array_equal(go, co) and np.array_equal(gv, cv)
    gpu.close()


@gpu_test
@pytest.mark.parametrize("placement", ["across-2^63", "top-of-64"])
def test_hit_families_inherit_the_pipeline(engine, placement):
    """The k-mer hits and the MEM hits of one 40-base read cut from the text locate through the same pipeline: every window's
    hits are locate(find(window)) of the oracle -- the 1-mers have thousands of hits each, `A` more than 8192 -- and the MEM
    hits are what tests/test_mem_hits.py expects."""
    from test_mem_hits import Oracle, assert_same
    g, ix, cpu = linear_index(placement)
    read = text_read(g, 31000, 40)
    assert len(read) == 40 and b"A" in read
    data, off = concat_patterns([read])
    gpu, lcp = engine.open_index(ix)
    most = 0
    for k in (1, 2):
        soff, seeds, hoff, hits = gpu.kmer_hits_batch(data, off, k, hit_max=0)
        windows = [read[j:j + k] for j in range(len(read) - k + 1)]
        assert soff.tolist() == [0, len(windows)] and len(seeds) == len(windows)
        for j, w in enumerate(windows):
            r = cpu.find(w)
            want = np.asarray(cpu.locate(r), dtype=np.uint64)
            assert tuple(int(x) for x in seeds[j]) == (j, k, r[0], r[1], cpu.count(r)), (k, j)
            assert np.array_equal(hits[int(hoff[j]):int(hoff[j + 1])], want), (k, j, w)
            most = max(most, len(want))
    assert most > BIG
    want = Oracle(cpu, [read]).expected(1, 0, False)
    assert len(want[1]) > 0 and len(want[3]) > 0
    assert_same(gpu.mem_hits_batch(data, off, 1, hit_max=0), want, placement)
    gpu.close()
