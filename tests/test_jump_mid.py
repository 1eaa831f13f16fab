"""jump_mid: the middle node slot of a jump entry holds the node after 2 or after 6 steps (kernels_find.hpp).  With 6 a
lane takes {len, 6, 4} steps per lookup and looks up only with 4 or more characters left; with 2 it takes {len, 4, 2} as
before.  Ranges are the oracle's under either value and either builder, the counters that are functions of the batch do
not move, the lookups and steps of a full chain follow from the take rule in closed form, and a small image keeps 2 by
default: the pinned counters of tests/test_find_lds_stage.py stand."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gcsa2_amd.hostview import concat_patterns
from test_find_only_jump import FIND_ONLY, DeviceBatch, chain_patterns, graph_cases
from test_find_lds_stage import PARENT_COUNTERS, batches_of

ENV = ("GCSA2_JUMP_TABLE", "GCSA2_JUMP_BUILD", "GCSA2_JUMP_MID", "GCSA2_KMER_TABLE", "GCSA2_PAIR_BLOCKS", "GCSA2_MEMORY_BUDGET_MB")
SIZES = (1, 63, 64, 65, 129)
LEFT = range(2, 18)             # characters left at a lane's first lookup: every tail 0..7 behind a full chain, twice
JUMP_MAX = 8


@pytest.fixture(scope="module")
def engine():
    from gcsa2_amd import binding
    assert binding.device_count() >= 1, "no MI355X visible"
    return binding


@contextlib.contextmanager
def env(**settings):
    """The knobs of index creation, set for one block: every name of ENV is unset but the ones given."""
    saved = {name: os.environ.pop(name, None) for name in ENV}
    try:
        for name, value in settings.items():
            assert name in ENV, name
            os.environ[name] = value
        yield
    finally:
        for name, value in saved.items():
            os.environ.pop(name, None)
            if value is not None:
                os.environ[name] = value


def create(engine, ix, **settings):
    with env(**settings):
        return engine.GCSA(ix, **FIND_ONLY)


def left_at_first_single(k, length, s):
    """Characters left when k_find2 first holds a range of one node, for a pattern over ACGT that occurs: it consumes the
    seed (k characters, when the pattern has that many; else one) and then two characters per pair step, one when one is
    left; `s` is the number of characters after which the range is one node.  None: never before the pattern ends."""
    c = k if 0 < k <= length else 1
    while c < s and c < length:
        c += 2 if length - c >= 2 else 1
    return length - c if c >= s and c < length else None


def single_after(cpu, texts):
    """Per text: the number of characters, read from its end, after which its range is one node (None: never, or the
    text does not occur).  The ranges of all suffixes in one oracle batch."""
    suffixes = [t[len(t) - c:] for t in texts for c in range(1, len(t) + 1)]
    data, off = concat_patterns(suffixes)
    ranges = cpu.find_batch(data, off)
    out, at = [], 0
    for t in texts:
        rows = ranges[at:at + len(t)]
        at += len(t)
        occurs = len(t) > 0 and int(rows[-1][0]) <= int(rows[-1][1])
        single = [c for c in range(1, len(t) + 1) if int(rows[c - 1][0]) == int(rows[c - 1][1])]
        out.append(single[0] if occurs and single else None)
    return out


def counts_of_tail(r, mid):
    """(lookups of the jump table, steps that fetch a block) of a lane that holds one node with r characters left on
    forced chains of JUMP_MAX or more nodes, from the take rule: an entry offers all 8 steps or a prefix of {4, 2}
    (mid = 2) or {6, 4} (mid = 6) of them, and is looked up only with at least the shorter prefix left; what is left
    then goes by a pair step, or by a single step when it is one character."""
    hi, lo = (6, 4) if mid == 6 else (4, 2)
    jumps = steps = 0
    while r > 0:
        if r >= lo:
            jumps += 1
            r -= JUMP_MAX if r >= JUMP_MAX else (hi if r >= hi else lo)
        else:
            steps += 1
            r -= 2 if r >= 2 else 1
    return jumps, steps


def test_take_rule_model():
    """The issue's table of requests per tail, from counts_of_tail."""
    assert [sum(counts_of_tail(r, 2)) for r in range(1, 8)] == [1, 1, 2, 1, 2, 2, 3]
    assert [sum(counts_of_tail(r, 6)) for r in range(1, 8)] == [1, 1, 2, 1, 2, 1, 2]


@pytest.fixture(scope="module")
def cases(engine):
    """Per graph of graph_cases: index arrays, oracle, walks.  Built once and left unchanged."""
    from oracle.oracle import OracleIndex
    return [(name, ix, OracleIndex(ix, **FIND_ONLY), [w for w in walks if len(w) > 0]) for name, ix, walks in graph_cases()]


@pytest.fixture(scope="module")
def prepared(engine, cases):
    """Per graph: the batches of the equivalence test with the oracle's ranges, and what the image with mid = 2 (the
    default) and the image without the table return for them."""
    out = []
    for at, (name, ix, cpu, walks) in enumerate(cases):
        plain = create(engine, ix)
        bare = create(engine, ix, GCSA2_JUMP_TABLE="0")
        assert plain.jump_mid() == 2 and plain.jump_table_bytes() == 16 * ix.n and bare.jump_table_bytes() == 0, name
        k = plain.kmer_table_k()
        assert bare.kmer_table_k() == k, name
        # suffixes of walks over ACGT, by the characters left at the first lookup
        texts = sorted(set(w for w in walks if set(w) <= set(b"ACGT")), key=lambda w: (-len(w), w))[:120]
        by_left = {}
        for w, s in zip(texts, single_after(cpu, texts)):
            for length in range(1, len(w) + 1):
                left = left_at_first_single(k, length, s) if s is not None else None
                if left in LEFT and len(by_left.setdefault(left, [])) < 2:
                    by_left[left].append(w[len(w) - length:])
        # one pattern per value first, so that every batch of a wave or more holds them all; then patterns that leave their chain
        pool = [(by_left[left][j], left) for j in range(2) for left in sorted(by_left) if j < len(by_left[left])]
        pool += [(p, None) for p in chain_patterns(cpu, walks, 0x6D0 + at)[len(walks):][:90] + [b"", b"N", b"A"]]
        lefts = set(left for p, left in pool[:SIZES[1]] if left is not None)
        batches = []
        for nq in SIZES:
            pats = [pool[q % len(pool)][0] for q in range(nq)]
            data, off = concat_patterns(pats)
            batch = DeviceBatch(data, off)
            want = cpu.find_batch(data, off)
            entry = {"nq": nq, "data": data, "off": off, "want": want}
            for label, gpu in (("plain", plain), ("bare", bare)):
                got = batch.run(lambda p, o, n, r: gpu.find_device(p, o, n, r, 0))
                assert np.array_equal(got, want), (name, nq, label)
                twin, entry[label] = batch.stats(gpu)
                assert np.array_equal(twin, want), (name, nq, label)
            batches.append(entry)
        plain.close()
        bare.close()
        out.append((name, ix, lefts, batches))
    return out


def test_lengths_cover_every_tail(prepared):
    seen = set()
    for name, ix, lefts, batches in prepared:
        print(f"    {name}: characters left at the first lookup {sorted(lefts)}")
        seen |= lefts
    assert seen >= set(LEFT), sorted(set(LEFT) - seen)
    # the walks of the two larger graphs are long enough for every value on one image
    for name, ix, lefts, batches in prepared:
        if name in ("snp40000", "dbg20"):
            assert lefts >= set(LEFT), (name, sorted(set(LEFT) - lefts))


@pytest.mark.parametrize("how", ["double", "walk"])
def test_equivalence(engine, prepared, how):
    moved = 0
    for name, ix, lefts, batches in prepared:
        gpu = create(engine, ix, GCSA2_JUMP_MID="6", GCSA2_JUMP_BUILD=how)
        assert gpu.jump_mid() == 6 and gpu.jump_table_bytes() == 16 * ix.n, (name, how)
        for entry in batches:
            batch, want, nq = DeviceBatch(entry["data"], entry["off"]), entry["want"], entry["nq"]
            got = batch.run(lambda p, o, n, r: gpu.find_device(p, o, n, r, 0))
            assert np.array_equal(got, want), (name, how, nq)                       # the oracle's, hence both other images'
            twin, seen = batch.stats(gpu)
            assert np.array_equal(twin, want), (name, how, nq)
            blocks, steps, lookups, jumps, fetch_steps, second = seen
            assert blocks == fetch_steps + second, (name, how, nq, seen)
            plain, bare = entry["plain"], entry["bare"]
            assert plain[0] == plain[4] + plain[5] and bare[0] == bare[4] + bare[5] and bare[3] == 0, (name, nq, plain, bare)
            assert steps == plain[1] and lookups == plain[2] == bare[2], (name, how, nq, seen, plain, bare)     # functions of the batch
            moved += (jumps, fetch_steps) != (plain[3], plain[4])
        gpu.close()
    assert moved > 0, moved             # the take rule was exercised: some batch's lookups and steps differ from mid = 2


@pytest.fixture(scope="module")
def linear(engine):
    """An unbranched graph of 3000 random bases (every node forced, every chain full away from the source): its sequence,
    index arrays and oracle, and the end positions of the test's substrings with the number of characters after which the
    range of a substring that ends there is one node."""
    from oracle.oracle import OracleIndex
    from workload import builder, graphs
    n = 3000
    g = graphs.linear_graph(n, 0x6A1, node_len=16)
    seq = bytes(b"$ACGTN#"[int(c)] for c in g.comp[1:n + 1])
    assert set(seq) <= set(b"ACGT")
    ix = builder.build(g, 16, sample_period=16, branching=8)
    cpu = OracleIndex(ix, **FIND_ONLY)
    ends = list(range(200, n - 50, 53))
    reach = 24
    singles = single_after(cpu, [seq[e - reach:e] for e in ends])
    assert all(s is not None for s in singles), singles
    return seq, ix, cpu, ends, singles


def test_closed_form_counters(engine, linear):
    seq, ix, cpu, ends, singles = linear
    images = {2: create(engine, ix), 6: create(engine, ix, GCSA2_JUMP_MID="6")}
    k = images[2].kmer_table_k()
    assert images[2].jump_mid() == 2 and images[6].jump_mid() == 6 and images[6].kmer_table_k() == k and k > 0
    assert images[2].pair_block_bytes() > 0 and images[6].pair_block_bytes() > 0
    for r in range(1, 25):
        pats, before = [], 0              # `before`: pair steps between the seed and the first range of one node
        for e, s in zip(ends, singles):
            for length in range(k, k + r + 24):
                if left_at_first_single(k, length, s) == r:
                    pats.append(seq[e - length:e])
                    before += (length - r - k) // 2
                    assert (length - r - k) % 2 == 0 and e - length >= 100
                    break
        assert len(pats) == len(ends), (r, len(pats))
        data, off = concat_patterns(pats)
        want = cpu.find_batch(data, off)
        assert all(int(a) == int(b) for a, b in want), r                    # every pattern occurs, once
        batch = DeviceBatch(data, off)
        total = {}
        for mid, gpu in images.items():
            got, seen = batch.stats(gpu)
            assert np.array_equal(got, want), (r, mid)
            blocks, steps, lookups, jumps, fetch_steps, second = seen
            tail_jumps, tail_steps = counts_of_tail(r, mid)
            print(f"    r = {r}, mid = {mid}: jumps {jumps}, fetch_steps {fetch_steps}; "
                  f"closed form {len(pats) * tail_jumps}, {before + len(pats) * tail_steps}")
            assert lookups == len(pats) and steps == sum(len(p) - k for p in pats), (r, mid, seen)
            assert jumps == len(pats) * tail_jumps, (r, mid, seen)
            assert fetch_steps == before + len(pats) * tail_steps, (r, mid, seen)
            assert blocks == fetch_steps + second, (r, mid, seen)
            total[mid] = jumps + fetch_steps
        if r % 8 in (6, 7):
            assert total[6] < total[2], (r, total)
        else:
            assert total[6] == total[2], (r, total)
    for gpu in images.values():
        gpu.close()


def test_default(engine, cases):
    # the host side of the rule: 6 where the table (16 bytes per path node) is larger than 256 MiB and pair blocks exist
    line = (256 << 20) // 16
    assert engine.jump_mid_default(line, True) == 2 and engine.jump_mid_default(line + 1, True) == 6
    assert engine.jump_mid_default(line + 1, False) == 2 and engine.jump_mid_default(1 << 36, False) == 2
    assert engine.jump_mid_default(0, True) == 2 and engine.jump_mid_default(1 << 30, True) == 6
    assert engine.jump_mid_default(5_726_623_061, True) == 6
    for at, (name, ix, cpu, walks) in enumerate(cases):
        assert 16 * ix.n <= (256 << 20), name
        for settings, mid in (({}, 2), ({"GCSA2_JUMP_MID": "6"}, 6), ({"GCSA2_JUMP_MID": "2"}, 2), ({"GCSA2_JUMP_MID": "4"}, 2),
                              ({"GCSA2_JUMP_MID": "66"}, 2), ({"GCSA2_JUMP_MID": ""}, 2), ({"GCSA2_JUMP_TABLE": "0", "GCSA2_JUMP_MID": "6"}, 2)):
            if at >= 3 and settings:                    # every graph's default; the knob on three of them
                continue
            gpu = create(engine, ix, **settings)
            assert gpu.jump_mid() == mid and (gpu.jump_table_bytes() > 0) == ("GCSA2_JUMP_TABLE" not in settings), (name, settings)
            gpu.close()
    # the default image still counts what tests/test_find_lds_stage.py pins
    at = [name for name, ix, cpu, walks in cases].index("linear")
    name, ix, cpu, walks = cases[at]
    gpu = create(engine, ix)
    for bname, pats in batches_of(cpu, walks, 0x5D0 + at):
        if bname in ("mixed-129", "lanes-alternating"):
            data, off = concat_patterns(pats)
            got, seen = DeviceBatch(data, off).stats(gpu)
            assert np.array_equal(got, cpu.find_batch(data, off)), bname
            assert seen == PARENT_COUNTERS[(name, bname)], (bname, seen)
    gpu.close()
