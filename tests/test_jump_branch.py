"""Branch records: with jump_mid = 6 the jump entry of a chain of at most 3 forced steps that stops in front of a node with
exactly two incoming labels, both fast characters, keeps the two predecessors of that node in its two unused node slots
(kernels_find.hpp).  A lane whose pattern follows the forced part and continues with either label takes len + 1 steps
from one lookup; in every other case the record is the ordinary entry of len steps.  Ranges are the oracle's under either
builder; the lookups and block steps of a lane follow from the rule, which a replica of the lane's decisions (no library
code: in-label sets from the index arrays, the node after each suffix from the oracle) predicts exactly; records are off
on every small image unless GCSA2_JUMP_BRANCH=1 and GCSA2_JUMP_MID=6 say otherwise."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gcsa2_amd.hostview import concat_patterns
from workload.index_arrays import unpack_bits
from test_find_only_jump import FIND_ONLY, DeviceBatch, chain_patterns, graph_cases
from test_find_lds_stage import PARENT_COUNTERS, batches_of

ENV = ("GCSA2_JUMP_TABLE", "GCSA2_JUMP_BUILD", "GCSA2_JUMP_MID", "GCSA2_JUMP_BRANCH", "GCSA2_KMER_TABLE", "GCSA2_PAIR_BLOCKS",
       "GCSA2_MEMORY_BUDGET_MB")
SIZES = (1, 63, 64, 65, 129)
LEFT = range(4, 18)             # characters left at a lane's first lookup
JUMP_MAX, BRANCH_MAX, TAKE_HI, TAKE_LO = 8, 3, 6, 4
FAST = (1, 2, 3, 4)             # comps of A, C, G, T
RECORDS = {"GCSA2_JUMP_MID": "6", "GCSA2_JUMP_BRANCH": "1"}
NO_RECORDS = {"GCSA2_JUMP_MID": "6", "GCSA2_JUMP_BRANCH": "0"}
ONE_CHARACTER_STEPS = {"GCSA2_KMER_TABLE": "0", "GCSA2_PAIR_BLOCKS": "0"}


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


def suffix_ranges(cpu, texts):
    """Per text: the oracle's range of each of its suffixes, row c - 1 for the suffix of c characters; one oracle batch."""
    suffixes = [t[len(t) - c:] for t in texts for c in range(1, len(t) + 1)]
    data, off = concat_patterns(suffixes)
    ranges = cpu.find_batch(data, off)
    out, at = [], 0
    for t in texts:
        out.append([(int(a), int(b)) for a, b in ranges[at:at + len(t)]])
        at += len(t)
    return out


def left_at_first_single(k, length, s):
    """Characters left when k_find2 first holds a range of one node, for a pattern over ACGT that occurs: it consumes the
    seed (k characters, when the pattern has that many; else one) and then two characters per pair step, one when one is
    left; `s` is the number of characters after which the range is one node.  None: never before the pattern ends."""
    c = k if 0 < k <= length else 1
    while c < s and c < length:
        c += 2 if length - c >= 2 else 1
    return length - c if c >= s and c < length else None


def in_label_masks(ix):
    """Per path node: bit c set = the node has a predecessor labelled comp c (the B_c of the index arrays)."""
    masks = np.zeros(ix.n, dtype=np.int64)
    for c in range(ix.sigma):
        words = ix.bwt[c]
        words = words.cpu().numpy() if hasattr(words, "cpu") else np.asarray(words)
        masks |= unpack_bits(words.view(np.uint64), ix.n).astype(np.int64) << c
    return masks


def lane_replica(masks, comps, rows, branch):
    """The lookups and block steps of one lane of k_find2 on an image without seed table and pair blocks (one character per
    step) whose jump entries offer {len, 6, 4} steps, with or without branch records, from the issue's rule.  `comps`: the
    pattern as comps, first character first; `rows`: the oracle's range of every suffix (suffix_ranges); `masks`: the
    in-label sets (in_label_masks).  Returns (jumps, fetch_steps, records): `records` lists, per lookup that read a
    record, (characters consumed before it, len, mask of the two-label node, steps taken)."""
    jumps = fetch_steps = 0
    records = []
    if len(comps) == 0:
        return jumps, fetch_steps, records
    c, i = 1, len(comps) - 1                    # characters consumed / left; the range is that of the suffix of c characters
    sp, ep = rows[0]
    done = sp > ep or i == 0
    tried = no_jump = False
    while not done:
        if sp == ep and i >= TAKE_LO and not tried and not no_jump:
            jumps += 1
            # the entry of node sp against the pattern: the chain is followed node by node through the oracle's ranges
            j, whole, mask = 0, False, 0
            while True:
                if j == JUMP_MAX:
                    whole = True                # a full entry, followed to its end
                    break
                a, b = rows[c + j - 1]
                assert a == b, (c, j, a, b)     # a matching label of a single node leads to a single node
                mask = int(masks[a])
                if not (bin(mask).count("1") == 1 and any(mask == 1 << f for f in FAST)):
                    whole = True                # the chain ends here: len = j, all of it followed
                    break
                if j == i or comps[i - 1 - j] not in FAST or mask != 1 << comps[i - 1 - j]:
                    break                       # the pattern ends on the chain or leaves it: usable = j < len
                j += 1
            record = (branch and whole and j <= BRANCH_MAX and bin(mask).count("1") == 2
                      and mask & ~sum(1 << f for f in FAST) == 0)
            if record and i >= j + 1 and comps[i - 1 - j] in FAST and (mask >> comps[i - 1 - j]) & 1:
                take, tried = j + 1, False
            elif whole and j > 0:
                take, tried = j, j < JUMP_MAX
            elif not whole and j >= TAKE_LO:
                take, tried = (TAKE_HI if j >= TAKE_HI else TAKE_LO), False
            else:
                take, tried, no_jump = 0, True, not whole
            if record:
                records.append((c, j, mask, take))
            if take > 0:
                c, i = c + take, i - take
                sp, ep = rows[c - 1]
                assert sp == ep, (c, sp, ep)
                done = i == 0
        else:
            fetch_steps += 1
            c, i = c + 1, i - 1
            sp, ep = rows[c - 1]
            done = sp > ep or i == 0
            tried = False
    return jumps, fetch_steps, records


def to_comps(ix, pattern):
    return [int(ix.char2comp[b]) for b in pattern]


def test_replica_on_a_made_up_chain():
    """The replica itself, on a hand-made case: nodes 0..9 in a line, labels A, except that node 3 has labels {C, G}."""
    masks = np.array([1 << 1] * 10, dtype=np.int64)
    masks[3] = (1 << 2) | (1 << 3)
    rows = [(c - 1, c - 1) for c in range(1, 11)]                   # the suffix of c characters is node c - 1
    # nine characters left at node 0: A A A, then C into node 3's predecessor, then five more A
    comps = [1, 1, 1, 1, 1, 2, 1, 1, 1, 1]
    # no records: lookup at node 0 takes 3 (whole chain), step out of node 3, lookup at node 4 (5 left): takes 4, one step
    assert lane_replica(masks, comps, rows, False)[:2] == (2, 2)
    # records: the lookup at node 0 takes 4, lookup at node 4 (5 left) takes 4, one step
    jumps, steps, records = lane_replica(masks, comps, rows, True)
    assert (jumps, steps) == (2, 1) and records == [(1, 3, 12, 4)]
    # a third character at node 3: the record is the ordinary entry, then the step (which the oracle's rows would empty)
    comps[5] = 4
    assert lane_replica(masks, comps, rows, True)[2] == [(1, 3, 12, 3)]


@pytest.fixture(scope="module")
def cases(engine):
    """Per graph of graph_cases: index arrays, oracle, walks.  Built once and left unchanged."""
    from oracle.oracle import OracleIndex
    return [(name, ix, OracleIndex(ix, **FIND_ONLY), [w for w in walks if len(w) > 0]) for name, ix, walks in graph_cases()]


@pytest.fixture(scope="module")
def prepared(engine, cases):
    """Per graph: the chain_patterns batch and batches of SIZES patterns whose first lookup has LEFT characters left, each
    with the oracle's ranges and with the ranges and counters of the image without records and of the image without the
    table."""
    out = []
    for at, (name, ix, cpu, walks) in enumerate(cases):
        plain = create(engine, ix, **NO_RECORDS)
        bare = create(engine, ix, GCSA2_JUMP_TABLE="0")
        assert plain.jump_mid() == 6 and plain.jump_branch() == 0 and plain.jump_table_bytes() == 16 * ix.n, name
        assert bare.jump_table_bytes() == 0 and bare.jump_branch() == 0, name
        k = plain.kmer_table_k()
        assert bare.kmer_table_k() == k, name
        texts = sorted(set(w for w in walks if set(w) <= set(b"ACGT")), key=lambda w: (-len(w), w))[:120]
        by_left = {}
        for w, rows in zip(texts, suffix_ranges(cpu, texts)):
            occurs = rows[-1][0] <= rows[-1][1]
            single = [c for c in range(1, len(w) + 1) if rows[c - 1][0] == rows[c - 1][1]]
            if not (occurs and single):
                continue
            for length in range(1, len(w) + 1):
                left = left_at_first_single(k, length, single[0])
                if left in LEFT and len(by_left.setdefault(left, [])) < 2:
                    by_left[left].append(w[len(w) - length:])
        chains = chain_patterns(cpu, walks, 0x7B0 + at)
        pool = [(by_left[left][j], left) for j in range(2) for left in sorted(by_left) if j < len(by_left[left])]
        pool += [(p, None) for p in chains[len(walks):][:90] + [b"", b"N", b"A"]]
        lefts = set(left for p, left in pool[:SIZES[1]] if left is not None)
        batches = []
        for pats in [chains] + [[pool[q % len(pool)][0] for q in range(nq)] for nq in SIZES]:
            data, off = concat_patterns(pats)
            batch = DeviceBatch(data, off)
            want = cpu.find_batch(data, off)
            entry = {"nq": len(pats), "data": data, "off": off, "want": want}
            for label, gpu in (("plain", plain), ("bare", bare)):
                got = batch.run(lambda p, o, n, r: gpu.find_device(p, o, n, r, 0))
                assert np.array_equal(got, want), (name, len(pats), label)
                twin, entry[label] = batch.stats(gpu)
                assert np.array_equal(twin, want), (name, len(pats), label)
            batches.append(entry)
        plain.close()
        bare.close()
        out.append((name, ix, lefts, batches))
    return out


def test_lengths_cover_every_tail(prepared):
    for name, ix, lefts, batches in prepared:
        print(f"    {name}: characters left at the first lookup {sorted(lefts)}")
        if name in ("snp40000", "dbg20"):
            assert lefts >= set(LEFT), (name, sorted(set(LEFT) - lefts))


def test_parity(engine, prepared):
    """Ranges of the image with records: the oracle's, hence those of the image without records, of the image without the
    table and of the instrumented twin; the counters that are functions of the batch do not move; the two builders give
    equal ranges and equal counters."""
    saved = 0
    for name, ix, lefts, batches in prepared:
        images = {how: create(engine, ix, GCSA2_JUMP_BUILD=how, **RECORDS) for how in ("double", "walk")}
        for how, gpu in images.items():
            assert gpu.jump_mid() == 6 and gpu.jump_branch() == 1 and gpu.jump_table_bytes() == 16 * ix.n, (name, how)
        for entry in batches:
            batch, want, nq = DeviceBatch(entry["data"], entry["off"]), entry["want"], entry["nq"]
            plain, bare = entry["plain"], entry["bare"]
            seen = {}
            for how, gpu in images.items():
                got = batch.run(lambda p, o, n, r: gpu.find_device(p, o, n, r, 0))
                assert np.array_equal(got, want), (name, how, nq)
                twin, seen[how] = batch.stats(gpu)
                assert np.array_equal(twin, want), (name, how, nq)
                blocks, steps, lookups, jumps, fetch_steps, second = seen[how]
                assert blocks == fetch_steps + second, (name, how, nq, seen[how])
                assert plain[0] == plain[4] + plain[5] and bare[0] == bare[4] + bare[5] and bare[3] == 0, (name, nq, plain, bare)
                assert steps == plain[1] == bare[1], (name, how, nq, seen[how], plain, bare)       # LF steps
                assert lookups == plain[2] == bare[2], (name, how, nq, seen[how], plain, bare)     # seed lookups
            assert seen["double"] == seen["walk"], (name, nq, seen)
            if name == "dbg20":
                print(f"    dbg20, {nq} patterns: without records {plain}, with {seen['walk']}")
                saved += plain[4] - seen["walk"][4]
        for gpu in images.values():
            gpu.close()
    assert saved > 0, saved             # the records were used: fewer block steps on the graph that has two-label nodes


@pytest.fixture(scope="module")
def stepwise(engine, cases):
    """The two graphs of the replica tests -- dbg20 of graph_cases and a de Bruijn graph of degree 12 with junction edges --
    with their in-label sets, walks over ACGT and the oracle's range of every suffix of every walk."""
    import torch
    from oracle.oracle import OracleIndex
    from workload import dbg_torch
    out = []
    name, ix, cpu, walks = [c for c in cases if c[0] == "dbg20"][0]
    out.append((name, ix, cpu, walks))
    ix12, dbg = dbg_torch.build_dbg(12, junctions=80, device=torch.device("cuda", 0))
    walks12 = []
    for m in (6, 9, 14, 22, 30):
        pats = dbg_torch.walk_patterns_device(dbg, 0, 40, m, 0x7C2 + m)[0]
        walks12 += [bytes(row) for row in pats.cpu().numpy()]
    out.append(("dbg12", ix12, OracleIndex(ix12, **FIND_ONLY), walks12))
    return [(name, ix, cpu, walks, in_label_masks(ix), suffix_ranges(cpu, walks)) for name, ix, cpu, walks in out]


def predicted(ix, masks, pats, rows, branch):
    jumps = steps = 0
    records = []
    for at, (p, r) in enumerate(zip(pats, rows)):
        j, s, rec = lane_replica(masks, to_comps(ix, p), r, branch)
        jumps, steps = jumps + j, steps + s
        records += [(at,) + x for x in rec]
    return jumps, steps, records


def test_records_follow_the_rule(engine, stepwise):
    for name, ix, cpu, walks, masks, rows in stepwise:
        images = {0: create(engine, ix, **NO_RECORDS, **ONE_CHARACTER_STEPS), 1: create(engine, ix, **RECORDS, **ONE_CHARACTER_STEPS)}
        totals = {}
        for branch, gpu in images.items():
            assert gpu.jump_branch() == branch and gpu.jump_mid() == 6 and gpu.kmer_table_k() == 0 and gpu.pair_block_bytes() == 0, name
            totals[branch] = [0, 0]
            for first in range(0, len(walks), 40):                  # one batch per walk length
                pats, part = walks[first:first + 40], rows[first:first + 40]
                data, off = concat_patterns(pats)
                want = cpu.find_batch(data, off)
                got, seen = DeviceBatch(data, off).stats(gpu)
                assert np.array_equal(got, want), (name, branch, first)
                jumps, steps, records = predicted(ix, masks, pats, part, branch == 1)
                print(f"    {name}, records {branch}, walks {first}..: jumps {seen[3]}, fetch_steps {seen[4]}; "
                      f"replica {jumps}, {steps}; {sum(1 for r in records if r[4] == r[2] + 1)} of {len(records)} records taken")
                assert seen[2] == 0 and seen[1] == sum(len(p) - 1 for p in pats), (name, branch, first, seen)
                assert seen[3] == jumps and seen[4] == steps, (name, branch, first, seen, jumps, steps)
                assert (branch == 1) or not records, (name, first)
                totals[branch][0] += seen[3]
                totals[branch][1] += seen[4]
            gpu.close()
        print(f"    {name}: (jumps, fetch_steps) without records {totals[0]}, with {totals[1]}")
        if name == "dbg20":
            assert totals[1][1] < totals[0][1], totals


def test_patterns_at_a_record(engine, stepwise):
    """At a record of every len 0..3: the patterns that go on with either label, with a third character, with N, that end
    exactly at the two-label node and one character behind it."""
    name, ix, cpu, walks, masks, rows = stepwise[0]
    assert name == "dbg20"
    jumps, steps, records = predicted(ix, masks, walks, rows, True)
    sites = {}
    for at, c, length, mask, take in records:
        if take == length + 1 and length not in sites and len(walks[at]) - c - length - 1 >= 1:
            sites[length] = (at, c, mask)
    assert sorted(sites) == [0, 1, 2, 3], sorted(sites)
    byte_of = {int(ix.char2comp[b]): b for b in b"ACGT"}
    pats, uses = [], []
    for length, (at, c, mask) in sorted(sites.items()):
        w = walks[at]
        tail = w[len(w) - c - length:]                              # ends exactly at the two-label node
        front = w[:len(w) - c - length - 1]                         # what the walk has in front of its label
        a, b = [f for f in FAST if (mask >> f) & 1]
        third = [f for f in FAST if not (mask >> f) & 1][0]
        assert len(tail) == c + length and w[len(front)] in (byte_of[a], byte_of[b])
        for x, record in ((byte_of[a], True), (byte_of[b], True), (byte_of[third], False), (ord("N"), False)):
            for pre in (b"", front, b"ACGT", b"TTGCA"):
                pats.append(pre + bytes([x]) + tail)                # pre = b"": ends one character behind the node
                # with the walk's own front the lane reaches the record as the walk's lane did, and either label takes it
                uses.append(record and pre == front)
        pats.append(tail)
        uses.append(False)
    data, off = concat_patterns(pats)
    want = cpu.find_batch(data, off)
    part = suffix_ranges(cpu, pats)
    for settings in (ONE_CHARACTER_STEPS, {}):
        for how in ("double", "walk"):
            gpu = create(engine, ix, GCSA2_JUMP_BUILD=how, **RECORDS, **settings)
            assert gpu.jump_branch() == 1, (settings, how)
            batch = DeviceBatch(data, off)
            got = batch.run(lambda p, o, n, r: gpu.find_device(p, o, n, r, 0))
            bad = [pats[q] for q in range(len(pats)) if not np.array_equal(got[q], want[q])]
            assert not bad, (settings, how, bad[:4])
            twin, seen = batch.stats(gpu)
            assert np.array_equal(twin, want), (settings, how)
            assert np.array_equal(gpu.find_batch(data, off), want), (settings, how)
            if settings:
                jumps, steps, records = predicted(ix, masks, pats, part, True)
                assert seen[3] == jumps and seen[4] == steps, (how, seen, jumps, steps)
                taken = set(r[0] for r in records if r[4] == r[2] + 1)
                assert all(q in taken for q in range(len(pats)) if uses[q]), (how, sorted(taken))
            gpu.close()
    assert sum(uses) >= 8, uses


def test_default(engine, cases):
    line = (256 << 20) // 16
    assert engine.jump_branch_default(line, True) == 0 and engine.jump_branch_default(line + 1, True) == 1
    assert engine.jump_branch_default(line + 1, False) == 0 and engine.jump_branch_default(1 << 36, False) == 0
    assert engine.jump_branch_default(0, True) == 0 and engine.jump_branch_default(5_726_623_061, True) == 1
    for at, (name, ix, cpu, walks) in enumerate(cases):
        assert 16 * ix.n <= (256 << 20), name
        for settings, mid, branch in (({}, 2, 0), ({"GCSA2_JUMP_MID": "6"}, 6, 0), ({"GCSA2_JUMP_BRANCH": "1"}, 2, 0),
                                      ({"GCSA2_JUMP_MID": "2", "GCSA2_JUMP_BRANCH": "1"}, 2, 0),
                                      ({"GCSA2_JUMP_MID": "6", "GCSA2_JUMP_BRANCH": "1"}, 6, 1),
                                      ({"GCSA2_JUMP_MID": "6", "GCSA2_JUMP_BRANCH": "0"}, 6, 0),
                                      ({"GCSA2_JUMP_MID": "6", "GCSA2_JUMP_BRANCH": "2"}, 6, 0),
                                      ({"GCSA2_JUMP_MID": "6", "GCSA2_JUMP_BRANCH": ""}, 6, 0),
                                      ({"GCSA2_JUMP_TABLE": "0", "GCSA2_JUMP_MID": "6", "GCSA2_JUMP_BRANCH": "1"}, 2, 0)):
            if at >= 3 and settings and name != "dbg20":            # every graph's default; the knobs on four of them
                continue
            gpu = create(engine, ix, **settings)
            assert gpu.jump_mid() == mid and gpu.jump_branch() == branch, (name, settings)
            assert gpu.jump_table_bytes() == (0 if "GCSA2_JUMP_TABLE" in settings else 16 * ix.n), (name, settings)
            gpu.close()
    # BRANCH=1 under mid = 2 builds no records: the table counts what the default image counts on the graph with two-label nodes
    name, ix, cpu, walks = [c for c in cases if c[0] == "dbg20"][0]
    data, off = concat_patterns(walks)
    counted = []
    for settings in ({}, {"GCSA2_JUMP_BRANCH": "1"}):
        gpu = create(engine, ix, **settings)
        got, seen = DeviceBatch(data, off).stats(gpu)
        assert np.array_equal(got, cpu.find_batch(data, off)), settings
        counted.append(seen)
        gpu.close()
    assert counted[0] == counted[1], counted
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
