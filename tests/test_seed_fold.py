"""The fold and the chunked locate that k-mer support, k-mer classes and k-mer top classes share (gcsa2_amd/csrc/host_fold.hpp):
one list of seed records through gcsa2_seed_support_device, gcsa2_seed_classes_device and gcsa2_seed_top_classes_device gives
one fold -- found, counted, distinct, values -- and each call's outputs are its own restatement's (test_kmer_support.Oracle,
test_kmer_classes.restate, test_kmer_top_classes.sparse_restate), whatever the chunks; the fold's early exits; the grammar of
GCSA2_SUPPORT_CHUNK."""
import numpy as np
import pytest

from gcsa2_amd.hostview import concat_patterns
from test_extend import BIG, indexed
from test_kmer_windows import reads_of
from test_kmer_support import (oracle_of, nonempty_of, DeviceReads, device_records, seed_support, assert_support, START, U64,
                               FIELDS as SUPPORT_FIELDS)
from test_kmer_classes import class_map, bins_of, to_device, NODE_SHIFT, UNKNOWN
import test_kmer_classes as dense
import test_kmer_top_classes as sparse

FOLD = ("found", "counted", "distinct", "values")       # what the shared fold and locate leave in every call's stats
CLASSES, TOP_N = 5, 3


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


@pytest.fixture(scope="module")
def records(big):
    """(seeds (m, 5), seed offsets (reads + 1)): the k = 3, stride-1 k-mer seed records of the batch, from gcsa2_kmer_hits_device."""
    reads = reads_of(BIG)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    p, o = batch.d_pat.data_ptr(), batch.d_off.data_ptr()
    sized = big.kmer_hits_batch(flat, off, 3, 1, 1, False)
    seeds = device_records(big, batch, lambda so, se, ho, hi, m, h: big.kmer_hits_device(p, o, batch.n, 3, 1, 1, 0, 0, so.data_ptr(), se.data_ptr(), m,
                                                                                       ho.data_ptr(), hi.data_ptr(), h), sized)
    seeds.setflags(write=False)
    return seeds, np.asarray(sized[0], dtype=np.uint64)


@pytest.fixture(scope="module")
def doubled(records):
    """The list concatenated with itself, so that every range folds: (seeds, weights cycling 0, 1, 3, group offsets -- the reads'
    records, twice)."""
    seeds, soff = records
    m = seeds.shape[0]
    assert int(soff[-1]) == m and m > 64
    assert (seeds[:, 4] > 64).any() and np.unique(seeds[:, 2:4], axis=0).shape[0] > 8
    both = np.concatenate([seeds, seeds])
    weights = np.asarray([(0, 1, 3)[i % 3] for i in range(2 * m)], dtype=np.uint64)
    goff = np.concatenate([soff, soff[1:] + np.uint64(m)])
    return both, weights, goff


class Consumers:
    """The three calls on one record list at NODE_SHIFT: `interleaved` classes, CLASSES of them, the top TOP_N, no flags."""

    def __init__(self, gpu, seeds, weights, goff):
        self.gpu, self.seeds, self.weights, self.goff = gpu, seeds, weights, goff
        self.m, self.n_groups = seeds.shape[0], len(goff) - 1
        self.n_bins = bins_of(BIG, NODE_SHIFT)
        self.cmap = class_map("interleaved", self.n_bins, CLASSES)
        self.d_seeds, self.d_goff = to_device(seeds) if self.m else None, to_device(goff)
        self.d_weights = None if weights is None else to_device(weights)

    def want(self, hit_max):
        """(support's (add, stats) or None where its restatement does not go, classes' (votes, calls, stats), top classes' (top,
        summaries, stats, tie), the folded records)."""
        oracle = oracle_of(BIG)
        classes, rec = dense.seeds_want(oracle, self.goff, self.seeds, self.weights, hit_max, NODE_SHIFT, self.cmap, CLASSES, 0)
        top, _ = sparse.seeds_want(oracle, self.goff, self.seeds, self.weights, hit_max, NODE_SHIFT, self.cmap, CLASSES, 0, TOP_N)
        if rec.counted:
            support = oracle.seeds(self.seeds, self.weights, hit_max).tally(NODE_SHIFT, False, self.n_bins)
        else:                                        # nothing to add: the fold's figures are those of the classes' restatement
            support = (np.zeros(self.n_bins, dtype=np.uint64),
                       dict(dict.fromkeys(SUPPORT_FIELDS, 0), windows=self.m, found=rec.found, counted=rec.counted))
        return support, classes, top, rec

    def run(self, hit_max):
        """Every call once: {name: (stats, every output buffer with its guard words)}."""
        import torch
        got = {"support": seed_support(self.gpu, self.seeds, self.weights, hit_max, NODE_SHIFT, 0, self.n_bins)}
        self.dense_out = dense.Outputs(self.n_groups, CLASSES)
        stats = dense.seed_call(self.gpu, self.d_goff, self.n_groups, self.d_seeds, self.m, self.d_weights, hit_max, NODE_SHIFT, 0, self.cmap, CLASSES, self.dense_out)
        self.top_out = sparse.Outputs(self.n_groups, TOP_N)
        top_stats = sparse.seed_call(self.gpu, self.d_goff, self.n_groups, self.d_seeds, self.m, self.d_weights, hit_max, NODE_SHIFT, 0, self.cmap, CLASSES, TOP_N,
                                     self.top_out)
        torch.cuda.synchronize()
        got["classes"] = (stats, self.dense_out.votes.cpu().numpy(), self.dense_out.calls.cpu().numpy())
        got["top"] = (top_stats, self.top_out.top.cpu().numpy(), self.top_out.sums.cpu().numpy())
        return got

    def check(self, hit_max, what):
        """One run against the restatements; the fold's four figures equal across the calls.  Returns (the run, the wanted)."""
        want = self.want(hit_max)
        support, classes, top, rec = want
        got = self.run(hit_max)
        assert_support(got["support"], support, self.n_bins, (what, "support"))
        self.dense_out.check(got["classes"][0], classes, (what, "classes"))
        self.top_out.check(got["top"][0], top, (what, "top classes"))
        fold = dict(found=rec.found, counted=rec.counted, distinct=rec.ranges.shape[0], values=rec.values.shape[0])
        for name in ("support", "classes", "top"):
            assert {f: got[name][0][f] for f in FOLD} == fold, (what, name, got[name][0], fold)
            assert got[name][0]["windows"] == self.m, (what, name)
        return got, want


def same_run(a, b):
    return all(a[name][0] == b[name][0] and all(np.array_equal(x, y) for x, y in zip(a[name][1:], b[name][1:])) for name in a)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", ("1", "64", None))
@pytest.mark.parametrize("hit_max", (0, 64))
def test_the_consumers_agree_on_one_record_list(big, doubled, monkeypatch, hit_max, chunk):
    """Every range of the doubled list folds (distinct = the ranges of the single list, counted = twice its counted records);
    under hit_max = 64 some records are counted and some are not.  A budget of 1 makes a chunk of every range, 64 a few ranges
    each, the default one chunk."""
    if chunk is None:
        monkeypatch.delenv("GCSA2_SUPPORT_CHUNK", raising=False)
    else:
        monkeypatch.setenv("GCSA2_SUPPORT_CHUNK", chunk)
    seeds, weights, goff = doubled
    _, (support, classes, top, rec) = Consumers(big, seeds, weights, goff).check(hit_max, (hit_max, chunk))
    assert rec.counted % 2 == 0 and 0 < rec.ranges.shape[0] <= rec.counted // 2 and rec.values.shape[0] >= rec.ranges.shape[0]
    if hit_max == 0:
        assert rec.counted == rec.found and rec.ranges.shape[0] > 8 and rec.values.shape[0] > 64
    else:
        assert 0 < rec.counted < rec.found
    assert support[1]["added"] > 0 and classes[2]["votes"] > 0 and top[2]["votes"] == classes[2]["votes"]


@pytest.mark.gpu
def test_the_early_exits_of_the_fold(big, records, monkeypatch):
    """(a) one record; (b) only empty ranges: nothing found; (c) only ranges above hit_max: found, none counted; (d) a range whose
    ep lies beyond the index: found, count() = 0.  From (b) on support adds nothing; classes and top classes write every row,
    call and summary of every group -- an empty group, the group of all records, an empty group -- and the stats are the
    restatement's."""
    monkeypatch.delenv("GCSA2_SUPPORT_CHUNK", raising=False)
    seeds, _ = records
    n = indexed(BIG)[1].n
    empties = np.asarray([[0, 5, 1, 0, 9], [0, 5, n + 3, n + 2, 1], [0, 0, 0, U64, 0], [3, 3, 7, 6, 1]], dtype=np.uint64)
    beyond = np.asarray([[0, 4, n - 2, n + 5, 3]], dtype=np.uint64)
    above = seeds[seeds[:, 4] > 64][:70]
    assert not nonempty_of(empties[:, 2:4]).any() and nonempty_of(beyond[:, 2:4]).all() and above.shape[0] == 70
    for what, some, hit_max, found, counted in (("one record", seeds[:1], 0, 1, 1), ("only empty ranges", empties, 0, 0, 0),
                                                ("only ranges above hit_max", above, 64, 70, 0), ("a range beyond the index", beyond, 0, 1, 0)):
        m = some.shape[0]
        weights = np.asarray([(3, 1, 0)[i % 3] for i in range(m)], dtype=np.uint64)
        goff = np.asarray([0, 0, m, m], dtype=np.uint64)
        got, (support, classes, top, rec) = Consumers(big, some, weights, goff).check(hit_max, what)
        assert (rec.found, rec.counted) == (found, counted), what
        if counted == 0:
            assert not support[0].any() and (got["support"][1][:support[0].shape[0]] == np.uint64(START)).all(), what
            assert got["support"][0] == dict(dict.fromkeys(SUPPORT_FIELDS, 0), windows=m, found=found), what
            assert not classes[0].any() and (classes[1] == np.asarray([UNKNOWN, 0, UNKNOWN, 0, 0, 0], dtype=np.uint64)).all(), what
            assert (top[0] == np.asarray([UNKNOWN, 0], dtype=np.uint64)).all() and not top[1].any(), what
        else:
            assert support[1]["added"] == 3 * rec.values.shape[0] > 0 and int(classes[1][1, 5]) == 1 and int(top[1][1, 2]) == 1, what


@pytest.mark.gpu
def test_the_knob_grammar(big, doubled, monkeypatch):
    """GCSA2_SUPPORT_CHUNK empty, zero, with trailing junk or no number at all is ignored: the outputs and the stats of the run
    without it."""
    seeds, weights, goff = doubled
    calls = Consumers(big, seeds, weights, goff)
    monkeypatch.delenv("GCSA2_SUPPORT_CHUNK", raising=False)
    unset, _ = calls.check(0, "unset")
    for value in ("", "0", "12x", "abc"):
        monkeypatch.setenv("GCSA2_SUPPORT_CHUNK", value)
        assert same_run(calls.run(0), unset), value
