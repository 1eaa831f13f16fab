"""Batched minimizer seeds (gcsa2_minimizers_device / _batch, gcsa2_minimizer_hits_device / _batch; kernels_minimizers.hpp):
the (w, k)-minimizers of every read, alone and as the windows of the k-mer hits.  The selection is checked against a Python
restatement of the header's definition (vectorised here, and compared with a second, literal form of it); ranges, counts and
hits are the CPU oracle's for the stride-1 windows (test_kmer_hits.Seeds, cached per graph and left unchanged), of which the
selected ones are taken."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from gcsa2_amd.hostview import concat_patterns
from test_oracle import CASES
from test_mem_hits import EDGE, SENTINEL
from test_extend import GRAPHS, BIG, indexed
from test_kmer_windows import reads_of
from test_kmer_hits import oracle_of, Seeds, Spins, DeviceReads, assert_device, assert_host, untouched, GUARD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
INVALID, MISSING, TOO_SMALL = -1, -5, -6
SKIP, SAMPLE = 0, 1
OTHER_SEED = 0x9D2C5680F00DFACE
SELECT_K = (1, 2, 3, 4, 8, 12, 16, 31, 32)
SELECT_W = (1, 2, 5, 11, 63, 64)
HITS_W = (1, 5, 11, 64)
HIT_MAX = (0, 1, 3, 64, U64)
NAMES = ("gcsa2_minimizers_device", "gcsa2_minimizers_batch", "gcsa2_minimizer_hits_device", "gcsa2_minimizer_hits_batch")


# ---- the definition, restated -----------------------------------------------------------------------------------------------

def mix64(x):
    z = (x + 0x9E3779B97F4A7C15) & U64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & U64
    return z ^ (z >> 31)


def mix64_np(x):
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def alphabet(which=BIG):
    ix = indexed(which)[0]
    return np.asarray(ix.char2comp, dtype=np.int64).copy(), int(ix.sigma)


def codes_of(read, c2c, sigma):
    comp = c2c[np.frombuffer(read, dtype=np.uint8)]
    return np.where((comp >= 1) & (comp <= min(4, sigma - 2)), comp - 1, -1)


def literal(read, k, w, seed, c2c, sigma):
    """The definition word for word, for one read: [(position, hash)] in ascending position."""
    code = [int(c) for c in codes_of(read, c2c, sigma)]
    W = max(0, len(read) - k + 1)
    valid = [all(code[j + i] >= 0 for i in range(k)) for j in range(W)]
    hashes = [mix64(sum(code[j + i] << (2 * (k - 1 - i)) for i in range(k)) ^ seed) if valid[j] else None for j in range(W)]
    chosen, a = set(), 0
    while a < W:
        if not valid[a]:
            a += 1
            continue
        b = a
        while b < W and valid[b]:
            b += 1
        spans = [(s, s + w) for s in range(a, b - w + 1)] if b - a >= w else [(a, b)]
        for s, e in spans:
            chosen.add(min((hashes[j], j) for j in range(s, e))[1])
        a = b
    return [(j, hashes[j]) for j in sorted(chosen)]


def restate(reads, k, w, seed, c2c, sigma):
    """The definition for a batch, vectorised: (min_offsets (reads + 1), minimizers (total, 2)).  The reads are laid end to
    end with one invalid character behind each, so that no window that crosses a boundary is valid and no run does."""
    n = len(reads)
    codes = np.concatenate([np.concatenate([codes_of(r, c2c, sigma), [-1]]) for r in reads] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in reads])]).astype(np.int64)[:n]
    M = codes.shape[0] - k + 1
    if M <= 0:
        return np.zeros(n + 1, dtype=np.uint64), np.zeros((0, 2), dtype=np.uint64)
    bad = np.concatenate([[0], np.cumsum(codes < 0)])
    valid = (bad[k:] - bad[:-k]) == 0
    key = np.zeros(M, dtype=np.uint64)
    for i in range(k):
        key = (key << np.uint64(2)) | np.maximum(codes[i:i + M], 0).astype(np.uint64)
    hashes = mix64_np(key ^ np.uint64(seed))
    s = np.arange(M)
    stops = np.concatenate([np.flatnonzero(~valid), [M]])
    run_end = stops[np.searchsorted(stops, s)]              # the first invalid window at or behind s
    length = np.minimum(w, run_end - s)
    begins = valid & ~np.concatenate([[False], valid[:-1]])
    selected = np.zeros(M, dtype=bool)
    full = np.flatnonzero(valid & (length == w))
    if full.size:
        view = np.lib.stride_tricks.sliding_window_view(hashes, w)
        selected[full + view[full].argmin(axis=1)] = True            # argmin: the first, so the leftmost, of equal hashes
    for a in np.flatnonzero(begins & (length < w)).tolist():
        selected[a + int(hashes[a:a + int(length[a])].argmin())] = True
    picked = np.flatnonzero(selected)
    owner = np.searchsorted(starts, picked, side="right") - 1
    mins = np.zeros((picked.shape[0], 2), dtype=np.uint64)
    mins[:, 0] = picked - starts[owner]
    mins[:, 1] = hashes[picked]
    moff = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))]).astype(np.uint64)
    return moff, mins


class MinSeeds:
    """The contract's arrays of the minimizer hits for one graph's batch: the oracle's stride-1 windows (test_kmer_hits.Seeds),
    of which the restatement's minimizers are taken."""

    def __init__(self, seeds, c2c, sigma):
        self.seeds, self.c2c, self.sigma = seeds, c2c, sigma
        self.cut = {}

    def windows(self, k, w, seed):
        if (k, w, seed) not in self.cut:
            woff, _, rng, cnt = self.seeds.exp.want(k, 1)
            moff, mins = restate(self.seeds.reads, k, w, seed, self.c2c, self.sigma)
            n = len(self.seeds.reads)
            owner = np.repeat(np.arange(n), np.diff(moff.astype(np.int64)))
            pick = woff[:-1].astype(np.int64)[owner] + mins[:, 0].astype(np.int64)
            r, c = rng[pick], cnt[pick]
            nonempty = ((r[:, 0] + np.uint64(1)) <= (r[:, 1] + np.uint64(1))) if pick.size else np.zeros(0, dtype=bool)
            nodes = np.where(nonempty, r[:, 1] + np.uint64(1) - r[:, 0], np.uint64(0)).astype(np.uint64)
            prof = np.zeros((n, 4), dtype=np.uint64)
            prof[:, 0] = np.diff(moff.astype(np.int64))
            for column, values in ((1, nonempty), (2, nodes), (3, c)):
                np.add.at(prof[:, column], owner, values.astype(np.uint64))
            records = np.zeros((int(nonempty.sum()), 5), dtype=np.uint64)
            records[:, 0], records[:, 1], records[:, 2:4], records[:, 4] = mins[nonempty, 0], k, r[nonempty], c[nonempty]
            soff = np.concatenate([[0], np.cumsum(prof[:, 1].astype(np.int64))]).astype(np.uint64)
            distinct, inverse = (np.unique(records[:, 2:5], axis=0, return_inverse=True) if records.shape[0]
                                 else (np.zeros((0, 3), dtype=np.uint64), np.zeros(0, dtype=np.int64)))
            self.cut[(k, w, seed)] = (prof, records, soff, distinct, np.asarray(inverse).reshape(-1), moff, mins)
        return self.cut[(k, w, seed)]

    def want(self, k, w, seed, hit_max, sample):
        """(seed_offsets, seeds, hit_offsets, hits, profiles)."""
        prof, records, soff, distinct, inverse, _, _ = self.windows(k, w, seed)
        per_range = [np.asarray(self.seeds.hits((int(sp), int(ep)), int(c), hit_max, sample), dtype=np.uint64) for sp, ep, c in distinct.tolist()]
        sizes = np.asarray([a.shape[0] for a in per_range], dtype=np.int64)[inverse] if records.shape[0] else np.zeros(0, dtype=np.int64)
        hoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        hits = np.concatenate([per_range[i] for i in inverse.tolist()] + [np.zeros(0, dtype=np.uint64)]).astype(np.uint64)
        return soff, records, hoff, hits, prof


@functools.lru_cache(maxsize=None)
def minimizers_of(which):
    return MinSeeds(oracle_of(which), *alphabet(which))


def random_read(rng, length, letters=b"ACGT"):
    return bytes(letters[int(x)] for x in rng.integers(0, len(letters), length))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_minimizer_calls_and_refuses_a_null_index():
    """1. The header declares the four calls, the built library exports them, binding.EXPORTS lists them; each refuses a NULL
    index with INVALID_ARGUMENT without a device, names the index and writes nothing."""
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    header = open(os.path.join(ROOT, "include", "gcsa2_hip.h")).read()
    for name in NAMES:
        assert ("int " + name + "(") in header and name in binding.EXPORTS and hasattr(ctypes.CDLL(binding.LIB_PATH), name), name
    assert "#define GCSA2_MINIMIZER_MAX_K 32" in header and "#define GCSA2_MINIMIZER_MAX_W 64" in header
    lib = binding.load_library()
    off = (ctypes.c_uint64 * 2)(0, 8)
    pat = (ctypes.c_uint8 * 8)(*b"ACGTACGT")
    moff = (ctypes.c_uint64 * 2)(7, 7)
    mins = (ctypes.c_uint64 * 10)(*([7] * 10))
    total = ctypes.c_uint64(7)
    rc = lib.gcsa2_minimizers_device(None, ctypes.addressof(pat), ctypes.addressof(off), 1, 4, 2, 0, ctypes.addressof(moff), ctypes.addressof(mins), 5,
                                     ctypes.byref(total), None)
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    rc = lib.gcsa2_minimizers_batch(None, pat, off, 1, 4, 2, 0, ctypes.addressof(moff), ctypes.addressof(mins), 5, ctypes.byref(total))
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    assert list(moff) == [7, 7] and list(mins) == [7] * 10 and total.value == 7
    prof = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    soff = (ctypes.c_uint64 * 2)(7, 7)
    seeds = (ctypes.c_uint64 * 25)(*([7] * 25))
    hoff = (ctypes.c_uint64 * 6)(*([7] * 6))
    hits = (ctypes.c_uint64 * 8)(*([7] * 8))
    total_seeds, total_hits = ctypes.c_uint64(7), ctypes.c_uint64(7)
    outputs = (ctypes.addressof(prof), ctypes.addressof(soff), ctypes.addressof(seeds), 5, ctypes.byref(total_seeds), ctypes.addressof(hoff),
               ctypes.addressof(hits), 8, ctypes.byref(total_hits))
    rc = lib.gcsa2_minimizer_hits_device(None, ctypes.addressof(pat), ctypes.addressof(off), 1, 4, 2, 0, 0, SKIP, *outputs, None)
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    rc = lib.gcsa2_minimizer_hits_batch(None, pat, off, 1, 4, 2, 0, 0, SKIP, *outputs)
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    assert list(prof) == [7] * 4 and list(soff) == [7, 7] and list(seeds) == [7] * 25 and list(hoff) == [7] * 6 and list(hits) == [7] * 8
    assert total_seeds.value == 7 and total_hits.value == 7


def test_the_restatement_is_the_definition():
    """2. The vectorised restatement equals the literal form (a loop over every span, min over (hash, position)) on random
    strings over ACGTNacgt$ of 0 .. 200 characters; w = 1 selects exactly the valid windows; a homopolymer selects exactly the
    span starts 0 .. W - w (the leftmost of equal hashes); another hash_seed changes the selection."""
    c2c, sigma = alphabet()
    assert sigma >= 6 and [int(c2c[c]) for c in b"ACGTacgt"] == [1, 2, 3, 4, 1, 2, 3, 4] and not 1 <= int(c2c[ord("N")]) <= 4
    rng = np.random.default_rng(0x3141)
    reads = [random_read(rng, int(length), b"ACGTNacgt$" if i % 3 else b"ACGT") for i, length in enumerate(rng.integers(0, 201, 300))]
    reads[:3] = [b"", b"A" * 200, random_read(rng, 200)]
    seeded = 0
    for k in (1, 4, 16, 32):
        for w in (1, 2, 5, 11, 64):
            for seed in (0, OTHER_SEED):
                moff, mins = restate(reads, k, w, seed, c2c, sigma)
                assert moff.shape[0] == len(reads) + 1 and int(moff[-1]) == mins.shape[0]
                for q, r in enumerate(reads):
                    got = [(int(p), int(h)) for p, h in mins[int(moff[q]):int(moff[q + 1])].tolist()]
                    assert got == literal(r, k, w, seed, c2c, sigma), (k, w, seed, q, r)
                    if w == 1:
                        code = codes_of(r, c2c, sigma)
                        assert [p for p, _ in got] == [j for j in range(max(0, len(r) - k + 1)) if (code[j:j + k] >= 0).all()], (k, q)
                homopolymer = [int(p) for p in mins[int(moff[1]):int(moff[2]), 0]]
                assert homopolymer == list(range(max(1, 200 - k + 1 - w + 1))), (k, w, homopolymer[:4])
            if w > 1:
                a, b = restate(reads, k, w, 0, c2c, sigma), restate(reads, k, w, OTHER_SEED, c2c, sigma)
                seeded += int(not np.array_equal(a[1][:, 0], b[1][:, 0]))
    assert seeded >= 12, seeded                              # every (k, w > 1) but the ones where nothing can differ


def test_the_batches_are_not_vacuous():
    """3. On the 6000-base graph with hash_seed 0: at k = 8 and every w, 0 < found < selected < windows, with found minimizers
    at or below and above the caps 1 and 3; at k = 4 every found one lies above 3 and at or below 64, at k <= 3 above 64; at
    k = 16, w = 11 there are reads with minimizers of which none is found, and reads shorter than k."""
    big = minimizers_of(BIG)
    reads = reads_of(BIG)
    for w in (1, 2, 5, 11):
        prof, records, _, _, _, moff, mins = big.windows(8, w, 0)
        windows = sum(max(0, len(r) - 8 + 1) for r in reads)
        assert 0 < records.shape[0] < mins.shape[0] < windows, (w, records.shape[0], mins.shape[0], windows)
        counts = records[:, 4]
        for cap in (1, 3):
            assert int((counts <= np.uint64(cap)).sum()) > 0 and int((counts > np.uint64(cap)).sum()) > 0, (w, cap)
    for w in (1, 5, 11):
        counts = big.windows(4, w, 0)[1][:, 4]
        assert counts.shape[0] > 0 and (counts > np.uint64(3)).all() and (counts <= np.uint64(64)).all(), w
        for k in (1, 2, 3):
            counts = big.windows(k, w, 0)[1][:, 4]
            assert counts.shape[0] > 0 and (counts > np.uint64(64)).all(), (k, w)
    prof = big.windows(16, 11, 0)[0]
    assert int(((prof[:, 0] > 0) & (prof[:, 1] == 0)).sum()) > 0 and sum(len(r) < 16 for r in reads) > 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

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


def device_minimizers(batch, gpu, k, w, seed, capacity, records=True):
    """gcsa2_minimizers_device on sentinel-filled buffers with GUARD entries behind each: (result or Gcsa2Error, min_offsets,
    minimizers), whole buffers."""
    import torch
    from gcsa2_amd.binding import Gcsa2Error
    s = np.uint64(SENTINEL).view(np.int64).item()
    d_moff = torch.full((batch.n + 1 + GUARD,), s, dtype=torch.int64, device=batch.dev)
    d_mins = torch.full((capacity + GUARD, 2), s, dtype=torch.int64, device=batch.dev)
    try:
        res = gpu.minimizers_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, k, w, seed, d_moff.data_ptr(),
                                    d_mins.data_ptr() if records else 0, capacity if records else 0)
    except Gcsa2Error as e:
        res = e
    torch.cuda.synchronize()
    return res, d_moff.cpu().numpy().view(np.uint64), d_mins.cpu().numpy().view(np.uint64)


def device_hits(batch, gpu, k, w, seed, hit_max, over, seed_capacity, hit_capacity, profiles=True, records=True):
    """gcsa2_minimizer_hits_device on sentinel-filled buffers, as test_kmer_hits.DeviceReads.hits."""
    import torch
    from gcsa2_amd.binding import Gcsa2Error
    s = np.uint64(SENTINEL).view(np.int64).item()
    d_prof = torch.full((batch.n + GUARD, 4), s, dtype=torch.int64, device=batch.dev) if profiles else None
    d_soff = torch.full((batch.n + 1 + GUARD,), s, dtype=torch.int64, device=batch.dev)
    d_seeds = torch.full((seed_capacity + GUARD, 5), s, dtype=torch.int64, device=batch.dev)
    d_hoff = torch.full((seed_capacity + 1 + GUARD,), s, dtype=torch.int64, device=batch.dev)
    d_hits = torch.full((hit_capacity + GUARD,), s, dtype=torch.int64, device=batch.dev)
    try:
        res = gpu.minimizer_hits_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, k, w, seed, hit_max, over,
                                        0 if d_prof is None else d_prof.data_ptr(), d_soff.data_ptr(), d_seeds.data_ptr() if records else 0,
                                        seed_capacity if records else 0, d_hoff.data_ptr(), d_hits.data_ptr() if records else 0,
                                        hit_capacity if records else 0)
    except Gcsa2Error as e:
        res = e
    torch.cuda.synchronize()
    return (res,) + tuple(None if t is None else t.cpu().numpy().view(np.uint64) for t in (d_soff, d_seeds, d_hoff, d_hits, d_prof))


def assert_selection(got, want, n, what):
    res, moff, mins = got
    w_moff, w_mins = want
    total = w_mins.shape[0]
    sentinel = np.uint64(SENTINEL)
    assert res == total, (what, res, total)
    assert np.array_equal(moff[:n + 1], w_moff) and (moff[n + 1:] == sentinel).all(), (what, "min_offsets")
    bad = np.nonzero((mins[:total] != w_mins).any(axis=1))[0]
    assert bad.size == 0, (what, "minimizers", int(bad.size), int(bad[0]), mins[bad[0]].tolist(), w_mins[bad[0]].tolist())
    assert (mins[total:] == sentinel).all(), (what, "behind the minimizers")


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_selection_parity(engine, which):
    """4. minimizers_device and minimizers_batch equal the restatement exactly -- offsets, positions, hashes -- for every k, w
    and two hash seeds, and the guards behind the buffers stay intact."""
    reads = reads_of(which)
    c2c, sigma = alphabet(which)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    for k in SELECT_K:
        for w in SELECT_W:
            for seed in (0, OTHER_SEED):
                want = restate(reads, k, w, seed, c2c, sigma)
                what = (GRAPHS[which][0], k, w, seed)
                assert_selection(device_minimizers(batch, gpu, k, w, seed, want[1].shape[0]), want, len(reads), what + ("device",))
                moff, mins = gpu.minimizers_batch(flat, off, k, w, seed)
                assert np.array_equal(moff, want[0]) and np.array_equal(mins, want[1]), what + ("host",)
    gpu.close()


def tile_reads(k, w, rng):
    """Reads built for the tile logic of the selection kernel at (k, w)."""
    reads = [random_read(rng, max(0, windows + k - 1) if windows else max(0, k - 1))
             for windows in (0, 1, max(w - 1, 0), w, w + 1, 63, 64, 65, 127, 128, 129)]
    reads.append(random_read(rng, 1000))
    long_read = random_read(rng, 300 + k)
    for at in (63, 64, 63 + k - 1, 64 + k - 1, 127, 128, 127 + k - 1, 128 + k - 1):          # the last character of a tile's windows, the first of the next
        reads.append(long_read[:at] + b"N" + long_read[at + 1:])
    period = max(w - 1, 1) + k - 1 + 1                      # runs of w - 1 valid windows between two Ns
    short_runs = bytearray(random_read(rng, 400))
    short_runs[period - 1::period] = b"N" * len(short_runs[period - 1::period])
    reads += [bytes(short_runs), b"N" * 150, b"", b"A" * 200, b"acgtACGT" * 20]
    reads += [random_read(rng, 73) for _ in range(8)]       # 73 = 9 * 8 + 1: these begin at every byte offset of a word (asserted by the test)
    return reads


@pytest.mark.gpu
def test_selection_on_tile_edges(big):
    """4. (continued) Reads with 0, 1, w - 1, w, w + 1, 63 .. 65 and 127 .. 129 windows, one of 1000 characters, an N at the last
    character of a tile and the first of the next, runs shorter than w, all-N, empty and homopolymer reads, reads that begin
    at every byte offset of an 8-byte word, in a pattern buffer of exactly total + 8 bytes with 0xFF filler."""
    c2c, sigma = alphabet()
    rng = np.random.default_rng(0x711E)
    for k in (1, 4, 16, 31, 32):
        for w in SELECT_W:
            reads = tile_reads(k, w, rng)
            flat, off = concat_patterns(reads)
            assert {int(o) % 8 for o in off[:-1]} == set(range(8))
            batch = DeviceReads(reads)
            assert batch.d_pat.shape[0] == batch.total + 8
            for seed in (0, OTHER_SEED):
                want = restate(reads, k, w, seed, c2c, sigma)
                assert_selection(device_minimizers(batch, big, k, w, seed, want[1].shape[0]), want, len(reads), ("tiles", k, w, seed))
            moff, mins = big.minimizers_batch(flat, off, k, w, 0)
            want = restate(reads, k, w, 0, c2c, sigma)
            assert np.array_equal(moff, want[0]) and np.array_equal(mins, want[1]), ("tiles, host", k, w)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_hits_parity(engine, which):
    """5. minimizer_hits_device and minimizer_hits_batch equal the oracle-derived (seed_offsets, seeds, hit_offsets, hits,
    profiles) exactly, for every k, w, cap and policy; the guards stay intact.  A range the reference would draw forever on
    is handled as in test_kmer_hits.py and never occurs for the caps 1, 3 and 64."""
    from gcsa2_amd.binding import Gcsa2Error
    oracle = minimizers_of(which)
    reads = reads_of(which)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    kmer_k = gpu.kmer_table_k()
    spun = 0
    for k in sorted({4, 8, 16, 32} | {x for x in (kmer_k - 1, kmer_k, kmer_k + 1) if 1 <= x <= 32}):
        for w in HITS_W:
            for hit_max in HIT_MAX:
                for sample in (False, True):
                    what = (GRAPHS[which][0], k, w, hit_max, sample)
                    try:
                        want = oracle.want(k, w, 0, hit_max, sample)
                    except Spins:
                        spun += 1
                        assert hit_max not in (1, 3, 64), what
                        with pytest.raises(Gcsa2Error) as err:
                            gpu.minimizer_hits_batch(flat, off, k, w, 0, hit_max, sample)
                        assert err.value.code == INVALID and "max_positions" in str(err.value), what
                        continue
                    m, h = want[1].shape[0], want[3].shape[0]
                    assert_device(device_hits(batch, gpu, k, w, 0, hit_max, int(sample), m, h), want, len(reads), what + ("device",))
                    assert_host(gpu.minimizer_hits_batch(flat, off, k, w, 0, hit_max, sample, profiles=True), want, what + ("host",))
    assert spun <= 16, spun
    want = oracle.want(8, 5, OTHER_SEED, 3, True)
    assert_device(device_hits(batch, gpu, 8, 5, OTHER_SEED, 3, SAMPLE, want[1].shape[0], want[3].shape[0]), want, len(reads), "another seed")
    gpu.close()


@pytest.mark.gpu
def test_w_1_is_the_stride_1_call(big):
    """6. On the reads without an invalid character, minimizer_hits_device(k, w = 1) equals kmer_hits_device(k, stride = 1)
    byte for byte in all five arrays; on the full batch it equals that call's output without the seeds of invalid windows.
    (The issue expected none of those on this graph.  There are 8 to 10 per k: three walks run into the sink, and windows
    such as TTT$ and T$#T are found.  They are taken out here as the contract says, not asserted away.)"""
    c2c, sigma = alphabet()
    reads = reads_of(BIG)
    clean = [r for r in reads if len(r) and (codes_of(r, c2c, sigma) >= 0).all()]
    assert 50 < len(clean) < len(reads)
    for k in (4, 16, 32):
        for some in (clean, reads):
            n = len(some)
            batch = DeviceReads(some)
            sizes = batch.hits(big, k, 1, 3, SAMPLE, 0, 0)[0].needed
            assert sizes[0] > 0 and sizes[1] > 0
            res, soff, seeds, hoff, hits, prof = batch.hits(big, k, 1, 3, SAMPLE, *sizes)
            assert res == sizes
            if some is clean:
                new = device_hits(batch, big, k, 1, 0, 3, SAMPLE, *sizes)
                assert new[0] == sizes
                for a, b in zip((soff, seeds, hoff, hits, prof), new[1:]):
                    assert np.array_equal(a, b), (k, "clean reads")
                continue
            m = sizes[0]
            seeds, hoff, prof = seeds[:m], hoff[:m + 1].astype(np.int64), prof[:n].copy()
            owner = np.repeat(np.arange(n), np.diff(soff[:n + 1].astype(np.int64)))
            keep = np.asarray([bool((codes_of(some[q][p:p + k], c2c, sigma) >= 0).all()) for q, p in zip(owner.tolist(), seeds[:, 0].tolist())])
            assert 0 < int((~keep).sum()) <= 10, (k, int((~keep).sum()))
            per_seed = np.diff(hoff)
            w_seeds = seeds[keep]
            w_soff = np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=n))]).astype(np.uint64)
            w_hoff = np.concatenate([[0], np.cumsum(per_seed[keep])]).astype(np.uint64)
            w_hits = hits[:sizes[1]][np.repeat(keep, per_seed)]
            prof[:, 0] = [sum(bool((codes_of(r[j:j + k], c2c, sigma) >= 0).all()) for j in range(max(0, len(r) - k + 1))) for r in some]
            for q, record in zip(owner[~keep].tolist(), seeds[~keep].tolist()):
                prof[q, 1:] -= np.asarray([1, record[3] + 1 - record[2], record[4]], dtype=np.uint64)
            want = (w_soff, w_seeds, w_hoff, w_hits, prof)
            assert_device(device_hits(batch, big, k, 1, 0, 3, SAMPLE, w_seeds.shape[0], w_hits.shape[0]), want, n, (k, "full batch"))


@pytest.mark.gpu
def test_buffer_contract(big):
    """7. Totals from a sizing call with NULL records; one seed or one hit short is refused with the right totals and nothing
    written, exact capacities succeed; minimizers_device one record short leaves the offsets complete and the records
    untouched.  Empty cases are fine."""
    from gcsa2_amd.binding import Gcsa2Error
    reads = reads_of(BIG)[90:130] + EDGE
    n = len(reads)
    oracle = MinSeeds(Seeds(indexed(BIG)[1], reads), *alphabet())
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    sentinel = np.uint64(SENTINEL)
    for k, w, hit_max, over in ((12, 5, 0, SKIP), (6, 3, 3, SAMPLE)):
        want = oracle.want(k, w, 0, hit_max, bool(over))
        m, h = want[1].shape[0], want[3].shape[0]
        assert m > 1 and h > 1
        got = device_hits(batch, big, k, w, 0, hit_max, over, 0, 0, records=False)
        assert got[0].code == TOO_SMALL and got[0].needed == (m, h) and untouched(got[1:]), (k, w)
        for mcap, hcap in ((m - 1, h), (m, h - 1)):
            got = device_hits(batch, big, k, w, 0, hit_max, over, mcap, hcap)
            assert got[0].code == TOO_SMALL and got[0].needed == (m, h) and untouched(got[1:]), (k, w, mcap, hcap)
            with pytest.raises(Gcsa2Error) as err:
                big.minimizer_hits_batch(flat, off, k, w, 0, hit_max, bool(over), out=(
                    np.zeros(n + 1, dtype=np.uint64), np.zeros((mcap, 5), dtype=np.uint64), np.zeros(mcap + 1, dtype=np.uint64), np.zeros(hcap, dtype=np.uint64)))
            assert err.value.code == TOO_SMALL and err.value.needed == (m, h)
        assert_device(device_hits(batch, big, k, w, 0, hit_max, over, m, h), want, n, (k, w, "exact"))
        assert_device(device_hits(batch, big, k, w, 0, hit_max, over, m, h, profiles=False), want, n, (k, w, "no profiles"))
        moff, mins = oracle.windows(k, w, 0)[5:7]
        total = mins.shape[0]
        res, got_moff, got_mins = device_minimizers(batch, big, k, w, 0, 0, records=False)
        assert res.code == TOO_SMALL and res.needed == total and np.array_equal(got_moff[:n + 1], moff) and (got_mins == sentinel).all()
        res, got_moff, got_mins = device_minimizers(batch, big, k, w, 0, total - 1)
        assert res.code == TOO_SMALL and res.needed == total
        assert np.array_equal(got_moff[:n + 1], moff) and (got_moff[n + 1:] == sentinel).all() and (got_mins == sentinel).all()
        with pytest.raises(Gcsa2Error) as err:
            big.minimizers_batch(flat, off, k, w, 0, out=(got_moff, np.full((total - 1, 2), SENTINEL, dtype=np.uint64)))
        assert err.value.code == TOO_SMALL and err.value.needed == total and np.array_equal(got_moff[:n + 1], moff)
    # no reads at all; reads all shorter than k; reads without a valid window; reads without a found minimizer
    for some, k in (([], 16), ([b"ACGT", b"", b"ACGTACG", b"A"], 8), ([b"NNNN", b"XYZ", b"NNNN", b""], 2), ([b"ACGTACGTACGTAAAACCCCGGGGTTTTACGT"], 32)):
        nn = len(some)
        small = DeviceReads(some)
        want = restate(some, k, 5, 0, *alphabet())
        res, soff, seeds, hoff, hits, prof = device_hits(small, big, k, 5, 0, 3, SAMPLE, 4, 4)
        assert res == (0, 0), (some, k)
        assert (soff[:nn + 1] == 0).all() and (soff[nn + 1:] == sentinel).all() and int(hoff[0]) == 0 and (hoff[1:] == sentinel).all()
        assert untouched([seeds, hits, prof[nn:]])
        assert prof[:nn].tolist() == [[int(c), 0, 0, 0] for c in np.diff(want[0].astype(np.int64))], (some, k)
        assert_selection(device_minimizers(small, big, k, 5, 0, want[1].shape[0]), want, nn, (some, k))
        got = big.minimizer_hits_batch(*concat_patterns(some), k, 5, 0, 3, True)
        assert got[0].tolist() == [0] * (nn + 1) and got[1].shape == (0, 5) and got[2].tolist() == [0] and got[3].shape == (0,)
        moff, mins = big.minimizers_batch(*concat_patterns(some), k, 5)
        assert np.array_equal(moff, want[0]) and np.array_equal(mins, want[1])


@pytest.mark.gpu
def test_refusals(engine, big, monkeypatch):
    """8. k = 0 and 33, w = 0 and 65, an unknown `over` and NULL totals are INVALID_ARGUMENT with nothing written; the hits need
    the samples (MISSING_COMPONENT); the selection alone works on a find-only image that has a jump table."""
    from gcsa2_amd.binding import Gcsa2Error
    reads = reads_of(BIG)
    n = len(reads)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    for k, w, over in ((0, 5, SKIP), (33, 5, SKIP), (8, 0, SKIP), (8, 65, SKIP), (8, 5, 7)):
        got = device_hits(batch, big, k, w, 0, 0, over, 64, 64)
        assert got[0].code == INVALID and got[0].needed == (0, 0) and untouched(got[1:]), (k, w, over)
        if over == SKIP:
            with pytest.raises(Gcsa2Error) as err:
                big.minimizer_hits_batch(flat, off, k, w, 0, 0, False)
            assert err.value.code == INVALID, (k, w)
            got = device_minimizers(batch, big, k, w, 0, 64)
            assert got[0].code == INVALID and got[0].needed == 0 and untouched(got[1:]), (k, w)
            with pytest.raises(Gcsa2Error) as err:
                big.minimizers_batch(flat, off, k, w)
            assert err.value.code == INVALID, (k, w)
    out = np.full(64, SENTINEL, dtype=np.uint64)
    total = ctypes.c_uint64(SENTINEL)
    p8, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    f, o = np.ascontiguousarray(flat, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64)
    L = big._L
    assert L.gcsa2_minimizers_batch(big._h, f.ctypes.data_as(p8), o.ctypes.data_as(p64), 2, 8, 5, 0, out.ctypes.data, out[8:].ctypes.data, 1, None) == INVALID
    assert L.gcsa2_minimizers_device(big._h, batch.d_pat.data_ptr(), batch.d_off.data_ptr(), 2, 8, 5, 0, out.ctypes.data, None, 0, None, None) == INVALID
    for totals in ((None, ctypes.byref(total)), (ctypes.byref(total), None)):
        assert L.gcsa2_minimizer_hits_batch(big._h, f.ctypes.data_as(p8), o.ctypes.data_as(p64), 2, 8, 5, 0, 0, SKIP, None, out.ctypes.data, out[8:].ctypes.data,
                                            1, totals[0], out[16:].ctypes.data, out[24:].ctypes.data, 1, totals[1]) == INVALID
        assert L.gcsa2_minimizer_hits_device(big._h, batch.d_pat.data_ptr(), batch.d_off.data_ptr(), 2, 8, 5, 0, 0, SKIP, None, out.ctypes.data, None,
                                             0, totals[0], out[16:].ctypes.data, None, 0, totals[1], None) == INVALID
    assert untouched([out]) and total.value == SENTINEL
    for bad in ([1, 20, 40], [0, 40, 20]):                   # the host forms refuse offsets that do not start at 0 or decrease
        o = np.asarray(bad, dtype=np.uint64)
        assert L.gcsa2_minimizers_batch(big._h, f.ctypes.data_as(p8), o.ctypes.data_as(p64), 2, 8, 5, 0, out.ctypes.data, out[8:].ctypes.data, 1,
                                        ctypes.byref(total)) == INVALID
        assert L.gcsa2_minimizer_hits_batch(big._h, f.ctypes.data_as(p8), o.ctypes.data_as(p64), 2, 8, 5, 0, 0, SKIP, None, out.ctypes.data, out[8:].ctypes.data,
                                            1, ctypes.byref(total), out[16:].ctypes.data, out[24:].ctypes.data, 1, ctypes.byref(total)) == INVALID
        assert untouched([out]), bad
    monkeypatch.setenv("GCSA2_JUMP_TABLE", "1")
    find_only = engine.GCSA(indexed(BIG)[0], with_samples=False, with_counters=False, with_lcp=False)
    monkeypatch.delenv("GCSA2_JUMP_TABLE")
    assert find_only.jump_table_bytes() > 0
    got = device_hits(batch, find_only, 16, 5, 0, 0, SKIP, 64, 64)
    assert got[0].code == MISSING and untouched(got[1:]), got[0]
    want = restate(reads, 16, 5, 0, *alphabet())
    assert_selection(device_minimizers(batch, find_only, 16, 5, 0, want[1].shape[0]), want, n, "find-only image")
    moff, mins = find_only.minimizers_batch(flat, off, 16, 5)
    assert np.array_equal(moff, want[0]) and np.array_equal(mins, want[1])
    find_only.close()


@pytest.mark.gpu
def test_independent_of_tables_and_pieces(engine, big, monkeypatch):
    """9. The same results with pair blocks and the seed table switched off, and from the host forms with the batch cut into
    several 1 MB pieces (library against library; the first repetition against the batch alone)."""
    reads = reads_of(BIG)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    default_k = big.kmer_table_k()
    cases = [(k, w, seed, hit_max, sample) for k, w, seed in ((8, 5, 0), (16, 11, OTHER_SEED), (32, 5, 0)) for hit_max, sample in ((0, False), (3, True))]
    base = {c: big.minimizer_hits_batch(flat, off, *c, profiles=True) for c in cases}
    assert all(v[1].shape[0] > 0 and v[3].shape[0] > 0 for v in base.values())
    try:
        for pair_blocks in (1, 0):
            for kmer_k in (0, default_k):
                big.set_tables(pair_blocks=pair_blocks, kmer_k=kmer_k)
                assert (big.pair_block_bytes() > 0) == bool(pair_blocks) and big.kmer_table_k() == kmer_k
                for c, want in base.items():
                    got = device_hits(batch, big, c[0], c[1], c[2], c[3], int(c[4]), want[1].shape[0], want[3].shape[0])
                    assert_device(got, want, len(reads), (pair_blocks, kmer_k, c))
    finally:
        big.set_tables(pair_blocks=1, kmer_k=default_k)
    monkeypatch.setenv("GCSA2_MS_PIECE_MB", "1")
    pieced, _ = engine.open_index(indexed(BIG)[0], device=0)
    monkeypatch.delenv("GCSA2_MS_PIECE_MB")
    repeats = (3 << 20) // sum(len(r) for r in reads) + 1
    many = reads * repeats
    many_flat, many_off = concat_patterns(many)
    assert int(many_off[-1]) >= 3 << 20                      # a piece holds at most 1 MB of reads: at least 3 pieces
    n = len(reads)
    for k, w, seed, hit_max, sample in ((32, 5, 0, 4, True), (16, 11, OTHER_SEED, 0, False)):
        a = pieced.minimizer_hits_batch(many_flat, many_off, k, w, seed, hit_max, sample, profiles=True)
        b = big.minimizer_hits_batch(many_flat, many_off, k, w, seed, hit_max, sample, profiles=True)
        assert_host(a, b, (k, w, "pieces"))
        alone = big.minimizer_hits_batch(flat, off, k, w, seed, hit_max, sample, profiles=True)
        m, h = alone[1].shape[0], alone[3].shape[0]
        assert m > 0 and h > 0 and a[1].shape[0] == repeats * m and a[3].shape[0] == repeats * h
        assert_host((a[0][:n + 1], a[1][:m], a[2][:m + 1], a[3][:h], a[4][:n]), alone, "first repetition")
        a = pieced.minimizers_batch(many_flat, many_off, k, w, seed)
        b = big.minimizers_batch(many_flat, many_off, k, w, seed)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (k, w, "pieces")
        alone = restate(reads, k, w, seed, *alphabet())
        total = alone[1].shape[0]
        assert total > 0 and a[1].shape[0] == repeats * total
        assert np.array_equal(a[0][:n + 1], alone[0]) and np.array_equal(a[1][:total], alone[1])
        assert np.array_equal(a[1][total * (repeats - 1):], alone[1])
    pieced.close()


@pytest.mark.gpu
def test_facade_minimizers(engine, tmp_path):
    """10. GCSA::minimizers and GCSA::minimizer_hits_batch from a C++ client (tests/cpp/minimizer_hits_client.cpp) print what the
    Python forms return."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    which = len(CASES) - 1
    reads = reads_of(which)
    assert all(b"\n" not in r for r in reads)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    save_host_view(indexed(which)[0], str(tmp_path / "index.g2hv"))
    (tmp_path / "reads.txt").write_bytes(b"".join(r + b"\n" for r in reads))
    exe = compile_client(str(tmp_path / "minimizer_hits_client"), os.path.join(ROOT, "tests", "cpp", "minimizer_hits_client.cpp"))
    data, off = concat_patterns(reads)
    for k, w, seed, hit_max, sample in ((5, 3, 0, 0, 0), (3, 2, OTHER_SEED, 3, 1), (7, 11, 1, 2, 0)):
        out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "reads.txt"), str(k), str(w), str(seed), str(hit_max), str(sample)],
                             capture_output=True, text=True, env=_run_env(), timeout=300)
        assert out.returncode == 0, out.stderr
        moff, mins = gpu.minimizers_batch(data, off, k, w, seed)
        soff, seeds, hoff, hits = gpu.minimizer_hits_batch(data, off, k, w, seed, hit_max, bool(sample))
        want = [f"read {q} {int(moff[q + 1] - moff[q])} {int(soff[q + 1] - soff[q])}" for q in range(len(reads))]
        want += [f"minimizer {i} {int(mins[i, 0])} {int(mins[i, 1])}" for i in range(mins.shape[0])]
        want += [f"seed {i} " + " ".join(str(int(x)) for x in seeds[i]) for i in range(seeds.shape[0])]
        want += [" ".join(["hits", str(i), str(int(hoff[i + 1] - hoff[i]))] + [str(int(v)) for v in hits[int(hoff[i]):int(hoff[i + 1])]])
                 for i in range(seeds.shape[0])]
        assert out.stdout.strip().split("\n") == want, (k, w, seed, hit_max, sample)
        assert mins.shape[0] >= seeds.shape[0] > 0 and hits.shape[0] > 0
    gpu.close()
