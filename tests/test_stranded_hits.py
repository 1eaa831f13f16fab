"""Stranded minimizer seeds (include/gcsa2_hip_strands.h; kernels_strands.hpp): gcsa2_canonical_minimizers_device / _batch and
gcsa2_stranded_minimizer_hits_device / _batch.  The selection is checked against a Python restatement of the header's definition
(vectorised here, and compared with a second, literal form of it).  Ranges, counts and hits are the CPU oracle's find / count /
locate on materialised strings: the batch P_0, R_0, P_1, R_1, ... with R = rc(P) made through the index's char2comp and its
inverse, of whose stride-1 windows (test_kmer_hits.Seeds, cached per graph and left unchanged) the selected ones are taken.

The batch of a graph is reads_of(which) plus the reverse complements of its unmutated walks: the graphs are forward-strand, so
without them the reverse groups are nearly empty at k >= 12."""
import ctypes
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import streams
from streams import Case, COMPLETE
from gcsa2_amd.hostview import concat_patterns
from test_oracle import CASES
from test_mem_hits import EDGE, SENTINEL
from test_extend import GRAPHS, BIG, indexed
from test_kmer_windows import reads_of, walks
from test_kmer_hits import Seeds, Spins, DeviceReads, assert_device, assert_host, untouched, GUARD, WAVE, WORKGROUP
from test_minimizer_hits import (mix64, mix64_np, alphabet, codes_of, random_read, tile_reads, device_hits as plain_device_hits, OTHER_SEED, SELECT_K,
                                 SELECT_W, HITS_W, HIT_MAX)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
INVALID, MISSING, TOO_SMALL = -1, -5, -6
SKIP, SAMPLE = 0, 1
FORWARD, REVERSE, BOTH = 1, 2, 3
NAMES = ("gcsa2_canonical_minimizers_device", "gcsa2_canonical_minimizers_batch", "gcsa2_stranded_minimizer_hits_device",
         "gcsa2_stranded_minimizer_hits_batch")


# ---- the definition, restated -----------------------------------------------------------------------------------------------

def key_of(code, j, k):
    return sum(code[j + i] << (2 * (k - 1 - i)) for i in range(k))


def rckey_of(code, j, k):
    return sum((3 - code[j + k - 1 - i]) << (2 * (k - 1 - i)) for i in range(k))


def literal(read, k, w, seed, c2c, sigma):
    """The definition word for word, for one read: [(position, chash, key, strand)] in ascending position."""
    code = [int(c) for c in codes_of(read, c2c, sigma)]
    W = max(0, len(read) - k + 1)
    valid = [all(code[j + i] >= 0 for i in range(k)) for j in range(W)]
    rec = {}
    for j in range(W):
        if valid[j]:
            key = key_of(code, j, k)
            hf, hr = mix64(key ^ seed), mix64(rckey_of(code, j, k) ^ seed)
            rec[j] = (min(hf, hr), key, 1 if hr < hf else 0)
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
            chosen.add(min((rec[j][0], j) for j in range(s, e))[1])
        a = b
    return [(j,) + rec[j] for j in sorted(chosen)]


def restate(reads, k, w, seed, c2c, sigma):
    """The definition for a batch, vectorised: (min_offsets (reads + 1), minimizers (total, 4) = {position, chash, key, strand}).
    The reads are laid end to end with one invalid character behind each, as test_minimizer_hits.restate does."""
    n = len(reads)
    codes = np.concatenate([np.concatenate([codes_of(r, c2c, sigma), [-1]]) for r in reads] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in reads])]).astype(np.int64)[:n]
    M = codes.shape[0] - k + 1
    if M <= 0:
        return np.zeros(n + 1, dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64)
    bad = np.concatenate([[0], np.cumsum(codes < 0)])
    valid = (bad[k:] - bad[:-k]) == 0
    key, rckey = np.zeros(M, dtype=np.uint64), np.zeros(M, dtype=np.uint64)
    for i in range(k):
        c = np.maximum(codes[i:i + M], 0).astype(np.uint64)
        key = (key << np.uint64(2)) | c
        rckey = rckey | ((np.uint64(3) - c) << np.uint64(2 * i))
    hf, hr = mix64_np(key ^ np.uint64(seed)), mix64_np(rckey ^ np.uint64(seed))
    hashes = np.minimum(hf, hr)
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
    mins = np.zeros((picked.shape[0], 4), dtype=np.uint64)
    mins[:, 0] = picked - starts[owner]
    mins[:, 1] = hashes[picked]
    mins[:, 2] = key[picked]
    mins[:, 3] = (hr[picked] < hf[picked])
    moff = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))]).astype(np.uint64)
    return moff, mins


def complement_table(c2c):
    """byte -> the byte of the complementary code (through char2comp and its inverse: the first byte of a comp); a byte
    without a code stays as it is, so that it is invalid on the other strand too."""
    first = {}
    for byte in range(256):
        first.setdefault(int(c2c[byte]), byte)
    table = np.arange(256, dtype=np.uint8)
    for byte in range(256):
        comp = int(c2c[byte])
        if 1 <= comp <= 4:
            table[byte] = first[1 + (3 - (comp - 1))]
    return table


def revcomp(read, c2c):
    return bytes(complement_table(c2c)[np.frombuffer(read, dtype=np.uint8)][::-1].tobytes())


@functools.lru_cache(maxsize=None)
def batch_of(which):
    """reads_of(which) plus the reverse complements of its unmutated walks (the first part of reads_of)."""
    reads = reads_of(which)
    base = walks(GRAPHS[which][1], 0x4B10 + which, 100 if which == BIG else 16)
    assert reads[:len(base)] == base
    c2c, _ = alphabet(which)
    return reads + [revcomp(r, c2c) for r in base], len(base)


class StrandSeeds:
    """The contract's arrays of the stranded hits for one batch: the oracle's stride-1 windows of P_0, R_0, P_1, R_1, ...
    (materialised), of which the restatement's canonical minimizers are taken on either strand."""

    def __init__(self, cpu, reads, c2c, sigma):
        self.reads, self.c2c, self.sigma = reads, c2c, sigma
        self.mirror = [revcomp(r, c2c) for r in reads]
        self.both = [x for pair in zip(reads, self.mirror) for x in pair]
        self.seeds = Seeds(cpu, self.both)
        self.cut = {}

    def windows(self, k, w, seed, strands):
        if (k, w, seed, strands) not in self.cut:
            n = len(self.reads)
            woff, _, rng, cnt = self.seeds.exp.want(k, 1)
            woff = woff.astype(np.int64)
            moff, mins = restate(self.reads, k, w, seed, self.c2c, self.sigma)
            owner = np.repeat(np.arange(n), np.diff(moff.astype(np.int64)))
            pos = mins[:, 0].astype(np.int64)
            length = np.asarray([len(r) for r in self.reads], dtype=np.int64)[owner] if n else np.zeros(0, dtype=np.int64)
            group = np.concatenate([2 * owner] * bool(strands & FORWARD) + [2 * owner + 1] * bool(strands & REVERSE)).astype(np.int64)
            where = np.concatenate([pos] * bool(strands & FORWARD) + [length - k - pos] * bool(strands & REVERSE)).astype(np.int64)
            order = np.lexsort((where, group))
            group, where = group[order], where[order]
            pick = woff[group] + where
            r, c = rng[pick], cnt[pick]
            nonempty = ((r[:, 0] + np.uint64(1)) <= (r[:, 1] + np.uint64(1))) if pick.size else np.zeros(0, dtype=bool)
            nodes = np.where(nonempty, r[:, 1] + np.uint64(1) - r[:, 0], np.uint64(0)).astype(np.uint64)
            prof = np.zeros((2 * n, 4), dtype=np.uint64)
            prof[:, 0] = np.bincount(group, minlength=2 * n)
            for column, values in ((1, nonempty), (2, nodes), (3, c)):
                np.add.at(prof[:, column], group, values.astype(np.uint64))
            records = np.zeros((int(nonempty.sum()), 5), dtype=np.uint64)
            records[:, 0], records[:, 1], records[:, 2:4], records[:, 4] = where[nonempty], k, r[nonempty], c[nonempty]
            soff = np.concatenate([[0], np.cumsum(prof[:, 1].astype(np.int64))]).astype(np.uint64)
            distinct, inverse = (np.unique(records[:, 2:5], axis=0, return_inverse=True) if records.shape[0]
                                 else (np.zeros((0, 3), dtype=np.uint64), np.zeros(0, dtype=np.int64)))
            self.cut[(k, w, seed, strands)] = (prof, records, soff, distinct, np.asarray(inverse).reshape(-1), moff, mins)
        return self.cut[(k, w, seed, strands)]

    def want(self, k, w, seed, strands, hit_max, sample):
        """(seed_offsets (2 n + 1), seeds, hit_offsets, hits, profiles (2 n))."""
        prof, records, soff, distinct, inverse, _, _ = self.windows(k, w, seed, strands)
        per_range = [np.asarray(self.seeds.hits((int(sp), int(ep)), int(c), hit_max, sample), dtype=np.uint64) for sp, ep, c in distinct.tolist()]
        sizes = np.asarray([a.shape[0] for a in per_range], dtype=np.int64)[inverse] if records.shape[0] else np.zeros(0, dtype=np.int64)
        hoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        hits = np.concatenate([per_range[i] for i in inverse.tolist()] + [np.zeros(0, dtype=np.uint64)]).astype(np.uint64)
        return soff, records, hoff, hits, prof


@functools.lru_cache(maxsize=None)
def stranded_of(which):
    return StrandSeeds(indexed(which)[1], batch_of(which)[0], *alphabet(which))


def interleave(fwd, rev):
    """The five arrays of GCSA2_STRAND_BOTH from those of FORWARD and REVERSE: group g of the one that has it."""
    f_soff, f_seeds, f_hoff, f_hits, f_prof = fwd
    r_soff, r_seeds, r_hoff, r_hits, r_prof = rev
    groups = f_soff.shape[0] - 1
    seeds, sizes, hits, per_group = [], [], [], []
    for g in range(groups):
        soff, rec, hoff, hit = (f_soff, f_seeds, f_hoff, f_hits) if g % 2 == 0 else (r_soff, r_seeds, r_hoff, r_hits)
        a, b = int(soff[g]), int(soff[g + 1])
        per_group.append(b - a)
        seeds.append(rec[a:b])
        sizes.append(np.diff(hoff[a:b + 1].astype(np.int64)))
        hits.append(hit[int(hoff[a]):int(hoff[b])])
    prof = np.where((np.arange(groups) % 2 == 0)[:, None], f_prof, r_prof).astype(np.uint64)
    return (np.concatenate([[0], np.cumsum(per_group)]).astype(np.uint64), np.concatenate(seeds + [np.zeros((0, 5), dtype=np.uint64)]),
            np.concatenate([[0], np.cumsum(np.concatenate(sizes + [np.zeros(0, dtype=np.int64)]))]).astype(np.uint64),
            np.concatenate(hits + [np.zeros(0, dtype=np.uint64)]), prof)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_stranded_calls_and_refuses_a_null_index():
    """1. The new header declares the four calls and the three GCSA2_STRAND_* constants, the built library exports them,
    STRAND_EXPORTS lists exactly them and none of them is in EXPORTS or CHAIN_EXPORTS; each refuses a NULL index with
    INVALID_ARGUMENT without a device, names the index and writes nothing."""
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    header = open(os.path.join(ROOT, "include", "gcsa2_hip_strands.h")).read()
    for name in NAMES:
        assert ("int " + name + "(") in header and hasattr(ctypes.CDLL(binding.LIB_PATH), name), name
        assert name not in binding.EXPORTS and name not in binding.CHAIN_EXPORTS, name
    assert sorted(binding.STRAND_EXPORTS) == sorted(NAMES)
    for name, value in (("FORWARD", 1), ("REVERSE", 2), ("BOTH", 3)):
        assert any(line.split()[:3] == ["#define", "GCSA2_STRAND_" + name, str(value)] for line in header.split("\n")), name
        assert getattr(binding, "STRAND_" + name) == value
    assert '#include "gcsa2_hip.h"' in header and "gcsa2_hip_strands.h" in open(os.path.join(ROOT, "include", "gcsa2_hip.h")).read()
    assert all(hasattr(binding.GCSA, m) for m in ("canonical_minimizers_device", "canonical_minimizers_batch", "stranded_minimizer_hits_device",
                                                  "stranded_minimizer_hits_batch"))
    lib = binding.load_library()
    off = (ctypes.c_uint64 * 2)(0, 8)
    pat = (ctypes.c_uint8 * 8)(*b"ACGTACGT")
    moff = (ctypes.c_uint64 * 2)(7, 7)
    mins = (ctypes.c_uint64 * 20)(*([7] * 20))
    total = ctypes.c_uint64(7)
    rc = lib.gcsa2_canonical_minimizers_device(None, ctypes.addressof(pat), ctypes.addressof(off), 1, 4, 2, 0, ctypes.addressof(moff), ctypes.addressof(mins), 5,
                                               ctypes.byref(total), None)
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    rc = lib.gcsa2_canonical_minimizers_batch(None, pat, off, 1, 4, 2, 0, ctypes.addressof(moff), ctypes.addressof(mins), 5, ctypes.byref(total))
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    assert list(moff) == [7, 7] and list(mins) == [7] * 20 and total.value == 7
    prof = (ctypes.c_uint64 * 8)(*([7] * 8))
    soff = (ctypes.c_uint64 * 3)(7, 7, 7)
    seeds = (ctypes.c_uint64 * 25)(*([7] * 25))
    hoff = (ctypes.c_uint64 * 6)(*([7] * 6))
    hits = (ctypes.c_uint64 * 8)(*([7] * 8))
    total_seeds, total_hits = ctypes.c_uint64(7), ctypes.c_uint64(7)
    outputs = (ctypes.addressof(prof), ctypes.addressof(soff), ctypes.addressof(seeds), 5, ctypes.byref(total_seeds), ctypes.addressof(hoff),
               ctypes.addressof(hits), 8, ctypes.byref(total_hits))
    rc = lib.gcsa2_stranded_minimizer_hits_device(None, ctypes.addressof(pat), ctypes.addressof(off), 1, 4, 2, 0, BOTH, 0, SKIP, *outputs, None)
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    rc = lib.gcsa2_stranded_minimizer_hits_batch(None, pat, off, 1, 4, 2, 0, BOTH, 0, SKIP, *outputs)
    assert rc == INVALID and "index" in lib.gcsa2_last_error().decode()
    assert list(prof) == [7] * 8 and list(soff) == [7] * 3 and list(seeds) == [7] * 25 and list(hoff) == [7] * 6 and list(hits) == [7] * 8
    assert total_seeds.value == 7 and total_hits.value == 7


def test_the_restatement_is_the_definition():
    """2. The vectorised restatement equals the literal form on random strings over ACGTNacgt$ of 0 .. 200 characters; rckey of
    rckey is key; a window that is its own reverse complement (even k only) has strand 0; a read that holds a window and its
    reverse complement inside one span selects the leftmost; and on reads in which no span holds two windows of one chash (a
    window and its reverse complement, or one k-mer twice) the canonical selection of rc(P) is the mirror image of that of P."""
    c2c, sigma = alphabet()
    assert sigma >= 6 and [int(c2c[c]) for c in b"ACGTacgt"] == [1, 2, 3, 4, 1, 2, 3, 4] and not 1 <= int(c2c[ord("N")]) <= 4
    assert revcomp(b"AACGTNacg$T", c2c) == b"A$CGTNACGTT"
    rng = np.random.default_rng(0x51A4D)
    reads = [random_read(rng, int(length), b"ACGTNacgt$" if i % 3 else b"ACGT") for i, length in enumerate(rng.integers(0, 201, 240))]
    reads[:3] = [b"", b"A" * 200, b"ACGT" * 50]
    mirrored = own = 0
    for k in (1, 4, 16, 32):
        for w in (1, 2, 5, 11, 64):
            for seed in (0, OTHER_SEED):
                moff, mins = restate(reads, k, w, seed, c2c, sigma)
                back = restate([revcomp(r, c2c) for r in reads], k, w, seed, c2c, sigma)
                assert moff.shape[0] == len(reads) + 1 and int(moff[-1]) == mins.shape[0]
                for q, r in enumerate(reads):
                    got = [tuple(int(x) for x in row) for row in mins[int(moff[q]):int(moff[q + 1])].tolist()]
                    want = literal(r, k, w, seed, c2c, sigma)
                    assert got == want, (k, w, seed, q, r)
                    code = [int(c) for c in codes_of(r, c2c, sigma)]
                    for j, chash, key, strand in want:
                        rckey = rckey_of(code, j, k)
                        assert key == key_of(code, j, k) and chash == min(mix64(key ^ seed), mix64(rckey ^ seed))
                        flipped = [3 - ((rckey >> (2 * (k - 1 - i))) & 3) for i in range(k)][::-1]
                        assert sum(c << (2 * (k - 1 - i)) for i, c in enumerate(flipped)) == key          # rckey of rckey
                        if rckey == key:
                            assert k % 2 == 0 and strand == 0, (k, j)
                            own += 1
                    # the mirror image, where no span holds one chash twice
                    if seed != 0 or w not in (5, 11):
                        continue
                    W = max(0, len(r) - k + 1)
                    every = literal(r, k, 1, seed, c2c, sigma)
                    clash = any(a[1] == b[1] and b[0] - a[0] < w for i, a in enumerate(every) for b in every[i + 1:i + w])
                    if not clash:
                        theirs = back[1][int(back[0][q]):int(back[0][q + 1])]
                        assert sorted(W - 1 - int(p) for p in theirs[:, 0]) == [j for j, _, _, _ in want], (k, w, q)
                        assert sorted(int(h) for h in theirs[:, 1]) == sorted(h for _, h, _, _ in want)
                        mirrored += bool(want)
    assert mirrored > 200 and own > 50, (mirrored, own)
    assert rckey_of([0, 1, 2, 3], 0, 4) == key_of([0, 1, 2, 3], 0, 4)          # ACGT is its own reverse complement
    # a window and its reverse complement in one span: the leftmost is selected, the other one is not
    x = b"ACGGT"
    read = x + revcomp(x, c2c)
    assert read[5:] != x and len(read) == 10
    for seed in range(200):
        every = literal(read, 5, 1, seed, c2c, sigma)
        assert every[0][1] == every[5][1] and every[0][3] != every[5][3]
        if every[0][1] == min(e[1] for e in every):
            assert [m[0] for m in literal(read, 5, 6, seed, c2c, sigma)] == [0]
            moff, mins = restate([read], 5, 6, seed, c2c, sigma)
            assert mins[:, 0].tolist() == [0]
            break
    else:
        raise AssertionError("no hash seed makes the pair the span's minimum")


def test_the_batches_are_not_vacuous():
    """3. On the 6000-base graph: at (16, 11) both strands are selected, and over all valid 16-mers of the existing reads 5035
    windows have strand 0 and 5172 strand 1; the walks have found seeds in their even group only, their reverse complements
    in their odd group only; at k = 8 some reads have found seeds in both groups, 2271 reverse-complement stride-1 windows of the
    existing reads are found, and there are counts at or below and above the caps 1 and 3; at k = 4 there are selected windows
    that are their own reverse complement."""
    c2c, sigma = alphabet()
    big = stranded_of(BIG)
    reads, walks_n = batch_of(BIG)
    old = len(reads_of(BIG))
    n = len(reads)
    assert n == old + walks_n
    mins = big.windows(16, 11, 0, BOTH)[6]
    assert int((mins[:, 3] == 0).sum()) > 100 and int((mins[:, 3] == 1).sum()) > 100
    moff, every = restate(reads_of(BIG), 16, 1, 0, c2c, sigma)
    assert (int((every[:, 3] == 0).sum()), int((every[:, 3] == 1).sum())) == (5035, 5172)
    prof = big.windows(16, 11, 0, BOTH)[0]
    found = prof[:, 1].astype(np.int64).reshape(n, 2)
    windows = prof[:, 0].astype(np.int64).reshape(n, 2)
    assert (windows[:, 0] == windows[:, 1]).all()
    assert (found[:walks_n, 1] == 0).all() and int((found[:walks_n, 0] > 0).sum()) >= walks_n - 5, found[:walks_n].tolist()
    assert (found[old:, 0] == 0).all() and int((found[old:, 1] > 0).sum()) >= walks_n - 5, found[old:].tolist()
    assert np.array_equal(found[:walks_n, 0], found[old:, 1])                                 # the same windows, from the other side
    prof8, records8 = big.windows(8, 5, 0, BOTH)[:2]
    found8 = prof8[:, 1].astype(np.int64).reshape(n, 2)
    assert int(((found8[:, 0] > 0) & (found8[:, 1] > 0)).sum()) > 10
    all8 = big.windows(8, 1, 0, REVERSE)[0]
    valid_found = int(all8[1:2 * old:2, 1].astype(np.int64).sum())
    woff, _, rng, _ = big.seeds.exp.want(8, 1)
    odd = np.concatenate([np.arange(int(woff[2 * q + 1]), int(woff[2 * q + 2])) for q in range(old)])
    stride1_found = int(((rng[odd, 0] + np.uint64(1)) <= (rng[odd, 1] + np.uint64(1))).sum())
    assert stride1_found == 2271 and 0 < valid_found <= stride1_found, (stride1_found, valid_found)
    for cap in (1, 3):
        counts = records8[:, 4]
        assert int((counts <= np.uint64(cap)).sum()) > 0 and int((counts > np.uint64(cap)).sum()) > 0, cap
    mins4 = big.windows(4, 5, 0, BOTH)[6]
    rc4 = np.zeros(mins4.shape[0], dtype=np.uint64)
    for i in range(4):
        rc4 |= (np.uint64(3) - ((mins4[:, 2] >> np.uint64(2 * (3 - i))) & np.uint64(3))) << np.uint64(2 * i)
    assert int((rc4 == mins4[:, 2]).sum()) > 0 and (mins4[rc4 == mins4[:, 2], 3] == 0).all()


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
    """gcsa2_canonical_minimizers_device on sentinel-filled buffers with GUARD entries behind each: (result or Gcsa2Error,
    min_offsets, minimizers), whole buffers."""
    import torch
    from gcsa2_amd.binding import Gcsa2Error
    s = np.uint64(SENTINEL).view(np.int64).item()
    d_moff = torch.full((batch.n + 1 + GUARD,), s, dtype=torch.int64, device=batch.dev)
    d_mins = torch.full((capacity + GUARD, 4), s, dtype=torch.int64, device=batch.dev)
    try:
        res = gpu.canonical_minimizers_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, k, w, seed, d_moff.data_ptr(),
                                              d_mins.data_ptr() if records else 0, capacity if records else 0)
    except Gcsa2Error as e:
        res = e
    torch.cuda.synchronize()
    return res, d_moff.cpu().numpy().view(np.uint64), d_mins.cpu().numpy().view(np.uint64)


def device_hits(batch, gpu, k, w, seed, strands, hit_max, over, seed_capacity, hit_capacity, profiles=True, records=True):
    """gcsa2_stranded_minimizer_hits_device on sentinel-filled buffers, as test_kmer_hits.DeviceReads.hits, for 2 n groups."""
    import torch
    from gcsa2_amd.binding import Gcsa2Error
    s = np.uint64(SENTINEL).view(np.int64).item()
    groups = 2 * batch.n
    d_prof = torch.full((groups + GUARD, 4), s, dtype=torch.int64, device=batch.dev) if profiles else None
    d_soff = torch.full((groups + 1 + GUARD,), s, dtype=torch.int64, device=batch.dev)
    d_seeds = torch.full((seed_capacity + GUARD, 5), s, dtype=torch.int64, device=batch.dev)
    d_hoff = torch.full((seed_capacity + 1 + GUARD,), s, dtype=torch.int64, device=batch.dev)
    d_hits = torch.full((hit_capacity + GUARD,), s, dtype=torch.int64, device=batch.dev)
    try:
        res = gpu.stranded_minimizer_hits_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), batch.n, k, w, seed, strands, hit_max, over,
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
    """4. canonical_minimizers_device and canonical_minimizers_batch equal the restatement exactly -- offsets, positions, hashes,
    keys, strands -- for every k, w and two hash seeds, and the guards behind the buffers stay intact."""
    reads = batch_of(which)[0]
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
                moff, mins = gpu.canonical_minimizers_batch(flat, off, k, w, seed)
                assert np.array_equal(moff, want[0]) and np.array_equal(mins, want[1]), what + ("host",)
    gpu.close()


@pytest.mark.gpu
def test_selection_on_tile_edges(big):
    """4. (continued) The reads of test_minimizer_hits.tile_reads: 0, 1, w - 1, w, w + 1, 63 .. 65 and 127 .. 129 windows, an N at
    each tile edge, runs shorter than w, every byte offset of a word, in a pattern buffer of exactly total + 8 bytes."""
    c2c, sigma = alphabet()
    rng = np.random.default_rng(0x711F)
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
            moff, mins = big.canonical_minimizers_batch(flat, off, k, w, 0)
            want = restate(reads, k, w, 0, c2c, sigma)
            assert np.array_equal(moff, want[0]) and np.array_equal(mins, want[1]), ("tiles, host", k, w)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_hits_parity(engine, which):
    """5. stranded_minimizer_hits_device and stranded_minimizer_hits_batch equal the oracle-derived (seed_offsets, seeds,
    hit_offsets, hits, profiles) exactly, for each of the three `strands`, every k, w, cap and policy; the guards stay intact;
    BOTH is the interleave of FORWARD and REVERSE.  A range the reference would draw forever on is handled as in
    test_minimizer_hits.py and never occurs for the caps 1, 3 and 64.  Below k = 4 a window occurs hundreds of times, and an
    uncapped hit list (hit_max 0 or 2^64 - 1) of the whole batch has tens of millions of entries: those combinations run on every
    16th read of the batch (reads, mutated reads, reads with an N, edge reads and reverse complements are all among them)."""
    from gcsa2_amd.binding import Gcsa2Error
    oracle = stranded_of(which)
    reads = batch_of(which)[0]
    n = len(reads)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    whole = (oracle, reads, n, DeviceReads(reads)) + concat_patterns(reads)
    few = reads[::16]
    light = (StrandSeeds(indexed(which)[1], few, *alphabet(which)), few, len(few), DeviceReads(few)) + concat_patterns(few)
    kmer_k = gpu.kmer_table_k()
    spun = 0
    for k in sorted({1, 4, 8, 16, 32} | {x for x in (kmer_k - 1, kmer_k, kmer_k + 1) if 1 <= x <= 32}):
        for w in HITS_W:
            for hit_max in HIT_MAX:
                oracle, reads, n, batch, flat, off = light if k < 4 and hit_max in (0, U64) else whole
                for sample in (False, True):
                    what = (GRAPHS[which][0], k, w, hit_max, sample)
                    try:
                        want = {s: oracle.want(k, w, 0, s, hit_max, sample) for s in (FORWARD, REVERSE, BOTH)}
                    except Spins:
                        spun += 1
                        assert hit_max not in (1, 3, 64), what
                        with pytest.raises(Gcsa2Error) as err:
                            gpu.stranded_minimizer_hits_batch(flat, off, k, w, 0, BOTH, hit_max, sample)
                        assert err.value.code == INVALID and "max_positions" in str(err.value), what
                        continue
                    assert_host(interleave(want[FORWARD], want[REVERSE]), want[BOTH], what + ("the interleave",))
                    for s in (FORWARD, REVERSE, BOTH):
                        m, h = want[s][1].shape[0], want[s][3].shape[0]
                        assert_device(device_hits(batch, gpu, k, w, 0, s, hit_max, int(sample), m, h), want[s], 2 * n, what + (s, "device"))
                        assert_host(gpu.stranded_minimizer_hits_batch(flat, off, k, w, 0, s, hit_max, sample, profiles=True), want[s], what + (s, "host"))
    assert spun <= 16, spun
    oracle, reads, n, batch, flat, off = whole
    want = oracle.want(8, 5, OTHER_SEED, BOTH, 3, True)
    assert_device(device_hits(batch, gpu, 8, 5, OTHER_SEED, BOTH, 3, SAMPLE, want[1].shape[0], want[3].shape[0]), want, 2 * n, "another seed")
    gpu.close()


def spread(soff, parity, n):
    """The seed offsets over 2 n groups of a CSR over n reads whose groups have the given parity; the others are empty."""
    soff = np.asarray(soff[:n + 1], dtype=np.uint64)
    return np.concatenate([soff[:1], np.repeat(soff[1:], 2)] if parity == 0 else [np.repeat(soff[:n], 2), soff[n:]])


@pytest.mark.gpu
def test_w_1_is_the_plain_call_on_either_strand(big):
    """6. Library against library at w = 1, where every valid window is selected whatever its hash: the even groups equal
    minimizer_hits_device(k, w = 1) on the reads byte for byte -- seeds, hit offsets and hits --, the odd groups equal that call
    on the materialised reverse complements, and BOTH is their interleave."""
    reads = batch_of(BIG)[0]
    n = len(reads)
    c2c, _ = alphabet()
    mirror = [revcomp(r, c2c) for r in reads]
    batch, other = DeviceReads(reads), DeviceReads(mirror)
    assert spread(np.arange(4, dtype=np.uint64), 0, 3).tolist() == [0, 1, 1, 2, 2, 3, 3] and spread(np.arange(4, dtype=np.uint64), 1, 3).tolist() == [0, 0, 1, 1, 2, 2, 3]
    for k in (4, 16, 32):
        got = {}
        for strands, plain_batch, parity in ((FORWARD, batch, 0), (REVERSE, other, 1)):
            sizes = plain_device_hits(plain_batch, big, k, 1, 0, 3, SAMPLE, 0, 0, records=False)[0].needed
            assert sizes[0] > 0 and sizes[1] > 0, (k, strands)
            res, soff, seeds, hoff, hits, prof = plain_device_hits(plain_batch, big, k, 1, 0, 3, SAMPLE, *sizes)
            assert res == sizes
            new = device_hits(batch, big, k, 1, 0, strands, 3, SAMPLE, *sizes)
            assert new[0] == sizes, (k, strands)
            for name, a, b in zip(("seeds", "hit_offsets", "hits"), (seeds, hoff, hits), new[2:5]):
                assert np.array_equal(a, b), (k, strands, name)
            assert np.array_equal(new[1][:2 * n + 1], spread(soff, parity, n)), (k, strands, "seed_offsets")
            w_prof = np.zeros((2 * n, 4), dtype=np.uint64)
            w_prof[parity::2] = prof[:n]
            assert np.array_equal(new[5][:2 * n], w_prof), (k, strands, "profiles")
            m, h = sizes
            got[strands] = (new[1][:2 * n + 1], new[2][:m], new[3][:m + 1], new[4][:h], new[5][:2 * n])
        want = interleave(got[FORWARD], got[REVERSE])
        assert_device(device_hits(batch, big, k, 1, 0, BOTH, 3, SAMPLE, want[1].shape[0], want[3].shape[0]), want, 2 * n, (k, "both"))


@pytest.mark.gpu
def test_order_across_wavefronts_and_workgroups(big):
    """7. Reads of 300 bases at w = 1: a group has more than 128 windows, so a read's two groups straddle wavefront and workgroup
    boundaries of the search, and the order in which wavefronts reserve their records can differ from window order.  All five
    arrays equal the oracle's; inside every group the positions ascend (the reverse group in ascending j')."""
    c2c, sigma = alphabet()
    long_walks = walks(GRAPHS[BIG][1], 0x57A4D, 12, lo=300, hi=300)
    reads = long_walks + [revcomp(r, c2c) for r in long_walks[:6]]
    n = len(reads)
    oracle = StrandSeeds(indexed(BIG)[1], reads, c2c, sigma)
    batch = DeviceReads(reads)
    for k, strands in ((8, BOTH), (16, BOTH), (8, REVERSE)):
        want = oracle.want(k, 1, 0, strands, 3, False)
        prof = want[4]
        asked = prof[:, 0].astype(np.int64)
        assert asked.max() > 2 * WAVE and int(asked.sum()) > 8 * WORKGROUP
        first = np.concatenate([[0], np.cumsum(asked)])[:-1]
        last = first + asked - 1
        has = asked > 0
        assert int((has & (first // WAVE != last // WAVE)).sum()) >= n and int((has & (first // WORKGROUP != last // WORKGROUP)).sum()) >= n
        m, h = want[1].shape[0], want[3].shape[0]
        assert 0 < m < int(asked.sum())
        got = device_hits(batch, big, k, 1, 0, strands, 3, SKIP, m, h)
        assert_device(got, want, 2 * n, (k, strands))
        soff, seeds = got[1].astype(np.int64), got[2]
        for g in range(2 * n):
            p = seeds[soff[g]:soff[g + 1], 0].astype(np.int64)
            assert (np.diff(p) > 0).all(), (k, strands, g)


@pytest.mark.gpu
def test_composition_with_clusters_and_chains(big):
    """8. The BOTH output goes into seed_clusters_device and seed_chains_device as it is, with n_groups = 2 n: at w = 1 the rows,
    summaries and stats equal the same calls on minimizer_hits_device(w = 1) of the interleaved batch P_0, R_0, P_1, R_1, ...,
    on the 6000-base graph with a coord_of_bin as in test_seed_chains.py."""
    import torch
    from test_kmer_classes import bins_of, to_device
    from test_seed_chains import params, UNKNOWN
    oracle = stranded_of(BIG)
    reads = batch_of(BIG)[0]
    n = len(reads)
    shift = 10
    n_bins = bins_of(BIG, shift)
    cmap = np.arange(n_bins, dtype=np.uint64) << np.uint64(shift)
    cmap[::11] = np.uint64(UNKNOWN)
    d_map = to_device(cmap)
    P = params(band=16, top_n=4, member_cap=4, lookback=32)
    batch, both = DeviceReads(reads), DeviceReads(oracle.both)
    dev = batch.dev
    anchors = 0
    for k, hit_max, over in ((16, 0, SKIP), (8, 8, SAMPLE)):
        sizes = device_hits(batch, big, k, 1, 0, BOTH, hit_max, over, 0, 0, records=False)[0].needed
        assert sizes == plain_device_hits(both, big, k, 1, 0, hit_max, over, 0, 0, records=False)[0].needed and sizes[0] > 0 and sizes[1] > 0
        m, h = sizes
        outs = []
        for stranded in (True, False):
            d_soff = torch.zeros(2 * n + 1, dtype=torch.int64, device=dev)
            d_seeds = torch.zeros((m, 5), dtype=torch.int64, device=dev)
            d_hoff = torch.zeros(m + 1, dtype=torch.int64, device=dev)
            d_hits = torch.zeros(h, dtype=torch.int64, device=dev)
            if stranded:
                res = big.stranded_minimizer_hits_device(batch.d_pat.data_ptr(), batch.d_off.data_ptr(), n, k, 1, 0, BOTH, hit_max, over, 0, d_soff.data_ptr(),
                                                         d_seeds.data_ptr(), m, d_hoff.data_ptr(), d_hits.data_ptr(), h)
            else:
                res = big.minimizer_hits_device(both.d_pat.data_ptr(), both.d_off.data_ptr(), 2 * n, k, 1, 0, hit_max, over, 0, d_soff.data_ptr(),
                                                d_seeds.data_ptr(), m, d_hoff.data_ptr(), d_hits.data_ptr(), h)
            assert res == sizes
            d_top = torch.zeros((2 * n, 4, 8), dtype=torch.int64, device=dev)
            d_sums = torch.zeros((2 * n, 3), dtype=torch.int64, device=dev)
            clusters = big.seed_clusters_device(d_soff.data_ptr(), 2 * n, d_seeds.data_ptr(), m, d_hoff.data_ptr(), d_hits.data_ptr(), h, shift, d_map.data_ptr(),
                                                n_bins, 16, 4, d_top.data_ptr(), d_sums.data_ptr())
            c_top = torch.zeros((2 * n, 4, 8), dtype=torch.int64, device=dev)
            c_members = torch.zeros((2 * n, 4, 4, 2), dtype=torch.int64, device=dev)
            c_sums = torch.zeros((2 * n, 3), dtype=torch.int64, device=dev)
            chains = big.seed_chains_device(d_soff.data_ptr(), 2 * n, d_seeds.data_ptr(), m, d_hoff.data_ptr(), d_hits.data_ptr(), h, shift, d_map.data_ptr(),
                                            n_bins, c_top.data_ptr(), c_members.data_ptr(), c_sums.data_ptr(), **P)
            torch.cuda.synchronize()
            outs.append((clusters, chains) + tuple(t.cpu().numpy() for t in (d_soff, d_seeds, d_hoff, d_hits, d_top, d_sums, c_top, c_members, c_sums)))
        assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1], (k, outs[0][:2], outs[1][:2])
        for name, a, b in zip(("seed_offsets", "seeds", "hit_offsets", "hits", "cluster rows", "cluster summaries", "chain rows", "chain members",
                               "chain summaries"), outs[0][2:], outs[1][2:]):
            assert np.array_equal(a, b), (k, name)
        assert outs[0][1]["groups"] == 2 * n and outs[0][1]["chains"] > 0 and outs[0][0]["groups"] == 2 * n
        rows = outs[0][8].reshape(n, 2, 4, 8)
        assert rows[:, 0].any() and rows[:, 1].any()                       # chains on either strand
        anchors += outs[0][1]["anchors"]
    assert anchors > 0


@pytest.mark.gpu
def test_buffer_contract(big):
    """9. Totals from a sizing call with NULL records; one seed or one hit short is refused with the right totals and nothing
    written, exact capacities succeed; canonical_minimizers_device one record short leaves the offsets complete and the
    records untouched.  The empty cases are fine."""
    from gcsa2_amd.binding import Gcsa2Error
    c2c, sigma = alphabet()
    some = reads_of(BIG)[90:130]
    reads = some + [revcomp(r, c2c) for r in reads_of(BIG)[:20]] + EDGE
    n = len(reads)
    oracle = StrandSeeds(indexed(BIG)[1], reads, c2c, sigma)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    sentinel = np.uint64(SENTINEL)
    for k, w, strands, hit_max, over in ((12, 5, BOTH, 0, SKIP), (6, 3, BOTH, 3, SAMPLE), (12, 5, REVERSE, 0, SKIP)):
        want = oracle.want(k, w, 0, strands, hit_max, bool(over))
        m, h = want[1].shape[0], want[3].shape[0]
        assert m > 1 and h > 1
        got = device_hits(batch, big, k, w, 0, strands, hit_max, over, 0, 0, records=False)
        assert got[0].code == TOO_SMALL and got[0].needed == (m, h) and untouched(got[1:]), (k, w)
        for mcap, hcap in ((m - 1, h), (m, h - 1)):
            got = device_hits(batch, big, k, w, 0, strands, hit_max, over, mcap, hcap)
            assert got[0].code == TOO_SMALL and got[0].needed == (m, h) and untouched(got[1:]), (k, w, mcap, hcap)
            with pytest.raises(Gcsa2Error) as err:
                big.stranded_minimizer_hits_batch(flat, off, k, w, 0, strands, hit_max, bool(over), out=(
                    np.zeros(2 * n + 1, dtype=np.uint64), np.zeros((mcap, 5), dtype=np.uint64), np.zeros(mcap + 1, dtype=np.uint64),
                    np.zeros(hcap, dtype=np.uint64)))
            assert err.value.code == TOO_SMALL and err.value.needed == (m, h)
        assert_device(device_hits(batch, big, k, w, 0, strands, hit_max, over, m, h), want, 2 * n, (k, w, "exact"))
        assert_device(device_hits(batch, big, k, w, 0, strands, hit_max, over, m, h, profiles=False), want, 2 * n, (k, w, "no profiles"))
        moff, mins = oracle.windows(k, w, 0, strands)[5:7]
        total = mins.shape[0]
        res, got_moff, got_mins = device_minimizers(batch, big, k, w, 0, 0, records=False)
        assert res.code == TOO_SMALL and res.needed == total and np.array_equal(got_moff[:n + 1], moff) and (got_mins == sentinel).all()
        res, got_moff, got_mins = device_minimizers(batch, big, k, w, 0, total - 1)
        assert res.code == TOO_SMALL and res.needed == total
        assert np.array_equal(got_moff[:n + 1], moff) and (got_moff[n + 1:] == sentinel).all() and (got_mins == sentinel).all()
        with pytest.raises(Gcsa2Error) as err:
            big.canonical_minimizers_batch(flat, off, k, w, 0, out=(got_moff, np.full((total - 1, 4), SENTINEL, dtype=np.uint64)))
        assert err.value.code == TOO_SMALL and err.value.needed == total and np.array_equal(got_moff[:n + 1], moff)
    # no reads at all; reads all shorter than k; reads without a valid window; reads without a found minimizer on either strand
    for some, k in (([], 16), ([b"ACGT", b"", b"ACGTACG", b"A"], 8), ([b"NNNN", b"XYZ", b"NNNN", b""], 2), ([b"ACGTACGTACGTAAAACCCCGGGGTTTTACGT"], 32)):
        nn = len(some)
        small = DeviceReads(some)
        want = restate(some, k, 5, 0, c2c, sigma)
        res, soff, seeds, hoff, hits, prof = device_hits(small, big, k, 5, 0, BOTH, 3, SAMPLE, 4, 4)
        assert res == (0, 0), (some, k)
        assert (soff[:2 * nn + 1] == 0).all() and (soff[2 * nn + 1:] == sentinel).all() and int(hoff[0]) == 0 and (hoff[1:] == sentinel).all()
        assert untouched([seeds, hits, prof[2 * nn:]])
        assert prof[:2 * nn].tolist() == [[int(c), 0, 0, 0] for c in np.repeat(np.diff(want[0].astype(np.int64)), 2)], (some, k)
        assert_selection(device_minimizers(small, big, k, 5, 0, want[1].shape[0]), want, nn, (some, k))
        got = big.stranded_minimizer_hits_batch(*concat_patterns(some), k, 5, 0, BOTH, 3, True)
        assert got[0].tolist() == [0] * (2 * nn + 1) and got[1].shape == (0, 5) and got[2].tolist() == [0] and got[3].shape == (0,)
        moff, mins = big.canonical_minimizers_batch(*concat_patterns(some), k, 5)
        assert np.array_equal(moff, want[0]) and np.array_equal(mins, want[1])


@pytest.mark.gpu
def test_refusals(engine, big, monkeypatch):
    """9. (continued) k = 0 and 33, w = 0 and 65, strands 0 and 4, an unknown `over` and NULL totals are INVALID_ARGUMENT with
    nothing written; host offsets that do not start at 0 or that decrease are refused; the hits need the samples
    (MISSING_COMPONENT); the selection alone works on a find-only image."""
    from gcsa2_amd.binding import Gcsa2Error
    reads = batch_of(BIG)[0]
    n = len(reads)
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    for k, w, strands, over in ((0, 5, BOTH, SKIP), (33, 5, BOTH, SKIP), (8, 0, BOTH, SKIP), (8, 65, BOTH, SKIP), (8, 5, 0, SKIP), (8, 5, 4, SKIP),
                                (8, 5, -1, SKIP), (8, 5, BOTH, 7)):
        got = device_hits(batch, big, k, w, 0, strands, 0, over, 64, 64)
        assert got[0].code == INVALID and got[0].needed == (0, 0) and untouched(got[1:]), (k, w, strands, over)
        if over == SKIP:
            with pytest.raises(Gcsa2Error) as err:
                big.stranded_minimizer_hits_batch(flat, off, k, w, 0, strands, 0, False)
            assert err.value.code == INVALID, (k, w, strands)
        if over == SKIP and strands == BOTH:
            got = device_minimizers(batch, big, k, w, 0, 64)
            assert got[0].code == INVALID and got[0].needed == 0 and untouched(got[1:]), (k, w)
            with pytest.raises(Gcsa2Error) as err:
                big.canonical_minimizers_batch(flat, off, k, w)
            assert err.value.code == INVALID, (k, w)
    out = np.full(64, SENTINEL, dtype=np.uint64)
    total = ctypes.c_uint64(SENTINEL)
    p8, p64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
    f, o = np.ascontiguousarray(flat, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.uint64)
    L = big._L
    assert L.gcsa2_canonical_minimizers_batch(big._h, f.ctypes.data_as(p8), o.ctypes.data_as(p64), 2, 8, 5, 0, out.ctypes.data, out[8:].ctypes.data, 1, None) == INVALID
    assert L.gcsa2_canonical_minimizers_device(big._h, batch.d_pat.data_ptr(), batch.d_off.data_ptr(), 2, 8, 5, 0, out.ctypes.data, None, 0, None, None) == INVALID
    for totals in ((None, ctypes.byref(total)), (ctypes.byref(total), None)):
        assert L.gcsa2_stranded_minimizer_hits_batch(big._h, f.ctypes.data_as(p8), o.ctypes.data_as(p64), 2, 8, 5, 0, BOTH, 0, SKIP, None, out.ctypes.data,
                                                     out[8:].ctypes.data, 1, totals[0], out[16:].ctypes.data, out[24:].ctypes.data, 1, totals[1]) == INVALID
        assert L.gcsa2_stranded_minimizer_hits_device(big._h, batch.d_pat.data_ptr(), batch.d_off.data_ptr(), 2, 8, 5, 0, BOTH, 0, SKIP, None, out.ctypes.data,
                                                      None, 0, totals[0], out[16:].ctypes.data, None, 0, totals[1], None) == INVALID
    assert untouched([out]) and total.value == SENTINEL
    for bad in ([1, 20, 40], [0, 40, 20]):                   # the host forms refuse offsets that do not start at 0 or decrease
        o = np.asarray(bad, dtype=np.uint64)
        assert L.gcsa2_canonical_minimizers_batch(big._h, f.ctypes.data_as(p8), o.ctypes.data_as(p64), 2, 8, 5, 0, out.ctypes.data, out[8:].ctypes.data, 1,
                                                  ctypes.byref(total)) == INVALID
        assert L.gcsa2_stranded_minimizer_hits_batch(big._h, f.ctypes.data_as(p8), o.ctypes.data_as(p64), 2, 8, 5, 0, BOTH, 0, SKIP, None, out.ctypes.data,
                                                     out[8:].ctypes.data, 1, ctypes.byref(total), out[16:].ctypes.data, out[24:].ctypes.data, 1,
                                                     ctypes.byref(total)) == INVALID
        assert untouched([out]), bad
    find_only = engine.GCSA(indexed(BIG)[0], with_samples=False, with_counters=False, with_lcp=False)
    got = device_hits(batch, find_only, 16, 5, 0, BOTH, 0, SKIP, 64, 64)
    assert got[0].code == MISSING and untouched(got[1:]), got[0]
    with pytest.raises(Gcsa2Error) as err:
        find_only.stranded_minimizer_hits_batch(flat, off, 16, 5)
    assert err.value.code == MISSING
    want = restate(reads, 16, 5, 0, *alphabet())
    assert_selection(device_minimizers(batch, find_only, 16, 5, 0, want[1].shape[0]), want, n, "find-only image")
    moff, mins = find_only.canonical_minimizers_batch(flat, off, 16, 5)
    assert np.array_equal(moff, want[0]) and np.array_equal(mins, want[1])
    find_only.close()


@pytest.mark.gpu
def test_independent_of_tables_and_pieces(engine, big, monkeypatch):
    """10. The same results with pair blocks and the seed table switched off (set_tables), and from the host forms with the batch
    cut into several 1 MB pieces (library against library; the first repetition against the batch alone)."""
    reads = batch_of(BIG)[0]
    batch = DeviceReads(reads)
    flat, off = concat_patterns(reads)
    default_k = big.kmer_table_k()
    cases = [(k, w, seed, strands, hit_max, sample) for k, w, seed, strands in ((8, 5, 0, BOTH), (16, 11, OTHER_SEED, BOTH), (32, 5, 0, REVERSE),
                                                                                  (max(default_k, 4), 1, 0, BOTH))
             for hit_max, sample in ((0, False), (3, True))] + [(1, 5, 0, BOTH, 3, True), (max(default_k - 1, 1), 5, 0, BOTH, 3, True)]
    base = {c: big.stranded_minimizer_hits_batch(flat, off, *c, profiles=True) for c in cases}
    assert all(v[1].shape[0] > 0 and v[3].shape[0] > 0 for v in base.values())
    try:
        for pair_blocks in (1, 0):
            for kmer_k in (0, default_k):
                big.set_tables(pair_blocks=pair_blocks, kmer_k=kmer_k)
                assert (big.pair_block_bytes() > 0) == bool(pair_blocks) and big.kmer_table_k() == kmer_k
                for c, want in base.items():
                    got = device_hits(batch, big, c[0], c[1], c[2], c[3], c[4], int(c[5]), want[1].shape[0], want[3].shape[0])
                    assert_device(got, want, 2 * len(reads), (pair_blocks, kmer_k, c))
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
    for k, w, seed, strands, hit_max, sample in ((32, 5, 0, BOTH, 4, True), (16, 11, OTHER_SEED, BOTH, 0, False), (16, 11, 0, REVERSE, 0, False)):
        a = pieced.stranded_minimizer_hits_batch(many_flat, many_off, k, w, seed, strands, hit_max, sample, profiles=True)
        b = big.stranded_minimizer_hits_batch(many_flat, many_off, k, w, seed, strands, hit_max, sample, profiles=True)
        assert_host(a, b, (k, w, "pieces"))
        alone = big.stranded_minimizer_hits_batch(flat, off, k, w, seed, strands, hit_max, sample, profiles=True)
        m, h = alone[1].shape[0], alone[3].shape[0]
        assert m > 0 and h > 0 and a[1].shape[0] == repeats * m and a[3].shape[0] == repeats * h
        assert_host((a[0][:2 * n + 1], a[1][:m], a[2][:m + 1], a[3][:h], a[4][:2 * n]), alone, "first repetition")
        assert np.array_equal(a[1][m * (repeats - 1):], alone[1]) and np.array_equal(a[4][2 * n * (repeats - 1):], alone[4])
        a = pieced.canonical_minimizers_batch(many_flat, many_off, k, w, seed)
        b = big.canonical_minimizers_batch(many_flat, many_off, k, w, seed)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (k, w, "pieces")
        alone = restate(reads, k, w, seed, *alphabet())
        total = alone[1].shape[0]
        assert total > 0 and a[1].shape[0] == repeats * total
        assert np.array_equal(a[0][:n + 1], alone[0]) and np.array_equal(a[1][:total], alone[1])
        assert np.array_equal(a[1][total * (repeats - 1):], alone[1])
    pieced.close()


# ---- the stream contract of the new header -------------------------------------------------------------------------------------
# One row per binding method: the C entry point it reaches and its contract class, in the header's words.
TABLE = {
    "canonical_minimizers_device":     ("gcsa2_canonical_minimizers_device", COMPLETE),
    "stranded_minimizer_hits_device":  ("gcsa2_stranded_minimizer_hits_device", COMPLETE),
}
BUILDERS = {}


def test_every_stream_entry_point_of_the_strands_header_has_a_row():
    """A declaration of include/gcsa2_hip_strands.h with a `void* stream` parameter (found with the regular expression of
    tests/test_stream_contract.py) has a row in TABLE; every row names a declaration and its binding method exists."""
    import test_stream_contract as contract
    from gcsa2_amd import binding
    with open(os.path.join(ROOT, "include", "gcsa2_hip_strands.h")) as f:
        declared = contract.declarations_with_a_stream(f.read())
    assert declared == {"gcsa2_canonical_minimizers_device", "gcsa2_stranded_minimizer_hits_device"}
    assert {c for c, _ in TABLE.values()} == declared
    assert all(hasattr(binding.GCSA, row) for row in TABLE)
    assert set(TABLE) == set(BUILDERS)


def selection_row(env, name):
    import test_stream_contract as contract
    ins, n, total = contract.reads_input()
    k, w = 8, 5
    host = [env.gpu.canonical_minimizers_batch(*env.flat(x), k, w, 7) for x in (0, 1)]
    cap = contract.sized(*(h[1].shape[0] for h in host))
    return Case(name, COMPLETE, ins, {"moff": 8 * (n + 1), "mins": 32 * cap},
                lambda p, s: env.gpu.canonical_minimizers_device(p["pat"], p["off"], n, k, w, 7, p["moff"], p["mins"], cap, s),
                view=lambda raw, total_: {"moff": raw["moff"], "mins": raw["mins"][:32 * total_]})


def hits_row(env, name):
    import test_stream_contract as contract
    ins, n, total = contract.reads_input()
    k, w = 8, 5
    host = [env.gpu.stranded_minimizer_hits_batch(*env.flat(x), k, w, 7, BOTH, contract.HIT_MAX, True) for x in (0, 1)]
    mcap, hcap = contract.sized(*(h[1].shape[0] for h in host)), contract.sized(*(h[3].shape[0] for h in host))
    return Case(name, COMPLETE, ins, contract.csr_outputs(2 * n, mcap, hcap, True),
                lambda p, s: env.gpu.stranded_minimizer_hits_device(p["pat"], p["off"], n, k, w, 7, BOTH, contract.HIT_MAX, contract.SAMPLE, p["prof"],
                                                                    p["soff"], p["seeds"], mcap, p["hoff"], p["hits"], hcap, s),
                view=contract.cut_csr(2 * n, "soff", 40))


BUILDERS["canonical_minimizers_device"] = selection_row
BUILDERS["stranded_minimizer_hits_device"] = hits_row


@pytest.fixture(scope="module")
def env(engine, big):
    import test_stream_contract as contract
    return contract.Env(engine, big, None, None, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TABLE))
def test_entry_point_on_a_caller_stream(env, name):
    """11. Both probes of tests/streams.py -- the caller's stream delayed with a decoy batch in place, and the null stream busy --
    and nothing left on the stream when the call returns, for one row."""
    case = BUILDERS[name](env, name)
    assert case.contract == TABLE[name][1]
    ms = case.time_ms()
    print(f"stream_contract timing: {name} {ms:.3f} ms (delay {streams.DELAY_MS:.0f} ms)")
    assert ms < streams.DELAY_MS, (name, ms, "the delay no longer outlasts the call: a smaller row, or a longer delay")
    streams.probe_delayed_inputs(case)
    streams.probe_busy_null_stream(case)


@pytest.mark.gpu
def test_two_callers_at_once(env):
    """11. (continued) Two host threads call both entry points at once on one handle, each on a stream of its own, four rounds in
    opposite order; every output equals what the call gave alone.  Errors are asserted in the main thread."""
    import torch
    cases = [BUILDERS[name](env, name) for name in sorted(TABLE)]
    want = {c.name: c.expected(0) for c in cases}
    threads_n, rounds = 2, 4
    plan = {(t, r, i): (cases[(i + t) % 2], cases[(i + t) % 2].device_inputs(0), cases[(i + t) % 2].device_outputs())
            for t in range(threads_n) for r in range(rounds) for i in range(2)}
    stream_of = [torch.cuda.Stream() for _ in range(threads_n)]
    torch.cuda.synchronize()
    errors, start = [], threading.Barrier(threads_n)

    def worker(t):
        try:
            S = stream_of[t]
            start.wait()
            for r in range(rounds):
                done = []
                for i in range(2):
                    c, ins, outs = plan[(t, r, i)]
                    done.append((c, ins, outs, c.run(ins, outs, S.cuda_stream)))
                S.synchronize()
                for c, ins, outs, result in done:
                    c.assert_equal(c.collect(ins, outs, result, "concurrent", stream=S), want[c.name], ("thread", t, "round", r))
        except Exception as e:          # noqa: BLE001  (reported below, in the main thread)
            errors.append((t, repr(e)))
            start.abort()

    workers = [threading.Thread(target=worker, args=(t,)) for t in range(threads_n)]
    for th in workers:
        th.start()
    for th in workers:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors[:3]


@pytest.mark.gpu
def test_facade_stranded_hits(engine, tmp_path):
    """12. GCSA::canonical_minimizers and GCSA::stranded_minimizer_hits_batch from a C++ client
    (tests/cpp/stranded_hits_client.cpp) print what the Python forms return."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    which = len(CASES) - 1
    reads = batch_of(which)[0]
    assert all(b"\n" not in r for r in reads)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    save_host_view(indexed(which)[0], str(tmp_path / "index.g2hv"))
    (tmp_path / "reads.txt").write_bytes(b"".join(r + b"\n" for r in reads))
    exe = compile_client(str(tmp_path / "stranded_hits_client"), os.path.join(ROOT, "tests", "cpp", "stranded_hits_client.cpp"))
    data, off = concat_patterns(reads)
    for k, w, seed, strands, hit_max, sample in ((5, 3, 0, BOTH, 0, 0), (3, 2, OTHER_SEED, REVERSE, 3, 1), (7, 11, 1, FORWARD, 2, 0)):
        out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "reads.txt"), str(k), str(w), str(seed), str(strands), str(hit_max),
                              str(sample)], capture_output=True, text=True, env=_run_env(), timeout=300)
        assert out.returncode == 0, out.stderr
        moff, mins = gpu.canonical_minimizers_batch(data, off, k, w, seed)
        soff, seeds, hoff, hits = gpu.stranded_minimizer_hits_batch(data, off, k, w, seed, strands, hit_max, bool(sample))
        want = [f"read {q} {int(moff[q + 1] - moff[q])}" for q in range(len(reads))]
        want += [f"group {g} {int(soff[g + 1] - soff[g])}" for g in range(2 * len(reads))]
        want += [f"minimizer {i} " + " ".join(str(int(x)) for x in mins[i]) for i in range(mins.shape[0])]
        want += [f"seed {i} " + " ".join(str(int(x)) for x in seeds[i]) for i in range(seeds.shape[0])]
        want += [" ".join(["hits", str(i), str(int(hoff[i + 1] - hoff[i]))] + [str(int(v)) for v in hits[int(hoff[i]):int(hoff[i + 1])]])
                 for i in range(seeds.shape[0])]
        assert out.stdout.strip().split("\n") == want, (k, w, seed, strands, hit_max, sample)
        assert 2 * mins.shape[0] >= seeds.shape[0] > 0 and hits.shape[0] > 0          # two strands per minimizer
    gpu.close()
