"""MEM hits (gcsa2_mem_hits_device / gcsa2_mem_hits_batch, kernels_mem.hpp): the break records of a batch with count() and
their locate() values -- all of them, or none / locate(range, hit_max) above the cap -- against the CPU oracle's matching
statistics, count() and locate(), and against the composition of the library's own public calls."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from workload import graphs
from workload.brute_builder import build
from workload.rng import SplitMix64
from gcsa2_amd.hostview import concat_patterns
from test_oracle import CASES, random_patterns
from test_gpu_parity import breaks_from_dense
from test_locate_max_batch import reference_spins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
EDGE = [b"", b"N", b"", b"ACGTNACGT", b"$", b"#A", b"", b"NNNN", b"A", b"TTTTTTTTTTTTTTTTTTTTTTTT", b"XYZ", b"AAAAAAAAAAAAAAAAAAAAAAAAAAAAAA"]
SENTINEL = 0x5A5A5A5A5A5A5A5A


class Spins(Exception):
    """The reference never returns for some sampled MEM (count() overstates its distinct values)."""


@pytest.fixture(scope="module")
def engine():
    from gcsa2_amd import binding
    assert binding.device_count() >= 1, "no MI355X visible"
    return binding


def substituted(pats, seed, period=9):
    """Each pattern with a substitution about every `period` characters."""
    rng = SplitMix64(seed)
    out = []
    for p in pats:
        b = bytearray(p)
        for i in range(len(b)):
            if rng.below(period) == 0:
                b[i] = b"ACGT"[(b"ACGT".find(bytes([b[i]])) + 1 + rng.below(3)) % 4] if b[i:i + 1] in (b"A", b"C", b"G", b"T") else b"A"[0]
        out.append(bytes(b))
    return out


class Oracle:
    """The expected CSRs from the oracle: match_stats_batch -> breaks_from_dense -> filter -> count -> locate."""
    def __init__(self, cpu, pats):
        self.cpu = cpu
        data, off = concat_patterns(pats)
        cm, _cr, _cf = cpu.match_stats_batch(data, off, threads=2)
        self.boff, self.brk = breaks_from_dense(cpu, pats, cm, off)
        self.counts, self.full, self.maxed = {}, {}, {}

    def count(self, r):
        if r not in self.counts:
            self.counts[r] = int(self.cpu.count(r))
        return self.counts[r]

    def hits(self, r, hit_max, sample):
        c = self.count(r)
        if c == 0:
            return []
        if hit_max == 0 or c <= hit_max:
            if r not in self.full:
                self.full[r] = [int(v) for v in self.cpu.locate(r)]
            return self.full[r]
        if not sample:
            return []
        if (r, hit_max) not in self.maxed:
            if reference_spins(self.cpu, r, hit_max):
                raise Spins(r)
            self.maxed[(r, hit_max)] = [int(v) for v in self.cpu.locate(r, max_positions=hit_max)]
        return self.maxed[(r, hit_max)]

    def expected(self, min_length, hit_max, sample):
        keep = self.brk[:, 1] >= min_length
        moff = [0]
        for q in range(self.boff.shape[0] - 1):
            moff.append(moff[-1] + int(keep[int(self.boff[q]):int(self.boff[q + 1])].sum()))
        rec = self.brk[keep]
        mems = np.zeros((rec.shape[0], 5), dtype=np.uint64)
        hoff, hits = [0], []
        for i, (p, ln, sp, ep) in enumerate(rec.tolist()):
            r = (int(sp), int(ep))
            mems[i] = (p, ln, sp, ep, self.count(r))
            h = self.hits(r, hit_max, sample)
            hits += h
            hoff.append(len(hits))
        return (np.asarray(moff, dtype=np.uint64), mems, np.asarray(hoff, dtype=np.uint64), np.asarray(hits, dtype=np.uint64))


def device_call(gpu, pats, min_length, hit_max, over, mem_capacity=None, hit_capacity=None, guard=64, sized=True):
    """gcsa2_mem_hits_device on sentinel-filled torch buffers with `guard` entries behind the capacities: (result or
    Gcsa2Error, mem_offsets, mems, hit_offsets, hits) as numpy (whole buffers, guards included)."""
    import torch
    from gcsa2_amd.binding import Gcsa2Error
    data, off = concat_patterns(pats)
    dev = torch.device("cuda", 0)
    nq, total = len(pats), int(off[-1])
    d_pat = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
    d_pat[:total] = torch.from_numpy(data[:total].copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    mcap = 4 * nq + 16 if mem_capacity is None else mem_capacity
    hcap = 64 * nq + 64 if hit_capacity is None else hit_capacity
    s = np.uint64(SENTINEL).view(np.int64).item()
    d_moff = torch.full((nq + 1,), s, dtype=torch.int64, device=dev)
    d_mems = torch.full((mcap + guard, 5), s, dtype=torch.int64, device=dev)
    d_hoff = torch.full((mcap + 1 + guard,), s, dtype=torch.int64, device=dev)
    d_hits = torch.full((hcap + guard,), s, dtype=torch.int64, device=dev)
    try:
        res = gpu.mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total if sized else None, min_length, hit_max, over,
                                  d_moff.data_ptr(), d_mems.data_ptr(), mcap, d_hoff.data_ptr(), d_hits.data_ptr(), hcap)
    except Gcsa2Error as e:
        res = e
    torch.cuda.synchronize()
    return tuple([res] + [t.cpu().numpy().view(np.uint64) for t in (d_moff, d_mems, d_hoff, d_hits)])


def assert_same(got, want, what):
    names = ("mem_offsets", "mems", "hit_offsets", "hits")
    for name, a, b in zip(names, got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name, a.shape, b.shape)


@pytest.mark.parametrize("which", range(len(CASES)), ids=[c[0] for c in CASES])
def test_oracle_parity(engine, which):
    """Every graph of test_oracle.CASES, random and substituted patterns plus the edge cases of test_match_breaks, every
    min_length, hit_max and policy: device form and host form equal the oracle's CSRs exactly."""
    from oracle.oracle import OracleIndex
    from gcsa2_amd.binding import Gcsa2Error
    name, g, K = CASES[which]
    ix = build(g, K, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    cpu = OracleIndex(ix)
    base = random_patterns(g, 3 * K, 0x7E0 + which, 300)
    pats = base + substituted(base[:150], 0x7F0 + which) + EDGE
    oracle = Oracle(cpu, pats)
    spun = 0
    for min_length in (1, 2, K, 2 * K):
        for hit_max in (0, 1, 3, 64, U64):
            for sample in (False, True):
                what = (name, min_length, hit_max, sample)
                try:
                    want = oracle.expected(min_length, hit_max, sample)
                except Spins:
                    spun += 1
                    with pytest.raises(Gcsa2Error) as err:
                        gpu.mem_hits_batch(*concat_patterns(pats), min_length, hit_max, sample)
                    assert err.value.code == -1 and "max_positions" in str(err.value), what
                    continue
                m, h = want[1].shape[0], want[3].shape[0]
                res, moff, mems, hoff, hits = device_call(gpu, pats, min_length, hit_max, int(sample), m + 5, h + 7, sized=(hit_max != 3))
                assert res == (m, h), (what, res)
                assert_same((moff, mems[:m], hoff[:m + 1], hits[:h]), want, what + ("device",))
                assert_same(gpu.mem_hits_batch(*concat_patterns(pats), min_length, hit_max, sample), want, what + ("host",))
    assert spun < 10, spun


def cap_index(engine):
    """The repeat-rich snp graph: short exact matches with counts in the thousands."""
    from workload import builder
    g = graphs.repeat_graph(1 << 15, 0x3C1, 0x3C2, snp_period=24, node_len=16)
    ix = builder.build(g, 16, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    return g, ix, gpu


def test_cap_bites(engine):
    """MEMs whose counts are far above hit_max, with a hit_max above 1024 (the sampled path's beyond-LDS fallback): SAMPLE
    equals gcsa2_locate_max value for value, SKIP leaves those MEMs with empty slots and their true counts."""
    from workload import patterns
    g, ix, gpu = cap_index(engine)
    import itertools
    pats = [bytes(k) for n in (1, 2, 3) for k in itertools.product(b"ACGT", repeat=n)]      # counts in the thousands
    pats += [bytes(p) for p in patterns.walk_patterns(g, 1000, 6, 0x3C3)] + [bytes(p) for p in patterns.walk_patterns(g, 500, 12, 0x3C4)]
    flat, off = concat_patterns(pats)
    for hit_max in (1, 8, 64, 1100):
        moff, mems, hoff, hits = gpu.mem_hits_batch(flat, off, 1, hit_max, True)
        smoff, smems, shoff, shits = gpu.mem_hits_batch(flat, off, 1, hit_max, False)
        assert np.array_equal(moff, smoff) and np.array_equal(mems, smems)
        counts = mems[:, 4].astype(np.uint64)
        over = counts > np.uint64(hit_max)
        assert int(over.sum()) >= 4 and int(counts.max()) > 2 * hit_max, (hit_max, int(over.sum()), int(counts.max()))
        assert np.array_equal(gpu.count_batch(mems[:, 2:4].copy()), counts)
        ranges = mems[over][:, 2:4].copy()
        lo, lv = gpu.locate_max_batch(ranges, hit_max)
        got = [hits[int(hoff[i]):int(hoff[i + 1])] for i in np.nonzero(over)[0]]
        assert all(np.array_equal(a, lv[int(lo[k]):int(lo[k + 1])]) for k, a in enumerate(got)), hit_max
        assert all(len(a) == hit_max for a in got)
        for i in np.nonzero(over)[0][:50]:
            assert hits[int(hoff[i]):int(hoff[i + 1])].tolist() == gpu.locate(tuple(int(x) for x in mems[i, 2:4]), max_positions=hit_max).tolist()
        sizes = np.diff(shoff)
        assert (sizes[over] == 0).all() and np.array_equal(sizes[~over], np.diff(hoff)[~over])
        keep = np.repeat(~over, np.diff(hoff).astype(np.int64))
        assert np.array_equal(shits, hits[keep])


def test_buffer_contract(engine):
    """Too small a MEM capacity, hit capacity, or both: BUFFER_TOO_SMALL with both totals the sizes needed, and the
    sentinel-filled buffers untouched, behind the capacities included; then a fitting call touches nothing behind them."""
    from workload import patterns
    g, ix, gpu = cap_index(engine)
    pats = [bytes(p) for p in patterns.walk_patterns(g, 500, 40, 0x3D1)]
    pats = substituted(pats, 0x3D2, period=13)
    for hit_max, sample in ((0, 0), (64, 0), (64, 1), (1100, 1)):
        want = gpu.mem_hits_batch(*concat_patterns(pats), 8, hit_max, bool(sample))
        m, h = want[1].shape[0], want[3].shape[0]
        assert m > 0 and h > 0
        for mcap, hcap in ((m - 1, h), (m, h - 1), (m - 1, h - 1), (0, 0)):
            res, moff, mems, hoff, hits = device_call(gpu, pats, 8, hit_max, sample, mcap, hcap)
            assert res.code == -6 and res.needed == (m, h), (hit_max, sample, mcap, hcap)
            assert (mems == np.uint64(SENTINEL)).all() and (hoff == np.uint64(SENTINEL)).all() and (hits == np.uint64(SENTINEL)).all()
        res, moff, mems, hoff, hits = device_call(gpu, pats, 8, hit_max, sample, m, h)
        assert res == (m, h)
        assert (mems[m:] == np.uint64(SENTINEL)).all() and (hoff[m + 1:] == np.uint64(SENTINEL)).all() and (hits[h:] == np.uint64(SENTINEL)).all()
        assert_same((moff, mems[:m], hoff[:m + 1], hits[:h]), want, (hit_max, sample))
        # the host form with the caller's arrays
        from gcsa2_amd.binding import Gcsa2Error
        nq = len(pats)
        with pytest.raises(Gcsa2Error) as err:
            gpu.mem_hits_batch(*concat_patterns(pats), 8, hit_max, bool(sample),
                               out=(np.zeros(nq + 1, dtype=np.uint64), np.zeros((m, 5), dtype=np.uint64), np.zeros(m + 1, dtype=np.uint64),
                                    np.zeros(h - 1, dtype=np.uint64)))
        assert err.value.code == -6 and err.value.needed == (m, h)


def test_refusals(engine):
    """min_length 0, an unknown policy and null buffers: INVALID_ARGUMENT; an index without the LCP array or the samples:
    MISSING_COMPONENT; an empty batch: all-zero offsets."""
    import torch
    from gcsa2_amd.binding import Gcsa2Error
    ix = build(graphs.paper_graph(), 3)
    gpu, _ = engine.open_index(ix, device=0)
    pats = [b"GAT", b"TACA", b""]
    flat, off = concat_patterns(pats)
    for args in ((0, 0, False), (0, 5, True)):
        with pytest.raises(Gcsa2Error) as err:
            gpu.mem_hits_batch(flat, off, *args)
        assert err.value.code == -1 and "min_length" in str(err.value)
    res, *_ = device_call(gpu, pats, 0, 0, 0)
    assert res.code == -1
    res, *_ = device_call(gpu, pats, 1, 0, 7)
    assert res.code == -1 and "policy" in str(res)
    dev = torch.device("cuda", 0)
    d_pat = torch.from_numpy(np.concatenate([flat, np.zeros(16, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    buf = torch.zeros(64, dtype=torch.int64, device=dev)
    for nulls in ((0, buf.data_ptr(), buf.data_ptr(), buf.data_ptr()), (buf.data_ptr(), buf.data_ptr(), 0, buf.data_ptr()),
                  (buf.data_ptr(), 0, buf.data_ptr(), buf.data_ptr()), (buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0)):
        with pytest.raises(Gcsa2Error) as err:
            gpu.mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), len(pats), None, 1, 0, 0, nulls[0], nulls[1], 4, nulls[2], nulls[3], 4)
        assert err.value.code == -1, nulls
    for kw in ({"with_lcp": False}, {"with_samples": False}):
        bare = engine.GCSA(ix, device=0, **kw)
        with pytest.raises(Gcsa2Error) as err:
            bare.mem_hits_batch(flat, off, 1, 0, False)
        assert err.value.code == -5, kw
        with pytest.raises(Gcsa2Error) as err:
            bare.mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), len(pats), None, 1, 0, 0, buf.data_ptr(), buf.data_ptr(), 4,
                                 buf.data_ptr(), buf.data_ptr(), 4)
        assert err.value.code == -5, kw
        bare.close()
    moff, mems, hoff, hits = gpu.mem_hits_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 1, 0, True)
    assert moff.tolist() == [0] and mems.shape == (0, 5) and hoff.tolist() == [0] and hits.shape[0] == 0
    buf.fill_(-1)
    assert gpu.mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), 0, 0, 1, 0, 1, buf.data_ptr(), buf.data_ptr(), 4,
                               buf[32:].data_ptr(), buf.data_ptr(), 4) == (0, 0)
    assert int(buf[0]) == 0 and int(buf[32]) == 0
    # patterns without any match of min_length: offsets all zero
    moff, mems, hoff, hits = gpu.mem_hits_batch(flat, off, 50, 0, False)
    assert moff.tolist() == [0, 0, 0, 0] and mems.shape[0] == 0 and hoff.tolist() == [0] and hits.shape[0] == 0


def composition(gpu, flat, off, min_length, hit_max, sample):
    """The same seeds through the public calls: match_breaks_batch -> count_batch -> locate_batch / locate_max_batch."""
    boff, brk, _, _ = gpu.match_breaks_batch(flat, off, min_length)
    ranges = brk[:, 2:4].copy()
    counts = gpu.count_batch(ranges) if ranges.shape[0] else np.zeros(0, dtype=np.uint64)
    full = (counts > 0) & ((hit_max == 0) | (counts <= np.uint64(hit_max)))
    samp = (counts > np.uint64(hit_max)) & (hit_max > 0) & sample
    sizes = np.zeros(ranges.shape[0], dtype=np.uint64)
    parts = {}
    for mask, fn in ((full, lambda r: gpu.locate_batch(r)), (samp, lambda r: gpu.locate_max_batch(r, hit_max))):
        idx = np.nonzero(mask)[0]
        if idx.shape[0]:
            o, v = fn(ranges[idx])
            for k, i in enumerate(idx):
                parts[int(i)] = v[int(o[k]):int(o[k + 1])]
                sizes[i] = o[k + 1] - o[k]
    hoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    hits = np.concatenate([parts[i] for i in sorted(parts)] + [np.zeros(0, dtype=np.uint64)]).astype(np.uint64)
    mems = np.concatenate([brk, counts.reshape(-1, 1)], axis=1).astype(np.uint64)
    return boff, mems, hoff, hits


def test_composition_larger_index(engine, monkeypatch):
    """An snp graph of 2^16 bases, a few thousand substituted patterns: mem_hits_batch equals the composition of the public
    calls; a host batch in several pieces (1 MB pieces) equals the batch in one."""
    from workload import builder, patterns
    g = graphs.snp_graph(1 << 16, 0x4E1, 0x4E2, snp_period=16, node_len=16)
    ix = builder.build(g, 32, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    pats = substituted([bytes(p) for p in patterns.walk_patterns(g, 4000, 120, 0x4E3)], 0x4E4, period=40)
    flat, off = concat_patterns(pats)
    for min_length, hit_max, sample in ((20, 0, False), (20, 2, False), (20, 2, True), (12, 1, True), (16, 8, True)):
        want = composition(gpu, flat, off, min_length, hit_max, sample)
        got = gpu.mem_hits_batch(flat, off, min_length, hit_max, sample)
        assert_same(got, want, (min_length, hit_max, sample))
    # several pieces: 3 MB of patterns in 1 MB pieces
    monkeypatch.setenv("GCSA2_MS_PIECE_MB", "1")
    pieced, _ = engine.open_index(ix, device=0)
    big = substituted([bytes(p) for p in patterns.walk_patterns(g, 32_000, 100, 0x4E5)], 0x4E6, period=40)
    flat, off = concat_patterns(big)
    assert int(off[-1]) >= 3 << 20
    for min_length, hit_max, sample in ((20, 0, False), (16, 4, True)):
        a = pieced.mem_hits_batch(flat, off, min_length, hit_max, sample)
        b = gpu.mem_hits_batch(flat, off, min_length, hit_max, sample)
        assert_same(a, b, (min_length, hit_max, sample))
        assert a[1].shape[0] > 30_000
    pieced.close()


def test_facade_mem_hits(engine, tmp_path):
    """GCSA::mem_hits_batch from a C++ client (tests/cpp/mem_hits_client.cpp) equals GCSA.mem_hits_batch."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    g = graphs.snp_graph(3000, 0x5F1, 0x5F2, snp_period=12, node_len=16)
    ix = build(g, 8, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    save_host_view(ix, str(tmp_path / "index.g2hv"))
    pats = random_patterns(g, 40, 0x5F3, 200)
    pats = [p for p in pats if b"\n" not in p] + [b"", b"ACGTACGT"]
    (tmp_path / "patterns.txt").write_bytes(b"".join(p + b"\n" for p in pats))
    flat, off = concat_patterns(pats)
    exe = compile_client(str(tmp_path / "mem_hits_client"), os.path.join(ROOT, "tests", "cpp", "mem_hits_client.cpp"))
    for min_length, hit_max, sample in ((4, 0, 0), (4, 3, 0), (4, 3, 1), (8, 64, 1)):
        out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "patterns.txt"), str(min_length), str(hit_max), str(sample)],
                             capture_output=True, text=True, env=_run_env(), timeout=300)
        assert out.returncode == 0, out.stderr
        moff, mems, hoff, hits = gpu.mem_hits_batch(flat, off, min_length, hit_max, bool(sample))
        want = [f"pattern {q} {int(moff[q + 1] - moff[q])}" for q in range(len(pats))]
        want += [f"mem {i} " + " ".join(str(int(x)) for x in mems[i]) for i in range(mems.shape[0])]
        want += [" ".join(["hits", str(i), str(int(hoff[i + 1] - hoff[i]))] + [str(int(v)) for v in hits[int(hoff[i]):int(hoff[i + 1])]])
                 for i in range(mems.shape[0])]
        assert out.stdout.strip().split("\n") == want, (min_length, hit_max, sample)
        assert mems.shape[0] > 0 and hits.shape[0] > 0
