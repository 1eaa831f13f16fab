"""Sub-MEM reseeding (gcsa2_sub_mem_hits_device / gcsa2_sub_mem_hits_batch, kernels_submem.hpp): inside every MEM of at
least reseed_length bases, the shorter matches that occur more often than the MEM, with count() and hits.  Against a Python
restatement of the walk over the CPU oracle's LF / count / parent, against the same walk driven through the library's
public batched calls, and (on the CPU) the walk against the "restart at every end position" form of its contract."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from workload import graphs
from workload.brute_builder import build
from gcsa2_amd.hostview import concat_patterns
from test_oracle import CASES, random_patterns
from test_mem_hits import Oracle, Spins, substituted, assert_same, SENTINEL, EDGE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1


def is_empty(r):
    """range_empty of the reference (utils.h): sp + 1 > ep + 1 in 64-bit arithmetic."""
    return ((r[0] + 1) & U64) > ((r[1] + 1) & U64)


def walk(cpu, pattern, b, length, c, min_length):
    """The contract's walk (include/gcsa2_hip.h) over the oracle's LF, count and parent: [(x, e - x, sp, ep, count)]."""
    n = cpu.n
    E = b + length
    x = e = E
    r, cnt = (0, n - 1), 0
    last_x = None
    out = []
    while e >= b + min_length:
        if x > b:
            r2 = cpu.LF(r, int(cpu.char2comp[pattern[x - 1]]))
            if not is_empty(r2):
                c2 = cpu.count(r2)
                if c2 > c:
                    x -= 1
                    r, cnt = r2, c2
                    continue
        if e - x >= min_length and (last_x is None or x < last_x):
            out.append((x, e - x, r[0], r[1], cnt))
            last_x = x
        if x == b:
            break
        if e == x:
            e -= 1
            x = e
            r = (0, n - 1)
            continue
        p = cpu.parent(r)
        assert p[4] < e - x, "parent() did not shorten the match"
        e = x + p[4]
        r = (p[0], p[1])
    return out


def restart(cpu, pattern, b, length, c, min_length):
    """The contract's meaning: for every end e (descending), the longest match ending at e whose every left extension keeps
    count(find(.)) > c, kept if it has min_length and is not contained in one taken for a larger e: [(s, e - s)]."""
    out = []
    best = None
    for e in range(b + length, b + min_length - 1, -1):
        s = e
        while s > b and cpu.count(cpu.find(pattern[s - 1:e])) > c:
            s -= 1
        if e - s >= min_length and (best is None or s < best):
            out.append((s, e - s))
            best = s
    return out


def expected(cpu, oracle, pats, moff, mems, min_length, reseed_length, hit_max, sample):
    """(sub_offsets, subs, hit_offsets, hits) from the Python walk and the oracle's locate / locate(range, max)."""
    soff, subs, hoff, hits = [0], [], [0], []
    q = 0
    for k in range(mems.shape[0]):
        while int(moff[q + 1]) <= k:
            q += 1
        b, ln, _sp, _ep, c = (int(v) for v in mems[k])
        found = walk(cpu, pats[q], b, ln, c, min_length) if ln >= reseed_length else []
        for rec in found:
            subs.append(rec)
            hits += oracle.hits((rec[2], rec[3]), hit_max, sample)
            hoff.append(len(hits))
        soff.append(len(subs))
    return (np.asarray(soff, dtype=np.uint64), np.asarray(subs, dtype=np.uint64).reshape(-1, 5), np.asarray(hoff, dtype=np.uint64),
            np.asarray(hits, dtype=np.uint64))


# ---- CPU: what the walk means ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", range(len(CASES)), ids=[c[0] for c in CASES])
def test_walk_is_the_restart_form(which):
    """On indexes whose order is at least the pattern length, the walk's sub-MEMs are exactly the restart form of the
    contract, computed from find() / count() of substrings, for the MEM's own count, c = 0 and other values of c."""
    from oracle.oracle import OracleIndex
    name, g, K = CASES[which]
    ix = build(g, K, sample_period=8, branching=4)
    cpu = OracleIndex(ix)
    pats = [p for p in random_patterns(g, K, 0x5B0 + which, 120) if len(p) <= K]
    pats = [p[:K] for p in substituted(pats, 0x5B1 + which, period=5)] + [p[:K] for p in pats]
    seen = 0
    for p in pats:
        for b in range(len(p)):
            for ln in range(1, len(p) - b + 1):
                if K >= 6 and (b * 7 + ln) % 3:
                    continue
                full = cpu.count(cpu.find(p[b:b + ln]))
                for c in {0, full, max(full - 1, 0), 1, 2}:
                    for min_length in (1, 2, 3):
                        got = walk(cpu, p, b, ln, c, min_length)
                        want = restart(cpu, p, b, ln, c, min_length)
                        assert [(s, n) for s, n, *_ in got] == want, (name, p, b, ln, c, min_length)
                        for s, n, sp, ep, cnt in got:
                            assert (sp, ep) == cpu.find(p[s:s + n]) and cnt == cpu.count((sp, ep)) and cnt > c
                        seen += len(got)
    assert seen > 20 * K, seen


def test_library_exports_sub_mem_hits_and_refuses_a_null_index():
    """The built library exports both calls; each refuses a NULL index with INVALID_ARGUMENT before touching a device."""
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    for name in ("gcsa2_sub_mem_hits_device", "gcsa2_sub_mem_hits_batch"):
        assert hasattr(ctypes.CDLL(binding.LIB_PATH), name)
    lib = binding.load_library()
    total_s, total_h = ctypes.c_uint64(7), ctypes.c_uint64(7)
    buf = (ctypes.c_uint64 * 16)()
    rc = lib.gcsa2_sub_mem_hits_device(None, None, None, 0, 0, None, None, 0, 1, 1, 0, 0, ctypes.addressof(buf), None, 0, ctypes.byref(total_s),
                                       ctypes.addressof(buf), None, 0, ctypes.byref(total_h), None)
    assert rc == -1 and "index" in lib.gcsa2_last_error().decode()
    rc = lib.gcsa2_sub_mem_hits_batch(None, None, buf, 0, buf, None, 0, 1, 1, 0, 0, ctypes.addressof(buf), None, 0, ctypes.byref(total_s),
                                      ctypes.addressof(buf), None, 0, ctypes.byref(total_h))
    assert rc == -1 and "index" in lib.gcsa2_last_error().decode()


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine():
    from gcsa2_amd import binding
    assert binding.device_count() >= 1, "no MI355X visible"
    return binding


def device_call(gpu, pats, moff, mems, min_length, reseed_length, hit_max, over, sub_capacity, hit_capacity, guard=64, n_mems=True):
    """gcsa2_sub_mem_hits_device on sentinel-filled torch buffers with `guard` entries behind the capacities: (result or
    Gcsa2Error, sub_offsets, subs, hit_offsets, hits) as numpy (whole buffers, guards included)."""
    import torch
    from gcsa2_amd.binding import Gcsa2Error
    data, off = concat_patterns(pats)
    dev = torch.device("cuda", 0)
    nq, total, nm = len(pats), int(off[-1]), mems.shape[0]
    d_pat = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
    d_pat[:total] = torch.from_numpy(data[:total].copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_moff = torch.from_numpy(np.ascontiguousarray(moff, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_mems = torch.from_numpy(np.ascontiguousarray(mems, dtype=np.uint64).view(np.int64).reshape(-1, 5).copy()).to(dev)
    s = np.uint64(SENTINEL).view(np.int64).item()
    d_soff = torch.full((nm + 1 + guard,), s, dtype=torch.int64, device=dev)
    d_subs = torch.full((sub_capacity + guard, 5), s, dtype=torch.int64, device=dev)
    d_hoff = torch.full((sub_capacity + 1 + guard,), s, dtype=torch.int64, device=dev)
    d_hits = torch.full((hit_capacity + guard,), s, dtype=torch.int64, device=dev)
    try:
        res = gpu.sub_mem_hits_device(d_pat.data_ptr(), d_off.data_ptr(), nq, total, d_moff.data_ptr(), d_mems.data_ptr(),
                                      nm if n_mems else None, min_length, reseed_length, hit_max, over, d_soff.data_ptr(), d_subs.data_ptr(),
                                      sub_capacity, d_hoff.data_ptr(), d_hits.data_ptr(), hit_capacity)
    except Gcsa2Error as e:
        res = e
    torch.cuda.synchronize()
    return tuple([res] + [t.cpu().numpy().view(np.uint64) for t in (d_soff, d_subs, d_hoff, d_hits)])


def check_call(gpu, pats, moff, mems, min_length, reseed_length, hit_max, sample, want, what):
    """Device form (exact capacities plus slack, n_mems given or read back) and host form both equal `want`."""
    s, h = want[1].shape[0], want[3].shape[0]
    nm = mems.shape[0]
    res, soff, subs, hoff, hits = device_call(gpu, pats, moff, mems, min_length, reseed_length, hit_max, int(sample), s + 3, h + 5,
                                              n_mems=(hit_max != 3))
    assert res == (s, h), (what, res)
    assert_same((soff[:nm + 1], subs[:s], hoff[:s + 1], hits[:h]), want, what + ("device",))
    assert (subs[s:] == np.uint64(SENTINEL)).all() and (hits[h:] == np.uint64(SENTINEL)).all() and (soff[nm + 1:] == np.uint64(SENTINEL)).all()
    flat, off = concat_patterns(pats)
    assert_same(gpu.sub_mem_hits_batch(flat, off, moff, mems, min_length, reseed_length, hit_max, sample), want, what + ("host",))


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(CASES)), ids=[c[0] for c in CASES])
def test_oracle_parity(engine, which):
    """Every graph of test_oracle.CASES, substituted random walks up to 3 x the order long (parent() jumps past the order) and
    the edge patterns; the MEMs of mem_hits_batch; two (min_length, reseed_length) pairs, hit_max 0 and 3, both policies:
    device and host forms equal the walk over the oracle with the oracle's hits."""
    from oracle.oracle import OracleIndex
    name, g, K = CASES[which]
    ix = build(g, K, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    cpu = OracleIndex(ix)
    base = random_patterns(g, 3 * K, 0x8A0 + which, 160)
    pats = substituted(base, 0x8B0 + which, period=11) + base[:40] + EDGE
    oracle = Oracle(cpu, pats)
    flat, off = concat_patterns(pats)
    spun, walked = 0, 0
    for mem_min, min_length, reseed_length in ((2, 2, 3), (max(2, K // 2), max(2, K // 2), (3 * max(2, K // 2) + 1) // 2), (1, 1, 2)):
        moff, mems, _, _ = gpu.mem_hits_batch(flat, off, mem_min, 0, False)
        for hit_max in (0, 3):
            for sample in (False, True):
                if hit_max == 0 and sample:
                    continue
                what = (name, min_length, reseed_length, hit_max, sample)
                try:
                    want = expected(cpu, oracle, pats, moff, mems, min_length, reseed_length, hit_max, sample)
                except Spins:
                    spun += 1
                    continue
                walked += want[1].shape[0]
                check_call(gpu, pats, moff, mems, min_length, reseed_length, hit_max, sample, want, what)
    assert spun < 3 and walked > 0, (spun, walked)


def repeat_index(engine):
    from workload import builder
    g = graphs.repeat_graph(1 << 15, 0x3C1, 0x3C2, snp_period=24, node_len=16)
    ix = builder.build(g, 16, sample_period=8, branching=4)
    gpu, lcp = engine.open_index(ix, device=0)
    return g, ix, gpu, lcp


def composition_core(gpu, lcp, flat, off, moff, mems, min_length, reseed_length, n, char2comp):
    """The walk for all reseeded MEMs at once, one round per step, through the public batched calls (lf_batch, count_batch,
    parent_batch): (sub_offsets, subs)."""
    nm = mems.shape[0]
    pid = np.searchsorted(moff, np.arange(nm, dtype=np.uint64), side="right").astype(np.int64) - 1
    start = off[pid].astype(np.int64)
    b = mems[:, 0].astype(np.int64)
    ln = mems[:, 1].astype(np.int64)
    c = mems[:, 4].astype(np.uint64)
    live = ln >= reseed_length
    x = (b + ln).copy()
    e = x.copy()
    r = np.zeros((nm, 2), dtype=np.uint64)
    r[:, 1] = n - 1
    cnt = np.zeros(nm, dtype=np.uint64)
    last_x = np.full(nm, np.iinfo(np.int64).max, dtype=np.int64)
    found = []
    live &= e >= b + min_length
    while live.any():
        idx = np.nonzero(live)[0]
        step = idx[x[idx] > b[idx]]
        ok = np.zeros(nm, dtype=bool)
        if step.shape[0]:
            comps = char2comp[flat[start[step] + x[step] - 1]]
            r2 = gpu.lf_batch(np.ascontiguousarray(r[step]), comps)
            nonempty = (r2[:, 0] + np.uint64(1)) <= (r2[:, 1] + np.uint64(1))
            cand = step[nonempty]
            if cand.shape[0]:
                c2 = gpu.count_batch(np.ascontiguousarray(r2[nonempty]))
                good = c2 > c[cand]
                g_idx = cand[good]
                x[g_idx] -= 1
                r[g_idx] = r2[nonempty][good]
                cnt[g_idx] = c2[good]
                ok[g_idx] = True
        fail = idx[~ok[idx]]
        emit = fail[(e[fail] - x[fail] >= min_length) & (x[fail] < last_x[fail])]
        found.append(np.stack([emit.astype(np.uint64), x[emit].astype(np.uint64), (e[emit] - x[emit]).astype(np.uint64), r[emit, 0], r[emit, 1],
                               cnt[emit]], axis=1))
        last_x[emit] = x[emit]
        done = fail[x[fail] == b[fail]]
        live[done] = False
        reset = fail[(x[fail] > b[fail]) & (e[fail] == x[fail])]
        e[reset] -= 1
        x[reset] = e[reset]
        r[reset, 0] = 0
        r[reset, 1] = n - 1
        up = fail[(x[fail] > b[fail]) & (e[fail] != x[fail])]
        if up.shape[0]:
            nodes = lcp.parent_batch(np.ascontiguousarray(r[up]))
            assert (nodes["node_lcp"].astype(np.int64) < e[up] - x[up]).all()
            e[up] = x[up] + nodes["node_lcp"].astype(np.int64)
            r[up, 0] = nodes["sp"]
            r[up, 1] = nodes["ep"]
        live &= e >= b + min_length
    rows = np.concatenate(found + [np.zeros((0, 6), dtype=np.uint64)])
    rows = rows[np.argsort(rows[:, 0], kind="stable")]          # a MEM's records stay in the order of its rounds
    soff = np.concatenate([[0], np.cumsum(np.bincount(rows[:, 0].astype(np.int64), minlength=nm))]).astype(np.uint64)
    return soff, np.ascontiguousarray(rows[:, 1:])


def with_hits(gpu, subs, hit_max, sample):
    """Hits of sub-MEMs through the public calls, mem_hits' rules: (hit_offsets, hits)."""
    ranges = np.ascontiguousarray(subs[:, 2:4])
    counts = subs[:, 4]
    full = (counts > 0) & ((hit_max == 0) | (counts <= np.uint64(hit_max)))
    samp = (counts > np.uint64(hit_max)) & (hit_max > 0) & sample
    sizes = np.zeros(ranges.shape[0], dtype=np.uint64)
    parts = {}
    for mask, fn in ((full, lambda rr: gpu.locate_batch(rr)), (samp, lambda rr: gpu.locate_max_batch(rr, hit_max))):
        idx = np.nonzero(mask)[0]
        if idx.shape[0]:
            o, v = fn(np.ascontiguousarray(ranges[idx]))
            for k, i in enumerate(idx):
                parts[int(i)] = v[int(o[k]):int(o[k + 1])]
                sizes[i] = o[k + 1] - o[k]
    hoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    hits = np.concatenate([parts[i] for i in sorted(parts)] + [np.zeros(0, dtype=np.uint64)]).astype(np.uint64)
    return hoff, hits


@pytest.mark.gpu
def test_composition_repeat_graph(engine):
    """The repeat-rich graph (sub-MEMs exist): the fused call equals the walk driven through lf_batch / count_batch /
    parent_batch, with hits through locate_batch / locate_max_batch."""
    from workload import patterns
    g, ix, gpu, lcp = repeat_index(engine)
    pats = substituted([bytes(p) for p in patterns.walk_patterns(g, 1500, 100, 0x9C1)], 0x9C2, period=40)
    flat, off = concat_patterns(pats)
    total_subs = 0
    for min_length, hit_max, sample in ((12, 0, False), (12, 8, True), (20, 8, False), (20, 64, True)):
        reseed_length = (3 * min_length + 1) // 2
        moff, mems, _, _ = gpu.mem_hits_batch(flat, off, min_length, 0, False)
        soff, subs = composition_core(gpu, lcp, flat, off, moff, mems, min_length, reseed_length, int(ix.n), np.asarray(ix.char2comp, dtype=np.uint8))
        hoff, hits = with_hits(gpu, subs, hit_max, sample)
        got = gpu.sub_mem_hits_batch(flat, off, moff, mems, min_length, reseed_length, hit_max, sample)
        assert_same(got, (soff, subs, hoff, hits), (min_length, hit_max, sample))
        total_subs += subs.shape[0]
    assert total_subs > 100, total_subs


@pytest.mark.gpu
def test_edge_cases(engine):
    """An empty batch; MEMs none of which reach reseed_length; reseed_length 0; min_length above every MEM; c = 0 and
    hand-made counts; MEMs at position 0 and at the pattern's end; patterns with N and characters outside the alphabet."""
    from oracle.oracle import OracleIndex
    name, g, K = CASES[-1]
    ix = build(g, K, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    cpu = OracleIndex(ix)
    # empty batch
    soff, subs, hoff, hits = gpu.sub_mem_hits_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64),
                                                    np.zeros((0, 5), dtype=np.uint64), 2, 3)
    assert soff.tolist() == [0] and subs.shape == (0, 5) and hoff.tolist() == [0] and hits.shape[0] == 0
    pats = [bytes(p) for p in random_patterns(g, 3 * K, 0x9E1, 60)]
    pats = substituted(pats, 0x9E2, period=7) + [b"ACGTNACGTNAC", b"XYZACGTACGT", b"NNNNACGT", b"ACGTXACGTACGTT"]
    flat, off = concat_patterns(pats)
    oracle = Oracle(cpu, pats)
    moff, mems, _, _ = gpu.mem_hits_batch(flat, off, 2, 0, False)
    assert mems.shape[0] > 20
    # no MEM reaches reseed_length: offsets all zero
    soff, subs, hoff, hits = gpu.sub_mem_hits_batch(flat, off, moff, mems, 2, 10 ** 6)
    assert soff.tolist() == [0] * (mems.shape[0] + 1) and subs.shape[0] == 0 and hoff.tolist() == [0]
    # min_length above every MEM
    soff, subs, hoff, hits = gpu.sub_mem_hits_batch(flat, off, moff, mems, 10 ** 6, 0)
    assert subs.shape[0] == 0 and soff.tolist() == [0] * (mems.shape[0] + 1)
    # hand-made MEMs: whole patterns, position 0, the pattern's end, c = 0 and other counts
    hand, hoffs = [], [0]
    for q, p in enumerate(pats):
        L = len(p)
        rows = []
        if L:
            rows += [(0, L, 0, 0, 0), (0, min(L, 3), 0, 0, 1), (max(L - 4, 0), min(L, 4), 0, 0, 0), (L // 2, L - L // 2, 0, 0, 2)]
            rows += [(1, L - 1, 0, 0, 5)] if L > 1 else []
        hand += rows
        hoffs.append(len(hand))
    hm = np.asarray(hand, dtype=np.uint64).reshape(-1, 5)
    ho = np.asarray(hoffs, dtype=np.uint64)
    for min_length, reseed_length in ((1, 0), (2, 0), (3, 4)):
        for hit_max, sample in ((0, False), (3, True)):
            want = expected(cpu, oracle, pats, ho, hm, min_length, reseed_length, hit_max, sample)
            check_call(gpu, pats, ho, hm, min_length, reseed_length, hit_max, sample, want, ("hand", min_length, reseed_length, hit_max, sample))


@pytest.mark.gpu
def test_buffer_contract_and_refusals(engine):
    """Too small a sub-MEM capacity, hit capacity or both: BUFFER_TOO_SMALL with both totals, sentinel-filled buffers
    untouched.  min_length 0, an unknown policy and a MEM beyond its pattern: INVALID_ARGUMENT, nothing written.  Missing LCP
    or samples: MISSING_COMPONENT.  mem_hits_batch on the same batch still equals the oracle."""
    from gcsa2_amd.binding import Gcsa2Error
    from workload import patterns
    from oracle.oracle import OracleIndex
    g, ix, gpu, _lcp = repeat_index(engine)
    pats = substituted([bytes(p) for p in patterns.walk_patterns(g, 300, 80, 0x9F1)], 0x9F2, period=40)
    flat, off = concat_patterns(pats)
    moff, mems, _, _ = gpu.mem_hits_batch(flat, off, 12, 0, False)
    nm = mems.shape[0]
    for hit_max, sample in ((0, 0), (8, 0), (8, 1)):
        want = gpu.sub_mem_hits_batch(flat, off, moff, mems, 12, 18, hit_max, bool(sample))
        s, h = want[1].shape[0], want[3].shape[0]
        assert s > 0 and h > 0
        for scap, hcap in ((s - 1, h), (s, h - 1), (s - 1, h - 1), (0, 0)):
            res, soff, subs, hoff, hits = device_call(gpu, pats, moff, mems, 12, 18, hit_max, sample, scap, hcap)
            assert res.code == -6 and res.needed == (s, h), (hit_max, sample, scap, hcap)
            for a in (soff, subs, hoff, hits):
                assert (a == np.uint64(SENTINEL)).all()
        res, soff, subs, hoff, hits = device_call(gpu, pats, moff, mems, 12, 18, hit_max, sample, s, h)
        assert res == (s, h)
        assert_same((soff[:nm + 1], subs[:s], hoff[:s + 1], hits[:h]), want, (hit_max, sample))
        assert (soff[nm + 1:] == np.uint64(SENTINEL)).all() and (subs[s:] == np.uint64(SENTINEL)).all()
        assert (hoff[s + 1:] == np.uint64(SENTINEL)).all() and (hits[h:] == np.uint64(SENTINEL)).all()
        with pytest.raises(Gcsa2Error) as err:
            gpu.sub_mem_hits_batch(flat, off, moff, mems, 12, 18, hit_max, bool(sample),
                                   out=(np.zeros(nm + 1, dtype=np.uint64), np.zeros((s, 5), dtype=np.uint64), np.zeros(s + 1, dtype=np.uint64),
                                        np.zeros(h - 1, dtype=np.uint64)))
        assert err.value.code == -6 and err.value.needed == (s, h)
    # refusals write nothing
    bad = mems.copy()
    bad[nm // 2, 1] = 10 ** 6                      # reaches beyond its pattern
    for args, word in (((0, 18, 0, 0), "min_length"), ((12, 18, 0, 7), "policy"), ((12, 18, 0, 0), "beyond")):
        src = bad if word == "beyond" else mems
        res, soff, subs, hoff, hits = device_call(gpu, pats, moff, src, *args, 64, 64)
        assert isinstance(res, Gcsa2Error) and res.code == -1 and word in str(res), (word, res)
        for a in (soff, subs, hoff, hits):
            assert (a == np.uint64(SENTINEL)).all(), word
    with pytest.raises(Gcsa2Error) as err:
        gpu.sub_mem_hits_batch(flat, off, moff, bad, 12, 18)
    assert err.value.code == -1
    for kw in ({"with_lcp": False}, {"with_samples": False}):
        bare = engine.GCSA(ix, device=0, **kw)
        with pytest.raises(Gcsa2Error) as err:
            bare.sub_mem_hits_batch(flat, off, moff, mems, 12, 18)
        assert err.value.code == -5, kw
        bare.close()
    # mem_hits is unchanged by the shared tail: the oracle's CSRs on a small case
    name, g2, K = CASES[-2]
    ix2 = build(g2, K, sample_period=8, branching=4)
    gpu2, _ = engine.open_index(ix2, device=0)
    cpu2 = OracleIndex(ix2)
    pats2 = substituted(random_patterns(g2, 3 * K, 0x9F3, 120), 0x9F4) + EDGE
    oracle = Oracle(cpu2, pats2)
    for min_length, hit_max, sample in ((2, 0, False), (K, 3, True), (1, 1, False)):
        assert_same(gpu2.mem_hits_batch(*concat_patterns(pats2), min_length, hit_max, sample), oracle.expected(min_length, hit_max, sample),
                    ("mem_hits", min_length, hit_max, sample))


@pytest.mark.gpu
def test_facade_sub_mem_hits(engine, tmp_path):
    """GCSA::sub_mem_hits_batch from a C++ client (tests/cpp/sub_mem_hits_client.cpp) equals GCSA.sub_mem_hits_batch."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    g = graphs.repeat_graph(1 << 12, 0x6A1, 0x6A2, snp_period=24, node_len=16)
    ix = build(g, 8, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    save_host_view(ix, str(tmp_path / "index.g2hv"))
    from workload import patterns
    pats = substituted([bytes(p) for p in patterns.walk_patterns(g, 200, 60, 0x6A3)], 0x6A4, period=30) + [b"", b"ACGTNACGT"]
    (tmp_path / "patterns.txt").write_bytes(b"".join(p + b"\n" for p in pats))
    flat, off = concat_patterns(pats)
    exe = compile_client(str(tmp_path / "sub_mem_hits_client"), os.path.join(ROOT, "tests", "cpp", "sub_mem_hits_client.cpp"))
    total = 0
    for min_length, reseed_length, hit_max, sample in ((6, 9, 0, 0), (6, 9, 3, 1), (4, 0, 3, 0)):
        out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "patterns.txt"), str(min_length), str(reseed_length),
                              str(hit_max), str(sample)], capture_output=True, text=True, env=_run_env(), timeout=300)
        assert out.returncode == 0, out.stderr
        moff, mems, _, _ = gpu.mem_hits_batch(flat, off, min_length, 0, False)
        soff, subs, hoff, hits = gpu.sub_mem_hits_batch(flat, off, moff, mems, min_length, reseed_length, hit_max, bool(sample))
        want = [f"mem {k} {int(soff[k + 1] - soff[k])}" for k in range(mems.shape[0])]
        want += [f"sub {i} " + " ".join(str(int(v)) for v in subs[i]) for i in range(subs.shape[0])]
        want += [" ".join(["hits", str(i), str(int(hoff[i + 1] - hoff[i]))] + [str(int(v)) for v in hits[int(hoff[i]):int(hoff[i + 1])]])
                 for i in range(subs.shape[0])]
        assert out.stdout.strip().split("\n") == want, (min_length, reseed_length, hit_max, sample)
        total += subs.shape[0]
    assert total > 0
