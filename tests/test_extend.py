"""Batched extend (gcsa2_extend_device / gcsa2_extend_batch, kernels_extend.hpp): the loop of find() continued from caller
ranges over substrings of a shared pattern set.  Against a Python restatement of the contract's walk (include/gcsa2_hip.h)
over the CPU oracle's LF, against find() where the two must agree, and against the composition of the library's own calls."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from workload import graphs
from workload.brute_builder import build
from workload.rng import SplitMix64
from gcsa2_amd.hostview import concat_patterns
from test_oracle import CASES, random_patterns
from test_mem_hits import EDGE, SENTINEL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
FLB_BITS = 384                      # positions per rank block of the single-character steps (csrc/layout.hpp); a pair block holds 192
BIG = len(CASES)                    # index of the 6000-base graph in GRAPHS
GRAPHS = [(name, g, K) for name, g, K in CASES] + [("snp6000", graphs.snp_graph(6000, 0xA1, 0xA2, snp_period=10, node_len=16), 16)]


def is_empty(r):
    """Range::empty of the reference (utils.h:93-96): sp + 1 > ep + 1 in 64-bit arithmetic."""
    return ((r[0] + 1) & U64) > ((r[1] + 1) & U64)


def walk(cpu, pattern, begin, end, start):
    """The contract's walk for one valid state: (matched, sp, ep, last_sp, last_ep)."""
    r = last = (int(start[0]), int(start[1]))
    matched, i = 0, end
    while i > begin and not is_empty(r) and cpu.n > 0:
        i -= 1
        r = cpu.LF(r, int(cpu.char2comp[pattern[i]]))
        if not is_empty(r):
            matched, last = matched + 1, r
    return (matched, r[0], r[1], last[0], last[1])


def is_valid(pats, s):
    return s[0] < len(pats) and s[1] <= s[2] <= len(pats[s[0]])


def restate(cpu, pats, states):
    """The expected (n, 5) array of a batch: the walk, or {UNKNOWN, start range twice} for an invalid state."""
    out = np.zeros((len(states), 5), dtype=np.uint64)
    for k, s in enumerate(states):
        s = [int(x) for x in s]
        out[k] = walk(cpu, pats[s[0]], s[1], s[2], (s[3], s[4])) if is_valid(pats, s) else (U64, s[3], s[4], s[3], s[4])
    return out


def case_patterns(which):
    name, g, K = GRAPHS[which]
    pats = random_patterns(g, 3 * K, 0xE70 + which, 200) + EDGE
    if which == BIG:
        pats += [p for p in random_patterns(g, 64, 0xE7F, 400) if len(p) >= 23]
    return pats


@functools.lru_cache(maxsize=None)
def indexed(which):
    from oracle.oracle import OracleIndex
    name, g, K = GRAPHS[which]
    if which == BIG:                   # the compiled builder: the same index as the brute-force one, in seconds at order 16
        from workload import builder
        ix = builder.build(g, K, sample_period=8, branching=4)
    else:
        ix = build(g, K, sample_period=8, branching=4)
    return ix, OracleIndex(ix)


def mutate(p, j):
    b = bytearray(p)
    b[j] = b"ACGT"[(b"ACGT".find(bytes(b[j:j + 1])) + 1) % 4]
    return bytes(b)


@functools.lru_cache(maxsize=None)
def batch(which):
    """(patterns, states as an (n, 5) uint64 array, the restatement's output) for one graph: 300 states on the small graphs,
    2000 on the 6000-base graph, every kind of state the contract names among them."""
    ix, cpu = indexed(which)
    n = cpu.n
    pats = case_patterns(which)
    count = 2000 if which == BIG else 300
    rng = SplitMix64(0xE7E0 + which)
    states = []
    empties = [q for q, p in enumerate(pats) if len(p) == 0]

    def window(q):
        b = rng.below(len(pats[q]) + 1)
        return b, b + rng.below(len(pats[q]) - b + 1)

    if which == BIG:
        # consumed lengths at the refill points of the pattern window and at both parities of a pair step: windows of exactly L
        # characters of a walk through the graph, from the root and from find() of what follows the window
        walks = [q for q, p in enumerate(pats) if q % 2 == 0 and q < 200 or q >= 200 + len(EDGE)]
        for L in (1, 2, 3, 23, 24, 25, 26, 31, 32, 33, 34, 57, 58, 59, 60, 61):
            fit = [q for q in walks if len(pats[q]) >= L and not is_empty(cpu.find(pats[q]))]
            for t in range(24):
                q = fit[rng.below(len(fit))]
                e = L + rng.below(len(pats[q]) - L + 1)
                start = (0, n - 1) if t % 2 == 0 or e == len(pats[q]) else cpu.find(pats[q][e:])
                states.append((q, e - L, e, start[0], start[1]))
        # a step that empties the range after exactly m matched characters, at both parities of what is left of the window:
        # a walk with one base changed at j, continued from find() of the unchanged characters behind j + m
        long_walks = [q for q in walks if len(pats[q]) >= 30 and not is_empty(cpu.find(pats[q]))]
        for m in (0, 1, 2, 3):
            for t in range(60):
                q = long_walks[rng.below(len(long_walks))]
                j = 2 + rng.below(len(pats[q]) - 20)
                pats.append(mutate(pats[q], j))
                start = cpu.find(pats[q][j + 1 + m:])
                states.append((len(pats) - 1, t % 2, j + 1 + m, start[0], start[1]))
        # a character that is not one of the four fast ones inside the consumed span, behind some matched ones
        for t in range(40):
            q = long_walks[rng.below(len(long_walks))]
            j = 1 + rng.below(len(pats[q]) - 8)
            b = bytearray(pats[q])
            b[j] = b"N$#X"[t % 4]
            pats.append(bytes(b))
            states.append((len(pats) - 1, 0, len(b), 0, n - 1))
    kind = 0
    while len(states) < count:
        q = rng.below(len(pats))
        p = pats[q]
        b, e = window(q)
        kind = (kind + 1) % 12
        if kind == 0:
            states.append((q, 0, len(p), 0, n - 1))                               # the root over a whole pattern
        elif kind == 1:
            states.append((q, b, e, 0, n - 1))                                    # the root over a window
        elif kind in (2, 3):
            c = rng.below(len(p) + 1)                                             # find() of a suffix, then the rest
            start = cpu.find(p[c:])
            states.append((q, 0 if kind == 2 else rng.below(c + 1), c, start[0], start[1]))
        elif kind in (4, 5):
            lo = rng.below(n)                                                     # an arbitrary range a <= b < n
            states.append((q, b, e, lo, lo + rng.below(n - lo)))
        elif kind == 6:
            v = rng.below(n)                                                      # a single path node
            states.append((q, b, e, v, v))
        elif kind == 7:
            v = rng.below(n)                                                      # an empty start range
            states.append((q, b, e) + [(v + 1, v), (1, 0), (0, U64), (v + 5, v)][rng.below(4)])
        elif kind == 8:
            states.append((q, b, b, 0, n - 1))                                    # begin == end
        elif kind == 9:
            states.append((empties[rng.below(len(empties))], 0, 0, 0, n - 1))     # an empty pattern
        elif kind == 10:
            for _ in range(3):                                                    # several states of one pattern
                b, e = window(q)
                states.append((q, b, e, 0, n - 1))
        else:
            v = rng.below(n)                                                      # invalid, all three kinds
            states.append([(len(pats) + rng.below(3), 0, 0, v, v), (len(pats) + (1 << 40), 0, 1, 0, n - 1), (q, e + 1, e, v, n - 1),
                           (q, 0, len(p) + 1 + rng.below(3), 0, n - 1), (q, U64, U64, 0, n - 1)][rng.below(5)])
    states = np.asarray(states[:count], dtype=np.uint64)
    return pats, states, restate(cpu, pats, states)


def assert_classes(pats, states, want):
    """What the batch of the 6000-base graph must hold, counted on the restatement's output."""
    n = indexed(BIG)[1].n
    valid = [k for k, s in enumerate(states.tolist()) if is_valid(pats, s)]
    ran, failed_at, parity, lengths, nonfast, split = 0, {}, {0: 0, 1: 0}, {}, 0, 0
    for k in valid:
        s, row = states[k].tolist(), want[k].tolist()
        width, matched = s[2] - s[1], row[0]
        if width == 0 or is_empty((s[3], s[4])):
            continue
        if is_empty((row[1], row[2])):
            failed_at[matched] = failed_at.get(matched, 0) + 1
            parity[(width - matched) % 2] += 1
            used = matched + 1
        else:
            assert matched == width
            ran += 1
            used = width
        lengths[used] = lengths.get(used, 0) + 1
        span = pats[s[0]][s[2] - used:s[2]]
        nonfast += any(c not in b"ACGT" for c in span)
        split += (s[3] // FLB_BITS) != ((s[4] + 1) // FLB_BITS)
    assert ran >= 20, ran
    for m in (0, 1, 2, 3):
        assert failed_at.get(m, 0) >= 20, (m, failed_at)
    assert parity[0] >= 20 and parity[1] >= 20, parity
    for L in (1, 2, 3, 23, 24, 25, 26, 31, 32, 33, 34):
        assert lengths.get(L, 0) >= 20, (L, lengths)
    assert sum(v for L, v in lengths.items() if L >= 57) >= 20, lengths
    assert nonfast >= 20 and split >= 20, (nonfast, split)
    kinds = [sum(1 for s in states.tolist() if s[0] >= len(pats)), sum(1 for s in states.tolist() if s[0] < len(pats) and s[1] > s[2]),
             sum(1 for s in states.tolist() if s[0] < len(pats) and s[1] <= s[2] and s[2] > len(pats[s[0]]))]
    assert min(kinds) >= 5, kinds
    assert len(set(states[:, 0].tolist())) < len(valid), "several states share a pattern"
    assert n > 2 * FLB_BITS


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_library_exports_extend_and_refuses_a_null_index():
    """The built library exports both calls; each refuses a NULL index with INVALID_ARGUMENT, names the index and writes
    nothing."""
    import __graft_entry__ as entry
    entry.build()
    from gcsa2_amd import binding
    for name in ("gcsa2_extend_device", "gcsa2_extend_batch"):
        assert hasattr(ctypes.CDLL(binding.LIB_PATH), name), name
    lib = binding.load_library()
    off = (ctypes.c_uint64 * 2)(0, 4)
    pat = (ctypes.c_uint8 * 8)(*b"ACGTACGT")
    states = (ctypes.c_uint64 * 5)(0, 0, 4, 0, 10)
    out = (ctypes.c_uint64 * 5)(7, 7, 7, 7, 7)
    rc = lib.gcsa2_extend_device(None, ctypes.addressof(pat), ctypes.addressof(off), 1, ctypes.addressof(states), 1, ctypes.addressof(out), None)
    assert rc == -1 and "index" in lib.gcsa2_last_error().decode()
    rc = lib.gcsa2_extend_batch(None, pat, off, 1, ctypes.addressof(states), 1, ctypes.addressof(out))
    assert rc == -1 and "index" in lib.gcsa2_last_error().decode()
    assert list(out) == [7] * 5


@pytest.mark.parametrize("which", range(len(GRAPHS)), ids=[c[0] for c in GRAPHS])
def test_walk_restates_the_contract(which):
    """The restatement itself, on the CPU: from the root it is find() wherever that is non-empty and both are empty otherwise,
    and find(P) == extend(find(P[c:]), P[:c]) exactly for random cuts c."""
    ix, cpu = indexed(which)
    name, g, K = GRAPHS[which]
    pats = random_patterns(g, 3 * K, 0xE70 + which, 200) + EDGE
    rng = SplitMix64(0xE7C + which)
    root = (0, cpu.n - 1)
    for p in pats:
        whole = cpu.find(p)
        m, sp, ep, lsp, lep = walk(cpu, p, 0, len(p), root)
        if is_empty(whole):
            assert is_empty((sp, ep)) or len(p) == 0, (name, p)
            assert m < len(p) or len(p) == 0
        else:
            assert (sp, ep) == whole == (lsp, lep) and m == len(p), (name, p)
        if m > 0:
            assert (lsp, lep) == cpu.find(p[len(p) - m:]), (name, p)           # the longest matched suffix
        for c in ({0, len(p) - 1, rng.below(len(p)), rng.below(len(p))} if len(p) > 0 else ()):      # c = len(p) is the root start above
            back = walk(cpu, p, 0, c, cpu.find(p[c:]))
            assert back[1:3] == whole, (name, p, c)
        b = rng.below(len(p) + 1)
        e = b + rng.below(len(p) - b + 1)
        sub = cpu.find(p[b:e])
        got = walk(cpu, p, b, e, root)
        assert got[1:3] == sub if not is_empty(sub) else is_empty(got[1:3]) or b == e, (name, p, b, e)


def test_the_large_batch_holds_every_class():
    """The batch the GPU tests run on the 6000-base graph meets the conditions they rely on (asserted there again)."""
    assert_classes(*batch(BIG))


# ---- GPU ---------------------------------------------------------------------------------------------------------------

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


def assert_rows(got, want, states, what):
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), states[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(CASES)), ids=[c[0] for c in CASES])
def test_extend_batch_equals_the_walk(engine, which):
    pats, states, want = batch(which)
    gpu, _ = engine.open_index(indexed(which)[0], device=0)
    data, off = concat_patterns(pats)
    assert_rows(gpu.extend_batch(data, off, states), want, states, GRAPHS[which][0])
    assert gpu.extend_batch(data, off, states[:0]).shape == (0, 5)
    gpu.close()


@pytest.mark.gpu
def test_extend_batch_equals_the_walk_on_the_large_graph(big):
    pats, states, want = batch(BIG)
    assert_classes(pats, states, want)
    data, off = concat_patterns(pats)
    assert big.pair_block_bytes() > 0 and big.kmer_table_k() > 0
    assert_rows(big.extend_batch(data, off, states), want, states, "snp6000")


@pytest.mark.gpu
def test_extend_is_the_same_with_and_without_the_tables(big):
    """Without pair blocks, and with the seed table dropped and at its default size: bit-equal results."""
    pats, states, want = batch(BIG)
    data, off = concat_patterns(pats)
    k = big.kmer_table_k()
    try:
        for pair_blocks, kmer_k in ((0, k), (0, 0), (1, 0), (1, k)):
            big.set_tables(pair_blocks=pair_blocks, kmer_k=kmer_k)
            assert (big.pair_block_bytes() > 0) == bool(pair_blocks) and big.kmer_table_k() == kmer_k
            assert_rows(big.extend_batch(data, off, states), want, states, (pair_blocks, kmer_k))
    finally:
        big.set_tables(pair_blocks=1, kmer_k=k)


@pytest.mark.gpu
@pytest.mark.parametrize("n_states", [1, 127, 128, 129])
def test_extend_device(big, n_states):
    """Caller-owned device buffers: the host form's results, nothing written behind d_out[n_states], enqueued on the caller's
    stream behind the work already there."""
    import torch
    pats, states, want = batch(BIG)
    data, off = concat_patterns(pats)
    states = np.ascontiguousarray(states[560:560 + n_states])
    host = big.extend_batch(data, off, states)
    assert_rows(host, want[560:560 + n_states], states, n_states)
    dev = torch.device("cuda", 0)
    total, guard = int(off[-1]), 16
    s = np.uint64(SENTINEL).view(np.int64).item()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_pat = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
        d_pat[:total] = torch.from_numpy(data[:total].copy()).to(dev)
        d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
        d_states = torch.from_numpy(states.view(np.int64).copy()).to(dev)
        d_out = torch.full((n_states + guard, 5), s, dtype=torch.int64, device=dev)
        big.extend_device(d_pat.data_ptr(), d_off.data_ptr(), len(pats), d_states.data_ptr(), n_states, d_out.data_ptr(), stream.cuda_stream)
        big.extend_device(d_pat.data_ptr(), d_off.data_ptr(), len(pats), d_states.data_ptr(), 0, 0, stream.cuda_stream)     # nothing to do
    stream.synchronize()
    got = d_out.cpu().numpy().view(np.uint64)
    assert_rows(got[:n_states], host, states, n_states)
    assert (got[n_states:] == np.uint64(SENTINEL)).all()


@pytest.mark.gpu
def test_fan_out_composes_with_find_and_lf_all(big):
    """find_batch of what follows a position, lf_all_batch there, extend_batch of every non-empty child over what precedes
    it: for each of A, C, G, T the result is find() of the pattern with that base at the position."""
    ix, cpu = indexed(BIG)
    g = GRAPHS[BIG][1]
    rng = SplitMix64(0xE7D)
    pats = [p for p in random_patterns(g, 40, 0xE7B, 800)[::2] if len(p) >= 2][:200]
    assert len(pats) == 200
    at = [rng.below(len(p)) for p in pats]
    data, off = concat_patterns(pats)
    tails, tail_off = concat_patterns([p[j + 1:] for p, j in zip(pats, at)])
    children = big.lf_all_batch(big.find_batch(tails, tail_off), 0)
    comps = [int(cpu.char2comp[c]) for c in b"ACGT"]
    states, owner = [], []
    for q, j in enumerate(at):
        for c in comps:
            r = (int(children[q, c, 0]), int(children[q, c, 1]))
            if not is_empty(r):
                states.append((q, 0, j, r[0], r[1]))
                owner.append((q, c))
    got = big.extend_batch(data, off, np.asarray(states, dtype=np.uint64))
    found = {key: (int(row[1]), int(row[2])) for key, row in zip(owner, got)}
    hits = 0
    for q, j in enumerate(at):
        for base, c in zip(b"ACGT", comps):
            want = cpu.find(pats[q][:j] + bytes([base]) + pats[q][j + 1:])
            if is_empty(want):
                assert (q, c) not in found or is_empty(found[(q, c)]), (q, j, base)
            else:
                assert found.get((q, c)) == want, (q, j, base)
                hits += 1
    assert hits >= 200


@pytest.mark.gpu
def test_facade_extend_batch(engine, tmp_path):
    """GCSA::extend_batch from a C++ client (tests/cpp/extend_client.cpp) prints the walk's values."""
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    which = len(CASES) - 1
    pats, states, want = batch(which)
    keep = [q for q, p in enumerate(pats) if b"\n" not in p]
    assert keep == list(range(len(pats)))
    save_host_view(indexed(which)[0], str(tmp_path / "index.g2hv"))
    (tmp_path / "patterns.txt").write_bytes(b"".join(p + b"\n" for p in pats))
    (tmp_path / "states.txt").write_text("".join(" ".join(str(int(x)) for x in s) + "\n" for s in states))
    exe = compile_client(str(tmp_path / "extend_client"), os.path.join(ROOT, "tests", "cpp", "extend_client.cpp"))
    out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "patterns.txt"), str(tmp_path / "states.txt")],
                         capture_output=True, text=True, env=_run_env(), timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().split("\n") == [f"state {i} " + " ".join(str(int(x)) for x in row) for i, row in enumerate(want)]
