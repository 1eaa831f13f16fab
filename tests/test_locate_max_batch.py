"""Batched locate(range, max_positions) (gcsa2_locate_max_batch / gcsa2_locate_max_into, kernels_locate_max.hpp) against
the CPU oracle's locate(range, max_positions) and the per-range gcsa2_locate_max: value for value, in order, for every range
of every batch."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from workload import graphs
from workload.brute_builder import build
from workload.rng import SplitMix64
from test_oracle import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
MAXES = (0, 1, 2, 3, 5, 64, 311, 312, 313, 1000, U64)
LMAX_MOST, LMAX_SET = 1024, 2048          # the kernel's LDS budget (kernels_locate_max.hpp)


@pytest.fixture(scope="module")
def engine():
    from gcsa2_amd import binding
    assert binding.device_count() >= 1, "no MI355X visible"
    return binding


class Mt64:
    """std::mt19937_64, to count the draws the reference's loop makes."""
    def __init__(self, seed):
        self.x = [seed & U64]
        for i in range(1, 312):
            p = self.x[-1]
            self.x.append((6364136223846793005 * (p ^ (p >> 62)) + i) & U64)
        self.pos = 312

    def __call__(self):
        if self.pos >= 312:
            x = self.x
            for k in range(312):
                y = (x[k] & 0xFFFFFFFF80000000) | (x[(k + 1) % 312] & 0x7FFFFFFF)
                x[k] = x[(k + 156) % 312] ^ (y >> 1) ^ (0xB5026F5AA96619E9 if y & 1 else 0)
            self.pos = 0
        y = self.x[self.pos]
        self.pos += 1
        y ^= (y >> 29) & 0x5555555555555555
        y ^= (y << 17) & 0x71D67FFFEDA60000
        y ^= (y << 37) & 0xFFF7EEE000000000
        y ^= y >> 43
        return y & U64


def reference_outputs(cpu, rng, mx):
    """Generator outputs GCSA::locate(range, max_positions) consumes (draws + shuffle), and the distinct values found."""
    sp, ep = rng
    total = cpu.count(rng)
    if total == 0:
        return 0, 0
    m = min(mx, total)
    if m >= total // 2:
        n = len(cpu.locate(rng))
        return (n if n > m else 0), n
    gen, found, used = Mt64(sp ^ ep), set(), 0
    while len(found) < m:
        pos = sp + gen() % (ep + 1 - sp)
        used += 1
        found.update(int(v) for v in cpu.locate((pos, pos)))
    return used + (len(found) if len(found) > m else 0), len(found)


def oracle_max(cpu, r, mx):
    """oracle_locate_max; with max_positions = 0 the result is always empty (the oracle hands back no buffer then)."""
    return [] if mx == 0 else [int(v) for v in cpu.locate(tuple(r), max_positions=mx)]


def reference_spins(cpu, r, mx):
    """True where the reference never returns: count() (which can overstate a range's distinct values, or wrap below zero
    on the small random graphs) sends it to the draw loop with fewer distinct values than it waits for."""
    total = cpu.count(r)
    if total == 0 or mx == 0:
        return False
    m = min(mx, total)
    return m < total // 2 and len(cpu.locate(r)) < m


def well_defined(cpu, ranges, mx):
    """The ranges the reference answers (wrapped counts included: at max_positions = 2^64 - 1 it locates them all)."""
    return [r for r in ranges if not reference_spins(cpu, r, mx)]


def wrapped(cpu, r):
    """count() wrapped below zero (the counters allow it for some ranges of the small random graphs)."""
    return cpu.count(r) >= (1 << 40)


def is_draw_error(err):
    msg = str(err.value)
    return err.value.code == -1 and ("64 * max_positions + 64" in msg or "draw forever" in msg)


def check_batch(gpu, cpu, ranges, mx, scalar_every=1):
    ranges = well_defined(cpu, ranges, mx)
    arr = np.array(ranges, dtype=np.uint64).reshape(-1, 2)
    offs, vals = gpu.locate_max_batch(arr, mx)
    assert offs.shape[0] == len(ranges) + 1 and int(offs[0]) == 0
    counts = gpu.count_batch(arr) if len(ranges) else np.zeros(0, dtype=np.uint64)
    for q, r in enumerate(ranges):
        got = vals[int(offs[q]):int(offs[q + 1])].tolist()
        assert len(got) <= min(mx, int(counts[q])), (r, mx)     # fewer where count() overstates the values
        assert got == oracle_max(cpu, r, mx), (r, mx)
        if q % scalar_every == 0 and not wrapped(cpu, r):       # (GCSA.locate sizes its buffer by count())
            assert got == gpu.locate(tuple(r), max_positions=mx).tolist(), (r, mx)
    return offs, vals


def small_ranges(ix, seed):
    rng = SplitMix64(seed)
    ranges = [(i, i) for i in range(ix.n)] + [(0, ix.n - 1)]
    for _ in range(120):
        a = rng.below(ix.n)
        ranges.append((a, min(ix.n - 1, a + rng.below(12))))
    ranges += [(1, 0), (5, 2), (ix.n, ix.n), (ix.n - 1, ix.n), (0, ix.n), (U64, U64), (3, U64)]
    return ranges


@pytest.mark.parametrize("table", [1, 0], ids=["table", "walk"])
@pytest.mark.parametrize("period", [8, 1], ids=["period8", "period1"])
@pytest.mark.parametrize("which", range(len(CASES)), ids=[c[0] for c in CASES])
def test_cases_all_ranges(engine, which, period, table):
    from oracle.oracle import OracleIndex
    name, g, K = CASES[which]
    ix = build(g, K, sample_period=period, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    gpu.set_tables(locate_table=table)
    cpu = OracleIndex(ix)
    ranges = small_ranges(ix, 0x3A0 + which)
    for mx in MAXES:
        check_batch(gpu, cpu, ranges, mx, scalar_every=1 if mx in (1, 3, 64) else 5)
    # where the reference would draw forever, the batch stops after 64 m + 64 draws and says so
    from gcsa2_amd.binding import Gcsa2Error
    spinning = [(r, mx) for mx in (3, 5, 64) for r in ranges if reference_spins(cpu, r, mx)]
    for r, mx in spinning[:2] + [x for x in spinning if wrapped(cpu, x[0])][:2]:
        with pytest.raises(Gcsa2Error) as err:
            gpu.locate_max_batch(np.array([r], dtype=np.uint64), mx)
        assert is_draw_error(err), str(err.value)
    # an empty batch
    offs, vals = gpu.locate_max_batch(np.zeros((0, 2), dtype=np.uint64), 5)
    assert offs.tolist() == [0] and vals.shape[0] == 0


def test_nodes_with_several_values(engine):
    """A graph whose path nodes carry several values (bubbles merge positions): the random branch inserts a draw's values
    in order and may overshoot m, so the shuffle runs after draws."""
    from oracle.oracle import OracleIndex
    g = graphs.snp_graph(400, 0x5A1, 0x5A2, snp_period=3, node_len=4)
    ix = build(g, 4, sample_period=4, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    cpu = OracleIndex(ix)
    several = [i for i in range(ix.n) if len(cpu.locate((i, i))) > 1]
    assert several, "no path node with several values"
    ranges = [(0, ix.n - 1)] + [(max(0, i - 20), min(ix.n - 1, i + 20)) for i in several[:40]]
    overshoot = 0
    for table in (1, 0):
        gpu.set_tables(locate_table=table)
        for mx in (1, 2, 3, 5, 7, 64, 100):
            check_batch(gpu, cpu, ranges, mx, scalar_every=3)
            if table == 1:
                overshoot += sum(1 for r in ranges if reference_outputs(cpu, r, mx)[1] > min(mx, cpu.count(r)))
    assert overshoot > 0


def test_twist_boundaries(engine):
    """Draws + shuffle of more than 312 and more than 624 generator outputs: ranges of short patterns on a ~2000-base graph."""
    from oracle.oracle import OracleIndex
    from gcsa2_amd.hostview import concat_patterns
    g = graphs.snp_graph(2000, 0x7B1, 0x7B2, snp_period=8, node_len=8)
    ix = build(g, 8, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    cpu = OracleIndex(ix)
    pats = [b"", b"A", b"C", b"G", b"T", b"AC", b"GT", b"CA", b"TG", b"ACG"]
    data, off = concat_patterns(pats)
    ranges = [tuple(int(x) for x in r) for r in cpu.find_batch(data, off)]
    ranges = [r for r in ranges if r[0] <= r[1]]
    maxes = (150, 200, 313, 400, 500, 700, 1000)
    used = [reference_outputs(cpu, r, mx)[0] for mx in maxes for r in ranges]
    assert max(used) > 624 and any(312 < u <= 624 for u in used), used
    for table in (1, 0):
        gpu.set_tables(locate_table=table)
        for mx in maxes:
            check_batch(gpu, cpu, ranges, mx, scalar_every=1)


def test_past_the_lds_budget(engine):
    """Ranges beyond the kernel's budget (m > 1024, or more than 2048 values in LDS) take the per-range path; mixed with
    ranges that stay on the device in one batch."""
    from oracle.oracle import OracleIndex
    g = graphs.snp_graph(6000, 0x8C1, 0x8C2, snp_period=10, node_len=16)
    ix = build(g, 8, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    cpu = OracleIndex(ix)
    rng = SplitMix64(0x8C3)
    ranges = [(0, ix.n - 1), (0, ix.n // 2), (ix.n // 3, ix.n - 1), (100, 2400), (50, 1100)]
    ranges += [(a, a + rng.below(40)) for a in (rng.below(ix.n - 50) for _ in range(60))]
    counts = gpu.count_batch(np.array(ranges, dtype=np.uint64))
    for mx in (1100, 2000, U64):
        beyond = [r for r, c in zip(ranges, counts) if min(mx, int(c)) > LMAX_MOST or
                  (min(mx, int(c)) >= int(c) // 2 and int(c) > LMAX_SET)]
        assert beyond, mx
        for table in (1, 0):
            gpu.set_tables(locate_table=table)
            check_batch(gpu, cpu, ranges, mx, scalar_every=1)


@pytest.mark.parametrize("shift", ["2^32", "bit63"])
def test_large_values(engine, shift):
    """node_type values across 2^32 and with bit 63 set (the locate table keeps those as indirect entries)."""
    from oracle.oracle import OracleIndex
    from workload import builder
    g = graphs.linear_graph(6000, 0x9D1, node_len=32)
    if shift == "2^32":
        g.value += np.uint64((1 << 32) - int(g.value.max()) // 2)
    else:
        g.value += np.uint64((1 << 63) - int(g.value.max()) // 2)
    ix = builder.build(g, 16, sample_period=16)
    gpu, _ = engine.open_index(ix, device=0)
    cpu = OracleIndex(ix)
    rng = SplitMix64(0x9D2)
    ranges = [(0, ix.n - 1)]
    for width in (1, 2, 5, 64, 200, 700, 3000):
        for _ in range(4):
            a = rng.below(ix.n - width)
            ranges.append((a, a + width - 1))
    for table in (1, 0):
        gpu.set_tables(locate_table=table)
        for mx in (1, 3, 64, 313, 1000, U64):
            offs, vals = check_batch(gpu, cpu, ranges, mx, scalar_every=2)
            if mx == U64:
                top = vals >> np.uint64(63) if shift == "bit63" else vals >> np.uint64(32)
                assert top.min() == 0 and top.max() == 1


def test_locate_max_into(engine):
    """Caller-owned device buffers: BUFFER_TOO_SMALL with the size needed and nothing written behind the capacity; a
    batch of 10^5 ranges bit-exact against the oracle on a seeded sample."""
    import torch
    from oracle.oracle import OracleIndex
    from gcsa2_amd.binding import Gcsa2Error
    from workload import builder
    g = graphs.snp_graph(20000, 0xAE1, 0xAE2, snp_period=12, node_len=16)
    ix = builder.build(g, 16, sample_period=16, branching=8)
    gpu, _ = engine.open_index(ix, device=0)
    cpu = OracleIndex(ix)
    rng = SplitMix64(0xAE3)
    ranges = []
    for _ in range(110_000):
        a = rng.below(ix.n)
        ranges.append((a, min(ix.n - 1, a + rng.below(64))))
    ranges[7] = (9, 8)
    ranges[11] = (ix.n, ix.n + 3)
    mx = 5
    ranges = well_defined(cpu, ranges, mx)[:100_000]     # (arbitrary ranges: a few have a count() the reference would spin on)
    nq = len(ranges)
    assert nq == 100_000
    arr = np.array(ranges, dtype=np.uint64)
    dev = torch.device("cuda:0")
    d_ranges = torch.from_numpy(arr.view(np.int64)).to(dev)
    d_offsets = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    need = int(np.minimum(gpu.count_batch(arr), np.uint64(mx)).sum())
    guard = 4096
    canary = 0x5A5A5A5A5A5A5A5A
    d_values = torch.full((need + guard,), canary, dtype=torch.int64, device=dev)
    with pytest.raises(Gcsa2Error) as err:
        gpu.locate_max_into(d_ranges.data_ptr(), nq, mx, d_offsets.data_ptr(), d_values.data_ptr(), need - 1)
    assert err.value.code == -6 and err.value.needed == need
    torch.cuda.synchronize()
    assert bool((d_values == canary).all())
    total = gpu.locate_max_into(d_ranges.data_ptr(), nq, mx, d_offsets.data_ptr(), d_values.data_ptr(), need)
    torch.cuda.synchronize()
    vals = d_values.cpu().numpy().view(np.uint64)
    offs = d_offsets.cpu().numpy().view(np.uint64)
    assert total <= need and total == int(offs[-1])            # fewer where count() overstates a range's values
    assert bool((vals[need:] == np.uint64(canary)).all())
    ho, hv = gpu.locate_max_batch(arr, mx)
    assert np.array_equal(ho, offs) and np.array_equal(hv, vals[:total])
    sample = SplitMix64(0xAE4)
    for _ in range(2000):
        q = sample.below(nq)
        assert vals[int(offs[q]):int(offs[q + 1])].tolist() == oracle_max(cpu, ranges[q], mx), ranges[q]
    for q in range(0, nq, nq // 200):
        assert vals[int(offs[q]):int(offs[q + 1])].tolist() == gpu.locate(ranges[q], max_positions=mx).tolist(), ranges[q]


def test_facade_locate_batch_max(engine, tmp_path):
    """GCSA::locate_batch(ranges, max_positions, offsets, values) from a C++ client (tests/cpp/locate_max_client.cpp),
    against the oracle and the per-range GCSA::locate(range, max_positions, results)."""
    from oracle.oracle import OracleIndex
    from gcsa2_amd.binding import save_host_view
    from test_facade import compile_client, _run_env
    g = graphs.snp_graph(2000, 0xBF1, 0xBF2, snp_period=12, node_len=16)
    ix = build(g, 8, sample_period=8, branching=4)
    cpu = OracleIndex(ix)
    save_host_view(ix, str(tmp_path / "index.g2hv"))
    rng = SplitMix64(0xBF3)
    ranges = [(0, ix.n - 1), (1, 0), (ix.n, ix.n)] + [(a, min(ix.n - 1, a + rng.below(300))) for a in
                                                      (rng.below(ix.n) for _ in range(100))]
    ranges = well_defined(cpu, well_defined(cpu, ranges, 3), 64)
    (tmp_path / "ranges.txt").write_text("".join(f"{a} {b}\n" for a, b in ranges))
    exe = compile_client(str(tmp_path / "locate_max_client"), os.path.join(ROOT, "tests", "cpp", "locate_max_client.cpp"))
    for mx in (0, 3, 64):
        out = subprocess.run([exe, str(tmp_path / "index.g2hv"), str(tmp_path / "ranges.txt"), str(mx)], capture_output=True,
                             text=True, env=_run_env(), timeout=300)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.strip().split("\n")
        assert len(lines) == 2 * len(ranges)
        for q, r in enumerate(ranges):
            want = oracle_max(cpu, r, mx)
            assert lines[q] == " ".join(["range", str(q), str(len(want))] + [str(v) for v in want]), (r, mx)
            assert lines[len(ranges) + q] == " ".join(["single", str(q), str(len(want))] + [str(v) for v in want]), (r, mx)


def test_wrapped_counts(engine):
    """Ranges sp <= ep < size() whose count() wraps below zero (2^64 - 1, 2^64 - 4, ...).  They get no slot from count():
    the batch answers them like the reference -- at max_positions = 2^64 - 1 it locates them all -- among ordinary ranges,
    with the offsets of the ranges behind them intact; where the reference would draw forever the call fails."""
    from oracle.oracle import OracleIndex
    from gcsa2_amd.binding import Gcsa2Error
    seen = 0
    for which, (name, g, K) in enumerate(CASES):
        ix = build(g, K, sample_period=8, branching=4)
        cpu = OracleIndex(ix)
        odd = [(a, b) for a in range(ix.n) for b in range(a, min(ix.n, a + 6)) if wrapped(cpu, (a, b))]
        if not odd:
            continue
        seen += len(odd)
        gpu, _ = engine.open_index(ix, device=0)
        ones = [(i, i) for i in range(min(ix.n, 6))]
        batch = ones[:1] + odd[:8] + ones + odd[8:16] + ones
        for table in (1, 0):
            gpu.set_tables(locate_table=table)
            offs, vals = check_batch(gpu, cpu, batch, U64)
            assert len(well_defined(cpu, batch, U64)) == len(batch)      # nothing left out at 2^64 - 1
            assert int(offs[-1]) == vals.shape[0] and np.all(np.diff(offs.astype(np.int64)) >= 0)
            for mx in (1, 2, 5):
                check_batch(gpu, cpu, batch, mx)
                bad = [r for r in odd if reference_spins(cpu, r, mx)]
                if bad:
                    with pytest.raises(Gcsa2Error) as err:
                        gpu.locate_max_batch(np.array(ones + bad[:1] + ones, dtype=np.uint64), mx)
                    assert is_draw_error(err), str(err.value)
    assert seen > 0, "no range with a wrapped count() in the test graphs"


def test_batch_size_limit(engine):
    """A batch of 2^24 ranges or more is refused before anything is read (the slots' scan must not wrap)."""
    import torch
    from gcsa2_amd.binding import Gcsa2Error
    ix = build(graphs.paper_graph(), 3, sample_period=8, branching=4)
    gpu, _ = engine.open_index(ix, device=0)
    buf = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    with pytest.raises(Gcsa2Error) as err:
        gpu.locate_max_into(buf.data_ptr(), 1 << 24, 5, buf.data_ptr(), buf.data_ptr(), 16)
    assert err.value.code == -6 and "split the batch" in str(err.value)
