"""One walk of the search tree of countKMers (kmer_walk, host_kmers.hpp) under gcsa2_count_kmers, the spectrum calls and
gcsa2_compare_kmers: what no single call's test pins is that the three agree, however the frontier is cut into pieces
(GCSA2_KMER_PIECE, read when a handle is created) and when the frontier runs empty.  The expectations are the CPU oracle's
countKMers alone; the graphs are those that test_kmer_spectrum has indexed."""
import ctypes
import functools
import inspect
import re

import numpy as np
import pytest

from workload import graphs
from workload.brute_builder import build
from test_mem_hits import SENTINEL
from test_kmer_spectrum import GRAPHS, NAMES, BIG, STATS, COUNTS, indexed, depths, expected, levels_of, raw_list, engine, lib  # noqa: F401 (fixtures)

WALKED = ("paper", "snp", "snp6000")
PIECES = ("", "4", "50")                                # "": the default piece, 2^27 states
N_HIST = 64


@functools.lru_cache(maxsize=None)
def oracle_count(which, k, ns):
    return indexed(which)[1].count_kmers(k, ns, force=True)


def opened(engine, monkeypatch, ix, piece):
    """A handle whose walks cut the frontier at `piece` children ("" leaves the default)."""
    if piece:
        monkeypatch.setenv("GCSA2_KMER_PIECE", piece)
    gpu = engine.GCSA(ix)
    if piece:
        monkeypatch.delenv("GCSA2_KMER_PIECE")
    return gpu


@functools.lru_cache(maxsize=None)
def dag():
    """A DAG whose longest path is 24 bases, at order 4, and per alphabet the smallest k without any k-mer."""
    from oracle.oracle import OracleIndex
    ix = build(graphs.linear_graph(24, 0x7, node_len=8), 4, sample_period=8, branching=4)
    cpu = OracleIndex(ix)
    first = {ns: next((k for k in range(1, 64) if cpu.count_kmers(k, ns, force=True) == 0), None) for ns in (False, True)}
    return ix, cpu, first


# ---- CPU ---------------------------------------------------------------------------------------------------------------

def test_library_exports_what_the_binding_declares(lib):
    """3. The built library exports every gcsa2_* symbol the binding declares: every name of binding.EXPORTS and every
    gcsa2_* function that binding.py calls through the loaded library, which EXPORTS lists in turn."""
    from gcsa2_amd import binding
    called = set(re.findall(r"\b_?L\.(gcsa2_\w+)", inspect.getsource(binding)))
    assert len(called) > 100 and called <= set(binding.EXPORTS), sorted(called - set(binding.EXPORTS))
    loaded = ctypes.CDLL(binding.LIB_PATH)
    missing = [name for name in sorted(called | set(binding.EXPORTS)) if not hasattr(loaded, name)]
    assert missing == []
    for name in ("gcsa2_count_kmers", "gcsa2_compare_kmers", "gcsa2_compare_kmers_records", "gcsa2_kmer_spectrum", "gcsa2_list_kmers",
                 "gcsa2_index_kmer_support_device"):
        assert name in binding.EXPORTS and hasattr(lib, name), name


def test_the_cases_are_not_vacuous():
    """What the GPU cases below rely on.  At piece 4 every frontier above the root is walked in several pieces on every
    graph, and at piece 50 the last two levels of the larger graphs are (the last one is cut for the list only: count, compare
    and the histogram take it whole); on snp6000 at k = K a level above the last spans workgroups.  The linear DAG runs out
    of k-mers below k = 64."""
    for name in WALKED:
        which = NAMES.index(name)
        K = GRAPHS[which][2]
        for ns in (False, True):
            tree = levels_of(which, ns)
            for d in range(1, K):
                assert len(tree.at(d)) * tree.limit > 2 * 4, (name, ns, d)
            if name != "paper":
                for d in (K - 2, K - 1):
                    assert len(tree.at(d)) * tree.limit > 2 * 50, (name, ns, d)
        assert expected(which, K - 1, False).m * levels_of(which, False).limit > 2 * 4, (name, "the last level is cut")
    K = GRAPHS[BIG][2]
    above = len(levels_of(BIG, False).at(K - 2))
    assert above > 256 and above * levels_of(BIG, False).limit > 2 * 4
    ix, cpu, first = dag()
    for ns in (False, True):
        assert first[ns] is not None and 4 < first[ns] < 63, ns
        assert cpu.count_kmers(first[ns] - 1, ns, force=True) > 0 and cpu.count_kmers(first[ns] + 1, ns, force=True) == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("piece", PIECES, ids=["default", "piece4", "piece50"])
@pytest.mark.parametrize("name", WALKED)
def test_the_calls_agree_on_one_walk(engine, monkeypatch, name, piece):
    """1. For k in 1, 2, 3, K // 2, K and K + 2 (forced) and both alphabets, count_kmers, the spectrum's kmers, the length of
    the list and compare_kmers of the index with itself are one number, the oracle's countKMers, and the comparison finds
    nothing on one side only -- at the default piece and with the frontier cut at 4 and 50 children.  (At piece 4 a piece is
    one state, a level of it one launch and one wait: snp6000 at k = 16 and 18 walks 0.2 M states four times per alphabet, and
    that case alone takes about a minute; every other case takes seconds or less.)"""
    which = NAMES.index(name)
    ix = indexed(which)[0]
    K = GRAPHS[which][2]
    gpu = opened(engine, monkeypatch, ix, piece)
    seen = 0
    for k in depths(which):
        assert k <= 64
        for ns in (False, True):
            what = (name, piece, k, ns)
            force = k > K
            want = oracle_count(which, k, ns)
            count = gpu.count_kmers(k, include_Ns=ns, force=force)
            stats = gpu.kmer_spectrum(k, n_hist=N_HIST, include_Ns=ns, force=force)[1]
            rc, rows, guard, listed = raw_list(engine, gpu, k, ns, force, COUNTS, 0, 0, count)      # one walk: room for count_kmers records
            compared = gpu.compare_kmers(gpu, k, include_Ns=ns, force=force)
            print(what, count, stats["kmers"], (rc, listed), compared, want)
            assert rc == 0 and (guard == np.uint64(SENTINEL)).all() and (rows[:listed, 4] == np.uint64(k)).all(), (what, rc, listed)
            assert count == stats["kmers"], what
            assert stats["kmers"] == listed, what
            assert listed == compared[0], what
            assert compared[0] == want, what
            assert compared[1:] == (0, 0), what
            seen += want
    assert seen > 0
    gpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("piece", ["", "4"], ids=["default", "piece4"])
def test_the_frontier_that_empties(engine, monkeypatch, piece):
    """2. On a DAG the tree ends: at the smallest k without k-mers and at the one after it -- the walk leaves at a level that
    produced nothing, before it reaches the last -- every call answers with zeros and succeeds; one step earlier there still
    are k-mers."""
    ix, cpu, first = dag()
    gpu = opened(engine, monkeypatch, ix, piece)
    for ns in (False, True):
        k0 = first[ns]
        assert gpu.count_kmers(k0 - 1, include_Ns=ns, force=True) == cpu.count_kmers(k0 - 1, ns, force=True) > 0
        for k in (k0, k0 + 1):
            what = (piece, ns, k)
            assert gpu.count_kmers(k, include_Ns=ns, force=True) == 0, what
            for counts in (True, False):
                hist, stats = gpu.kmer_spectrum(k, n_hist=N_HIST, counts=counts, include_Ns=ns, force=True)
                assert stats == dict.fromkeys(STATS, 0) and hist.shape == (N_HIST,) and not hist.any(), (what, counts, stats)
            assert gpu.list_kmers(k, include_Ns=ns, force=True).shape == (0, 8), what
            assert gpu.compare_kmers(gpu, k, include_Ns=ns, force=True) == (0, 0, 0), what
    gpu.close()
