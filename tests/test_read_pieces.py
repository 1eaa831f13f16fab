"""The piece loop that the host forms of the read calls share (for_read_pieces, seed_pieces_batch; host_batch.hpp), where a
host thread carries MORE THAN ONE piece.  The "in pieces" tests of the calls cut 3 MB of reads into 3 pieces for the default 4
threads, so every thread carries one piece there, and what a thread keeps from one piece to the next -- the rebased offsets,
its device buffers, its stream -- is never used twice.  Here the same batch runs under GCSA2_MS_THREADS=1 (one thread carries
all pieces) and GCSA2_MS_THREADS=2 (thread 0 carries pieces 0 and 2).  Library against library: the handle without pieces is
the reference, computed once per call and left unchanged; what that handle returns is held against the oracle by the tests of
each call."""
import contextlib
import os

import numpy as np
import pytest

from gcsa2_amd.hostview import concat_patterns
from test_extend import BIG, indexed
from test_kmer_windows import reads_of
from test_kmer_classes import class_map, NODE_SHIFT

TOO_SMALL = -6
PIECE = 1 << 20                                         # GCSA2_MS_PIECE_MB=1
THREADS = (1, 2)
PER_PIECE = ("distinct", "values")                      # stats that are sums over the pieces: a range is folded within its piece


@contextlib.contextmanager
def environment(**values):
    before = {name: os.environ.get(name) for name in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for name, value in before.items():
            if value is None:
                del os.environ[name]
            else:
                os.environ[name] = value


@pytest.fixture(scope="module")
def engine():
    from gcsa2_amd import binding
    assert binding.device_count() >= 1, "no MI355X visible"
    return binding


@pytest.fixture(scope="module")
def handles(engine):
    """The 6000-base index: without pieces, in 1 MB pieces on the default 4 threads, and in 1 MB pieces on 1 and 2 threads."""
    ix = indexed(BIG)[0]
    opened = {"whole": engine.open_index(ix, device=0)[0]}
    with environment(GCSA2_MS_PIECE_MB="1"):
        opened["default"] = engine.open_index(ix, device=0)[0]
        for threads in THREADS:
            with environment(GCSA2_MS_THREADS=str(threads)):
                opened[threads] = engine.open_index(ix, device=0)[0]
    yield opened
    for gpu in opened.values():
        gpu.close()


@pytest.fixture(scope="module")
def batch():
    """The reads of the "in pieces" tests: those of the 6000-base graph, repeated to just over 3 MB."""
    once = reads_of(BIG)
    reads = once * ((3 << 20) // sum(len(r) for r in once) + 1)
    flat, off = concat_patterns(reads)
    assert 3 * PIECE <= int(off[-1]) < 4 * PIECE        # three or four pieces: fewer threads than pieces
    return flat, off, len(reads)


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i, a.shape, b.shape)
        for field in (a.dtype.names or (None,)):        # the sparse rows and summaries are records
            assert np.array_equal(a if field is None else a[field], b if field is None else b[field]), (what, i, field)


def same_stats(piece, whole, default, what):
    """Everything but the per-piece sums equals the handle without pieces; those equal the same pieces on the default threads."""
    assert {f: v for f, v in piece.items() if f not in PER_PIECE} == {f: v for f, v in whole.items() if f not in PER_PIECE}, what
    assert piece == default, what


@pytest.mark.gpu
def test_kmer_windows(handles, batch):
    flat, off, _ = batch
    want = handles["whole"].kmer_windows_batch(flat, off, 32, 1, counts=True)
    assert 0 < int(want[1][:, 1].sum()) < int(want[0][-1])
    for threads in THREADS:
        same(handles[threads].kmer_windows_batch(flat, off, 32, 1, counts=True), want, threads)


@pytest.mark.gpu
def test_kmer_hits_with_profiles(handles, batch):
    flat, off, n = batch
    want = handles["whole"].kmer_hits_batch(flat, off, 32, 1, 4, True, profiles=True)
    m, h = want[1].shape[0], want[3].shape[0]
    assert m > 0 and h > 0 and len(want) == 5
    for threads in THREADS:
        same(handles[threads].kmer_hits_batch(flat, off, 32, 1, 4, True, profiles=True), want, threads)
    # a seed buffer one short of the total, two threads: refused with both exact totals
    from gcsa2_amd.binding import Gcsa2Error
    with pytest.raises(Gcsa2Error) as err:
        handles[2].kmer_hits_batch(flat, off, 32, 1, 4, True, out=(np.zeros(n + 1, dtype=np.uint64), np.zeros((m - 1, 5), dtype=np.uint64),
                                                                   np.zeros(m, dtype=np.uint64), np.zeros(h, dtype=np.uint64)))
    assert err.value.code == TOO_SMALL and err.value.needed == (m, h)


@pytest.mark.gpu
def test_capped_seeds(handles, batch):
    flat, off, _ = batch
    want = handles["whole"].capped_seeds_batch(flat, off, 8, 0, 3, 2, True)
    assert want[1].shape[0] > 0 and want[3].shape[0] > 0
    for threads in THREADS:
        same(handles[threads].capped_seeds_batch(flat, off, 8, 0, 3, 2, True), want, threads)


@pytest.mark.gpu
def test_capped_seeds_second_run_of_a_piece(handles, batch):
    """min_length = 1 under a max_count that no range exceeds: every matched character is a seed.  A piece of `bytes` bytes and
    `count` reads first runs with room for bytes / 8 + count + 1 seeds; over all pieces that is at most off[-1] / 8 + reads +
    pieces.  More seeds than that in total means that at least one piece was refused once and ran again at the exact size."""
    flat, off, n = batch
    args = (flat, off, 1, 0, 1 << 40, 1, False)
    want = handles["whole"].capped_seeds_batch(*args)
    pieces_upper = int(off[-1]) // PIECE + 1
    assert want[1].shape[0] > int(off[-1]) // 8 + n + pieces_upper, (want[1].shape[0], int(off[-1]), n)
    for threads in THREADS:
        same(handles[threads].capped_seeds_batch(*args), want, threads)


@pytest.mark.gpu
def test_kmer_support(handles, batch):
    flat, off, _ = batch
    whole = handles["whole"]
    n_bins = (int(whole.locate_batch(np.asarray([[0, indexed(BIG)[0].n - 1]], dtype=np.uint64))[1].max()) >> NODE_SHIFT) + 1 - 2
    args = (flat, off, 16, 1, 3, NODE_SHIFT)
    want, want_stats = whole.kmer_support_batch(*args, n_bins=n_bins)
    _, default_stats = handles["default"].kmer_support_batch(*args, n_bins=n_bins)
    assert int(want.sum()) > 0
    for threads in THREADS:
        got, stats = handles[threads].kmer_support_batch(*args, n_bins=n_bins)
        same((got,), (want,), threads)
        same_stats(stats, want_stats, default_stats, threads)


@pytest.mark.gpu
def test_kmer_classes_and_top_classes(handles, batch):
    flat, off, _ = batch
    whole = handles["whole"]
    n_bins = (int(whole.locate_batch(np.asarray([[0, indexed(BIG)[0].n - 1]], dtype=np.uint64))[1].max()) >> NODE_SHIFT) + 1
    dense = (flat, off, 16, class_map("interleaved", n_bins, 5), 5, 1, 3, NODE_SHIFT)
    sparse = (flat, off, 16, class_map("interleaved", n_bins, 100003), 100003, 5, 1, 3, NODE_SHIFT)
    for name, args in (("kmer_classes_batch", dense), ("kmer_top_classes_batch", sparse)):
        rows, records, want_stats = getattr(whole, name)(*args)
        _, _, default_stats = getattr(handles["default"], name)(*args)
        assert want_stats["votes"] > 0
        for threads in THREADS:
            got_rows, got_records, stats = getattr(handles[threads], name)(*args)
            same((got_rows, got_records), (rows, records), (name, threads))
            same_stats(stats, want_stats, default_stats, (name, threads))
