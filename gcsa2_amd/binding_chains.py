"""ctypes binding of the seed-chain calls (include/gcsa2_hip_chains.h), as binding.py is of include/gcsa2_hip.h: the constants and
structures of that header, the argument types of its five calls and the methods that `binding.GCSA` inherits (ChainCalls).
One module per header: binding.EXPORTS lists the declarations of gcsa2_hip.h name for name and every gcsa2_* call of binding.py,
CHAIN_EXPORTS does the same for this header and this module.  binding.py re-exports every name here."""
import ctypes as C

import numpy as np

from .hostview import u64p, u8p

CHAIN_TOP_LIMIT = 64        # GCSA2_CHAIN_TOP_LIMIT
CHAIN_LOOKBACK_LIMIT = 64   # GCSA2_CHAIN_LOOKBACK_LIMIT
CHAIN_LDS_DEFAULT = 4096    # the default of GCSA2_CHAIN_LDS (the test knob of the chain calls)
CHAIN = np.dtype([(f, np.uint64) for f in ("score", "anchors", "matched", "drift", "read_begin", "read_end", "ref_begin", "ref_end")])     # gcsa2_chain
CHAIN_ANCHOR = np.dtype([("x", np.uint64), ("position", np.uint32), ("length", np.uint32)])     # gcsa2_chain_anchor
CHAIN_SUMMARY = np.dtype([(f, np.uint64) for f in ("anchors", "unplaced", "chains")])     # gcsa2_chain_summary
CHAIN_STATS = ("groups", "invalid_groups", "seeds", "anchors", "unplaced", "chains", "spilled")     # gcsa2_chain_stats
# gcsa2_chain_params in the order of its fields, with the defaults of the binding's keyword arguments
CHAIN_DEFAULTS = dict(band=64, max_gap=5000, lookback=16, match=1, gap=1, min_score=0, top_n=5, member_cap=0)


class ChainParams(C.Structure):
    """gcsa2_chain_params."""
    _fields_ = [(name, C.c_uint64) for name in CHAIN_DEFAULTS]


def chain_params(**params):
    """The gcsa2_chain_params of keyword arguments: CHAIN_DEFAULTS where one is not given; an unknown name is a TypeError."""
    unknown = set(params) - set(CHAIN_DEFAULTS)
    if unknown:
        raise TypeError("unknown chain parameters: " + ", ".join(sorted(unknown)))
    return ChainParams(*(int(params.get(name, default)) for name, default in CHAIN_DEFAULTS.items()))


# the calls of include/gcsa2_hip_chains.h (EXPORTS is the list of include/gcsa2_hip.h, name for name)
CHAIN_EXPORTS = ["gcsa2_seed_chains_device", "gcsa2_kmer_chains_device", "gcsa2_minimizer_chains_device", "gcsa2_kmer_chains_batch",
                 "gcsa2_minimizer_chains_batch"]


def declare_chain_calls(L):
    """The argument types of the five calls on the loaded library (binding.load_library)."""
    vp, u64 = C.c_void_p, C.c_uint64
    L.gcsa2_seed_chains_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, u64, vp, u64, vp, vp, vp, vp, vp, vp]
    L.gcsa2_kmer_chains_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, C.c_int, u64, vp, u64, vp, vp, vp, vp, vp, vp]
    L.gcsa2_minimizer_chains_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, u64, C.c_int, u64, vp, u64, vp, vp, vp, vp, vp, vp]
    L.gcsa2_kmer_chains_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, C.c_int, u64, vp, u64, vp, vp, vp, vp, vp]
    L.gcsa2_minimizer_chains_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, u64, C.c_int, u64, vp, u64, vp, vp, vp, vp, vp]


class ChainCalls:
    """The chain methods of binding.GCSA (self._L: the loaded library, self._h: the handle)."""

    def _chains_done(self, rc, stats, want_stats):
        from . import binding
        if rc != 0:
            raise binding.Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
        return dict(zip(CHAIN_STATS, (int(x) for x in stats))) if want_stats else None

    def seed_chains_device(self, d_group_offsets, n_groups, d_seeds, n_seeds, d_hit_offsets, d_hits, n_hits, shift, d_coord_of_bin, n_bins,
                           d_top, d_members, d_summaries, stream=0, want_stats=True, **params):
        """gcsa2_seed_chains_device on caller-owned device buffers (raw pointers): a seed CSR with its hit offsets and hits as any
        hits call emits them, d_coord_of_bin n_bins u64, d_top n_groups x top_n records of CHAIN, d_members n_groups x top_n x
        member_cap records of CHAIN_ANCHOR and d_summaries n_groups records of CHAIN_SUMMARY, all written (0 / None: not wanted).
        The parameters are keyword arguments with the defaults CHAIN_DEFAULTS.  Complete on return.  Returns the stats as a dict
        of CHAIN_STATS, or None with want_stats=False (a NULL stats pointer)."""
        stats = (C.c_uint64 * len(CHAIN_STATS))() if want_stats else None
        p = chain_params(**params)
        rc = self._L.gcsa2_seed_chains_device(self._h, d_group_offsets or None, int(n_groups), d_seeds or None, int(n_seeds), d_hit_offsets or None,
                                              d_hits or None, int(n_hits), int(shift), d_coord_of_bin or None, int(n_bins), C.addressof(p),
                                              d_top or None, d_members or None, d_summaries or None, stats, stream)
        return self._chains_done(rc, stats, want_stats)

    def kmer_chains_device(self, d_patterns, d_offsets, n_patterns, k, stride, hit_max, sample, shift, d_coord_of_bin, n_bins, d_top, d_members,
                           d_summaries, stream=0, want_stats=True, **params):
        """gcsa2_kmer_chains_device: kmer_hits_device and seed_chains_device in one call, the hits staying on the device."""
        stats = (C.c_uint64 * len(CHAIN_STATS))() if want_stats else None
        p = chain_params(**params)
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        rc = self._L.gcsa2_kmer_chains_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(stride), int(hit_max), over, int(shift),
                                              d_coord_of_bin or None, int(n_bins), C.addressof(p), d_top or None, d_members or None, d_summaries or None,
                                              stats, stream)
        return self._chains_done(rc, stats, want_stats)

    def minimizer_chains_device(self, d_patterns, d_offsets, n_patterns, k, w, hash_seed, hit_max, sample, shift, d_coord_of_bin, n_bins, d_top,
                                d_members, d_summaries, stream=0, want_stats=True, **params):
        """gcsa2_minimizer_chains_device: minimizer_hits_device and seed_chains_device in one call."""
        stats = (C.c_uint64 * len(CHAIN_STATS))() if want_stats else None
        p = chain_params(**params)
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        rc = self._L.gcsa2_minimizer_chains_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(w), int(hash_seed), int(hit_max), over,
                                                   int(shift), d_coord_of_bin or None, int(n_bins), C.addressof(p), d_top or None, d_members or None,
                                                   d_summaries or None, stats, stream)
        return self._chains_done(rc, stats, want_stats)

    def _chains_batch(self, call, patterns, offsets, head, hit_max, sample, shift, coord_of_bin, top, members, summaries, params):
        from . import binding
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        coord_of_bin = np.ascontiguousarray(coord_of_bin, dtype=np.uint64)
        n = max(offsets.shape[0], 1) - 1
        p = chain_params(**params)
        top_n = p.top_n if p.top_n <= CHAIN_TOP_LIMIT else 0
        members = bool(members) and p.member_cap > 0
        rows = n * top_n * p.member_cap if members else 0
        out_top = np.zeros((n, top_n), dtype=CHAIN) if top else None
        out_members = np.zeros((n, top_n, p.member_cap) if rows < (1 << 32) else (0, 0, 0), dtype=CHAIN_ANCHOR) if members else None
        out_sums = np.zeros(n, dtype=CHAIN_SUMMARY) if summaries else None
        stats = (C.c_uint64 * len(CHAIN_STATS))()
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        binding._check(call(self._h, binding._p8(patterns), binding._p64(offsets), n, *head, int(hit_max), over, int(shift),
                    coord_of_bin.ctypes.data if coord_of_bin.shape[0] else None, coord_of_bin.shape[0], C.addressof(p),
                    out_top.ctypes.data if top else None, out_members.ctypes.data if members else None, out_sums.ctypes.data if summaries else None, stats))
        return out_top, out_members, out_sums, dict(zip(CHAIN_STATS, (int(x) for x in stats)))

    def kmer_chains_batch(self, patterns, offsets, k, coord_of_bin, stride=1, hit_max=0, sample=False, shift=10, top=True, members=True, summaries=True,
                          **params):
        """Per read, the top_n colinear chains of the hits of its k-mers (gcsa2_kmer_chains_batch): (top, members, summaries,
        stats).  top: (reads, top_n) of CHAIN, larger score first, all zero behind the last chain; members: (reads, top_n,
        member_cap) of CHAIN_ANCHOR, every chain from its end backwards (None with member_cap == 0); summaries: (reads,) of
        CHAIN_SUMMARY; each is None when not asked for.  stats: a dict of CHAIN_STATS.  coord_of_bin: uint64 coordinates of the
        bins value >> shift, UNKNOWN for a bin without one.  The chain parameters are keyword arguments (CHAIN_DEFAULTS)."""
        return self._chains_batch(self._L.gcsa2_kmer_chains_batch, patterns, offsets, (int(k), int(stride)), hit_max, sample, shift, coord_of_bin, top,
                                  members, summaries, params)

    def minimizer_chains_batch(self, patterns, offsets, k, w, coord_of_bin, hash_seed=0, hit_max=0, sample=False, shift=10, top=True, members=True,
                               summaries=True, **params):
        """The same over the (w, k)-minimizers of every read (gcsa2_minimizer_chains_batch)."""
        return self._chains_batch(self._L.gcsa2_minimizer_chains_batch, patterns, offsets, (int(k), int(w), int(hash_seed)), hit_max, sample, shift,
                                  coord_of_bin, top, members, summaries, params)
