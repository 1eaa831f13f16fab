"""ctypes binding of the chain-pair calls (include/gcsa2_hip_pairs.h), as binding_chains.py is of include/gcsa2_hip_chains.h: the
constants and structures of that header, the argument types of its three calls and the methods that `binding.GCSA` inherits
(PairCalls).  PAIR_EXPORTS lists the declarations of the header name for name.  binding.py re-exports every name here."""
import ctypes as C

import numpy as np

from .binding_chains import CHAIN, CHAIN_ANCHOR, CHAIN_SUMMARY, CHAIN_STATS, CHAIN_TOP_LIMIT, chain_params
from .hostview import u64p, u8p

PAIR_TOP_LIMIT = 64         # GCSA2_PAIR_TOP_LIMIT
PAIR_FR = 0                 # GCSA2_PAIR_FR: inward, the forward-strand mate upstream
PAIR_RF = 1                 # GCSA2_PAIR_RF: outward
PAIR_FF = 2                 # GCSA2_PAIR_FF: same strand, mate 1 upstream on its own strand
CHAIN_PAIR = np.dtype([(f, np.uint64) for f in ("score", "fragment", "penalty", "chain_score", "left_group", "left_chain", "right_group",
                                                "right_chain")])     # gcsa2_chain_pair
PAIR_SUMMARY = np.dtype([(f, np.uint64) for f in ("candidates", "proper", "kept", "ignored", "mate1_score", "mate1_at", "mate2_score",
                                                  "mate2_at")])     # gcsa2_pair_summary
PAIR_STATS = ("pairs", "candidates", "proper", "kept", "ignored", "paired", "unique", "unique_fragment_sum")     # gcsa2_pair_stats
# gcsa2_pair_params in the order of its fields, with the defaults of the binding's keyword arguments
PAIR_DEFAULTS = dict(orientation=0, min_fragment=0, max_fragment=1000, mean_fragment=400, unit=16, cost=1, min_score=0, top_n=2)


class PairParams(C.Structure):
    """gcsa2_pair_params."""
    _fields_ = [(name, C.c_uint64) for name in PAIR_DEFAULTS]


def pair_params(**params):
    """The gcsa2_pair_params of keyword arguments: PAIR_DEFAULTS where one is not given; an unknown name is a TypeError."""
    unknown = set(params) - set(PAIR_DEFAULTS)
    if unknown:
        raise TypeError("unknown pair parameters: " + ", ".join(sorted(unknown)))
    return PairParams(*(int(params.get(name, default)) for name, default in PAIR_DEFAULTS.items()))


# the calls of include/gcsa2_hip_pairs.h
PAIR_EXPORTS = ["gcsa2_chain_pairs_device", "gcsa2_minimizer_chain_pairs_device", "gcsa2_minimizer_chain_pairs_batch"]


def declare_pair_calls(L):
    """The argument types of the three calls on the loaded library (binding.load_library)."""
    vp, u64 = C.c_void_p, C.c_uint64
    L.gcsa2_chain_pairs_device.argtypes = [vp, vp, u64, u64, vp, vp, vp, vp, vp]
    L.gcsa2_minimizer_chain_pairs_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, u64, C.c_int, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gcsa2_minimizer_chain_pairs_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, u64, C.c_int, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, vp]


class PairCalls:
    """The chain-pair methods of binding.GCSA (self._L: the loaded library, self._h: the handle)."""

    def _pairs_check(self, rc):
        from . import binding
        if rc != 0:
            raise binding.Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))

    def chain_pairs_device(self, d_chains, n_pairs, chain_top_n, d_top, d_summaries, stream=0, want_stats=True, **pair):
        """gcsa2_chain_pairs_device on caller-owned device buffers (raw pointers): d_chains the four chain rows of every pair, 4
        n_pairs x chain_top_n records of CHAIN in the group order of stranded_minimizer_hits_device on interleaved mates; d_top
        n_pairs x top_n records of CHAIN_PAIR and d_summaries n_pairs records of PAIR_SUMMARY, both written (0 / None: not
        wanted).  The pair parameters are keyword arguments with the defaults PAIR_DEFAULTS.  Complete on return.  Returns the
        stats as a dict of PAIR_STATS, or None with want_stats=False (a NULL stats pointer)."""
        stats = (C.c_uint64 * len(PAIR_STATS))() if want_stats else None
        p = pair_params(**pair)
        self._pairs_check(self._L.gcsa2_chain_pairs_device(self._h, d_chains or None, int(n_pairs), int(chain_top_n), C.addressof(p), d_top or None,
                                                           d_summaries or None, stats, stream))
        return dict(zip(PAIR_STATS, (int(x) for x in stats))) if want_stats else None

    def minimizer_chain_pairs_device(self, d_patterns, d_offsets, n_patterns, k, w, hash_seed, hit_max, sample, shift, d_coord_of_bin, n_bins, d_chains,
                                     d_members, d_chain_summaries, d_top, d_summaries, stream=0, want_stats=True, pair=None, **params):
        """gcsa2_minimizer_chain_pairs_device: stranded_minimizer_hits_device (both strands), seed_chains_device over the 2
        n_patterns groups and chain_pairs_device over the n_patterns / 2 pairs of interleaved mates in one call, hits and -- with
        d_chains 0 / None -- chain rows staying on the device.  The pair parameters come as pair=dict(...) (PAIR_DEFAULTS), the
        chain parameters as keyword arguments (CHAIN_DEFAULTS).  Returns (chain stats, pair stats) as dicts, or (None, None) with
        want_stats=False."""
        chain_stats = (C.c_uint64 * len(CHAIN_STATS))() if want_stats else None
        stats = (C.c_uint64 * len(PAIR_STATS))() if want_stats else None
        cp, pp = chain_params(**params), pair_params(**(pair or {}))
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        self._pairs_check(self._L.gcsa2_minimizer_chain_pairs_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(w), int(hash_seed), int(hit_max), over,
                                                                     int(shift), d_coord_of_bin or None, int(n_bins), C.addressof(cp), C.addressof(pp),
                                                                     d_chains or None, d_members or None, d_chain_summaries or None, d_top or None,
                                                                     d_summaries or None, chain_stats, stats, stream))
        if not want_stats:
            return None, None
        return dict(zip(CHAIN_STATS, (int(x) for x in chain_stats))), dict(zip(PAIR_STATS, (int(x) for x in stats)))

    def minimizer_chain_pairs_batch(self, patterns, offsets, k, w, coord_of_bin, hash_seed=0, hit_max=0, sample=False, shift=10, chains=True, members=True,
                                    chain_summaries=True, top=True, summaries=True, pair=None, **params):
        """Per pair of interleaved mates (reads 2p and 2p + 1), the top_n placements of a chain of one mate and a chain of the other
        under the fragment model of `pair` (gcsa2_minimizer_chain_pairs_batch): (chains, members, chain_summaries, top, summaries,
        chain_stats, pair_stats).  chains: (2 reads, chain top_n) of CHAIN, group 2q + s the strand s of read q; members: (2
        reads, chain top_n, member_cap) of CHAIN_ANCHOR (None with member_cap == 0); chain_summaries: (2 reads,) of CHAIN_SUMMARY;
        top: (pairs, top_n) of CHAIN_PAIR, larger score first, all zero behind the last placement; summaries: (pairs,) of
        PAIR_SUMMARY; each is None when not asked for.  The stats are dicts of CHAIN_STATS and PAIR_STATS.  The pair parameters
        come as pair=dict(...) (PAIR_DEFAULTS), the chain parameters as keyword arguments (CHAIN_DEFAULTS)."""
        from . import binding
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        coord_of_bin = np.ascontiguousarray(coord_of_bin, dtype=np.uint64)
        n = max(offsets.shape[0], 1) - 1
        cp, pp = chain_params(**params), pair_params(**(pair or {}))
        chain_top_n = cp.top_n if cp.top_n <= CHAIN_TOP_LIMIT else 0
        top_n = pp.top_n if pp.top_n <= PAIR_TOP_LIMIT else 0
        members = bool(members) and cp.member_cap > 0
        rows = 2 * n * chain_top_n * cp.member_cap if members else 0
        out_chains = np.zeros((2 * n, chain_top_n), dtype=CHAIN) if chains else None
        out_members = np.zeros((2 * n, chain_top_n, cp.member_cap) if rows < (1 << 32) else (0, 0, 0), dtype=CHAIN_ANCHOR) if members else None
        out_chain_sums = np.zeros(2 * n, dtype=CHAIN_SUMMARY) if chain_summaries else None
        out_top = np.zeros((n // 2, top_n), dtype=CHAIN_PAIR) if top else None
        out_sums = np.zeros(n // 2, dtype=PAIR_SUMMARY) if summaries else None
        chain_stats = (C.c_uint64 * len(CHAIN_STATS))()
        stats = (C.c_uint64 * len(PAIR_STATS))()
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        at = lambda a: a.ctypes.data if a is not None else None
        self._pairs_check(self._L.gcsa2_minimizer_chain_pairs_batch(self._h, binding._p8(patterns), binding._p64(offsets), n, int(k), int(w), int(hash_seed),
                                                                    int(hit_max), over, int(shift), coord_of_bin.ctypes.data if coord_of_bin.shape[0] else None,
                                                                    coord_of_bin.shape[0], C.addressof(cp), C.addressof(pp), at(out_chains), at(out_members),
                                                                    at(out_chain_sums), at(out_top), at(out_sums), chain_stats, stats))
        return (out_chains, out_members, out_chain_sums, out_top, out_sums, dict(zip(CHAIN_STATS, (int(x) for x in chain_stats))),
                dict(zip(PAIR_STATS, (int(x) for x in stats))))
