"""ctypes binding of the stranded minimizer calls (include/gcsa2_hip_strands.h), as binding_chains.py is of
include/gcsa2_hip_chains.h: the constants of that header, the argument types of its four calls and the methods that
`binding.GCSA` inherits (StrandCalls).  STRAND_EXPORTS lists the declarations of the header name for name.  binding.py
re-exports every name here."""
import ctypes as C

import numpy as np

from .hostview import u64p, u8p

STRAND_FORWARD = 1          # GCSA2_STRAND_FORWARD: the groups 2q, the reads as written
STRAND_REVERSE = 2          # GCSA2_STRAND_REVERSE: the groups 2q + 1, their reverse complements
STRAND_BOTH = 3             # GCSA2_STRAND_BOTH
CANONICAL_MINIMIZER = ("position", "hash", "key", "strand")     # gcsa2_canonical_minimizer, four u64

# the calls of include/gcsa2_hip_strands.h
STRAND_EXPORTS = ["gcsa2_canonical_minimizers_device", "gcsa2_canonical_minimizers_batch", "gcsa2_stranded_minimizer_hits_device",
                  "gcsa2_stranded_minimizer_hits_batch"]


def declare_strand_calls(L):
    """The argument types of the four calls on the loaded library (binding.load_library)."""
    vp, u64 = C.c_void_p, C.c_uint64
    L.gcsa2_canonical_minimizers_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, vp, vp, u64, u64p, vp]
    L.gcsa2_canonical_minimizers_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, vp, vp, u64, u64p]
    L.gcsa2_stranded_minimizer_hits_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, C.c_int, u64, C.c_int, vp, vp, vp, u64, u64p, vp, vp, u64, u64p, vp]
    L.gcsa2_stranded_minimizer_hits_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, C.c_int, u64, C.c_int, vp, vp, vp, u64, u64p, vp, vp, u64, u64p]


class StrandCalls:
    """The stranded minimizer methods of binding.GCSA (self._L: the loaded library, self._h: the handle)."""

    def _strand_refusal(self, rc, needed):
        from . import binding
        err = binding.Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
        err.needed = needed
        return err

    def canonical_minimizers_batch(self, patterns, offsets, k, w, hash_seed=0, out=None):
        """The canonical (w, k)-minimizers of every read of a batch in host memory (gcsa2_canonical_minimizers_batch):
        (min_offsets (reads + 1), minimizers (total, 4) = {position, hash, key, strand}).  minimizers_batch with the smaller one
        of the hashes of a window and of its reverse complement as the window's hash, so that a read and its reverse complement
        select the same k-mers; key is the 2-bit packed window as written, strand 1 where the reverse complement's hash won.
        `out` = (min_offsets, minimizers) arrays of the caller; too small ones raise BUFFER_TOO_SMALL with `needed`."""
        from . import binding
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.shape[0], 1) - 1
        total = C.c_uint64()

        def call(moff, mins):
            assert moff.dtype == np.uint64 and moff.shape[0] >= n + 1 and mins.dtype == np.uint64 and mins.flags.c_contiguous and mins.shape[1] == 4
            return self._L.gcsa2_canonical_minimizers_batch(self._h, binding._p8(patterns), binding._p64(offsets), n, int(k), int(w), int(hash_seed),
                                                            moff.ctypes.data, mins.ctypes.data, mins.shape[0], C.byref(total))

        if out is not None:
            moff, mins = out
            rc = call(moff, mins)
        else:
            moff = np.zeros(n + 1, dtype=np.uint64)
            mins = np.zeros((0, 4), dtype=np.uint64)
            rc = call(moff, mins)
            if rc == binding.STATUS_BUFFER_TOO_SMALL and total.value > 0:
                mins = np.zeros((total.value, 4), dtype=np.uint64)
                rc = call(moff, mins)
        if rc == binding.STATUS_BUFFER_TOO_SMALL:
            raise self._strand_refusal(rc, total.value)
        binding._check(rc)
        return moff[: n + 1], mins[: total.value]

    def canonical_minimizers_device(self, d_patterns, d_offsets, n_patterns, k, w, hash_seed, d_min_offsets, d_minimizers, capacity, stream=0):
        """gcsa2_canonical_minimizers_device on caller-owned device buffers (raw pointers): d_min_offsets n_patterns + 1 u64,
        d_minimizers `capacity` records of four u64 {position, hash, key, strand} (0 / None with capacity 0: a sizing call).
        Complete on return.  Returns the number of minimizers; raises Gcsa2Error with `.needed` = that number otherwise."""
        needed = C.c_uint64()
        rc = self._L.gcsa2_canonical_minimizers_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(w), int(hash_seed), d_min_offsets,
                                                       d_minimizers or None, int(capacity), C.byref(needed), stream)
        if rc != 0:
            raise self._strand_refusal(rc, needed.value)
        return needed.value

    def stranded_minimizer_hits_batch(self, patterns, offsets, k, w, hash_seed=0, strands=STRAND_BOTH, hit_max=0, sample=False, profiles=False,
                                      out=None):
        """The canonical minimizers of every read that occur, on both strands, as seeds with counts and positions
        (gcsa2_stranded_minimizer_hits_batch).  Two groups per read: group 2q the minimizers of read q found as written, group
        2q + 1 the same windows found as windows of its reverse complement, in that read's coordinates; `strands` (STRAND_FORWARD,
        STRAND_REVERSE, STRAND_BOTH) leaves the groups of the other strand empty.  Returns (seed_offsets (2 reads + 1), seeds
        (total, 5) = {position, length = k, sp, ep, count}, hit_offsets (total + 1), hits[, profiles (2 reads, 4)]).  The buffers
        are sized from a first refusal.  `out` = (seed_offsets, seeds, hit_offsets, hits) arrays of the caller; too small ones
        raise BUFFER_TOO_SMALL with `needed` = (seeds, hits)."""
        from . import binding
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.shape[0], 1) - 1
        over = 1 if sample else 0
        prof = np.zeros((2 * n, 4), dtype=np.uint64) if profiles else None
        total_m, total_h = C.c_uint64(), C.c_uint64()

        def call(soff, seeds, hoff, hits):
            assert soff.dtype == np.uint64 and soff.shape[0] >= 2 * n + 1 and seeds.dtype == np.uint64 and seeds.flags.c_contiguous
            assert seeds.shape[1] == 5 and hoff.dtype == np.uint64 and hoff.shape[0] >= seeds.shape[0] + 1 and hits.dtype == np.uint64
            return self._L.gcsa2_stranded_minimizer_hits_batch(self._h, binding._p8(patterns), binding._p64(offsets), n, int(k), int(w), int(hash_seed),
                                                               int(strands), int(hit_max), over, None if prof is None else prof.ctypes.data,
                                                               soff.ctypes.data, seeds.ctypes.data, seeds.shape[0], C.byref(total_m), hoff.ctypes.data,
                                                               hits.ctypes.data, hits.shape[0], C.byref(total_h))

        if out is not None:
            soff, seeds, hoff, hits = out
            rc = call(soff, seeds, hoff, hits)
        else:
            mcap, hcap = 0, 0
            soff = np.zeros(2 * n + 1, dtype=np.uint64)
            for _ in range(2):
                seeds = np.zeros((mcap, 5), dtype=np.uint64)
                hoff = np.zeros(mcap + 1, dtype=np.uint64)
                hits = np.zeros(hcap, dtype=np.uint64)
                rc = call(soff, seeds, hoff, hits)
                if rc != binding.STATUS_BUFFER_TOO_SMALL:
                    break
                mcap, hcap = max(mcap, total_m.value), max(hcap, total_h.value)
        if rc == binding.STATUS_BUFFER_TOO_SMALL:
            raise self._strand_refusal(rc, (total_m.value, total_h.value))
        binding._check(rc)
        m, h = total_m.value, total_h.value
        res = (soff[: 2 * n + 1], seeds[:m], hoff[: m + 1], hits[:h])
        return res + (prof,) if profiles else res

    def stranded_minimizer_hits_device(self, d_patterns, d_offsets, n_patterns, k, w, hash_seed, strands, hit_max, sample, d_profiles, d_seed_offsets,
                                       d_seeds, seed_capacity, d_hit_offsets, d_hits, hit_capacity, stream=0):
        """gcsa2_stranded_minimizer_hits_device on caller-owned device buffers (raw pointers): d_profiles 2 n_patterns records of
        four u64 (0 / None: not wanted), d_seed_offsets 2 n_patterns + 1 u64, the rest as for minimizer_hits_device.  `sample`: a
        bool, or the `over` policy as an int.  Complete on return.  Returns (seeds, hits); raises Gcsa2Error (BUFFER_TOO_SMALL,
        `.needed` = (seeds, hits)) when a buffer is too small.  The output is a seed CSR over 2 n_patterns groups: it goes into
        seed_clusters_device and seed_chains_device as it is."""
        total_m, total_h = C.c_uint64(), C.c_uint64()
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        rc = self._L.gcsa2_stranded_minimizer_hits_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(w), int(hash_seed), int(strands),
                                                          int(hit_max), over, d_profiles or None, d_seed_offsets, d_seeds or None, int(seed_capacity),
                                                          C.byref(total_m), d_hit_offsets, d_hits or None, int(hit_capacity), C.byref(total_h), stream)
        if rc != 0:
            raise self._strand_refusal(rc, (total_m.value, total_h.value))
        return total_m.value, total_h.value
