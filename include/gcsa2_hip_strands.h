/* gcsa2_hip_strands.h -- stranded minimizer seeds: the canonical (w, k)-minimizers of every read and their hits on both strands.
 * Part of the C ABI of gcsa2_hip.h (gcsa2_index, gcsa2_mem, gcsa2_kmer_profile, the status codes, the GCSA2_MEM_OVER_* policies
 * and gcsa2_last_error() are declared there).
 *
 * ---- stranded minimizer seeds -----------------------------------------------------------------------------------------------
 * gcsa2_minimizers_device selects and gcsa2_minimizer_hits_device searches every read as it is written.  Half of all reads come
 * from the reverse strand; a forward-strand index finds nothing for them, and a read and its reverse complement do not even
 * select the same k-mers.  Here the selection is strand-invariant, and one call seeds both strands of every read at the same
 * k-mers: the reverse strand of a read, reported in the coordinates of the reverse-complemented read, is a second group of
 * seed records behind the read's own.
 *
 * DEFINITION.  Codes, valid windows, key(j), mix64, spans and "leftmost of equal (hash, position)" are those of
 * gcsa2_minimizers_device.
 *
 * For a valid window j of read P:
 *
 *   - rckey(j) = sum over i of (3 - code(P[j + k - 1 - i])) << 2 (k - 1 - i).  This is the key of the window's reverse complement
 *     under the code complement c -> 3 - c.  In the default alphabet that is A<->T and C<->G.
 *   - hf = mix64(key ^ hash_seed) and hr = mix64(rckey ^ hash_seed).
 *   - chash(j) = min(hf, hr).
 *   - strand(j) = 1 if hr < hf, else 0.  A window that is its own reverse complement has strand 0.
 *   - The canonical minimizers of a read are the windows that the spans select by smallest (chash, position).  They are listed
 *     in ascending position.
 *
 * A window and a second window that is its reverse complement have the same chash.  The leftmost wins.  This is the one place
 * where the selection of rc(P) is not the mirror image of the selection of P.  The contract below never re-selects on the
 * reverse strand, so it does not depend on this.
 *
 * SELECTION CALL.  gcsa2_canonical_minimizers_device / _batch have the signatures of gcsa2_minimizers_device / _batch.  The
 * record type is gcsa2_canonical_minimizer { uint64_t position, hash, key, strand; }.
 *
 *   - hash is chash.
 *   - key is key(position) of the window as written.
 *   - The selection needs nothing of the index but its alphabet.
 *   - Capacities, sizing calls and refusals are those of gcsa2_minimizers_device.
 *
 * HITS CALL.  gcsa2_stranded_minimizer_hits_device, plus _batch for host memory.
 *
 *   - strands is GCSA2_STRAND_FORWARD (1), GCSA2_STRAND_REVERSE (2) or GCSA2_STRAND_BOTH (3).
 *   - The output always has 2 n_patterns groups.  A strand that was not asked for gives empty groups and zero profiles.
 *   - The record type stays gcsa2_mem.
 *
 * For read q = P of length L, with canonical minimizers at positions j_1 < ... < j_m:
 *
 *   - GROUP 2q holds the j_i whose find(P[j_i, j_i + k)) is not empty.  They come in ascending j_i, as
 *     { position = j_i, length = k, sp, ep, count }.
 *   - GROUP 2q + 1 is the same windows seen from R = rc(P).
 *       - The comp sequence of R is R[t] = 1 + (3 - code(P[L - 1 - t])).
 *       - Window j_i is window j'_i = L - k - j_i of R.
 *       - Its seeds come in ascending j', which is descending j.
 *       - Each seed is { position = j'_i, length = k, sp, ep, count } with (sp, ep) the backward search of R[j', j' + k).
 *       - That range is bit for bit what gcsa2_find_device returns for the byte string whose comps these are.
 *       - Only windows of valid characters are ever complemented.
 *   - Hits per seed follow the hit_max, GCSA2_MEM_OVER_SKIP and GCSA2_MEM_OVER_SAMPLE rules of gcsa2_mem_hits_device.
 *   - d_profiles[g] = { windows = m, found, nodes, occurrences } per group.
 *   - The totals, "nothing written on refusal", sizing calls, GCSA2_ERR_MISSING_COMPONENT without samples or counters, and
 *     "complete on return" are those of gcsa2_minimizer_hits_device.
 *   - Limits: fewer than 2^31 reads and fewer than 2^32 stride-1 windows per call, and fewer than 2^32 searched windows (the
 *     minimizers times the strands asked for).  Above a limit the call returns GCSA2_ERR_BUFFER_TOO_SMALL with a message.
 *   - GCSA2_ERR_INVALID_ARGUMENT, before any device is touched and with nothing written, for: k or w out of range; strands of 0
 *     or above 3; an unknown `over`; a NULL index or total; and the reverse strand on an alphabet with fewer than four codes
 *     (sigma < 6), where a complement may be no character of the index.
 *
 * So the output of GCSA2_STRAND_BOTH is a seed CSR over the batch P_0, R_0, P_1, R_1, ... with every read's two strands seeded at
 * the same k-mers.  It goes into gcsa2_seed_clusters_device, gcsa2_seed_chains_device, gcsa2_seed_support_device or
 * gcsa2_sub_mem_hits_device as it is, with n_groups = 2 n.
 *
 * A minimizer window has at most 32 valid bases, so the whole window is one 64-bit key, which the selection kernel
 * (gcsa2_minimizers_device's tile walk with the canonical hash, in the same two passes) already holds in a register; its reverse
 * complement is a bit-reverse, a swap inside the bit pairs, a NOT and a shift of that key.  A small kernel turns the minimizer
 * CSR into the group CSR and the list of (key, position) per searched window, group-major, the reverse group reversed.  The
 * search has one lane per (window, strand) and reads no pattern byte: the seed-table index is the low bits of the key, the
 * next one or two characters are its low bits after a shift.  Behind the search the call is gcsa2_kmer_hits_device's.
 * Device scratch: per read 32 bytes, per minimizer 32 bytes, per searched window 16 bytes, then that of gcsa2_kmer_hits_device
 * with the searched windows as the windows.
 *
 * Out of scope: a stranded form of the stride-window k-mer calls (a window with an N has no complement; w = 1 gives every valid
 * window), fused stranded cluster and chain calls (the composition above keeps everything on the device), syncmers, w > 64 and
 * k > 32. */
#ifndef GCSA2_HIP_STRANDS_H
#define GCSA2_HIP_STRANDS_H

#include "gcsa2_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GCSA2_STRAND_FORWARD 1                   /* the groups 2q: the reads as written */
#define GCSA2_STRAND_REVERSE 2                   /* the groups 2q + 1: their reverse complements */
#define GCSA2_STRAND_BOTH    3
typedef struct gcsa2_canonical_minimizer { uint64_t position, hash, key, strand; } gcsa2_canonical_minimizer;
int gcsa2_canonical_minimizers_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                                      uint64_t k, uint64_t w, uint64_t hash_seed,
                                      uint64_t* d_min_offsets,             /* n_patterns + 1 */
                                      gcsa2_canonical_minimizer* d_minimizers, uint64_t capacity, uint64_t* total, void* stream);
/* The same for a batch in host memory, as gcsa2_minimizers_batch. */
int gcsa2_canonical_minimizers_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                                     uint64_t k, uint64_t w, uint64_t hash_seed, uint64_t* min_offsets,
                                     gcsa2_canonical_minimizer* minimizers, uint64_t capacity, uint64_t* total);
int gcsa2_stranded_minimizer_hits_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                                         uint64_t k, uint64_t w, uint64_t hash_seed, int strands, uint64_t hit_max, int over,
                                         gcsa2_kmer_profile* d_profiles,   /* 2 n_patterns, or NULL */
                                         uint64_t* d_seed_offsets,         /* 2 n_patterns + 1 */
                                         gcsa2_mem* d_seeds, uint64_t seed_capacity, uint64_t* total_seeds,
                                         uint64_t* d_hit_offsets,          /* seed_capacity + 1 */
                                         uint64_t* d_hits, uint64_t hit_capacity, uint64_t* total_hits, void* stream);
/* The host form, as gcsa2_minimizer_hits_batch: pieces of whole reads with their two groups each, group order kept; on
 * GCSA2_ERR_BUFFER_TOO_SMALL a batch in one piece writes nothing, one in pieces leaves the result arrays unspecified. */
int gcsa2_stranded_minimizer_hits_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                                        uint64_t k, uint64_t w, uint64_t hash_seed, int strands, uint64_t hit_max, int over,
                                        gcsa2_kmer_profile* profiles, uint64_t* seed_offsets, gcsa2_mem* seeds, uint64_t seed_capacity,
                                        uint64_t* total_seeds, uint64_t* hit_offsets, uint64_t* hits, uint64_t hit_capacity,
                                        uint64_t* total_hits);

#ifdef __cplusplus
}
#endif
#endif /* GCSA2_HIP_STRANDS_H */
