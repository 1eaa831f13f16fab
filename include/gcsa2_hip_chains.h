/* gcsa2_hip_chains.h -- seed chains: per read the top colinear chains of its seed hits.  Part of the C ABI of gcsa2_hip.h
 * (gcsa2_index, gcsa2_mem, the status codes, GCSA2_UNKNOWN and gcsa2_last_error() are declared there).
 *
 * ---- seed chains --------------------------------------------------------------------------------------------------------------
 * A diagonal band (gcsa2_seed_clusters_device) says where a read goes; it does not say which of its anchors are colinear, it has
 * no score that pays for gaps, and it does not list the anchors an extender must connect.  A mapper chains its anchors next.
 * Here the hits stay on the device and what leaves is, per read (or group of seed records), the top_n chains of 64 bytes each,
 * optionally the first member_cap anchors of each from its end backwards, and a summary.  The geometry is the caller's, as for
 * the clusters: a map from bins of located values to coordinates.
 *
 * DEFINITION (gcsa2_seed_chains_device).
 *   - Inputs, groups and INVALID groups: exactly those of gcsa2_seed_clusters_device.  A seed CSR, hit offsets and hits as every
 *     hits call emits them; a seed-offset array serves as d_group_offsets (n_groups + 1 entries); of a seed only `position` and
 *     `length` are read; d_hit_offsets has n_seeds + 1 entries, d_hits n_hits.  A group whose group offsets decrease or reach
 *     beyond n_seeds, or whose hit offsets over its seeds decrease or reach beyond n_hits, is NOT READ any further; its row,
 *     its member rows and its summary are zero and it counts in stats.invalid_groups.  A group without a seed is valid.
 *   - ANCHORS of group g: every pair (seed i of the group, hit v = d_hits[h]) with h in [d_hit_offsets[i], d_hit_offsets[i + 1]).
 *     Anchors are a multiset.
 *   - Placement: bin = v >> shift.  The anchor is UNPLACED if bin >= n_bins, if d_coord_of_bin[bin] == GCSA2_UNKNOWN, if
 *     position >= 2^32, length >= 2^32 or position + length >= 2^32, or if x >= 2^62, where
 *     x = d_coord_of_bin[bin] + (v & (2^shift - 1)) in 64-bit wrapping arithmetic.  Every quantity below is then plain,
 *     non-wrapping 64-bit arithmetic.  A placed anchor is (q, l, x) = (position, length, x), with qe = q + l and xe = x + l.
 *   - Order: the placed anchors of a group sorted by (x, q, l) ascending, unsigned.  The PLACE of an anchor is its index in that
 *     order.  Equal triples are indistinguishable, so the order is total for every purpose below.
 *   - Link j -> i (places) is ALLOWED iff j < i and i - j <= lookback; q_j < q_i and x_j < x_i; dq = qe_i - qe_j and
 *     dx = xe_i - xe_j are both >= 1 and <= max_gap; drift(j, i) = |dx - dq| <= band.  gain(j, i) = min(l_i, dq, dx).
 *   - Scores: w_i = match l_i and f(i) = max(w_i, max over allowed j of f(j) + match gain(j, i) - gap drift(j, i)).  A
 *     predecessor is chosen only if its value is strictly greater than w_i; among predecessors of equal value the largest j
 *     wins.  pred(i) is that j, or none.  All f >= 0.
 *   - Chains (greedy, disjoint): visit the anchors as chain ends in the order (larger f first, then smaller place), skipping an
 *     anchor that is already used.  From an unused end e walk e, pred(e), ... while the anchor is unused, marking each walked
 *     anchor used; the walk stops at no predecessor or at a used anchor u.  anchors = the number walked.  matched = the sum of
 *     gain over the chain's links, plus l of its first anchor (the last one walked) if the walk ended at no predecessor, plus
 *     gain(u, first) if it stopped at u.  drift = the sum of drift over the same links, u -> first included.
 *     score = match matched - gap drift as a SIGNED number (equivalently f(e), or f(e) - f(u)).  read_begin, ref_begin = q, x of
 *     the first anchor; read_end, ref_end = qe, xe of e.  The chain is KEPT iff score >= min_score; the marks of a walk that is
 *     not kept stay.
 *   - The top row: order the kept chains by larger score, then larger anchors, then smaller place of the end.
 *     d_top[g top_n + j] for j < min(top_n, kept) is the j-th kept chain; every later entry of the row is all zero (anchors == 0
 *     marks an empty entry).
 *   - Members: written only if member_cap > 0 and d_members != NULL.  The row of chain slot (g, j) is
 *     d_members[(g top_n + j) member_cap ..): that chain's anchors from its END backwards (entry 0 is the end anchor) as
 *     {x, position, length}, min(anchors, member_cap) entries; the rest of the row, and the row of an empty slot, is zero.
 *   - summary(g) = { anchors = the placed anchors, unplaced = the others, chains = the kept chains of the group }.
 *   - stats: groups = n_groups; seeds, anchors, unplaced, chains = the sums over the valid groups; spilled = the number of
 *     groups that took the large path (below), the only field that may depend on GCSA2_CHAIN_LDS.
 *   - Rows, member rows and summaries are WRITTEN in full for every group, and nothing behind them.  d_top, d_members,
 *     d_summaries and stats may each be NULL; all four NULL is valid and does the work.
 *
 * GCSA2_ERR_INVALID_ARGUMENT, before any device is touched, with nothing written and stats untouched: what
 * gcsa2_seed_clusters_device refuses (a NULL index, top_n == 0 or top_n > GCSA2_CHAIN_TOP_LIMIT, shift >= 64, n_bins == 0 or a
 * NULL map, NULL d_group_offsets with n_groups > 0, NULL d_seeds or d_hit_offsets with n_seeds > 0, NULL d_hits with n_hits > 0,
 * n_groups, n_seeds or n_hits >= 2^32), NULL params, lookback outside 1 .. GCSA2_CHAIN_LOOKBACK_LIMIT, match outside
 * 1 .. 65536, gap > 65536, max_gap outside 1 .. 2^32 - 1, min_score >= 2^62, and member_cap > 0 with
 * n_groups top_n member_cap >= 2^32.  band is any value.  n_groups == 0 is GCSA2_OK with zero stats.  The call needs no
 * component of the image.  Enqueued on `stream`, complete on return.
 *
 * The fused forms gcsa2_kmer_chains_device and gcsa2_minimizer_chains_device: the hits never leave the device.  LAW: their rows,
 * member rows, summaries and stats equal gcsa2_kmer_hits_device (gcsa2_minimizer_hits_device) with the same arguments into large
 * enough buffers followed by gcsa2_seed_chains_device with the seed offsets as the groups, word for word.  Refusals, limits and
 * missing components (samples and counters) are those of the hits call plus those above.  They run the hits call's own core
 * into scratch of the call and then the chain core: there is no second search kernel.
 *
 * One workgroup owns a group of up to 4096 anchors, 32 bytes of LDS per anchor: a single wavefront for a group of up to 256
 * anchors, 256 lanes above.  It packs the placed anchors into LDS, sorts them by (x, q, l) (bitonic), runs the dynamic program
 * -- sequential in i, lane k of one wavefront evaluating predecessor i - 1 - k, which is why lookback <= 64 --, sorts the places
 * by (f, place), walks the chains and keeps the top row in the registers of one wavefront.  Groups above the capacity take the
 * LARGE path -- device-wide radix sorts, then the same dynamic program, walk and ranking code over global memory --, exact for
 * any number of anchors.  GCSA2_CHAIN_LDS (a test knob, read per call; a power of two, 64 .. 4096, anything else is ignored)
 * sets the capacity; no result but stats.spilled depends on it.  Global atomics serve the stats only. */
#ifndef GCSA2_HIP_CHAINS_H
#define GCSA2_HIP_CHAINS_H

#include "gcsa2_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GCSA2_CHAIN_TOP_LIMIT 64                 /* top_n may be 1 .. GCSA2_CHAIN_TOP_LIMIT */
#define GCSA2_CHAIN_LOOKBACK_LIMIT 64            /* lookback may be 1 .. GCSA2_CHAIN_LOOKBACK_LIMIT */
typedef struct gcsa2_chain_params {
  uint64_t band, max_gap, lookback, match, gap, min_score, top_n, member_cap;
} gcsa2_chain_params;
typedef struct gcsa2_chain {
  uint64_t score, anchors, matched, drift, read_begin, read_end, ref_begin, ref_end;
} gcsa2_chain;
typedef struct gcsa2_chain_anchor { uint64_t x; uint32_t position, length; } gcsa2_chain_anchor;
typedef struct gcsa2_chain_summary { uint64_t anchors, unplaced, chains; } gcsa2_chain_summary;
typedef struct gcsa2_chain_stats { uint64_t groups, invalid_groups, seeds, anchors, unplaced, chains, spilled; } gcsa2_chain_stats;
int gcsa2_seed_chains_device(const gcsa2_index* index, const uint64_t* d_group_offsets, uint64_t n_groups /* n_groups + 1 offsets */,
                             const gcsa2_mem* d_seeds, uint64_t n_seeds,
                             const uint64_t* d_hit_offsets /* n_seeds + 1 */, const uint64_t* d_hits, uint64_t n_hits,
                             uint64_t shift, const uint64_t* d_coord_of_bin, uint64_t n_bins, const gcsa2_chain_params* params,
                             gcsa2_chain* d_top /* n_groups x top_n, row-major, or NULL */,
                             gcsa2_chain_anchor* d_members /* n_groups x top_n x member_cap, or NULL */,
                             gcsa2_chain_summary* d_summaries /* n_groups, or NULL */,
                             gcsa2_chain_stats* stats /* host, or NULL */, void* stream);
int gcsa2_kmer_chains_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                             uint64_t k, uint64_t stride, uint64_t hit_max, int over,
                             uint64_t shift, const uint64_t* d_coord_of_bin, uint64_t n_bins, const gcsa2_chain_params* params,
                             gcsa2_chain* d_top, gcsa2_chain_anchor* d_members, gcsa2_chain_summary* d_summaries,
                             gcsa2_chain_stats* stats, void* stream);
int gcsa2_minimizer_chains_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                                  uint64_t k, uint64_t w, uint64_t hash_seed, uint64_t hit_max, int over,
                                  uint64_t shift, const uint64_t* d_coord_of_bin, uint64_t n_bins, const gcsa2_chain_params* params,
                                  gcsa2_chain* d_top, gcsa2_chain_anchor* d_members, gcsa2_chain_summary* d_summaries,
                                  gcsa2_chain_stats* stats, void* stream);
/* The same for reads and the coordinate map in host memory, into host arrays, as gcsa2_kmer_clusters_batch: offsets[0] == 0,
 * decreasing offsets are refused; a large batch travels in pieces of whole reads (GCSA2_MS_PIECE_MB, GCSA2_MS_THREADS); the map
 * is uploaded once, a row belongs to one read and so does not depend on the cut, stats are summed over the pieces. */
int gcsa2_kmer_chains_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                            uint64_t k, uint64_t stride, uint64_t hit_max, int over,
                            uint64_t shift, const uint64_t* coord_of_bin, uint64_t n_bins, const gcsa2_chain_params* params,
                            gcsa2_chain* top /* host, n_patterns x top_n, or NULL */,
                            gcsa2_chain_anchor* members /* host, n_patterns x top_n x member_cap, or NULL */,
                            gcsa2_chain_summary* summaries /* host, or NULL */, gcsa2_chain_stats* stats);
int gcsa2_minimizer_chains_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                                 uint64_t k, uint64_t w, uint64_t hash_seed, uint64_t hit_max, int over,
                                 uint64_t shift, const uint64_t* coord_of_bin, uint64_t n_bins, const gcsa2_chain_params* params,
                                 gcsa2_chain* top, gcsa2_chain_anchor* members, gcsa2_chain_summary* summaries,
                                 gcsa2_chain_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* GCSA2_HIP_CHAINS_H */
