/* gcsa2_hip_pairs.h -- chain pairs: per read pair the top placements of a chain of one mate and a chain of the other under a
 * fragment model.  Part of the C ABI of gcsa2_hip.h (gcsa2_index, the status codes, GCSA2_UNKNOWN and gcsa2_last_error() are
 * declared there); the chain rows are those of gcsa2_hip_chains.h, the group order is that of gcsa2_hip_strands.h.
 *
 * ---- chain pairs ------------------------------------------------------------------------------------------------------------
 * gcsa2_stranded_minimizer_hits_device seeds both strands of every read, gcsa2_seed_chains_device chains every group.  Short
 * reads come in pairs: with the mates interleaved as reads 2p and 2p + 1, a pair has four chain rows, and a paired-end mapper
 * joins them next.  It asks which chain of one mate and which chain of the other lie on opposite strands, in the right order
 * and a plausible fragment length apart, what each such placement scores, and whether a second one is nearly as good.  Here the
 * rows stay on the device and what leaves is, per pair, the top_n placements of 64 bytes each and a summary.
 *
 * DEFINITION (gcsa2_chain_pairs_device).  Everything is plain, non-wrapping 64-bit arithmetic.
 *   - Groups: pair p owns the groups 4p + 2m + s, mate m in {0, 1}, strand s in {0, 1}: the group order of
 *     gcsa2_stranded_minimizer_hits_device on an interleaved batch.  The row of group g is
 *     d_chains[g chain_top_n .. (g + 1) chain_top_n).  Every entry of a row is examined; an empty entry in the middle of a row
 *     does not end it.  Only score, anchors, ref_begin and ref_end of an entry are read.
 *   - An entry is EMPTY iff anchors == 0.  A non-empty entry is VALID iff score < 2^62, ref_begin < ref_end and ref_end < 2^62;
 *     otherwise it is IGNORED.
 *   - Combinations: per orientation two, c = 0 and c = 1, each a left and a right group (m, s):
 *       GCSA2_PAIR_FR   (0,0) -> (1,1)   and   (1,0) -> (0,1)
 *       GCSA2_PAIR_RF   (0,1) -> (1,0)   and   (1,1) -> (0,0)
 *       GCSA2_PAIR_FF   (0,0) -> (1,0)   and   (1,1) -> (0,1)
 *   - A CANDIDATE is (c, i, j): valid entry i = L of the left group and valid entry j = R of the right group of combination c.
 *     It is PROPER iff L.ref_begin <= R.ref_begin, L.ref_end <= R.ref_end and fragment = R.ref_end - L.ref_begin lies in
 *     [min_fragment, max_fragment].  A proper fragment is at least 1, so fragment == 0 marks an empty output entry.
 *   - deviation = |fragment - mean_fragment|; penalty = cost (deviation / unit), the division an integer one;
 *     chain_score = L.score + R.score; score = chain_score - min(penalty, chain_score).  A proper candidate is KEPT iff
 *     score >= min_score.
 *   - The top row: order the kept candidates by larger score, then smaller deviation, then smaller (c, i, j).
 *     d_top[p top_n + r] for r < min(top_n, kept) is the r-th kept candidate: { score, fragment, penalty, chain_score,
 *     left_group, left_chain = i, right_group, right_chain = j }, the groups written as 2m + s.  Every later entry of the row is
 *     all zero.
 *   - summary(p) = { candidates (both combinations, every valid x valid), proper, kept, ignored (the ignored entries of the four
 *     rows), mate1_score, mate1_at, mate2_score, mate2_at }.  mateN_score is the largest score over the valid entries of mate
 *     N's two groups and mateN_at = (2m + s) << 32 | entry, the smallest such value among equal scores; a mate without a valid
 *     entry has mateN_score = 0 and mateN_at = GCSA2_UNKNOWN.  These are what an unpaired fallback or a rescue needs.
 *   - stats: pairs = n_pairs; candidates, proper, kept, ignored = the sums over the pairs; paired = the pairs with kept >= 1;
 *     unique = the pairs with kept == 1, unique_fragment_sum = the sum of their one fragment (a caller estimates mean_fragment
 *     from a first batch run with cost = 0).
 *   - Rows and summaries are WRITTEN in full for every pair, and nothing behind them.  d_top, d_summaries and stats may each be
 *     NULL; all three NULL is valid and does the work.
 *
 * GCSA2_ERR_INVALID_ARGUMENT, before any device is touched, with nothing written and stats untouched: a NULL index or NULL
 * params, orientation > 2, top_n or chain_top_n of 0 or above GCSA2_PAIR_TOP_LIMIT, min_fragment > max_fragment, max_fragment
 * or mean_fragment >= 2^32, unit == 0, cost > 65536, min_score >= 2^62, n_pairs >= 2^30, NULL d_chains with n_pairs > 0.
 * With these bounds every intermediate fits 64 bits.  n_pairs == 0 is GCSA2_OK with zero stats.  The call needs no component
 * of the image.  Enqueued on `stream`, complete on return.
 *
 * The fused form gcsa2_minimizer_chain_pairs_device goes from interleaved reads to ranked placements in one call.  LAW: its rows,
 * member rows, summaries and both stats equal, word for word, gcsa2_stranded_minimizer_hits_device(..., GCSA2_STRAND_BOTH, ...)
 * into large enough buffers, then gcsa2_seed_chains_device with the seed offsets as 2 n_patterns groups, then
 * gcsa2_chain_pairs_device with n_pairs = n_patterns / 2 and chain_top_n = the chain parameters' top_n.  It takes the refusals
 * of the three calls, and an odd n_patterns is GCSA2_ERR_INVALID_ARGUMENT; limits and missing components are those of the
 * stranded hits call.  It runs that call's own core into scratch of the call, then the chain core and the pair core: there is no
 * second search or chain kernel.  The chain rows live in scratch when d_chains is NULL.
 *
 * One wavefront owns a pair: lane j holds entry j of each of the pair's four rows in registers (the four words that are read,
 * as 16-byte loads), validity is four ballots, and for every valid entry of a left group, broadcast to the wavefront, lane j
 * evaluates the candidate with entry j of the right group.  The running top row stays in the wavefront's registers; the lanes
 * below top_n rebuild their entry from the rows and store it.  No LDS for the data, global atomics for the stats only.
 *
 * Out of scope: mate rescue, base-level extension, mapping quality, discordant-pair reports, clipping-aware fragment lengths
 * (the fragment is between chain extents, not read ends), and one chain forced into at most one pair. */
#ifndef GCSA2_HIP_PAIRS_H
#define GCSA2_HIP_PAIRS_H

#include "gcsa2_hip_chains.h"
#include "gcsa2_hip_strands.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GCSA2_PAIR_TOP_LIMIT 64                  /* top_n and chain_top_n may be 1 .. GCSA2_PAIR_TOP_LIMIT */
#define GCSA2_PAIR_FR 0   /* inward: the forward-strand mate upstream */
#define GCSA2_PAIR_RF 1   /* outward */
#define GCSA2_PAIR_FF 2   /* same strand, mate 1 upstream on its own strand */
typedef struct gcsa2_pair_params  { uint64_t orientation, min_fragment, max_fragment, mean_fragment, unit, cost, min_score, top_n; } gcsa2_pair_params;
typedef struct gcsa2_chain_pair   { uint64_t score, fragment, penalty, chain_score, left_group, left_chain, right_group, right_chain; } gcsa2_chain_pair;
typedef struct gcsa2_pair_summary { uint64_t candidates, proper, kept, ignored, mate1_score, mate1_at, mate2_score, mate2_at; } gcsa2_pair_summary;
typedef struct gcsa2_pair_stats   { uint64_t pairs, candidates, proper, kept, ignored, paired, unique, unique_fragment_sum; } gcsa2_pair_stats;
int gcsa2_chain_pairs_device(const gcsa2_index* index, const gcsa2_chain* d_chains /* 4 n_pairs x chain_top_n */, uint64_t n_pairs, uint64_t chain_top_n,
                             const gcsa2_pair_params* params, gcsa2_chain_pair* d_top /* n_pairs x top_n, or NULL */,
                             gcsa2_pair_summary* d_summaries /* n_pairs, or NULL */, gcsa2_pair_stats* stats /* host, or NULL */, void* stream);
int gcsa2_minimizer_chain_pairs_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns /* even */,
                                       uint64_t k, uint64_t w, uint64_t hash_seed, uint64_t hit_max, int over,
                                       uint64_t shift, const uint64_t* d_coord_of_bin, uint64_t n_bins,
                                       const gcsa2_chain_params* chain_params, const gcsa2_pair_params* pair_params,
                                       gcsa2_chain* d_chains /* 2 n_patterns x chain top_n, or NULL */, gcsa2_chain_anchor* d_members /* or NULL */,
                                       gcsa2_chain_summary* d_chain_summaries /* 2 n_patterns, or NULL */,
                                       gcsa2_chain_pair* d_top /* n_patterns / 2 x top_n, or NULL */, gcsa2_pair_summary* d_summaries /* n_patterns / 2, or NULL */,
                                       gcsa2_chain_stats* chain_stats, gcsa2_pair_stats* pair_stats, void* stream);
/* The same for reads and the coordinate map in host memory, into host arrays, as gcsa2_minimizer_chains_batch: a large batch
 * travels in pieces of whole PAIRS; per-pair outputs are indexed by pair, per-group outputs by group; both stats are summed over
 * the pieces.  An odd n_patterns is refused with nothing written. */
int gcsa2_minimizer_chain_pairs_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns /* even */,
                                      uint64_t k, uint64_t w, uint64_t hash_seed, uint64_t hit_max, int over,
                                      uint64_t shift, const uint64_t* coord_of_bin, uint64_t n_bins,
                                      const gcsa2_chain_params* chain_params, const gcsa2_pair_params* pair_params,
                                      gcsa2_chain* chains, gcsa2_chain_anchor* members, gcsa2_chain_summary* chain_summaries,
                                      gcsa2_chain_pair* top, gcsa2_pair_summary* summaries,
                                      gcsa2_chain_stats* chain_stats, gcsa2_pair_stats* pair_stats);

#ifdef __cplusplus
}
#endif
#endif /* GCSA2_HIP_PAIRS_H */
