// kernels_pairs.hpp -- chain pairs (gcsa2_chain_pairs_device and its fused forms, include/gcsa2_hip_pairs.h): per read pair
// the top_n placements of a chain of one mate and a chain of the other under a fragment model.  Included by gcsa2_hip.hip after
// kernels_chains.hpp; of kernels_clusters.hpp it uses the top row in the registers of a wavefront (clu_ahead, clu_top_insert)
// and the pad CLU_NONE.
//
// Data flow: one kernel, k_chain_pairs<orientation>.  One wavefront owns a pair, four pairs to a workgroup of TPB, the pairs
// strided over a capped grid.  Lane j loads entry j of the pair's four chain rows -- the four words that are read -- into
// registers; four ballots say which entries are valid; per combination the wavefront walks the valid entries of the left group,
// broadcasts each, and lane j evaluates the candidate with entry j of the right group.  The kept candidates ahead of entry
// top_n - 1 of the running top row join it (clu_top_insert); the lanes below top_n rebuild their entry from the rows with two
// lane-indexed shuffles per word and store it.  No LDS for the data; the counters of a workgroup meet in LDS for one atomic each.
#pragma once

namespace {

constexpr u64 PAIR_LIMIT = u64(1) << 62;                    // a chain with a score or a ref_end at or beyond it is ignored
// the counters of a call, in the order of gcsa2_pair_stats behind `pairs`
enum : u32 { PAIR_CANDIDATES = 0, PAIR_PROPER = 1, PAIR_KEPT = 2, PAIR_IGNORED = 3, PAIR_PAIRED = 4, PAIR_UNIQUE = 5, PAIR_FRAGMENT_SUM = 6, PAIR_WORDS = 7 };
static_assert(GCSA2_PAIR_TOP_LIMIT == 64 && GCSA2_PAIR_TOP_LIMIT == GCSA2_CHAIN_TOP_LIMIT, "one lane per entry of a chain row and of the top row");
static_assert(sizeof(gcsa2_chain_pair) == 64 && sizeof(gcsa2_pair_summary) == 64 && sizeof(gcsa2_pair_stats) == 64 && sizeof(gcsa2_pair_params) == 64,
              "eight words each");
static_assert(sizeof(gcsa2_pair_stats) == (1 + PAIR_WORDS) * sizeof(u64), "pairs, then the counters");
static_assert(TPB == 256, "four wavefronts, four pairs, to a workgroup");

// top_n and chain_top_n are 1 .. 64; max_fragment, mean_fragment < 2^32; cost <= 2^16; min_score < 2^62 (the refusals).  So
// deviation < 2^32, penalty <= 2^16 (2^32 - 1) < 2^48, chain_score < 2^63, and the key of a candidate
// deviation << 13 | c << 12 | i << 6 | j is below 2^45 < CLU_NONE.
struct PairParams { u64 min_fragment, max_fragment, mean_fragment, unit, cost, min_score; u32 top_n, chain_top_n; };

// the left and right group (2m + s) of combination c of an orientation
template<u32 O> __device__ __forceinline__ constexpr u32 pair_left(u32 c)
{
  return (O == GCSA2_PAIR_FR ? (c == 0 ? 0u : 2u) : O == GCSA2_PAIR_RF ? (c == 0 ? 1u : 3u) : (c == 0 ? 0u : 3u));
}
template<u32 O> __device__ __forceinline__ constexpr u32 pair_right(u32 c)
{
  return (O == GCSA2_PAIR_FR ? (c == 0 ? 3u : 1u) : O == GCSA2_PAIR_RF ? (c == 0 ? 2u : 0u) : (c == 0 ? 2u : 1u));
}

// words `at` and `at + 1` of a chain record (at even): one 16-byte load where the rows are 16-byte aligned
__device__ __forceinline__ void pair_load2(const u64* __restrict__ rec, u32 at, bool aligned, u64& a, u64& b)
{
  if(aligned) { const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(rec + at); a = v.x; b = v.y; }
  else { a = rec[at]; b = rec[at + 1]; }
}

// penalty = cost (deviation / unit); deviation < 2^32, so a unit of 2^32 or more divides it to 0 and the division is one of 32 bits
__device__ __forceinline__ u64 pair_penalty(const PairParams& P, u64 deviation)
{
  return ((P.unit >> 32) != 0 ? 0 : P.cost * u64(u32(deviation) / u32(P.unit)));
}

// the larger score, then the smaller `at`, of two (score, at); (0, CLU_NONE) is "no valid entry": every valid one is ahead of it
__device__ __forceinline__ void pair_best(u64& s, u64& at, u64 os, u64 oat)
{
  if(clu_ahead(os, oat, s, at)) { s = os; at = oat; }
}

// Per workgroup at most PAIR_WORDS atomics, one a counter.
template<u32 O>
__global__ __launch_bounds__(TPB) void k_chain_pairs(const u64* __restrict__ chains, u64 n_pairs, PairParams P, bool aligned, u64* __restrict__ top,
                                                     u64* __restrict__ summaries, unsigned long long* __restrict__ stat)
{
  __shared__ u64 sums[TPB / 64][PAIR_WORDS];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  const u64 lane_bit = u64(1) << lane;
  u64 all[PAIR_WORDS] = {0, 0, 0, 0, 0, 0, 0};
  for(u64 p = u64(blockIdx.x) * (TPB / 64) + wave; p < n_pairs; p += u64(gridDim.x) * (TPB / 64))
  {
    // the four rows: score, ref_begin, ref_end of entry `lane`, and which entries are valid
    u64 sc[4], rb[4], re[4], valid[4], ignored = 0;
#pragma unroll
    for(u32 g = 0; g < 4; g++)
    {
      u64 anchors = 0;
      sc[g] = 0; rb[g] = 0; re[g] = 0;
      if(lane < P.chain_top_n)
      {
        const u64* rec = chains + ((4 * p + g) * P.chain_top_n + lane) * 8;
        pair_load2(rec, 0, aligned, sc[g], anchors);
        pair_load2(rec, 6, aligned, rb[g], re[g]);
      }
      const bool ok = (anchors != 0 && sc[g] < PAIR_LIMIT && rb[g] < re[g] && re[g] < PAIR_LIMIT);
      valid[g] = __ballot(ok);
      ignored += u64(__popcll(__ballot(anchors != 0 && !ok)));
    }
    // the candidates of both combinations
    u64 rs = 0, rk = CLU_NONE, rx = 0, candidates = 0, proper = 0, kept = 0;
#pragma unroll
    for(u32 c = 0; c < 2; c++)
    {
      constexpr u32 L0 = pair_left<O>(0), L1 = pair_left<O>(1), R0 = pair_right<O>(0), R1 = pair_right<O>(1);
      const u32 L = (c == 0 ? L0 : L1), R = (c == 0 ? R0 : R1);
      const bool right = (valid[R] & lane_bit) != 0;
      candidates += u64(__popcll(valid[L])) * u64(__popcll(valid[R]));
      for(u64 left = valid[L]; left != 0; left &= left - 1)
      {
        const int i = __ffsll((unsigned long long)left) - 1;
        const u64 ls = __shfl(sc[L], i, 64), lb = __shfl(rb[L], i, 64), le = __shfl(re[L], i, 64);
        const u64 fragment = re[R] - lb;                       // used only if lb <= rb[R] < re[R]
        const bool fits = (right && lb <= rb[R] && le <= re[R] && fragment >= P.min_fragment && fragment <= P.max_fragment);
        const u64 deviation = (fragment > P.mean_fragment ? fragment - P.mean_fragment : P.mean_fragment - fragment);
        u64 s = 0, k = CLU_NONE;
        bool keep = false;
        if(fits)
        {
          const u64 chain_score = ls + sc[R], penalty = pair_penalty(P, deviation);
          s = chain_score - (penalty < chain_score ? penalty : chain_score);
          keep = (s >= P.min_score);
          k = (deviation << 13) | (u64(c) << 12) | (u64(i) << 6) | lane;
        }
        proper += u64(__popcll(__ballot(fits)));
        const u64 keeps = __ballot(keep);
        if(keeps == 0) { continue; }
        kept += u64(__popcll(keeps));
        const u64 cut_s = __shfl(rs, int(P.top_n - 1), 64), cut_k = __shfl(rk, int(P.top_n - 1), 64);
        for(u64 fresh = __ballot(keep && clu_ahead(s, k, cut_s, cut_k)); fresh != 0; fresh &= fresh - 1)
        {
          const int src = __ffsll((unsigned long long)fresh) - 1;
          clu_top_insert(rs, rk, rx, __shfl(s, src, 64), __shfl(k, src, 64), 0);
        }
      }
    }
    // the row: lane r rebuilds entry r from its key.  Every lane takes part in the shuffles; a lane without an entry reads lane 0.
    const u32 winners = u32(kept < P.top_n ? kept : P.top_n);
    {
      constexpr u32 L0 = pair_left<O>(0), L1 = pair_left<O>(1), R0 = pair_right<O>(0), R1 = pair_right<O>(1);
      const bool mine = (lane < winners);
      const u64 key = (mine ? rk : 0), deviation = key >> 13;
      const u32 c = u32(key >> 12) & 1, i = u32(key >> 6) & 63, j = u32(key) & 63;
      const u64 ls0 = __shfl(sc[L0], int(i), 64), ls1 = __shfl(sc[L1], int(i), 64), lb0 = __shfl(rb[L0], int(i), 64), lb1 = __shfl(rb[L1], int(i), 64);
      const u64 os0 = __shfl(sc[R0], int(j), 64), os1 = __shfl(sc[R1], int(j), 64), oe0 = __shfl(re[R0], int(j), 64), oe1 = __shfl(re[R1], int(j), 64);
      if(top != nullptr && lane < P.top_n)
      {
        u64 out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if(mine)
        {
          out[0] = rs; out[1] = (c == 0 ? oe0 - lb0 : oe1 - lb1); out[2] = pair_penalty(P, deviation); out[3] = (c == 0 ? ls0 + os0 : ls1 + os1);
          out[4] = (c == 0 ? L0 : L1); out[5] = i; out[6] = (c == 0 ? R0 : R1); out[7] = j;
        }
        u64* dst = top + (p * P.top_n + lane) * 8;
        if(aligned)
        {
#pragma unroll
          for(u32 word = 0; word < 8; word += 2) { *reinterpret_cast<ulonglong2*>(dst + word) = make_ulonglong2(out[word], out[word + 1]); }
        }
        else
        {
#pragma unroll
          for(u32 word = 0; word < 8; word++) { dst[word] = out[word]; }
        }
      }
      // the one fragment of a pair with one kept candidate is that of lane 0's entry
      const u64 first = __shfl((c == 0 ? oe0 - lb0 : oe1 - lb1), 0, 64);
      all[PAIR_CANDIDATES] += candidates; all[PAIR_PROPER] += proper; all[PAIR_KEPT] += kept; all[PAIR_IGNORED] += ignored;
      if(kept >= 1) { all[PAIR_PAIRED]++; }
      if(kept == 1) { all[PAIR_UNIQUE]++; all[PAIR_FRAGMENT_SUM] += first; }
    }
    // the summary: per mate the best valid entry of its two groups, the smallest (group, entry) among equal scores
    if(summaries != nullptr)
    {
      u64 best[2], at[2];
#pragma unroll
      for(u32 m = 0; m < 2; m++)
      {
        best[m] = 0; at[m] = CLU_NONE;
#pragma unroll
        for(u32 s = 0; s < 2; s++)
        {
          const u32 g = 2 * m + s;
          if((valid[g] & lane_bit) != 0) { pair_best(best[m], at[m], sc[g], (u64(g) << 32) | lane); }
        }
#pragma unroll
        for(u32 o = 32; o > 0; o >>= 1)
        {
          const u64 os = __shfl_xor(best[m], o, 64), oat = __shfl_xor(at[m], o, 64);
          pair_best(best[m], at[m], os, oat);
        }
      }
      if(lane == 0)
      {
        u64* dst = summaries + p * 8;
        dst[0] = candidates; dst[1] = proper; dst[2] = kept; dst[3] = ignored;
        dst[4] = best[0]; dst[5] = at[0]; dst[6] = best[1]; dst[7] = at[1];             // CLU_NONE is GCSA2_UNKNOWN
      }
    }
  }
  // what the workgroup counted: every lane of a wavefront holds the wavefront's sums
  if(lane == 0)
  {
#pragma unroll
    for(u32 f = 0; f < PAIR_WORDS; f++) { sums[wave][f] = all[f]; }
  }
  __syncthreads();
  if(threadIdx.x < PAIR_WORDS)
  {
    u64 sum = 0;
    for(u32 w = 0; w < TPB / 64; w++) { sum += sums[w][threadIdx.x]; }
    if(sum != 0) { atomicAdd(stat + threadIdx.x, (unsigned long long)sum); }
  }
}
static_assert(CLU_NONE == GCSA2_UNKNOWN, "mateN_at of a mate without a valid entry");

}  // namespace
