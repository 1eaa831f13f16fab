// kernels_strands.hpp -- stranded minimizer seeds (gcsa2_hip_strands.h): the canonical (w, k)-minimizers of every read
// (gcsa2_canonical_minimizers_device), the list of searched windows of both strands and the k-mer seed search over windows
// that are 64-bit keys (gcsa2_stranded_minimizer_hits_device).
// Part of the single translation unit gcsa2_hip.hip (device code, anonymous namespace).
#pragma once

#include "kernels_minimizers.hpp"
#include "../../include/gcsa2_hip_strands.h"

using namespace g2;

namespace {

// The key of the reverse complement of the k-mer `key` (2 k bits, the first character on top) under the code complement
// c -> 3 - c: the bit-reverse puts the last character on top with the two bits of every code swapped, the swap inside the pairs
// puts them back, the NOT complements every code, and the shift drops the 64 - 2 k bits that lay above the key (by 0 at k = 32).
__device__ __forceinline__ u64 mini_rckey(u64 key, u32 k)
{
  const u64 r = __brevll(key);
  const u64 codes = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
  return ~codes >> (64 - 2 * k);
}

// k_minimizers' tile walk with chash = min(mix64(key ^ seed), mix64(rckey ^ seed)) as the hash of a window; the records carry
// the key of the window as written and the strand whose hash won (1: the reverse complement's; 0 on a tie, which only a window
// that is its own reverse complement has).  A sibling kernel over the same text: k_minimizers keeps its code.
template<bool PLACE>
__global__ __launch_bounds__(MINI_TPB) void k_canonical_minimizers(DevImage img, const u8* __restrict__ patterns, const u64* __restrict__ offsets,
                                                                   u64 n_patterns, u32 k, u32 w, u64 hash_seed, u64* __restrict__ sizes,
                                                                   const u64* __restrict__ min_offsets, gcsa2_canonical_minimizer* __restrict__ recs)
{
#define MINI_CANONICAL 1
#include "kernels_minimizers_body.hpp"
#undef MINI_CANONICAL
}

constexpr u32 STRAND_LANES = 16;               // lanes that share a read in k_strand_windows

// The minimizer CSR (min_offsets, mins) as the group CSR of the search (group_offsets, 2 n_patterns + 1 entries) and its list
// of windows, group-major: group 2q = the minimizers of read q as written, {key, position} in ascending position; group 2q + 1 =
// the same windows of the read's reverse complement, {rckey, L - k - position}, in ascending position there -- the reverse group
// reversed.  A strand that is not asked for has empty groups and no entry in the list.  Sixteen lanes per read.
__global__ __launch_bounds__(TPB) void k_strand_windows(const u64* __restrict__ offsets, u64 n_patterns, u32 k, const u64* __restrict__ min_offsets,
                                                        const gcsa2_canonical_minimizer* __restrict__ mins, u32 strands,
                                                        u64* __restrict__ group_offsets, ulonglong2* __restrict__ wins)
{
  const u64 t = u64(blockIdx.x) * TPB + threadIdx.x, q = t / STRAND_LANES;
  const u32 sub = u32(t % STRAND_LANES);
  if(q > n_patterns) { return; }
  const u64 per = (strands == GCSA2_STRAND_BOTH ? 2 : 1);
  const u64 from = min_offsets[q];
  if(q == n_patterns) { if(sub == 0) { group_offsets[2 * q] = per * from; } return; }
  const u64 m = min_offsets[q + 1] - from, len = offsets[q + 1] - offsets[q];
  const bool fwd = (strands & GCSA2_STRAND_FORWARD) != 0, rev = (strands & GCSA2_STRAND_REVERSE) != 0;
  const u64 fwd_at = per * from, rev_at = fwd_at + (fwd ? m : 0);
  if(sub == 0) { group_offsets[2 * q] = fwd_at; group_offsets[2 * q + 1] = rev_at; }
  for(u64 x = sub; x < m; x += STRAND_LANES)
  {
    const u64 position = mins[from + x].position, key = mins[from + x].key;      // position + k <= len: a window of the read
    if(fwd) { wins[fwd_at + x] = make_ulonglong2(key, position); }
    if(rev) { wins[rev_at + (m - 1 - x)] = make_ulonglong2(mini_rckey(key, k), len - k - position); }
  }
}

// The k-mer seed search (k_kmer_seeds) over windows that are keys: lane g searches the k characters of wins[g].x -- character i
// of the window at bits [2 (k - 1 - i), 2 (k - 1 - i) + 2), every one a fast character (comp = 1 + code) -- and emits
// wins[g].y as the seed's position.  The backward search consumes the key from its low end: the seed-table index is its low
// 2 kmer_k bits, the next one or two characters are its low bits after a shift.  There is no pattern byte, no bad-character
// path and no refill.  Block fetch, evaluation, pair outcome with its single-step replay (the key is not shifted then) are
// those of kernels_windows_body.hpp; the lane's final range goes through the same kernels_windows_tail.hpp.
template<bool PAIR>
__global__ __launch_bounds__(TPB2, FIND_WAVES) void k_strand_seeds(DevImage img, u64 k, const ulonglong2* __restrict__ wins,
                                                                   const u64* __restrict__ window_offsets, const u64* __restrict__ owners, u64 total,
                                                                   gcsa2_kmer_profile* __restrict__ profiles, SeedEmit emit)
{
  constexpr bool COUNTS = true;
  u64* const out = nullptr;
  u64* const counts = nullptr;
  __shared__ ulonglong2 stage[TPB2 * 8];
  __shared__ u64 crange[2 * MAX_SIGMA];
  if(threadIdx.x < 2 * MAX_SIGMA) { crange[threadIdx.x] = img.crange[threadIdx.x]; }
  __syncthreads();

  const u64 first = u64(blockIdx.x) * TPB2;            // < total: the grid covers the windows exactly
  const u32 lane = threadIdx.x & 63;
  ulonglong2* wave_stage = stage + (threadIdx.x & ~63u) * 8;
  const u64 gid = first + threadIdx.x;
  const bool live = gid < total;

  u64 q = ~u64(0), sp = 0, ep = img.n - 1, i = 0;
  u64 win = 0;                                 // the characters not yet consumed, the next one in the low two bits
  bool done = true;
  [[maybe_unused]] u32 force_single = 0;       // PAIR: characters that must be consumed by single steps (replay)

  if(live)
  {
    q = owner_in_wave(owners, window_offsets, total, gid, true);
    const u64 at = window_offsets[q], j = gid - at;
    if(j == 0 && profiles != nullptr) { reinterpret_cast<u64*>(profiles + q)[0] = window_offsets[q + 1] - at; }
    if(img.n > 0)                                              // gcsa.h:99 (k >= 1)
    {
      win = wins[gid].x;
      const u32 tk = img.kmer_k;                               // <= 16
      bool seeded = false;
      if(tk > 0 && k >= tk)
      {
        const u64 entry = img.kmer_table[win & ((u64(1) << (2 * tk)) - 1)];
        if((entry >> SEED_SP_BITS) != SEED_WIDE)               // a wide range is not in the table
        {
          sp = entry & SEED_SP_MASK; ep = sp + (entry >> SEED_SP_BITS) - 1;
          i = k - tk; win >>= 2 * tk; seeded = true;
        }
      }
      if(!seeded)
      {
        i = k - 1;
        const u32 comp = 1 + (u32(win) & 3);
        win >>= 2;
        sp = crange[2 * comp]; ep = crange[2 * comp + 1];      // charRange, gcsa.h:101-102, 150-153
      }
      done = range_empty(sp, ep) || i == 0;                    // gcsa.h:103
    }
  }

  while(true)
  {
    if(!__any(!done)) { break; }
    const bool stepping = !done;
    u32 r_sp = 0, r_ep = 0, idx_sp = 0, idx_ep = 0;
    bool pair = false;
    if(stepping)
    {
      if constexpr(PAIR)
      {
        if(force_single == 0 && i >= 2)
        {
          pair = true;
          const u32 c2 = u32(win) & 3, c1 = u32(win >> 2) & 3;     // positions i - 1 and i - 2
          u32 b_sp, b_ep;
          pair_block_of(sp, b_sp, r_sp); pair_block_of(ep + 1, b_ep, r_ep);
          const u32 head = (c1 * 4 + c2) * u32(img.flp_nblocks);
          idx_sp = (head + b_sp) | PAIR_FLAG; idx_ep = (head + b_ep) | PAIR_FLAG;
        }
      }
      if(!pair)
      {
        i--;
        if constexpr(PAIR) { force_single -= (force_single > 0 ? 1 : 0); }
        const u32 comp = 1 + (u32(win) & 3);
        win >>= 2;
        u32 b_sp, b_ep;
        flb_block_of(sp, b_sp, r_sp); flb_block_of(ep + 1, b_ep, r_ep);
        idx_sp = comp * u32(img.flb_nblocks) + b_sp; idx_ep = comp * u32(img.flb_nblocks) + b_ep;
      }
    }
    PairEnd p_sp = {0, 0, 0}, p_ep = {0, 0, 0};   // a single step keeps (edge, node) in .raw / .node
    const bool need2 = stepping && idx_ep != idx_sp;
    ulonglong2 blk[8];
    fetch_blocks<PAIR>(img.flb, idx_sp, stepping, wave_stage, lane, img.flp);
    if(stepping)
    {
      read_block(wave_stage, lane, blk);
      if(PAIR && pair)
      {
        p_sp = eval_pair(blk, r_sp, false);
        if(idx_ep == idx_sp) { p_ep = eval_pair(blk, r_ep, true); }
      }
      else
      {
        eval_endpoint(blk, r_sp, 0, p_sp.raw, p_sp.node);
        if(idx_ep == idx_sp) { eval_endpoint(blk, r_ep, 1, p_ep.raw, p_ep.node); }
      }
    }
    if(__any(need2))
    {
      __builtin_amdgcn_wave_barrier();
      fetch_blocks<PAIR>(img.flb, idx_ep, need2, wave_stage, lane, img.flp);
      if(need2)
      {
        read_block(wave_stage, lane, blk);
        if(PAIR && pair) { p_ep = eval_pair(blk, r_ep, true); }
        else { eval_endpoint(blk, r_ep, 1, p_ep.raw, p_ep.node); }
      }
    }
    __builtin_amdgcn_wave_barrier();
    if(stepping)
    {
      if(PAIR && pair)
      {
        u64 a = 0, b = 0;
        const u32 outcome = pair_outcome(p_sp, p_ep, idx_ep == idx_sp, a, b);
        if(outcome == 2) { sp = p_sp.node; ep = p_ep.node; i -= 2; win >>= 4; done = (i == 0); }     // neither step empties
        else if(outcome == 1) { sp = a; ep = b; i -= 2; win >>= 4; done = true; }     // the second step empties, gcsa.h:160
        else { force_single = 2; }                             // replayed as two single steps from the unchanged (sp, ep)
      }
      else
      {
        const u64 a = p_sp.raw, b = p_ep.raw - 1;              // edge space
        if(range_empty(a, b)) { sp = a; ep = b; done = true; } // gcsa.h:160
        else { sp = p_sp.node; ep = p_ep.node; done = (i == 0); }   // gcsa.h:161, 103
      }
    }
  }

#define KMER_WINDOWS_EMIT 1
#define KMER_WINDOWS_POSITION(g) (wins[g].y)
#include "kernels_windows_tail.hpp"
#undef KMER_WINDOWS_POSITION
#undef KMER_WINDOWS_EMIT
}

}  // namespace
