// kernels_extend.hpp -- extend: the backward search of gcsa.h:96-110 continued from caller-supplied ranges over substrings of a
// shared pattern set (gcsa2_extend_device).  The block machinery is k_find2's (kernels_find.hpp).
// Part of the single translation unit gcsa2_hip.hip (device code, anonymous namespace).
#pragma once

#include "kernels_find.hpp"

using namespace g2;

namespace {

// One lane = one search state (pattern, begin, end, sp, ep): the loop `while(!empty(range) && end != begin) range =
// LF(range, *--end)` from (sp, ep) over P[begin, end), with the number of steps that left a non-empty range and the last such
// range kept beside the range the loop ends with (the contract is in gcsa2_hip.h).  Per step the wave fetches its 64 blocks as
// k_find2 does -- eight lanes per 128-byte block, staged in LDS -- and the pattern characters come from the same packed window.
//
// What differs from k_find2:
//   - The range is the caller's, so its two positions are clamped to n before they select a block (memory safety only, as in
//     lf_step_wave; a range the search itself produced is never changed by that).
//   - The seed table answers for the root only: a state that starts at (0, n - 1) takes its entry when that is a non-empty,
//     non-wide range -- then all k steps were non-empty and the entry is the range after them.  An empty entry does not say
//     WHICH step emptied, and `matched` is that step's number: such a state steps from the start.
//   - PAIR: a two-character step is taken only when it proves BOTH steps non-empty.  k_find2 also takes the outcome "the
//     second step empties" from the pair block (its edge-space integers are there); the range after the first step -- `last`
//     here -- is not, so that outcome is replayed as two single steps as well.
//   - No jump table (valid from any range, but not worth a second code path here) and no counters.
template<bool PAIR>
__global__ __launch_bounds__(TPB2, FIND_WAVES) void k_extend(DevImage img, const u8* __restrict__ patterns, const u64* __restrict__ offsets,
                                                             u64 n_patterns, const gcsa2_search_state* __restrict__ states, u64 ns,
                                                             gcsa2_extension* __restrict__ out)
{
  __shared__ ulonglong2 stage[TPB2 * 8];
  __shared__ u8 c2c[256];
  c2c[threadIdx.x] = img.char2comp[threadIdx.x];
  c2c[threadIdx.x + TPB2] = img.char2comp[threadIdx.x + TPB2];
  __syncthreads();

  const u32 lane = threadIdx.x & 63;
  ulonglong2* wave_stage = stage + (threadIdx.x & ~63u) * 8;
  const u64 gid = u64(blockIdx.x) * TPB2 + threadIdx.x;

  u64 sp = 0, ep = 0, last_sp = 0, last_ep = 0, matched = GCSA2_UNKNOWN;
  u64 i = 0;                                   // characters of P[begin, end) not yet consumed; p = &P[begin]
  const u8* p = patterns;
  bool done = true;
  u64 win_code = 0;                            // packed pattern window (k_find2)
  u32 win_used = ~u32(0), win_bad = 0;
  [[maybe_unused]] u32 force_single = 0;       // PAIR: characters that must be consumed by single steps (replay)

  if(gid < ns)
  {
    const u64* s = reinterpret_cast<const u64*>(states + gid);
    const u64 pattern = s[0], begin = s[1], end = s[2];
    sp = s[3]; ep = s[4]; last_sp = sp; last_ep = ep;
    if(pattern < n_patterns)                   // an invalid state reads neither an offset nor a pattern byte
    {
      const u64 first = offsets[pattern], len = offsets[pattern + 1] - first;
      if(begin <= end && end <= len)
      {
        matched = 0;
        p = patterns + first + begin; i = end - begin;
        done = (i == 0 || range_empty(sp, ep) || img.n == 0);
        const u32 k = img.kmer_k;
        if(!done && sp == 0 && ep == img.n - 1 && k > 0 && i >= k)
        {
          u64 tix = 0;
          bool fast = true;
          for(u32 j = 0; j < k; j++)               // j-th character from the end
          {
            const u32 comp = c2c[p[i - 1 - j]];
            fast = fast && (comp - 1 < 4);
            tix |= u64((comp - 1) & 3) << (2 * j);
          }
          const u64 entry = img.kmer_table[fast ? tix : 0], len_field = entry >> SEED_SP_BITS;
          if(fast && len_field != 0 && len_field != SEED_WIDE)
          {
            sp = entry & SEED_SP_MASK; ep = sp + len_field - 1;
            i -= k; matched = k; done = (i == 0);
          }
        }
      }
    }
  }

  while(true)
  {
    if(!__any(!done)) { break; }
    // The next pattern characters as 2-bit codes, refilled once per 24 consumed characters (k_find2's window: position
    // win_top - 1 - r at bits [2r, 2r + 2) of win_code, bit r of win_bad = "not a fast character").
    if(!done && win_used > 24)
    {
      win_used = 0; win_code = 0; win_bad = 0;
      const u64 count = (i < 32 ? i : 32), low = reinterpret_cast<u64>(p) + i - count, base = low & ~u64(7);
      u64 w[5];
      const u64 last = (low + count - 1) & ~u64(7);             // never read past the word of the last byte needed
#pragma unroll
      for(u32 k = 0; k < 5; k++) { const u64 a = base + 8 * k; w[k] = *reinterpret_cast<const u64*>(a < last ? a : last); }
      for(u32 r = 0; r < count; r++)
      {
        const u64 at = (low - base) + (count - 1 - r);         // byte offset of position win_top - 1 - r
        u64 word = w[0];
#pragma unroll
        for(u32 k = 1; k < 5; k++) { if((at >> 3) == k) { word = w[k]; } }
        const u32 c = u32(c2c[u32(word >> ((at & 7) * 8)) & 0xFF]) - 1;
        win_code |= u64(c & 3) << (2 * r);
        win_bad |= u32(c < 4 ? 0 : 1) << r;
      }
    }
    const bool stepping = !done;
    u32 comp = 0, r_sp = 0, r_ep = 0, idx_sp = 0, idx_ep = 0;
    bool pair = false;
    if(stepping)
    {
      const u64 at_sp = clampu(sp, img.n), at_ep = clampu(ep + 1, img.n);
      if constexpr(PAIR)
      {
        if(force_single == 0 && i >= 2)
        {
          const u32 r = win_used;                              // window slot of position i - 1; i - 2 is slot r + 1
          pair = ((win_bad >> r) & 3) == 0;                    // both are fast characters
          if(pair)
          {
            const u32 c2 = u32(win_code >> (2 * r)) & 3, c1 = u32(win_code >> (2 * r + 2)) & 3;
            u32 b_sp, b_ep;
            pair_block_of(at_sp, b_sp, r_sp); pair_block_of(at_ep, b_ep, r_ep);
            const u32 first = (c1 * 4 + c2) * u32(img.flp_nblocks);
            idx_sp = (first + b_sp) | PAIR_FLAG; idx_ep = (first + b_ep) | PAIR_FLAG;
          }
        }
      }
      if(!pair)
      {
        i--;
        if constexpr(PAIR) { force_single -= (force_single > 0 ? 1 : 0); }
        const u32 r = win_used++;
        if((win_bad >> r) & 1) { comp = c2c[p[i]]; }           // rare: the byte itself
        else { comp = 1 + (u32(win_code >> (2 * r)) & 3); }
        if(comp >= u32(img.sigma)) { comp = u32(img.sigma) - 1; }     // memory safety only
        u32 b_sp, b_ep;
        flb_block_of(at_sp, b_sp, r_sp); flb_block_of(at_ep, b_ep, r_ep);
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
        if(pair_outcome(p_sp, p_ep, idx_ep == idx_sp, a, b) == 2)     // neither step empties
        {
          sp = p_sp.node; ep = p_ep.node; i -= 2; win_used += 2; matched += 2; done = (i == 0);
        }
        else { force_single = 2; }               // one of them empties: two single steps from the unchanged (sp, ep)
      }
      else
      {
        const u64 a = p_sp.raw, b = p_ep.raw - 1;              // edge space
        if(range_empty(a, b)) { last_sp = sp; last_ep = ep; sp = a; ep = b; done = true; }     // gcsa.h:160
        else { sp = p_sp.node; ep = p_ep.node; matched++; done = (i == 0); }                   // gcsa.h:161, 103
      }
    }
  }
  if(gid < ns)
  {
    if(!range_empty(sp, ep)) { last_sp = sp; last_ep = ep; }  // no step emptied: the last non-empty range is the final one
    u64* o = reinterpret_cast<u64*>(out + gid);
    o[0] = matched; o[1] = sp; o[2] = ep; o[3] = last_sp; o[4] = last_ep;
  }
}

}  // namespace
