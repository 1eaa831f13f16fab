// kernels_seeds.hpp -- capped seeds (gcsa2_capped_seeds_device): per read, the shortest matches of at least min_length bases
// that occur at most max_count times, found right to left, the search starting again behind every seed and after every
// failure with the character that failed.  Included by gcsa2_hip.hip after kernels_locate.hpp (count_range) and
// kernels_find.hpp (lf_step_wave).  No LCP array is read.
//
// Data flow: k_capped_seeds<false> (seeds per read) -> exclusive scan (the CSR offsets) -> k_capped_seeds<true> (the same
// walk again, records written at their CSR slots) -> the classify / locate / gather tail of mem_hits (kernels_mem.hpp), fed
// the counts the walk computed.
//
// The walk of one read P of length L (the contract is in include/gcsa2_hip.h), with [i, e) the match and r its range:
//   e = L;  while e > 0:  i = e, r = root;  loop:
//     i == 0 -> the read is done;  e - i == max_length -> e = i, next attempt (the step is not taken)
//     r2 = LF(r, P[i - 1]);  empty -> e = (i == e ? e - 1 : i), next attempt
//     i -= 1, r = r2;  e - i >= min_length and count(r) <= max_count -> emit, e = i, next attempt
// Everything that needs no LF step (the read's start, the cut, an attempt's setup) is settled between two rounds, so a lane
// that holds a read asks for blocks in every round.  Without pair blocks the rounds of a read are its LF steps: at most 2 L.
//
// PAIR (the image has pair blocks): while an attempt is short of min_length by two characters or more, neither the range
// after the next character nor its count is needed, and the two steps go in one request, as in k_extend
// (kernels_extend.hpp) -- taken only when the pair block proves BOTH steps non-empty.  Otherwise one of them empties, and
// which one decides `fail`: the two steps are replayed singly from the unchanged range.  Every field stays the walk's.
// Two passes of the same deterministic walk, as k_submem_walk: the seeds of a batch have no useful bound to size record
// scratch from ahead of time, and the first pass keeps no records.
#pragma once

constexpr u32 SEEDS_REFILL_AT = 8;              // idle lanes of a wave that make it draw new reads

// Control words of one call (zeroed by the host): [0] a walk overran its round bound, [1] the work counter of the
// persistent lanes.
constexpr u32 SEEDS_CTL_WORDS = 2;

// One lane per read; persistent lanes draw reads 0 .. nq through ctl[1].  Every lane of a wave calls lf_step_wave in every
// round (PAIR: the same fetch written out, pair and single steps side by side in one wavefront; the block fetch is
// wave-cooperative); a lane whose match has min_length characters then takes count_range of the new range.  WRITE = false:
// sizes[q] = the seeds of read q.  WRITE = true: seed j of read q at seed_offsets[q] + j, as {position, length, sp, ep} into recs
// and its count into counts (never beyond seed_offsets[q + 1]).  A walk that exceeds 2 L + 2 LF steps sets ctl[0] and ends (a
// pair request that is replayed takes no step; two single steps follow each).
template<bool WRITE, bool PAIR>
__global__ __launch_bounds__(TPB2) void k_capped_seeds(DevImage img, const u8* __restrict__ patterns, const u64* __restrict__ offsets, u64 nq,
                                                       u64 min_length, u64 max_length, u64 max_count, unsigned long long* __restrict__ ctl,
                                                       u64* __restrict__ sizes, const u64* __restrict__ seed_offsets, u64* __restrict__ recs,
                                                       u64* __restrict__ counts)
{
  __shared__ ulonglong2 stage[TPB2 * 8];
  __shared__ u8 c2c[256];
  c2c[threadIdx.x] = img.char2comp[threadIdx.x];
  c2c[threadIdx.x + TPB2] = img.char2comp[threadIdx.x + TPB2];
  __syncthreads();
  const u32 lane = threadIdx.x & 63;
  ulonglong2* wave_stage = stage + (threadIdx.x & ~63u) * 8;
  const u64 root_ep = img.n - 1;
  bool has = false, exhausted = false;
  u64 q = 0, i = 0, e = 0, sp = 0, ep = 0, steps = 0, limit = 0, n_seeds = 0, out_at = 0, out_end = 0;
  [[maybe_unused]] u32 force_single = 0;       // PAIR: characters that must be consumed by single steps (replay)
  const u8* pat = nullptr;
  auto finish = [&]()
  {
    if constexpr(!WRITE) { sizes[q] = n_seeds; }
    has = false;
  };
  // what lies between two LF steps: the end of the read, the cut by max_length.  Leaves the lane with a step to take
  // (i > 0, e - i below a non-zero max_length) or without a read.
  auto settle = [&]()
  {
    while(true)
    {
      if(e < min_length || i == 0) { finish(); return; }        // no match ending at e or before it can reach min_length
      if(max_length != 0 && e - i == max_length) { e = i; sp = 0; ep = root_ep; continue; }
      return;
    }
  };
  auto start = [&](u64 item)
  {
    q = item;
    const u64 first = offsets[q], length = offsets[q + 1] - first;
    pat = patterns + first;
    e = i = length;
    sp = 0; ep = root_ep;
    steps = 0; limit = 2 * length + 2; n_seeds = 0;
    if constexpr(PAIR) { force_single = 0; }
    if constexpr(WRITE) { out_at = seed_offsets[q]; out_end = seed_offsets[q + 1]; }
    has = true;
    settle();
  };
  while(true)
  {
    const u64 idle = __ballot(!has);
    if(!exhausted && (u32(__popcll(idle)) >= SEEDS_REFILL_AT || idle == ~u64(0)))
    {
      const u32 want = u32(__popcll(idle)), leader = u32(__ffsll((long long)idle)) - 1;
      unsigned long long base = 0;
      if(lane == leader) { base = atomicAdd(ctl + 1, (unsigned long long)want); }
      base = __shfl(base, leader, 64);
      if(!has)
      {
        const u64 mine = base + __popcll(idle & ((u64(1) << lane) - 1));
        if(mine < nq) { start(mine); }
      }
      exhausted = (base + want >= nq);
    }
    if(!__any(has))
    {
      if(exhausted) { break; }
      continue;
    }
    u64 nsp = 0, nep = 0, took = 1;             // the range after this round's step(s), the characters consumed
    if constexpr(!PAIR)
    {
      const u32 comp = has ? u32(c2c[pat[i - 1]]) : 0u;             // settle(): i > 0
      lf_step_wave(img, sp, ep, comp, has, wave_stage, lane, nsp, nep);
      if(!has) { continue; }
    }
    else
    {
      u32 idx_sp = 0, idx_ep = 0, r_sp = 0, r_ep = 0;
      bool pair = false;
      if(has)
      {
        const u64 at_sp = clampu(sp, img.n), at_ep = clampu(ep + 1, img.n);
        if(force_single == 0 && i >= 2 && e - i + 2 <= min_length)
        {
          const u32 c2 = u32(c2c[pat[i - 1]]) - 1, c1 = u32(c2c[pat[i - 2]]) - 1;      // the first and the second step
          pair = (c1 < 4 && c2 < 4);                             // both are fast characters
          if(pair)
          {
            u32 b_sp, b_ep;
            pair_block_of(at_sp, b_sp, r_sp); pair_block_of(at_ep, b_ep, r_ep);
            const u32 first = (c1 * 4 + c2) * u32(img.flp_nblocks);
            idx_sp = (first + b_sp) | PAIR_FLAG; idx_ep = (first + b_ep) | PAIR_FLAG;
          }
        }
        if(!pair)
        {
          u32 comp = c2c[pat[i - 1]];                            // settle(): i > 0
          if(comp >= u32(img.sigma)) { comp = u32(img.sigma) - 1; }     // memory safety only
          u32 b_sp, b_ep;
          flb_block_of(at_sp, b_sp, r_sp); flb_block_of(at_ep, b_ep, r_ep);
          idx_sp = comp * u32(img.flb_nblocks) + b_sp; idx_ep = comp * u32(img.flb_nblocks) + b_ep;
        }
      }
      PairEnd p_sp = {0, 0, 0}, p_ep = {0, 0, 0};   // a single step keeps (edge, node) in .raw / .node
      const bool need2 = has && idx_ep != idx_sp;
      ulonglong2 blk[8];
      fetch_blocks<true>(img.flb, idx_sp, has, wave_stage, lane, img.flp);
      if(has)
      {
        read_block(wave_stage, lane, blk);
        if(pair)
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
        fetch_blocks<true>(img.flb, idx_ep, need2, wave_stage, lane, img.flp);
        if(need2)
        {
          read_block(wave_stage, lane, blk);
          if(pair) { p_ep = eval_pair(blk, r_ep, true); }
          else { eval_endpoint(blk, r_ep, 1, p_ep.raw, p_ep.node); }
        }
      }
      __builtin_amdgcn_wave_barrier();
      if(!has) { continue; }
      if(pair)
      {
        u64 a = 0, b = 0;
        if(pair_outcome(p_sp, p_ep, idx_ep == idx_sp, a, b) != 2) { force_single = 2; continue; }      // one of them empties: two single steps from the unchanged range
        nsp = p_sp.node; nep = p_ep.node; took = 2;
      }
      else
      {
        force_single -= (force_single > 0 ? 1 : 0);
        const u64 a = p_sp.raw, b = p_ep.raw - 1;              // edge space (gcsa.h:160-161)
        if(range_empty(a, b)) { nsp = a; nep = b; } else { nsp = p_sp.node; nep = p_ep.node; }
      }
    }
    if(range_empty(nsp, nep))
    {
      // the next attempt ends with the character that failed; a first step that failed moves the end by one
      e = (i == e ? e - 1 : i); i = e; sp = 0; ep = root_ep;
      if constexpr(PAIR) { force_single = 0; }
    }
    else
    {
      i -= took; sp = nsp; ep = nep;
      if(e - i >= min_length)
      {
        const u64 cnt = count_range(img, sp, ep);
        if(cnt <= max_count)
        {
          if constexpr(WRITE)
          {
            const u64 at = out_at + n_seeds;
            if(at < out_end)
            {
              ulonglong2* dst = reinterpret_cast<ulonglong2*>(recs + 4 * at);
              dst[0] = make_ulonglong2(i, e - i);
              dst[1] = make_ulonglong2(sp, ep);
              counts[at] = cnt;
            }
          }
          n_seeds++;
          e = i; sp = 0; ep = root_ep;
        }
      }
    }
    steps += took;
    if(steps > limit) { atomicOr(ctl, 1ull); finish(); continue; }
    settle();
  }
}
