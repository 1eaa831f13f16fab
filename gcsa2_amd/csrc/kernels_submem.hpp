// kernels_submem.hpp -- sub-MEM reseeding (gcsa2_sub_mem_hits_device): inside every MEM of at least reseed_length bases, the
// shorter matches that occur more often than the MEM itself.  Included by gcsa2_hip.hip after kernels_lcp.hpp (lcp_parent),
// kernels_locate.hpp (count_range) and kernels_find.hpp (lf_step_wave).
//
// Data flow: k_submem_prep (one lane per MEM: its pattern from the MEM offsets, the bounds check, whether it is reseeded) ->
// hipcub select (the list of reseeded MEMs) -> k_submem_walk<false> (sub-MEMs per MEM) -> exclusive scan (the CSR offsets) ->
// k_submem_walk<true> (the same walk again, records written at their CSR slots) -> the classify / locate / gather tail of
// mem_hits (kernels_mem.hpp), fed the counts the walk computed.
//
// The walk of one MEM {b, l, c} (E = b + l; the contract is in include/gcsa2_hip.h): the LF + parent() interplay of
// k_match_stats2 restricted to [b, E), where a step also fails when count() of the new range is <= c.
//   x = e = E, r = root;  while e >= b + min_length:
//     if x > b and LF(r, P[x - 1]) is non-empty with count > c: x -= 1, take it
//     else: emit [x, e) if e - x >= min_length and x < last_x;  stop at x == b;  x == e: e -= 1, restart at the root;
//           otherwise r = parent(r), e = x + its lcp
// Two passes of the same deterministic walk -- count, then write at the scanned offsets -- rather than per-wave slot blocks
// and a scatter: the sub-MEMs of a batch have no useful bound to size record scratch from ahead of time.
#pragma once

constexpr u64 SUBMEM_NOT_RESEEDED = ~u64(0);    // pid entry of a MEM that is not walked
constexpr u32 SUBMEM_REFILL_AT = 8;             // idle lanes of a wave that make it draw new MEMs

// Control words of one call (zeroed by the host): [0] a MEM lies beyond its pattern, [1] a walk overran its round bound,
// [2] reseeded MEMs (the select's output), [3] the work counter of the persistent lanes.
constexpr u32 SUBMEM_CTL_WORDS = 4;

// One lane per MEM k: its pattern q (the last q < nq with mem_offsets[q] <= k), the check position + length <= |P_q|, and
// flag[k] = (length >= reseed_length).  pid[k] = q, or SUBMEM_NOT_RESEEDED.
__global__ __launch_bounds__(TPB) void k_submem_prep(const u64* __restrict__ offsets, u64 nq, const u64* __restrict__ mem_offsets,
                                                     const u64* __restrict__ mems, u64 n_mems, u64 reseed_length,
                                                     u64* __restrict__ pid, u8* __restrict__ flag, unsigned long long* __restrict__ ctl)
{
  const u64 k = u64(blockIdx.x) * TPB + threadIdx.x;
  if(k >= n_mems) { return; }
  u64 lo = 0, hi = nq - 1;
  while(lo < hi)
  {
    const u64 mid = lo + (hi - lo + 1) / 2;
    if(mem_offsets[mid] <= k) { lo = mid; } else { hi = mid - 1; }
  }
  const u64 position = mems[5 * k], length = mems[5 * k + 1];
  const u64 size = offsets[lo + 1] - offsets[lo];
  const bool inside = mem_offsets[lo] <= k && position <= size && length <= size - position;
  if(!inside) { atomicOr(ctl, 1ull); }
  const bool walk = inside && length >= reseed_length;
  pid[k] = walk ? lo : SUBMEM_NOT_RESEEDED;
  flag[k] = walk ? 1 : 0;
}

// The walk, one lane per reseeded MEM; persistent lanes draw MEMs from work[0 .. nr) through ctl[3].  Every lane of a wave
// calls lf_step_wave in every round (the block fetch is wave-cooperative); a lane then takes count_range of the new range and,
// on failure, lcp_parent.  WRITE = false: sizes[k] = the sub-MEMs of MEM k.  WRITE = true: record j of MEM k at
// sub_offsets[k] + j, as {position, length, sp, ep} into recs and its count into counts (never beyond sub_offsets[k + 1]).
// A walk that exceeds 2 l + 2 rounds, or a parent() whose lcp does not shorten the match, sets ctl[1] and ends.
template<bool WRITE>
__global__ __launch_bounds__(TPB2) void k_submem_walk(DevImage img, const u8* __restrict__ patterns, const u64* __restrict__ offsets,
                                                      const u64* __restrict__ mems, const u64* __restrict__ pid, const u32* __restrict__ work,
                                                      u64 nr, u64 min_length, unsigned long long* __restrict__ ctl, u64* __restrict__ sizes,
                                                      const u64* __restrict__ sub_offsets, u64* __restrict__ recs, u64* __restrict__ counts)
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
  u64 k = 0, b = 0, c = 0, x = 0, e = 0, sp = 0, ep = 0, cnt = 0, last_x = 0, rounds = 0, limit = 0, n_sub = 0, out_at = 0, out_end = 0;
  const u8* pat = nullptr;
  auto finish = [&]()
  {
    if constexpr(!WRITE) { sizes[k] = n_sub; }
    has = false;
  };
  auto start = [&](u64 item)
  {
    k = work[item];
    b = mems[5 * k];
    const u64 length = mems[5 * k + 1];
    c = mems[5 * k + 4];
    pat = patterns + offsets[pid[k]];
    x = e = b + length;
    sp = 0; ep = root_ep; cnt = 0;
    last_x = ~u64(0); rounds = 0; limit = 2 * length + 2; n_sub = 0;
    if constexpr(WRITE) { out_at = sub_offsets[k]; out_end = sub_offsets[k + 1]; }
    has = true;
    if(length < min_length) { finish(); }
  };
  while(true)
  {
    const u64 idle = __ballot(!has);
    if(!exhausted && (u32(__popcll(idle)) >= SUBMEM_REFILL_AT || idle == ~u64(0)))
    {
      const u32 want = u32(__popcll(idle)), leader = u32(__ffsll((long long)idle)) - 1;
      unsigned long long base = 0;
      if(lane == leader) { base = atomicAdd(ctl + 3, (unsigned long long)want); }
      base = __shfl(base, leader, 64);
      if(!has)
      {
        const u64 mine = base + __popcll(idle & ((u64(1) << lane) - 1));
        if(mine < nr) { start(mine); }
      }
      exhausted = (base + want >= nr);
    }
    if(!__any(has))
    {
      if(exhausted) { break; }
      continue;
    }
    const bool stepping = has && x > b;
    const u32 comp = stepping ? u32(c2c[pat[x - 1]]) : 0u;
    u64 nsp = 0, nep = 0;
    lf_step_wave(img, sp, ep, comp, stepping, wave_stage, lane, nsp, nep);
    if(!has) { continue; }
    bool extended = false;
    if(stepping && !range_empty(nsp, nep))
    {
      const u64 ncnt = count_range(img, nsp, nep);
      if(ncnt > c) { x--; sp = nsp; ep = nep; cnt = ncnt; extended = true; }
    }
    if(!extended)
    {
      // the match ending at e cannot be extended: the candidate [x, e)
      if(e - x >= min_length && x < last_x)
      {
        if constexpr(WRITE)
        {
          const u64 at = out_at + n_sub;
          if(at < out_end)
          {
            ulonglong2* dst = reinterpret_cast<ulonglong2*>(recs + 4 * at);
            dst[0] = make_ulonglong2(x, e - x);
            dst[1] = make_ulonglong2(sp, ep);
            counts[at] = cnt;
          }
        }
        n_sub++;
        last_x = x;
      }
      if(x == b) { finish(); continue; }
      if(e == x) { e--; x = e; sp = 0; ep = root_ep; cnt = 0; }
      else
      {
        gcsa2_stnode node;
        lcp_parent(img, sp, ep, node);
        if(node.node_lcp >= e - x) { atomicOr(ctl + 1, 1ull); finish(); continue; }      // parent() must shorten the match
        e = x + node.node_lcp; sp = node.sp; ep = node.ep;
      }
    }
    if(e < b + min_length) { finish(); continue; }
    if(++rounds > limit) { atomicOr(ctl + 1, 1ull); finish(); }
  }
}
