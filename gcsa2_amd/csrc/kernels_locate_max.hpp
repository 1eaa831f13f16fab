// kernels_locate_max.hpp -- batched GCSA::locate(range, max_positions, results) (src/gcsa.cpp:844-878).
// Part of the single translation unit gcsa2_hip.hip (device code, anonymous namespace).
//
// One wavefront (the whole workgroup) per range, the reference's std::mt19937_64(sp ^ ep) in LDS (mt64.hpp):
//   count(range) <= 0 or max_positions == 0: nothing (the slot is empty; the kernel does not look at the range).
//   m >= count / 2: every path node of the range is located, 64 at a time, into LDS; bitonic sort + unique there.
//   otherwise:      64 draws at a time (never across a twist), one lane each locates its node; the values are inserted in
//                   draw order into an LDS set (a wave-wide membership scan per value) and the first draw after which the
//                   set holds m values ends the loop: the generator's position moves by that draw count only, so the
//                   speculative draws behind it never reach the shuffle.  At most 64 m + 64 draws (an index whose count()
//                   overstates its distinct values would make the reference spin): LMAX_FLAG_DRAWS.
//   n > m values:   deterministicShuffle (utils.h:359-370): the indices rng() % i, i = n .. 1, by 64 lanes at a time,
//                   then the chain of swaps on one lane; the first m are sorted again.
// A range with fewer distinct values than min(max_positions, count) -- count() overstating them, which the reference allows
// -- writes what it has and its size to sizes[q]; the host then closes the gaps (the reference returns those values).
// LDS budget: m <= LMAX_MOST and at most LMAX_SET values (raw, before unique, in the first branch).  A range beyond it is
// listed in `fallback` and the host runs it through the per-range path (locate_max_bounded in gcsa2_hip.hip).
#pragma once

#include "kernels_locate.hpp"
#include "mt64.hpp"

using namespace g2;

namespace {

constexpr u32 LMAX_MOST = 1024;            // largest max_positions (after the clamp to count) on the device path
constexpr u32 LMAX_SET = 2048;             // values a range may hold in LDS (a power of two: the sort pads to one)
constexpr u32 LMAX_FLAG_DRAWS = 1;         // a range drew 64 m + 64 positions without finding m distinct values
constexpr u32 LMAX_FLAG_SIZE = 2;          // a range has fewer distinct values than its slot (sizes[q]: how many)
constexpr u32 LMAX_FLAG_SLOT = 4;          // a range's count differs from the one its slot was sized with

struct LocateMaxShared
{
  u64 mt[mt64::N];                         // 2.5 KB
  u64 vals[LMAX_SET];                      // 16 KB
  unsigned short idx[LMAX_SET];            // 4 KB: the shuffle's rng() % i
  u64 C[MAX_SIGMA + 1];
};

// locateInternal(node) (gcsa.cpp:880-896) of one lane: the locate table's entry when there is one (k_locate_tab's
// decoding: a LOCATE_DIRECT entry is the single value, any other the first sample and the walk's length), else the walk.
struct NodeValues { u64 s, steps, direct; u32 cnt; u32 is_direct; };

__device__ __forceinline__ NodeValues node_values(const DevImage& img, const u64* C, u64 node)
{
  NodeValues r{0, 0, 0, 1, 0};
  if(img.locate_tab != nullptr)
  {
    const u64 entry = img.locate_tab[node];
    if(entry & LOCATE_DIRECT) { r.direct = entry & ~LOCATE_DIRECT; r.is_direct = 1; return r; }
    r.s = entry & ((u64(1) << LOCATE_INDEX_BITS) - 1); r.steps = entry >> LOCATE_INDEX_BITS;
  }
  else
  {
    u64 srank;
    while(!bv_get_rank(img.sampled, node, srank)) { node = lf_node(img, C, node); r.steps++; }   // gcsa.cpp:883-887
    r.s = (srank > 0 ? bv_select(img.samples, srank) + 1 : 0);                                    // firstSample, gcsa.h:202-206
  }
  r.cnt = sample_run(img, r.s);
  return r;
}

__device__ __forceinline__ u64 node_value(const DevImage& img, const NodeValues& r, u32 j)
{
  return r.is_direct ? r.direct : packed_get(img.stored, img.sample_width, r.s + j) + r.steps;   // gcsa.cpp:893
}

// Ascending bitonic sort of v[0, n) in LDS by one wavefront; v[n, P) (P = the next power of two) is overwritten.
__device__ void lmax_sort(u64* v, u32 n, u32 lane)
{
  if(n <= 1) { return; }
  u32 P = 2;
  while(P < n) { P <<= 1; }
  for(u32 i = n + lane; i < P; i += 64) { v[i] = ~u64(0); }
  __syncthreads();
  for(u32 k = 2; k <= P; k <<= 1)
  {
    for(u32 j = k >> 1; j > 0; j >>= 1)
    {
      for(u32 p = lane; p < P / 2; p += 64)
      {
        const u32 i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i + j;
        const u64 a = v[i], b = v[l];
        if((a > b) == ((i & k) == 0)) { v[i] = b; v[l] = a; }
      }
      __syncthreads();
    }
  }
}

// Removes the duplicates of the sorted v[0, n) in place; returns the number of distinct values.
__device__ u32 lmax_unique(u64* v, u32 n, u32 lane)
{
  u32 out = 0;
  u64 last = 0;                                  // the previous chunk's last value
  for(u32 b = 0; b < n; b += 64)
  {
    const u32 i = b + lane;
    const bool live = i < n;
    const u64 x = live ? v[i] : 0;
    u64 prev = __shfl_up(x, 1);
    if(lane == 0) { prev = last; }
    const bool keep = live && (i == 0 || x != prev);
    const u64 mask = __ballot(keep);
    last = __shfl(x, 63);
    __syncthreads();                             // the chunk is read before any of it is overwritten
    if(keep) { v[out + u32(__popcll(mask & ((u64(1) << lane) - 1)))] = x; }
    out += u32(__popcll(mask));
    __syncthreads();
  }
  return out;
}

__device__ void lmax_seed(u64* x, u64 seed, u32 lane)
{
  if(lane == 0) { mt64::seed(x, seed); }
  __syncthreads();
}

// The three-phase twist of mt64.hpp on one wavefront.
__device__ void lmax_twist(u64* x, u32 lane)
{
  for(int p = 0; p < 3; p++)
  {
    const int end = mt64::phase_begin(p + 1);
    for(int b = mt64::phase_begin(p); b < end; b += 64)
    {
      const int k = b + int(lane);
      const u64 v = (k < end ? mt64::twist_word_at(x, k) : 0);
      __syncthreads();
      if(k < end) { x[k] = v; }
      __syncthreads();
    }
  }
}

// The next c = min(want, 64, 312 - pos) outputs (after a twist when the block is used up): lane j < c gets output pos + j.
// The caller moves pos by the number of outputs it consumes.
__device__ u32 lmax_draw(u64* x, u32& pos, u64 want, u32 lane, u64& r)
{
  if(pos >= u32(mt64::N)) { lmax_twist(x, lane); pos = 0; }
  u64 c = u64(mt64::N) - pos;
  if(c > 64) { c = 64; }
  if(c > want) { c = want; }
  r = (lane < c ? mt64::temper(x[pos + lane]) : 0);
  return u32(c);
}

// A count() of 2^40 or more is no count of values: it is what count() gives when it wraps below zero, which the counters
// allow for some ranges of some graphs.  Such a range gets no slot from the sizes pass (the slots' sum would wrap); it is
// listed in `odd`, the host answers it by the per-range path and gives it a slot of its real size before the scan.  With
// every other slot below 2^40 and fewer than LMAX_BATCH ranges, the scan cannot wrap.
constexpr u64 LMAX_COUNT_LIMIT = u64(1) << 40;
constexpr u64 LMAX_BATCH = u64(1) << 24;

// sizes[q] = min(max_positions, count(range q)); sizes[nq] = 0 (the exclusive scan's total).  ctl[3]: ranges listed in `odd`.
__global__ __launch_bounds__(TPB) void k_locate_max_sizes(DevImage img, const u64* __restrict__ ranges, u64 nq, u64 max_positions,
                                                          u64* __restrict__ sizes, unsigned long long* __restrict__ ctl,
                                                          u64* __restrict__ odd)
{
  const u64 q = u64(blockIdx.x) * TPB + threadIdx.x;
  if(q > nq) { return; }
  if(q == nq) { sizes[q] = 0; return; }
  const u64 total = count_range(img, ranges[2 * q], ranges[2 * q + 1]);
  if(total >= LMAX_COUNT_LIMIT) { sizes[q] = 0; odd[atomicAdd(&ctl[3], 1ull)] = q; return; }
  sizes[q] = (max_positions < total ? max_positions : total);
}

// ctl[0]: LMAX_FLAG_* bits; ctl[1]: ranges listed in `fallback`; ctl[2]: the first range that set a flag.
__global__ __launch_bounds__(64) void k_locate_max(DevImage img, const u64* __restrict__ ranges, u64 nq, u64 max_positions,
                                                   const u64* __restrict__ offsets, u64* __restrict__ values,
                                                   unsigned long long* __restrict__ ctl, u64* __restrict__ fallback,
                                                   u64* __restrict__ sizes)
{
  __shared__ LocateMaxShared sh;
  const u32 lane = threadIdx.x;
  if(lane <= u32(MAX_SIGMA)) { sh.C[lane] = img.C[lane]; }
  __syncthreads();
  for(u64 q = blockIdx.x; q < nq; q += gridDim.x)
  {
    const u64 out = offsets[q], slot = offsets[q + 1] - out;
    if(slot == 0) { continue; }                                  // count 0 or max_positions 0 (gcsa.cpp:849)
    const u64 sp = ranges[2 * q], ep = ranges[2 * q + 1];
    const u64 total = count_range(img, sp, ep);
    if(total >= LMAX_COUNT_LIMIT) { continue; }                 // answered on the host (k_locate_max_sizes)
    const u64 m = (max_positions < total ? max_positions : total);
    if(m != slot) { if(lane == 0) { atomicOr(&ctl[0], (unsigned long long)LMAX_FLAG_SLOT); atomicMin(&ctl[2], (unsigned long long)q); } continue; }
    if(m > LMAX_MOST) { if(lane == 0) { fallback[atomicAdd(&ctl[1], 1ull)] = q; } continue; }
    u32 n = 0, pos = 0;
    bool seeded = false, over = false;
    if(m >= total / 2)                                           // locate everything (gcsa.cpp:855-858)
    {
      for(u64 b = sp; b <= ep; b += 64)
      {
        const u64 node = b + lane;
        NodeValues r{0, 0, 0, 0, 0};
        if(node <= ep) { r = node_values(img, sh.C, node); }
        u64 incl = r.cnt;                                        // inclusive scan of the value counts over the wave
#pragma unroll
        for(u32 d = 1; d < 64; d <<= 1)
        {
          const u64 o = __shfl_up(incl, d);
          if(lane >= d) { incl += o; }
        }
        const u64 sum = __shfl(incl, 63);
        if(n + sum > LMAX_SET) { over = true; break; }
        for(u32 j = 0; j < r.cnt; j++) { sh.vals[n + u32(incl) - r.cnt + j] = node_value(img, r, j); }
        n += u32(sum);
      }
      if(over) { if(lane == 0) { fallback[atomicAdd(&ctl[1], 1ull)] = q; } __syncthreads(); continue; }
      __syncthreads();
      lmax_sort(sh.vals, n, lane);
      n = lmax_unique(sh.vals, n, lane);
      if(n < m)                                                  // count() overstates the range's values: the reference
      {                                                          // returns them all, fewer than the slot holds
        for(u32 i = lane; i < n; i += 64) { values[out + i] = sh.vals[i]; }
        if(lane == 0) { sizes[q] = n; atomicOr(&ctl[0], (unsigned long long)LMAX_FLAG_SIZE); }
        __syncthreads();
        continue;
      }
    }
    else                                                         // random positions (gcsa.cpp:859-871)
    {
      lmax_seed(sh.mt, sp ^ ep, lane);
      pos = u32(mt64::N); seeded = true;
      const u64 len = ep + 1 - sp, most = 64 * m + 64;
      u64 draws = 0;
      bool stuck = false;
      while(n < m)
      {
        if(draws >= most) { stuck = true; break; }
        u64 r;
        const u32 c = lmax_draw(sh.mt, pos, most - draws, lane, r);
        NodeValues mine{0, 0, 0, 0, 0};
        if(lane < c) { mine = node_values(img, sh.C, sp + r % len); }
        u32 used = c;
        for(u32 j = 0; j < c && !over; j++)                      // draw order
        {
          NodeValues w;
          w.s = __shfl(mine.s, int(j)); w.steps = __shfl(mine.steps, int(j)); w.direct = __shfl(mine.direct, int(j));
          w.cnt = __shfl(mine.cnt, int(j)); w.is_direct = __shfl(mine.is_direct, int(j));
          for(u32 t = 0; t < w.cnt; t++)
          {
            const u64 v = node_value(img, w, t);
            bool found = false;
            for(u32 i = lane; i < n; i += 64) { found = found || sh.vals[i] == v; }
            if(!__any(found))
            {
              if(n >= LMAX_SET) { over = true; break; }
              if(lane == 0) { sh.vals[n] = v; }
              n++;
            }
            __syncthreads();
          }
          if(!over && n >= m) { used = j + 1; break; }
        }
        if(over) { break; }
        pos += used; draws += used;                              // the draws behind the deciding one are given back
      }
      if(over) { if(lane == 0) { fallback[atomicAdd(&ctl[1], 1ull)] = q; } __syncthreads(); continue; }
      if(stuck) { if(lane == 0) { atomicOr(&ctl[0], (unsigned long long)LMAX_FLAG_DRAWS); atomicMin(&ctl[2], (unsigned long long)q); } __syncthreads(); continue; }
      lmax_sort(sh.vals, n, lane);
    }
    if(n > m)                                                    // deterministicShuffle + resize (gcsa.cpp:873-877)
    {
      if(!seeded) { lmax_seed(sh.mt, sp ^ ep, lane); pos = u32(mt64::N); }
      for(u32 t = 0; t < n; )
      {
        u64 r;
        const u32 c = lmax_draw(sh.mt, pos, n - t, lane, r);
        if(lane < c) { sh.idx[t + lane] = (unsigned short)(r % u64(n - t - lane)); }
        pos += c; t += c;
      }
      __syncthreads();
      if(lane == 0)
      {
        for(u32 t = 0; t < n; t++)
        {
          const u32 i = n - t, o = sh.idx[t];
          const u64 a = sh.vals[i - 1];
          sh.vals[i - 1] = sh.vals[o]; sh.vals[o] = a;
        }
      }
      __syncthreads();
      lmax_sort(sh.vals, u32(m), lane);
    }
    for(u32 i = lane; i < m; i += 64) { values[out + i] = sh.vals[i]; }
    __syncthreads();                                             // LDS is the next range's
  }
}

}  // namespace
