// kernels_mem.hpp -- MEM hits (gcsa2_mem_hits_device): the glue between the break records of k_match_stats2 and the two
// locate paths (locate_core for the ranges located in full, locate_max_core for the sampled ones).  Included by
// gcsa2_hip.hip after kernels_locate.hpp (count_range).
//
// Data flow: k_mem_classify (one lane per break record: count(), the gcsa2_mem record, its class) -> one exclusive scan of
// MemScan words (positions in both dense range lists and the count() sum of the full class) -> k_mem_compact (the two
// (sp, ep) lists) -> the locate passes -> k_mem_spread (full class only: its offsets onto the MEMs) or k_mem_sizes + scan +
// k_mem_gather (both classes: the hits in MEM order).
#pragma once

constexpr u64 MEM_SUM_CAP = u64(1) << 62;       // the count() sum saturates here: two operands never overflow
constexpr u64 MEM_CLASS_LOW = 0xFFFFFFFFull;    // MemScan::cls: full class in the low half, sampled class in the high half

struct MemScan
{
  u64 cls;      // MEMs of the full class (bits 0..31) and of the sampled class (bits 32..63)
  u64 sum;      // count() of the full class, saturating at MEM_SUM_CAP: bounds the values locate() gives it
};

struct MemScanOp
{
  __host__ __device__ __forceinline__ MemScan operator()(const MemScan& a, const MemScan& b) const
  {
    const u64 s = a.sum + b.sum;
    return MemScan{a.cls + b.cls, s < MEM_SUM_CAP ? s : MEM_SUM_CAP};
  }
};

// One lane per break record {position, length, sp, ep}; lane m writes the scan's closing zero.  The record becomes a
// gcsa2_mem {position, length, sp, ep, count}; the class: count 0 -> none, hit_max 0 or count <= hit_max -> full,
// otherwise sampled (sample != 0) or none.  A random 2-rank + 2-select gather per lane, like k_count; `known` (sub-MEMs, whose
// walk computed every count) replaces the gather with counts[i].
__global__ __launch_bounds__(TPB) void k_mem_classify(DevImage img, const u64* __restrict__ breaks, const u64* __restrict__ known, u64 m,
                                                      u64 hit_max, int sample, u64* __restrict__ mems, MemScan* __restrict__ words)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  if(i > m) { return; }
  if(i == m) { words[m] = MemScan{0, 0}; return; }
  const ulonglong2* src = reinterpret_cast<const ulonglong2*>(breaks + 4 * i);
  const ulonglong2 a = src[0], b = src[1];
  const u64 count = (known != nullptr ? known[i] : count_range(img, b.x, b.y));
  u64* dst = mems + 5 * i;
  dst[0] = a.x; dst[1] = a.y; dst[2] = b.x; dst[3] = b.y; dst[4] = count;
  MemScan w{0, 0};
  if(count != 0)
  {
    if(hit_max == 0 || count <= hit_max) { w.cls = 1; w.sum = (count < MEM_SUM_CAP ? count : MEM_SUM_CAP); }
    else if(sample) { w.cls = u64(1) << 32; }
  }
  words[i] = w;
}

// The dense (sp, ep) lists of both classes, in MEM order, from the exclusive scan `pos` (m + 1 entries).
__global__ __launch_bounds__(TPB) void k_mem_compact(const u64* __restrict__ mems, u64 m, const MemScan* __restrict__ pos,
                                                     u64* __restrict__ full, u64* __restrict__ sampled)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  if(i >= m) { return; }
  const u64 here = pos[i].cls, next = pos[i + 1].cls;
  if(here == next) { return; }
  const ulonglong2 r = make_ulonglong2(mems[5 * i + 2], mems[5 * i + 3]);
  if((next & MEM_CLASS_LOW) != (here & MEM_CLASS_LOW)) { reinterpret_cast<ulonglong2*>(full)[here & MEM_CLASS_LOW] = r; }
  else { reinterpret_cast<ulonglong2*>(sampled)[here >> 32] = r; }
}

// Full class only: MEM i's hits start where the full list's entry for it (or the next one) starts.  i = 0 .. m.
__global__ __launch_bounds__(TPB) void k_mem_spread(const MemScan* __restrict__ pos, u64 m, const u64* __restrict__ full_offsets,
                                                    u64* __restrict__ hit_offsets)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  if(i <= m) { hit_offsets[i] = full_offsets[pos[i].cls & MEM_CLASS_LOW]; }
}

// Both classes: the number of hits of every MEM (0 for entry m), to be scanned into the hit offsets.
__global__ __launch_bounds__(TPB) void k_mem_sizes(const MemScan* __restrict__ pos, u64 m, const u64* __restrict__ full_offsets,
                                                   const u64* __restrict__ sampled_offsets, u64* __restrict__ sizes)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  if(i > m) { return; }
  u64 size = 0;
  if(i < m)
  {
    const u64 here = pos[i].cls, next = pos[i + 1].cls;
    const u64 f = here & MEM_CLASS_LOW, s = here >> 32;
    if((next & MEM_CLASS_LOW) != f) { size = full_offsets[f + 1] - full_offsets[f]; }
    else if(next != here) { size = sampled_offsets[s + 1] - sampled_offsets[s]; }
  }
  sizes[i] = size;
}

// Both classes: one lane per hit.  The workgroup finds the MEMs of its first and last hit, each lane then the MEM of its own
// hit inside that window (the last i with hit_offsets[i] <= j), and copies the value from the class's list.
__global__ __launch_bounds__(TPB) void k_mem_gather(const MemScan* __restrict__ pos, u64 m, const u64* __restrict__ hit_offsets, u64 total,
                                                    const u64* __restrict__ full_offsets, const u64* __restrict__ full_values,
                                                    const u64* __restrict__ sampled_offsets, const u64* __restrict__ sampled_values,
                                                    u64* __restrict__ hits)
{
  __shared__ u64 window[2];
  const u64 first = u64(blockIdx.x) * TPB;
  auto owner = [&](u64 j, u64 lo, u64 hi) -> u64     // last i in [lo, hi] with hit_offsets[i] <= j (hit_offsets[lo] <= j)
  {
    while(lo < hi)
    {
      const u64 mid = lo + (hi - lo + 1) / 2;
      if(hit_offsets[mid] <= j) { lo = mid; } else { hi = mid - 1; }
    }
    return lo;
  };
  if(threadIdx.x < 2)
  {
    const u64 last = (first + TPB - 1 < total ? first + TPB - 1 : total - 1);
    window[threadIdx.x] = owner(threadIdx.x == 0 ? first : last, 0, m - 1);
  }
  __syncthreads();
  const u64 j = first + threadIdx.x;
  if(j >= total) { return; }
  const u64 i = owner(j, window[0], window[1]);
  const u64 k = j - hit_offsets[i];
  const u64 here = pos[i].cls, next = pos[i + 1].cls;
  const u64 f = here & MEM_CLASS_LOW, s = here >> 32;
  hits[j] = ((next & MEM_CLASS_LOW) != f) ? full_values[full_offsets[f] + k] : sampled_values[sampled_offsets[s] + k];
}
