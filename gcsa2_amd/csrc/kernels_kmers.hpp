// kernels_kmers.hpp -- the search tree of countKMers (src/algorithms.cpp:364-421) on the device: level-synchronous from the
// root range, comps 1..limit per state, empty children dropped.  Every index-side k-mer call walks it (the host side is
// kmer_walk in host_kmers.hpp):
//   gcsa2_count_kmers                         k_kmer_expand per level; the last level only counts
//   gcsa2_compare_kmers[_records]             k_kmer_compare: the same tree over pairs of ranges, one per index
//   gcsa2_kmer_spectrum, gcsa2_list_kmers,    k_kmer_expand per level above the last (with the keys of the children for the
//   gcsa2_index_kmer_support_device           list) -> k_spectrum_leaf on the parents at depth k - 1: the children are expanded
//                                             in registers and never stored as states; a value per k-mer -- count(range) or
//                                             Range::length(range) -- is summed, binned, listed or handed on as seed records
// Included by gcsa2_hip.hip after kernels_locate.hpp (count_range, wg_reserve) and kernels_support.hpp (wave_sum).
#pragma once

namespace {

constexpr int KMER_CHUNK = 4;       // comps per batch of independent block loads (the fast characters)

// KMerComparisonState::set (algorithms.cpp:451-457): comp of extension step i at bits [3i, 3i + 3).
// (The reference also evaluates `comp >> (64 - bit)` for bit == 0, a shift by the word size; the intended
// "|= 0 unless the comp straddles two words" is what is restated here.)
__device__ __forceinline__ void kmer_set(u64* kmer, u32 i, u64 comp)
{
  u32 offset = (i * 3) >> 6, bit = (i * 3) & 63;
  kmer[offset] |= comp << bit;
  if(bit > 61) { kmer[offset + 1] |= comp >> (64 - bit); }
}

// ---- countKMers frontier expansion (src/algorithms.cpp:364-421) -------------------------------
// One lane per search state (a non-empty range at depth d): its children are LF_fast / LF_all of
// the range (src/gcsa.cpp:742-798) for comps 1..limit; non-empty children are appended to `out`
// (wave-aggregated atomic slot allocation) as long as their slot lies below `capacity`; *counter counts
// them all.  capacity == 0 with null outputs only counts (the last level of gcsa2_count_kmers).
// KEYS: the keys of the children travel with them: the comp of extension step `depth` at bits
// [3 depth, 3 depth + 3) of the parent's key (kmer_set; the packing of gcsa2_compare_kmers_records).
template<bool KEYS>
__global__ __launch_bounds__(TPB) void k_kmer_expand(DevImage img, const u64* __restrict__ in, const u64* __restrict__ in_keys, u64 n_in, u32 limit,
                                                     u32 depth, u64* __restrict__ out, u64* __restrict__ out_keys, u64 capacity,
                                                     unsigned long long* __restrict__ counter)
{
  __shared__ WgSlots slots;
  const u64 q = u64(blockIdx.x) * TPB + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const u64 below = (u64(1) << lane) - 1;
  const bool live = q < n_in;
  const ulonglong2 r = live ? reinterpret_cast<const ulonglong2*>(in)[q] : make_ulonglong2(1, 0);
  u64 key[3] = {0, 0, 0};
  if(KEYS && live) { key[0] = in_keys[3 * q]; key[1] = in_keys[3 * q + 1]; key[2] = in_keys[3 * q + 2]; }
  for(u32 c0 = 1; c0 <= limit; c0 += KMER_CHUNK)
  {
    u64 csp[KMER_CHUNK], cep[KMER_CHUNK], mask[KMER_CHUNK];
    lf_children<KMER_CHUNK>(img, c0, limit, live, r.x, r.y, csp, cep);
    u32 wave_count = 0;
#pragma unroll
    for(int j = 0; j < KMER_CHUNK; j++)
    {
      mask[j] = __ballot(live && c0 + u32(j) <= limit && !range_empty(csp[j], cep[j]));
      wave_count += u32(__popcll(mask[j]));
    }
    u64 slot = wg_reserve(slots, counter, wave_count);
#pragma unroll
    for(int j = 0; j < KMER_CHUNK; j++)
    {
      const u64 at = slot + __popcll(mask[j] & below);
      if(((mask[j] >> lane) & 1) && at < capacity)        // (the host sizes `out` for limit children per state: always true there)
      {
        reinterpret_cast<ulonglong2*>(out)[at] = make_ulonglong2(csp[j], cep[j]);
        if(KEYS)
        {
          u64 child[3] = {key[0], key[1], key[2]};
          kmer_set(child, depth, c0 + u32(j));
          out_keys[3 * at] = child[0]; out_keys[3 * at + 1] = child[1]; out_keys[3 * at + 2] = child[2];
        }
      }
      slot += __popcll(mask[j]);
    }
  }
}

// ---- compareKMers frontier expansion (src/algorithms.cpp:505-616) ------------------------------
// A state is a pair of ranges, one per index; a child survives if it is non-empty in at least one
// index.  The two images are read through pointers (two DevImage values would not fit the 4 KB
// kernel-argument segment).
// mode 0: expand (children appended to out / out_keys, counters[0] = number of children)
// mode 1: classify the children: counters[1] += shared, counters[2] += left only, counters[3] += right only
// mode 2: like 1, and the left-only / right-only children are written as 8-u64 KMerComparisonState
//         records (left range, right range, k, kmer[3]) to left_records / right_records
__global__ __launch_bounds__(TPB) void k_kmer_compare(const DevImage* __restrict__ left, const DevImage* __restrict__ right,
                                                      const u64* __restrict__ in, const u64* __restrict__ in_keys, u64 n_in,
                                                      u32 limit, u32 depth, int mode,
                                                      u64* __restrict__ out, u64* __restrict__ out_keys,
                                                      unsigned long long* __restrict__ counters,
                                                      u64* __restrict__ left_records, u64* __restrict__ right_records)
{
  __shared__ WgSlots slots;
  u64 q = u64(blockIdx.x) * TPB + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const u64 below = (u64(1) << lane) - 1;
  bool live = q < n_in;
  ulonglong2 l = make_ulonglong2(1, 0), r = make_ulonglong2(1, 0);
  u64 key[3] = {0, 0, 0};
  if(live)
  {
    l = reinterpret_cast<const ulonglong2*>(in)[2 * q]; r = reinterpret_cast<const ulonglong2*>(in)[2 * q + 1];
    if(in_keys != nullptr) { key[0] = in_keys[3 * q]; key[1] = in_keys[3 * q + 1]; key[2] = in_keys[3 * q + 2]; }
  }
  unsigned long long shared_total = 0;          // mode 1 / 2: k-mers in both indexes, per wave
  for(u32 c0 = 1; c0 <= limit; c0 += KMER_CHUNK)
  {
    u64 lcsp[KMER_CHUNK], lcep[KMER_CHUNK], rcsp[KMER_CHUNK], rcep[KMER_CHUNK];
    lf_children<KMER_CHUNK>(*left, c0, limit, live, l.x, l.y, lcsp, lcep);
    lf_children<KMER_CHUNK>(*right, c0, limit, live, r.x, r.y, rcsp, rcep);
    u64 lmask[KMER_CHUNK], rmask[KMER_CHUNK];      // children that are non-empty on the left / right
    u32 any_count = 0, lonly_count = 0, ronly_count = 0;
#pragma unroll
    for(int j = 0; j < KMER_CHUNK; j++)
    {
      const bool active = live && c0 + u32(j) <= limit;
      lmask[j] = __ballot(active && !range_empty(lcsp[j], lcep[j]));
      rmask[j] = __ballot(active && !range_empty(rcsp[j], rcep[j]));
      any_count += u32(__popcll(lmask[j] | rmask[j]));
      lonly_count += u32(__popcll(lmask[j] & ~rmask[j]));
      ronly_count += u32(__popcll(rmask[j] & ~lmask[j]));
      shared_total += (unsigned long long)__popcll(lmask[j] & rmask[j]);
    }
    if(mode == 0)
    {
      u64 slot = wg_reserve(slots, counters, any_count);
#pragma unroll
      for(int j = 0; j < KMER_CHUNK; j++)
      {
        const u64 mask = lmask[j] | rmask[j];
        if(out != nullptr && ((mask >> lane) & 1))
        {
          const u64 at = slot + __popcll(mask & below);
          reinterpret_cast<ulonglong2*>(out)[2 * at] = make_ulonglong2(lcsp[j], lcep[j]);
          reinterpret_cast<ulonglong2*>(out)[2 * at + 1] = make_ulonglong2(rcsp[j], rcep[j]);
          if(out_keys != nullptr)
          {
            u64 child[3] = {key[0], key[1], key[2]};
            kmer_set(child, depth, c0 + u32(j));
            out_keys[3 * at] = child[0]; out_keys[3 * at + 1] = child[1]; out_keys[3 * at + 2] = child[2];
          }
        }
        slot += __popcll(mask);
      }
      continue;
    }
    u64 lslot = wg_reserve(slots, counters + 2, lonly_count);
    u64 rslot = wg_reserve(slots, counters + 3, ronly_count);
    if(mode == 2)
    {
#pragma unroll
      for(int j = 0; j < KMER_CHUNK; j++)
      {
        const u64 lonly = lmask[j] & ~rmask[j], ronly = rmask[j] & ~lmask[j];
        const bool mine_left = (lonly >> lane) & 1, mine_right = (ronly >> lane) & 1;
        if(mine_left || mine_right)
        {
          u64 child[3] = {key[0], key[1], key[2]};
          kmer_set(child, depth, c0 + u32(j));
          u64* rec = (mine_left ? left_records + 8 * (lslot + __popcll(lonly & below)) : right_records + 8 * (rslot + __popcll(ronly & below)));
          rec[0] = lcsp[j]; rec[1] = lcep[j]; rec[2] = rcsp[j]; rec[3] = rcep[j]; rec[4] = u64(depth) + 1;
          rec[5] = child[0]; rec[6] = child[1]; rec[7] = child[2];
        }
        lslot += __popcll(lonly); rslot += __popcll(ronly);
      }
    }
  }
  if(mode != 0) { wg_reserve(slots, counters + 1, u32(shared_total)); }
}

// ---- the index k-mer spectrum: the last level of the tree with a value per k-mer ----------------

// device counters of one walk (SPEC_CURSOR: the slots of the level that runs, cleared by the host before every launch)
enum : u32 { SPEC_KMERS = 0, SPEC_NODES = 1, SPEC_OCCURRENCES = 2, SPEC_UNIQUE = 3, SPEC_MAX = 4, SPEC_CURSOR = 5, SPEC_WORDS = 8 };

// what the leaf kernel writes besides the sums: the histogram alone, gcsa2_mem records {0, k, sp, ep, count()} of every state
// with their count()s in an array of their own (the `known` of k_seed_cap), or gcsa2_index_kmer records of the states
// whose value lies in a window
enum : int { SPEC_HISTOGRAM = 0, SPEC_SEEDS = 1, SPEC_LIST = 2 };

// Histogram bins kept per workgroup in LDS.  Values 0 .. SPECTRUM_LDS_BINS - 1 (after the clamp to n_hist - 1) are counted
// there and flushed with one global atomic per workgroup and non-zero bin; larger ones go to global memory one by one.
constexpr u32 SPECTRUM_LDS_BINS = 64;
constexpr u32 SPECTRUM_LEAF_GROUPS_PER_CU = 12;     // four times the 3 workgroups a CU holds at the kernel's 3 waves per SIMD

// The last level: one lane per state of depth k - 1 (`depth`), whose non-empty children are the k-mers.  value = count(range)
// with counts != 0, Range::length(range) otherwise (count_range is then never evaluated: an image without counters will do).
// A workgroup takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of TPB states and keeps its sums and its LDS table over
// all of them: the host launches a few workgroups per CU's worth of residency (SPECTRUM_LEAF_GROUPS_PER_CU), so that the
// atomics below number thousands per level, not one set per 256 states.  (One workgroup per tile had 5 atomics per workgroup
// on one cache line: 2.5 ms of 7.5 ms on 89 M 14-mers; profiles/kmer_spectrum.md.)
//   stat[SPEC_KMERS .. SPEC_UNIQUE] += the number of children, the sum of their lengths, the sum of count() (counts != 0 only),
//   the children of value 1; stat[SPEC_MAX] = max(value).  Per wavefront the two numbers are ballots and popcounts and the two
//   sums a butterfly; the waves meet in LDS, and the workgroup issues one atomic per field that is not zero.
//   hist (n_hist > 0 words, or nullptr): hist[min(value, n_hist - 1)] += 1 per child.  Value 1 -- nearly every k-mer of a
//   graph index -- is not even an LDS atomic: the wave's popcount is added once.
//   SPEC_SEEDS: every child leaves {0, depth + 1, sp, ep, value} at its slot of recs and value at the same slot of rec_counts.
//   SPEC_LIST: the children with min_value <= value and (max_value == 0 or value <= max_value) leave
//   {sp, ep, counts ? value : 0, length, depth + 1, kmer[3]}.  Slots come from stat[SPEC_CURSOR] (wg_reserve), which counts on
//   when `capacity` is passed; nothing is written behind it.
template<int MODE>
__global__ __launch_bounds__(TPB, 3) void k_spectrum_leaf(DevImage img, const u64* __restrict__ in, const u64* __restrict__ in_keys, u64 n_in, u32 limit,
                                                       u32 depth, int counts, unsigned long long* __restrict__ hist, u64 n_hist,
                                                       unsigned long long* __restrict__ stat, u64 min_value, u64 max_value,
                                                       u64* __restrict__ recs, u64* __restrict__ rec_counts, u64 capacity)
{
  constexpr u32 WAVES = TPB / 64;
  __shared__ WgSlots slots;
  __shared__ u32 low[SPECTRUM_LDS_BINS];
  __shared__ unsigned long long part[WAVES][5];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 below = (u64(1) << lane) - 1;
  for(u32 b = threadIdx.x; b < SPECTRUM_LDS_BINS; b += TPB) { low[b] = 0; }
  __syncthreads();
  const u64 last_bin = (n_hist > 0 ? n_hist - 1 : 0);
  u64 wave_kmers = 0, wave_unique = 0;            // uniform in the wavefront
  u64 my_nodes = 0, my_occurrences = 0, my_max = 0;
  for(u64 tile = blockIdx.x; tile * TPB < n_in; tile += gridDim.x)        // (uniform in the workgroup)
  {
    const u64 q = tile * TPB + threadIdx.x;
    const bool live = q < n_in;
    const ulonglong2 r = live ? reinterpret_cast<const ulonglong2*>(in)[q] : make_ulonglong2(1, 0);
    u64 key[3] = {0, 0, 0};
    if(MODE == SPEC_LIST && live) { key[0] = in_keys[3 * q]; key[1] = in_keys[3 * q + 1]; key[2] = in_keys[3 * q + 2]; }
    for(u32 c0 = 1; c0 <= limit; c0 += KMER_CHUNK)
    {
      u64 csp[KMER_CHUNK], cep[KMER_CHUNK], value[KMER_CHUNK], emit[KMER_CHUNK];
      lf_children<KMER_CHUNK>(img, c0, limit, live, r.x, r.y, csp, cep);
      u32 wave_count = 0;
#pragma unroll
      for(int j = 0; j < KMER_CHUNK; j++)
      {
        const bool alive = live && c0 + u32(j) <= limit && !range_empty(csp[j], cep[j]);
        u64 nodes = 0;
        value[j] = 0;
        if(alive)
        {
          nodes = cep[j] + 1 - csp[j];
          value[j] = (counts != 0 ? count_range(img, csp[j], cep[j]) : nodes);
          my_nodes += nodes;
          if(counts != 0) { my_occurrences += value[j]; }
          my_max = (value[j] > my_max ? value[j] : my_max);
          if(hist != nullptr && value[j] != 1)
          {
            const u64 bin = (value[j] < last_bin ? value[j] : last_bin);
            if(bin < SPECTRUM_LDS_BINS) { atomicAdd(&low[bin], 1u); }
            else { atomicAdd(hist + bin, 1ull); }                              // bin <= n_hist - 1
          }
        }
        const u64 mask = __ballot(alive);
        wave_kmers += u64(__popcll(mask));
        wave_unique += u64(__popcll(__ballot(alive && value[j] == 1)));
        emit[j] = 0;
        if(MODE == SPEC_SEEDS) { emit[j] = mask; }
        if(MODE == SPEC_LIST) { emit[j] = __ballot(alive && value[j] >= min_value && (max_value == 0 || value[j] <= max_value)); }
        wave_count += u32(__popcll(emit[j]));
      }
      if(MODE == SPEC_HISTOGRAM) { continue; }
      u64 slot = wg_reserve(slots, stat + SPEC_CURSOR, wave_count);
#pragma unroll
      for(int j = 0; j < KMER_CHUNK; j++)
      {
        const u64 at = slot + __popcll(emit[j] & below);
        if(((emit[j] >> lane) & 1) && at < capacity)
        {
          if(MODE == SPEC_SEEDS)
          {
            u64* rec = recs + 5 * at;
            rec[0] = 0; rec[1] = u64(depth) + 1; rec[2] = csp[j]; rec[3] = cep[j]; rec[4] = value[j];
            rec_counts[at] = value[j];
          }
          else
          {
            u64 child[3] = {key[0], key[1], key[2]};
            kmer_set(child, depth, c0 + u32(j));
            u64* rec = recs + 8 * at;
            rec[0] = csp[j]; rec[1] = cep[j]; rec[2] = (counts != 0 ? value[j] : 0); rec[3] = cep[j] + 1 - csp[j]; rec[4] = u64(depth) + 1;
            rec[5] = child[0]; rec[6] = child[1]; rec[7] = child[2];
          }
        }
        slot += __popcll(emit[j]);
      }
    }
  }
  my_nodes = wave_sum(my_nodes);
  my_occurrences = wave_sum(my_occurrences);
#pragma unroll
  for(u32 o = 32; o > 0; o >>= 1) { const u64 other = __shfl_xor(my_max, o, 64); my_max = (other > my_max ? other : my_max); }
  if(lane == 0)
  {
    part[wave][0] = wave_kmers; part[wave][1] = my_nodes; part[wave][2] = my_occurrences; part[wave][3] = wave_unique; part[wave][4] = my_max;
    if(hist != nullptr && wave_unique != 0) { atomicAdd(&low[last_bin < 1 ? last_bin : 1], u32(wave_unique)); }
  }
  __syncthreads();
  if(threadIdx.x < 4)
  {
    unsigned long long sum = 0;
    for(u32 w = 0; w < WAVES; w++) { sum += part[w][threadIdx.x]; }
    if(sum != 0) { atomicAdd(stat + threadIdx.x, sum); }                     // SPEC_KMERS .. SPEC_UNIQUE are words 0 .. 3
  }
  if(threadIdx.x == 4)
  {
    unsigned long long most = 0;
    for(u32 w = 0; w < WAVES; w++) { most = (part[w][4] > most ? part[w][4] : most); }
    if(most != 0) { atomicMax(stat + SPEC_MAX, most); }
  }
  if(hist != nullptr)
  {
    for(u32 b = threadIdx.x; b < SPECTRUM_LDS_BINS; b += TPB) { if(low[b] != 0) { atomicAdd(hist + b, (unsigned long long)low[b]); } }   // low[b] != 0 only for b <= n_hist - 1
  }
}

}  // namespace
