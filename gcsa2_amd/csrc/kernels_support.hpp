// kernels_support.hpp -- k-mer support (gcsa2_kmer_support_device, gcsa2_seed_support_device): seed records in any order
// become per-bin sums.  Included by gcsa2_hip.hip after kernels_locate.hpp (count_range, k_block_owners, owner_in_wave).
//
// Data flow, the host side of which is host_fold.hpp up to the last kernel: fold_seed_ranges -- k_seed_cap (one lane per
// record: count(), the cap, the counted records compacted in arrival order) -> two stable radix passes by ep, then sp
// (hipCUB) -> k_support_heads + an inclusive scan (the run number of every record) -> k_support_runs (per run {sp, ep},
// count() and the summed weight) -> a scan of the runs' count() -- then cut_chunks (k_support_cut) and, per chunk of runs,
// for_located_chunks -- locate_core(sort = 1) into scratch of the chunk's size, k_block_owners over its value offsets -- and
// k_support_add.  k-mer classes (kernels_classes.hpp) take the same way to their own last kernels.
// Nothing here is kept in an order the caller sees; the sums are integers, so the result does not depend on arrival.
#pragma once

namespace {

// device counters of one call
// (SUP_CURSOR: the counted records in the low half, the found ones in the high half; SUP_CUT: two words)
enum : u32 { SUP_CURSOR = 0, SUP_ADDED = 1, SUP_DROPPED = 2, SUP_CUT = 3, SUP_WORDS = 8 };

// The sum of v over the lanes of the wavefront, in every lane.
__device__ __forceinline__ u64 wave_sum(u64 v)
{
#pragma unroll
  for(u32 o = 32; o > 0; o >>= 1) { v += __shfl_xor(v, o, 64); }
  return v;
}

// A run: neighbouring lanes with equal keys (the same key may come again further on: that is another run).  The inclusive sum
// of v over the lanes of the own run at and below this lane; `tail`: this lane is the last of its run in the wavefront and
// holds the run's sum.  Every lane takes part.
__device__ __forceinline__ u64 wave_run_sum(u64 key, u64 v, u32 lane, bool& tail)
{
  const u64 below_key = __shfl_up(key, 1, 64);
  const u64 heads = __ballot(lane == 0 || below_key != key);                  // bit 0 is always set
  const u32 first = 63u - u32(__clzll((long long)(heads & (~u64(0) >> (63 - lane)))));      // where the own run begins
#pragma unroll
  for(u32 o = 1; o < 64; o <<= 1)
  {
    const u64 below = __shfl_up(v, o, 64);
    if(lane >= first + o) { v += below; }
  }
  tail = (lane == 63 || ((heads >> (lane + 1)) & 1) != 0);
  return v;
}

// The cap and the compaction of both consumers of seed records: k_seed_cap<false, const u64*> for k-mer support,
// k_seed_cap<true> for k-mer classes (kernels_classes.hpp).
// One lane per record: `words` u64 per record with (sp, ep) at words 2 and 3 (4: the arrival records of k_kmer_seeds, whose
// count() is known[i]; 5: gcsa2_mem, whose count field is NOT read -- count() is evaluated here).  found: a non-empty range;
// counted: found, count() != 0 (a range that reaches beyond the index has none) and hit_max == 0 or count() <= hit_max.  The
// counted lanes of a workgroup are ranked -- a ballot per wavefront, the wavefronts' numbers through LDS -- and the workgroup
// reserves their places with ONE atomic add on stat[SUP_CURSOR], which carries the found records in its high half (both
// numbers stay below 2^32); the lanes leave (sp, ep, count()) at their places, in arrival order between workgroups.
// What else a record leaves follows SLOTS.  false: its weight at its place, out[place] = weights[i], when `out` is there.
// true: out[i] = the compacted place of record i, or SEED_SLOT_NONE when it is not counted; no weights travel (a vote is
// weighted by the record that casts it, not by its run), and the kernel has no such parameter: `Weights` is empty.  That is
// why the weights are a pack -- an instance's argument offsets are part of its code, and with its own parameter list each
// instance is, instruction for instruction, the kernel it replaced (k_support_class, k_classes_fold;
// profiles/seed_fold_refactor.md).
// (The first form had every wavefront add to three counters of one cache line: 6.3 M atomics on three addresses were 75 ms
// of a 115 ms call on 135 M records; profiles/kmer_support.md.)
constexpr u32 SEED_CAP_TPB = 1024;
constexpr u32 SEED_SLOT_NONE = 0xFFFFFFFFu;        // a record that is not counted (compacted places stay below: fewer than 2^32 records)

template<bool SLOTS, class... Weights>
__global__ __launch_bounds__(SEED_CAP_TPB) void k_seed_cap(DevImage img, const u64* __restrict__ recs, u32 words, const u64* __restrict__ known,
                                                           Weights __restrict__... weights, u64 m, u64 hit_max, unsigned long long* __restrict__ stat,
                                                           u64* __restrict__ sp_out, u64* __restrict__ ep_out, u64* __restrict__ count_out,
                                                           std::conditional_t<SLOTS, u32, u64>* __restrict__ out)
{
  static_assert(sizeof...(Weights) == (SLOTS ? 0 : 1), "the weights travel exactly when the slots do not");
  constexpr u32 WAVES = SEED_CAP_TPB / 64;
  __shared__ u32 wave_counted[WAVES], wave_found[WAVES];
  __shared__ u64 group_base;
  const u64 i = u64(blockIdx.x) * SEED_CAP_TPB + threadIdx.x;
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  u64 sp = 0, ep = 0, count = 0;
  bool found = false, counted = false;
  if(i < m)
  {
    sp = recs[u64(words) * i + 2]; ep = recs[u64(words) * i + 3];
    found = !range_empty(sp, ep);
    if(found)
    {
      count = (known != nullptr ? known[i] : count_range(img, sp, ep));
      counted = (count != 0 && (hit_max == 0 || count <= hit_max));
    }
  }
  const u64 f = __ballot(found), c = __ballot(counted);
  if(lane == 0) { wave_found[wave] = u32(__popcll(f)); wave_counted[wave] = u32(__popcll(c)); }
  __syncthreads();
  if(threadIdx.x == 0)
  {
    u64 all_found = 0, all_counted = 0;
    for(u32 w = 0; w < WAVES; w++) { all_found += wave_found[w]; all_counted += wave_counted[w]; }
    const u64 word = (all_found << 32) | all_counted;
    group_base = (word != 0 ? u64(atomicAdd(stat + SUP_CURSOR, (unsigned long long)word)) & 0xFFFFFFFFull : 0);
  }
  __syncthreads();
  if(counted)
  {
    u64 at = group_base + u64(__popcll(c & ((u64(1) << lane) - 1)));        // at < m: no more places are reserved than records exist
    for(u32 w = 0; w < wave; w++) { at += wave_counted[w]; }
    sp_out[at] = sp; ep_out[at] = ep; count_out[at] = count;
    if constexpr(SLOTS) { out[i] = u32(at); }
    else if(out != nullptr) { out[at] = (weights, ...)[i]; }
  }
  else if(SLOTS && i < m) { out[i] = SEED_SLOT_NONE; }
}

__global__ __launch_bounds__(TPB) void k_support_iota(u32* __restrict__ dst, u64 count)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  if(i < count) { dst[i] = u32(i); }
}

__global__ __launch_bounds__(TPB) void k_support_gather(const u64* __restrict__ src, const u32* __restrict__ perm, u64 count, u64* __restrict__ dst)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  if(i < count) { dst[i] = src[perm[i]]; }
}

// Records sorted by (sp, ep): sp[i] in sorted order, ep through the permutation.  head[i] = 1 where a run begins.
__global__ __launch_bounds__(TPB) void k_support_heads(const u64* __restrict__ sp, const u64* __restrict__ ep, const u32* __restrict__ perm, u64 count,
                                                       u32* __restrict__ head)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  if(i >= count) { return; }
  head[i] = (i == 0 || sp[i] != sp[i - 1] || ep[perm[i]] != ep[perm[i - 1]]) ? 1u : 0u;
}

// run: the inclusive scan of head (run of record i = run[i] - 1).  The head of a run writes its range and count(); the weights
// of a run (1 each without `weights`) are summed per wavefront and reach mult[run] (zeroed beforehand) with one atomic per
// (wavefront, run) -- 1000 windows of one k-mer are sixteen atomics, not 1000.
__global__ __launch_bounds__(TPB) void k_support_runs(const u64* __restrict__ sp, const u64* __restrict__ ep, const u64* __restrict__ counts,
                                                      const u64* __restrict__ weights, const u32* __restrict__ perm, const u32* __restrict__ run,
                                                      u64 count, u64* __restrict__ ranges, u64* __restrict__ run_counts,
                                                      unsigned long long* __restrict__ mult)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const bool live = i < count;
  u64 r = ~u64(0), w = 0;
  if(live)
  {
    const u32 p = perm[i];
    r = u64(run[i]) - 1;
    w = (weights != nullptr ? weights[p] : 1);
    if(i == 0 || run[i - 1] != run[i])
    {
      reinterpret_cast<ulonglong2*>(ranges)[r] = make_ulonglong2(sp[i], ep[p]);
      run_counts[r] = counts[p];
    }
  }
  bool tail = false;
  const u64 sum = wave_run_sum(r, w, lane, tail);
  if(live && tail && sum != 0) { atomicAdd(mult + r, (unsigned long long)sum); }
}

// The end of the chunk that begins with run q0: the largest q1 in (q0, min(runs, q0 + most)] with run_off[q1] - run_off[q0] <=
// budget, and q0 + 1 when even the first run exceeds it -- a chunk always holds a run.  out = {q1, the chunk's count() sum}.
__global__ void k_support_cut(const u64* __restrict__ run_off, u64 runs, u64 q0, u64 budget, u64 most, unsigned long long* __restrict__ out)
{
  u64 lo = q0 + 1, hi = (runs - q0 > most ? q0 + most : runs);
  const u64 base = run_off[q0];
  while(lo < hi)
  {
    const u64 mid = (lo + hi + 1) >> 1;
    if(run_off[mid] - base <= budget) { lo = mid; } else { hi = mid - 1; }
  }
  out[0] = lo; out[1] = run_off[lo] - base;
}

// One lane per located value of a chunk of runs: offsets / values are the chunk's CSR from locate_core(sort = 1) (`runs`
// ranges, `total` values, total >= 1), owners its k_block_owners table over 64 values, mult the chunk's summed weights.
// The lane finds its run inside its wavefront's bracket, takes bin = value >> shift, and with per_bin drops out when the
// value below it in the same run has the same bin (the values of a run are sorted, so equal bins are neighbours).  A bin
// >= n_bins is not written: its weight goes to SUP_DROPPED.  Neighbouring lanes with the same bin -- values of one node, and
// of neighbouring runs on one node -- are summed in the wavefront and issue ONE 64-bit atomic add; added and dropped are
// wavefront sums, one atomic each.
__global__ __launch_bounds__(TPB) void k_support_add(const u64* __restrict__ offsets, const u64* __restrict__ values, const u64* __restrict__ owners,
                                                     u64 runs, u64 total, const unsigned long long* __restrict__ mult, u32 shift, int per_bin,
                                                     unsigned long long* __restrict__ support, u64 n_bins, unsigned long long* __restrict__ stat)
{
  const u64 j = u64(blockIdx.x) * TPB + threadIdx.x;
  const u32 lane = threadIdx.x & 63;
  const bool live = j < total;
  const u64 r = owner_in_wave(owners, offsets, total, live ? j : 0, live);
  u64 bin = ~u64(0), add = 0, drop = 0;
  if(live)
  {
    bin = values[j] >> shift;
    const bool repeat = per_bin && j > offsets[r] && (values[j - 1] >> shift) == bin;
    const u64 w = (repeat ? 0 : u64(mult[r]));
    if(bin < n_bins) { add = w; } else { drop = w; }
  }
  bool tail = false;
  const u64 sum = wave_run_sum(bin, add, lane, tail);
  if(live && tail && sum != 0 && bin < n_bins) { atomicAdd(support + bin, (unsigned long long)sum); }
  const u64 added = wave_sum(add), dropped = wave_sum(drop);
  if(lane == 0)
  {
    if(added != 0) { atomicAdd(stat + SUP_ADDED, (unsigned long long)added); }
    if(dropped != 0) { atomicAdd(stat + SUP_DROPPED, (unsigned long long)dropped); }
  }
  (void)runs;
}

}  // namespace
