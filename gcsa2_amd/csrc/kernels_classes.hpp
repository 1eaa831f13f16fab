// kernels_classes.hpp -- k-mer classes (gcsa2_kmer_classes_device, gcsa2_seed_classes_device): per read (or group of seed
// records) the votes of its counted records over classes of bins of located values.  The transpose of k-mer support: the same
// search, fold and chunked locate, but the sums stay with the read.  Included by gcsa2_hip.hip after kernels_support.hpp
// (k_support_iota / gather / heads / runs / cut, wave_sum) and kernels_locate.hpp (count_range, k_block_owners, owner_in_wave).
//
// Data flow: k_classes_fold (k_support_class's cap and compaction; additionally every record keeps its compacted place or
// "not counted") -> the sorts, heads and runs of kernels_support.hpp, unchanged -> k_classes_run_of (compacted place -> run) ->
// per chunk of runs locate_core(sort = 1), k_classes_keys (one key (run, class) per located value), a radix sort and a
// run-length encoding of the keys (hipCUB), k_classes_sign (the encoded keys become the runs' SIGNATURES: per run the list of
// (class, n_c) with n_c > 0, the values without a class last) -> k_classes_vote (one wavefront per read: its records look up
// run -> signature and add into a row of 64-bit counters in LDS; the row and the call leave with plain stores).
// The signatures of all runs are kept: at most one entry per distinct located value, whatever the number of records.
#pragma once

namespace {

// device counters of one call (CLS_CURSOR: the counted records in the low half, the found ones in the high half, as SUP_CURSOR;
// CLS_CUT: two words, k_support_cut's answer)
enum : u32 { CLS_CURSOR = 0, CLS_VOTES = 1, CLS_UNCLASSIFIED = 2, CLS_AMBIGUOUS = 3, CLS_CUT = 4, CLS_WORDS = 8 };

constexpr u32 CLASS_SLOT_NONE = 0xFFFFFFFFu;       // a record that is not counted (compacted places stay below: fewer than 2^32 records)
constexpr u32 CLASS_KEY_BITS = 13;                 // a key is run << 13 | class, class 0 .. 4095 or CLASS_KEY_NONE
constexpr u32 CLASS_KEY_NONE = 4096;               // "no class": sorts behind every class of its run
static_assert(GCSA2_CLASS_LIMIT == CLASS_KEY_NONE, "a class id and `no class` fit the key's low bits");
constexpr u32 CLASSES_FOLD_TPB = 1024;

// k_support_class with one more output: slot[i] = the compacted place of record i, or CLASS_SLOT_NONE when it is not counted.
// No weights travel: a vote is weighted by the record that casts it, not by its run.  One atomic per workgroup.
__global__ __launch_bounds__(CLASSES_FOLD_TPB) void k_classes_fold(DevImage img, const u64* __restrict__ recs, u32 words, const u64* __restrict__ known,
                                                                   u64 m, u64 hit_max, unsigned long long* __restrict__ stat, u64* __restrict__ sp_out,
                                                                   u64* __restrict__ ep_out, u64* __restrict__ count_out, u32* __restrict__ slot)
{
  constexpr u32 WAVES = CLASSES_FOLD_TPB / 64;
  __shared__ u32 wave_counted[WAVES], wave_found[WAVES];
  __shared__ u64 group_base;
  const u64 i = u64(blockIdx.x) * CLASSES_FOLD_TPB + threadIdx.x;
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
    group_base = (word != 0 ? u64(atomicAdd(stat + CLS_CURSOR, (unsigned long long)word)) & 0xFFFFFFFFull : 0);
  }
  __syncthreads();
  if(counted)
  {
    u64 at = group_base + u64(__popcll(c & ((u64(1) << lane) - 1)));        // at < m: no more places are reserved than records exist
    for(u32 w = 0; w < wave; w++) { at += wave_counted[w]; }
    sp_out[at] = sp; ep_out[at] = ep; count_out[at] = count;
    slot[i] = u32(at);
  }
  else if(i < m) { slot[i] = CLASS_SLOT_NONE; }
}

// perm: the compacted place of the record at sorted place i; run: the inclusive scan of the heads.  run_of[place] = its run.
__global__ __launch_bounds__(TPB) void k_classes_run_of(const u32* __restrict__ perm, const u32* __restrict__ run, u64 count, u32* __restrict__ run_of)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  if(i < count) { run_of[perm[i]] = run[i] - 1; }
}

// One lane per located value of a chunk of runs (offsets / values / owners as in k_support_add): its key, the run inside the
// chunk above the class of the value's bin.  A bin beyond the map and a class id >= n_classes (GCSA2_CLASS_NONE among them)
// are "no class".  The bin is taken unsigned.
__global__ __launch_bounds__(TPB) void k_classes_keys(const u64* __restrict__ offsets, const u64* __restrict__ values, const u64* __restrict__ owners,
                                                      u64 total, u32 shift, const u32* __restrict__ class_of_bin, u64 n_bins, u32 n_classes,
                                                      u64* __restrict__ keys)
{
  const u64 j = u64(blockIdx.x) * TPB + threadIdx.x;
  const bool live = j < total;
  const u64 r = owner_in_wave(owners, offsets, total, live ? j : 0, live);
  if(!live) { return; }
  const u64 bin = values[j] >> shift;
  u32 cls = CLASS_KEY_NONE;
  if(bin < n_bins)
  {
    const u32 id = class_of_bin[bin];
    if(id < n_classes) { cls = id; }
  }
  keys[j] = (r << CLASS_KEY_BITS) | cls;
}

// The chunk's sorted keys, run-length encoded: `unique` keys with their `lengths`, *n_entries of them.  Entry e becomes the
// signature entry n_c << 32 | class at sig[base + e]; the first and the last entry of a run write the run's span
// {begin, end} of entries (zeroed beforehand: a run without a value has the empty span).  q0: the chunk's first run.
__global__ __launch_bounds__(TPB) void k_classes_sign(const u64* __restrict__ unique, const u32* __restrict__ lengths, const u32* __restrict__ n_entries,
                                                      u64 q0, u64 base, u64* __restrict__ sig, u64* __restrict__ span)
{
  const u64 e = u64(blockIdx.x) * TPB + threadIdx.x, n = *n_entries;
  if(e >= n) { return; }
  const u64 key = unique[e], run = key >> CLASS_KEY_BITS;
  sig[base + e] = (u64(lengths[e]) << 32) | (key & ((u64(1) << CLASS_KEY_BITS) - 1));
  if(e == 0 || (unique[e - 1] >> CLASS_KEY_BITS) != run) { span[2 * (q0 + run)] = base + e; }
  if(e + 1 == n || (unique[e + 1] >> CLASS_KEY_BITS) != run) { span[2 * (q0 + run) + 1] = base + e + 1; }
}

// (votes, class) a ahead of b: more votes, the lower id on a tie.  A lane without a candidate holds (0, GCSA2_UNKNOWN).
__device__ __forceinline__ bool class_ahead(u64 va, u64 ca, u64 vb, u64 cb) { return va > vb || (va == vb && ca < cb); }

// One wavefront (= one workgroup) per read or group, the workgroups striding over them; row: n_classes 64-bit counters in
// dynamic LDS.  WINDOWS: group q owns the windows [group_off[q], group_off[q + 1]) of the search, whose record -- if the window
// was found -- sits at wave_base[w / 64] + the found lanes below it in wave_mask[w / 64] (k_kmer_seeds' arrival order: no
// record is moved into window order).  Otherwise group q owns the records [group_off[q], group_off[q + 1]); a group whose
// offsets decrease or reach beyond `limit` is not read.  slot == nullptr: there is no record at all.
// A counted record of run r reads r's signature: `none` from its last entry, the number of classes from its span; it adds
// w n_c (PER_WINDOW: w) to row[c] with 64-bit LDS adds unless UNAMBIGUOUS bars it.  Then the lanes store the row (if asked
// for) and keep their two best classes, six shuffle rounds merge them, and lane 0 stores the call.  The statistics are summed
// in registers over all groups of the workgroup: three atomics per workgroup at its end, none per read.
template<bool WINDOWS>
__global__ __launch_bounds__(64) void k_classes_vote(const u64* __restrict__ group_off, u64 n_groups, u64 limit, const u32* __restrict__ wave_base,
                                                     const u64* __restrict__ wave_mask, const u32* __restrict__ slot, const u32* __restrict__ run_of,
                                                     const u64* __restrict__ span, const u64* __restrict__ sig, const u64* __restrict__ weights,
                                                     int flags, u32 n_classes, u64* __restrict__ votes, gcsa2_class_call* __restrict__ calls,
                                                     unsigned long long* __restrict__ stat)
{
  extern __shared__ unsigned long long row[];
  const u32 lane = threadIdx.x;
  const bool per_window = (flags & GCSA2_CLASS_PER_WINDOW) != 0, unambiguous = (flags & GCSA2_CLASS_UNAMBIGUOUS) != 0;
  u64 all_votes = 0, all_none = 0, all_ambiguous = 0;
  for(u64 q = blockIdx.x; q < n_groups; q += gridDim.x)
  {
    for(u32 c = lane; c < n_classes; c += 64) { row[c] = 0; }
    __syncthreads();
    u64 begin = 0, end = 0, counted = 0;
    if(slot != nullptr)
    {
      begin = group_off[q]; end = group_off[q + 1];
      if(begin > end || end > limit) { begin = 0; end = 0; }
    }
    for(u64 i = begin + lane; i < end; i += 64)
    {
      u64 rec = i;
      if constexpr(WINDOWS)
      {
        const u64 mask = wave_mask[i / 64], bit = u64(1) << (i & 63);
        if((mask & bit) == 0) { continue; }
        rec = u64(wave_base[i / 64]) + u64(__popcll(mask & (bit - 1)));
      }
      const u32 place = slot[rec];
      if(place == CLASS_SLOT_NONE) { continue; }
      counted++;
      const u32 r = run_of[place];
      const u64 first = span[2 * u64(r)], last = span[2 * u64(r) + 1];
      if(first >= last) { continue; }
      const u64 tail = sig[last - 1];
      const u64 none = (u32(tail) == CLASS_KEY_NONE ? tail >> 32 : 0);
      const u64 classes = last - first - (none != 0 ? 1 : 0);
      all_none += none;
      if(classes >= 2) { all_ambiguous++; }
      if(classes == 0 || (unambiguous && classes != 1)) { continue; }
      const u64 w = (weights != nullptr ? weights[rec] : 1);
      for(u64 x = first; x < first + classes; x++)
      {
        const u64 entry = sig[x];
        atomicAdd(row + u32(entry), (unsigned long long)(per_window ? w : w * (entry >> 32)));
      }
    }
    __syncthreads();
    u64 total = 0, v1 = 0, c1 = GCSA2_UNKNOWN, v2 = 0, c2 = GCSA2_UNKNOWN;
    for(u32 c = lane; c < n_classes; c += 64)
    {
      const u64 v = row[c];
      if(votes != nullptr) { votes[q * n_classes + c] = v; }
      total += v;
      if(v == 0) { continue; }
      if(class_ahead(v, c, v1, c1)) { v2 = v1; c2 = c1; v1 = v; c1 = c; }
      else if(class_ahead(v, c, v2, c2)) { v2 = v; c2 = c; }
    }
#pragma unroll
    for(u32 o = 32; o > 0; o >>= 1)
    {
      const u64 w1 = __shfl_xor(v1, o, 64), d1 = __shfl_xor(c1, o, 64), w2 = __shfl_xor(v2, o, 64), d2 = __shfl_xor(c2, o, 64);
      if(class_ahead(w1, d1, v1, c1))
      {
        if(class_ahead(v1, c1, w2, d2)) { v2 = v1; c2 = c1; } else { v2 = w2; c2 = d2; }
        v1 = w1; c1 = d1;
      }
      else if(class_ahead(w1, d1, v2, c2)) { v2 = w1; c2 = d1; }
    }
    total = wave_sum(total);
    counted = wave_sum(counted);
    if(lane == 0)
    {
      all_votes += total;
      if(calls != nullptr)
      {
        u64* dst = reinterpret_cast<u64*>(calls + q);
        dst[0] = c1; dst[1] = v1; dst[2] = c2; dst[3] = v2; dst[4] = total; dst[5] = counted;
      }
    }
    __syncthreads();                                         // the row is read before the next group zeroes it
  }
  all_none = wave_sum(all_none); all_ambiguous = wave_sum(all_ambiguous);
  if(lane == 0)
  {
    if(all_votes != 0) { atomicAdd(stat + CLS_VOTES, (unsigned long long)all_votes); }
    if(all_none != 0) { atomicAdd(stat + CLS_UNCLASSIFIED, (unsigned long long)all_none); }
    if(all_ambiguous != 0) { atomicAdd(stat + CLS_AMBIGUOUS, (unsigned long long)all_ambiguous); }
  }
}

}  // namespace
