// kernels_classes.hpp -- k-mer classes (gcsa2_kmer_classes_device, gcsa2_seed_classes_device): per read (or group of seed
// records) the votes of its counted records over classes of bins of located values.  The transpose of k-mer support: the same
// search, fold and chunked locate, but the sums stay with the read.  Included by gcsa2_hip.hip after kernels_support.hpp
// (k_support_iota / gather / heads / runs / cut, wave_sum) and kernels_locate.hpp (count_range, k_block_owners, owner_in_wave).
//
// Data flow: fold_seed_ranges with slots (host_fold.hpp) -- k_seed_cap<true> (the cap and compaction of k-mer support; instead
// of a weight every record keeps its compacted place or "not counted") -> the sorts, heads and runs of
// kernels_support.hpp, unchanged -> k_classes_run_of (compacted place -> run) -- then cut_chunks and, per chunk of runs,
// for_located_chunks -- locate_core(sort = 1), k_block_owners -- and k_classes_keys (one key (run, class) per located value), a
// radix sort and a run-length encoding of the keys (hipCUB), k_classes_sign (the encoded keys become the runs' SIGNATURES: per
// run the list of (class, n_c) with n_c > 0, the values without a class last) -> k_classes_vote (one wavefront per read: its
// records look up run -> signature and add into a row of 64-bit counters in LDS; the row and the call leave with plain stores).
// The signatures of all runs are kept: at most one entry per distinct located value, whatever the number of records.
// The sparse form (gcsa2_kmer_top_classes_device, gcsa2_seed_top_classes_device) takes the same way with the WIDE instances of
// the key and signature kernels and ends in k_classes_top (a hash table in LDS instead of the row; per read its top classes).
#pragma once

namespace {

// device counters of one call (CLS_CURSOR: the counted records in the low half, the found ones in the high half, as SUP_CURSOR;
// CLS_CUT: two words, k_support_cut's answer)
enum : u32 { CLS_CURSOR = 0, CLS_VOTES = 1, CLS_UNCLASSIFIED = 2, CLS_AMBIGUOUS = 3, CLS_CUT = 4, CLS_WORDS = 8 };

constexpr u32 CLASS_KEY_BITS = 13;                 // a key is run << 13 | class, class 0 .. 4095 or CLASS_KEY_NONE
constexpr u32 CLASS_KEY_NONE = 4096;               // "no class": sorts behind every class of its run
static_assert(GCSA2_CLASS_LIMIT == CLASS_KEY_NONE, "a class id and `no class` fit the key's low bits");
// The wide keys of gcsa2_kmer_top_classes_device: a class id of 32 bits, so a key is run << 33 | class with "no class" =
// 2^32 behind every class of its run (a chunk has fewer than 2^31 runs), and a signature entry n_c << 32 | class with
// 0xFFFFFFFF for "no class" (a class id is below n_classes <= 0xFFFFFFFF).
constexpr u32 WIDE_KEY_BITS = 33;
constexpr u64 WIDE_KEY_NONE = u64(1) << 32;
constexpr u32 WIDE_SIG_NONE = 0xFFFFFFFFu;

// perm: the compacted place of the record at sorted place i; run: the inclusive scan of the heads.  run_of[place] = its run.
__global__ __launch_bounds__(TPB) void k_classes_run_of(const u32* __restrict__ perm, const u32* __restrict__ run, u64 count, u32* __restrict__ run_of)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  if(i < count) { run_of[perm[i]] = run[i] - 1; }
}

// One lane per located value of a chunk of runs (offsets / values / owners as in k_support_add): its key, the run inside the
// chunk above the class of the value's bin.  A bin beyond the map and a class id >= n_classes (GCSA2_CLASS_NONE among them)
// are "no class".  The bin is taken unsigned.  WIDE: the wide key, and n_classes of 64 bits.
template<bool WIDE>
__global__ __launch_bounds__(TPB) void k_classes_keys(const u64* __restrict__ offsets, const u64* __restrict__ values, const u64* __restrict__ owners,
                                                      u64 total, u32 shift, const u32* __restrict__ class_of_bin, u64 n_bins,
                                                      std::conditional_t<WIDE, u64, u32> n_classes, u64* __restrict__ keys)
{
  const u64 j = u64(blockIdx.x) * TPB + threadIdx.x;
  const bool live = j < total;
  const u64 r = owner_in_wave(owners, offsets, total, live ? j : 0, live);
  if(!live) { return; }
  const u64 bin = values[j] >> shift;
  std::conditional_t<WIDE, u64, u32> cls = (WIDE ? WIDE_KEY_NONE : CLASS_KEY_NONE);
  if(bin < n_bins)
  {
    const u32 id = class_of_bin[bin];
    if(id < n_classes) { cls = id; }
  }
  keys[j] = (r << (WIDE ? WIDE_KEY_BITS : CLASS_KEY_BITS)) | cls;
}

// The chunk's sorted keys, run-length encoded: `unique` keys with their `lengths`, *n_entries of them.  Entry e becomes the
// signature entry n_c << 32 | class (WIDE: WIDE_SIG_NONE for "no class") at sig[base + e]; the first and the last entry of a
// run write the run's span {begin, end} of entries (zeroed beforehand: a run without a value has the empty span).  q0: the
// chunk's first run.
template<bool WIDE>
__global__ __launch_bounds__(TPB) void k_classes_sign(const u64* __restrict__ unique, const u32* __restrict__ lengths, const u32* __restrict__ n_entries,
                                                      u64 q0, u64 base, u64* __restrict__ sig, u64* __restrict__ span)
{
  constexpr u32 BITS = (WIDE ? WIDE_KEY_BITS : CLASS_KEY_BITS);
  const u64 e = u64(blockIdx.x) * TPB + threadIdx.x, n = *n_entries;
  if(e >= n) { return; }
  const u64 key = unique[e], run = key >> BITS;
  const u64 cls = key & ((u64(1) << BITS) - 1);
  sig[base + e] = (u64(lengths[e]) << 32) | (WIDE && cls == WIDE_KEY_NONE ? u64(WIDE_SIG_NONE) : cls);
  if(e == 0 || (unique[e - 1] >> BITS) != run) { span[2 * (q0 + run)] = base + e; }
  if(e + 1 == n || (unique[e + 1] >> BITS) != run) { span[2 * (q0 + run) + 1] = base + e + 1; }
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
      if(place == SEED_SLOT_NONE) { continue; }
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

// ---- the sparse form (gcsa2_kmer_top_classes_device, gcsa2_seed_top_classes_device) -------------------------------------------

constexpr u32 TOP_KEY_EMPTY = 0xFFFFFFFFu;         // never a class: ids are below n_classes <= 0xFFFFFFFF
constexpr u32 TOP_PROBES = 16;                     // a longer probe sequence counts as a full table
constexpr u32 TOP_SLOTS_MIN = 64, TOP_SLOTS_MAX = 4096, TOP_SLOTS_DEFAULT = 512;     // 12 bytes of LDS per slot: 48 KB at most
static_assert(GCSA2_TOP_LIMIT == 64, "lane j of the wavefront holds the j-th class of the running top row");

// murmur3's finaliser, a bijection of 32-bit words: the high bits choose the pass of a class, the low bits its first slot
__device__ __forceinline__ u32 top_hash(u32 c)
{
  c ^= c >> 16; c *= 0x85EBCA6Bu; c ^= c >> 13; c *= 0xC2B2AE35u; c ^= c >> 16;
  return c;
}

// k_classes_vote without the dense row: one wavefront (= one workgroup) per read or group, the same records and signatures
// (wide entries: WIDE_SIG_NONE for "no class"), added into a hash table in dynamic LDS -- `slots` (a power of two >= 64)
// 64-bit counters, then `slots` 32-bit keys; open addressing, linear probing, at most TOP_PROBES places.  A read is processed
// in 2^pbits passes: pass p takes the classes whose hash has p in its top pbits bits, so every class lives in exactly one
// pass, and `voted`, `total` and the top row add up over the passes.  A class that finds no place within its probes makes
// the wavefront start the read again with pbits + 1: exact whatever the number of classes, because the hash is a bijection --
// at pbits = 32 - log2(slots) the classes of a pass have distinct first slots and nothing is ever probed twice.
// The running top row lives in registers, lane j holding the j-th class (votes, id) in class_ahead order.  After a pass every
// lane reads slots / 64 entries ONCE; an entry joins the row only if it is ahead of the row's entry top_n - 1 (a ballot), by
// one wave-wide insertion (a ballot and four 64-bit shuffles).  In a random table order that is about
// top_n (1 + ln(voted / top_n)) insertions per read instead of top_n slots / 64 LDS reads per lane.
// No global atomics but the three per workgroup for the stats.
template<bool WINDOWS>
__global__ __launch_bounds__(64) void k_classes_top(const u64* __restrict__ group_off, u64 n_groups, u64 limit, const u32* __restrict__ wave_base,
                                                    const u64* __restrict__ wave_mask, const u32* __restrict__ slot, const u32* __restrict__ run_of,
                                                    const u64* __restrict__ span, const u64* __restrict__ sig, const u64* __restrict__ weights,
                                                    int flags, u32 slots, u32 top_n, gcsa2_class_vote* __restrict__ top,
                                                    gcsa2_top_summary* __restrict__ summaries, unsigned long long* __restrict__ stat)
{
  extern __shared__ unsigned long long top_lds[];
  unsigned long long* const vals = top_lds;
  u32* const keys = reinterpret_cast<u32*>(top_lds + slots);
  const u32 lane = threadIdx.x;
  const bool per_window = (flags & GCSA2_CLASS_PER_WINDOW) != 0, unambiguous = (flags & GCSA2_CLASS_UNAMBIGUOUS) != 0;
  u32 slot_bits = 6;
  while((u32(1) << slot_bits) < slots) { slot_bits++; }
  u64 all_votes = 0, all_none = 0, all_ambiguous = 0;
  for(u64 q = blockIdx.x; q < n_groups; q += gridDim.x)
  {
    u64 begin = 0, end = 0;
    if(slot != nullptr)
    {
      begin = group_off[q]; end = group_off[q + 1];
      if(begin > end || end > limit) { begin = 0; end = 0; }
    }
    u64 tv = 0, tc = GCSA2_UNKNOWN, voted = 0, total = 0, counted = 0, none_sum = 0, ambiguous = 0;
    for(u32 pbits = 0; ; pbits++)
    {
      tv = 0; tc = GCSA2_UNKNOWN; voted = 0; total = 0;
      bool full = false;
      for(u64 pass = 0; pass < (u64(1) << pbits) && !full; pass++)
      {
        for(u32 s = lane; s < slots; s += 64) { keys[s] = TOP_KEY_EMPTY; vals[s] = 0; }
        __syncthreads();
        counted = 0; none_sum = 0; ambiguous = 0;                // the same in every pass; the last pass's are kept
        bool lost = false;
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
          if(place == SEED_SLOT_NONE) { continue; }
          counted++;
          const u32 r = run_of[place];
          const u64 first = span[2 * u64(r)], last = span[2 * u64(r) + 1];
          if(first >= last) { continue; }
          const u64 tail = sig[last - 1];
          const u64 none = (u32(tail) == WIDE_SIG_NONE ? tail >> 32 : 0);
          const u64 classes = last - first - (none != 0 ? 1 : 0);
          none_sum += none;
          if(classes >= 2) { ambiguous++; }
          if(classes == 0 || (unambiguous && classes != 1)) { continue; }
          const u64 w = (weights != nullptr ? weights[rec] : 1);
          for(u64 x = first; x < first + classes; x++)
          {
            const u64 entry = sig[x];
            const u32 c = u32(entry), h = top_hash(c);
            if(pbits != 0 && u64(h >> (32 - pbits)) != pass) { continue; }
            u32 at = h & (slots - 1), probe = 0;
            for(; probe < TOP_PROBES; probe++, at = (at + 1) & (slots - 1))
            {
              const u32 old = atomicCAS(keys + at, TOP_KEY_EMPTY, c);
              if(old == TOP_KEY_EMPTY || old == c) { break; }
            }
            if(probe == TOP_PROBES) { lost = true; continue; }
            atomicAdd(vals + at, (unsigned long long)(per_window ? w : w * (entry >> 32)));
          }
        }
        __syncthreads();
        // the classes of a pass with distinct first slots never probe: at the last pbits a pass cannot be full
        full = (__any(lost) != 0) && pbits + slot_bits < 32;
        if(!full)
        {
          for(u32 s = lane; s < slots; s += 64)                 // slots is a multiple of 64: the whole wavefront takes every turn
          {
            const u64 v = vals[s], c = keys[s];
            total += v;
            if(v != 0) { voted++; }
            const u64 cut_v = __shfl(tv, int(top_n - 1), 64), cut_c = __shfl(tc, int(top_n - 1), 64);
            u64 fresh = __ballot(v != 0 && class_ahead(v, c, cut_v, cut_c));
            while(fresh != 0)
            {
              const int src = __ffsll((unsigned long long)fresh) - 1;
              fresh &= fresh - 1;
              const u64 nv = __shfl(v, src, 64), nc = __shfl(c, src, 64);
              const u32 pos = u32(__popcll(__ballot(class_ahead(tv, tc, nv, nc))));      // the row is sorted: those ahead are a prefix
              const u64 uv = __shfl_up(tv, 1, 64), uc = __shfl_up(tc, 1, 64);
              if(lane == pos) { tv = nv; tc = nc; }
              else if(lane > pos) { tv = uv; tc = uc; }
            }
          }
        }
        __syncthreads();                                         // the table is read before the next pass clears it
      }
      if(!full) { break; }
    }
    voted = wave_sum(voted);
    total = wave_sum(total);
    counted = wave_sum(counted);
    all_none += none_sum; all_ambiguous += ambiguous;
    if(top != nullptr && lane < top_n)
    {
      u64* dst = reinterpret_cast<u64*>(top + q * top_n + lane);
      dst[0] = tc; dst[1] = tv;
    }
    if(lane == 0)
    {
      all_votes += total;
      if(summaries != nullptr)
      {
        u64* dst = reinterpret_cast<u64*>(summaries + q);
        dst[0] = voted; dst[1] = total; dst[2] = counted;
      }
    }
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
