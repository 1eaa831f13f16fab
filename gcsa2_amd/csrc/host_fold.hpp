// host_fold.hpp -- what every consumer of seed records does before its own kernels: the cap, the fold of equal ranges into
// runs, the cut of the runs into chunks, and the locate pass of every chunk.  k-mer support (support_tail) adds the located
// values into bins; k-mer classes (classes_tail) turn them into signatures and votes.
// Host code only.  Part of the single translation unit gcsa2_hip.hip, which includes it once Scratch, locate_core and the
// kernels of kernels_support.hpp and kernels_classes.hpp are defined.
#pragma once

namespace {

static_assert(SUP_CURSOR == CLS_CURSOR && SUP_WORDS == CLS_WORDS, "both callers' counters begin with the cursor word");

constexpr u64 SUPPORT_CHUNK_DEFAULT = u64(1) << 22;    // values (before deduplication) located per chunk: the smallest budget within 2.5 % of the best time, profiles/kmer_support.md

// GCSA2_SUPPORT_CHUNK (a test knob, read per call): the value budget of a chunk.  The result never depends on it.
u64 support_chunk_budget()
{
  u64 budget = SUPPORT_CHUNK_DEFAULT, v = 0;
  if(env_count("GCSA2_SUPPORT_CHUNK", &v) && v >= 1) { budget = v; }
  return std::min(budget, (u64(1) << 31) - 1);       // one pass of the locate pipeline
}

// The counted records of a call folded into runs of equal ranges.  Per run q < distinct: ranges[2 q] = {sp, ep}, mult[q] the
// summed weight, run_off[q] the count()s of the runs below it (distinct + 1 entries).  With slots: slot[i] is the compacted
// place of record i or SEED_SLOT_NONE, run_of[place] its run, span two zeroed words per run (the caller's).
struct SeedFold
{
  u64 found = 0, counted = 0, distinct = 0;
  u64 *ranges = nullptr, *run_off = nullptr;
  unsigned long long* mult = nullptr;
  u32 *slot = nullptr, *run_of = nullptr;
  u64* span = nullptr;
};

// Steps 1 and 2 of a call: m (< 2^32) records of `words` u64 with (sp, ep) at words 2 and 3, their count()s in `known` or
// (nullptr) computed here.  Zeroes the caller's SUP_WORDS counters at `stat`; the cap first (only the counted records reach
// the sort), then stable radix passes by ep and by sp over as many bits as a path node has, heads, runs.  `weights` (or
// nullptr: 1 each) are summed per run; `slots`: every record keeps its compacted place instead (k_seed_cap<true>) and no weight
// travels (weights == nullptr).  Without a counted record -- m == 0 among that -- nothing beyond found and counted is made:
// what is still to be written is the caller's.  Host round trips: the number of counted records, the number of distinct
// ranges.  Scratch: per record 24 bytes (and 4 or, with weights, 8); per counted record 32 bytes (and 4) and the sorts'
// temporaries; per distinct range 40 bytes (and 16).  Leaves scratch.settled false.
int fold_seed_ranges(const gcsa2_index* ix, const u64* recs, u32 words, const u64* known, const u64* weights, u64 m, u64 hit_max, bool slots,
                     unsigned long long* stat, SeedFold& fold, Scratch& scratch, hipStream_t st)
{
  HIP_TRY(hipMemsetAsync(stat, 0, SUP_WORDS * sizeof(unsigned long long), st));
  scratch.settled = false;
  if(m == 0) { return GCSA2_OK; }
  u64 *csp = nullptr, *cep = nullptr, *ccnt = nullptr, *cw = nullptr;
  if(slots) { HIP_TRY(scratch.get(fold.slot, m)); }
  HIP_TRY(scratch.get(csp, m)); HIP_TRY(scratch.get(cep, m)); HIP_TRY(scratch.get(ccnt, m));
  if(weights != nullptr) { HIP_TRY(scratch.get(cw, m)); }
  const dim3 cap_grid(unsigned((m + SEED_CAP_TPB - 1) / SEED_CAP_TPB));
  if(slots) { hipLaunchKernelGGL((k_seed_cap<true>), cap_grid, dim3(SEED_CAP_TPB), 0, st, ix->img, recs, words, known, m, hit_max, stat, csp, cep, ccnt, fold.slot); }
  else { hipLaunchKernelGGL((k_seed_cap<false, const u64*>), cap_grid, dim3(SEED_CAP_TPB), 0, st, ix->img, recs, words, known, weights, m, hit_max, stat, csp, cep, ccnt, cw); }
  LAUNCH_CHECK("k_seed_cap");
  unsigned long long host_stat[SUP_WORDS];
  HIP_TRY(hipMemcpyAsync(host_stat, stat, sizeof(host_stat), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const u64 c = host_stat[SUP_CURSOR] & 0xFFFFFFFFull;
  fold.found = host_stat[SUP_CURSOR] >> 32;
  fold.counted = c;
  if(c == 0) { return GCSA2_OK; }
  u64 top = (ix->img.n > ix->img.e ? ix->img.n : ix->img.e);
  int bits = 1;
  while(bits < 64 && (top >> bits) != 0) { bits++; }
  u64 *key_a = nullptr, *key_b = nullptr, *run_counts = nullptr;
  u32 *perm_a = nullptr, *perm_b = nullptr, *head = nullptr, *run = nullptr;
  char* tmp = nullptr;
  HIP_TRY(scratch.get(key_a, c)); HIP_TRY(scratch.get(key_b, c));
  HIP_TRY(scratch.get(perm_a, c)); HIP_TRY(scratch.get(perm_b, c));
  HIP_TRY(scratch.get(head, c)); HIP_TRY(scratch.get(run, c));
  if(slots) { HIP_TRY(scratch.get(fold.run_of, c)); }
  size_t sort_bytes = 0, scan_bytes = 0, sum_bytes = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, cep, key_a, perm_a, perm_b, size_t(c), 0, bits, st));
  HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, head, run, size_t(c), st));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, sum_bytes, key_a, key_b, size_t(c + 1), st));
  HIP_TRY(scratch.get(tmp, std::max(sort_bytes, std::max(scan_bytes, sum_bytes))));
  hipLaunchKernelGGL(k_support_iota, dim3(grid_for(c)), dim3(TPB), 0, st, perm_a, c);
  LAUNCH_CHECK("k_support_iota");
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, cep, key_a, perm_a, perm_b, size_t(c), 0, bits, st));      // perm_b: by ep
  hipLaunchKernelGGL(k_support_gather, dim3(grid_for(c)), dim3(TPB), 0, st, csp, perm_b, c, key_a);
  LAUNCH_CHECK("k_support_gather");
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, key_a, key_b, perm_b, perm_a, size_t(c), 0, bits, st));    // key_b, perm_a: by (sp, ep)
  hipLaunchKernelGGL(k_support_heads, dim3(grid_for(c)), dim3(TPB), 0, st, key_b, cep, perm_a, c, head);
  LAUNCH_CHECK("k_support_heads");
  HIP_TRY(hipcub::DeviceScan::InclusiveSum(tmp, scan_bytes, head, run, size_t(c), st));
  if(slots)
  {
    hipLaunchKernelGGL(k_classes_run_of, dim3(grid_for(c)), dim3(TPB), 0, st, perm_a, run, c, fold.run_of);
    LAUNCH_CHECK("k_classes_run_of");
  }
  u32 d32 = 0;
  HIP_TRY(hipMemcpyAsync(&d32, run + (c - 1), sizeof(u32), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const u64 d = d32;
  fold.distinct = d;
  HIP_TRY(scratch.get(fold.ranges, 2 * d)); HIP_TRY(scratch.get(run_counts, d + 1)); HIP_TRY(scratch.get(fold.run_off, d + 1)); HIP_TRY(scratch.get(fold.mult, d));
  if(slots) { HIP_TRY(scratch.get(fold.span, 2 * d)); }
  HIP_TRY(hipMemsetAsync(fold.mult, 0, d * sizeof(unsigned long long), st));
  if(slots) { HIP_TRY(hipMemsetAsync(fold.span, 0, 2 * d * sizeof(u64), st)); }
  HIP_TRY(hipMemsetAsync(run_counts + d, 0, sizeof(u64), st));
  hipLaunchKernelGGL(k_support_runs, dim3(grid_for(c)), dim3(TPB), 0, st, key_b, cep, ccnt, static_cast<const u64*>(cw), perm_a, run, c, fold.ranges, run_counts, fold.mult);
  LAUNCH_CHECK("k_support_runs");
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, sum_bytes, run_counts, fold.run_off, size_t(d + 1), st));
  return GCSA2_OK;
}

// Step 3: the chunks of the fold's runs, q0 .. q1 - 1 with the count() sum `raw` within the budget, one run at least.
struct SeedChunk { u64 q0, q1, raw; };
struct SeedChunks
{
  std::vector<SeedChunk> list;
  u64 most_runs = 0, most_raw = 0, all_raw = 0;
};

// d_cut: two counter words of the caller's.  One host round trip per chunk.  `who` begins the message of a failure.
int cut_chunks(const gcsa2_index* ix, const SeedFold& fold, unsigned long long* d_cut, const char* who, SeedChunks& chunks, Scratch& scratch, hipStream_t st)
{
  const u64 budget = support_chunk_budget(), d = fold.distinct;
  for(u64 q0 = 0; q0 < d; )
  {
    unsigned long long cut[2] = {0, 0};
    hipLaunchKernelGGL(k_support_cut, dim3(1), dim3(1), 0, st, fold.run_off, d, q0, budget, ix->tune.locate_split_queries, d_cut);
    LAUNCH_CHECK("k_support_cut");
    HIP_TRY(hipMemcpyAsync(cut, d_cut, sizeof(cut), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const u64 q1 = cut[0], raw = cut[1];
    if(q1 <= q0 || q1 > d) { scratch.settled = true; return fail(GCSA2_ERR_HIP, std::string(who) + ": a chunk without a range"); }
    chunks.list.push_back(SeedChunk{q0, q1, raw});
    chunks.most_runs = std::max(chunks.most_runs, q1 - q0); chunks.most_raw = std::max(chunks.most_raw, raw); chunks.all_raw += raw;
    q0 = q1;
  }
  return GCSA2_OK;
}

// The front of step 4: off / val / owners once at the size of the largest chunk, then prepare() -- the caller's own buffers of
// that size -- and chunk by chunk, in the same scratch, locate_core(sort = 1) and k_block_owners; a chunk with a value goes to
// body(chunk, runs, total, off, val, owners, values), `values` being those of the chunks before it.  Both return a status.
// *values_out: the values of all chunks.  Host round trips: those of every chunk's locate pass.  Scratch: 8 bytes per range
// and 8 1/8 bytes per value of the largest chunk.
template<class Prepare, class Body>
int for_located_chunks(const gcsa2_index* ix, const SeedFold& fold, const SeedChunks& chunks, const char* who, u64* values_out, Scratch& scratch, hipStream_t st,
                       Prepare prepare, Body body)
{
  const u64 most_raw = chunks.most_raw;
  u64 *off = nullptr, *val = nullptr, *owners = nullptr;
  HIP_TRY(scratch.get(off, chunks.most_runs + 1)); HIP_TRY(scratch.get(val, most_raw)); HIP_TRY(scratch.get(owners, most_raw / OWNER_SPAN + 3));
  int rc = prepare();
  if(rc != GCSA2_OK) { return rc; }
  u64 values = 0;
  for(const SeedChunk& chunk : chunks.list)
  {
    const u64 runs = chunk.q1 - chunk.q0;
    u64 total = 0;
    ValuesProvider provide = [val, most_raw](u64 count) -> u64* { return count <= most_raw ? val : nullptr; };
    rc = locate_core(ix, fold.ranges + 2 * chunk.q0, runs, 1, off, provide, &total, st, val, most_raw);
    if(rc != GCSA2_OK) { return rc; }
    if(total == 0) { continue; }
    if(total > most_raw || values + total > chunks.all_raw)      // (the provider refuses such a count: never met)
    {
      scratch.settled = true;
      return fail(GCSA2_ERR_HIP, std::string(who) + ": a chunk with more values than its ranges count");
    }
    const u64 spans = (total + OWNER_SPAN - 1) / OWNER_SPAN;
    hipLaunchKernelGGL(k_block_owners, dim3(grid_for(spans + 1)), dim3(TPB), 0, st, off, runs, total, OWNER_SPAN, spans, owners);
    LAUNCH_CHECK("k_block_owners");
    rc = body(chunk, runs, total, off, val, owners, values);
    if(rc != GCSA2_OK) { return rc; }
    values += total;
  }
  *values_out = values;
  return GCSA2_OK;
}

}  // namespace
