// host_anchors.hpp -- the skeleton that seed clusters and seed chains share.  Both take a CSR of seed records with their hits,
// turn every (seed, hit) pair into a placed anchor, work per group -- in LDS, or device-wide for the groups above a capacity --
// and write a top row and a summary per group.  Here, once: the plan with its host round trip (anchors_plan), the two launch
// shapes of the LDS kernels (anchors_lds_launches), the head of the large path (anchors_large_offsets), the tail that brings
// the counters home (anchors_tail), the argument checks of the seed forms (seed_form_checks), the fused entry points
// (fused_hits, fused_stranded_hits, fused_anchors_entry) and the host forms (anchors_batch).  clusters_core and chains_core (gcsa2_hip.hip) keep
// what is theirs: the sorts, scans and score of the clusters, the sorts, dynamic program and finish of the chains.
// Host code only.  Part of the single translation unit gcsa2_hip.hip, which includes it once Scratch, stats_entry, the hits
// calls (kmer_hits_found, minimizer_select) and the kernels of kernels_clusters.hpp are defined.
#pragma once

namespace {

// GCSA2_CLUSTER_LDS for the cluster calls, GCSA2_CHAIN_LDS for the chain calls (test knobs, read per call): the anchors of a
// group that k_clusters_lds (k_chains_lds) holds, a power of two from CLU_CAP_MIN to CLU_CAP_DEFAULT; anything else is ignored.
// No result but stats.spilled depends on it.
u32 cluster_capacity(const char* knob)
{
  u64 v = 0;
  if(env_count(knob, &v) && v >= CLU_CAP_MIN && v <= CLU_CAP_DEFAULT && (v & (v - 1)) == 0) { return u32(v); }
  return CLU_CAP_DEFAULT;
}

// What the plan leaves: the counters (CLU_WORDS), per group its anchors or "invalid" (info) and its anchors if it is above the
// capacity (lsize, n_groups + 1 words), the anchors above the capacity in all (count < 2^32) and the largest group in LDS.
struct AnchorPlan { unsigned long long* stat = nullptr; u64 *info = nullptr, *lsize = nullptr, count = 0, most = 0; };

// The first step of a core (n_groups >= 1; n_groups, n_seeds, n_hits < 2^32): k_clusters_plan and the call's one host round
// trip before its end.  `what` ("clusters", "chains") heads the two refusals, which cannot be met unless the plan kernel is
// wrong; the stream is idle at both, so the arena may go back as it is.  Scratch: 16 bytes per group.  Leaves
// scratch.settled false: anchors_tail, or whoever returns before it once a kernel is launched, sets it.
int anchors_plan(const gcsa2_index* ix, const u64* goff, u64 n_groups, u64 n_seeds, const u64* hoff, u64 n_hits, u32 cap, const char* what, AnchorPlan& plan,
                 Scratch& scratch, hipStream_t st)
{
  HIP_TRY(scratch.get(plan.stat, CLU_WORDS));
  HIP_TRY(scratch.get(plan.info, n_groups));
  HIP_TRY(scratch.get(plan.lsize, n_groups + 1));
  HIP_TRY(hipMemsetAsync(plan.stat, 0, CLU_WORDS * sizeof(unsigned long long), st));
  scratch.settled = false;
  const u64 resident = u64(ix->compute_units) * 8;
  hipLaunchKernelGGL(k_clusters_plan, dim3(unsigned(std::min<u64>((n_groups + 3) / 4, resident))), dim3(TPB), 0, st, goff, n_groups, n_seeds, hoff, n_hits,
                     u64(cap), plan.info, plan.lsize, plan.stat);
  LAUNCH_CHECK("k_clusters_plan");
  unsigned long long host_stat[CLU_WORDS];
  HIP_TRY(hipMemcpyAsync(host_stat, plan.stat, sizeof(host_stat), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  plan.count = host_stat[CLU_LARGE]; plan.most = host_stat[CLU_MAX_SMALL];
  if(plan.count >= (u64(1) << 32)) { scratch.settled = true; return fail(GCSA2_ERR_HIP, std::string(what) + ": more anchors than hits"); }
  if(plan.most > cap) { scratch.settled = true; return fail(GCSA2_ERR_HIP, std::string(what) + ": a group in LDS above the capacity"); }
  return GCSA2_OK;
}

// The groups in LDS: one wavefront each up to CLU_WAVE_MAX anchors, a workgroup of TPB lanes each above (that launch only if
// there is such a group); a launch takes the LDS of its largest group.  launch(width, grid, lds, fit, above, spill) launches
// the caller's kernel<T>, T = decltype(width)::value, with `fit` anchors of LDS for the groups of above < anchors <= spill;
// `wide` is its kernel<TPB>, `name` the kernel's.
template<u32 T> using LdsWidth = std::integral_constant<u32, T>;
template<class Launch>
int anchors_lds_launches(const gcsa2_index* ix, u64 n_groups, u64 most, u32 cap, const void* wide, const char* name, Launch launch)
{
  const auto grid = [&](size_t lds, u64 limit)
  {
    const u64 per_cu = std::max<u64>(1, std::min<u64>(limit, (160u << 10) / (lds + 2048)));
    return dim3(unsigned(std::min<u64>(n_groups, u64(ix->compute_units) * per_cu * 4)));
  };
  u32 fit = CLU_CAP_MIN;
  while(fit < most && fit < CLU_WAVE_MAX) { fit *= 2; }
  const u64 narrow = std::min<u64>(fit, cap);                 // the groups of up to this many anchors
  size_t lds = size_t(fit) * CLU_LDS_BYTES;
  launch(LdsWidth<64>(), grid(lds, 32), lds, fit, u64(0), narrow);
  LAUNCH_CHECK(name);
  if(most > narrow)
  {
    while(fit < most) { fit *= 2; }
    lds = size_t(fit) * CLU_LDS_BYTES;
    if(lds > (48u << 10)) { HIP_TRY(hipFuncSetAttribute(wide, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds))); }
    launch(LdsWidth<TPB>(), grid(lds, 8), lds, fit, narrow, u64(cap));
    LAUNCH_CHECK(name);
  }
  return GCSA2_OK;
}

// The head of the large path (plan.count > 0): loff (n_groups + 1), the exclusive scan of lsize -- the anchors of group g are
// the places [loff[g], loff[g + 1]) of every array of the path.  rest(bytes) is the caller's, between the request of loff and
// that of hipCUB's space: it requests its arrays and raises `bytes` to what its sorts and scans need.
template<class Rest>
int anchors_large_offsets(const AnchorPlan& plan, u64 n_groups, u64*& loff, char*& tmp, size_t& bytes, Scratch& scratch, hipStream_t st, Rest rest)
{
  HIP_TRY(scratch.get(loff, n_groups + 1));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, plan.lsize, loff, size_t(n_groups + 1), st));
  const int rc = rest(bytes);
  if(rc != GCSA2_OK) { return rc; }
  HIP_TRY(scratch.get(tmp, bytes));
  HIP_TRY(hipMemsetAsync(plan.lsize + n_groups, 0, sizeof(u64), st));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, plan.lsize, loff, size_t(n_groups + 1), st));
  return GCSA2_OK;
}

// The end of a core: the counters come home, the arena is settled, and every field of *out but `groups` is filled; `found`
// is the field of the clusters or of the chains.
template<class Stats>
int anchors_tail(const AnchorPlan& plan, Stats* out, uint64_t Stats::* found, Scratch& scratch, hipStream_t st)
{
  unsigned long long host_stat[CLU_WORDS];
  HIP_TRY(hipMemcpyAsync(host_stat, plan.stat, sizeof(host_stat), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  scratch.settled = true;
  out->invalid_groups = host_stat[CLU_INVALID]; out->seeds = host_stat[CLU_SEEDS]; out->anchors = host_stat[CLU_ANCHORS];
  out->unplaced = host_stat[CLU_UNPLACED]; out->*found = host_stat[CLU_CLUSTERS]; out->spilled = host_stat[CLU_SPILLED];
  return GCSA2_OK;
}

// what gcsa2_seed_clusters_device and gcsa2_seed_chains_device (`name`: "seed_clusters", "seed_chains") refuse of their CSR
int seed_form_checks(const std::string& name, const void* goff, u64 n_groups, const void* seeds, u64 n_seeds, const void* hoff, const void* hits, u64 n_hits)
{
  if(n_groups > 0 && goff == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, name + ": d_group_offsets is NULL"); }
  if(n_seeds > 0 && seeds == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, name + ": d_seeds is NULL"); }
  if(n_seeds > 0 && hoff == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, name + ": d_hit_offsets is NULL"); }
  if(n_hits > 0 && hits == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, name + ": d_hits is NULL"); }
  const char* many = (n_groups >= (u64(1) << 32) ? "groups" : n_seeds >= (u64(1) << 32) ? "seeds" : n_hits >= (u64(1) << 32) ? "hits" : nullptr);
  if(many != nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, name + ": 2^32 or more " + many + " in one call; split the batch"); }
  return GCSA2_OK;
}

// What the fused forms run first, after their argument checks (0 < n_patterns < 2^32): the windows (every stride-th, or the
// minimizers) and the hits call's own core behind them (kmer_hits_found) into scratch of this call.  The hit buffer is sized
// by a guess -- four hits per window, no more than hit_max allows -- and a batch beyond it runs the hits again with the size
// the first run reported.  `name` is the call's ("kmer_clusters"), `what` heads the refusal of 2^32 seeds or hits.
struct FusedHits { u64 *seed_off = nullptr, *hit_off = nullptr, *hit_values = nullptr, m = 0, h = 0; gcsa2_mem* seeds = nullptr; };

// Behind the windows: `total` of them with the offsets `woff` over n_groups "reads" (kmer_hits_found: at j stride, at the
// positions of `mins`, or the keys of `wins` -- the groups of a stranded call).
int fused_hits_found(const gcsa2_index* ix, Scratch& scratch, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_groups, u64 k, u64 stride, const u64* woff,
                     u64 total, const gcsa2_minimizer* mins, const ulonglong2* wins, u64 hit_max, int over, const char* what, FusedHits& out, hipStream_t st)
{
  u64 *seed_off = nullptr, *hit_off = nullptr, *hit_values = nullptr, m = 0, h = 0;
  gcsa2_mem* seeds = nullptr;
  u64 room = std::max<u64>(4 * total, 1024);
  if(hit_max > 0 && hit_max < 4) { room = std::max<u64>(hit_max * total, 1); }
  HIP_TRY(scratch.get(seed_off, n_groups + 1));
  HIP_TRY(scratch.get(seeds, total));
  HIP_TRY(scratch.get(hit_off, total + 1));
  HIP_TRY(scratch.get(hit_values, room));
  int rc = kmer_hits_found(ix, scratch, d_patterns, d_offsets, n_groups, k, stride, woff, total, mins, hit_max, over, nullptr, seed_off, seeds,
                           total, &m, hit_off, hit_values, room, &h, st, wins);
  if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && m <= total && h > room)
  {
    room = h;
    HIP_TRY(scratch.get(hit_values, room));
    g_error.clear();
    rc = kmer_hits_found(ix, scratch, d_patterns, d_offsets, n_groups, k, stride, woff, total, mins, hit_max, over, nullptr, seed_off, seeds,
                         total, &m, hit_off, hit_values, room, &h, st, wins);
  }
  if(rc != GCSA2_OK) { return rc; }
  if(m >= (u64(1) << 32) || h >= (u64(1) << 32))
  {
    return fail(GCSA2_ERR_BUFFER_TOO_SMALL, std::string(what) + ": 2^32 or more seeds or hits in one call; split the batch");
  }
  out.seed_off = seed_off; out.seeds = seeds; out.hit_off = hit_off; out.hit_values = hit_values; out.m = m; out.h = h;
  return GCSA2_OK;
}

int fused_hits(const gcsa2_index* ix, Scratch& scratch, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 stride, bool minimizers,
               u64 w, u64 hash_seed, u64 hit_max, int over, const char* name, const char* what, FusedHits& out, hipStream_t st)
{
  u64 *woff = nullptr, total = 0;
  gcsa2_minimizer* mins = nullptr;
  const int rc = (minimizers ? minimizer_select(ix, scratch, d_patterns, d_offsets, n_patterns, k, w, hash_seed, nullptr, true, nullptr, 0, name, st,
                                                woff, mins, total)
                             : window_plan(scratch, d_offsets, n_patterns, k, stride, nullptr, name, st, woff, total));
  if(rc != GCSA2_OK) { return rc; }
  return fused_hits_found(ix, scratch, d_patterns, d_offsets, n_patterns, k, (minimizers ? 1 : stride), woff, total, mins, nullptr, hit_max, over, what, out, st);
}

// The same on both strands of every read (gcsa2_stranded_minimizer_hits_device's own core, 0 < n_patterns < 2^31): the seed CSR
// has 2 n_patterns groups.
int fused_stranded_hits(const gcsa2_index* ix, Scratch& scratch, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 w, u64 hash_seed,
                        u64 hit_max, int over, const char* name, const char* what, FusedHits& out, hipStream_t st)
{
  u64 *goff = nullptr, searched = 0;
  ulonglong2* wins = nullptr;
  const int rc = stranded_windows(ix, scratch, d_patterns, d_offsets, n_patterns, k, w, hash_seed, GCSA2_STRAND_BOTH, name, st, goff, wins, searched);
  if(rc != GCSA2_OK) { return rc; }
  return fused_hits_found(ix, scratch, nullptr, nullptr, 2 * n_patterns, k, 1, goff, searched, nullptr, wins, hit_max, over, what, out, st);
}

// the windows of a fused or host form: every stride-th k-mer, or the (w, k)-minimizers
struct AnchorWindows { u64 k, stride; bool minimizers; u64 w, hash_seed, hit_max; int over; };

int windows_checks(const gcsa2_index* ix, const AnchorWindows& win)
{
  u64 unused_seeds = 0, unused_hits = 0;
  return (win.minimizers ? minimizer_hits_checks(ix, win.k, win.w, win.over, &unused_seeds, &unused_hits)
                         : kmer_hits_checks(ix, win.k, win.stride, win.over, &unused_seeds, &unused_hits));
}

// The fused device forms (`name`: "kmer_clusters", "minimizer_chains", ...): checks(), the job's own refusals, in front of
// those of the windows and of the reads; then fused_hits and core -- clusters_core or chains_core -- with the seed offsets as
// the groups.
template<class Stats, class Job, class Checks, class Core>
int fused_anchors_entry(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, const AnchorWindows& win, const Job& job,
                        const char* name, const char* what, Checks checks, Core core, Stats* stats, void* stream)
{
  int rc = checks();
  if(rc != GCSA2_OK) { return rc; }
  rc = windows_checks(ix, win);
  if(rc != GCSA2_OK) { return rc; }
  if(n_patterns > 0 && d_offsets == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, std::string(name) + ": d_offsets is NULL"); }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, std::string(name) + ": 2^32 or more reads in one call; split the batch"); }
  Stats pre{};
  pre.groups = n_patterns;
  return stats_entry(name, ix, stats, pre, n_patterns == 0, [&](Stats& sums) -> int
  {
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scratch scratch(ix, st);
    FusedHits f;
    const int hits_rc = fused_hits(ix, scratch, d_patterns, d_offsets, n_patterns, win.k, win.stride, win.minimizers, win.w, win.hash_seed, win.hit_max, win.over,
                                   name, what, f, st);
    if(hits_rc != GCSA2_OK) { return hits_rc; }
    return core(ix, f.seed_off, n_patterns, f.seeds, f.m, f.hit_off, f.hit_values, f.h, job, &sums, scratch, st);
  });
}

// one output array of a host form: per_read records of `size` bytes for every read (for every unit of reads, where the form has
// such units: anchors_batch); not asked for without a host pointer or records
struct PieceOutput { void* host; u64 per_read; size_t size; };

// The host forms (`name`: the whole "gcsa2_kmer_clusters_batch").  The coordinate map goes to the device once; each piece
// (for_read_pieces) is one fused device call on its thread's stream -- call(piece, d_patterns, d_offsets, d_map, d_outs,
// stats) -> status, d_outs[i] the device array of outs[i] or nullptr -- into device arrays of its own, copied to the piece's
// place in the caller's arrays.  `unit` > 1 (the chain pairs: 2): the reads come in units of that many, n_patterns is a multiple
// of it (checks() refuses anything else), a piece holds whole units -- the cut is read_cut over every unit-th offset -- and an
// output has its per_read records per unit.  Stats may be several structs of counters side by side.
template<class Stats, size_t N, class Checks, class Call>
int anchors_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, u64 n_patterns, const AnchorWindows& win, const uint64_t* coord_of_bin,
                  u64 n_bins, const PieceOutput (&outs)[N], Stats* stats, const char* name, Checks checks, Call call, u64 unit = 1)
{
  int rc = checks();
  if(rc != GCSA2_OK) { return rc; }
  rc = windows_checks(ix, win);
  if(rc != GCSA2_OK) { return rc; }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, std::string(name) + ": 2^32 or more reads in one call; split the batch"); }
  Stats sums{};
  if(n_patterns == 0) { if(stats != nullptr) { *stats = sums; } return GCSA2_OK; }
  if(offsets == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, std::string(name) + ": offsets is NULL"); }
  rc = reads_ok(patterns, offsets, n_patterns, name);
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  g_error.clear();
  if(host_windows(offsets, n_patterns, win.k, (win.minimizers ? 1 : win.stride)) >= (u64(1) << 32))
  {
    return fail(GCSA2_ERR_BUFFER_TOO_SMALL, std::string(name) + ": 2^32 or more windows in one call; split the batch");
  }
  DeviceGuard guard(ix->device);
  DBuf<u64> d_map;
  HIP_TRY(d_map.alloc(n_bins));
  HIP_TRY(hipMemcpy(d_map.p, coord_of_bin, n_bins * sizeof(u64), hipMemcpyHostToDevice));
  std::vector<u64> cut;
  if(unit == 1) { cut = read_cut(ix, offsets, n_patterns); }
  else
  {
    std::vector<u64> unit_offsets(n_patterns / unit + 1);
    for(u64 i = 0; i < unit_offsets.size(); i++) { unit_offsets[i] = offsets[i * unit]; }
    cut = read_cut(ix, unit_offsets.data(), n_patterns / unit);
    for(u64& at : cut) { at *= unit; }
  }
  std::vector<Stats> done(cut.size() - 1);
  rc = for_read_pieces(ix, offsets, cut, [&](const ReadPiece& p, Outcome& out) -> bool
  {
    DBuf<u8> d_pat, d_out[N]; DBuf<u64> d_off;
    void* d_outs[N];
    if(!upload_reads(p, patterns, d_pat, d_off, out)) { return false; }
    hipError_t e = hipSuccess;
    for(size_t i = 0; i < N; i++)
    {
      if(e == hipSuccess && outs[i].host != nullptr && outs[i].per_read > 0) { e = d_out[i].alloc(p.count / unit * outs[i].per_read * outs[i].size); }
      d_outs[i] = d_out[i].p;
    }
    if(e != hipSuccess) { out.hip_error("upload of a piece", e); return false; }
    const int piece_rc = call(p, d_pat.p, d_off.p, d_map.p, d_outs, &done[p.c]);
    if(piece_rc != GCSA2_OK) { out.set(piece_rc, g_error); return false; }
    for(size_t i = 0; i < N; i++)
    {
      const size_t read_bytes = outs[i].per_read * outs[i].size;
      if(e == hipSuccess && d_outs[i] != nullptr) { e = hipMemcpy(static_cast<u8*>(outs[i].host) + p.b / unit * read_bytes, d_outs[i], p.count / unit * read_bytes, hipMemcpyDeviceToHost); }
    }
    if(e != hipSuccess) { out.hip_error("download of a piece", e); return false; }
    return true;
  });
  if(rc != GCSA2_OK) { return rc; }
  for(const Stats& s : done) { sum_stats(sums, s); }
  if(stats != nullptr) { *stats = sums; }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string(name) + ": " + e.what()); }
}

}  // namespace
