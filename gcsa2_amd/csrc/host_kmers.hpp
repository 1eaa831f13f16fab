// host_kmers.hpp -- the index-side k-mer calls: countKMers, compareKMers and the index k-mer spectrum.  All of them walk the
// search tree of countKMers (kernels_kmers.hpp) and share one walk, kmer_walk; a call adds the launch of a level above the
// last and what it does at the last level.
// Host code only.  Part of the single translation unit gcsa2_hip.hip, which includes it once support_checks / support_tail
// and Scratch are defined (gcsa2_index_kmer_support_device hands its k-mers on to them).
#pragma once

namespace {

// One frontier buffer per depth of the search, reused by every piece of that depth (a depth-first walk over pieces: when a
// piece of depth d is taken up, everything below the piece before it is finished) and grown to the largest piece seen.
struct KmerBufs
{
  std::vector<u64*> p; std::vector<size_t> cap;
  ~KmerBufs() { for(u64* q : p) { if(q != nullptr) { (void)hipFree(q); } } }
  hipError_t get(size_t depth, size_t bytes, u64*& out)
  {
    if(p.size() <= depth) { p.resize(depth + 1, nullptr); cap.resize(depth + 1, 0); }
    if(cap[depth] < bytes)
    {
      if(p[depth] != nullptr) { (void)hipFree(p[depth]); p[depth] = nullptr; cap[depth] = 0; }
      hipError_t e = hipMalloc(reinterpret_cast<void**>(&p[depth]), bytes);
      if(e != hipSuccess) { p[depth] = nullptr; return e; }
      cap[depth] = bytes;
    }
    out = p[depth];
    return hipSuccess;
  }
};

// The level-synchronous search tree of countKMers (src/algorithms.cpp:387-421, there a seed DFS + OpenMP) below a frontier of
// `n` states at depth `depth`: state_words u64 per state (2: a range sp, ep; 4: compareKMers' range per index) and, with_keys,
// 3 u64 of key per state.  A frontier whose children might not fit one buffer (n x limit > piece; 2^27 states = 2 GB, tests cut
// finer with GCSA2_KMER_PIECE) is cut in halves that are searched one after the other IN PLACE; the children of a piece go
// into the buffer of their depth.  (Until late round 4 the halves were copied, larger levels were expanded twice -- a counting
// pass, then a filling pass -- and every piece allocated and freed its buffer: k = 17 on the 5.73 G-node index, a last frontier
// of 3.4 G states, took 4.5 s, most of it in hipMalloc / hipFree of gigabyte blocks.)
//   expand: the launch alone of a level above the last: the children of the n states go to next / next_keys, which have room
//           for n x limit of them, and *cursor, cleared before the launch, counts them
//   leaf:   the last level (the n states are the parents at depth k - 1), whatever the call does there; it is cut like the
//           others only with last_piece != 0
struct KmerWalk
{
  u64 k; u32 limit; u64 piece, last_piece; u32 state_words; bool with_keys;
  hipStream_t st; unsigned long long* cursor;
  std::function<int(const u64* frontier, const u64* keys, u64 n, u64 depth, u64* next, u64* next_keys, u64 room)> expand;
  std::function<int(const u64* frontier, const u64* keys, u64 n, u64 depth)> leaf;
  KmerBufs states, keys;
};

inline int kmer_cursor_clear(const KmerWalk& w)
{
  HIP_TRY(hipMemsetAsync(w.cursor, 0, sizeof(unsigned long long), w.st));
  return GCSA2_OK;
}

// Waits for the stream.  On the null stream the blocking copy does both: copy + wait there cost countKMers at k = 8, eight
// levels of a few microseconds each, 0.28 ms instead of 0.21 ms (profiles/kmer_walk_refactor.md).
inline int kmer_cursor_read(const KmerWalk& w, u64& produced)
{
  unsigned long long c = 0;
  if(w.st == nullptr) { HIP_TRY(hipMemcpy(&c, w.cursor, sizeof(c), hipMemcpyDeviceToHost)); }
  else
  {
    HIP_TRY(hipMemcpyAsync(&c, w.cursor, sizeof(c), hipMemcpyDeviceToHost, w.st));
    HIP_TRY(hipStreamSynchronize(w.st));
  }
  produced = c;
  return GCSA2_OK;
}

int kmer_walk(KmerWalk& w, const u64* frontier, const u64* keys, u64 n, u64 depth)
{
  while(depth < w.k && n > 0)
  {
    const bool last = (depth + 1 == w.k);
    const u64 piece = (last ? w.last_piece : w.piece);
    if(piece != 0 && n * w.limit > piece && n > 1)      // halves, one after the other, in place
    {
      const u64 half = n / 2;
      int rc = kmer_walk(w, frontier, keys, half, depth);
      if(rc == GCSA2_OK) { rc = kmer_walk(w, frontier + w.state_words * half, (keys != nullptr ? keys + 3 * half : nullptr), n - half, depth); }
      return rc;
    }
    if(last) { return w.leaf(frontier, keys, n, depth); }
    const u64 room = n * w.limit;      // one pass into the buffer of the next depth, sized for the worst case (`limit` children per state)
    u64 *next = nullptr, *next_keys = nullptr, produced = 0;
    int rc = kmer_cursor_clear(w);          // (before the buffers: a hipMalloc of theirs then runs beside it)
    if(rc != GCSA2_OK) { return rc; }
    HIP_TRY(w.states.get(size_t(depth + 1), size_t(room * w.state_words * sizeof(u64)), next));
    if(w.with_keys) { HIP_TRY(w.keys.get(size_t(depth + 1), size_t(room * 3 * sizeof(u64)), next_keys)); }
    rc = w.expand(frontier, keys, n, depth, next, next_keys, room);
    if(rc == GCSA2_OK) { rc = kmer_cursor_read(w, produced); }
    if(rc != GCSA2_OK) { return rc; }
    if(produced > room) { return fail(GCSA2_ERR_HIP, "k-mer spectrum: more states than a piece has room for"); }
    frontier = next; keys = next_keys; n = produced; depth++;
  }
  return GCSA2_OK;
}

// The walk from the root state (state_words words; its key is empty).
int kmer_walk_root(KmerWalk& w, const u64* root_words)
{
  u64 *frontier = nullptr, *keys = nullptr;
  HIP_TRY(w.states.get(0, w.state_words * sizeof(u64), frontier));
  HIP_TRY(hipMemcpyAsync(frontier, root_words, w.state_words * sizeof(u64), hipMemcpyHostToDevice, w.st));
  if(w.with_keys) { HIP_TRY(w.keys.get(0, 3 * sizeof(u64), keys)); HIP_TRY(hipMemsetAsync(keys, 0, 3 * sizeof(u64), w.st)); }
  HIP_TRY(hipStreamSynchronize(w.st));          // the root may be pageable stack memory
  return kmer_walk(w, frontier, keys, 1, 0);
}

// countKMers returns 0 for these (algorithms.cpp:391-395); so does every output of the spectrum calls
inline bool kmer_nothing(const gcsa2_index* ix, u64 k, int force) { return (k > ix->order && !force) || ix->img.n == 0; }

// comps 1..limit (algorithms.cpp:369, 379)
inline u32 kmer_limit(const gcsa2_index* ix, int include_ns) { return u32(include_ns ? ix->img.sigma - 2 : ix->img.fast_chars); }

}  // namespace

// countKMers(index, k, parameters) (src/algorithms.cpp:387-421): the count is the number of non-empty states at depth k.
extern "C" int gcsa2_count_kmers(const gcsa2_index* ix, uint64_t k, int include_ns, int force, uint64_t* result)
{
  CHECK_INDEX(ix);
  if(result == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null result"); }
  *result = 0;
  if(k == 0) { *result = 1; return GCSA2_OK; }                       // algorithms.cpp:390
  if(kmer_nothing(ix, k, force)) { return GCSA2_OK; }
  if(ix->img.sigma < 3) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "alphabet too small for countKMers"); }
  DeviceGuard guard(ix->device);
  DBuf<unsigned long long> counter;
  HIP_TRY(counter.alloc(1));
  u64 total = 0;
  KmerWalk w{k, kmer_limit(ix, include_ns), ix->tune.kmer_piece, 0, 2, false, nullptr, counter.p};
  w.expand = [&](const u64* frontier, const u64* keys, u64 n, u64 depth, u64* next, u64* next_keys, u64 room) -> int
  {
    hipLaunchKernelGGL((k_kmer_expand<false>), dim3(grid_for(n)), dim3(TPB), 0, w.st, ix->img, frontier, keys, n, w.limit, u32(depth), next, next_keys,
                       room, w.cursor);
    LAUNCH_CHECK("k_kmer_expand");
    return GCSA2_OK;
  };
  w.leaf = [&](const u64* frontier, const u64* keys, u64 n, u64 depth) -> int      // the children only have to be counted (no buffer: any size)
  {
    u64 produced = 0;
    int rc = kmer_cursor_clear(w);
    if(rc != GCSA2_OK) { return rc; }
    hipLaunchKernelGGL((k_kmer_expand<false>), dim3(grid_for(n)), dim3(TPB), 0, w.st, ix->img, frontier, keys, n, w.limit, u32(depth), (u64*)nullptr,
                       (u64*)nullptr, u64(0), w.cursor);
    LAUNCH_CHECK("k_kmer_expand");
    rc = kmer_cursor_read(w, produced);
    total += produced;
    return rc;
  };
  const u64 root[2] = {0, ix->img.n - 1};
  const int rc = kmer_walk_root(w, root);
  if(rc != GCSA2_OK) { return rc; }
  *result = total;
  return GCSA2_OK;
}

// compareKMers(left, right, k, parameters) (src/algorithms.cpp:534-616).  With record buffers the states of
// the unique k-mers are returned as the reference dumps them to output.left / output.right (:606-610).
namespace {

// The same walk over pairs of ranges (4 u64 per state; with records also the 3-u64 keys): a frontier of any size, where
// round 3 refused more than 2^27 / limit states.  counters: word 0 is the walk's cursor, 1 .. 3 are the last level's shared /
// left-only / right-only children.
int compare_kmers_impl(const gcsa2_index* left, const gcsa2_index* right, uint64_t k, int include_ns, int force, uint64_t* result,
                       uint64_t* left_records, uint64_t left_capacity, uint64_t* right_records, uint64_t right_capacity, bool records)
{
  CHECK_INDEX(left); CHECK_INDEX(right);
  if(result == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null result"); }
  result[0] = result[1] = result[2] = 0;
  if(k == 0) { result[0] = 1; return GCSA2_OK; }                                            // :539
  if((k > left->order || k > right->order) && !force) { return GCSA2_OK; }                   // :540-549
  if(k > 64) { return GCSA2_OK; }                                                            // :550-554 (MAX_K)
  if(left->img.sigma != right->img.sigma || left->img.fast_chars != right->img.fast_chars) { return GCSA2_OK; }   // :556-560
  if(left->device != right->device) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "both indexes must live on the same device"); }
  if(left->img.n == 0 || right->img.n == 0 || left->img.sigma < 3) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "empty index or alphabet too small"); }
  try {
  DeviceGuard guard(left->device);
  DBuf<DevImage> images; DBuf<unsigned long long> counters;
  HIP_TRY(images.alloc(2)); HIP_TRY(counters.alloc(4));
  HIP_TRY(hipMemcpy(images.p, &left->img, sizeof(DevImage), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(images.p + 1, &right->img, sizeof(DevImage), hipMemcpyHostToDevice));
  u64 shared = 0, left_only = 0, right_only = 0;       // totals (the unique ones count on even when their records no longer fit)
  KmerWalk w{k, kmer_limit(left, include_ns), left->tune.kmer_piece, 0, 4, records, nullptr, counters.p};
  const auto launch = [&](const u64* frontier, const u64* keys, u64 n, u64 depth, int mode, u64* next, u64* next_keys, u64* d_left, u64* d_right) -> int
  {
    hipLaunchKernelGGL(k_kmer_compare, dim3(grid_for(n)), dim3(TPB), 0, w.st, images.p, images.p + 1, frontier, keys, n, w.limit, u32(depth), mode,
                       next, next_keys, counters.p, d_left, d_right);
    LAUNCH_CHECK("k_kmer_compare");
    return GCSA2_OK;
  };
  w.expand = [&](const u64* frontier, const u64* keys, u64 n, u64 depth, u64* next, u64* next_keys, u64) -> int
  {
    return launch(frontier, keys, n, depth, 0, next, next_keys, nullptr, nullptr);
  };
  w.leaf = [&](const u64* frontier, const u64* keys, u64 n, u64 depth) -> int      // classify the children; any size
  {
    unsigned long long found[3] = {0, 0, 0};
    HIP_TRY(hipMemset(counters.p + 1, 0, sizeof(found)));
    int rc = launch(frontier, keys, n, depth, 1, nullptr, nullptr, nullptr, nullptr);
    if(rc != GCSA2_OK) { return rc; }
    HIP_TRY(hipMemcpy(found, counters.p + 1, sizeof(found), hipMemcpyDeviceToHost));
    const u64 l = found[1], r = found[2];
    if(records && (l > 0 || r > 0) && left_only + l <= left_capacity && right_only + r <= right_capacity)
    {
      DBuf<u64> d_left, d_right;
      HIP_TRY(d_left.alloc(8 * l)); HIP_TRY(d_right.alloc(8 * r));
      HIP_TRY(hipMemset(counters.p + 1, 0, sizeof(found)));
      rc = launch(frontier, keys, n, depth, 2, nullptr, nullptr, d_left.p, d_right.p);
      if(rc != GCSA2_OK) { return rc; }
      if(l > 0) { HIP_TRY(hipMemcpy(left_records + 8 * left_only, d_left.p, 8 * l * sizeof(u64), hipMemcpyDeviceToHost)); }
      if(r > 0) { HIP_TRY(hipMemcpy(right_records + 8 * right_only, d_right.p, 8 * r * sizeof(u64), hipMemcpyDeviceToHost)); }
    }
    shared += found[0]; left_only += l; right_only += r;
    return GCSA2_OK;
  };
  const u64 root[4] = {0, left->img.n - 1, 0, right->img.n - 1};
  const int rc = kmer_walk_root(w, root);
  if(rc != GCSA2_OK) { return rc; }
  result[0] = shared; result[1] = left_only; result[2] = right_only;
  if(records && (result[1] > left_capacity || result[2] > right_capacity)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "record buffers smaller than result[1] / result[2]"); }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("compareKMers: ") + e.what()); }
}

} // namespace

extern "C" int gcsa2_compare_kmers(const gcsa2_index* left, const gcsa2_index* right, uint64_t k, int include_ns, int force,
                                   uint64_t* result)
{
  return compare_kmers_impl(left, right, k, include_ns, force, result, nullptr, 0, nullptr, 0, false);
}

extern "C" int gcsa2_compare_kmers_records(const gcsa2_index* left, const gcsa2_index* right, uint64_t k, int include_ns, int force,
                                           uint64_t* result, uint64_t* left_records, uint64_t left_capacity,
                                           uint64_t* right_records, uint64_t right_capacity)
{
  if((left_records == nullptr && left_capacity > 0) || (right_records == nullptr && right_capacity > 0)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null record buffer"); }
  return compare_kmers_impl(left, right, k, include_ns, force, result, left_records, left_capacity, right_records, right_capacity, true);
}

// ==== index k-mer spectrum: the k-mers of the index itself, binned, listed or summed per graph node ====
namespace {

// what the three calls refuse before any device is touched
int spectrum_checks(const gcsa2_index* ix, u64 k, int flags, int known_flags, const char* name)
{
  CHECK_INDEX(ix);
  if(k == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, std::string(name) + ": k must be at least 1"); }
  if((flags & ~known_flags) != 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, std::string(name) + ": unknown flags"); }
  if(ix->img.sigma < 3) { return fail(GCSA2_ERR_INVALID_ARGUMENT, std::string(name) + ": alphabet too small for countKMers"); }
  return GCSA2_OK;
}

int spectrum_counters(const gcsa2_index* ix, int flags, const char* name)
{
  if((flags & GCSA2_SPECTRUM_COUNTS) != 0 && !ix->img.has_counters)
  {
    return fail(GCSA2_ERR_MISSING_COMPONENT, std::string(name) + ": GCSA2_SPECTRUM_COUNTS on an index that was created without counters");
  }
  return GCSA2_OK;
}

constexpr u64 SPECTRUM_EMIT_PIECE = u64(1) << 24;     // records of one piece: 1 GB of gcsa2_index_kmer, 0.8 GB of gcsa2_mem and counts

// GCSA2_SPECTRUM_GROUPS (a test knob, read per call): the workgroups of k_spectrum_leaf, each of which takes every
// gridDim.x-th tile of 256 states.  The result never depends on it.
u64 spectrum_leaf_groups(const gcsa2_index* ix)
{
  u64 groups = u64(ix->compute_units) * SPECTRUM_LEAF_GROUPS_PER_CU, v = 0;
  if(env_count("GCSA2_SPECTRUM_GROUPS", &v) && v >= 1) { groups = v; }
  return std::min(groups, u64(1) << 31);
}

// The walk of the spectrum calls, on the caller's stream.  The levels above the last are k_kmer_expand, with keys in the list
// mode; the last is k_spectrum_leaf on the parents at depth k - 1.  SPEC_HISTOGRAM: the last level needs no buffer and takes a
// frontier of any size.  The emitting modes cut the last level too, so that the children of a piece -- at most
// min(kmer_piece, SPECTRUM_EMIT_PIECE) -- fit the record buffer, and hand every piece's m > 0 records (and, SPEC_SEEDS, their
// count()s) to `sink` before the next piece overwrites them.
// stat is SPEC_WORDS words at the end of which the five sums stand (read them after the stream has been waited for: the last
// leaf kernel of the histogram mode is left in flight).
struct Spectrum
{
  const gcsa2_index* ix; hipStream_t st; u32 limit; u64 k; int mode; int counts;
  unsigned long long* stat; unsigned long long* hist; u64 n_hist; u64 min_value, max_value;
  std::function<int(const u64* d_recs, const u64* d_counts, u64 m)> sink;
};

int spectrum_walk(const Spectrum& c)
{
  const bool with_keys = (c.mode == SPEC_LIST);
  KmerBufs records, record_counts;
  KmerWalk w{c.k, c.limit, c.ix->tune.kmer_piece, (c.mode == SPEC_HISTOGRAM ? 0 : std::min<u64>(c.ix->tune.kmer_piece, SPECTRUM_EMIT_PIECE)), 2,
             with_keys, c.st, c.stat + SPEC_CURSOR};
  w.expand = [&](const u64* frontier, const u64* keys, u64 n, u64 depth, u64* next, u64* next_keys, u64 room) -> int
  {
    if(with_keys)
    {
      hipLaunchKernelGGL((k_kmer_expand<true>), dim3(grid_for(n)), dim3(TPB), 0, c.st, c.ix->img, frontier, keys, n, c.limit, u32(depth), next, next_keys,
                         room, w.cursor);
    }
    else
    {
      hipLaunchKernelGGL((k_kmer_expand<false>), dim3(grid_for(n)), dim3(TPB), 0, c.st, c.ix->img, frontier, keys, n, c.limit, u32(depth), next, next_keys,
                         room, w.cursor);
    }
    LAUNCH_CHECK("k_kmer_expand");
    return GCSA2_OK;
  };
  w.leaf = [&](const u64* frontier, const u64* keys, u64 n, u64 depth) -> int
  {
    const u64 room = n * c.limit;
    u64 *recs = nullptr, *rec_counts = nullptr, produced = 0;
    const dim3 leaf_grid(unsigned(std::min<u64>((n + TPB - 1) / TPB, spectrum_leaf_groups(c.ix))));
    int rc = kmer_cursor_clear(w);
    if(rc != GCSA2_OK) { return rc; }
    if(c.mode == SPEC_HISTOGRAM)
    {
      hipLaunchKernelGGL((k_spectrum_leaf<SPEC_HISTOGRAM>), leaf_grid, dim3(TPB), 0, c.st, c.ix->img, frontier, keys, n, c.limit, u32(depth),
                         c.counts, c.hist, c.n_hist, c.stat, u64(0), u64(0), recs, rec_counts, u64(0));
      LAUNCH_CHECK("k_spectrum_leaf");
      return GCSA2_OK;
    }
    if(c.mode == SPEC_SEEDS)
    {
      HIP_TRY(records.get(0, size_t(room * 5 * sizeof(u64)), recs));
      HIP_TRY(record_counts.get(0, size_t(room * sizeof(u64)), rec_counts));
      hipLaunchKernelGGL((k_spectrum_leaf<SPEC_SEEDS>), leaf_grid, dim3(TPB), 0, c.st, c.ix->img, frontier, keys, n, c.limit, u32(depth),
                         c.counts, c.hist, c.n_hist, c.stat, u64(0), u64(0), recs, rec_counts, room);
    }
    else
    {
      HIP_TRY(records.get(0, size_t(room * 8 * sizeof(u64)), recs));
      hipLaunchKernelGGL((k_spectrum_leaf<SPEC_LIST>), leaf_grid, dim3(TPB), 0, c.st, c.ix->img, frontier, keys, n, c.limit, u32(depth),
                         c.counts, c.hist, c.n_hist, c.stat, c.min_value, c.max_value, recs, rec_counts, room);
    }
    LAUNCH_CHECK("k_spectrum_leaf");
    rc = kmer_cursor_read(w, produced);
    if(rc != GCSA2_OK) { return rc; }
    if(produced > room) { return fail(GCSA2_ERR_HIP, "k-mer spectrum: more records than a piece has room for"); }
    return (produced > 0 ? c.sink(recs, rec_counts, produced) : GCSA2_OK);
  };
  HIP_TRY(hipMemsetAsync(c.stat, 0, SPEC_WORDS * sizeof(unsigned long long), c.st));
  const u64 root[2] = {0, c.ix->img.n - 1};
  return kmer_walk_root(w, root);
}

}  // namespace

extern "C" {

int gcsa2_kmer_spectrum(const gcsa2_index* ix, uint64_t k, int include_ns, int force, int flags, uint64_t* histogram, uint64_t n_hist,
                        gcsa2_spectrum_stats* stats)
{
  int rc = spectrum_checks(ix, k, flags, GCSA2_SPECTRUM_COUNTS, "kmer_spectrum");
  if(rc != GCSA2_OK) { return rc; }
  if(histogram == nullptr && n_hist > 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_spectrum: histogram is NULL with n_hist > 0"); }
  rc = spectrum_counters(ix, flags, "kmer_spectrum");
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  g_error.clear();
  for(u64 i = 0; i < n_hist; i++) { histogram[i] = 0; }
  gcsa2_spectrum_stats sums{};
  if(stats != nullptr) { *stats = sums; }
  if(kmer_nothing(ix, k, force)) { return GCSA2_OK; }
  DeviceGuard guard(ix->device);
  DBuf<unsigned long long> stat, hist;
  HIP_TRY(stat.alloc(SPEC_WORDS));
  if(n_hist > 0) { HIP_TRY(hist.alloc(n_hist)); HIP_TRY(hipMemset(hist.p, 0, n_hist * sizeof(unsigned long long))); }
  rc = spectrum_walk(Spectrum{ix, nullptr, kmer_limit(ix, include_ns), k, SPEC_HISTOGRAM, int((flags & GCSA2_SPECTRUM_COUNTS) != 0), stat.p,
                              (n_hist > 0 ? hist.p : nullptr), n_hist, 0, 0, nullptr});
  if(rc != GCSA2_OK) { return rc; }
  unsigned long long host_stat[SPEC_WORDS];
  HIP_TRY(hipMemcpy(host_stat, stat.p, sizeof(host_stat), hipMemcpyDeviceToHost));
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the histogram is copied as it stands");
  if(n_hist > 0) { HIP_TRY(hipMemcpy(histogram, hist.p, n_hist * sizeof(u64), hipMemcpyDeviceToHost)); }
  sums.kmers = host_stat[SPEC_KMERS]; sums.nodes = host_stat[SPEC_NODES]; sums.occurrences = host_stat[SPEC_OCCURRENCES];
  sums.unique = host_stat[SPEC_UNIQUE]; sums.max_value = host_stat[SPEC_MAX];
  if(stats != nullptr) { *stats = sums; }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_kmer_spectrum: ") + e.what()); }
}

int gcsa2_list_kmers(const gcsa2_index* ix, uint64_t k, int include_ns, int force, int flags, uint64_t min_value, uint64_t max_value,
                     gcsa2_index_kmer* records, uint64_t capacity, uint64_t* total)
{
  int rc = spectrum_checks(ix, k, flags, GCSA2_SPECTRUM_COUNTS, "list_kmers");
  if(rc != GCSA2_OK) { return rc; }
  if(total == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "list_kmers: total is NULL"); }
  if(k > 64) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "list_kmers: k must be at most 64 (the key holds 64 steps)"); }
  if(max_value != 0 && min_value > max_value) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "list_kmers: min_value exceeds max_value"); }
  if(records == nullptr && capacity > 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "list_kmers: records is NULL with capacity > 0"); }
  rc = spectrum_counters(ix, flags, "list_kmers");
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  g_error.clear();
  *total = 0;
  if(kmer_nothing(ix, k, force)) { return GCSA2_OK; }
  static_assert(sizeof(gcsa2_index_kmer) == 8 * sizeof(u64), "gcsa2_index_kmer is eight words");
  DeviceGuard guard(ix->device);
  DBuf<unsigned long long> stat;
  HIP_TRY(stat.alloc(SPEC_WORDS));
  u64 listed = 0;
  Spectrum run{ix, nullptr, kmer_limit(ix, include_ns), k, SPEC_LIST, int((flags & GCSA2_SPECTRUM_COUNTS) != 0), stat.p, nullptr, 0,
               min_value, max_value, nullptr};
  run.sink = [&](const u64* d_recs, const u64*, u64 m) -> int     // a piece that no longer fits is counted, not copied
  {
    if(listed + m <= capacity) { HIP_TRY(hipMemcpy(records + listed, d_recs, m * sizeof(gcsa2_index_kmer), hipMemcpyDeviceToHost)); }
    listed += m;
    return GCSA2_OK;
  };
  rc = spectrum_walk(run);
  if(rc != GCSA2_OK) { return rc; }
  *total = listed;
  if(listed > capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "list_kmers: capacity is smaller than *total"); }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_list_kmers: ") + e.what()); }
}

int gcsa2_index_kmer_support_device(const gcsa2_index* ix, uint64_t k, int include_ns, int force, uint64_t hit_max, uint64_t shift, int flags,
                                    uint64_t* d_support, uint64_t n_bins, gcsa2_support_stats* stats, void* stream)
{
  CHECK_INDEX(ix);
  if(k == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "index_kmer_support: k must be at least 1"); }
  if(ix->img.sigma < 3) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "index_kmer_support: alphabet too small for countKMers"); }
  int rc = support_checks(ix, shift, flags, d_support, n_bins, "d_support");
  if(rc != GCSA2_OK) { return rc; }
  gcsa2_support_stats sums{};
  if(kmer_nothing(ix, k, force)) { if(stats != nullptr) { *stats = sums; } return GCSA2_OK; }
  try {   // no C++ exception may cross the C boundary
  g_error.clear();
  DeviceGuard guard(ix->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  DBuf<unsigned long long> stat;
  HIP_TRY(stat.alloc(SPEC_WORDS));
  Spectrum run{ix, st, kmer_limit(ix, include_ns), k, SPEC_SEEDS, 1, stat.p, nullptr, 0, 0, 0, nullptr};
  run.sink = [&](const u64* d_recs, const u64* d_counts, u64 m) -> int       // one piece: the core of gcsa2_seed_support_device
  {
    gcsa2_support_stats piece{};
    Scratch scratch(ix, st);
    const int piece_rc = support_tail(ix, d_recs, 5, d_counts, nullptr, m, hit_max, shift, flags, d_support, n_bins, &piece, scratch, st);
    if(piece_rc != GCSA2_OK) { return piece_rc; }
    sums.windows += m; sums.found += piece.found; sums.counted += piece.counted; sums.distinct += piece.distinct;
    sums.values += piece.values; sums.added += piece.added; sums.dropped += piece.dropped;
    return GCSA2_OK;
  };
  rc = spectrum_walk(run);
  if(rc == GCSA2_OK && stats != nullptr) { *stats = sums; }
  return rc;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_index_kmer_support_device: ") + e.what()); }
}

}  // extern "C"
