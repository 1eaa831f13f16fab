// gcsa2_hip.hip -- MI355X (gfx950) batched backward-search engine for GCSA2 indexes:
// kernels + the C ABI of include/gcsa2_hip.h.  Written for CDNA4 only (wave64, no CUDA paths).
//
// One translation unit: the device code lives in kernels_*.hpp, this file holds the host side
// (device image staging, handles, launches, the extern "C" entry points); what carries a batch in host memory to the
// kernels and back is in host_batch.hpp, the index-side k-mer calls in host_kmers.hpp.
//
// Kernel <-> reference map (paths relative to the reference tree):
//   kernels_find.hpp    k_find2 / k_find      GCSA::find                 include/gcsa/gcsa.h:96-110
//                       k_lf2                 GCSA::LF(range, comp)      include/gcsa/gcsa.h:155-162, 262-274
//                       k_lf_node             GCSA::LF(path_node)        include/gcsa/gcsa.h:165-183
//                       k_lf_all              GCSA::LF_fast / LF_all     src/gcsa.cpp:742-798
//   kernels_locate.hpp  k_count               GCSA::count, Sada*::count  src/gcsa.cpp:802-809, support.h:255-258,329-335
//                       k_locate_*            GCSA::locate(range), locateInternal, removeDuplicates
//                                                                        src/gcsa.cpp:827-842, 880-896, utils.h:350-357
//   kernels_mem.hpp     k_mem_*               a MEM finder's count() + locate() per match (vg's seeding), src/gcsa.cpp:802-878
//   kernels_minimizers.hpp k_minimizers      the (w, k)-minimizers of every read (gcsa2_minimizers_device)
//                       k_minimizer_seeds     k_kmer_seeds over the selected windows (gcsa2_minimizer_hits_device)
//   kernels_strands.hpp k_canonical_minimizers the same selection by the smaller hash of a window and its reverse complement
//                       k_strand_windows      the minimizer CSR as the searched windows of both strands, as 64-bit keys
//                       k_strand_seeds        k_kmer_seeds over such keys (gcsa2_stranded_minimizer_hits_device)
//   kernels_windows.hpp k_kmer_windows        GCSA::find + GCSA::count of every k-mer window of every read, per-read sums
//                       k_kmer_seeds          the same search, emitting the found windows as seed records (gcsa2_kmer_hits_device)
//                                                                        include/gcsa/gcsa.h:96-110, src/gcsa.cpp:802-809
//   kernels_seeds.hpp   k_capped_seeds        GCSA::LF(range, comp) + GCSA::count per step: the shortest matches under an occurrence cap
//                                                                        include/gcsa/gcsa.h:155-162, src/gcsa.cpp:802-809
//   kernels_support.hpp k_support_*           GCSA::locate(range) of every distinct range of a batch, summed per node id (no counterpart)
//   kernels_classes.hpp k_classes_*           the same ranges, voted per read over classes of node ids (no counterpart)
//   kernels_clusters.hpp k_clusters_*         per read the top diagonal bands of its seed hits (no counterpart)
//   kernels_chains.hpp  k_chains_*            per read the top colinear chains of its seed hits (no counterpart)
//   kernels_pairs.hpp   k_chain_pairs         per read pair the top placements of two mates' chains under a fragment model (no counterpart)
//                                                                        src/gcsa.cpp:827-842
//   kernels_kmers.hpp   k_kmer_expand         countKMers                 src/algorithms.cpp:364-421
//                       k_kmer_compare        compareKMers               src/algorithms.cpp:505-616
//                       k_spectrum_leaf       the last level of the same tree with count() / Range::length per k-mer: histogram, list,
//                                             seed records for k_support_*  src/algorithms.cpp:364-421, src/gcsa.cpp:802-809
//   kernels_lcp.hpp    k_parent / k_depth / k_sv / k_rmq   LCPArray     include/gcsa/lcp.h:137-178, src/lcp.cpp:276-519
#include "layout.hpp"
#include "sdsl_reader.hpp"
#include "sdsl_writer.hpp"
#include "../../include/gcsa2_hip.h"
#include "../../include/gcsa2_hip_chains.h"
#include "../../include/gcsa2_hip_strands.h"
#include "../../include/gcsa2_hip_pairs.h"

#include <hipcub/hipcub.hpp>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <functional>
#include <atomic>
#include <memory>
#include <mutex>
#include <new>
#include <random>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_set>
#include <vector>

using namespace g2;

#include "kernels_common.hpp"
#include "kernels_find.hpp"
#include "kernels_extend.hpp"
#include "kernels_locate.hpp"
#include "kernels_locate_max.hpp"
#include "kernels_mem.hpp"
#include "kernels_windows.hpp"
#include "kernels_minimizers.hpp"
#include "kernels_strands.hpp"
#include "kernels_lcp.hpp"
#include "kernels_submem.hpp"
#include "kernels_seeds.hpp"
#include "kernels_support.hpp"
#include "kernels_classes.hpp"
#include "kernels_clusters.hpp"
#include "kernels_chains.hpp"
#include "kernels_pairs.hpp"
#include "kernels_kmers.hpp"
#include "kernels_mailbox.hpp"
#include "kernels_build.hpp"

// ==========================================================================================
// host code

constexpr unsigned RESULT_SLOTS = 1024;     // concurrent locate calls per handle before two share a slot

// Staging of the host-pointer entry points (`*_batch`): a stream, a grow-only device arena and a pinned host arena.
// A handle keeps a small pool of them, one per concurrent caller, so that a call costs no hipMalloc / hipFree
// and small transfers go through pinned memory asynchronously on the call's own stream.
struct Staging
{
  hipStream_t stream = nullptr;
  char* d = nullptr; size_t d_cap = 0;
  char* h = nullptr; size_t h_cap = 0;       // pinned (hipHostMalloc)
  char* z = nullptr;                         // pinned, coherent, ZERO_COPY_ARENA bytes: kernels of small calls read and write it directly
};

struct gcsa2_index
{
  int device = 0;
  DevImage img;
  void* d_base = nullptr;
  void* d_kmer = nullptr;
  void* d_pred4 = nullptr;
  void* d_locate = nullptr;
  void* d_jump = nullptr;
  void* d_pairs = nullptr;
  hipMemPool_t pool = nullptr;   // stream-ordered scratch of the query pipelines (owned; the default pool is not touched)
  // Small results the host reads back (totals of the locate pipeline) live in per-handle slots, not in per-call
  // scratch: no allocation per call.  (Round 1 moved them here after stale read-backs out of pool memory, about one
  // call in 5000; tools/hip/pool_readback_repro.hip shows the ROCm pool itself delivers 1.1 M such read-backs
  // correctly in every stream / host-memory combination, so that symptom was this engine's then-code, not ROCm.)
  unsigned long long* d_slots = nullptr;
  unsigned long long* h_slots = nullptr;     // the same slots in page-locked host memory the device writes and the host polls (read_totals)
  mutable std::atomic<unsigned> next_slot{0};
  mutable std::atomic<unsigned long long> next_ticket{1};
  mutable std::atomic<int> single_backoff{0};     // locate(): calls that skip the one-kernel attempt after it met a misfit (locate_chunk)
  // the resident wavefront that answers scalar calls (kernels_mailbox.hpp): its slot in page-locked memory, its stream
  struct Mailbox { MailSlot* slot = nullptr; hipStream_t stream = nullptr; std::mutex lock; unsigned long long ticket = 0, launches = 0, calls = 0; bool failed = false; };
  mutable Mailbox mail;
  mutable std::mutex staging_lock;
  mutable std::vector<Staging*> staging_pool;
  int compute_units = 256;
  u64 bytes = 0;
  u64 order = 0;
  // Host pipeline of the large host-pointer batches (gcsa2_find_batch): PIPE_LANES host threads, each with two pinned + device
  // staging sets and a stream of its own, made at the first large batch and kept (one pipelined call at a time per handle).
  struct PipeSet { char* h = nullptr; char* d = nullptr; hipEvent_t done = nullptr; bool busy = false; u64 first = 0, count = 0; };
  // uploads, kernel and downloads on the lane's one stream: a download stream of its own per lane lost, 0.86 -> 0.51 G queries/s
  struct PipeLane { hipStream_t stream = nullptr; PipeSet set[2]; };
  mutable std::mutex pipe_lock;
  mutable std::vector<PipeLane> pipe;
  // scratch arenas of the locate pipeline that are not in use (struct Scratch)
  struct Arena { char* base = nullptr; size_t bytes = 0; };
  mutable std::mutex arena_lock;
  mutable std::vector<Arena> arenas;
  // tuning knobs, read from the environment ONCE, when the index is created (A/B measurements; results never depend on them)
  struct Tuning
  {
    u32 cool_down = COOL_DOWN;         // GCSA2_COOL_DOWN: characters stepped singly after a step that needed parent()
    u32 ms_refill_at = MS_REFILL_AT;   // GCSA2_MS_REFILL_AT: persistent matching statistics, idle lanes of a wave that trigger a refill
    u64 ms_grid = 0;                   // GCSA2_MS_GRID: ... most workgroups launched (0: what the device holds at once)
    u64 locate_split = (u64(1) << 31) - 1;   // GCSA2_LOCATE_SPLIT: most values (before deduplication) one pass of the locate pipeline handles
    u64 locate_split_queries = u64(1) << 30; // GCSA2_LOCATE_SPLIT_QUERIES: most ranges one pass handles (its lists and grids are 32-bit)
    u64 pipe_chunk = u64(1) << 18;     // GCSA2_PIPE_CHUNK (log2): patterns per chunk of the host pipeline
    u32 pipe_lanes = 6;                // GCSA2_PIPE_LANES: host threads (each with its streams and staging sets) of the large host batches
    u32 ms_threads = 4;                   // GCSA2_MS_THREADS: host threads (one stream each) that send the pieces
    u64 kmer_piece = u64(1) << 27;        // GCSA2_KMER_PIECE (tests): children of one piece of a countKMers / compareKMers frontier
    u64 ms_piece_bytes = u64(32) << 20;   // GCSA2_MS_PIECE_MB: pattern bytes per piece of the large host batches of matching statistics / break points
    bool pipe_blocking = false;        // GCSA2_PIPE_BLOCKING=1: the lanes' events are made with hipEventBlockingSync
    bool ms_pieces = true;             // GCSA2_MS_PIECES=0: large host batches of matching statistics go through one copy in, one launch, one copy out
    bool zero_copy = true;             // GCSA2_ZERO_COPY=0: small host-pointer calls copy through the arenas like large ones
    u32 seed_wide = (u32(1) << 24) - 1;   // GCSA2_SEED_WIDE: seed-table entries of this many path nodes or more are marked, not stored (tests)
    bool locate_trace = false;         // GCSA2_LOCATE_TRACE=1: host-clock stamps of a locate pass on stderr (profiles/r04_locate.md)
    u32 split_target = SPLIT_TARGET;   // GCSA2_SPLIT_TARGET (tests): values per bucket k_over_split aims at
    u32 split_skew = BIG_SEGMENT;      // GCSA2_SPLIT_SKEW (tests): buckets of more values than this count as skewed and go to the radix sort
    bool locate_fused_compact = true;  // GCSA2_LOCATE_FUSED_COMPACT=0: caller-owned buffers also take the four-kernel compaction of the job interface (A/B)
    bool locate_single = true;         // GCSA2_LOCATE_SINGLE=0: batches of one-value ranges go through the general locate pipeline too (A/B)
    bool locate_fuse = true;           // GCSA2_LOCATE_FUSE=0: wide ranges of one-value path nodes go through the table pass like the others (A/B; round 6)
    u64 fuse_above = BIG_SEGMENT;      // GCSA2_LOCATE_FUSE_ABOVE (tests): path nodes from which such a range is a candidate for the fused split
    bool mailbox = true;               // GCSA2_MAILBOX=0: one-query calls of LF / count / parent / LF(node) take the launch path like any batch (A/B; round 6)
    u64 mailbox_park_us = 200;         // GCSA2_MAILBOX_PARK_US: the resident wavefront leaves after this long without a request
    u64 mailbox_life_ms = 20;          // GCSA2_MAILBOX_LIFE_MS: ... and after this long whatever happens (the next call launches it again)
    bool locate_in_place = true;       // GCSA2_LOCATE_IN_PLACE=0: caller-owned buffers that hold the raw values are not used as the sort's target (A/B; round 6)
    size_t arena_cap = size_t(24) << 30;  // GCSA2_ARENA_CAP_MB: most scratch a handle keeps between calls per arena (struct Scratch)
    u64 budget_bytes = 0;              // GCSA2_MEMORY_BUDGET_MB: most device memory the image may take (0: what the device has free)
  } tune;
};

struct gcsa2_locate_job
{
  int device = 0;
  u64 nq = 0, total = 0;
  u64* d_offsets = nullptr;   // nq + 1
  u64* d_values = nullptr;    // total
  hipStream_t stream = nullptr;   // the stream the job ran on
};

namespace {

thread_local std::string g_error;

int fail(int code, const std::string& msg) { g_error = msg; return code; }

// A knob that is a count: the whole string a decimal number.  false: unset, empty or anything else (*v is then untouched).
bool env_count(const char* name, u64* v)
{
  const char* env = std::getenv(name);
  if(env == nullptr || *env == 0) { return false; }
  char* end = nullptr;
  const unsigned long long got = std::strtoull(env, &end, 10);
  if(end == env || *end != 0) { return false; }
  *v = got;
  return true;
}

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if(e_ != hipSuccess) { \
  return fail(e_ == hipErrorOutOfMemory ? GCSA2_ERR_OUT_OF_MEMORY : GCSA2_ERR_HIP, \
              std::string(#expr) + ": " + hipGetErrorString(e_)); } } while(0)

inline unsigned grid_for(u64 n) { return unsigned((n + TPB - 1) / TPB); }

// what a memory budget (GCSA2_MEMORY_BUDGET_MB, read at create time) leaves for the next optional table
inline u64 budget_left(const gcsa2_index* ix) { return ix->tune.budget_bytes > ix->bytes ? ix->tune.budget_bytes - ix->bytes : 0; }

// The jump table of a find-only image is built without being asked for (gcsa2_index_create).
constexpr bool JUMP_DEFAULT_FIND_ONLY = true;
// Free-memory test of the jump table, the largest optional table (16 bytes per path node; the others take a fraction
// of what is free): `bytes` more must leave a sixteenth of the device's memory free for the caller's batches and the
// handle's scratch pool -- 18 GB of a 288 GB device, where the 91.6 GB table of a 5.73 G-node index goes on top of a 175 GB image.
inline bool jump_table_fits(u64 bytes, u64 free_bytes, u64 total_bytes) { return bytes <= free_bytes && free_bytes - bytes >= total_bytes / 16; }
// Steps behind the middle node slot of a jump entry (DevImage::jump_mid).  6 saves a lookup on chain tails of 6 and 7
// characters and leaves tails of 2 and 3 to the pair step; that pays where a lookup is an HBM request, i.e. where the
// table does not stay in the last-level cache (the 256 MiB Infinity Cache), and where a pair step exists to take two
// characters in one request.  Everywhere else the entry keeps the node after 2 steps.
constexpr u64 LAST_LEVEL_CACHE_BYTES = u64(256) << 20;
inline u32 jump_mid_default(u64 nodes, bool pair_blocks) { return pair_blocks && nodes * sizeof(ulonglong2) > LAST_LEVEL_CACHE_BYTES ? 6 : 2; }
// Branch records (DevImage::jump_branch) save a block fetch at a two-label node for a lookup that lands on it: a trade of
// requests, which pays under the same rule, and they need the two free slots that only jump_mid = 6 leaves in a short entry.
inline bool jump_branch_default(u64 nodes, bool pair_blocks) { return jump_mid_default(nodes, pair_blocks) == 6; }

inline void launch_walk(const gcsa2_index* ix, const u64* d_ranges, u64 nq, const u64* node_off, const u64* raw_off,
                        u64 total_nodes, u64* values, u64* owners, hipStream_t stream);

// ---- the optional tables of an image (pair blocks, k-mer seed table, locate table): built at create time and again by
// gcsa2_index_set_tables.  Each maker leaves the image without the table when it fails.

inline u64 pair_block_bytes_of(const DevImage& img) { return 16 * (img.n / PAIR_BITS + 1) * FLB_BYTES; }
inline bool pair_blocks_possible(const DevImage& img) { return img.sigma >= 5 && img.n > 0 && 16 * (img.n / PAIR_BITS + 1) < u64(PAIR_FLAG); }
inline bool seed_table_possible(const DevImage& img) { return img.sigma >= 5 && (img.n > img.e ? img.n : img.e) + 2 < (u64(1) << SEED_SP_BITS); }
inline bool locate_table_possible(const DevImage& img) { return img.has_samples && img.pred4 != nullptr && img.n > 0; }

void drop_pair_blocks(gcsa2_index* ix)
{
  if(ix->d_pairs != nullptr) { (void)hipFree(ix->d_pairs); ix->d_pairs = nullptr; ix->bytes -= pair_block_bytes_of(ix->img); }
  ix->img.flp = nullptr; ix->img.flp_nblocks = 0;
}

hipError_t make_pair_blocks(gcsa2_index* ix)
{
  drop_pair_blocks(ix);
  DevImage& img = ix->img;
  const u64 nb = img.n / PAIR_BITS + 1, pair_bytes = pair_block_bytes_of(img);
  hipError_t e = hipMalloc(&ix->d_pairs, pair_bytes);
  if(e == hipSuccess)
  {
    img.flp_nblocks = nb;
    const u64 slice = u64(1) << 20;          // blocks per launch: 2^20 x 4 workgroups of 192 threads
    for(u64 first = 0; first < nb && e == hipSuccess; first += slice)
    {
      const u64 count = (nb - first < slice ? nb - first : slice);
      hipLaunchKernelGGL(k_build_pair_blocks, dim3(unsigned(count), 4), dim3(unsigned(PAIR_BITS)), 0, nullptr, img, first, static_cast<u64*>(ix->d_pairs));
      e = hipGetLastError();
    }
    if(e == hipSuccess) { e = hipDeviceSynchronize(); }
  }
  if(e != hipSuccess)
  {
    if(ix->d_pairs != nullptr) { (void)hipFree(ix->d_pairs); ix->d_pairs = nullptr; }
    img.flp_nblocks = 0; (void)hipGetLastError();
    return e;
  }
  img.flp = static_cast<const u64*>(ix->d_pairs);
  ix->bytes += pair_bytes;
  return hipSuccess;
}

void drop_seed_table(gcsa2_index* ix)
{
  if(ix->d_kmer != nullptr) { (void)hipFree(ix->d_kmer); ix->d_kmer = nullptr; ix->bytes -= u64(8) << (2 * ix->img.kmer_k); }
  ix->img.kmer_table = nullptr; ix->img.kmer_k = 0;
}

// find() of every k-mer over comps 1..4, level by level in place (kernels_find.hpp: k_seed_level); 1 <= k <= 16
hipError_t make_seed_table(gcsa2_index* ix, u32 k)
{
  drop_seed_table(ix);
  DevImage& img = ix->img;
  img.seed_wide = ix->tune.seed_wide;
  const u64 entry_bytes = 8, entries = u64(1) << (2 * k);
  hipError_t e = hipMalloc(&ix->d_kmer, entries * entry_bytes);
  const u64 slice = u64(1) << 30;            // a HIP grid holds < 2^32 threads
  for(u32 j = 0; j < k && e == hipSuccess; j++)
  {
    // level j + 1 from level j: first the quarters with a non-zero leading code, then level j in place
    const u64 have = u64(1) << (2 * j), want = have << 2;
    for(int pass = 0; pass < 2 && e == hipSuccess; pass++)
    {
      const u64 lo = (j == 0 ? 0 : (pass == 0 ? have : 0)), hi = (j == 0 ? (pass == 0 ? want : 0) : (pass == 0 ? want : have));
      for(u64 first = lo; first < hi && e == hipSuccess; first += slice)
      {
        u64 count = (hi - first < slice ? hi - first : slice);
        hipLaunchKernelGGL(k_seed_level, dim3(grid_for(count)), dim3(TPB), 0, nullptr, img, j, first, first + count, static_cast<u64*>(ix->d_kmer));
        e = hipGetLastError();
      }
    }
  }
  if(e == hipSuccess) { e = hipDeviceSynchronize(); }
  if(e != hipSuccess)
  {
    if(ix->d_kmer != nullptr) { (void)hipFree(ix->d_kmer); ix->d_kmer = nullptr; }
    (void)hipGetLastError();
    return e;
  }
  img.kmer_table = static_cast<const u64*>(ix->d_kmer); img.kmer_k = k;
  ix->bytes += entries * entry_bytes;
  return hipSuccess;
}

void drop_locate_table(gcsa2_index* ix)
{
  if(ix->d_locate != nullptr) { (void)hipFree(ix->d_locate); ix->d_locate = nullptr; ix->bytes -= ix->img.n * sizeof(u64); }
  ix->img.locate_tab = nullptr;
}

// the walk of locateInternal (gcsa.cpp:880-896) memoised for every path node; false when an entry does not fit or on any error
bool make_locate_table(gcsa2_index* ix)
{
  drop_locate_table(ix);
  u32* d_overflow = nullptr; u32 overflow = 1;
  hipError_t e = hipMalloc(&ix->d_locate, ix->img.n * sizeof(u64));
  if(e == hipSuccess) { e = hipMalloc(reinterpret_cast<void**>(&d_overflow), sizeof(u32)); }
  if(e == hipSuccess) { e = hipMemset(d_overflow, 0, sizeof(u32)); }
  if(e == hipSuccess)
  {
    const u64 slice = u64(1) << 30;
    for(u64 first = 0; first < ix->img.n && e == hipSuccess; first += slice)
    {
      u64 count = (ix->img.n - first < slice ? ix->img.n - first : slice);
      hipLaunchKernelGGL(k_build_locate_table, dim3(unsigned((count + TPB2 - 1) / TPB2)), dim3(TPB2), 0, nullptr,
                         ix->img, first, static_cast<u64*>(ix->d_locate), d_overflow);
      e = hipGetLastError();
    }
    if(e == hipSuccess) { e = hipMemcpy(&overflow, d_overflow, sizeof(u32), hipMemcpyDeviceToHost); }
  }
  if(d_overflow) { (void)hipFree(d_overflow); }
  if(e == hipSuccess && overflow == 0)
  {
    ix->img.locate_tab = static_cast<const u64*>(ix->d_locate);
    ix->bytes += ix->img.n * sizeof(u64);
    return true;
  }
  if(ix->d_locate) { (void)hipFree(ix->d_locate); ix->d_locate = nullptr; }
  (void)hipGetLastError();
  return false;
}

// host-side staging of the device image --------------------------------------------------

// The image is laid out first (offsets only), allocated once, and filled by the kernels of kernels_build.hpp.
struct Planner
{
  u64 words = 0;               // image size so far, in u64 units; every piece starts on a 64-byte boundary
  u64 reserve(u64 nwords, u64 align_words = 8)
  {
    u64 off = (words + align_words - 1) / align_words * align_words;
    words = off + nwords;
    return off;
  }
};

struct BVPlan { u64 blocks_off = 0, hints_off = 0, size = 0, nblocks = 0, ones = 0, nhints = 0; bool hints = false; };

BVPlan plan_bv(Planner& pl, u64 size, bool with_select)
{
  BVPlan p;
  p.size = size; p.nblocks = size / BLOCK_BITS + 1; p.hints = with_select;
  p.blocks_off = pl.reserve(p.nblocks * BLOCK_WORDS);
  if(with_select)
  {
    p.nhints = size / SELECT_SAMPLE + 2;      // ones / SELECT_SAMPLE + 2 are read (bv_select); ones <= size is known after the build
    p.hints_off = pl.reserve((p.nhints + 1) / 2);
  }
  return p;
}

// Device scratch of one image build: a plain bit array in flight, the per-block popcounts and their prefix sums.
struct BuildScratch
{
  u64 *plain = nullptr, *counts = nullptr, *before = nullptr;
  void* cub = nullptr;
  size_t cub_bytes = 0;
  hipError_t alloc(u64 max_bits)
  {
    const u64 words = (max_bits + 63) / 64 + 1, blocks = max_bits / BLOCK_BITS + 1 + 2 * MAX_SIGMA;   // `before` also receives the charRange table
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&plain), words * sizeof(u64));
    if(e == hipSuccess) { e = hipMalloc(reinterpret_cast<void**>(&counts), blocks * sizeof(u64)); }
    if(e == hipSuccess) { e = hipMalloc(reinterpret_cast<void**>(&before), blocks * sizeof(u64)); }
    if(e == hipSuccess) { e = hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, counts, before, int(blocks)); }
    if(e == hipSuccess) { e = hipMalloc(&cub, cub_bytes > 0 ? cub_bytes : 8); }
    return e;
  }
  ~BuildScratch()
  {
    if(plain) { (void)hipFree(plain); } if(counts) { (void)hipFree(counts); }
    if(before) { (void)hipFree(before); } if(cub) { (void)hipFree(cub); }
  }
};

// RB64 form of one plain bit array (`plain` in host OR device memory) at its planned place in the image; fills p.ones.
hipError_t build_bv(u64* d_base, BVPlan& p, const u64* plain, BuildScratch& s)
{
  const u64 words = (p.size + 63) / 64;
  hipError_t e = hipSuccess;
  if(words > 0) { e = hipMemcpy(s.plain, plain, words * sizeof(u64), hipMemcpyDefault); }
  if(e != hipSuccess) { return e; }
  u64* blocks = d_base + p.blocks_off;
  hipLaunchKernelGGL(k_rb64_fill, dim3(grid_for(p.nblocks)), dim3(TPB), 0, nullptr, s.plain, p.size, p.nblocks, blocks, s.counts);
  size_t bytes = s.cub_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(s.cub, bytes, s.counts, s.before, int(p.nblocks));
  if(e != hipSuccess) { return e; }
  hipLaunchKernelGGL(k_rb64_counts, dim3(grid_for(p.nblocks)), dim3(TPB), 0, nullptr, s.before, p.nblocks, blocks);
  u64 last[2] = { 0, 0 };
  e = hipMemcpy(&last[0], s.before + (p.nblocks - 1), sizeof(u64), hipMemcpyDeviceToHost);
  if(e == hipSuccess) { e = hipMemcpy(&last[1], s.counts + (p.nblocks - 1), sizeof(u64), hipMemcpyDeviceToHost); }
  if(e != hipSuccess) { return e; }
  p.ones = last[0] + last[1];
  if(p.hints)
  {
    hipLaunchKernelGGL(k_select_hints, dim3(grid_for(p.nhints)), dim3(TPB), 0, nullptr, blocks, p.nblocks, p.nhints,
                       reinterpret_cast<u32*>(d_base + p.hints_off));
  }
  return hipGetLastError();
}

DevBV resolve(const BVPlan& p, const u64* d_base)
{
  DevBV bv;
  bv.blocks = d_base + p.blocks_off;
  bv.hints = p.hints ? reinterpret_cast<const u32*>(d_base + p.hints_off) : nullptr;
  bv.size = p.size; bv.nblocks = p.nblocks; bv.ones = p.ones;
  return bv;
}

struct DeviceGuard
{
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev)
  {
    if(hipGetDevice(&prev) != hipSuccess) { prev = -1; }
    ok = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() { if(prev >= 0) { (void)hipSetDevice(prev); } }
};

constexpr size_t PINNED_ARENA = size_t(8) << 20;       // per staging object
constexpr size_t PINNED_MAX_COPY = size_t(2) << 20;    // larger transfers go straight from / to the caller's memory
constexpr size_t DEVICE_ARENA_KEEP = size_t(512) << 20; // a larger arena is released with the call that needed it
// A call that moves at most this much (the scalar find() / LF() / count() / parent() of the facade, batches of a few hundred
// queries) makes no copies at all: its buffers are carved out of pinned host memory that the kernel reads and writes over the
// bus, so the call is one launch and one stream synchronisation instead of two or three copies around them.
constexpr size_t ZERO_COPY_ARENA = size_t(32) << 10;

// One host-pointer call's lease on a Staging object of the handle (see Staging).
class Lease
{
public:
  explicit Lease(const gcsa2_index* ix) : ix(ix), s(nullptr), d_used(0), h_used(0), busy(false), zero(false)
  {
    std::lock_guard<std::mutex> hold(ix->staging_lock);
    if(!ix->staging_pool.empty()) { s = ix->staging_pool.back(); ix->staging_pool.pop_back(); }
  }
  ~Lease()
  {
    if(s == nullptr) { return; }
    if(busy) { (void)hipStreamSynchronize(s->stream); }       // an early error return: nothing of this call may still be in flight
    if(s->d_cap > DEVICE_ARENA_KEEP) { (void)hipFree(s->d); s->d = nullptr; s->d_cap = 0; }
    std::lock_guard<std::mutex> hold(ix->staging_lock);
    ix->staging_pool.push_back(s);
  }
  Lease(const Lease&) = delete;
  Lease& operator=(const Lease&) = delete;

  // device bytes this call will carve out of the arena (sum of its buffers, each rounded up to 256 bytes)
  // zero_copy_ok: every buffer of the call is only ever touched by kernels and by up() / down()
  hipError_t begin(size_t device_bytes, bool zero_copy_ok = false)
  {
    if(s == nullptr)
    {
      s = new(std::nothrow) Staging();
      if(s == nullptr) { return hipErrorOutOfMemory; }
      hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
      if(e == hipSuccess) { e = hipHostMalloc(reinterpret_cast<void**>(&s->h), PINNED_ARENA, hipHostMallocDefault); }
      if(e == hipSuccess) { e = hipHostMalloc(reinterpret_cast<void**>(&s->z), ZERO_COPY_ARENA + 64, hipHostMallocMapped | hipHostMallocCoherent); }
      if(e != hipSuccess)
      {
        if(s->stream) { (void)hipStreamDestroy(s->stream); } if(s->h) { (void)hipHostFree(s->h); }
        delete s; s = nullptr; return e;
      }
      s->h_cap = PINNED_ARENA;
    }
    zero = (zero_copy_ok && ix->tune.zero_copy && device_bytes <= ZERO_COPY_ARENA);
    if(zero) { d_used = 0; h_used = 0; pending.clear(); busy = true; return hipSuccess; }
    if(device_bytes > s->d_cap)
    {
      if(s->d != nullptr) { (void)hipFree(s->d); s->d = nullptr; s->d_cap = 0; }
      size_t want = device_bytes + (device_bytes >> 2) + 4096;
      hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d), want);
      if(e != hipSuccess) { return e; }
      s->d_cap = want;
    }
    d_used = 0; h_used = 0; pending.clear(); busy = true;
    return hipSuccess;
  }
  static size_t need(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }
  template<class T> T* dev(u64 count)
  {
    char* p = (zero ? s->z : s->d) + d_used;
    d_used += need(count * sizeof(T));
    return reinterpret_cast<T*>(p);
  }
  hipStream_t stream() const { return s->stream; }

  hipError_t up(void* d, const void* h, size_t bytes)
  {
    if(bytes == 0) { return hipSuccess; }
    if(in_zero_arena(d)) { std::memcpy(d, h, bytes); return hipSuccess; }
    char* slot = pinned(bytes);
    if(slot == nullptr) { return hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s->stream); }
    std::memcpy(slot, h, bytes);
    return hipMemcpyAsync(d, slot, bytes, hipMemcpyHostToDevice, s->stream);
  }
  hipError_t down(void* h, const void* d, size_t bytes)
  {
    if(bytes == 0) { return hipSuccess; }
    if(in_zero_arena(d)) { pending.push_back(Pending{h, static_cast<const char*>(d), bytes}); return hipSuccess; }
    char* slot = pinned(bytes);
    if(slot == nullptr) { return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s->stream); }
    pending.push_back(Pending{h, slot, bytes});
    return hipMemcpyAsync(slot, d, bytes, hipMemcpyDeviceToHost, s->stream);
  }
  // wait for everything enqueued on the call's stream and hand the staged results to the caller.  A zero-copy call (the
  // facade's scalar find() / LF() / count() / parent()) waits for a ticket that a one-thread kernel behind its work writes
  // into the page-locked arena, instead of for hipStreamSynchronize: 8 against 13 us on this path (tests/perf/launch_latency.hip)
  hipError_t finish()
  {
    hipError_t e = hipSuccess;
    if(zero)
    {
      volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(s->z + ZERO_COPY_ARENA);
      const unsigned long long ticket = ix->next_ticket.fetch_add(1);
      hipLaunchKernelGGL(k_ticket, dim3(1), dim3(1), 0, s->stream, flag, ticket);
      e = hipGetLastError();
      for(u64 spins = 1; e == hipSuccess && *flag != ticket; spins++)
      {
        if(spins > 100000) { std::this_thread::yield(); }
        if((spins & 0x3FFF) == 0)
        {
          const hipError_t q = hipStreamQuery(s->stream);
          if(q == hipSuccess) { break; }                        // idle: the ticket is there (or the launch was lost: checked below)
          if(q != hipErrorNotReady) { e = q; }
        }
      }
      if(e == hipSuccess && *flag != ticket) { e = hipStreamSynchronize(s->stream); }
      std::atomic_thread_fence(std::memory_order_acquire);
    }
    else { e = hipStreamSynchronize(s->stream); }
    if(e == hipSuccess) { for(const Pending& p : pending) { std::memcpy(p.user, p.slot, p.bytes); } }
    pending.clear(); busy = false;
    return e;
  }

private:
  bool in_zero_arena(const void* p) const
  {
    const char* c = static_cast<const char*>(p);
    return zero && c >= s->z && c < s->z + ZERO_COPY_ARENA;
  }
  char* pinned(size_t bytes)
  {
    if(bytes > PINNED_MAX_COPY || h_used + bytes > s->h_cap) { return nullptr; }
    char* p = s->h + h_used;
    h_used += (bytes + 63) / 64 * 64;
    return p;
  }
  struct Pending { void* user; const char* slot; size_t bytes; };
  const gcsa2_index* ix; Staging* s; size_t d_used, h_used; bool busy, zero;
  std::vector<Pending> pending;
};

inline hipError_t pool_alloc(const gcsa2_index* ix, void** p, size_t bytes, hipStream_t stream)
{
  return ix->pool != nullptr ? hipMallocFromPoolAsync(p, bytes, ix->pool, stream) : hipMallocAsync(p, bytes, stream);
}

// stream-ordered scratch: no device-wide synchronisation from allocation or release
// Scratch of one locate pass: carved out of an ARENA the handle keeps (one per concurrent call; grown to the largest pass seen,
// released by gcsa2_index_trim).  Round 3 took every buffer from the stream-ordered pool: fifteen hipFreeAsync calls at the end
// of a pass cost 1.0-1.4 ms of host time -- a quarter of a 4.4 ms batch (GCSA2_LOCATE_TRACE, profiles/r04_locate.md).
// A buffer that does not fit the arena is a plain allocation for this pass; the arena is re-made at the new size when the pass
// ends.  The arena goes back to the handle only when the stream is known to be idle (`settled`, or a synchronisation here).
struct Scratch
{
  const gcsa2_index* ix; hipStream_t stream;
  gcsa2_index::Arena arena;
  size_t used = 0, wanted = 0;
  std::vector<void*> extra;
  bool settled = false;
  Scratch(const gcsa2_index* ix, hipStream_t s) : ix(ix), stream(s)
  {
    std::lock_guard<std::mutex> guard(ix->arena_lock);
    size_t best = 0;
    for(size_t i = 1; i < ix->arenas.size(); i++) { if(ix->arenas[i].bytes > ix->arenas[best].bytes) { best = i; } }
    if(!ix->arenas.empty()) { arena = ix->arenas[best]; ix->arenas.erase(ix->arenas.begin() + long(best)); }
  }
  ~Scratch()
  {
    if(!settled) { (void)hipStreamSynchronize(stream); }
    for(void* p : extra) { (void)hipFree(p); }
    // the arena grows to 1.125 x the largest request, up to tune.arena_cap (GCSA2_ARENA_CAP_MB, default 24 GB): what a pass
    // needs beyond it is allocated and freed by that pass, so that one huge locate() does not pin tens of GB on the handle
    // until gcsa2_index_trim
    size_t want = wanted + wanted / 8;
    if(want > ix->tune.arena_cap) { want = ix->tune.arena_cap; }
    if(want > arena.bytes)
    {
      if(arena.base != nullptr) { (void)hipFree(arena.base); }
      arena.base = nullptr; arena.bytes = 0;
      void* fresh = nullptr;
      if(hipMalloc(&fresh, want) == hipSuccess) { arena.base = static_cast<char*>(fresh); arena.bytes = want; }
      else { (void)hipGetLastError(); }
    }
    if(arena.base != nullptr)
    {
      std::lock_guard<std::mutex> guard(ix->arena_lock);
      ix->arenas.push_back(arena);
    }
  }
  template<class T> hipError_t get(T*& p, u64 count)
  {
    const size_t bytes = (size_t(count > 0 ? count : 1) * sizeof(T) + 255) & ~size_t(255);
    wanted += bytes;
    if(arena.base != nullptr && used + bytes <= arena.bytes) { p = reinterpret_cast<T*>(arena.base + used); used += bytes; return hipSuccess; }
    void* raw = nullptr;
    hipError_t e = hipMalloc(&raw, bytes);
    if(e == hipSuccess) { extra.push_back(raw); p = static_cast<T*>(raw); }
    return e;
  }
};

}  // namespace

#include "host_batch.hpp"

namespace {

// ---- the mailbox: scalar calls answered by a resident wavefront (kernels_mailbox.hpp) ---------------------------------------
constexpr int MAIL_UNAVAILABLE = 1;          // internal, not a gcsa2_status: take the launch path
constexpr unsigned long long MAIL_TICKS_PER_US = 100;      // wall_clock64(): the constant 100 MHz counter

inline void mailbox_launch(const gcsa2_index* ix, unsigned long long answered)
{
  gcsa2_index::Mailbox& m = ix->mail;
  volatile MailSlot* s = m.slot;
  s->alive = 1;
  std::atomic_thread_fence(std::memory_order_seq_cst);
  hipLaunchKernelGGL(k_mailbox, dim3(1), dim3(64), 0, m.stream, ix->img, m.slot, answered, ix->tune.mailbox_park_us * MAIL_TICKS_PER_US,
                     ix->tune.mailbox_life_ms * 1000 * MAIL_TICKS_PER_US);
  m.launches++;
}

// One request through the slot.  GCSA2_OK with the results, MAIL_UNAVAILABLE when the mailbox is switched off, held by another
// host thread (that thread's loop keeps the wavefront; this call takes the launch path instead of queueing behind it) or could
// not be set up; an error when the device does not answer.
int mailbox_call(const gcsa2_index* ix, unsigned long long op, unsigned long long a0, unsigned long long a1, unsigned long long a2, u64* results, int n_results)
{
  gcsa2_index::Mailbox& m = ix->mail;
  if(!ix->tune.mailbox || m.failed) { return MAIL_UNAVAILABLE; }
  std::unique_lock<std::mutex> hold(m.lock, std::try_to_lock);
  if(!hold.owns_lock()) { return MAIL_UNAVAILABLE; }
  if(m.slot == nullptr)
  {
    void* raw = nullptr;
    if(hipHostMalloc(&raw, sizeof(MailSlot), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); m.failed = true; return MAIL_UNAVAILABLE; }
    std::memset(raw, 0, sizeof(MailSlot));
    if(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(raw); m.failed = true; return MAIL_UNAVAILABLE; }
    m.slot = static_cast<MailSlot*>(raw);
  }
  volatile MailSlot* s = m.slot;
  const unsigned long long ticket = ++m.ticket;
  m.calls++;
  s->op = op; s->arg[0] = a0; s->arg[1] = a1; s->arg[2] = a2;
  std::atomic_thread_fence(std::memory_order_release);
  if(s->alive == 0) { mailbox_launch(ix, ticket - 1); if(hipGetLastError() != hipSuccess) { m.failed = true; return MAIL_UNAVAILABLE; } }
  s->request = ticket;
  const auto t0 = std::chrono::steady_clock::now();
  for(u64 spins = 1; s->done != ticket || s->front != ticket; spins++)       // (both ends of the answer's line: kernels_mailbox.hpp)
  {
    __builtin_ia32_pause();
    if(s->alive == 0)
    {
      // the wavefront has left -- perhaps after answering in its last look at the slot; if not, the next instance answers
      std::atomic_thread_fence(std::memory_order_acquire);
      if(s->done == ticket && s->front == ticket) { break; }
      mailbox_launch(ix, ticket - 1);
      if(hipGetLastError() != hipSuccess) { m.failed = true; return fail(GCSA2_ERR_HIP, "mailbox: the resident kernel could not be launched"); }
    }
    if((spins & 0xFFFF) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10))
    {
      m.failed = true;
      return fail(GCSA2_ERR_HIP, "mailbox: the device did not answer a scalar call within 10 s");
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  for(int k = 0; k < n_results; k++) { results[k] = s->result[k]; }
  return GCSA2_OK;
}

// ends the resident wavefront (before the image changes or goes away) and, with `release`, gives the slot and the stream back
void mailbox_stop(const gcsa2_index* ix, bool release)
{
  gcsa2_index::Mailbox& m = ix->mail;
  std::lock_guard<std::mutex> hold(m.lock);
  if(m.slot == nullptr) { return; }
  volatile MailSlot* s = m.slot;
  if(s->alive != 0 && !m.failed)
  {
    const unsigned long long ticket = ++m.ticket;
    s->op = MAIL_QUIT;
    std::atomic_thread_fence(std::memory_order_release);
    s->request = ticket;
  }
  (void)hipStreamSynchronize(m.stream);                       // (an instance that had left already: nothing to wait for)
  s->alive = 0; s->done = m.ticket; s->front = m.ticket;
  if(release)
  {
    (void)hipStreamDestroy(m.stream); (void)hipHostFree(m.slot);
    m.slot = nullptr; m.stream = nullptr;
  }
}

}  // namespace

namespace {
// owners: scratch of total_nodes / OWNER_SPAN + 3 entries (k_block_owners).  Values in path order (the table walk has an
// unordered two-pass form for the sorted mode: locate_chunk).
inline void launch_walk(const gcsa2_index* ix, const u64* d_ranges, u64 nq, const u64* node_off, const u64* raw_off,
                        u64 total_nodes, u64* values, u64* owners, hipStream_t stream)
{
  if(ix->img.locate_tab != nullptr)
  {
    const u64 blocks = grid_for(total_nodes), spans = (total_nodes + OWNER_SPAN - 1) / OWNER_SPAN;
    hipLaunchKernelGGL(k_block_owners, dim3(grid_for(spans + 1)), dim3(TPB), 0, stream, node_off, nq, total_nodes, OWNER_SPAN, spans, owners);
    hipLaunchKernelGGL(k_locate_tab, dim3(unsigned(blocks)), dim3(TPB), 0, stream,
                       ix->img, d_ranges, nq, node_off, raw_off, total_nodes, values, owners);
  }
  else if(ix->img.pred4 != nullptr)
  {
    const u64 blocks = (total_nodes + TPB2 - 1) / TPB2, spans = (total_nodes + OWNER_SPAN - 1) / OWNER_SPAN;
    hipLaunchKernelGGL(k_block_owners, dim3(grid_for(spans + 1)), dim3(TPB), 0, stream, node_off, nq, total_nodes, OWNER_SPAN, spans, owners);
    hipLaunchKernelGGL(k_locate_walk2, dim3(unsigned(blocks)), dim3(TPB2), 0, stream,
                       ix->img, d_ranges, nq, node_off, raw_off, total_nodes, values, owners);
  }
  else
  {
    hipLaunchKernelGGL(k_locate_walk, dim3(grid_for(total_nodes)), dim3(TPB), 0, stream,
                       ix->img, d_ranges, nq, node_off, raw_off, total_nodes, values);
  }
}
}  // namespace

extern "C" {

const char* gcsa2_last_error(void) { return g_error.c_str(); }

int gcsa2_device_count(void)
{
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if(e != hipSuccess) { return fail(GCSA2_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
  return count;
}

int gcsa2_index_create(const gcsa2_host_view* v, int device, gcsa2_index** out)
{
  if(v == nullptr || out == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null argument"); }
  *out = nullptr;
  if(v->sigma == 0 || v->sigma > GCSA2_MAX_SIGMA || v->char2comp == nullptr || v->C == nullptr ||
     v->bwt == nullptr || v->edge_bits == nullptr)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "host view lacks alphabet / bwt / edges or sigma out of range");
  }
  if(v->lcp_data != nullptr && v->lcp_levels > u64(MAX_LCP_LEVELS)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "too many LCP levels"); }
  // Consistency of the view itself: the query kernels index device memory with these values and, like the
  // reference's low-level interface (gcsa.h:133-135), do not check them again.
  for(int b = 0; b < 256; b++)
  {
    if(v->char2comp[b] >= v->sigma) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "alpha.char2comp maps a byte to a comp >= sigma"); }
  }
  for(u64 c = 0; c < v->sigma; c++)
  {
    if(v->C[c] > v->C[c + 1]) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "alpha.C is not non-decreasing"); }
  }
  if(v->C[v->sigma] != v->edges) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "alpha.C[sigma] differs from header.edges"); }
  if(v->sampled_path_bits != nullptr)
  {
    if(v->stored_samples == nullptr || v->sample_bits == nullptr || v->sample_width == 0 || v->sample_width > 64)
    {
      return fail(GCSA2_ERR_INVALID_ARGUMENT, "samples: missing array or sample width out of range");
    }
  }
  if(v->extra_filter_bits != nullptr && (v->extra_values_bits == nullptr || v->redundant_bits == nullptr))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "counters: missing array");
  }
  if(v->lcp_data != nullptr)
  {
    // LCPArray (src/lcp.cpp:224-259): level 0 = one value per path node, every further level one value per
    // `branching` values of the level below, up to a single root.  A stale .lcp beside an index (another graph,
    // another order) would otherwise send parent() outside the index and hang the LF + parent loop.
    if(v->lcp_offsets == nullptr || v->lcp_levels == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "LCP: missing offsets"); }
    if(v->lcp_branching < 2) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "LCP: branching factor below 2"); }
    if(v->path_nodes > 0 && v->lcp_size != v->path_nodes) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "LCP: header.size differs from the number of path nodes (an .lcp file of another index?)"); }
    u64 level_size = v->lcp_size, at = 0, top_size = 0;
    for(u64 l = 0; l < v->lcp_levels; l++)
    {
      if(v->lcp_offsets[l] != at) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "LCP: offsets do not match the level sizes implied by the branching factor"); }
      at += level_size; top_size = level_size;
      if(l + 1 < v->lcp_levels && level_size <= 1) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "LCP: levels above the root"); }
      level_size = (level_size + v->lcp_branching - 1) / v->lcp_branching;
    }
    if(v->lcp_offsets[v->lcp_levels] != at) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "LCP: offsets do not match the level sizes implied by the branching factor"); }
    if(top_size > 1) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "LCP: the top level is not a single root"); }
  }
  int count = gcsa2_device_count();
  if(count <= 0) { return fail(GCSA2_ERR_NO_DEVICE, "no HIP device visible: " + g_error); }
  if(device < 0 || device >= count) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "device index out of range"); }

  if(v->sigma * (v->path_nodes / FLB_BITS + 1) >= u64(PAIR_FLAG) || v->lcp_size / 16 + 16 >= u64(PAIR_FLAG))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "index too large: the block and LCP-window indices of the fetch keep two flag bits");
  }
  if(v->path_nodes > MAX_PATH_NODES || v->edges > 2 * MAX_PATH_NODES)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "index of more than 2^38 path nodes: beyond what one device holds and what the block indices of this build address");
  }
  gcsa2_index* ix = new(std::nothrow) gcsa2_index();
  if(ix == nullptr) { return fail(GCSA2_ERR_OUT_OF_MEMORY, "host allocation failed"); }
  ix->device = device; ix->order = v->order;
  {
    auto knob = [](const char* name, long fallback, long lo, long hi) -> long
    {
      const char* e = std::getenv(name);
      long val = (e != nullptr && *e != 0 ? std::atol(e) : fallback);
      return val < lo ? lo : (val > hi ? hi : val);
    };
    ix->tune.cool_down = u32(knob("GCSA2_COOL_DOWN", COOL_DOWN, 0, 1000));
    ix->tune.ms_refill_at = u32(knob("GCSA2_MS_REFILL_AT", MS_REFILL_AT, 1, 64));
    ix->tune.ms_grid = u64(knob("GCSA2_MS_GRID", 0, 0, long(1) << 30));
    ix->tune.locate_split = u64(knob("GCSA2_LOCATE_SPLIT", (long(1) << 31) - 1, 2, (long(1) << 31) - 1));
    ix->tune.locate_split_queries = u64(knob("GCSA2_LOCATE_SPLIT_QUERIES", long(1) << 30, 1, long(1) << 30));
    ix->tune.zero_copy = (knob("GCSA2_ZERO_COPY", 1, 0, 1) != 0);
    ix->tune.pipe_lanes = u32(knob("GCSA2_PIPE_LANES", 6, 1, 16));
    ix->tune.pipe_chunk = u64(1) << knob("GCSA2_PIPE_CHUNK", 18, 15, 20);
    ix->tune.pipe_blocking = (knob("GCSA2_PIPE_BLOCKING", 0, 0, 1) != 0);
    ix->tune.ms_pieces = (knob("GCSA2_MS_PIECES", 1, 0, 1) != 0);
    ix->tune.ms_piece_bytes = u64(knob("GCSA2_MS_PIECE_MB", 32, 1, 1024)) << 20;
    ix->tune.ms_threads = u32(knob("GCSA2_MS_THREADS", 4, 1, 16));
    ix->tune.kmer_piece = u64(knob("GCSA2_KMER_PIECE", long(1) << 27, 4, long(1) << 27));
    ix->tune.locate_trace = (knob("GCSA2_LOCATE_TRACE", 0, 0, 1) != 0);
    ix->tune.locate_single = (knob("GCSA2_LOCATE_SINGLE", 1, 0, 1) != 0);
    ix->tune.locate_fused_compact = (knob("GCSA2_LOCATE_FUSED_COMPACT", 1, 0, 1) != 0);
    ix->tune.locate_fuse = (knob("GCSA2_LOCATE_FUSE", 1, 0, 1) != 0);
    ix->tune.fuse_above = u64(knob("GCSA2_LOCATE_FUSE_ABOVE", BIG_SEGMENT, 1, long(1) << 40));
    ix->tune.locate_in_place = (knob("GCSA2_LOCATE_IN_PLACE", 1, 0, 1) != 0);
    ix->tune.mailbox = (knob("GCSA2_MAILBOX", 1, 0, 1) != 0);
    ix->tune.mailbox_park_us = u64(knob("GCSA2_MAILBOX_PARK_US", 200, 1, 1000000));
    ix->tune.mailbox_life_ms = u64(knob("GCSA2_MAILBOX_LIFE_MS", 20, 1, 10000));
    ix->tune.split_skew = u32(knob("GCSA2_SPLIT_SKEW", BIG_SEGMENT, 16, BIG_SEGMENT));
    ix->tune.split_target = u32(knob("GCSA2_SPLIT_TARGET", SPLIT_TARGET, 1, 4096));
    ix->tune.arena_cap = size_t(knob("GCSA2_ARENA_CAP_MB", 24576, 0, long(1) << 20)) << 20;    // 24 GB: 1/12 of an MI355X's HBM per arena
    ix->tune.seed_wide = u32(knob("GCSA2_SEED_WIDE", long(SEED_WIDE), 2, long(SEED_WIDE)));     // tests: meet the marked seed entries
    {
      const char* b = std::getenv("GCSA2_MEMORY_BUDGET_MB");           // megabytes, fractions allowed (small test indexes)
      const double mb = (b != nullptr && *b != 0 ? std::atof(b) : 0.0);
      ix->tune.budget_bytes = (mb > 0.0 ? u64(mb * 1048576.0) : 0);
    }
  }
  std::memset(&ix->img, 0, sizeof(DevImage));
  DevImage& img = ix->img;
  img.n = v->path_nodes; img.e = v->edges; img.sigma = v->sigma; img.fast_chars = v->fast_chars;
  for(u64 c = 0; c <= v->sigma; c++) { img.C[c] = v->C[c]; }
  std::memcpy(img.char2comp, v->char2comp, 256);

  try
  {
    // Layout first.  All B_c back to back with identical geometry (k_find selects by base + comp * stride).
    Planner pl;
    std::vector<BVPlan> bwt(v->sigma);
    for(u64 c = 0; c < v->sigma; c++)
    {
      bwt[c] = plan_bv(pl, img.n, false);
      if(c > 0 && bwt[c].blocks_off != bwt[0].blocks_off + c * (bwt[0].nblocks * BLOCK_WORDS))
      {
        delete ix; return fail(GCSA2_ERR_INVALID_ARGUMENT, "internal: B_c stride mismatch");
      }
    }
    BVPlan edges = plan_bv(pl, img.e, false);
    img.flb_nblocks = img.n / FLB_BITS + 1;
    const u64 flb_off = pl.reserve(v->sigma * img.flb_nblocks * FLB_WORDS, FLB_WORDS);
    BVPlan sampled, samples, xfilter, xvalues, redundant;
    u64 stored_off = 0, lcp_off = 0, stored_words = 0, max_bits = (img.n > img.e ? img.n : img.e);
    img.has_samples = (v->sampled_path_bits != nullptr);
    if(img.has_samples)
    {
      sampled = plan_bv(pl, img.n, false);
      samples = plan_bv(pl, v->sample_count, true);
      stored_words = (v->sample_count * v->sample_width + 63) / 64;
      stored_off = pl.reserve(stored_words + 2);
      img.sample_count = v->sample_count; img.sample_width = v->sample_width;
      if(v->sample_count > max_bits) { max_bits = v->sample_count; }
    }
    img.has_counters = (v->extra_filter_bits != nullptr);
    if(img.has_counters)
    {
      xfilter = plan_bv(pl, img.n, false);
      xvalues = plan_bv(pl, v->extra_values_len, true);
      redundant = plan_bv(pl, v->redundant_len, true);
      if(v->extra_values_len > max_bits) { max_bits = v->extra_values_len; }
      if(v->redundant_len > max_bits) { max_bits = v->redundant_len; }
    }
    img.has_lcp = (v->lcp_data != nullptr);
    if(img.has_lcp)
    {
      img.lcp_size = v->lcp_size; img.lcp_branching = v->lcp_branching; img.lcp_levels = v->lcp_levels;
      img.lcp_shift = 0;
      if((v->lcp_branching & (v->lcp_branching - 1)) == 0) { while((u64(1) << img.lcp_shift) < v->lcp_branching) { img.lcp_shift++; } }
      for(u64 l = 0; l <= v->lcp_levels; l++) { img.lcp_offsets[l] = v->lcp_offsets[l]; }
      img.lcp_values = v->lcp_offsets[v->lcp_levels];
      lcp_off = pl.reserve((img.lcp_values + 7) / 8 + 18);  // 128-byte window reads around the last values stay inside (parent_from_window)
    }

    DeviceGuard guard(device);
    if(!guard.ok) { delete ix; return fail(GCSA2_ERR_HIP, "hipSetDevice failed"); }
    {
      int cus = 0;
      if(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) { ix->compute_units = cus; }
      // Query scratch is stream-ordered memory from a pool OWNED BY THIS HANDLE, which keeps what it has grown to
      // instead of returning it to the driver at every synchronisation.  The device's default pool (and with it
      // the caller's own hipMallocAsync behaviour) is left alone.
      hipMemPoolProps props;
      std::memset(&props, 0, sizeof(props));
      props.allocType = hipMemAllocationTypePinned;
      props.handleTypes = hipMemHandleTypeNone;
      props.location.type = hipMemLocationTypeDevice;
      props.location.id = device;
      if(hipMemPoolCreate(&ix->pool, &props) == hipSuccess && ix->pool != nullptr)
      {
        uint64_t keep = ~uint64_t(0);
        (void)hipMemPoolSetAttribute(ix->pool, hipMemPoolAttrReleaseThreshold, &keep);
      }
      else { ix->pool = nullptr; }           // falls back to the default pool with its default threshold
      (void)hipGetLastError();
    }
    ix->bytes = pl.words * sizeof(u64);
    hipError_t e = hipMalloc(&ix->d_base, ix->bytes > 0 ? ix->bytes : 8);
    if(e != hipSuccess) { delete ix; return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("hipMalloc(image): ") + hipGetErrorString(e)); }
    e = hipMemset(ix->d_base, 0, ix->bytes > 0 ? ix->bytes : 8);       // alignment gaps, the words behind the samples and the LCP values
    if(e == hipSuccess) { e = hipMalloc(reinterpret_cast<void**>(&ix->d_slots), RESULT_SLOTS * TOTAL_WORDS * sizeof(unsigned long long)); }
    if(e == hipSuccess) { e = hipHostMalloc(reinterpret_cast<void**>(&ix->h_slots), RESULT_SLOTS * TOTAL_WORDS * sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent); }
    if(e == hipSuccess) { std::memset(ix->h_slots, 0, RESULT_SLOTS * TOTAL_WORDS * sizeof(unsigned long long)); }
    if(e != hipSuccess) { gcsa2_index_destroy(ix); return fail(GCSA2_ERR_HIP, std::string("image allocation: ") + hipGetErrorString(e)); }

    // The image is built on the device from the plain arrays of the view, each of them copied once (they may already be in
    // device memory): rank blocks, select hints, the fused FLB128 blocks and the charRange table (kernels_build.hpp).
    u64* wbase = static_cast<u64*>(ix->d_base);
    const u64* base = wbase;
    {
      BuildScratch scratch;
      const char* step = "scratch";
      auto run = [&](const char* name, BVPlan& plan, const u64* plain, DevBV& dst)
      {
        if(e != hipSuccess) { return; }
        step = name;
        e = build_bv(wbase, plan, plain, scratch);
        dst = resolve(plan, base);
      };
      auto copy = [&](const char* name, u64 word_off, const void* src, u64 bytes)
      {
        if(e != hipSuccess || bytes == 0) { return; }
        step = name;
        e = hipMemcpy(wbase + word_off, src, bytes, hipMemcpyDefault);
      };
      e = scratch.alloc(max_bits);
      for(u64 c = 0; c < v->sigma; c++) { run("bwt", bwt[c], v->bwt[c], img.bwt[c]); }
      run("edges", edges, v->edge_bits, img.edges);
      if(e == hipSuccess)
      {
        step = "fused blocks";
        hipLaunchKernelGGL(k_build_flb, dim3(grid_for(img.flb_nblocks), unsigned(v->sigma)), dim3(TPB), 0, nullptr, img, wbase + flb_off);
        hipLaunchKernelGGL(k_crange, dim3(1), dim3(64), 0, nullptr, img, scratch.before);
        e = hipGetLastError();
        if(e == hipSuccess) { e = hipMemcpy(img.crange, scratch.before, 2 * v->sigma * sizeof(u64), hipMemcpyDeviceToHost); }
        img.flb = base + flb_off;
      }
      if(img.has_samples)
      {
        run("sampled_paths", sampled, v->sampled_path_bits, img.sampled);
        run("samples", samples, v->sample_bits, img.samples);
        copy("stored_samples", stored_off, v->stored_samples, stored_words * sizeof(u64));
        img.stored = base + stored_off;
      }
      if(img.has_counters)
      {
        run("extra_pointers.filter", xfilter, v->extra_filter_bits, img.xfilter);
        run("extra_pointers.values", xvalues, v->extra_values_bits, img.xvalues);
        run("redundant_pointers", redundant, v->redundant_bits, img.redundant);
      }
      if(img.has_lcp)
      {
        copy("lcp", lcp_off, v->lcp_data, img.lcp_values);
        img.lcp = reinterpret_cast<const u8*>(base + lcp_off);
      }
      if(e == hipSuccess) { step = "synchronize"; e = hipDeviceSynchronize(); }
      if(e != hipSuccess) { g_error = step; }
    }
    if(e != hipSuccess)
    {
      const std::string step = g_error;
      gcsa2_index_destroy(ix);
      return fail(GCSA2_ERR_HIP, "image build (" + step + "): " + hipGetErrorString(e));
    }

    // pred4 nibbles (first predecessor comp + sampled flag), built on the device
    img.pred4 = nullptr;
    if(img.sigma <= 8 && img.n > 0)
    {
      u64 nwords = (img.n / BLOCK_BITS + 1) * PAYLOAD_WORDS;
      e = hipMalloc(&ix->d_pred4, nwords * 4 * sizeof(u64));
      if(e == hipSuccess)
      {
        hipLaunchKernelGGL(k_build_pred4, dim3(grid_for(nwords)), dim3(TPB), 0, nullptr, img, nwords, static_cast<u64*>(ix->d_pred4));
        e = hipGetLastError();
        if(e == hipSuccess) { e = hipDeviceSynchronize(); }
      }
      if(e != hipSuccess)
      {
        gcsa2_index_destroy(ix);       // releases whatever has been allocated so far
        return fail(GCSA2_ERR_HIP, std::string("pred4: ") + hipGetErrorString(e));
      }
      img.pred4 = static_cast<const u64*>(ix->d_pred4);
      ix->bytes += nwords * 4 * sizeof(u64);
    }

    // FLP128 pair blocks (two characters per step), built on the device: 10.7 bytes per path node.  Default on;
    // skipped when GCSA2_PAIR_BLOCKS=0, when comps 1..4 do not exist, or when they would take more than a third
    // of the free device memory (find() then steps one character at a time, with identical results).
    img.flp = nullptr; img.flp_nblocks = 0;
    {
      const char* penv = std::getenv("GCSA2_PAIR_BLOCKS");
      const u64 pair_bytes = pair_block_bytes_of(img);
      size_t free_bytes = 0, total_bytes = 0;
      bool fits = hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess && pair_bytes <= free_bytes / 3;
      if(fits && ix->tune.budget_bytes > 0)
      {
        // Under a memory budget (GCSA2_MEMORY_BUDGET_MB) the tables are taken in the order of what they buy find() per byte:
        // a seed table of up to an eighth of what the budget leaves (every character it covers removes one LF step per query
        // for 4x the bytes), then the pair blocks (half the memory requests of the remaining steps for 10.7 bytes per path
        // node), then the seed table grown into what is left, then the locate table (8 bytes per path node; locate() only).
        const u64 left = budget_left(ix);
        u64 reserve = 0;
        for(u32 k0 = 1; k0 <= 16 && (u64(8) << (2 * k0)) <= left / 8; k0++) { reserve = u64(8) << (2 * k0); }
        fits = pair_bytes + reserve <= left;
      }
      if(!(penv != nullptr && std::atoi(penv) == 0) && pair_blocks_possible(img) && fits)
      {
        e = make_pair_blocks(ix);
        if(e != hipSuccess)
        {
          gcsa2_index_destroy(ix);
          return fail(GCSA2_ERR_HIP, std::string("pair blocks: ") + hipGetErrorString(e));
        }
      }
    }

    // k-mer seed table, only if comps 1..4 exist.  Default: the largest k <= 16 whose table (4^k entries of 8 bytes)
    // is at most twice the index image (with the pair blocks) -- each extra character saves one LF step per query
    // and quadruples the table; HBM capacity is what this GPU has to spare.  GCSA2_KMER_TABLE=k asks for exactly
    // k (<= 16; 0 disables).  Either way the table must fit in a quarter of the free device memory.
    u32 k = 0;
    const u64 entry_bytes = 8;
    const char* env = std::getenv("GCSA2_KMER_TABLE");
    {
      size_t free_bytes = 0, total_bytes = 0;
      if(hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) { free_bytes = 0; }
      if(env != nullptr)
      {
        k = u32(std::atoi(env));
        if(k > 16) { k = 16; }
        while(k > 0 && (entry_bytes << (2 * k)) > free_bytes / 4) { k--; }
      }
      else
      {
        const u64 image_bytes = 2 * ix->bytes;
        while(k < 16 && (entry_bytes << (2 * (k + 1))) <= image_bytes && (entry_bytes << (2 * (k + 1))) <= free_bytes / 4) { k++; }
      }
      if(ix->tune.budget_bytes > 0) { while(k > 0 && (entry_bytes << (2 * k)) > budget_left(ix)) { k--; } }
    }
    if(!seed_table_possible(img)) { k = 0; }
    img.kmer_k = 0; img.kmer_table = nullptr; img.seed_wide = ix->tune.seed_wide;
    if(k > 0)
    {
      e = make_seed_table(ix, k);
      if(e != hipSuccess)
      {
        gcsa2_index_destroy(ix);
        return fail(GCSA2_ERR_HIP, std::string("k-mer table: ") + hipGetErrorString(e));
      }
    }
  }
  catch(const std::bad_alloc&)
  {
    gcsa2_index_destroy(ix); return fail(GCSA2_ERR_OUT_OF_MEMORY, "host allocation failed");
  }

  DeviceGuard table_guard(device);       // the guard above ended with the try block
  if(!table_guard.ok) { gcsa2_index_destroy(ix); return fail(GCSA2_ERR_HIP, "hipSetDevice failed"); }

  // memoised locate walks: 8 bytes per path node, built with the walk kernel itself.  Optional: skipped
  // when GCSA2_LOCATE_TABLE=0, when it would take more than a third of the free memory, or when an
  // entry does not fit (then locate() walks as before).
  ix->img.locate_tab = nullptr;
  {
    const char* env = std::getenv("GCSA2_LOCATE_TABLE");
    size_t free_bytes = 0, total_bytes = 0;
    bool wanted = locate_table_possible(ix->img) && !(env != nullptr && std::atoi(env) == 0);
    if(wanted && ix->tune.budget_bytes > 0 && ix->img.n * sizeof(u64) > budget_left(ix)) { wanted = false; }
    if(wanted && hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess && ix->img.n * sizeof(u64) <= free_bytes / 3)
    {
      (void)make_locate_table(ix);
    }
  }
  // memoised unary LF chains for find(): 16 bytes per path node.  An image WITH samples has it only on request
  // (GCSA2_JUMP_TABLE=1; round 2: the table costs more than the locate table and such an image serves locate() too).  A
  // find-only image -- created without samples, so it has no locate table and find() is all it serves -- gets it by
  // default (JUMP_DEFAULT_FIND_ONLY), in the locate table's place: last under a memory budget, and only where it leaves
  // a sixteenth of the device free (jump_table_fits); GCSA2_JUMP_TABLE=0 switches it off.  Two builders with identical output: doubling
  // (1 -> 2 -> 4 -> 8 steps) through a second buffer that is released afterwards where both buffers pass the
  // free-memory test, otherwise one pass of chain walks into the table itself (k_jump_walk); GCSA2_JUMP_BUILD=double|walk
  // forces one of them (tests).  A table that cannot be had is left out without an error.  The middle slot of its entries
  // holds the node after jump_mid steps: jump_mid_default(), or GCSA2_JUMP_MID=2|6 (any other value is ignored).  Branch
  // records are written only with jump_mid = 6: where jump_branch_default() says so -- forcing GCSA2_JUMP_MID=6 on a small
  // image does not switch them on -- or as GCSA2_JUMP_BRANCH=0|1 says.
  ix->img.jump_tab = nullptr; ix->img.jump_mid = 2; ix->img.jump_branch = 0;
  {
    const char* env = std::getenv("GCSA2_JUMP_TABLE");
    const char* how = std::getenv("GCSA2_JUMP_BUILD");
    const char* mid = std::getenv("GCSA2_JUMP_MID");
    const char* branch = std::getenv("GCSA2_JUMP_BRANCH");
    size_t free_bytes = 0, total_bytes = 0;
    const u64 n = ix->img.n, bytes = n * sizeof(ulonglong2);
    const bool wanted = (env != nullptr && *env != 0 ? std::atoi(env) != 0 : JUMP_DEFAULT_FIND_ONLY && !ix->img.has_samples);
    if(wanted && n > 0 && n <= JUMP_NODE_MASK && ix->img.sigma >= 5 &&
       (ix->tune.budget_bytes == 0 || bytes <= budget_left(ix)) &&
       hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess && jump_table_fits(bytes, free_bytes, total_bytes))
    {
      bool doubling = jump_table_fits(2 * bytes, free_bytes, total_bytes);
      if(how != nullptr && std::strcmp(how, "walk") == 0) { doubling = false; }
      if(how != nullptr && std::strcmp(how, "double") == 0) { doubling = true; }        // a failed allocation still ends without a table
      ix->img.jump_mid = u16(jump_mid_default(n, ix->img.flp != nullptr));
      if(mid != nullptr && (std::strcmp(mid, "2") == 0 || std::strcmp(mid, "6") == 0)) { ix->img.jump_mid = u16(mid[0] - '0'); }
      bool records = jump_branch_default(n, ix->img.flp != nullptr);
      if(branch != nullptr && (std::strcmp(branch, "0") == 0 || std::strcmp(branch, "1") == 0)) { records = (branch[0] == '1'); }
      ix->img.jump_branch = (records && ix->img.jump_mid == 6 ? 1 : 0);
      void* other = nullptr;
      hipError_t e = hipMalloc(&ix->d_jump, bytes);
      if(e == hipSuccess && doubling) { e = hipMalloc(&other, bytes); }
      ulonglong2 *a = static_cast<ulonglong2*>(ix->d_jump), *b = static_cast<ulonglong2*>(other);
      const u64 slice = u64(1) << 30;
      for(u64 first = 0; first < n && e == hipSuccess; first += slice)
      {
        u64 count = (n - first < slice ? n - first : slice);
        if(doubling) { hipLaunchKernelGGL(k_jump_init, dim3(grid_for(count)), dim3(TPB), 0, nullptr, ix->img, first, a); }
        else { hipLaunchKernelGGL(k_jump_walk, dim3(grid_for(count)), dim3(TPB), 0, nullptr, ix->img, first, a); }
        e = hipGetLastError();
      }
      for(u32 have = 1; doubling && have < JUMP_MAX && e == hipSuccess; have *= 2)
      {
        for(u64 first = 0; first < n && e == hipSuccess; first += slice)
        {
          u64 count = (n - first < slice ? n - first : slice);
          hipLaunchKernelGGL(k_jump_double, dim3(grid_for(count)), dim3(TPB), 0, nullptr, a, n, first, have, u32(ix->img.jump_mid), b);
          e = hipGetLastError();
        }
        std::swap(a, b);
      }
      if(e == hipSuccess) { e = hipDeviceSynchronize(); }
      // three doubling rounds: the result is in the buffer that was `other` at the start
      if(e == hipSuccess)
      {
        if(b) { (void)hipFree(b); }
        ix->d_jump = a;
        ix->img.jump_tab = a; ix->bytes += bytes;
      }
      else
      {
        if(ix->d_jump) { (void)hipFree(ix->d_jump); } if(other) { (void)hipFree(other); }
        ix->d_jump = nullptr; ix->img.jump_mid = 2; ix->img.jump_branch = 0; (void)hipGetLastError();
      }
    }
  }
  *out = ix;
  return GCSA2_OK;
}

int gcsa2_index_set_tables(gcsa2_index* ix, int pair_blocks, int kmer_k, int locate_table)
{
  if(ix == nullptr || pair_blocks < -1 || pair_blocks > 1 || locate_table < -1 || locate_table > 1 || kmer_k < -1 || kmer_k > 16)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "set_tables: pair_blocks / locate_table in {-1, 0, 1}, kmer_k in -1 .. 16");
  }
  DeviceGuard guard(ix->device);
  if(!guard.ok) { return fail(GCSA2_ERR_HIP, "hipSetDevice failed"); }
  mailbox_stop(ix, false);                   // (so does the resident wavefront of the scalar calls)
  HIP_TRY(hipDeviceSynchronize());           // launches in flight hold the old pointers
  // drops first, so that what is built next finds the memory
  if(pair_blocks == 0) { drop_pair_blocks(ix); }
  if(locate_table == 0) { drop_locate_table(ix); }
  if(kmer_k >= 0 && u32(kmer_k) != ix->img.kmer_k) { drop_seed_table(ix); }
  if(kmer_k > 0 && ix->img.kmer_k == 0)
  {
    if(!seed_table_possible(ix->img)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "this index cannot have a seed table (no comps 1..4, or positions beyond 40 bits)"); }
    hipError_t e = make_seed_table(ix, u32(kmer_k));
    if(e != hipSuccess) { return fail(e == hipErrorOutOfMemory ? GCSA2_ERR_OUT_OF_MEMORY : GCSA2_ERR_HIP, std::string("k-mer table: ") + hipGetErrorString(e)); }
  }
  if(pair_blocks == 1 && ix->img.flp == nullptr)
  {
    if(!pair_blocks_possible(ix->img)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "this index cannot have pair blocks"); }
    hipError_t e = make_pair_blocks(ix);
    if(e != hipSuccess) { return fail(e == hipErrorOutOfMemory ? GCSA2_ERR_OUT_OF_MEMORY : GCSA2_ERR_HIP, std::string("pair blocks: ") + hipGetErrorString(e)); }
  }
  if(locate_table == 1 && ix->img.locate_tab == nullptr)
  {
    if(!locate_table_possible(ix->img)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "this index cannot have a locate table (no samples)"); }
    if(!make_locate_table(ix)) { return fail(GCSA2_ERR_OUT_OF_MEMORY, "locate table: no memory, or an entry that does not fit"); }
  }
  return GCSA2_OK;
}

namespace {
// the host pipeline of the large host-pointer batches and the staging objects of the small ones (pinned + device memory)
void release_host_staging(gcsa2_index* ix)
{
  std::lock_guard<std::mutex> pipe_guard(ix->pipe_lock);
  for(gcsa2_index::PipeLane& lane : ix->pipe)
  {
    for(gcsa2_index::PipeSet& set : lane.set)
    {
      if(set.h) { (void)hipHostFree(set.h); }
      if(set.d) { (void)hipFree(set.d); }
      if(set.done) { (void)hipEventDestroy(set.done); }
    }
    if(lane.stream) { (void)hipStreamDestroy(lane.stream); }
  }
  ix->pipe.clear();
  std::lock_guard<std::mutex> staging_guard(ix->staging_lock);
  for(Staging* st : ix->staging_pool)
  {
    if(st->stream) { (void)hipStreamDestroy(st->stream); }
    if(st->d) { (void)hipFree(st->d); }
    if(st->h) { (void)hipHostFree(st->h); }
    if(st->z) { (void)hipHostFree(st->z); }
    delete st;
  }
  ix->staging_pool.clear();
  std::lock_guard<std::mutex> arena_guard(ix->arena_lock);
  for(gcsa2_index::Arena& a : ix->arenas) { if(a.base) { (void)hipFree(a.base); } }
  ix->arenas.clear();
}
}  // namespace

int gcsa2_index_trim(gcsa2_index* ix)
{
  if(ix == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null index"); }
  DeviceGuard guard(ix->device);
  if(!guard.ok) { return fail(GCSA2_ERR_HIP, "hipSetDevice failed"); }
  mailbox_stop(ix, true);                                      // (the resident wavefront holds a copy of the image's pointers)
  HIP_TRY(hipDeviceSynchronize());
  release_host_staging(ix);
  if(ix->pool != nullptr) { HIP_TRY(hipMemPoolTrimTo(ix->pool, 0)); }
  return GCSA2_OK;
}

// Shape of the host pipeline (gcsa2_find_batch / _packed): lanes = host threads with their streams and staging sets (1..16),
// chunk_log2 = log2 of the patterns per chunk (15..20); 0 / negative leaves a value as it is; blocking: 1 = the lanes sleep in
// hipEventSynchronize (hipEventBlockingSync), 0 = they spin, -1 = as it is.  Gives the current pipeline back.
int gcsa2_index_set_pipeline(gcsa2_index* ix, int lanes, int chunk_log2, int blocking)
{
  if(ix == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null index"); }
  if(lanes > 16 || chunk_log2 > 20 || (chunk_log2 > 0 && chunk_log2 < 15)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "host pipeline: lanes 1..16, chunk_log2 15..20"); }
  const int rc = gcsa2_index_trim(ix);
  if(rc != GCSA2_OK) { return rc; }
  std::lock_guard<std::mutex> hold(ix->pipe_lock);
  if(lanes > 0) { ix->tune.pipe_lanes = u32(lanes); }
  if(chunk_log2 > 0) { ix->tune.pipe_chunk = u64(1) << chunk_log2; }
  if(blocking >= 0) { ix->tune.pipe_blocking = (blocking != 0); }
  return GCSA2_OK;
}

void gcsa2_index_destroy(gcsa2_index* ix)
{
  if(ix == nullptr) { return; }
  DeviceGuard guard(ix->device);
  mailbox_stop(ix, true);
  if(ix->d_base) { (void)hipFree(ix->d_base); }
  if(ix->d_kmer) { (void)hipFree(ix->d_kmer); }
  if(ix->d_pred4) { (void)hipFree(ix->d_pred4); }
  if(ix->d_locate) { (void)hipFree(ix->d_locate); }
  if(ix->d_jump) { (void)hipFree(ix->d_jump); }
  if(ix->d_pairs) { (void)hipFree(ix->d_pairs); }
  if(ix->d_slots) { (void)hipFree(ix->d_slots); }
  if(ix->h_slots) { (void)hipHostFree(ix->h_slots); }
  if(ix->pool) { (void)hipDeviceSynchronize(); (void)hipMemPoolDestroy(ix->pool); }
  release_host_staging(ix);
  delete ix;
}

// scalar calls answered by the resident wavefront so far, and how often it had to be launched (diagnostics, tests)
int gcsa2_mailbox_stats(const gcsa2_index* ix, uint64_t* calls, uint64_t* launches)
{
  if(ix == nullptr || calls == nullptr || launches == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null argument"); }
  std::lock_guard<std::mutex> hold(ix->mail.lock);
  *calls = ix->mail.calls; *launches = ix->mail.launches;
  return GCSA2_OK;
}

uint64_t gcsa2_size(const gcsa2_index* ix) { return ix->img.n; }
uint64_t gcsa2_edge_count(const gcsa2_index* ix) { return ix->img.e; }
uint64_t gcsa2_order(const gcsa2_index* ix) { return ix->order; }
uint64_t gcsa2_sample_count(const gcsa2_index* ix) { return ix->img.sample_count; }
uint64_t gcsa2_sample_bits(const gcsa2_index* ix) { return ix->img.sample_width; }
int gcsa2_device(const gcsa2_index* ix) { return ix->device; }
uint64_t gcsa2_device_bytes(const gcsa2_index* ix) { return ix->bytes; }
uint64_t gcsa2_block_bits(const gcsa2_index*) { return BLOCK_BITS; }

// ---- device-pointer entry points: enqueue only -------------------------------------------

#define CHECK_INDEX(ix) do { if((ix) == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null index"); } } while(0)
#define LAUNCH_CHECK(name) do { hipError_t e_ = hipGetLastError(); if(e_ != hipSuccess) { \
  return fail(GCSA2_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e_)); } } while(0)

}  // extern "C"

namespace {

// one input array of `in_words` u64 per query, one output array of `out_words` u64 per query, one kernel in between
template<class Launch>
int simple_batch(const gcsa2_index* ix, const uint64_t* in, u64 in_words, uint64_t* out, u64 out_words, u64 nq, const char* name, Launch launch)
{
  DeviceGuard guard(ix->device);
  Lease lease(ix);
  HIP_TRY(lease.begin(Lease::need(in_words * nq * 8) + Lease::need(out_words * nq * 8), true));
  u64* d_in = lease.dev<u64>(in_words * nq); u64* d_out = lease.dev<u64>(out_words * nq);
  HIP_TRY(lease.up(d_in, in, in_words * nq * sizeof(u64)));
  launch(d_in, d_out, lease.stream());
  { hipError_t e_ = hipGetLastError(); if(e_ != hipSuccess) { return fail(GCSA2_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e_)); } }
  HIP_TRY(lease.down(out, d_out, out_words * nq * sizeof(u64)));
  HIP_TRY(lease.finish());
  return GCSA2_OK;
}

// k_find2 instantiation for this image: JUMP with the jump table, PAIR with the pair blocks
template<bool STATS>
void launch_find2(const gcsa2_index* ix, unsigned grid, hipStream_t st, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 nq,
                  uint64_t* d_ranges, unsigned long long* d_stats, const u32* perm)
{
  const bool jump = ix->img.jump_tab != nullptr, pair = ix->img.flp != nullptr;
#define G2_FIND2(J, P) hipLaunchKernelGGL((k_find2<STATS, J, P>), dim3(grid), dim3(TPB2), 0, st, \
                                          ix->img, d_patterns, d_offsets, nq, d_ranges, d_stats, perm)
  if(jump && pair) { G2_FIND2(true, true); }
  else if(jump) { G2_FIND2(true, false); }
  else if(pair) { G2_FIND2(false, true); }
  else { G2_FIND2(false, false); }
#undef G2_FIND2
}

}  // namespace

extern "C" {

int gcsa2_find_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets,
                      uint64_t nq, uint64_t* d_ranges, void* stream)
{
  CHECK_INDEX(ix);
  DeviceGuard guard(ix->device);          // the launch goes to the index's device whatever the caller's current one is
  if(nq == 0) { return GCSA2_OK; }
  launch_find2<false>(ix, unsigned((nq + TPB2 - 1) / TPB2), static_cast<hipStream_t>(stream), d_patterns, d_offsets, nq, d_ranges,
                      nullptr, nullptr);
  LAUNCH_CHECK("k_find2");
  return GCSA2_OK;
}

// find() of patterns handed over as 2-bit codes, all of one length (kernels_find.hpp: k_find2<.., PACKED>)
int gcsa2_find_packed_device(const gcsa2_index* ix, const uint64_t* d_codes, uint64_t pattern_length, uint64_t nq, uint64_t* d_ranges, void* stream)
{
  CHECK_INDEX(ix);
  DeviceGuard guard(ix->device);
  if(nq == 0) { return GCSA2_OK; }
  if(pattern_length == 0 || pattern_length >= (u64(1) << 32)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "packed patterns: the common length must be 1 .. 2^32 - 1"); }
  if(ix->img.sigma < 5) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "packed patterns need the comps 1..4"); }
  const unsigned grid = unsigned((nq + TPB2 - 1) / TPB2);
  const u8* codes = reinterpret_cast<const u8*>(d_codes);
  const u64* length = reinterpret_cast<const u64*>(pattern_length);       // PACKED: the offsets argument carries the length
  hipStream_t st = static_cast<hipStream_t>(stream);
  if(ix->img.flp != nullptr)
  {
    hipLaunchKernelGGL((k_find2<false, false, true, true>), dim3(grid), dim3(TPB2), 0, st, ix->img, codes, length, nq, d_ranges, (unsigned long long*)nullptr, (const u32*)nullptr);
  }
  else
  {
    hipLaunchKernelGGL((k_find2<false, false, false, true>), dim3(grid), dim3(TPB2), 0, st, ix->img, codes, length, nq, d_ranges, (unsigned long long*)nullptr, (const u32*)nullptr);
  }
  LAUNCH_CHECK("k_find2<packed>");
  return GCSA2_OK;
}

int gcsa2_find_device_variant(const gcsa2_index* ix, int variant, const uint8_t* d_patterns, const uint64_t* d_offsets,
                              uint64_t nq, uint64_t* d_ranges, void* stream)
{
  CHECK_INDEX(ix);
  if(nq == 0) { return GCSA2_OK; }
  if(variant == 2) { return gcsa2_find_device(ix, d_patterns, d_offsets, nq, d_ranges, stream); }
  if(variant == 4)   // length-bucketed: sort query ids by pattern length, then k_find2 through the permutation
  {
    if(nq >= (u64(1) << 31)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "length-bucketed find is limited to 2^31 queries per launch"); }
    hipStream_t st = static_cast<hipStream_t>(stream);
    DeviceGuard guard(ix->device);
    u32 *len_in = nullptr, *len_out = nullptr, *idx_in = nullptr, *idx_out = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, len_in, len_out, idx_in, idx_out, int(nq), 0, 32, st));
    HIP_TRY(pool_alloc(ix, reinterpret_cast<void**>(&len_in), 4 * nq * sizeof(u32), st));     // four u32 arrays
    HIP_TRY(pool_alloc(ix, &tmp, tmp_bytes, st));
    len_out = len_in + nq; idx_in = len_out + nq; idx_out = idx_in + nq;
    hipLaunchKernelGGL(k_pattern_lengths, dim3(grid_for(nq)), dim3(TPB), 0, st, d_offsets, nq, len_in, idx_in);
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, len_in, len_out, idx_in, idx_out, int(nq), 0, 32, st);
    if(e == hipSuccess)
    {
      launch_find2<false>(ix, unsigned((nq + TPB2 - 1) / TPB2), st, d_patterns, d_offsets, nq, d_ranges, nullptr, idx_out);
      e = hipGetLastError();
    }
    (void)hipFreeAsync(tmp, st); (void)hipFreeAsync(len_in, st);    // stream-ordered: freed after the kernel
    if(e != hipSuccess) { return fail(GCSA2_ERR_HIP, std::string("length-bucketed find: ") + hipGetErrorString(e)); }
    return GCSA2_OK;
  }
  return fail(GCSA2_ERR_INVALID_ARGUMENT, "unknown find variant (2: default, 4: queries ordered by pattern length first)");
}

int gcsa2_find_stats_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets,
                            uint64_t nq, uint64_t* d_ranges, uint64_t* d_stats, void* stream)
{
  CHECK_INDEX(ix);
  DeviceGuard guard(ix->device);          // the launch goes to the index's device whatever the caller's current one is
  if(d_stats == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null stats buffer"); }
  if(nq == 0) { return GCSA2_OK; }
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64 atomics");
  launch_find2<true>(ix, unsigned((nq + TPB2 - 1) / TPB2), static_cast<hipStream_t>(stream), d_patterns, d_offsets, nq, d_ranges,
                     reinterpret_cast<unsigned long long*>(d_stats), nullptr);
  LAUNCH_CHECK("k_find2<stats>");
  return GCSA2_OK;
}

uint64_t gcsa2_pair_block_bytes(const gcsa2_index* ix) { return ix->img.flp != nullptr ? 16 * ix->img.flp_nblocks * FLB_BYTES : 0; }
uint64_t gcsa2_find_block_bytes(const gcsa2_index*) { return FLB_BYTES; }
uint64_t gcsa2_kmer_table_k(const gcsa2_index* ix) { return ix->img.kmer_k; }
uint64_t gcsa2_jump_table_bytes(const gcsa2_index* ix) { return ix->img.jump_tab != nullptr ? ix->img.n * sizeof(ulonglong2) : 0; }
int gcsa2_jump_mid(const gcsa2_index* ix) { return int(ix->img.jump_mid); }
int gcsa2_jump_mid_default(uint64_t nodes, int pair_blocks) { return int(jump_mid_default(nodes, pair_blocks != 0)); }
int gcsa2_jump_branch(const gcsa2_index* ix) { return int(ix->img.jump_branch); }
int gcsa2_jump_branch_default(uint64_t nodes, int pair_blocks) { return jump_branch_default(nodes, pair_blocks != 0) ? 1 : 0; }
uint64_t gcsa2_locate_table_bytes(const gcsa2_index* ix) { return ix->img.locate_tab != nullptr ? ix->img.n * sizeof(u64) : 0; }

int gcsa2_lf_device(const gcsa2_index* ix, const uint64_t* d_in, const uint8_t* d_comps, uint64_t nq,
                    uint64_t* d_out, void* stream)
{
  CHECK_INDEX(ix);
  DeviceGuard guard(ix->device);          // the launch goes to the index's device whatever the caller's current one is
  if(nq == 0) { return GCSA2_OK; }
  hipLaunchKernelGGL(k_lf2, dim3(unsigned((nq + TPB2 - 1) / TPB2)), dim3(TPB2), 0, static_cast<hipStream_t>(stream),
                     ix->img, d_in, d_comps, nq, d_out);
  LAUNCH_CHECK("k_lf2");
  return GCSA2_OK;
}

// extend: the backward search continued from caller ranges (kernels_extend.hpp); enqueue only, invalid states are marked by the kernel
int gcsa2_extend_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                        const gcsa2_search_state* d_states, uint64_t n_states, gcsa2_extension* d_out, void* stream)
{
  CHECK_INDEX(ix);
  if(n_states == 0) { return GCSA2_OK; }
  if(d_states == nullptr || d_out == nullptr || (n_patterns > 0 && d_offsets == nullptr)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  if(n_states >= (u64(1) << 31) * TPB2) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "extend: 2^38 or more states in one launch; split the batch"); }
  DeviceGuard guard(ix->device);          // the launch goes to the index's device whatever the caller's current one is
  static_assert(sizeof(gcsa2_search_state) == 40 && sizeof(gcsa2_extension) == 40, "five u64 each");
  const dim3 grid(unsigned((n_states + TPB2 - 1) / TPB2));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if(ix->img.flp != nullptr) { hipLaunchKernelGGL(k_extend<true>, grid, dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, n_patterns, d_states, n_states, d_out); }
  else { hipLaunchKernelGGL(k_extend<false>, grid, dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, n_patterns, d_states, n_states, d_out); }
  LAUNCH_CHECK("k_extend");
  return GCSA2_OK;
}

int gcsa2_count_device(const gcsa2_index* ix, const uint64_t* d_ranges, uint64_t nq, uint64_t* d_counts, void* stream)
{
  CHECK_INDEX(ix);
  DeviceGuard guard(ix->device);          // the launch goes to the index's device whatever the caller's current one is
  if(!ix->img.has_counters) { return fail(GCSA2_ERR_MISSING_COMPONENT, "index was created without counters"); }
  if(nq == 0) { return GCSA2_OK; }
  hipLaunchKernelGGL(k_count, dim3(grid_for(nq)), dim3(TPB), 0, static_cast<hipStream_t>(stream),
                     ix->img, d_ranges, nq, d_counts);
  LAUNCH_CHECK("k_count");
  return GCSA2_OK;
}

int gcsa2_parent_device(const gcsa2_index* ix, const uint64_t* d_ranges, uint64_t nq, gcsa2_stnode* d_nodes, void* stream)
{
  CHECK_INDEX(ix);
  DeviceGuard guard(ix->device);          // the launch goes to the index's device whatever the caller's current one is
  if(!ix->img.has_lcp) { return fail(GCSA2_ERR_MISSING_COMPONENT, "index was created without an LCP array"); }
  if(nq == 0) { return GCSA2_OK; }
  hipLaunchKernelGGL(k_parent, dim3(grid_for(nq)), dim3(TPB), 0, static_cast<hipStream_t>(stream),
                     ix->img, d_ranges, nq, d_nodes);
  LAUNCH_CHECK("k_parent");
  return GCSA2_OK;
}

void gcsa2_locate_discard(gcsa2_locate_job* job)
{
  if(job == nullptr) { return; }
  DeviceGuard guard(job->device);
  if(job->d_offsets) { (void)hipFree(job->d_offsets); }
  if(job->d_values) { (void)hipFree(job->d_values); }
  delete job;
}

// The locate pipeline proper.  d_offsets (nq + 1 entries) is written on the device; values_for(count)
// hands out the buffer for `count` values once that is known (nullptr = refuse); *total_out = number of
// values.  Complete (stream synchronised) on return.
typedef std::function<u64*(u64)> ValuesProvider;

} // extern "C"

namespace {

constexpr int LOCATE_NEEDS_SPLIT = 1;      // internal: not a gcsa2_status

// The totals of a pass on the host: k_publish_totals copies the slot to page-locked host memory and writes a ticket behind
// it; the host polls the ticket (tests/perf/launch_latency.hip: 8 us against 13 us for launch + hipStreamSynchronize, and
// against the 100-400 us a hipMemcpyAsync into pageable memory + synchronise took on this path: three of them were 1.2 ms of
// a 5 ms locate() batch, profiles/r03_locate.md).  The stream is asked now and then, so that a failed launch ends the wait.
int read_totals(const gcsa2_index* ix, unsigned slot, unsigned long long (&totals)[TOTAL_WORDS], hipStream_t stream)
{
  const unsigned long long ticket = ix->next_ticket.fetch_add(1);
  volatile unsigned long long* h = ix->h_slots + u64(TOTAL_WORDS) * slot;
  hipLaunchKernelGGL(k_publish_totals, dim3(1), dim3(64), 0, stream, ix->d_slots + u64(TOTAL_WORDS) * slot, h, ticket);
  LAUNCH_CHECK("k_publish_totals");
  for(u64 spins = 1; h[TOTAL_WORDS - 1] != ticket; spins++)
  {
    if(spins > 20000) { std::this_thread::yield(); }          // a long pass (tens of milliseconds of sorting): leave the core to others
    if((spins & 0xFFF) == 0)
    {
      const hipError_t q = hipStreamQuery(stream);
      if(q == hipSuccess) { if(h[TOTAL_WORDS - 1] == ticket) { break; } return fail(GCSA2_ERR_HIP, "locate: the stream went idle without publishing its totals"); }
      if(q != hipErrorNotReady) { return fail(GCSA2_ERR_HIP, std::string("locate: ") + hipGetErrorString(q)); }
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  for(u32 i = 0; i < TOTAL_WORDS; i++) { totals[i] = h[i]; }
  return GCSA2_OK;
}

// One pass of the locate pipeline.  The flag words' prefix sums are 32-bit, so a pass takes fewer than 2^31 values before
// deduplication; a larger batch returns LOCATE_NEEDS_SPLIT (allow_split) with the exclusive scan of the per-query raw counts
// left in d_offsets, and locate_core below cuts it.
// known_out / known_capacity: the caller's own value buffer (gcsa2_locate_into).  The pass then never waits for the number of
// distinct values: the compaction writes into the buffer under a capacity guard and the total is read with the final
// synchronisation (too small a buffer is reported then, as before).  Host round trips of a pass in sorted mode: the totals
// after the size scans (needed for the scratch), one more only if some segment has more than 4096 values, the end.
int locate_chunk(const gcsa2_index* ix, const u64* d_ranges, u64 nq, int sort, u64* d_offsets,
                 const ValuesProvider& values_for, u64* total_out, hipStream_t stream, bool allow_split,
                 u64* known_out = nullptr, u64 known_capacity = 0)
{
  *total_out = 0;
  if(nq == 0)
  {
    HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(u64), stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return GCSA2_OK;
  }
  Scratch scratch(ix, stream);
  const auto t_start = std::chrono::steady_clock::now();
  double stamps[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto stamp = [&](int k) { if(ix->tune.locate_trace) { stamps[k] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count(); } };

  // [node_counts | raw_counts | node_off] (nq + 1 each), [seg_begin | seg_end] (nq each), the totals; the
  // scan of the raw counts goes straight into the job's offsets (final as they are unless duplicates
  // have to be removed, rewritten in place otherwise)
  u64* sizes = nullptr; u64* segs = nullptr;
  const unsigned slot = ix->next_slot.fetch_add(1) % RESULT_SLOTS;
  unsigned long long* d_totals = ix->d_slots + u64(TOTAL_WORDS) * slot;
  // The one-kernel attempt costs a batch that does not fit it a launch, a host poll and nq words of scratch: after a
  // misfit the next calls on this handle go straight to the pipeline, and every eighth one tries again.
  bool try_single = (ix->img.locate_tab != nullptr && ix->tune.locate_single);
  if(try_single && ix->single_backoff.load(std::memory_order_relaxed) > 0) { ix->single_backoff.fetch_sub(1, std::memory_order_relaxed); try_single = false; }
  if(try_single)
  {
    // every range one path node with one directly stored value?  Then this kernel is the whole answer (k_locate_single); the
    // first misfit sends the batch through the pipeline below.  (The answer does not depend on `sort`: one value per range.)
    // (into scratch, copied out on success: a batch with a misfit must not leave values of this attempt in the caller's buffer
    // beyond what the pipeline then writes)
    u64* out = nullptr;
    HIP_TRY(scratch.get(out, nq));
    HIP_TRY(hipMemsetAsync(d_totals, 0, TOTAL_WORDS * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(k_locate_single, dim3(grid_for(nq + 1)), dim3(TPB), 0, stream, ix->img, d_ranges, nq, d_offsets, out, nq, d_totals);
    LAUNCH_CHECK("k_locate_single");
    unsigned long long first[TOTAL_WORDS];
    int rc1 = read_totals(ix, slot, first, stream);              // in stream order behind the kernel
    if(rc1 != GCSA2_OK) { return rc1; }
    scratch.settled = true;
    if(first[0] == 0)
    {
      *total_out = nq;
      u64* dest = known_out;
      if(known_out != nullptr) { if(known_capacity < nq) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "values buffer too small"); } }
      else
      {
        dest = values_for(nq);
        if(dest == nullptr) { return g_error.empty() ? fail(GCSA2_ERR_BUFFER_TOO_SMALL, "values buffer too small") : GCSA2_ERR_BUFFER_TOO_SMALL; }
      }
      scratch.settled = false;
      HIP_TRY(hipMemcpyAsync(dest, out, nq * sizeof(u64), hipMemcpyDeviceToDevice, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      scratch.settled = true;
      return GCSA2_OK;
    }
    ix->single_backoff.store(7, std::memory_order_relaxed);
    scratch.settled = false;
  }
  // Round 6: a wide range whose path nodes have one value each does not go through the table pass -- the workgroup that splits
  // its values reads them from the locate table itself (k_classify_fused, k_over_split): (sorted mode, table)
  const bool fuse = (sort && ix->img.locate_tab != nullptr && ix->tune.locate_fuse && ix->img.sample_width < 63);
  const u64 fuse_above = (fuse ? ix->tune.fuse_above : 0);
  HIP_TRY(scratch.get(sizes, 3 * (nq + 1))); HIP_TRY(scratch.get(segs, 7 * nq));
  u64 *node_counts = sizes, *raw_counts = sizes + (nq + 1), *node_off = sizes + 2 * (nq + 1), *raw_off = d_offsets;
  u64 *seg_begin = segs, *seg_end = segs + nq, *huge_begin = segs + 2 * nq, *huge_end = segs + 3 * nq, *over_begin = segs + 4 * nq, *over_end = segs + 5 * nq;
  const u64** over_src = reinterpret_cast<const u64**>(segs + 6 * nq);
  u64* candidates = over_end;                                  // (consumed by k_classify_fused before k_collect_multi writes the list)
  HIP_TRY(hipMemsetAsync(d_totals, 0, TOTAL_WORDS * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_locate_sizes, dim3(grid_for(nq)), dim3(TPB), 0, stream, ix->img, d_ranges, nq, node_counts, raw_counts, d_totals, fuse_above, candidates);
  LAUNCH_CHECK("k_locate_sizes");
  if(fuse_above != 0)
  {
    hipLaunchKernelGGL(k_classify_fused, dim3(unsigned(nq < 8192 ? nq : 8192)), dim3(64), 0, stream, ix->img, d_ranges, candidates, d_totals, node_counts);
    LAUNCH_CHECK("k_classify_fused");
  }

  // exclusive scans over nq + 1 entries: entry nq becomes the total
  size_t tmp_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, node_counts, node_off, size_t(nq + 1), stream));
  char* tmp = nullptr;
  HIP_TRY(scratch.get(tmp, tmp_bytes));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, node_counts, node_off, size_t(nq + 1), stream));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, raw_counts, raw_off, size_t(nq + 1), stream));
  // segments with more than one raw value: the only ones removeDuplicates has to touch
  // sorted, every segment beyond the medium class goes through the duplicate filter first (listed as huge); unsorted, only the
  // ones the workgroup sort cannot hold
  const u32 big_limit = (sort ? MEDIUM_SEGMENT : BIG_SEGMENT);
  hipLaunchKernelGGL(k_collect_multi, dim3(unsigned((nq + COLLECT_THREADS - 1) / COLLECT_THREADS)), dim3(COLLECT_THREADS), 0, stream, node_off, raw_off, nq, d_totals, seg_begin, seg_end, huge_begin, huge_end, MEDIUM_SEGMENT, big_limit,
                     d_ranges, ix->img.locate_tab, over_begin, over_end, over_src);
  LAUNCH_CHECK("k_collect_multi");
  unsigned long long totals[TOTAL_WORDS];
  stamp(0);
  int rc = read_totals(ix, slot, totals, stream);
  if(rc != GCSA2_OK) { return rc; }
  stamp(1);
  scratch.settled = true;            // the totals have arrived: nothing of this pass is in flight (until the next launch)
  const u64 total_nodes = totals[T_NODES], total_raw = totals[T_RAW], multi = totals[T_MULTI], huge_a = totals[T_HUGE_A], huge_b = totals[T_HUGE_B];
  const u64 large = totals[T_LARGE], medium = totals[T_MEDIUM];
  if(total_raw > ix->tune.locate_split || nq > ix->tune.locate_split_queries)
  {
    if(allow_split) { return LOCATE_NEEDS_SPLIT; }
    return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "locate: one range alone has 2^31 or more values before deduplication");
  }

  // the per-workgroup owners of the walk kernel (k_block_owners) fit into one of the count arrays, which the scans have
  // consumed, unless the ranges are wide; the other one serves as the per-query slot counters of the unordered table walk
  u64* owners = raw_counts;
  if(total_nodes / OWNER_SPAN + 3 > nq + 1) { HIP_TRY(scratch.get(owners, total_nodes / OWNER_SPAN + 3)); }
  u64* extra_slots = node_counts;

  if(total_raw == 0)
  {
    HIP_TRY(hipMemsetAsync(d_offsets, 0, (nq + 1) * sizeof(u64), stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return GCSA2_OK;
  }
  if(!sort || multi == 0)
  {
    // sort == false (gcsa.cpp:827-842 without removeDuplicates): values in path order, the values of
    // one path node in sample order, duplicates kept -- exactly the walk's output.  With at most one
    // value per query that output is already sorted and distinct.
    u64* out = (known_out != nullptr ? (total_raw <= known_capacity ? known_out : nullptr) : values_for(total_raw));
    if(out == nullptr) { *total_out = total_raw; return g_error.empty() ? fail(GCSA2_ERR_BUFFER_TOO_SMALL, "values buffer too small") : GCSA2_ERR_BUFFER_TOO_SMALL; }
    scratch.settled = false;
    launch_walk(ix, d_ranges, nq, node_off, raw_off, total_nodes, out, owners, stream);
    LAUNCH_CHECK("k_locate_walk");
    HIP_TRY(hipStreamSynchronize(stream));
    scratch.settled = true;
    *total_out = total_raw;
    return GCSA2_OK;
  }

  u64 *sorted = nullptr, *words = nullptr; u32 *word_counts = nullptr, *word_before = nullptr;
  const u64 nwords = total_raw / 64 + 1;
  // Round 6: a caller's buffer that holds the values BEFORE deduplication is the target of the table pass and of every sort;
  // when no sort meets a duplicate (the flag totals[T_DUPS]) the values are final where they lie, at the offsets of the size
  // scan, and nothing is compacted; otherwise k_mark_compact compacts in place.  (A buffer sized for the distinct values only
  // keeps the scratch array and the out-of-place compaction.)
  // The job interface (the library makes the value buffer) takes the same path when the values before deduplication are at most
  // 2^30 (8 GB): the buffer is then made for THEM, before the sorts instead of behind them -- a job's buffer may be longer than
  // its `total`.
  if(known_out == nullptr && ix->tune.locate_fused_compact && ix->tune.locate_in_place && total_raw <= (u64(1) << 30))
  {
    u64* made = values_for(total_raw);
    if(made == nullptr) { return g_error.empty() ? fail(GCSA2_ERR_BUFFER_TOO_SMALL, "values buffer too small") : GCSA2_ERR_BUFFER_TOO_SMALL; }
    known_out = made; known_capacity = total_raw;
  }
  const bool in_place = (known_out != nullptr && ix->tune.locate_fused_compact && ix->tune.locate_in_place && total_raw <= known_capacity);
  if(in_place) { sorted = known_out; } else { HIP_TRY(scratch.get(sorted, total_raw)); }
  bool force_compact = !in_place;
  HIP_TRY(scratch.get(words, nwords)); HIP_TRY(scratch.get(word_counts, nwords + 1)); HIP_TRY(scratch.get(word_before, nwords + 1));
  scratch.settled = false;
  if(total_nodes == 0) { }                                     // (every range with values is fused: nothing for the table pass)
  else if(ix->img.locate_tab != nullptr)
  {
    // unordered table walk in two passes (kernels_locate.hpp): single values at once, the path nodes with several values
    // marked (one word per 64 nodes) and worked through afterwards.  (The second pass runs whenever the first one may have
    // marked a node: also a node with ONE value is marked when that value does not fit a direct entry.)
    const u64 blocks = grid_for(total_nodes), spans = (total_nodes + OWNER_SPAN - 1) / OWNER_SPAN;
    u64* later_words = nullptr;
    HIP_TRY(scratch.get(later_words, spans));
    HIP_TRY(hipMemsetAsync(extra_slots, 0, nq * sizeof(u64), stream));
    hipLaunchKernelGGL(k_block_owners, dim3(grid_for(spans + 1)), dim3(TPB), 0, stream, node_off, nq, total_nodes, OWNER_SPAN, spans, owners);
    hipLaunchKernelGGL(k_locate_tab_unordered, dim3(unsigned((blocks + TAB_SPANS - 1) / TAB_SPANS)), dim3(TPB), 0, stream, ix->img, d_ranges, nq, node_off, raw_off,
                       total_nodes, sorted, owners, later_words, spans);
    if(total_raw > total_nodes || ix->img.sample_width >= 63)
    {
      hipLaunchKernelGGL(k_locate_tab_rest, dim3(grid_for(spans)), dim3(TPB), 0, stream, ix->img, d_ranges, node_off, raw_off, total_nodes, sorted,
                         owners, later_words, spans, reinterpret_cast<unsigned long long*>(extra_slots));
    }
  }
  else { launch_walk(ix, d_ranges, nq, node_off, raw_off, total_nodes, sorted, owners, stream); }
  LAUNCH_CHECK("k_locate_walk");

  // removeDuplicates: queries with up to SMALL_SEGMENT values are sorted in registers, up to MEDIUM_SEGMENT by a wavefront
  // and up to BIG_SEGMENT by a workgroup in LDS, all in place.  Longer ones first lose their duplicates (k_dedup_huge) and
  // join those lists with their distinct values (the sorts are launched over upper bounds of the list lengths and read the
  // lengths on the device); a segment with more than BIG_SEGMENT distinct values is split into buckets (k_over_split), and a
  // skewed bucket goes to the device-wide radix sort over (segment, value) keys.  Then flag + scan + compact.
  u64 over = totals[T_OVER], over_values = totals[T_OVER_VALUES];      // (the fused ranges: k_collect_multi listed them)
  const u64 huge = huge_a + huge_b;
  // the slots behind the distinct values of a filtered segment are marked in a bitmap instead of being filled and read again
  // (k_dedup_huge, k_mark_compact) -- when the one-sweep compaction is the one that will run
  // (an index whose values lie below 2^32 -- samples of at most 31 bits + fewer than 2^23 steps -- gets the 32-bit hash table)
  const bool narrow_values = (ix->img.sample_width <= 31);
  unsigned long long* dead = nullptr;
  if(huge > 0 && known_out != nullptr && ix->tune.locate_fused_compact)
  {
    HIP_TRY(scratch.get(dead, nwords));
    HIP_TRY(hipMemsetAsync(dead, 0, nwords * sizeof(unsigned long long), stream));
  }
  if(huge_a > 0)
  {
    // (64-bit words for the short segments whatever the index: with 32-bit words -- 32 KB, five workgroups on a CU instead of two --
    // this kernel was SLOWER on the 2^23 repeat graph, 0.81 against 0.62 ms for the 32-mer batch; the long segments' kernel gains, 3.6 -> 2.9 ms)
    hipLaunchKernelGGL((k_dedup_huge<BIG_SEGMENT, false, 512, unsigned long long>), dim3(unsigned(huge_a)), dim3(512), 0, stream, huge_begin, huge_end, nq - 1, sorted, nq,
                       MEDIUM_SEGMENT, d_totals, seg_begin, seg_end, over_begin, over_end, over_src, dead);
    LAUNCH_CHECK("k_dedup_huge");
  }
  if(huge_b > 0)
  {
    if(narrow_values)
    {
      hipLaunchKernelGGL((k_dedup_huge<2 * BIG_SEGMENT, true, 1024, u32>), dim3(unsigned(huge_b)), dim3(1024), 0, stream, huge_begin, huge_end, nq - 1, sorted, nq,
                         MEDIUM_SEGMENT, d_totals, seg_begin, seg_end, over_begin, over_end, over_src, dead);
    }
    else
    {
      hipLaunchKernelGGL((k_dedup_huge<2 * BIG_SEGMENT, true, 1024, unsigned long long>), dim3(unsigned(huge_b)), dim3(1024), 0, stream, huge_begin, huge_end, nq - 1, sorted, nq,
                         MEDIUM_SEGMENT, d_totals, seg_begin, seg_end, over_begin, over_end, over_src, dead);
    }
    LAUNCH_CHECK("k_dedup_huge");
    stamp(2);
    rc = read_totals(ix, slot, totals, stream);          // only these segments can overflow
    if(rc != GCSA2_OK) { return rc; }
    over = totals[T_OVER]; over_values = totals[T_OVER_VALUES];
    stamp(3);
  }
  hipLaunchKernelGGL(k_sort_small, dim3(grid_for(nq)), dim3(TPB), 0, stream, raw_off, nq, sorted, d_totals);
  LAUNCH_CHECK("k_sort_small");
  if(medium + huge > 0)
  {
    hipLaunchKernelGGL(k_sort_medium, dim3(unsigned(medium + huge)), dim3(64), 0, stream, seg_begin, seg_end, nq - 1, sorted, d_totals);
    LAUNCH_CHECK("k_sort_medium");
  }
  if(large + huge > 0)
  {
    hipLaunchKernelGGL((k_sort_big<4096, 0>), dim3(unsigned(large + huge)), dim3(big_threads<4096>()), 0, stream, seg_begin, seg_end, sorted, d_totals + T_LARGE, d_totals + T_DUPS);
    hipLaunchKernelGGL((k_sort_big<BIG_SEGMENT, 4096>), dim3(unsigned(large + huge)), dim3(big_threads<BIG_SEGMENT>()), 0, stream, seg_begin, seg_end, sorted, d_totals + T_LARGE, d_totals + T_DUPS);
    LAUNCH_CHECK("k_sort_big");
  }
  auto radix_over = [&](u64* over_begin, u64* over_end, u64 over, u64 over_values) -> int
  {
    force_compact = true;                                      // (the library's sort does not say whether it met duplicates)
    // keys = (rank of the segment) << value_bits | value; a value is a sample + fewer than 2^23 steps
    u32 value_bits = u32(ix->img.sample_width > 24 ? ix->img.sample_width : 24) + 1, rank_bits = 1;
    while((u64(1) << rank_bits) < over) { rank_bits++; }
    u64 *over_off = nullptr, *over_len = nullptr;
    HIP_TRY(scratch.get(over_off, over + 1)); HIP_TRY(scratch.get(over_len, over + 1));
    hipLaunchKernelGGL(k_over_lengths, dim3(grid_for(over + 1)), dim3(TPB), 0, stream, over_begin, over_end, over, over_len);
    size_t scan_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, over_len, over_off, size_t(over + 1), stream));
    char* scan_tmp = nullptr;
    HIP_TRY(scratch.get(scan_tmp, scan_bytes));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, over_len, over_off, size_t(over + 1), stream));
    if(value_bits + rank_bits <= 64)
    {
      u64 *keys_a = nullptr, *keys_b = nullptr;
      HIP_TRY(scratch.get(keys_a, over_values)); HIP_TRY(scratch.get(keys_b, over_values));
      hipLaunchKernelGGL(k_over_pack, dim3(grid_for(over_values)), dim3(TPB), 0, stream, over_begin, over_off, over, over_values, sorted, value_bits, keys_a);
      LAUNCH_CHECK("k_over_pack");
      hipcub::DoubleBuffer<u64> keys(keys_a, keys_b);
      size_t sort_bytes = 0;
      HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, keys, size_t(over_values), 0, int(value_bits + rank_bits), stream));
      char* sort_tmp = nullptr;
      HIP_TRY(scratch.get(sort_tmp, sort_bytes));
      HIP_TRY(hipcub::DeviceRadixSort::SortKeys(sort_tmp, sort_bytes, keys, size_t(over_values), 0, int(value_bits + rank_bits), stream));
      hipLaunchKernelGGL(k_over_unpack, dim3(grid_for(over_values)), dim3(TPB), 0, stream, over_begin, over_off, over_values, keys.Current(), value_bits, sorted);
      LAUNCH_CHECK("k_over_unpack");
    }
    else
    {
      // (values too wide to share a key with the segment rank: the library's segmented sort, from a copy)
      u64* raw = nullptr;
      HIP_TRY(scratch.get(raw, total_raw));
      HIP_TRY(hipMemcpyAsync(raw, sorted, total_raw * sizeof(u64), hipMemcpyDeviceToDevice, stream));
      size_t sort_bytes = 0;
      HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, sort_bytes, raw, sorted, int(total_raw), int(over), over_begin, over_end, 0, 64, stream));
      char* sort_tmp = nullptr;
      HIP_TRY(scratch.get(sort_tmp, sort_bytes));
      HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(sort_tmp, sort_bytes, raw, sorted, int(total_raw), int(over), over_begin, over_end, 0, 64, stream));
    }
    return GCSA2_OK;
  };
  if(over > 0)
  {
    // segments of more than BIG_SEGMENT distinct values: one workgroup each splits its segment into buckets that the
    // workgroup sort holds (k_over_split); what a skewed segment leaves over goes to the device-wide radix sort
    const u64 bucket_cap = over_values / 64 + over + 16;                  // listed buckets have more than 64 values
    u64 *split_tmp = nullptr, *bkt_begin = nullptr, *bkt_end = nullptr, *skew_begin = nullptr, *skew_end = nullptr;
    HIP_TRY(scratch.get(split_tmp, total_raw));
    HIP_TRY(scratch.get(bkt_begin, bucket_cap)); HIP_TRY(scratch.get(bkt_end, bucket_cap));
    const u32 skew_above = ix->tune.split_skew;                            // BIG_SEGMENT (lower in tests): what the workgroup sort takes
    const u64 skew_cap = over_values / skew_above + over + 16;
    HIP_TRY(scratch.get(skew_begin, skew_cap)); HIP_TRY(scratch.get(skew_end, skew_cap));
    const u64 mid_cap = over_values / BUCKET_BY_WAVE + over + 16;         // buckets of 513 .. 1024 values
    u64 *mid_begin = nullptr, *mid_end = nullptr;
    HIP_TRY(scratch.get(mid_begin, mid_cap)); HIP_TRY(scratch.get(mid_end, mid_cap));
    hipLaunchKernelGGL(k_over_split, dim3(unsigned(over)), dim3(SPLIT_THREADS), 0, stream, over_begin, over_end, sorted, split_tmp,
                       bkt_begin, bkt_end, skew_begin, skew_end, d_totals, skew_above, ix->tune.split_target, bucket_cap - 1, over_src, mid_begin, mid_end);
    LAUNCH_CHECK("k_over_split");
    rc = read_totals(ix, slot, totals, stream);
    if(rc != GCSA2_OK) { return rc; }
    const u64 buckets = totals[T_BUCKETS], big_buckets = totals[T_BIG_BUCKETS], skew = totals[T_SKEW], skew_values = totals[T_SKEW_VALUES];
    const u64 mid_buckets = totals[T_MID_BUCKETS];
    if(buckets + big_buckets > bucket_cap || mid_buckets > mid_cap) { return fail(GCSA2_ERR_HIP, "locate: more buckets than the split reserved"); }
    if(buckets > 0)
    {
      hipLaunchKernelGGL(k_sort_bucket<BUCKET_BY_WAVE>, dim3(unsigned(buckets)), dim3(64), 0, stream, bkt_begin, bkt_end, sorted, split_tmp, d_totals);
      LAUNCH_CHECK("k_sort_bucket");
    }
    if(mid_buckets > 0)
    {
      hipLaunchKernelGGL(k_sort_bucket<MEDIUM_SEGMENT>, dim3(unsigned(mid_buckets)), dim3(64), 0, stream, mid_begin, mid_end, sorted, split_tmp, d_totals);
      LAUNCH_CHECK("k_sort_bucket (513 .. 1024 values)");
    }
    if(big_buckets > 0)                                       // (listed from the back of the same arrays)
    {
      hipLaunchKernelGGL((k_sort_big<4096, MEDIUM_SEGMENT>), dim3(unsigned(big_buckets)), dim3(big_threads<4096>()), 0, stream, bkt_begin, bkt_end, sorted, d_totals + T_BIG_BUCKETS, d_totals + T_DUPS, split_tmp, bucket_cap - 1);
      hipLaunchKernelGGL((k_sort_big<BIG_SEGMENT, 4096>), dim3(unsigned(big_buckets)), dim3(big_threads<BIG_SEGMENT>()), 0, stream, bkt_begin, bkt_end, sorted, d_totals + T_BIG_BUCKETS, d_totals + T_DUPS, split_tmp, bucket_cap - 1);
      LAUNCH_CHECK("k_sort_big (buckets)");
    }
    if(skew > 0) { rc = radix_over(skew_begin, skew_end, skew, skew_values); if(rc != GCSA2_OK) { return rc; } }
  }
  if(in_place && !force_compact)
  {
    // every value is sorted in the caller's buffer, at the offsets of the size scan (d_offsets): if no sort met a duplicate, that
    // is the result.  (One poll of the totals -- the pass is complete behind it; a launch of the compaction that finds out on
    // the device that it has nothing to do cost 0.34 ms of the 8.8 ms of the 16-mer batch on the 2^30-base text.)
    stamp(4);
    rc = read_totals(ix, slot, totals, stream);
    if(rc != GCSA2_OK) { return rc; }
    stamp(5);
    if(totals[T_DUPS] == 0)
    {
      scratch.settled = true;
      *total_out = total_raw;
      HIP_TRY(hipStreamSynchronize(stream));
      stamp(6);
      return GCSA2_OK;
    }
  }
  if(known_out != nullptr && ix->tune.locate_fused_compact)
  {
    // the caller owns the values buffer: marks, counts, prefix sums and compaction in one sweep (k_mark_compact)
    const u64 tiles = (nwords * 64 + COMPACT_TILE - 1) / COMPACT_TILE;
    unsigned long long* tile_status = nullptr;
    HIP_TRY(scratch.get(tile_status, tiles + 1));                         // (+ the ticket counter behind the last tile)
    HIP_TRY(hipMemsetAsync(tile_status, 0, (tiles + 1) * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(words, 0, nwords * sizeof(u64), stream));
    hipLaunchKernelGGL(k_mark_starts, dim3(grid_for(nq)), dim3(TPB), 0, stream, raw_off, nq, words);
    hipLaunchKernelGGL(k_mark_compact, dim3(unsigned(tiles)), dim3(COMPACT_THREADS), 0, stream, sorted, total_raw, nwords, words, word_before,
                       known_out, known_capacity, tile_status, reinterpret_cast<unsigned int*>(tile_status + tiles), d_totals + T_UNIQUE, reinterpret_cast<const u64*>(dead));
    LAUNCH_CHECK("k_mark_starts / k_mark_compact");
    hipLaunchKernelGGL(k_final_offsets, dim3(grid_for(nq + 1)), dim3(TPB), 0, stream, words, word_before, nq, total_raw, nwords, d_offsets);
    LAUNCH_CHECK("k_final_offsets");
    stamp(4);
    rc = read_totals(ix, slot, totals, stream);          // in stream order behind everything above: the pass is complete
    if(rc != GCSA2_OK) { return rc; }
    stamp(5);
    scratch.settled = true;
    *total_out = totals[T_UNIQUE];
    if(totals[T_UNIQUE] > known_capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "values buffer too small"); }
    HIP_TRY(hipStreamSynchronize(stream));
    stamp(6);
    return GCSA2_OK;
  }
  hipLaunchKernelGGL(k_mark_changes, dim3(grid_for(nwords * 64)), dim3(TPB), 0, stream, sorted, total_raw, words);
  hipLaunchKernelGGL(k_mark_starts, dim3(grid_for(nq)), dim3(TPB), 0, stream, raw_off, nq, words);
  hipLaunchKernelGGL(k_word_counts, dim3(grid_for(nwords + 1)), dim3(TPB), 0, stream, words, nwords, word_counts);
  LAUNCH_CHECK("k_mark_changes / k_mark_starts / k_word_counts");
  size_t scan_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, word_counts, word_before, size_t(nwords + 1), stream));
  char* scan_tmp = nullptr;
  HIP_TRY(scratch.get(scan_tmp, scan_bytes));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, word_counts, word_before, size_t(nwords + 1), stream));
  hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, stream, word_before + nwords, d_totals + T_UNIQUE);
  LAUNCH_CHECK("k_publish");
  u64 total_unique = 0;
  u64* out = known_out;
  u64 capacity = known_capacity;
  if(out == nullptr)                 // the values buffer is made for the number of distinct values: wait for it
  {
    rc = read_totals(ix, slot, totals, stream);
    if(rc != GCSA2_OK) { return rc; }
    total_unique = totals[T_UNIQUE];
    *total_out = total_unique;
    scratch.settled = true;
    out = values_for(total_unique);
    if(out == nullptr) { return g_error.empty() ? fail(GCSA2_ERR_BUFFER_TOO_SMALL, "values buffer too small") : GCSA2_ERR_BUFFER_TOO_SMALL; }
    capacity = total_unique;
    scratch.settled = false;
  }
  hipLaunchKernelGGL(k_compact, dim3(grid_for(total_raw)), dim3(TPB), 0, stream, sorted, words, word_before, total_raw, out, capacity);
  LAUNCH_CHECK("k_compact");
  hipLaunchKernelGGL(k_final_offsets, dim3(grid_for(nq + 1)), dim3(TPB), 0, stream, words, word_before, nq, total_raw, nwords, d_offsets);
  LAUNCH_CHECK("k_final_offsets");
  stamp(4);
  if(known_out != nullptr)
  {
    rc = read_totals(ix, slot, totals, stream);          // in stream order behind everything above: the pass is complete
    if(rc != GCSA2_OK) { return rc; }
    stamp(5);
    scratch.settled = true;
    total_unique = totals[T_UNIQUE];
    *total_out = total_unique;
    if(total_unique > known_capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "values buffer too small"); }
  }
  HIP_TRY(hipStreamSynchronize(stream));
  scratch.settled = true;
  stamp(6);
  if(ix->tune.locate_trace)
  {
    std::fprintf(stderr, "[locate] enqueued sizes %.0f us | totals %.0f | walk + filter enqueued %.0f | totals %.0f | sorts + flags + compact enqueued %.0f | totals %.0f | done %.0f\n",
                 stamps[0], stamps[1], stamps[2], stamps[3], stamps[4], stamps[5], stamps[6]);
  }
  return GCSA2_OK;
}

// largest q1 in (q0, min(nq, q0 + most)] with raw_off[q1] - raw_off[q0] <= limit (q0 if even the first query exceeds it); one thread
__global__ void k_locate_cut(const u64* __restrict__ raw_off, u64 nq, u64 q0, u64 limit, u64 most, unsigned long long* __restrict__ out)
{
  u64 lo = q0, hi = (nq - q0 > most ? q0 + most : nq);
  const u64 base = raw_off[q0];
  while(lo < hi)
  {
    const u64 mid = (lo + hi + 1) >> 1;
    if(raw_off[mid] - base <= limit) { lo = mid; } else { hi = mid - 1; }
  }
  *out = lo;
}

__global__ __launch_bounds__(TPB) void k_uniform_offsets(u64* __restrict__ dst, u64 count, u64 stride)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  if(i < count) { dst[i] = i * stride; }
}

__global__ __launch_bounds__(TPB) void k_shift_offsets(const u64* __restrict__ src, u64 count, u64 base, u64* __restrict__ dst)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  if(i < count) { dst[i] = src[i] + base; }
}

// The locate pipeline for batches of any size: one pass when the batch has at most 2^30 ranges and fewer than 2^31 values before deduplication (the
// paper's 16-mer batch has 2.5 G, paper.tex:403), otherwise consecutive sub-batches of queries, each below that, whose value
// arrays are concatenated and whose offsets are shifted -- the same CSR a single pass would give.
int locate_core(const gcsa2_index* ix, const u64* d_ranges, u64 nq, int sort, u64* d_offsets,
                const ValuesProvider& values_for, u64* total_out, hipStream_t stream, u64* known_out = nullptr, u64 known_capacity = 0)
{
  int rc = locate_chunk(ix, d_ranges, nq, sort, d_offsets, values_for, total_out, stream, true, known_out, known_capacity);
  if(rc != LOCATE_NEEDS_SPLIT) { return rc; }
  struct Part { u64 q0 = 0, q1 = 0, total = 0; u64* d_off = nullptr; u64* d_val = nullptr; };
  std::vector<Part> parts;
  struct Release { std::vector<Part>& p; ~Release() { for(Part& x : p) { if(x.d_off) { (void)hipFree(x.d_off); } if(x.d_val) { (void)hipFree(x.d_val); } } } } release{parts};
  unsigned long long* d_cut = ix->d_slots + TOTAL_WORDS * (ix->next_slot.fetch_add(1) % RESULT_SLOTS);
  u64 q0 = 0;
  while(q0 < nq)                                   // d_offsets still holds the scan of the raw counts
  {
    unsigned long long q1 = 0;
    hipLaunchKernelGGL(k_locate_cut, dim3(1), dim3(1), 0, stream, d_offsets, nq, q0, ix->tune.locate_split, ix->tune.locate_split_queries, d_cut);
    HIP_TRY(hipMemcpyAsync(&q1, d_cut, sizeof(q1), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if(q1 <= q0) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "locate: one range alone has 2^31 or more values before deduplication"); }
    Part part; part.q0 = q0; part.q1 = q1;
    parts.push_back(part);
    q0 = q1;
  }
  u64 total = 0;
  for(Part& part : parts)
  {
    const u64 count = part.q1 - part.q0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&part.d_off), (count + 1) * sizeof(u64)));
    Part* self = &part;
    ValuesProvider own = [self](u64 values) -> u64*
    {
      hipError_t e = hipMalloc(reinterpret_cast<void**>(&self->d_val), (values > 0 ? values : 1) * sizeof(u64));
      if(e != hipSuccess) { fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("hipMalloc(values of a sub-batch): ") + hipGetErrorString(e)); return nullptr; }
      return self->d_val;
    };
    g_error.clear();
    rc = locate_chunk(ix, d_ranges + 2 * part.q0, count, sort, part.d_off, own, &part.total, stream, false);
    if(rc != GCSA2_OK) { return rc; }
    total += part.total;
  }
  *total_out = total;
  u64* out = values_for(total);
  if(out == nullptr) { return g_error.empty() ? fail(GCSA2_ERR_BUFFER_TOO_SMALL, "values buffer too small") : GCSA2_ERR_BUFFER_TOO_SMALL; }
  u64 base = 0;
  for(Part& part : parts)
  {
    const u64 count = part.q1 - part.q0;
    if(part.total > 0) { HIP_TRY(hipMemcpyAsync(out + base, part.d_val, part.total * sizeof(u64), hipMemcpyDeviceToDevice, stream)); }
    hipLaunchKernelGGL(k_shift_offsets, dim3(grid_for(count)), dim3(TPB), 0, stream, part.d_off, count, base, d_offsets + part.q0);
    base += part.total;
  }
  HIP_TRY(hipMemcpyAsync(d_offsets + nq, &total, sizeof(u64), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return GCSA2_OK;
}

int locate_checks(const gcsa2_index* ix, u64 nq)
{
  if(!ix->img.has_samples || !ix->img.has_counters)
  {
    return fail(GCSA2_ERR_MISSING_COMPONENT, "locate needs samples and counters (extra_pointers sizes the output)");
  }
  if(nq >= (u64(1) << 38)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "locate batch of >= 2^38 ranges; split the batch"); }      // (batches beyond 2^30 ranges run in sub-batches: locate_core)
  return GCSA2_OK;
}

}  // namespace

extern "C" {

int gcsa2_locate_device(const gcsa2_index* ix, const uint64_t* d_ranges, uint64_t nq, int sort, gcsa2_locate_job** job_out,
                        const uint64_t** d_offsets, const uint64_t** d_values, uint64_t* total_values, void* stream_)
{
  CHECK_INDEX(ix);
  if(job_out == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null job pointer"); }
  *job_out = nullptr;
  int rc = locate_checks(ix, nq);
  if(rc != GCSA2_OK) { return rc; }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DeviceGuard guard(ix->device);
  gcsa2_locate_job* job = new(std::nothrow) gcsa2_locate_job();
  if(job == nullptr) { return fail(GCSA2_ERR_OUT_OF_MEMORY, "host allocation failed"); }
  job->device = ix->device; job->nq = nq; job->stream = stream;
  struct Cleanup { gcsa2_locate_job*& j; bool armed = true; ~Cleanup() { if(armed) { gcsa2_locate_discard(j); j = nullptr; } } };
  Cleanup cleanup{job};

  // the job's buffers are read back by the host (locate_run / locate_fetch): plain hipMalloc, not pool memory
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&job->d_offsets), (nq + 1) * sizeof(u64)));
  ValuesProvider provide = [job](u64 count) -> u64*
  {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&job->d_values), (count > 0 ? count : 1) * sizeof(u64));
    if(e != hipSuccess) { fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("hipMalloc(values): ") + hipGetErrorString(e)); return nullptr; }
    return job->d_values;
  };
  g_error.clear();
  rc = locate_core(ix, d_ranges, nq, sort, job->d_offsets, provide, &job->total, stream);
  if(rc != GCSA2_OK) { return rc; }
  cleanup.armed = false; *job_out = job;
  if(d_offsets) { *d_offsets = job->d_offsets; }
  if(d_values) { *d_values = job->d_values; }
  if(total_values) { *total_values = job->total; }
  return GCSA2_OK;
}

int gcsa2_locate_into(const gcsa2_index* ix, const uint64_t* d_ranges, uint64_t nq, int sort, uint64_t* d_offsets,
                      uint64_t* d_values, uint64_t capacity, uint64_t* total_values, void* stream_)
{
  CHECK_INDEX(ix);
  if(d_offsets == nullptr || total_values == nullptr || (d_values == nullptr && capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  int rc = locate_checks(ix, nq);
  if(rc != GCSA2_OK) { return rc; }
  DeviceGuard guard(ix->device);
  ValuesProvider provide = [d_values, capacity](u64 count) -> u64* { return count <= capacity ? d_values : nullptr; };
  g_error.clear();
  const auto t0 = std::chrono::steady_clock::now();
  rc = locate_core(ix, d_ranges, nq, sort, d_offsets, provide, total_values, static_cast<hipStream_t>(stream_), d_values, capacity);
  if(ix->tune.locate_trace)
  {
    std::fprintf(stderr, "[locate] gcsa2_locate_into: %.0f us\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  return rc;
}

// ---- host-pointer entry points: copy in, run, copy out, synchronise ----------------------

} // extern "C"

namespace {

// ---- large host batches: the two chunk sources of the host pipeline (host_batch.hpp: pipe_run) -----------------------------

// Patterns as bytes with offsets: chunks of at most PIPE_CHUNK_QUERIES patterns and PIPE_CHUNK_BYTES pattern bytes.
int find_pipelined(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t nq, uint64_t* ranges)
{
  std::lock_guard<std::mutex> hold(ix->pipe_lock);
  u64 PIPE_CHUNK_QUERIES = 0;
  int rc = pipe_begin(ix, nq, PIPE_CHUNK_QUERIES);
  if(rc != GCSA2_OK) { return rc; }
  // chunk boundaries.  The offsets are validated by the lanes, chunk by chunk, while they rebase them (a serial pass over
  // 10 M offsets costs as much as the whole batch); here only the boundaries are looked at, defensively.
  std::vector<u64> cut(1, 0);
  while(cut.back() < nq)
  {
    const u64 b = cut.back();
    u64 e = (nq - b < PIPE_CHUNK_QUERIES ? nq : b + PIPE_CHUNK_QUERIES);
    if(offsets[e] < offsets[b]) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "pattern offsets are not non-decreasing"); }
    if(offsets[e] - offsets[b] > PIPE_CHUNK_BYTES)
    {
      u64 lo = b, hi = e;                                    // largest e' with offsets[e'] - offsets[b] <= PIPE_CHUNK_BYTES
      while(lo < hi) { const u64 mid = (lo + hi + 1) / 2; if(offsets[mid] >= offsets[b] && offsets[mid] - offsets[b] <= PIPE_CHUNK_BYTES) { lo = mid; } else { hi = mid - 1; } }
      e = lo;
      if(e == b) { return PIPE_PATTERN_TOO_LONG; }           // the caller takes the single-copy path
    }
    cut.push_back(e);
  }
  // each of the caller's three arrays on its own: where it lies when it is page-locked, through the lane's pinned set when not
  const bool direct_pat = page_locked(patterns, offsets[nq] - offsets[0]), direct_off = page_locked(offsets, (nq + 1) * sizeof(u64)),
             direct_out = page_locked(ranges, 2 * nq * sizeof(u64));
  // pageable result arrays are filled by the lanes anyway: their ranges come home in the narrow form; a page-locked array is
  // written in place, which takes the 16-byte pairs.  (The packed form below keeps the narrow wire even then; the two
  // choices have not been measured against each other.)
  const u64 wire = (direct_out ? 16 : pipe_wire_bytes(ix));
  auto stage = [&](u64 c, gcsa2_index::PipeLane& lane, gcsa2_index::PipeSet& set, Outcome& out) -> bool
  {
    const u64 b = cut[c], e = cut[c + 1], count = e - b, base = offsets[b], bytes = offsets[e] - base;
    char* h_pat = set.h; u64* h_off = reinterpret_cast<u64*>(set.h + (PIPE_CHUNK_BYTES + 64));
    // the chunk's pattern bytes land at the same phase within 16 bytes as in the caller's array (the kernel reads aligned
    // words around a pattern's ends); with the caller's absolute offsets the kernel gets the pointer moved back by `base`
    const u64 phase = 16 + (base & 15);
    // patterns of one length (k-mer batches): the chunk's offsets are base + i * length, made on the device instead of sent
    const u64 stride = (offsets[b + 1] - base);
    u64 bad = 0, ragged = 0;
    if(direct_off) { for(u64 i = 1; i <= count; i++) { const u64 o = offsets[b + i]; bad |= u64(o < offsets[b + i - 1]); ragged |= (o - base) ^ (i * stride); } }
    else { for(u64 i = 0; i <= count; i++) { const u64 o = offsets[b + i]; h_off[i] = o - base; bad |= u64(i > 0 && o < offsets[b + i - 1]); ragged |= (o - base) ^ (i * stride); } }
    if(bad != 0 || bytes > PIPE_CHUNK_BYTES) { out.set(GCSA2_ERR_INVALID_ARGUMENT, "pattern offsets are not non-decreasing"); return false; }
    const bool uniform = (ragged == 0);
    char* d_pat = set.d; u64* d_off = reinterpret_cast<u64*>(set.d + (PIPE_CHUNK_BYTES + 64));
    hipError_t err = hipSuccess;
    if(direct_pat) { err = hipMemcpyAsync(d_pat + phase, patterns + base, bytes, hipMemcpyHostToDevice, lane.stream); }
    else
    {
      std::memcpy(h_pat + phase, patterns + base, bytes);
      err = hipMemcpyAsync(d_pat, h_pat, (phase + bytes + 7) / 8 * 8, hipMemcpyHostToDevice, lane.stream);
    }
    if(err == hipSuccess && uniform)
    {
      hipLaunchKernelGGL(k_uniform_offsets, dim3(grid_for(count + 1)), dim3(TPB), 0, lane.stream, d_off, count + 1, stride);
      err = hipGetLastError();
    }
    else if(err == hipSuccess)
    {
      err = hipMemcpyAsync(d_off, direct_off ? offsets + b : h_off, (count + 1) * sizeof(u64), hipMemcpyHostToDevice, lane.stream);
    }
    if(err != hipSuccess) { out.hip_error("hipMemcpyAsync", err); return false; }
    const uint8_t* d_first = reinterpret_cast<const uint8_t*>(d_pat + phase) - (direct_off && !uniform ? base : 0);
    const int rc_find = gcsa2_find_device(ix, d_first, d_off, count, reinterpret_cast<u64*>(set.d + pipe_out_at(PIPE_CHUNK_QUERIES)), lane.stream);
    if(rc_find != GCSA2_OK) { out.set(rc_find, g_error); return false; }
    set.first = b; set.count = count;
    return true;
  };
  return pipe_run(ix, cut.size() - 1, PIPE_CHUNK_QUERIES, wire, direct_out, ranges, stage);
}

// Patterns as 2-bit codes of one length (gcsa2_find_batch_packed): a chunk is a fixed number of patterns, its code words up
// the link (8 bytes per 32 characters), one launch, its ranges down; no offsets at all.
int find_packed_pipelined(const gcsa2_index* ix, const uint64_t* codes, u64 length, uint64_t nq, uint64_t* ranges)
{
  std::lock_guard<std::mutex> hold(ix->pipe_lock);
  u64 PIPE_CHUNK_QUERIES = 0;
  int rc = pipe_begin(ix, nq, PIPE_CHUNK_QUERIES);
  if(rc != GCSA2_OK) { return rc; }
  const u64 words = (length + 31) >> 5;
  u64 per_chunk = PIPE_CHUNK_BYTES / (8 * words);
  if(per_chunk > PIPE_CHUNK_QUERIES) { per_chunk = PIPE_CHUNK_QUERIES; }
  if(per_chunk == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "packed patterns: one pattern exceeds a pipeline chunk"); }
  // the narrow wire whenever the index allows it; a page-locked result array is written in place only on the 16-byte wire
  const bool direct_in = page_locked(codes, nq * words * 8), direct_out = page_locked(ranges, 2 * nq * sizeof(u64));
  auto stage = [&](u64 c, gcsa2_index::PipeLane& lane, gcsa2_index::PipeSet& set, Outcome& out) -> bool
  {
    const u64 b = c * per_chunk, count = (nq - b < per_chunk ? nq - b : per_chunk), bytes = count * words * 8;
    hipError_t err = hipSuccess;
    if(direct_in) { err = hipMemcpyAsync(set.d, codes + b * words, bytes, hipMemcpyHostToDevice, lane.stream); }
    else
    {
      std::memcpy(set.h, codes + b * words, bytes);
      err = hipMemcpyAsync(set.d, set.h, bytes, hipMemcpyHostToDevice, lane.stream);
    }
    if(err != hipSuccess) { out.hip_error("hipMemcpyAsync", err); return false; }
    const int rc_find = gcsa2_find_packed_device(ix, reinterpret_cast<const u64*>(set.d), length, count, reinterpret_cast<u64*>(set.d + pipe_out_at(PIPE_CHUNK_QUERIES)), lane.stream);
    if(rc_find != GCSA2_OK) { out.set(rc_find, g_error); return false; }
    set.first = b; set.count = count;
    return true;
  };
  return pipe_run(ix, (nq + per_chunk - 1) / per_chunk, PIPE_CHUNK_QUERIES, pipe_wire_bytes(ix), direct_out, ranges, stage);
}

}  // namespace

extern "C" {

// find() of `nq` patterns of `pattern_length` characters each, given as 2-bit codes in host memory (layout: gcsa2_hip.h)
int gcsa2_find_batch_packed(const gcsa2_index* ix, const uint64_t* codes, uint64_t pattern_length, uint64_t nq, uint64_t* ranges)
{
  CHECK_INDEX(ix);
  if(nq == 0) { return GCSA2_OK; }
  if(codes == nullptr || ranges == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  if(pattern_length == 0 || pattern_length >= (u64(1) << 32)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "packed patterns: the common length must be 1 .. 2^32 - 1"); }
  try
  {
    // (patterns whose codes alone exceed a pipeline chunk -- 32 M characters -- take the single copy below)
    if(nq >= PIPE_MIN_QUERIES / 4 && ((pattern_length + 31) >> 5) * 8 <= PIPE_CHUNK_BYTES) { return find_packed_pipelined(ix, codes, pattern_length, nq, ranges); }
    // small batches: one copy in, one launch, one copy out
    DeviceGuard guard(ix->device);
    const u64 words = (pattern_length + 31) >> 5;
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, nq * words * 8 + nq * 16));
    u64* d_codes = static_cast<u64*>(d); u64* d_out = d_codes + nq * words;
    hipError_t e = hipMemcpy(d_codes, codes, nq * words * 8, hipMemcpyHostToDevice);
    int rc = (e == hipSuccess ? gcsa2_find_packed_device(ix, d_codes, pattern_length, nq, d_out, nullptr) : fail(GCSA2_ERR_HIP, hipGetErrorString(e)));
    if(rc == GCSA2_OK) { e = hipMemcpy(ranges, d_out, nq * 16, hipMemcpyDeviceToHost); if(e != hipSuccess) { rc = fail(GCSA2_ERR_HIP, hipGetErrorString(e)); } }
    (void)hipFree(d);
    return rc;
  }
  catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_find_batch_packed: ") + e.what()); }
}

int gcsa2_find_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t nq, uint64_t* ranges)
{
  CHECK_INDEX(ix);
  if(nq == 0) { return GCSA2_OK; }
  if(offsets == nullptr || ranges == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  if(nq >= PIPE_MIN_QUERIES)
  {
    try
    {
      const int rc = find_pipelined(ix, patterns, offsets, nq, ranges);
      if(rc != PIPE_PATTERN_TOO_LONG) { return rc; }
    }
    catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_find_batch: ") + e.what()); }
  }
  if(!offsets_ok(offsets, nq)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "pattern offsets are not non-decreasing"); }
  DeviceGuard guard(ix->device);
  const u64 total = offsets[nq];
  Lease lease(ix);
  HIP_TRY(lease.begin(Lease::need(total + 16) + Lease::need((nq + 1) * 8) + Lease::need(2 * nq * 8), true));
  u8* d_pat = lease.dev<u8>(total + 16); u64* d_off = lease.dev<u64>(nq + 1); u64* d_out = lease.dev<u64>(2 * nq);
  HIP_TRY(lease.up(d_pat, patterns, total));
  HIP_TRY(lease.up(d_off, offsets, (nq + 1) * sizeof(u64)));
  int rc = gcsa2_find_device(ix, d_pat, d_off, nq, d_out, lease.stream());
  if(rc != GCSA2_OK) { return rc; }
  HIP_TRY(lease.down(ranges, d_out, 2 * nq * sizeof(u64)));
  HIP_TRY(lease.finish());
  return GCSA2_OK;
}

int gcsa2_lf_batch(const gcsa2_index* ix, const uint64_t* in, const uint8_t* comps, uint64_t nq, uint64_t* out)
{
  CHECK_INDEX(ix);
  if(nq == 0) { return GCSA2_OK; }
  DeviceGuard guard(ix->device);
  if(nq == 1)                                // the per-character caller (gcsa.h:155-162 in a loop): through the resident wavefront
  {
    u64 r[2];
    const int rc = mailbox_call(ix, MAIL_LF, in[0], in[1], comps[0], r, 2);
    if(rc == GCSA2_OK) { out[0] = r[0]; out[1] = r[1]; return GCSA2_OK; }
    if(rc != MAIL_UNAVAILABLE) { return rc; }
  }
  Lease lease(ix);
  HIP_TRY(lease.begin(2 * Lease::need(2 * nq * 8) + Lease::need(nq), true));
  u64* d_in = lease.dev<u64>(2 * nq); u64* d_out = lease.dev<u64>(2 * nq); u8* d_c = lease.dev<u8>(nq);
  HIP_TRY(lease.up(d_in, in, 2 * nq * sizeof(u64)));
  HIP_TRY(lease.up(d_c, comps, nq));
  int rc = gcsa2_lf_device(ix, d_in, d_c, nq, d_out, lease.stream());
  if(rc != GCSA2_OK) { return rc; }
  HIP_TRY(lease.down(out, d_out, 2 * nq * sizeof(u64)));
  HIP_TRY(lease.finish());
  return GCSA2_OK;
}

// The host form of extend, in one piece: patterns, offsets and states copied in, one launch, the results copied out.
int gcsa2_extend_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                       const gcsa2_search_state* states, uint64_t n_states, gcsa2_extension* out)
{
  CHECK_INDEX(ix);
  if(n_states == 0) { return GCSA2_OK; }
  if(states == nullptr || out == nullptr || (n_patterns > 0 && offsets == nullptr)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  if(n_patterns > 0 && (offsets[0] != 0 || !offsets_ok(offsets, n_patterns))) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "pattern offsets must start at 0 and be non-decreasing"); }
  const u64 total = (n_patterns > 0 ? offsets[n_patterns] : 0);
  if(patterns == nullptr && total > 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  DeviceGuard guard(ix->device);
  Lease lease(ix);
  HIP_TRY(lease.begin(Lease::need(total + 16) + Lease::need((n_patterns + 1) * 8) + 2 * Lease::need(n_states * 40), true));
  u8* d_pat = lease.dev<u8>(total + 16); u64* d_off = lease.dev<u64>(n_patterns + 1);
  gcsa2_search_state* d_states = lease.dev<gcsa2_search_state>(n_states); gcsa2_extension* d_out = lease.dev<gcsa2_extension>(n_states);
  HIP_TRY(lease.up(d_pat, patterns, total));
  if(n_patterns > 0) { HIP_TRY(lease.up(d_off, offsets, (n_patterns + 1) * sizeof(u64))); }
  HIP_TRY(lease.up(d_states, states, n_states * sizeof(gcsa2_search_state)));
  int rc = gcsa2_extend_device(ix, d_pat, d_off, n_patterns, d_states, n_states, d_out, lease.stream());
  if(rc != GCSA2_OK) { return rc; }
  HIP_TRY(lease.down(out, d_out, n_states * sizeof(gcsa2_extension)));
  HIP_TRY(lease.finish());
  return GCSA2_OK;
}

int gcsa2_lf_node_batch(const gcsa2_index* ix, const uint64_t* in, uint64_t nq, uint64_t* out)
{
  CHECK_INDEX(ix);
  if(nq == 0) { return GCSA2_OK; }
  DeviceGuard guard(ix->device);
  if(nq == 1)
  {
    const int rc = mailbox_call(ix, MAIL_LF_NODE, in[0], 0, 0, out, 1);
    if(rc != MAIL_UNAVAILABLE) { return rc; }
  }
  Lease lease(ix);
  HIP_TRY(lease.begin(2 * Lease::need(nq * 8), true));
  u64* d_in = lease.dev<u64>(nq); u64* d_out = lease.dev<u64>(nq);
  HIP_TRY(lease.up(d_in, in, nq * sizeof(u64)));
  hipLaunchKernelGGL(k_lf_node, dim3(grid_for(nq)), dim3(TPB), 0, lease.stream(), ix->img, d_in, nq, d_out);
  LAUNCH_CHECK("k_lf_node");
  HIP_TRY(lease.down(out, d_out, nq * sizeof(u64)));
  HIP_TRY(lease.finish());
  return GCSA2_OK;
}

int gcsa2_char_range(const gcsa2_index* ix, uint8_t comp, uint64_t* sp, uint64_t* ep)
{
  CHECK_INDEX(ix);
  if(comp >= ix->img.sigma) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "comp >= sigma"); }
  // charRange(comp) = find() of a one-character pattern whose byte maps to comp
  int byte = -1;
  for(int b = 0; b < 256; b++) { if(ix->img.char2comp[b] == comp) { byte = b; break; } }
  if(byte < 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "no byte maps to this comp"); }
  uint8_t pat = uint8_t(byte);
  uint64_t off[2] = {0, 1}, rng[2];
  int rc = gcsa2_find_batch(ix, &pat, off, 1, rng);
  if(rc != GCSA2_OK) { return rc; }
  *sp = rng[0]; *ep = rng[1];
  return GCSA2_OK;
}

int gcsa2_lf_all_batch(const gcsa2_index* ix, const uint64_t* in, uint64_t nq, int all, uint64_t* out)
{
  CHECK_INDEX(ix);
  if(nq == 0) { return GCSA2_OK; }
  DeviceGuard guard(ix->device);
  const u64 sigma = ix->img.sigma;
  Lease lease(ix);
  HIP_TRY(lease.begin(Lease::need(2 * nq * 8) + Lease::need(2 * nq * sigma * 8), true));
  u64* d_in = lease.dev<u64>(2 * nq); u64* d_out = lease.dev<u64>(2 * nq * sigma);
  HIP_TRY(lease.up(d_in, in, 2 * nq * sizeof(u64)));
  hipLaunchKernelGGL(k_lf_all, dim3(grid_for(nq)), dim3(TPB), 0, lease.stream(), ix->img, d_in, nq, all, d_out);
  LAUNCH_CHECK("k_lf_all");
  HIP_TRY(lease.down(out, d_out, 2 * nq * sigma * sizeof(u64)));
  HIP_TRY(lease.finish());
  return GCSA2_OK;
}

int gcsa2_count_batch(const gcsa2_index* ix, const uint64_t* ranges, uint64_t nq, uint64_t* counts)
{
  CHECK_INDEX(ix);
  if(nq == 0) { return GCSA2_OK; }
  DeviceGuard guard(ix->device);
  if(nq == 1 && ix->img.has_counters)
  {
    const int rc1 = mailbox_call(ix, MAIL_COUNT, ranges[0], ranges[1], 0, counts, 1);
    if(rc1 != MAIL_UNAVAILABLE) { return rc1; }
  }
  Lease lease(ix);
  HIP_TRY(lease.begin(Lease::need(2 * nq * 8) + Lease::need(nq * 8), true));
  u64* d_in = lease.dev<u64>(2 * nq); u64* d_out = lease.dev<u64>(nq);
  HIP_TRY(lease.up(d_in, ranges, 2 * nq * sizeof(u64)));
  int rc = gcsa2_count_device(ix, d_in, nq, d_out, lease.stream());
  if(rc != GCSA2_OK) { return rc; }
  HIP_TRY(lease.down(counts, d_out, nq * sizeof(u64)));
  HIP_TRY(lease.finish());
  return GCSA2_OK;
}

int gcsa2_locate_run(const gcsa2_index* ix, const uint64_t* ranges, uint64_t nq, int sort, uint64_t* offsets, gcsa2_locate_job** job)
{
  CHECK_INDEX(ix);
  if(offsets == nullptr || job == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  DeviceGuard guard(ix->device);
  Lease lease(ix);
  HIP_TRY(lease.begin(Lease::need(2 * nq * 8)));
  u64* d_in = lease.dev<u64>(2 * nq);
  HIP_TRY(lease.up(d_in, ranges, 2 * nq * sizeof(u64)));
  const u64* d_off = nullptr;
  int rc = gcsa2_locate_device(ix, d_in, nq, sort, job, &d_off, nullptr, nullptr, lease.stream());
  if(rc != GCSA2_OK) { return rc; }
  HIP_TRY(lease.down(offsets, d_off, (nq + 1) * sizeof(u64)));      // in the job's stream order
  HIP_TRY(lease.finish());
  (*job)->stream = nullptr;       // the lease's stream belongs to the index; the job is complete and may outlive it
  return GCSA2_OK;
}

int gcsa2_locate_fetch(gcsa2_locate_job* job, uint64_t* values, uint64_t capacity)
{
  if(job == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null job"); }
  if(capacity < job->total) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "values buffer smaller than offsets[n_queries]"); }
  {
    DeviceGuard guard(job->device);
    if(job->total > 0)
    {
      HIP_TRY(hipMemcpyAsync(values, job->d_values, job->total * sizeof(u64), hipMemcpyDeviceToHost, job->stream));
      HIP_TRY(hipStreamSynchronize(job->stream));
    }
  }
  gcsa2_locate_discard(job);
  return GCSA2_OK;
}

int gcsa2_parent_batch(const gcsa2_index* ix, const uint64_t* ranges, uint64_t nq, gcsa2_stnode* nodes)
{
  CHECK_INDEX(ix);
  if(!ix->img.has_lcp) { return fail(GCSA2_ERR_MISSING_COMPONENT, "index was created without an LCP array"); }
  if(nq == 0) { return GCSA2_OK; }
  static_assert(sizeof(gcsa2_stnode) == 5 * sizeof(u64), "gcsa2_stnode is five packed u64");
  if(nq == 1)
  {
    DeviceGuard guard(ix->device);
    const int rc = mailbox_call(ix, MAIL_PARENT, ranges[0], ranges[1], 0, reinterpret_cast<uint64_t*>(nodes), 5);
    if(rc != MAIL_UNAVAILABLE) { return rc; }
  }
  return simple_batch(ix, ranges, 2, reinterpret_cast<uint64_t*>(nodes), 5, nq, "k_parent", [&](u64* d_in, u64* d_out, hipStream_t st)
  { hipLaunchKernelGGL(k_parent, dim3(grid_for(nq)), dim3(TPB), 0, st, ix->img, d_in, nq, reinterpret_cast<gcsa2_stnode*>(d_out)); });
}

int gcsa2_depth_batch(const gcsa2_index* ix, const uint64_t* ranges, uint64_t nq, uint64_t* depths)
{
  CHECK_INDEX(ix);
  if(!ix->img.has_lcp) { return fail(GCSA2_ERR_MISSING_COMPONENT, "index was created without an LCP array"); }
  if(nq == 0) { return GCSA2_OK; }
  return simple_batch(ix, ranges, 2, depths, 1, nq, "k_depth", [&](u64* d_in, u64* d_out, hipStream_t st)
  { hipLaunchKernelGGL(k_depth, dim3(grid_for(nq)), dim3(TPB), 0, st, ix->img, d_in, nq, d_out); });
}

int gcsa2_sv_batch(const gcsa2_index* ix, int op, const uint64_t* positions, uint64_t nq, uint64_t* results)
{
  CHECK_INDEX(ix);
  if(!ix->img.has_lcp) { return fail(GCSA2_ERR_MISSING_COMPONENT, "index was created without an LCP array"); }
  if(op < 0 || op > 3) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "op must be 0..3"); }
  if(nq == 0) { return GCSA2_OK; }
  return simple_batch(ix, positions, 1, results, 2, nq, "k_sv", [&](u64* d_in, u64* d_out, hipStream_t st)
  { hipLaunchKernelGGL(k_sv, dim3(grid_for(nq)), dim3(TPB), 0, st, ix->img, op, d_in, nq, d_out); });
}

int gcsa2_rmq_batch(const gcsa2_index* ix, const uint64_t* ranges, uint64_t nq, uint64_t* results)
{
  CHECK_INDEX(ix);
  if(!ix->img.has_lcp) { return fail(GCSA2_ERR_MISSING_COMPONENT, "index was created without an LCP array"); }
  if(nq == 0) { return GCSA2_OK; }
  return simple_batch(ix, ranges, 2, results, 2, nq, "k_rmq", [&](u64* d_in, u64* d_out, hipStream_t st)
  { hipLaunchKernelGGL(k_rmq, dim3(grid_for(nq)), dim3(TPB), 0, st, ix->img, d_in, nq, d_out); });
}

int gcsa2_sample_range_batch(const gcsa2_index* ix, const uint64_t* nodes, uint64_t nq, uint64_t* out)
{
  CHECK_INDEX(ix);
  if(!ix->img.has_samples) { return fail(GCSA2_ERR_MISSING_COMPONENT, "index was created without samples"); }
  if(nq == 0) { return GCSA2_OK; }
  return simple_batch(ix, nodes, 1, out, 3, nq, "k_sample_range", [&](u64* d_in, u64* d_out, hipStream_t st)
  { hipLaunchKernelGGL(k_sample_range, dim3(grid_for(nq)), dim3(TPB), 0, st, ix->img, d_in, nq, d_out); });
}

int gcsa2_sample_batch(const gcsa2_index* ix, const uint64_t* idx, uint64_t nq, uint64_t* values, uint8_t* last)
{
  CHECK_INDEX(ix);
  if(!ix->img.has_samples) { return fail(GCSA2_ERR_MISSING_COMPONENT, "index was created without samples"); }
  if(nq == 0) { return GCSA2_OK; }
  DeviceGuard guard(ix->device);
  Lease lease(ix);
  HIP_TRY(lease.begin(2 * Lease::need(nq * 8) + Lease::need(nq), true));
  u64* d_in = lease.dev<u64>(nq); u64* d_val = lease.dev<u64>(nq); u8* d_last = lease.dev<u8>(nq);
  HIP_TRY(lease.up(d_in, idx, nq * sizeof(u64)));
  hipLaunchKernelGGL(k_sample, dim3(grid_for(nq)), dim3(TPB), 0, lease.stream(), ix->img, d_in, nq, d_val, d_last);
  LAUNCH_CHECK("k_sample");
  HIP_TRY(lease.down(values, d_val, nq * sizeof(u64)));
  HIP_TRY(lease.down(last, d_last, nq));
  HIP_TRY(lease.finish());
  return GCSA2_OK;
}

uint64_t gcsa2_sampled_positions(const gcsa2_index* ix) { return ix->img.has_samples ? ix->img.sampled.ones : 0; }
uint64_t gcsa2_lcp_size(const gcsa2_index* ix) { return ix->img.lcp_size; }
uint64_t gcsa2_lcp_values(const gcsa2_index* ix) { return ix->img.lcp_values; }
uint64_t gcsa2_lcp_levels(const gcsa2_index* ix) { return ix->img.lcp_levels; }
uint64_t gcsa2_lcp_branching(const gcsa2_index* ix) { return ix->img.lcp_branching; }
uint64_t gcsa2_sigma(const gcsa2_index* ix) { return ix->img.sigma; }
uint64_t gcsa2_fast_chars(const gcsa2_index* ix) { return ix->img.fast_chars; }
void gcsa2_derive_comp2char(const uint8_t* char2comp, uint64_t sigma, uint8_t* comp2char)
{
  if(char2comp == nullptr || comp2char == nullptr) { return; }
  for(u64 c = 0; c < sigma; c++)
  {
    int first = -1, upper = -1;
    for(int b = 0; b < 256; b++)
    {
      if(char2comp[b] != c) { continue; }
      if(first < 0) { first = b; }
      if(upper < 0 && !(b >= 'a' && b <= 'z') && b != 0) { upper = b; }
    }
    comp2char[c] = u8(upper >= 0 ? upper : (first >= 0 ? first : 0));
  }
  if(sigma == 7)
  {
    const char* dflt = "$ACGTN#";
    bool is_default = true;
    for(u64 c = 0; c < 7; c++) { is_default = is_default && char2comp[u8(dflt[c])] == c; }
    if(is_default) { for(u64 c = 0; c < 7; c++) { comp2char[c] = u8(dflt[c]); } }
  }
}

void gcsa2_alphabet(const gcsa2_index* ix, uint8_t* char2comp, uint64_t* C)
{
  if(char2comp) { std::memcpy(char2comp, ix->img.char2comp, 256); }
  if(C) { for(u64 c = 0; c <= ix->img.sigma; c++) { C[c] = ix->img.C[c]; } }
}

int gcsa2_lcp_access_batch(const gcsa2_index* ix, const uint64_t* positions, uint64_t nq, uint64_t* out)
{
  CHECK_INDEX(ix);
  if(!ix->img.has_lcp) { return fail(GCSA2_ERR_MISSING_COMPONENT, "index was created without an LCP array"); }
  if(nq == 0) { return GCSA2_OK; }
  return simple_batch(ix, positions, 1, out, 1, nq, "k_lcp_access", [&](u64* d_in, u64* d_out, hipStream_t st)
  { hipLaunchKernelGGL(k_lcp_access, dim3(grid_for(nq)), dim3(TPB), 0, st, ix->img, d_in, nq, d_out); });
}

// GCSA::locate(range, max_positions, results) (src/gcsa.cpp:844-878): host control flow with the
// reference's std::mt19937_64 draws; every locateInternal() runs on the device.  The reference's
// unordered_set is replaced by a sorted unique vector: its iteration order never reaches the
// output, because deterministicShuffle sorts first (utils.h:359-370) and the result is sorted last.
int gcsa2_locate_max(const gcsa2_index* ix, uint64_t sp, uint64_t ep, uint64_t max_positions,
                     uint64_t* values, uint64_t capacity, uint64_t* count_out)
{
  CHECK_INDEX(ix);
  if(count_out == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null count pointer"); }
  *count_out = 0;
  try {   // no C++ exception may cross the C boundary
  uint64_t range[2] = {sp, ep}, total = 0;
  int rc = gcsa2_count_batch(ix, range, 1, &total);
  if(rc != GCSA2_OK) { return rc; }
  if(total == 0) { return GCSA2_OK; }
  if(max_positions > total) { max_positions = total; }
  std::mt19937_64 rng(sp ^ ep);
  std::vector<u64> results;
  auto locate_ranges = [&](const std::vector<u64>& rr, std::vector<u64>& dst) -> int
  {
    u64 nq = rr.size() / 2;
    std::vector<u64> offs(nq + 1);
    gcsa2_locate_job* job = nullptr;
    int r = gcsa2_locate_run(ix, rr.data(), nq, 1, offs.data(), &job);
    if(r != GCSA2_OK) { return r; }
    dst.resize(offs[nq]);
    return gcsa2_locate_fetch(job, dst.data(), dst.size());
  };
  if(max_positions >= total / 2)   // just locate everything (gcsa.cpp:855-858)
  {
    rc = locate_ranges({sp, ep}, results);
    if(rc != GCSA2_OK) { return rc; }
  }
  else                             // random positions until enough distinct values (gcsa.cpp:859-871)
  {
    std::vector<u64> found, tmp;
    while(found.size() < max_positions)
    {
      u64 pos = sp + rng() % (ep + 1 - sp);
      rc = locate_ranges({pos, pos}, tmp);
      if(rc != GCSA2_OK) { return rc; }
      found.insert(found.end(), tmp.begin(), tmp.end());
      std::sort(found.begin(), found.end());
      found.erase(std::unique(found.begin(), found.end()), found.end());
    }
    results.swap(found);
  }
  if(results.size() > max_positions)   // deterministicShuffle + truncate (gcsa.cpp:873-877)
  {
    std::sort(results.begin(), results.end());
    for(u64 i = results.size(); i > 0; i--) { std::swap(results[i - 1], results[rng() % i]); }
    results.resize(max_positions);
  }
  std::sort(results.begin(), results.end());
  if(results.size() > capacity) { *count_out = results.size(); return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "values buffer too small"); }
  std::memcpy(values, results.data(), results.size() * sizeof(u64));
  *count_out = results.size();
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_locate_max: ") + e.what()); }
}

}  // extern "C"

namespace {
// GCSA::locate(range, max_positions) of one range for the batch's host path: the reference's control flow and draws, like
// gcsa2_locate_max, with every loop bounded.  In the random branch the range's distinct values are counted first: with fewer
// than m of them the reference's loop never ends, and the call fails instead.  The draws then go 256 at a time through one
// locate pass (a copy of the generator makes them; the generator itself advances by the draws used), at most 64 m + 64 of
// them, as in the kernel.
int locate_max_bounded(const gcsa2_index* ix, u64 sp, u64 ep, u64 max_positions, std::vector<u64>& results)
{
  results.clear();
  u64 range[2] = {sp, ep}, total = 0;
  int rc = gcsa2_count_batch(ix, range, 1, &total);
  if(rc != GCSA2_OK) { return rc; }
  if(total == 0) { return GCSA2_OK; }
  const u64 m = (max_positions < total ? max_positions : total);
  std::mt19937_64 rng(sp ^ ep);
  auto locate_ranges = [&](const std::vector<u64>& rr, int sort, std::vector<u64>& offs, std::vector<u64>& dst) -> int
  {
    const u64 n = rr.size() / 2;
    offs.assign(n + 1, 0);
    gcsa2_locate_job* job = nullptr;
    int r = gcsa2_locate_run(ix, rr.data(), n, sort, offs.data(), &job);
    if(r != GCSA2_OK) { return r; }
    dst.resize(offs[n] > 0 ? offs[n] : 1);
    r = gcsa2_locate_fetch(job, dst.data(), dst.size());
    dst.resize(offs[n]);
    return r;
  };
  std::vector<u64> offs;
  rc = locate_ranges({sp, ep}, 1, offs, results);               // every distinct value (gcsa.cpp:855-858)
  if(rc != GCSA2_OK) { return rc; }
  if(m < total / 2)                                              // random positions (gcsa.cpp:859-871)
  {
    if(results.size() < m)
    {
      return fail(GCSA2_ERR_INVALID_ARGUMENT, "locate_max: range (" + std::to_string(sp) + ", " + std::to_string(ep) + ") has " +
                  std::to_string(results.size()) + " distinct values, fewer than max_positions and count() (" + std::to_string(total) +
                  ") would make the reference draw forever");
    }
    const u64 most = 64 * m + 64;                                // m <= the range's distinct values < 2^40
    std::unordered_set<u64> found;
    std::vector<u64> batch, boffs, bvals;
    u64 draws = 0;
    while(found.size() < m)
    {
      if(draws >= most)
      {
        return fail(GCSA2_ERR_INVALID_ARGUMENT, "locate_max: range (" + std::to_string(sp) + ", " + std::to_string(ep) +
                    ") drew 64 * max_positions + 64 positions without finding max_positions distinct values");
      }
      const u64 want = (most - draws < 256 ? most - draws : 256);
      std::mt19937_64 ahead = rng;
      batch.clear();
      for(u64 k = 0; k < want; k++) { const u64 pos = sp + ahead() % (ep + 1 - sp); batch.push_back(pos); batch.push_back(pos); }
      rc = locate_ranges(batch, 0, boffs, bvals);
      if(rc != GCSA2_OK) { return rc; }
      u64 used = want;
      for(u64 k = 0; k < want; k++)
      {
        for(u64 i = boffs[k]; i < boffs[k + 1]; i++) { found.insert(bvals[i]); }
        if(found.size() >= m) { used = k + 1; break; }
      }
      rng.discard(used); draws += used;
    }
    results.assign(found.begin(), found.end());
  }
  if(results.size() > m)                                         // deterministicShuffle + truncate (gcsa.cpp:873-877)
  {
    std::sort(results.begin(), results.end());
    for(u64 i = results.size(); i > 0; i--) { std::swap(results[i - 1], results[rng() % i]); }
    results.resize(m);
  }
  std::sort(results.begin(), results.end());
  return GCSA2_OK;
}

// Batched locate(range, max_positions) (kernels_locate_max.hpp): sizes min(max_positions, count) -- a range with a wrapped
// count() answered on the host first and given its real size --, their exclusive scan into d_offsets, the total read back,
// the value buffer from `provide`, one wavefront per range, then the ranges beyond the kernel's LDS budget through
// locate_max_bounded.  A range with fewer values than its slot (count() overstating its distinct values, which the reference
// allows) leaves a gap that is closed on the host, offsets included.  Synchronous.  Nothing is written to the values when
// `provide` refuses their number.
int locate_max_core(const gcsa2_index* ix, const u64* d_ranges, u64 nq, u64 max_positions, u64* d_offsets,
                    const std::function<int(u64, u64**)>& provide, u64* total_out, hipStream_t st)
{
  *total_out = 0;
  if(nq >= LMAX_BATCH) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "locate_max batch of >= 2^24 ranges; split the batch"); }
  if(nq == 0) { HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(u64), st)); HIP_TRY(hipStreamSynchronize(st)); return GCSA2_OK; }
  struct Bufs
  {
    hipStream_t st; u64* sizes = nullptr; u64* list = nullptr; u64* odd = nullptr; void* tmp = nullptr; unsigned long long* ctl = nullptr;
    ~Bufs() { for(void* p : {(void*)sizes, (void*)list, (void*)odd, tmp, (void*)ctl}) { if(p) { (void)hipFreeAsync(p, st); } } }
  } b{st};
  HIP_TRY(pool_alloc(ix, reinterpret_cast<void**>(&b.sizes), (nq + 1) * sizeof(u64), st));
  HIP_TRY(pool_alloc(ix, reinterpret_cast<void**>(&b.list), nq * sizeof(u64), st));
  HIP_TRY(pool_alloc(ix, reinterpret_cast<void**>(&b.odd), nq * sizeof(u64), st));
  HIP_TRY(pool_alloc(ix, reinterpret_cast<void**>(&b.ctl), 4 * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(b.ctl, 0, 4 * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(b.ctl + 2, 0xFF, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_locate_max_sizes, dim3(grid_for(nq + 1)), dim3(TPB), 0, st, ix->img, d_ranges, nq, max_positions, b.sizes, b.ctl, b.odd);
  LAUNCH_CHECK("k_locate_max_sizes");
  unsigned long long ctl[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(ctl, b.ctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  std::vector<std::pair<u64, std::vector<u64>>> odd(ctl[3]);     // (range, values): ranges whose count() wrapped
  if(!odd.empty())
  {
    std::vector<u64> list(odd.size());
    HIP_TRY(hipMemcpy(list.data(), b.odd, list.size() * sizeof(u64), hipMemcpyDeviceToHost));
    std::sort(list.begin(), list.end());
    for(size_t i = 0; i < list.size(); i++)
    {
      u64 r[2];
      HIP_TRY(hipMemcpy(r, d_ranges + 2 * list[i], sizeof(r), hipMemcpyDeviceToHost));
      odd[i].first = list[i];
      int rc = locate_max_bounded(ix, r[0], r[1], max_positions, odd[i].second);
      if(rc != GCSA2_OK) { return rc; }
      const u64 size = odd[i].second.size();
      HIP_TRY(hipMemcpy(b.sizes + list[i], &size, sizeof(u64), hipMemcpyHostToDevice));
    }
  }
  size_t tmp_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, b.sizes, d_offsets, size_t(nq + 1), st));
  HIP_TRY(pool_alloc(ix, &b.tmp, tmp_bytes, st));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(b.tmp, tmp_bytes, b.sizes, d_offsets, size_t(nq + 1), st));
  u64 total = 0;
  HIP_TRY(hipMemcpyAsync(&total, d_offsets + nq, sizeof(u64), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *total_out = total;
  if(total == 0) { return GCSA2_OK; }
  u64* d_values = nullptr;
  const int got_values = provide(total, &d_values);
  if(got_values != GCSA2_OK) { return got_values; }
  const u64 grid = (nq < (u64(1) << 20) ? nq : (u64(1) << 20));
  hipLaunchKernelGGL(k_locate_max, dim3(unsigned(grid)), dim3(64), 0, st, ix->img, d_ranges, nq, max_positions, d_offsets, d_values, b.ctl, b.list, b.sizes);
  LAUNCH_CHECK("k_locate_max");
  HIP_TRY(hipMemcpyAsync(ctl, b.ctl, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if(ctl[0] & (LMAX_FLAG_DRAWS | LMAX_FLAG_SLOT))
  {
    const std::string what = (ctl[0] & LMAX_FLAG_DRAWS) ? "drew 64 * max_positions + 64 positions without finding max_positions distinct values"
                                                        : "changed its count() between the two passes";
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "locate_max: range " + std::to_string(ctl[2]) + " " + what +
                                            " (count() overstates the range's values: a broken index)");
  }
  for(const auto& o : odd)   // their slots have their real sizes
  {
    u64 off = 0;
    HIP_TRY(hipMemcpy(&off, d_offsets + o.first, sizeof(u64), hipMemcpyDeviceToHost));
    if(!o.second.empty()) { HIP_TRY(hipMemcpy(d_values + off, o.second.data(), o.second.size() * sizeof(u64), hipMemcpyHostToDevice)); }
  }
  bool short_ranges = (ctl[0] & LMAX_FLAG_SIZE) != 0;
  std::vector<std::pair<u64, u64>> short_fallbacks;         // (range, values) of per-range results shorter than their slot
  if(ctl[1] > 0)      // beyond the LDS budget: the per-range path, written into the range's slot
  {
    std::vector<u64> list(ctl[1]), got;
    HIP_TRY(hipMemcpy(list.data(), b.list, list.size() * sizeof(u64), hipMemcpyDeviceToHost));
    std::sort(list.begin(), list.end());
    for(u64 q : list)
    {
      u64 r[2], off[2];
      HIP_TRY(hipMemcpy(r, d_ranges + 2 * q, sizeof(r), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(off, d_offsets + q, sizeof(off), hipMemcpyDeviceToHost));
      int rc = locate_max_bounded(ix, r[0], r[1], max_positions, got);
      if(rc != GCSA2_OK) { return rc; }
      const u64 cnt = got.size();
      if(cnt > off[1] - off[0]) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "locate_max: a range's result is larger than its slot"); }
      if(cnt < off[1] - off[0]) { short_fallbacks.emplace_back(q, cnt); short_ranges = true; }
      if(cnt > 0) { HIP_TRY(hipMemcpy(d_values + off[0], got.data(), cnt * sizeof(u64), hipMemcpyHostToDevice)); }
    }
  }
  if(short_ranges)    // ranges with fewer values than their slot (count() overstating them): close the gaps, new offsets
  {
    std::vector<u64> offs(nq + 1), sizes(nq), vals(total);
    HIP_TRY(hipMemcpy(offs.data(), d_offsets, offs.size() * sizeof(u64), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sizes.data(), b.sizes, sizes.size() * sizeof(u64), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vals.data(), d_values, vals.size() * sizeof(u64), hipMemcpyDeviceToHost));
    for(const auto& f : short_fallbacks) { sizes[f.first] = f.second; }
    u64 kept = 0;
    for(u64 q = 0; q < nq; q++)
    {
      const u64 from = offs[q], len = sizes[q];
      offs[q] = kept;
      std::memmove(vals.data() + kept, vals.data() + from, len * sizeof(u64));
      kept += len;
    }
    offs[nq] = kept;
    HIP_TRY(hipMemcpy(d_offsets, offs.data(), offs.size() * sizeof(u64), hipMemcpyHostToDevice));
    if(kept > 0) { HIP_TRY(hipMemcpy(d_values, vals.data(), kept * sizeof(u64), hipMemcpyHostToDevice)); }
    *total_out = kept;
  }
  return GCSA2_OK;
}
}  // namespace

extern "C" {

int gcsa2_locate_max_into(const gcsa2_index* ix, const uint64_t* d_ranges, uint64_t nq, uint64_t max_positions, uint64_t* d_offsets,
                          uint64_t* d_values, uint64_t capacity, uint64_t* total, void* stream)
{
  CHECK_INDEX(ix);
  if(total == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null total pointer"); }
  *total = 0;
  if(d_offsets == nullptr || (d_ranges == nullptr && nq > 0) || (d_values == nullptr && capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  int rc = locate_checks(ix, nq);
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  auto provide = [d_values, capacity](u64 count, u64** out) -> int
  {
    if(count > capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "values buffer too small"); }
    *out = d_values;
    return GCSA2_OK;
  };
  const int core_rc = locate_max_core(ix, d_ranges, nq, max_positions, d_offsets, provide, total, static_cast<hipStream_t>(stream));
  // the core releases its stream-ordered scratch (hipFreeAsync) behind its last wait: "complete on return" is an idle stream
  const hipError_t idle = hipStreamSynchronize(static_cast<hipStream_t>(stream));
  if(core_rc == GCSA2_OK && idle != hipSuccess) { return fail(GCSA2_ERR_HIP, std::string("gcsa2_locate_max_into: ") + hipGetErrorString(idle)); }
  return core_rc;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_locate_max_into: ") + e.what()); }
}

int gcsa2_locate_max_batch(const gcsa2_index* ix, const uint64_t* ranges, uint64_t nq, uint64_t max_positions, uint64_t* offsets,
                           uint64_t* values, uint64_t capacity, uint64_t* total)
{
  CHECK_INDEX(ix);
  if(total == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null total pointer"); }
  *total = 0;
  if(offsets == nullptr || (ranges == nullptr && nq > 0) || (values == nullptr && capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  int rc = locate_checks(ix, nq);
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  struct Bufs { u64* ranges = nullptr; u64* offsets = nullptr; u64* values = nullptr;
                ~Bufs() { for(u64* p : {ranges, offsets, values}) { if(p) { (void)hipFree(p); } } } } b;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b.ranges), (nq > 0 ? 2 * nq : 1) * sizeof(u64)));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b.offsets), (nq + 1) * sizeof(u64)));
  if(nq > 0) { HIP_TRY(hipMemcpy(b.ranges, ranges, 2 * nq * sizeof(u64), hipMemcpyHostToDevice)); }
  auto provide = [&b, capacity](u64 count, u64** out) -> int
  {
    if(count > capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "values buffer too small"); }
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&b.values), count * sizeof(u64)));
    *out = b.values;
    return GCSA2_OK;
  };
  rc = locate_max_core(ix, b.ranges, nq, max_positions, b.offsets, provide, total, nullptr);
  if(rc == GCSA2_OK || rc == GCSA2_ERR_BUFFER_TOO_SMALL) { HIP_TRY(hipMemcpy(offsets, b.offsets, (nq + 1) * sizeof(u64), hipMemcpyDeviceToHost)); }
  if(rc != GCSA2_OK) { return rc; }
  if(*total > 0) { HIP_TRY(hipMemcpy(values, b.values, *total * sizeof(u64), hipMemcpyDeviceToHost)); }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_locate_max_batch: ") + e.what()); }
}

}  // extern "C"

namespace {
int match_stats_launch(const gcsa2_index* ix, int variant, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t nq, u64 total_bytes,
                       uint16_t* d_ms, uint64_t* d_ranges, uint64_t* d_fallbacks, hipStream_t st, const BreakSink* sink = nullptr);
int group_comm_init(gcsa2_group* g);
}  // namespace

#include "comm.hpp"

extern "C" {

// ---- single-process multi-GPU: replicated index, contiguous query shards ---------------------
// Queries are independent and the index is read-only (the reference's only data-parallel query
// path is the static split of verifyIndex, src/algorithms.cpp:106-114), so every device gets a
// replica and a contiguous shard.  gcsa2_group_find_batch (host buffers): one host thread per device
// stages its shard, runs k_find2 and copies its ranges straight into the caller's buffer.
// gcsa2_group_find_device (device buffers): every device searches its shard on its own stream and the
// ranges are gathered in the root's HBM with one grouped RCCL send / recv over xGMI (comm.hpp).

struct gcsa2_group
{
  std::vector<gcsa2_index*> replicas;
  std::vector<hipStream_t> streams;        // one per replica, on its device
  std::vector<ncclComm_t> comms;           // ncclCommInitAll over the device list; empty = peer copies instead
  std::vector<u64*> scratch;               // per replica: ranges of its shard before the gather (replicas 1..)
  std::vector<u64> scratch_pairs;
  bool comm_tried = false;
  std::mutex lock;                         // group_find_device calls are serialized (they share streams and scratch)
};

int gcsa2_group_create(const gcsa2_host_view* view, const int* devices, int n_devices, gcsa2_group** out)
{
  if(view == nullptr || devices == nullptr || out == nullptr || n_devices <= 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "bad group arguments"); }
  *out = nullptr;
  gcsa2_group* g = new(std::nothrow) gcsa2_group();
  if(g == nullptr) { return fail(GCSA2_ERR_OUT_OF_MEMORY, "host allocation failed"); }
  for(int i = 0; i < n_devices; i++)
  {
    gcsa2_index* ix = nullptr;
    int rc = gcsa2_index_create(view, devices[i], &ix);
    hipStream_t st = nullptr;
    if(rc == GCSA2_OK)
    {
      DeviceGuard guard(devices[i]);
      if(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { rc = fail(GCSA2_ERR_HIP, "hipStreamCreate failed"); gcsa2_index_destroy(ix); }
    }
    if(rc != GCSA2_OK)
    {
      std::string msg = g_error;
      gcsa2_group_destroy(g);
      return fail(rc, msg);
    }
    g->replicas.push_back(ix); g->streams.push_back(st);
    g->scratch.push_back(nullptr); g->scratch_pairs.push_back(0);
  }
  *out = g;
  return GCSA2_OK;
}

void gcsa2_group_destroy(gcsa2_group* g)
{
  if(g == nullptr) { return; }
  for(size_t i = 0; i < g->comms.size(); i++)
  {
    if(g->comms[i] != nullptr) { DeviceGuard guard(g->replicas[i]->device); (void)rccl().CommDestroy(g->comms[i]); }
  }
  for(size_t i = 0; i < g->replicas.size(); i++)
  {
    DeviceGuard guard(g->replicas[i]->device);
    if(i < g->streams.size() && g->streams[i] != nullptr) { (void)hipStreamDestroy(g->streams[i]); }
    if(i < g->scratch.size() && g->scratch[i] != nullptr) { (void)hipFree(g->scratch[i]); }
  }
  for(gcsa2_index* r : g->replicas) { gcsa2_index_destroy(r); }
  delete g;
}

int gcsa2_group_uses_rccl(const gcsa2_group* g) { return (g != nullptr && !g->comms.empty()) ? 1 : 0; }

int gcsa2_group_find_device(gcsa2_group* g, const uint8_t* const* d_patterns, const uint64_t* const* d_offsets,
                            const uint64_t* counts, uint64_t* d_ranges_root)
{
  if(g == nullptr || g->replicas.empty()) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null or empty group"); }
  if(d_patterns == nullptr || d_offsets == nullptr || counts == nullptr || d_ranges_root == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  try {
  std::lock_guard<std::mutex> hold(g->lock);
  const int G = int(g->replicas.size());
  { int rc = group_comm_init(g); if(rc != GCSA2_OK) { return rc; } }
  // every replica searches its shard on its own stream; replica 0 writes straight into the result buffer
  std::vector<u64> first(size_t(G) + 1, 0);
  for(int r = 0; r < G; r++) { first[size_t(r) + 1] = first[size_t(r)] + counts[r]; }
  for(int r = 0; r < G; r++)
  {
    if(counts[r] == 0) { continue; }
    u64* dst = d_ranges_root;
    if(r > 0)
    {
      DeviceGuard guard(g->replicas[r]->device);
      if(g->scratch_pairs[r] < counts[r])
      {
        if(g->scratch[r] != nullptr) { (void)hipFree(g->scratch[r]); g->scratch[r] = nullptr; g->scratch_pairs[r] = 0; }
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&g->scratch[r]), counts[r] * 2 * sizeof(u64)));
        g->scratch_pairs[r] = counts[r];
      }
      dst = g->scratch[r];
    }
    int rc = gcsa2_find_device(g->replicas[r], d_patterns[r], d_offsets[r], counts[r], dst, g->streams[r]);
    if(rc != GCSA2_OK) { return rc; }
  }
  // the gather: ranges of replica r land at d_ranges_root + 2 * first[r]
  if(!g->comms.empty())
  {
    RcclApi& api = rccl();
    RCCL_TRY(api.GroupStart());
    ncclResult_t res = ncclSuccess;
    for(int r = 1; r < G && res == ncclSuccess; r++)
    {
      if(counts[r] == 0) { continue; }
      res = api.Send(g->scratch[r], counts[r] * 2, ncclUint64, 0, g->comms[r], g->streams[r]);
      if(res == ncclSuccess) { res = api.Recv(d_ranges_root + 2 * first[r], counts[r] * 2, ncclUint64, r, g->comms[0], g->streams[0]); }
    }
    ncclResult_t end = api.GroupEnd();
    if(res != ncclSuccess) { return fail(GCSA2_ERR_HIP, std::string("ncclSend / ncclRecv: ") + api.GetErrorString(res)); }
    if(end != ncclSuccess) { return fail(GCSA2_ERR_HIP, std::string("ncclGroupEnd: ") + api.GetErrorString(end)); }
  }
  else
  {
    for(int r = 1; r < G; r++)
    {
      if(counts[r] == 0) { continue; }
      DeviceGuard guard(g->replicas[r]->device);
      HIP_TRY(hipMemcpyPeerAsync(d_ranges_root + 2 * first[r], g->replicas[0]->device, g->scratch[r], g->replicas[r]->device,
                                 counts[r] * 2 * sizeof(u64), g->streams[r]));
    }
  }
  for(int r = 0; r < G; r++)
  {
    DeviceGuard guard(g->replicas[r]->device);
    HIP_TRY(hipStreamSynchronize(g->streams[r]));
  }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_group_find_device: ") + e.what()); }
}

}  // extern "C"

namespace {

// The gather of the group entry points: src[r] (bytes[r] bytes, on the device of replica r, produced on streams[r]) lands at
// dst_root + at[r] on the device of replica 0.  One grouped RCCL send / recv when the group has a communicator, peer copies
// otherwise.  Replica 0's own part is a device copy on its stream (skipped when it is already in place).
int group_gather(gcsa2_group* g, const std::vector<const void*>& src, const std::vector<u64>& bytes, char* dst_root, const std::vector<u64>& at)
{
  const int G = int(g->replicas.size());
  if(bytes[0] > 0 && src[0] != dst_root + at[0])
  {
    DeviceGuard guard(g->replicas[0]->device);
    HIP_TRY(hipMemcpyAsync(dst_root + at[0], src[0], bytes[0], hipMemcpyDeviceToDevice, g->streams[0]));
  }
  if(!g->comms.empty())
  {
    RcclApi& api = rccl();
    RCCL_TRY(api.GroupStart());
    ncclResult_t res = ncclSuccess;
    for(int r = 1; r < G && res == ncclSuccess; r++)
    {
      if(bytes[size_t(r)] == 0) { continue; }
      res = api.Send(src[size_t(r)], bytes[size_t(r)], ncclUint8, 0, g->comms[size_t(r)], g->streams[size_t(r)]);
      if(res == ncclSuccess) { res = api.Recv(dst_root + at[size_t(r)], bytes[size_t(r)], ncclUint8, r, g->comms[0], g->streams[0]); }
    }
    ncclResult_t end = api.GroupEnd();
    if(res != ncclSuccess) { return fail(GCSA2_ERR_HIP, std::string("ncclSend / ncclRecv: ") + api.GetErrorString(res)); }
    if(end != ncclSuccess) { return fail(GCSA2_ERR_HIP, std::string("ncclGroupEnd: ") + api.GetErrorString(end)); }
  }
  else
  {
    for(int r = 1; r < G; r++)
    {
      if(bytes[size_t(r)] == 0) { continue; }
      DeviceGuard guard(g->replicas[size_t(r)]->device);
      HIP_TRY(hipMemcpyPeerAsync(dst_root + at[size_t(r)], g->replicas[0]->device, src[size_t(r)], g->replicas[size_t(r)]->device,
                                 bytes[size_t(r)], g->streams[size_t(r)]));
    }
  }
  return GCSA2_OK;
}

int group_sync(gcsa2_group* g)
{
  for(size_t r = 0; r < g->replicas.size(); r++)
  {
    DeviceGuard guard(g->replicas[r]->device);
    HIP_TRY(hipStreamSynchronize(g->streams[r]));
  }
  return GCSA2_OK;
}

// One communicator per device (ncclCommInitAll), made at the first device-resident group call.  RCCL needs distinct
// devices; a group that lists a device twice (or a host without RCCL) gathers with peer copies instead.
int group_comm_init(gcsa2_group* g)
{
  if(g->comm_tried) { return GCSA2_OK; }
  g->comm_tried = true;
  const int G = int(g->replicas.size());
  std::vector<int> devs;
  bool distinct = true;
  for(int r = 0; r < G; r++)
  {
    for(int d : devs) { distinct = distinct && d != g->replicas[size_t(r)]->device; }
    devs.push_back(g->replicas[size_t(r)]->device);
  }
  if(G > 1 && distinct && rccl().ok)
  {
    g->comms.assign(size_t(G), nullptr);
    ncclResult_t r = rccl().CommInitAll(g->comms.data(), G, devs.data());
    if(r != ncclSuccess) { g->comms.clear(); return fail(GCSA2_ERR_HIP, std::string("ncclCommInitAll: ") + rccl().GetErrorString(r)); }
  }
  return GCSA2_OK;
}

__global__ __launch_bounds__(TPB) void k_rebase_offsets(u64* __restrict__ offsets, u64 count, u64 base)
{
  const u64 i = u64(blockIdx.x) * TPB + threadIdx.x;
  if(i < count) { offsets[i] += base; }
}

}  // namespace

extern "C" {

// Matching statistics of a batch sharded over the group (BASELINE configs[4] on N GPUs): replica r runs its shard
// (d_patterns[r], d_offsets[r] rebased to 0, counts[r] patterns of pattern_bytes[r] bytes in all) and the three result arrays
// are gathered on replica 0's device in query order.  Complete on return.
int gcsa2_group_match_stats_device(gcsa2_group* g, const uint8_t* const* d_patterns, const uint64_t* const* d_offsets, const uint64_t* counts,
                                   const uint64_t* pattern_bytes, uint16_t* d_ms_root, uint64_t* d_ranges_root, uint64_t* d_fallbacks_root)
{
  if(g == nullptr || g->replicas.empty()) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null or empty group"); }
  if(d_patterns == nullptr || d_offsets == nullptr || counts == nullptr || pattern_bytes == nullptr || d_ms_root == nullptr || d_ranges_root == nullptr)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  try {
  std::lock_guard<std::mutex> hold(g->lock);
  const size_t G = g->replicas.size();
  int rc = group_comm_init(g);
  if(rc != GCSA2_OK) { return rc; }
  std::vector<const void*> ms(G, nullptr), rng(G, nullptr), fb(G, nullptr);
  std::vector<u64> ms_bytes(G, 0), rng_bytes(G, 0), fb_bytes(G, 0), ms_at(G, 0), rng_at(G, 0), fb_at(G, 0);
  std::vector<void*> scratch;
  struct Release { gcsa2_group* g; std::vector<void*>& p; std::vector<int> dev; ~Release() { for(size_t i = 0; i < p.size(); i++) { DeviceGuard guard(dev[i]); (void)hipFree(p[i]); } } } release{g, scratch, {}};
  u64 q_before = 0, b_before = 0;
  for(size_t r = 0; r < G; r++)
  {
    ms_at[r] = 2 * b_before; rng_at[r] = 16 * q_before; fb_at[r] = 8 * q_before;
    ms_bytes[r] = 2 * pattern_bytes[r]; rng_bytes[r] = 16 * counts[r]; fb_bytes[r] = 8 * counts[r];
    q_before += counts[r]; b_before += pattern_bytes[r];
    if(counts[r] == 0) { continue; }
    const gcsa2_index* ix = g->replicas[r];
    DeviceGuard guard(ix->device);
    // the kernel wants an 8-byte aligned statistics array with 4 spare entries: a scratch copy per replica (replica 0's
    // slice of the result starts at 0 and is used in place)
    char* buf = nullptr;
    const u64 ms_room = (2 * pattern_bytes[r] + 8 * sizeof(uint16_t) + 15) / 16 * 16;
    uint16_t* my_ms = d_ms_root; u64* my_rng = d_ranges_root; u64* my_fb = d_fallbacks_root;
    if(r > 0)
    {
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&buf), ms_room + 24 * counts[r]));
      scratch.push_back(buf); release.dev.push_back(ix->device);
      my_ms = reinterpret_cast<uint16_t*>(buf); my_rng = reinterpret_cast<u64*>(buf + ms_room); my_fb = my_rng + 2 * counts[r];
    }
    else if(d_fallbacks_root == nullptr) { fb_bytes[0] = 0; }
    rc = match_stats_launch(ix, 0, d_patterns[r], d_offsets[r], counts[r], pattern_bytes[r], my_ms, my_rng, my_fb, g->streams[r]);
    if(rc != GCSA2_OK) { return rc; }
    ms[r] = my_ms; rng[r] = my_rng; fb[r] = my_fb;
  }
  if(d_fallbacks_root == nullptr) { for(size_t r = 0; r < G; r++) { fb_bytes[r] = 0; } }
  rc = group_gather(g, ms, ms_bytes, reinterpret_cast<char*>(d_ms_root), ms_at);
  if(rc == GCSA2_OK) { rc = group_gather(g, rng, rng_bytes, reinterpret_cast<char*>(d_ranges_root), rng_at); }
  if(rc == GCSA2_OK && d_fallbacks_root != nullptr) { rc = group_gather(g, fb, fb_bytes, reinterpret_cast<char*>(d_fallbacks_root), fb_at); }
  int sc = group_sync(g);
  return rc != GCSA2_OK ? rc : sc;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_group_match_stats_device: ") + e.what()); }
}

// locate() of a batch of ranges sharded over the group: replica r locates d_ranges[r] (counts[r] ranges); the root receives the
// CSR of the whole batch in query order -- per-rank totals first, then the offsets (rebased) and the values (SURVEY.md 8(e):
// "all-gather of per-rank counts, then gatherv of the CSR values").  *job owns the values on replica 0's device.
int gcsa2_group_locate_device(gcsa2_group* g, const uint64_t* const* d_ranges, const uint64_t* counts, int sort, uint64_t* d_offsets_root,
                              gcsa2_locate_job** job_out, const uint64_t** d_values_root, uint64_t* total_values)
{
  if(g == nullptr || g->replicas.empty()) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null or empty group"); }
  if(d_ranges == nullptr || counts == nullptr || d_offsets_root == nullptr || job_out == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  *job_out = nullptr;
  try {
  std::lock_guard<std::mutex> hold(g->lock);
  const size_t G = g->replicas.size();
  int rc = group_comm_init(g);
  if(rc != GCSA2_OK) { return rc; }
  // every replica locates its shard from its own host thread (the locate pipeline synchronises its stream)
  std::vector<gcsa2_locate_job*> jobs(G, nullptr);
  std::vector<int> status(G, GCSA2_OK);
  std::vector<std::string> messages(G);
  struct Discard { std::vector<gcsa2_locate_job*>& j; ~Discard() { for(gcsa2_locate_job* x : j) { gcsa2_locate_discard(x); } } } discard{jobs};
  {
    Workers workers;
    for(size_t r = 0; r < G; r++)
    {
      workers.emplace_back([&, r]()
      {
        status[r] = gcsa2_locate_device(g->replicas[r], d_ranges[r], counts[r], sort, &jobs[r], nullptr, nullptr, nullptr, g->streams[r]);
        if(status[r] != GCSA2_OK) { messages[r] = g_error; }
      });
    }
    workers.join();
  }
  for(size_t r = 0; r < G; r++) { if(status[r] != GCSA2_OK) { return fail(status[r], "shard " + std::to_string(r) + ": " + messages[r]); } }
  u64 total = 0, q_before = 0;
  std::vector<const void*> off(G, nullptr), val(G, nullptr);
  std::vector<u64> off_bytes(G, 0), val_bytes(G, 0), off_at(G, 0), val_at(G, 0), base(G, 0);
  for(size_t r = 0; r < G; r++)
  {
    base[r] = total; off_at[r] = 8 * q_before; val_at[r] = 8 * total;
    off[r] = jobs[r]->d_offsets; off_bytes[r] = 8 * counts[r];
    val[r] = jobs[r]->d_values; val_bytes[r] = 8 * jobs[r]->total;
    total += jobs[r]->total; q_before += counts[r];
  }
  const gcsa2_index* root = g->replicas[0];
  gcsa2_locate_job* result = new(std::nothrow) gcsa2_locate_job();
  if(result == nullptr) { return fail(GCSA2_ERR_OUT_OF_MEMORY, "host allocation failed"); }
  result->device = root->device; result->nq = q_before; result->total = total;
  {
    DeviceGuard guard(root->device);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&result->d_values), (total > 0 ? total : 1) * sizeof(u64));
    if(e != hipSuccess) { delete result; return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("hipMalloc(values): ") + hipGetErrorString(e)); }
  }
  rc = group_gather(g, off, off_bytes, reinterpret_cast<char*>(d_offsets_root), off_at);
  if(rc == GCSA2_OK) { rc = group_gather(g, val, val_bytes, reinterpret_cast<char*>(result->d_values), val_at); }
  if(rc == GCSA2_OK) { rc = group_sync(g); }
  if(rc == GCSA2_OK)
  {
    DeviceGuard guard(root->device);
    u64 at = 0;
    for(size_t r = 0; r < G; r++)
    {
      if(counts[r] > 0 && base[r] > 0)
      {
        hipLaunchKernelGGL(k_rebase_offsets, dim3(grid_for(counts[r])), dim3(TPB), 0, g->streams[0], d_offsets_root + at, counts[r], base[r]);
      }
      at += counts[r];
    }
    hipError_t e = hipMemcpyAsync(d_offsets_root + q_before, &total, sizeof(u64), hipMemcpyHostToDevice, g->streams[0]);
    if(e == hipSuccess) { e = hipStreamSynchronize(g->streams[0]); }
    if(e != hipSuccess) { rc = fail(GCSA2_ERR_HIP, std::string("offsets of the gathered batch: ") + hipGetErrorString(e)); }
  }
  if(rc != GCSA2_OK) { gcsa2_locate_discard(result); return rc; }
  *job_out = result;
  if(d_values_root) { *d_values_root = result->d_values; }
  if(total_values) { *total_values = total; }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_group_locate_device: ") + e.what()); }
}

// ---- the same two queries with one process per GPU (gcsa2_comm): every rank works on its contiguous shard, the results are
// gathered on the root through gcsa2_comm_gather's grouped send / recv ----------------------------------------------------------

// counts[r] / pattern_bytes[r]: patterns and pattern bytes of rank r's shard (the same arrays on every rank).  Enqueue-only on
// `stream` (the scratch of the shard's results is stream-ordered); the root's arrays are complete when the stream is.
int gcsa2_comm_match_stats(gcsa2_comm* c, const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, const uint64_t* counts,
                           const uint64_t* pattern_bytes, int root, uint16_t* d_ms_root, uint64_t* d_ranges_root, uint64_t* d_fallbacks_root,
                           void* stream)
{
  CHECK_INDEX(ix);
  if(c == nullptr || counts == nullptr || pattern_bytes == nullptr || root < 0 || root >= c->world) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "bad arguments"); }
  if(c->rank == root && (d_ms_root == nullptr || d_ranges_root == nullptr || d_fallbacks_root == nullptr)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "the root needs all three result buffers"); }
  if(ix->device != c->device) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "index and communicator are on different devices"); }
  DeviceGuard guard(c->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const u64 nq = counts[c->rank], bytes = pattern_bytes[c->rank];
  const u64 ms_room = (2 * bytes + 8 * sizeof(uint16_t) + 15) / 16 * 16;
  char* buf = nullptr;
  HIP_TRY(pool_alloc(ix, reinterpret_cast<void**>(&buf), ms_room + 24 * nq + 16, st));
  uint16_t* my_ms = reinterpret_cast<uint16_t*>(buf); u64* my_rng = reinterpret_cast<u64*>(buf + ms_room); u64* my_fb = my_rng + 2 * nq;
  // A rank whose kernel launch fails still takes part in the three gathers (its buffers exist; the root receives whatever they
  // hold) and reports the error afterwards: leaving now would keep the other ranks waiting in ncclSend / ncclRecv for ever.
  // (The allocation above is the one failure that cannot be carried through: without a buffer there is nothing to send.)
  const int launch_rc = (nq > 0 ? match_stats_launch(ix, 0, d_patterns, d_offsets, nq, bytes, my_ms, my_rng, my_fb, st) : GCSA2_OK);
  const std::string launch_error = (launch_rc != GCSA2_OK ? g_error : std::string());
  std::vector<u64> sizes(size_t(c->world));
  int rc = GCSA2_OK;
  for(int part = 0; part < 3; part++)
  {
    for(int r = 0; r < c->world; r++) { sizes[size_t(r)] = (part == 0 ? 2 * pattern_bytes[r] : (part == 1 ? 16 * counts[r] : 8 * counts[r])); }
    const void* src = (part == 0 ? static_cast<const void*>(my_ms) : (part == 1 ? static_cast<const void*>(my_rng) : static_cast<const void*>(my_fb)));
    void* dst = (part == 0 ? static_cast<void*>(d_ms_root) : (part == 1 ? static_cast<void*>(d_ranges_root) : static_cast<void*>(d_fallbacks_root)));
    const int g_rc = gather_bytes(c, src, sizes.data(), dst, root, st);
    if(rc == GCSA2_OK) { rc = g_rc; }
  }
  (void)hipFreeAsync(buf, st);
  if(launch_rc != GCSA2_OK) { return fail(launch_rc, launch_error); }
  return rc;
}

// locate() of this rank's shard (counts[rank] ranges); on the root: d_offsets_root (sum of counts + 1 entries) and a job that owns
// the values of the whole batch in query order.  Per-rank totals travel first (8 bytes each), then the offsets and the values
// (SURVEY.md 8(e)).  Complete on return (the sizes of the second gather are read on the host).
int gcsa2_comm_locate(gcsa2_comm* c, const gcsa2_index* ix, const uint64_t* d_ranges, const uint64_t* counts, int sort, int root,
                      uint64_t* d_offsets_root, gcsa2_locate_job** job_root, const uint64_t** d_values_root, uint64_t* total_values, void* stream)
{
  CHECK_INDEX(ix);
  if(c == nullptr || counts == nullptr || root < 0 || root >= c->world) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "bad arguments"); }
  if(c->rank == root && (d_offsets_root == nullptr || job_root == nullptr)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "the root needs result buffers"); }
  if(ix->device != c->device) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "index and communicator are on different devices"); }
  if(job_root != nullptr) { *job_root = nullptr; }
  try {
  DeviceGuard guard(c->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t W = size_t(c->world);
  const bool is_root = (c->rank == root);
  // A rank whose own part fails must not leave the others waiting in ncclSend / ncclRecv: it still joins the first gather, with
  // FAILED as its total, and the later gathers with nothing to send; the root, which sees the mark, expects nothing from that
  // rank, lets the healthy ranks finish and reports the failure.  Every rank returns its own status.
  constexpr u64 FAILED = ~u64(0);
  gcsa2_locate_job* mine = nullptr;
  const int local_rc = gcsa2_locate_device(ix, d_ranges, counts[c->rank], sort, &mine, nullptr, nullptr, nullptr, st);
  const std::string local_error = (local_rc != GCSA2_OK ? g_error : std::string());
  struct Discard { gcsa2_locate_job*& j; ~Discard() { gcsa2_locate_discard(j); } } discard{mine};
  // 1. per-rank totals: the last entry of every rank's offsets (a slot of the handle: no allocation that could fail in between)
  std::vector<u64> eight(W, sizeof(u64)), totals(W, 0);
  const unsigned slot = ix->next_slot.fetch_add(1) % RESULT_SLOTS;
  u64* d_mark = reinterpret_cast<u64*>(ix->d_slots + u64(TOTAL_WORDS) * slot);
  u64* d_totals = nullptr;
  struct FreeAsync { u64*& p; hipStream_t st; ~FreeAsync() { if(p != nullptr) { (void)hipFreeAsync(p, st); } } } free_totals{d_totals, st};
  int rc = GCSA2_OK;
  if(is_root)
  {
    hipError_t e = pool_alloc(ix, reinterpret_cast<void**>(&d_totals), W * sizeof(u64), st);
    if(e != hipSuccess) { rc = fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("pool_alloc(totals): ") + hipGetErrorString(e)); }
  }
  if(rc != GCSA2_OK) { return rc; }               // (the root without 8 bytes per rank: nothing can be received at all)
  const u64* my_total = (mine != nullptr ? mine->d_offsets + counts[c->rank] : d_mark);
  if(mine == nullptr)
  {
    const u64 mark = FAILED;
    hipError_t e = hipMemcpyAsync(d_mark, &mark, sizeof(u64), hipMemcpyHostToDevice, st);
    if(e == hipSuccess) { e = hipStreamSynchronize(st); }
    if(e != hipSuccess) { return fail(local_rc, local_error); }    // the device itself is gone
  }
  rc = gather_bytes(c, my_total, eight.data(), d_totals, root, st);
  if(rc == GCSA2_OK && is_root)
  {
    hipError_t e = hipMemcpyAsync(totals.data(), d_totals, W * sizeof(u64), hipMemcpyDeviceToHost, st);
    if(e != hipSuccess) { rc = fail(GCSA2_ERR_HIP, std::string("totals of the shards: ") + hipGetErrorString(e)); }
  }
  if(rc == GCSA2_OK)
  {
    hipError_t e = hipStreamSynchronize(st);
    if(e != hipSuccess) { rc = fail(GCSA2_ERR_HIP, std::string("totals of the shards: ") + hipGetErrorString(e)); }
  }
  if(rc != GCSA2_OK) { return rc; }
  if(!is_root) { totals[size_t(c->rank)] = (mine != nullptr ? mine->total : FAILED); }
  // 2. offsets (counts[r] entries each) and values (totals[r] each); a peer only needs its own sizes
  std::vector<u64> off_bytes(W), val_bytes(W);
  u64 total = 0, queries = 0;
  int failed_rank = -1;
  for(size_t r = 0; r < W; r++)
  {
    const bool bad = (totals[r] == FAILED);
    if(bad) { totals[r] = 0; if(failed_rank < 0) { failed_rank = int(r); } }
    off_bytes[r] = (bad ? 0 : 8 * counts[r]); val_bytes[r] = 8 * totals[r]; total += totals[r]; queries += counts[r];
  }
  gcsa2_locate_job* result = nullptr;
  // a rank whose pass failed sends zero bytes -- from a device address that always exists (a custom transport may look at it)
  const u64* my_offsets = (mine != nullptr ? mine->d_offsets : d_mark);
  const u64* my_values = (mine != nullptr ? mine->d_values : d_mark);
  if(is_root)
  {
    result = new(std::nothrow) gcsa2_locate_job();
    hipError_t e = hipSuccess;
    if(result != nullptr)
    {
      result->device = c->device; result->nq = queries; result->total = total;
      e = hipMalloc(reinterpret_cast<void**>(&result->d_values), (total > 0 ? total : 1) * sizeof(u64));
    }
    if(result == nullptr || e != hipSuccess)
    {
      // the peers are about to send: without a buffer the communicator cannot complete this call on any rank
      delete result;
      return fail(GCSA2_ERR_OUT_OF_MEMORY, "no memory for the values of the batch on the root (the other ranks of this call will not return: destroy the communicator)");
    }
  }
  rc = gather_bytes(c, my_offsets, off_bytes.data(), d_offsets_root, root, st);
  {
    const int g_rc = gather_bytes(c, my_values, val_bytes.data(), is_root ? result->d_values : nullptr, root, st);
    if(rc == GCSA2_OK) { rc = g_rc; }
  }
  if(rc == GCSA2_OK && local_rc != GCSA2_OK) { rc = fail(local_rc, local_error); }
  if(rc == GCSA2_OK && failed_rank >= 0) { rc = fail(GCSA2_ERR_HIP, "locate failed on rank " + std::to_string(failed_rank) + " of the communicator; the batch is incomplete"); }
  if(rc == GCSA2_OK && is_root)
  {
    u64 at = 0, base = 0;
    for(size_t r = 0; r < W; r++)
    {
      if(counts[r] > 0 && base > 0) { hipLaunchKernelGGL(k_rebase_offsets, dim3(grid_for(counts[r])), dim3(TPB), 0, st, d_offsets_root + at, counts[r], base); }
      at += counts[r]; base += totals[r];
    }
    hipError_t e = hipMemcpyAsync(d_offsets_root + queries, &total, sizeof(u64), hipMemcpyHostToDevice, st);
    if(e != hipSuccess) { rc = fail(GCSA2_ERR_HIP, std::string("offsets of the gathered batch: ") + hipGetErrorString(e)); }
  }
  hipError_t se = hipStreamSynchronize(st);
  if(rc == GCSA2_OK && se != hipSuccess) { rc = fail(GCSA2_ERR_HIP, std::string("gather: ") + hipGetErrorString(se)); }
  if(rc != GCSA2_OK) { gcsa2_locate_discard(result); return rc; }
  if(is_root)
  {
    *job_root = result;
    if(d_values_root) { *d_values_root = result->d_values; }
    if(total_values) { *total_values = total; }
  }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_comm_locate: ") + e.what()); }
}

int gcsa2_group_size(const gcsa2_group* g) { return g == nullptr ? 0 : int(g->replicas.size()); }

const gcsa2_index* gcsa2_group_index(const gcsa2_group* g, int i)
{
  return (g == nullptr || i < 0 || i >= int(g->replicas.size())) ? nullptr : g->replicas[size_t(i)];
}

int gcsa2_group_find_batch(const gcsa2_group* g, const uint8_t* patterns, const uint64_t* offsets, uint64_t nq, uint64_t* ranges)
{
  if(g == nullptr || g->replicas.empty()) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null or empty group"); }
  if(nq == 0) { return GCSA2_OK; }
  if(offsets == nullptr || ranges == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  if(!offsets_ok(offsets, nq)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "pattern offsets are not non-decreasing"); }
  try {   // no C++ exception may cross the C boundary
  const u64 G = g->replicas.size(), base = nq / G, rem = nq % G;
  std::vector<int> status(G, GCSA2_OK);
  std::vector<std::string> messages(G);
  Workers workers;
  u64 begin = 0;
  for(u64 r = 0; r < G; r++)
  {
    u64 count = base + (r < rem ? 1 : 0), b = begin;
    begin += count;
    if(count == 0) { continue; }
    workers.emplace_back([&, r, b, count]()
    {
      try
      {
        std::vector<u64> local;
        status[r] = gcsa2_find_batch(g->replicas[r], patterns + offsets[b], rebase_piece(offsets, b, count, local), count, ranges + 2 * b);
        if(status[r] != GCSA2_OK) { messages[r] = g_error; }     // g_error is thread-local
      }
      catch(const std::exception& e) { status[r] = GCSA2_ERR_OUT_OF_MEMORY; messages[r] = e.what(); }
    });
  }
  workers.join();
  for(u64 r = 0; r < G; r++) { if(status[r] != GCSA2_OK) { return fail(status[r], "shard " + std::to_string(r) + ": " + messages[r]); } }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_group_find_batch: ") + e.what()); }
}

}  // extern "C"

// Matching statistics (LF + parent fused); see k_match_stats2.  variant 2 = one lane per pattern, 5 = persistent lanes that draw
// patterns from a counter, 0 = the library chooses by batch size.  total_bytes = offsets[nq] when the caller knows it (GCSA2_UNKNOWN: read back from the
// device, which waits for the stream once).
namespace {
int match_stats_launch(const gcsa2_index* ix, int variant, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t nq, u64 total_bytes,
                       uint16_t* d_ms, uint64_t* d_ranges, uint64_t* d_fallbacks, hipStream_t st, const BreakSink* sink)
{
  CHECK_INDEX(ix);
  DeviceGuard guard(ix->device);
  if(!ix->img.has_lcp) { return fail(GCSA2_ERR_MISSING_COMPONENT, "index was created without an LCP array"); }
  if(variant != 0 && variant != 2 && variant != 5)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "unknown matching statistics variant (0: the library chooses; 2 / 5: a lane per pattern / persistent lanes)");
  }
  if(nq == 0 || ix->img.n == 0) { return GCSA2_OK; }
  if(total_bytes == GCSA2_UNKNOWN)
  {
    HIP_TRY(hipMemcpyAsync(&total_bytes, d_offsets + nq, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  // pre-pass: the patterns as 16-byte records, last character first (k_pack_records); stream-ordered scratch
  ulonglong2* recs = nullptr;
  HIP_TRY(pool_alloc(ix, reinterpret_cast<void**>(&recs), ((total_bytes >> 5) + nq + 6) * sizeof(ulonglong2), st));
  hipLaunchKernelGGL(k_pack_records, dim3(grid_for(nq)), dim3(TPB), 0, st, ix->img, d_patterns, d_offsets, nq, recs);
  const u32 cool = ix->tune.cool_down;
  unsigned short* out = reinterpret_cast<unsigned short*>(d_ms);
  const u64 lanes_grid = (nq + TPB2 - 1) / TPB2;
  const bool pair = ix->img.flp != nullptr;
  unsigned long long* queue = nullptr;
  const u64 resident = ix->tune.ms_grid != 0 ? ix->tune.ms_grid : u64(ix->compute_units) * 8;     // workgroups the device holds at 4 waves per SIMD
  // variant 0 chooses: a batch of more than two generations of workgroups goes to the persistent lanes -- patterns that need
  // parent() take three times the rounds of those that do not, and a wave whose lanes own fixed patterns waits for its slowest
  // (1 M x 256 bp, half with mismatches: 114 -> 128 M patterns/s; without mismatches 242 -> 236; profiles/r03_match_stats.md)
  if(variant == 0) { variant = (lanes_grid > 2 * resident ? 5 : 2); }
  if(variant == 5)
  {
    hipError_t qe = pool_alloc(ix, reinterpret_cast<void**>(&queue), sizeof(unsigned long long), st);
    if(qe == hipSuccess) { qe = hipMemsetAsync(queue, 0, sizeof(unsigned long long), st); }
    if(qe != hipSuccess) { (void)hipFreeAsync(recs, st); return fail(GCSA2_ERR_HIP, std::string("matching statistics queue: ") + hipGetErrorString(qe)); }
    const unsigned grid = unsigned(lanes_grid < resident ? lanes_grid : resident);
    unsigned long long* none = nullptr;
    if(sink != nullptr && sink->max_length != 0 && pair)
    {
      hipLaunchKernelGGL((k_match_stats2<true, true, false, true, true>), dim3(grid), dim3(TPB2), 0, st,
                         ix->img, d_patterns, d_offsets, nq, out, d_ranges, d_fallbacks, cool, queue, ix->tune.ms_refill_at, recs, none, *sink);
    }
    else if(sink != nullptr && sink->max_length != 0)
    {
      hipLaunchKernelGGL((k_match_stats2<false, true, false, true, true>), dim3(grid), dim3(TPB2), 0, st,
                         ix->img, d_patterns, d_offsets, nq, out, d_ranges, d_fallbacks, cool, queue, ix->tune.ms_refill_at, recs, none, *sink);
    }
    else if(sink != nullptr && pair)
    {
      hipLaunchKernelGGL((k_match_stats2<true, true, false, true>), dim3(grid), dim3(TPB2), 0, st,
                         ix->img, d_patterns, d_offsets, nq, out, d_ranges, d_fallbacks, cool, queue, ix->tune.ms_refill_at, recs, none, *sink);
    }
    else if(sink != nullptr)
    {
      hipLaunchKernelGGL((k_match_stats2<false, true, false, true>), dim3(grid), dim3(TPB2), 0, st,
                         ix->img, d_patterns, d_offsets, nq, out, d_ranges, d_fallbacks, cool, queue, ix->tune.ms_refill_at, recs, none, *sink);
    }
    else if(pair)
    {
      hipLaunchKernelGGL((k_match_stats2<true, true>), dim3(grid), dim3(TPB2), 0, st,
                         ix->img, d_patterns, d_offsets, nq, out, d_ranges, d_fallbacks, cool, queue, ix->tune.ms_refill_at, recs);
    }
    else
    {
      hipLaunchKernelGGL((k_match_stats2<false, true>), dim3(grid), dim3(TPB2), 0, st,
                         ix->img, d_patterns, d_offsets, nq, out, d_ranges, d_fallbacks, cool, queue, ix->tune.ms_refill_at, recs);
    }
  }
  else if(sink != nullptr)
  {
    unsigned long long* none = nullptr;
    if(sink->max_length != 0 && pair)
    {
      hipLaunchKernelGGL((k_match_stats2<true, false, false, true, true>), dim3(unsigned(lanes_grid)), dim3(TPB2), 0, st,
                         ix->img, d_patterns, d_offsets, nq, out, d_ranges, d_fallbacks, cool, none, 64u, recs, none, *sink);
    }
    else if(sink->max_length != 0)
    {
      hipLaunchKernelGGL((k_match_stats2<false, false, false, true, true>), dim3(unsigned(lanes_grid)), dim3(TPB2), 0, st,
                         ix->img, d_patterns, d_offsets, nq, out, d_ranges, d_fallbacks, cool, none, 64u, recs, none, *sink);
    }
    else if(pair)
    {
      hipLaunchKernelGGL((k_match_stats2<true, false, false, true>), dim3(unsigned(lanes_grid)), dim3(TPB2), 0, st,
                         ix->img, d_patterns, d_offsets, nq, out, d_ranges, d_fallbacks, cool, none, 64u, recs, none, *sink);
    }
    else
    {
      hipLaunchKernelGGL((k_match_stats2<false, false, false, true>), dim3(unsigned(lanes_grid)), dim3(TPB2), 0, st,
                         ix->img, d_patterns, d_offsets, nq, out, d_ranges, d_fallbacks, cool, none, 64u, recs, none, *sink);
    }
  }
  else if(pair)
  {
    hipLaunchKernelGGL((k_match_stats2<true, false>), dim3(unsigned(lanes_grid)), dim3(TPB2), 0, st,
                       ix->img, d_patterns, d_offsets, nq, out, d_ranges, d_fallbacks, cool, (unsigned long long*)nullptr, 64u, recs);
  }
  else
  {
    hipLaunchKernelGGL((k_match_stats2<false, false>), dim3(unsigned(lanes_grid)), dim3(TPB2), 0, st,
                       ix->img, d_patterns, d_offsets, nq, out, d_ranges, d_fallbacks, cool, (unsigned long long*)nullptr, 64u, recs);
  }
  hipError_t le = hipGetLastError();
  if(queue != nullptr) { (void)hipFreeAsync(queue, st); }
  (void)hipFreeAsync(recs, st);                                        // stream-ordered: released after the kernel
  if(le != hipSuccess) { return fail(GCSA2_ERR_HIP, std::string("k_match_stats2: ") + hipGetErrorString(le)); }
  return GCSA2_OK;
}
}  // namespace

extern "C" int gcsa2_match_stats_device_variant(const gcsa2_index* ix, int variant, const uint8_t* d_patterns, const uint64_t* d_offsets,
                                                uint64_t nq, uint16_t* d_ms, uint64_t* d_ranges, uint64_t* d_fallbacks, void* stream)
{
  return match_stats_launch(ix, variant, d_patterns, d_offsets, nq, GCSA2_UNKNOWN, d_ms, d_ranges, d_fallbacks, static_cast<hipStream_t>(stream));
}

extern "C" int gcsa2_match_stats_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t nq,
                                        uint16_t* d_ms, uint64_t* d_ranges, uint64_t* d_fallbacks, void* stream)
{
  return match_stats_launch(ix, 0, d_patterns, d_offsets, nq, GCSA2_UNKNOWN, d_ms, d_ranges, d_fallbacks, static_cast<hipStream_t>(stream));
}

// Matching statistics as BREAK POINTS (k_match_stats2<.., BREAKS>): the CSR of the left-maximal matches of every pattern.
// Complete on return: the number of records is read back, and a buffer that is too small is refused with the number needed.
// max_length > 0: no match grows beyond that many characters (k_match_stats2<.., CAP>); 0, or a value no pattern reaches: no cap.
namespace {
inline u64 effective_cap(u64 max_length) { return max_length >= (u64(1) << 32) ? 0 : max_length; }   // (a pattern is shorter than 2^32 characters)
#define CHECK_CAP(min_length, max_length) \
  do { if(effective_cap(max_length) != 0 && (min_length) > (max_length)) \
       { return fail(GCSA2_ERR_INVALID_ARGUMENT, "min_length exceeds max_length: no match could be reported"); } } while(0)
}  // namespace

int gcsa2_match_breaks_bounded_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t nq, uint64_t total_bytes,
                                      int variant, uint64_t min_length, uint64_t max_length, uint64_t* d_break_offsets, gcsa2_break* d_breaks,
                                      uint64_t capacity, uint64_t* total_breaks, uint64_t* d_ranges, uint64_t* d_fallbacks, void* stream)
{
  CHECK_INDEX(ix);
  CHECK_CAP(min_length, max_length);
  if(d_break_offsets == nullptr || total_breaks == nullptr || (d_breaks == nullptr && capacity > 0)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  if(nq >= (u64(1) << 31) - 1) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "batch of >= 2^31 patterns; split the batch"); }
  DeviceGuard guard(ix->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  *total_breaks = 0;
  if(nq == 0 || ix->img.n == 0)
  {
    HIP_TRY(hipMemsetAsync(d_break_offsets, 0, (nq + 1) * sizeof(u64), st));
    HIP_TRY(hipStreamSynchronize(st));
    return GCSA2_OK;
  }
  const auto t_start = std::chrono::steady_clock::now();
  auto since = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count(); };
  Scratch scratch(ix, st);
  // slots of the temporary records: what the caller's buffer holds + one block per wavefront that may leave a hole
  // (the wavefronts that can leave one: with a lane per pattern every wave of the grid, on the persistent lanes -- what
  // match_stats_launch picks for a batch of more than two generations of workgroups -- only the resident ones; and never more
  // records than one per pattern position and one per pattern, whatever the caller's capacity is: ADVICE r04)
  const u64 lane_waves = (nq + 63) / 64, lanes_grid = (nq + TPB2 - 1) / TPB2;
  const u64 resident = ix->tune.ms_grid != 0 ? ix->tune.ms_grid : u64(ix->compute_units) * 8;
  const bool persistent = (variant == 5 || (variant == 0 && lanes_grid > 2 * resident));
  const u64 waves = (persistent && resident * (TPB2 / 64) < lane_waves ? resident * (TPB2 / 64) : lane_waves);
  const u64 most = (total_bytes != GCSA2_UNKNOWN && total_bytes + nq < capacity ? total_bytes + nq : capacity);
  const u64 tmp_slots = most + (waves + 1) * BREAK_BLOCK;
  BreakSink sink{nullptr, tmp_slots, nullptr, nullptr, u32(min_length > 0xFFFFFFFFull ? 0xFFFFFFFFull : min_length), u32(effective_cap(max_length))};
  u64 *wide = nullptr, *own_ranges = nullptr;
  const unsigned slot = ix->next_slot.fetch_add(1) % RESULT_SLOTS;
  unsigned long long* d_totals = ix->d_slots + u64(TOTAL_WORDS) * slot;
  sink.counter = d_totals;
  HIP_TRY(scratch.get(sink.tmp, tmp_slots * BREAK_WORDS));
  HIP_TRY(scratch.get(sink.counts, nq));
  HIP_TRY(scratch.get(wide, nq + 1));
  if(d_ranges == nullptr) { HIP_TRY(scratch.get(own_ranges, 2 * nq)); d_ranges = own_ranges; }
  HIP_TRY(hipMemsetAsync(d_totals, 0, TOTAL_WORDS * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(sink.counts, 0, nq * sizeof(u32), st));
  const double t_alloc = since();
  int rc = match_stats_launch(ix, variant, d_patterns, d_offsets, nq, total_bytes, nullptr, d_ranges, d_fallbacks, st, &sink);
  if(rc != GCSA2_OK) { return rc; }
  const double t_launched = since();
  hipLaunchKernelGGL(k_widen_counts, dim3(grid_for(nq + 1)), dim3(TPB), 0, st, sink.counts, nq, wide);
  size_t scan_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, wide, d_break_offsets, size_t(nq + 1), st));
  char* scan_tmp = nullptr;
  HIP_TRY(scratch.get(scan_tmp, scan_bytes));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, wide, d_break_offsets, size_t(nq + 1), st));
  hipLaunchKernelGGL(k_copy_word, dim3(1), dim3(1), 0, st, d_break_offsets + nq, reinterpret_cast<u64*>(d_totals + 1));
  unsigned long long totals[TOTAL_WORDS];
  rc = read_totals(ix, slot, totals, st);
  if(rc != GCSA2_OK) { return rc; }
  scratch.settled = true;
  const double t_totals = since();
  const u64 reserved = totals[0], found = totals[1];          // slots the wavefronts reserved (with holes), records in all
  *total_breaks = found;
  if(found > capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "break buffer too small"); }
  //  the record scratch is sized from the caller's `total_bytes`: if that figure was too small the wavefronts
  // reserved slots beyond the scratch and dropped those records -- refused, not returned as a CSR with holes
  if(reserved > tmp_slots)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "match_breaks: total_bytes is smaller than the patterns' total length (more break records than the scratch sized from it holds)");
  }
  if(found > 0)
  {
    scratch.settled = false;
    const u64 stored = reserved;
    hipLaunchKernelGGL(k_breaks_scatter, dim3(grid_for(stored)), dim3(TPB), 0, st, sink.tmp, stored, d_break_offsets, reinterpret_cast<u64*>(d_breaks), capacity);
    LAUNCH_CHECK("k_breaks_scatter");
  }
  HIP_TRY(hipStreamSynchronize(st));
  scratch.settled = true;
  if(ix->tune.locate_trace)
  {
    std::fprintf(stderr, "[breaks] scratch %.0f us | launched %.0f | totals %.0f | done %.0f (arena %zu of %zu bytes, %zu extra allocations)\n",
                 t_alloc, t_launched, t_totals, since(), scratch.used, scratch.arena.bytes, scratch.extra.size());
  }
  return GCSA2_OK;
}

int gcsa2_match_breaks_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t nq, uint64_t total_bytes,
                              int variant, uint64_t min_length, uint64_t* d_break_offsets, gcsa2_break* d_breaks, uint64_t capacity, uint64_t* total_breaks,
                              uint64_t* d_ranges, uint64_t* d_fallbacks, void* stream)
{
  return gcsa2_match_breaks_bounded_device(ix, d_patterns, d_offsets, nq, total_bytes, variant, min_length, 0, d_break_offsets, d_breaks, capacity,
                                           total_breaks, d_ranges, d_fallbacks, stream);
}

namespace {

// The break points of a large host batch, in pieces like the dense statistics of match_stats_pieced (a MEM finder's reads live in host memory:
// one copy in, one kernel, copies out leaves the device idle two thirds of the time).  A piece's records land in the caller's
// array behind those of the pieces before it, so the pieces COMMIT in order: when its kernel has finished a piece knows its
// number of records, waits for the running total of the pieces before it (they started earlier; the wait is the tail of one
// kernel at most), takes its place and downloads there.  The device-side record buffer of a piece is sized by an estimate
// (one record per 8 pattern bytes; a piece that needs more runs again with the exact size).  Once the caller's capacity is
// exceeded the remaining pieces only count: GCSA2_ERR_BUFFER_TOO_SMALL with the number of records of the whole batch.
int match_breaks_pieced(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t nq, uint64_t min_length, uint64_t max_length,
                        uint64_t* break_offsets, gcsa2_break* breaks, uint64_t capacity, uint64_t* total_breaks, uint64_t* ranges, uint64_t* fallbacks)
{
  const std::vector<u64> cut = cut_pieces(offsets, nq, ix->tune.ms_piece_bytes);
  const u64 pieces = cut.size() - 1;
  const unsigned threads = unsigned(pieces < ix->tune.ms_threads ? pieces : ix->tune.ms_threads);
  struct Order { std::mutex m; std::condition_variable cv; u64 next = 0, base = 0; bool failed = false; } order;
  auto work = [&](unsigned t, Outcome& out)
  {
    DeviceGuard guard(ix->device);
    std::vector<u64> local;
    auto give_up = [&](int rc, const std::string& what)
    {
      out.set(rc, what);
      std::lock_guard<std::mutex> hold(order.m);
      order.failed = true;
      order.cv.notify_all();
    };
    try {
    for(u64 c = t; c < pieces && out.status == GCSA2_OK; c += threads)
    {
      const u64 b = cut[c], count = cut[c + 1] - b, first = offsets[b], bytes = offsets[b + count] - first;
      rebase_piece(offsets, b, count, local);
      u64 room = bytes / 8 + count + 1, found = 0;
      bool placed = false;
      for(int attempt = 0; attempt < 2 && !placed && out.status == GCSA2_OK; attempt++)
      {
        Lease lease(ix);
        hipError_t e = lease.begin(Lease::need(bytes + 16) + 2 * Lease::need((count + 1) * 8) + Lease::need(room * 32) + Lease::need(2 * count * 8) + Lease::need(count * 8));
        if(e != hipSuccess) { give_up(GCSA2_ERR_OUT_OF_MEMORY, std::string("staging of a piece: ") + hipGetErrorString(e)); break; }
        u8* d_pat = lease.dev<u8>(bytes + 16); u64* d_off = lease.dev<u64>(count + 1); u64* d_boff = lease.dev<u64>(count + 1);
        gcsa2_break* d_brk = reinterpret_cast<gcsa2_break*>(lease.dev<u64>(4 * room));
        u64* d_rng = lease.dev<u64>(2 * count); u64* d_fb = lease.dev<u64>(count);
        e = lease.up(d_pat, patterns + first, bytes);
        if(e == hipSuccess) { e = lease.up(d_off, local.data(), (count + 1) * sizeof(u64)); }
        if(e != hipSuccess) { give_up(GCSA2_ERR_HIP, std::string("upload of a piece: ") + hipGetErrorString(e)); break; }
        const int rc = gcsa2_match_breaks_bounded_device(ix, d_pat, d_off, count, bytes, 0, min_length, max_length, d_boff, d_brk, room, &found, d_rng, d_fb, lease.stream());
        if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && attempt == 0 && found > room) { room = found; (void)lease.finish(); continue; }    // the estimate was short: once more, exactly
        if(rc != GCSA2_OK) { give_up(rc, g_error); break; }
        // commit in piece order: the position of this piece's first record
        u64 at = 0;
        {
          std::unique_lock<std::mutex> hold(order.m);
          order.cv.wait(hold, [&]() { return order.next == c || order.failed; });
          if(order.failed) { out.set(GCSA2_ERR_HIP, "another piece of the batch failed"); out.echo = true; break; }      // (reported only if no piece says why)
          at = order.base; order.base += found; order.next = c + 1;
          order.cv.notify_all();
        }
        placed = true;
        if(at + found <= capacity)
        {
          e = lease.down(local.data(), d_boff, (count + 1) * sizeof(u64));
          if(e == hipSuccess && found > 0) { e = lease.down(breaks + at, d_brk, found * sizeof(gcsa2_break)); }
          if(e == hipSuccess && ranges != nullptr) { e = lease.down(ranges + 2 * b, d_rng, 2 * count * sizeof(u64)); }
          if(e == hipSuccess && fallbacks != nullptr) { e = lease.down(fallbacks + b, d_fb, count * sizeof(u64)); }
          if(e == hipSuccess) { e = lease.finish(); }
          if(e != hipSuccess) { give_up(GCSA2_ERR_HIP, std::string("download of a piece: ") + hipGetErrorString(e)); break; }
          for(u64 i = 0; i <= count; i++) { break_offsets[b + i] = local[i] + at; }     // (the last entry is the next piece's first: same value)
        }
        else { (void)lease.finish(); }
      }
    }
    } catch(const std::exception& e) { give_up(GCSA2_ERR_OUT_OF_MEMORY, std::string("a piece of the batch: ") + e.what()); }     // (here, not in fan_out: the other pieces must not wait for this one)
  };
  const int rc = fan_out(threads, nullptr, work);
  if(rc != GCSA2_OK) { return rc; }
  *total_breaks = order.base;
  if(order.base > capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "break buffer too small"); }
  return GCSA2_OK;
}

}  // namespace

// The break points of a batch in host memory: one copy in, gcsa2_match_breaks_bounded_device, the CSR out.
int gcsa2_match_breaks_bounded_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t nq, uint64_t min_length,
                                     uint64_t max_length, uint64_t* break_offsets, gcsa2_break* breaks, uint64_t capacity, uint64_t* total_breaks,
                                     uint64_t* ranges, uint64_t* fallbacks)
{
  CHECK_INDEX(ix);
  CHECK_CAP(min_length, max_length);
  if(nq == 0)             // an empty batch: no records, whatever the (possibly null) input arrays are
  {
    if(total_breaks != nullptr) { *total_breaks = 0; }
    if(break_offsets != nullptr) { break_offsets[0] = 0; }
    return GCSA2_OK;
  }
  if(offsets == nullptr || break_offsets == nullptr || total_breaks == nullptr || (breaks == nullptr && capacity > 0) || (patterns == nullptr && offsets[nq] > offsets[0]))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  *total_breaks = 0;
  u64 longest = 0;
  if(offsets[0] != 0 || !offsets_ok(offsets, nq, &longest)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "pattern offsets must start at 0 and be non-decreasing"); }
  try
  {
    if(ix->tune.ms_pieces && offsets[nq] >= 2 * ix->tune.ms_piece_bytes && longest <= ix->tune.ms_piece_bytes)
    {
      return match_breaks_pieced(ix, patterns, offsets, nq, min_length, max_length, break_offsets, breaks, capacity, total_breaks, ranges, fallbacks);
    }
    DeviceGuard guard(ix->device);
    const u64 total = offsets[nq];
    Lease lease(ix);
    HIP_TRY(lease.begin(Lease::need(total + 16) + Lease::need((nq + 1) * 8) + Lease::need((nq + 1) * 8) + Lease::need((capacity > 0 ? capacity : 1) * 32)
                        + Lease::need(2 * nq * 8) + Lease::need(nq * 8)));
    u8* d_pat = lease.dev<u8>(total + 16); u64* d_off = lease.dev<u64>(nq + 1); u64* d_boff = lease.dev<u64>(nq + 1);
    gcsa2_break* d_brk = reinterpret_cast<gcsa2_break*>(lease.dev<u64>(4 * (capacity > 0 ? capacity : 1)));
    u64* d_rng = lease.dev<u64>(2 * nq); u64* d_fb = lease.dev<u64>(nq);
    HIP_TRY(lease.up(d_pat, patterns, total));
    HIP_TRY(lease.up(d_off, offsets, (nq + 1) * sizeof(u64)));
    int rc = gcsa2_match_breaks_bounded_device(ix, d_pat, d_off, nq, total, 0, min_length, max_length, d_boff, d_brk, capacity, total_breaks, d_rng, d_fb, lease.stream());
    if(rc != GCSA2_OK) { return rc; }
    HIP_TRY(lease.down(break_offsets, d_boff, (nq + 1) * sizeof(u64)));
    if(*total_breaks > 0) { HIP_TRY(lease.down(breaks, d_brk, *total_breaks * sizeof(gcsa2_break))); }
    if(ranges != nullptr) { HIP_TRY(lease.down(ranges, d_rng, 2 * nq * sizeof(u64))); }
    if(fallbacks != nullptr) { HIP_TRY(lease.down(fallbacks, d_fb, nq * sizeof(u64))); }
    HIP_TRY(lease.finish());
    return GCSA2_OK;
  }
  catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_match_breaks_batch: ") + e.what()); }
}

int gcsa2_match_breaks_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t nq, uint64_t min_length,
                             uint64_t* break_offsets, gcsa2_break* breaks, uint64_t capacity, uint64_t* total_breaks,
                             uint64_t* ranges, uint64_t* fallbacks)
{
  return gcsa2_match_breaks_bounded_batch(ix, patterns, offsets, nq, min_length, 0, break_offsets, breaks, capacity, total_breaks, ranges, fallbacks);
}

// Diagnostic: the default kernel instrumented with shader-clock counters per phase of its round (k_match_stats2<.., PROF>),
// same results; d_prof[0..15] (zeroed by the caller) receives the cycle sums and event counts listed at the kernel.
extern "C" int gcsa2_match_stats_profile_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t nq,
                                                uint64_t total_bytes, uint16_t* d_ms, uint64_t* d_ranges, uint64_t* d_fallbacks,
                                                uint64_t* d_prof, void* stream)
{
  CHECK_INDEX(ix);
  DeviceGuard guard(ix->device);
  if(!ix->img.has_lcp || ix->img.flp == nullptr) { return fail(GCSA2_ERR_MISSING_COMPONENT, "the profiled kernel needs the LCP array and the pair blocks"); }
  if(d_prof == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null profile buffer"); }
  if(nq == 0 || ix->img.n == 0) { return GCSA2_OK; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  ulonglong2* recs = nullptr;
  HIP_TRY(pool_alloc(ix, reinterpret_cast<void**>(&recs), ((total_bytes >> 5) + nq + 6) * sizeof(ulonglong2), st));
  hipLaunchKernelGGL(k_pack_records, dim3(grid_for(nq)), dim3(TPB), 0, st, ix->img, d_patterns, d_offsets, nq, recs);
  hipLaunchKernelGGL((k_match_stats2<true, false, true>), dim3(unsigned((nq + TPB2 - 1) / TPB2)), dim3(TPB2), 0, st,
                     ix->img, d_patterns, d_offsets, nq, reinterpret_cast<unsigned short*>(d_ms), d_ranges, d_fallbacks, ix->tune.cool_down,
                     (unsigned long long*)nullptr, 64u, recs, reinterpret_cast<unsigned long long*>(d_prof));
  hipError_t le = hipGetLastError();
  (void)hipFreeAsync(recs, st);
  if(le != hipSuccess) { return fail(GCSA2_ERR_HIP, std::string("k_match_stats2<prof>: ") + hipGetErrorString(le)); }
  return GCSA2_OK;
}

extern "C" int gcsa2_match_stats_device_sized(const gcsa2_index* ix, int variant, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t nq,
                                              uint64_t total_pattern_bytes, uint16_t* d_ms, uint64_t* d_ranges, uint64_t* d_fallbacks, void* stream)
{
  return match_stats_launch(ix, variant, d_patterns, d_offsets, nq, total_pattern_bytes, d_ms, d_ranges, d_fallbacks, static_cast<hipStream_t>(stream));
}

namespace {

// one copy in, one launch, copies out (offsets[0] = 0)
int match_stats_single(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t nq, u64 longest,
                       uint16_t* ms, uint64_t* ranges, uint64_t* fallbacks)
{
  DeviceGuard guard(ix->device);
  const u64 total = offsets[nq];
  Lease lease(ix);
  HIP_TRY(lease.begin(Lease::need(total + 16) + Lease::need((nq + 1) * 8) + Lease::need(2 * nq * 8) + Lease::need(nq * 8) + Lease::need((total + 8) * 2)));
  u8* d_pat = lease.dev<u8>(total + 16); u64* d_off = lease.dev<u64>(nq + 1); u64* d_rng = lease.dev<u64>(2 * nq);
  u64* d_fb = lease.dev<u64>(nq); uint16_t* d_ms = lease.dev<uint16_t>(total + 8);
  HIP_TRY(lease.up(d_pat, patterns, total));
  HIP_TRY(lease.up(d_off, offsets, (nq + 1) * sizeof(u64)));
  // ragged batches (longest pattern > 1.25 x the mean) large enough to fill the device go to the persistent lanes
  const bool ragged = nq >= MS_REFILL_MIN && double(longest) * double(nq) > 1.25 * double(total);
  int rc = match_stats_launch(ix, ragged ? 5 : 0, d_pat, d_off, nq, total, d_ms, d_rng, d_fb, lease.stream());
  if(rc != GCSA2_OK) { return rc; }
  HIP_TRY(lease.down(ms, d_ms, total * sizeof(uint16_t)));
  HIP_TRY(lease.down(ranges, d_rng, 2 * nq * sizeof(u64)));
  if(fallbacks != nullptr) { HIP_TRY(lease.down(fallbacks, d_fb, nq * sizeof(u64))); }
  HIP_TRY(lease.finish());
  return GCSA2_OK;
}

// A large host batch moves three times the pattern bytes over the link (one byte in, two out per position) and the kernel
// is faster than that: it is cut into pieces of tune.ms_piece_bytes pattern bytes which MS_PIECE_THREADS host threads send through
// the single-copy path, each on the stream and arenas of its own lease -- one piece's upload, another's kernel and a third's
// download overlap.  (1 M x 256 bp on the chr22-like index: 22.4 ms = 45 M patterns/s in a row, 17.5 ms = 57 M/s in pieces;
// eight threads or 8 MB pieces change nothing: what is left is the rate of copies to and from pageable memory,
// tests/perf/ms_host_batch.py.  Staging those copies ourselves through a ring of pinned 2 MB pieces was measured and is
// twice as slow as the runtime's own path for pageable memory: 47 ms in a row, 24-28 ms in pieces.)
// (pieces of tune.ms_piece_bytes = 32 MB (GCSA2_MS_PIECE_MB) for batches of two pieces' worth (64 MB) and more, on tune.ms_threads = 4 host threads: fields of
// gcsa2_index::Tuning.  Round 4 re-measured the piece size, 1 M x 256 bp: dense statistics on the chr22-like index 15.9-17.4 ms
// with 16 MB, 15.0 with 32, 16.1 with 64, 18.9 with 128, 22.3 in one copy; break points of at least 20 bp on the 5.73 G-node index 24.5 /
// 16.7 / 16.9 / 19.5 ms and 17.9 in one copy -- a piece must still fill the device: the kernel's time per pattern is latency, not work;
// profiles/r04_host.md)

int match_stats_pieced(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t nq, u64 longest,
                       uint16_t* ms, uint64_t* ranges, uint64_t* fallbacks)
{
  const std::vector<u64> cut = cut_pieces(offsets, nq, ix->tune.ms_piece_bytes);
  const u64 pieces = cut.size() - 1;
  const unsigned threads = unsigned(pieces < ix->tune.ms_threads ? pieces : ix->tune.ms_threads);
  return fan_out(threads, nullptr, [&](unsigned t, Outcome& out)
  {
    std::vector<u64> local;
    for(u64 c = t; c < pieces && out.status == GCSA2_OK; c += threads)
    {
      const u64 b = cut[c], count = cut[c + 1] - b, base = offsets[b];
      const int rc = match_stats_single(ix, patterns + base, rebase_piece(offsets, b, count, local), count, longest, ms + base, ranges + 2 * b,
                                        fallbacks != nullptr ? fallbacks + b : nullptr);
      if(rc != GCSA2_OK) { out.set(rc, g_error); }
    }
  });
}

}  // namespace

extern "C" int gcsa2_match_stats_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t nq,
                                       uint16_t* ms, uint64_t* ranges, uint64_t* fallbacks)
{
  CHECK_INDEX(ix);
  if(nq == 0) { return GCSA2_OK; }
  if(offsets == nullptr || ms == nullptr || ranges == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  u64 longest = 0;
  if(!offsets_ok(offsets, nq, &longest)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "pattern offsets are not non-decreasing"); }
  try
  {
    if(ix->tune.ms_pieces && offsets[0] == 0 && offsets[nq] >= 2 * ix->tune.ms_piece_bytes && longest <= ix->tune.ms_piece_bytes)
    {
      return match_stats_pieced(ix, patterns, offsets, nq, longest, ms, ranges, fallbacks);
    }
  }
  catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_match_stats_batch: ") + e.what()); }
  return match_stats_single(ix, patterns, offsets, nq, longest, ms, ranges, fallbacks);
}

// ---- host-view container file ("G2HV"): the interchange format between a process that can read
// .gcsa / .lcp files (the reference + SDSL) and GPU nodes that cannot. --------
// Layout (little endian): char magic[4] = "G2HV"; u32 version = 1; u64 header[12] = path_nodes,
// edges, order, sigma, fast_chars, sample_count, sample_width, extra_values_len, redundant_len,
// lcp_size, lcp_branching, lcp_levels; u64 flags (bit 0 samples, bit 1 counters, bit 2 lcp);
// then the arrays in the order of gcsa2_host_view, each as u64 byte length + bytes padded to 8.

struct gcsa2_view_storage
{
  gcsa2_host_view view;
  std::vector<std::vector<u64>> blobs;    // 8-byte aligned backing store
  std::vector<const u64*> bwt;
  std::vector<uint8_t> comp2char;         // alpha.comp2char as the file had it (GCSA::load keeps it, so serialize() must too)
};

namespace {

constexpr u32 G2HV_VERSION = 1;

u64 words_for_bits(u64 bits) { return (bits + 63) / 64; }

bool write_blob(FILE* f, const void* data, u64 bytes)
{
  u64 padded = (bytes + 7) & ~u64(7);
  static const char zeros[8] = {0};
  if(fwrite(&bytes, 8, 1, f) != 1) { return false; }
  if(bytes > 0 && fwrite(data, 1, bytes, f) != bytes) { return false; }
  if(padded > bytes && fwrite(zeros, 1, padded - bytes, f) != padded - bytes) { return false; }
  return true;
}

bool read_blob(FILE* f, std::vector<u64>& dst, u64& bytes)
{
  if(fread(&bytes, 8, 1, f) != 1) { return false; }
  if(bytes > (u64(1) << 40)) { return false; }
  dst.assign((bytes + 7) / 8 + 2, 0);        // two spare words: word-granular readers may overrun
  u64 padded = (bytes + 7) & ~u64(7);
  return padded == 0 || fread(dst.data(), 1, padded, f) == padded;
}

}  // namespace

extern "C" int gcsa2_host_view_save(const gcsa2_host_view* v, const char* path)
{
  if(v == nullptr || path == nullptr || v->char2comp == nullptr || v->C == nullptr || v->bwt == nullptr || v->edge_bits == nullptr)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "incomplete host view");
  }
  FILE* f = fopen(path, "wb");
  if(f == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, std::string("cannot open ") + path); }
  bool ok = true;
  u64 flags = (v->sampled_path_bits ? 1 : 0) | (v->extra_filter_bits ? 2 : 0) | (v->lcp_data ? 4 : 0);
  u64 header[12] = { v->path_nodes, v->edges, v->order, v->sigma, v->fast_chars, v->sample_count, v->sample_width,
                     v->extra_values_len, v->redundant_len, v->lcp_size, v->lcp_branching, v->lcp_levels };
  ok = ok && fwrite("G2HV", 1, 4, f) == 4 && fwrite(&G2HV_VERSION, 4, 1, f) == 1;
  ok = ok && fwrite(header, 8, 12, f) == 12 && fwrite(&flags, 8, 1, f) == 1;
  ok = ok && write_blob(f, v->char2comp, 256) && write_blob(f, v->C, (v->sigma + 1) * 8);
  for(u64 c = 0; ok && c < v->sigma; c++) { ok = write_blob(f, v->bwt[c], words_for_bits(v->path_nodes) * 8); }
  ok = ok && write_blob(f, v->edge_bits, words_for_bits(v->edges) * 8);
  if(flags & 1)
  {
    ok = ok && write_blob(f, v->sampled_path_bits, words_for_bits(v->path_nodes) * 8);
    ok = ok && write_blob(f, v->stored_samples, words_for_bits(v->sample_count * v->sample_width) * 8);
    ok = ok && write_blob(f, v->sample_bits, words_for_bits(v->sample_count) * 8);
  }
  if(flags & 2)
  {
    ok = ok && write_blob(f, v->extra_filter_bits, words_for_bits(v->path_nodes) * 8);
    ok = ok && write_blob(f, v->extra_values_bits, words_for_bits(v->extra_values_len) * 8);
    ok = ok && write_blob(f, v->redundant_bits, words_for_bits(v->redundant_len) * 8);
  }
  if(flags & 4)
  {
    ok = ok && write_blob(f, v->lcp_offsets, (v->lcp_levels + 1) * 8);
    ok = ok && write_blob(f, v->lcp_data, v->lcp_offsets[v->lcp_levels]);
  }
  ok = (fclose(f) == 0) && ok;
  return ok ? GCSA2_OK : fail(GCSA2_ERR_INVALID_ARGUMENT, std::string("write error on ") + path);
}

extern "C" void gcsa2_host_view_free(gcsa2_view_storage* storage) { delete storage; }

extern "C" const gcsa2_host_view* gcsa2_host_view_get(const gcsa2_view_storage* storage) { return storage ? &storage->view : nullptr; }

extern "C" int gcsa2_host_view_load(const char* path, gcsa2_view_storage** out)
{
  if(path == nullptr || out == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null argument"); }
  *out = nullptr;
  FILE* f = fopen(path, "rb");
  if(f == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, std::string("cannot open ") + path); }
  struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
  try
  {
    char magic[4]; u32 version = 0; u64 header[12], flags = 0;
    if(fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "G2HV", 4) != 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "not a G2HV file: invalid tag"); }
    if(fread(&version, 4, 1, f) != 1 || version != G2HV_VERSION) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: unsupported version"); }
    if(fread(header, 8, 12, f) != 12 || fread(&flags, 8, 1, f) != 1) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: truncated header"); }
    if(header[3] == 0 || header[3] > GCSA2_MAX_SIGMA || header[11] > u64(MAX_LCP_LEVELS)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: header out of range"); }
    std::unique_ptr<gcsa2_view_storage> st(new gcsa2_view_storage());
    gcsa2_host_view& v = st->view;
    std::memset(&v, 0, sizeof(v));
    v.path_nodes = header[0]; v.edges = header[1]; v.order = header[2]; v.sigma = header[3]; v.fast_chars = header[4];
    v.sample_count = header[5]; v.sample_width = header[6]; v.extra_values_len = header[7]; v.redundant_len = header[8];
    v.lcp_size = header[9]; v.lcp_branching = header[10]; v.lcp_levels = header[11];
    u64 nblobs = 2 + v.sigma + 1 + ((flags & 1) ? 3 : 0) + ((flags & 2) ? 3 : 0) + ((flags & 4) ? 2 : 0);
    st->blobs.resize(nblobs);
    std::vector<u64> sizes(nblobs, 0);
    for(u64 b = 0; b < nblobs; b++)
    {
      if(!read_blob(f, st->blobs[b], sizes[b])) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: truncated array"); }
    }
    u64 b = 0;
    auto expect = [&](u64 bytes) -> bool { return sizes[b] == bytes; };
    if(!expect(256)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: char2comp size"); }
    v.char2comp = reinterpret_cast<const uint8_t*>(st->blobs[b++].data());
    if(!expect((v.sigma + 1) * 8)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: C size"); }
    v.C = st->blobs[b++].data();
    for(u64 c = 0; c < v.sigma; c++)
    {
      if(!expect(words_for_bits(v.path_nodes) * 8)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: bwt size"); }
      st->bwt.push_back(st->blobs[b++].data());
    }
    v.bwt = st->bwt.data();
    if(!expect(words_for_bits(v.edges) * 8)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: edges size"); }
    v.edge_bits = st->blobs[b++].data();
    if(flags & 1)
    {
      if(v.sample_width == 0 || v.sample_width > 64 || v.sample_count > (u64(1) << 46)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: sample header out of range"); }
      if(!expect(words_for_bits(v.path_nodes) * 8)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: sampled_paths size"); }
      v.sampled_path_bits = st->blobs[b++].data();
      if(!expect(words_for_bits(v.sample_count * v.sample_width) * 8)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: stored_samples size"); }
      v.stored_samples = st->blobs[b++].data();
      if(!expect(words_for_bits(v.sample_count) * 8)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: samples size"); }
      v.sample_bits = st->blobs[b++].data();
    }
    if(flags & 2)
    {
      if(!expect(words_for_bits(v.path_nodes) * 8)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: extra_pointers.filter size"); }
      v.extra_filter_bits = st->blobs[b++].data();
      if(!expect(words_for_bits(v.extra_values_len) * 8)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: extra_pointers.values size"); }
      v.extra_values_bits = st->blobs[b++].data();
      if(!expect(words_for_bits(v.redundant_len) * 8)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: redundant_pointers size"); }
      v.redundant_bits = st->blobs[b++].data();
    }
    if(flags & 4)
    {
      if(!expect((v.lcp_levels + 1) * 8)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: lcp offsets size"); }
      v.lcp_offsets = st->blobs[b++].data();
      if(sizes[b] != v.lcp_offsets[v.lcp_levels]) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "G2HV: lcp data size"); }
      v.lcp_data = reinterpret_cast<const uint8_t*>(st->blobs[b++].data());
    }
    *out = st.release();
    return GCSA2_OK;
  }
  catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_host_view_load: ") + e.what()); }
}

extern "C" int gcsa2_index_create_from_file(const char* path, int device, gcsa2_index** out)
{
  gcsa2_view_storage* st = nullptr;
  int rc = gcsa2_host_view_load(path, &st);
  if(rc != GCSA2_OK) { return rc; }
  rc = gcsa2_index_create(&st->view, device, out);
  gcsa2_host_view_free(st);
  return rc;
}

// ---- `.gcsa` / `.lcp` files as written by GCSA::serialize / LCPArray::serialize ---------------------
// Member order: src/gcsa.cpp:140-216 (GCSA), src/support.cpp:229-250 (Alphabet), :401-418 (SadaCount),
// :493-516 (SadaSparse), src/files.cpp:513-537 / :581-603 (headers), src/lcp.cpp:116-143 (LCPArray).
// SDSL container encodings: sdsl_reader.hpp (format parity unpinned, see its header).

namespace {

// `exact`: the stream must end with the structure (a file); otherwise trailing bytes are left to the caller
void load_gcsa_members(sdsl_file::Cursor& in, gcsa2_view_storage& st, bool exact)
{
  using namespace sdsl_file;
  gcsa2_host_view& v = st.view;

  // GCSAHeader (files.cpp:527-543): tag, version, path_nodes, edges, order, flags
  u32 tag = in.get<u32>("header.tag"), version = in.get<u32>("header.version");
  v.path_nodes = in.get<u64>("header.path_nodes"); v.edges = in.get<u64>("header.edges"); v.order = in.get<u64>("header.order");
  u64 flags = in.get<u64>("header.flags");
  if(tag != 0x6C5A6C5Au || version != 3 || flags != 0)
  {
    in.error("Invalid header: tag " + std::to_string(tag) + ", version " + std::to_string(version) + ", flags " + std::to_string(flags)
             + " (expected GCSA version 3 as written by GCSA::serialize / sdsl::store_to_file; a file wrapped in another"
               " container, e.g. a tagged stream, has to be unwrapped first)");
  }

  // Alphabet (support.cpp:243-250)
  IntVector char2comp = read_int_vector(in, 8, "alpha.char2comp");
  IntVector comp2char = read_int_vector(in, 8, "alpha.comp2char");
  IntVector C = read_int_vector(in, 64, "alpha.C");
  v.sigma = in.get<u64>("alpha.sigma"); v.fast_chars = in.get<u64>("alpha.fast_chars");
  if(char2comp.size() != 256) { in.error("alpha.char2comp must have 256 entries"); }
  if(v.sigma == 0 || v.sigma > GCSA2_MAX_SIGMA || C.size() != v.sigma + 1) { in.error("alphabet size out of range or alpha.C of the wrong length"); }
  if(v.fast_chars >= v.sigma) { in.error("alpha.fast_chars out of range"); }
  if(comp2char.size() == v.sigma)
  {
    std::vector<u64> words;
    comp2char.copy_words(words);
    st.comp2char.assign(reinterpret_cast<const uint8_t*>(words.data()), reinterpret_cast<const uint8_t*>(words.data()) + v.sigma);
    v.comp2char = st.comp2char.data();
  }

  st.blobs.resize(2 + v.sigma + 9);
  u64 b = 0;
  char2comp.copy_words(st.blobs[b]); v.char2comp = reinterpret_cast<const uint8_t*>(st.blobs[b++].data());
  C.copy_words(st.blobs[b]); v.C = st.blobs[b++].data();

  // fast_bwt, fast_rank (empty), sparse_bwt, sparse_rank (empty): gcsa.cpp:196-202.  LF reads fast_bwt for
  // 1 <= comp <= fast_chars and sparse_bwt otherwise (gcsa.h:262-274).
  std::vector<std::vector<u64>> fast(v.sigma), sparse(v.sigma);
  std::vector<u64> fast_size(v.sigma), sparse_size(v.sigma);
  for(u64 c = 0; c < v.sigma; c++) { read_bit_vector_il(in, fast[c], fast_size[c], "fast_bwt"); }
  for(u64 c = 0; c < v.sigma; c++) { read_sd_vector(in, sparse[c], sparse_size[c], "sparse_bwt"); }
  for(u64 c = 0; c < v.sigma; c++)
  {
    const bool is_fast = (c > 0 && c <= v.fast_chars);
    if((is_fast ? fast_size[c] : sparse_size[c]) != v.path_nodes) { in.error("BWT bitvector of comp " + std::to_string(c) + " does not have path_nodes bits"); }
    st.blobs[b].swap(is_fast ? fast[c] : sparse[c]);
    st.bwt.push_back(st.blobs[b++].data());
  }
  v.bwt = st.bwt.data();

  u64 size = 0;
  read_bit_vector_il(in, st.blobs[b], size, "edges");                   // + edge_rank (empty)
  if(size != v.edges) { in.error("edges does not have header.edges bits"); }
  v.edge_bits = st.blobs[b++].data();
  read_bit_vector_il(in, st.blobs[b], size, "sampled_paths");           // + sampled_path_rank (empty)
  if(size != v.path_nodes) { in.error("sampled_paths does not have path_nodes bits"); }
  v.sampled_path_bits = st.blobs[b++].data();

  IntVector stored = read_int_vector(in, 0, "stored_samples");
  v.sample_count = stored.size(); v.sample_width = stored.width;
  stored.copy_words(st.blobs[b]); v.stored_samples = st.blobs[b++].data();
  read_bit_vector(in, st.blobs[b], size, "samples");
  if(size != v.sample_count) { in.error("samples and stored_samples differ in length"); }
  v.sample_bits = st.blobs[b++].data();
  skip_select_mcl(in, "sample_select");

  // extra_pointers (SadaSparse, support.cpp:509-516): filter, filter_rank (empty), values, value_select (empty)
  read_sd_vector(in, st.blobs[b], size, "extra_pointers.filter");
  if(size != v.path_nodes) { in.error("extra_pointers.filter does not have path_nodes bits"); }
  v.extra_filter_bits = st.blobs[b++].data();
  read_sd_vector(in, st.blobs[b], v.extra_values_len, "extra_pointers.values");
  v.extra_values_bits = st.blobs[b++].data();
  // redundant_pointers (SadaCount, support.cpp:414-418): data, select
  read_bit_vector(in, st.blobs[b], v.redundant_len, "redundant_pointers.data");
  v.redundant_bits = st.blobs[b++].data();
  skip_select_mcl(in, "redundant_pointers.select");

  if(exact && !in.at_end()) { in.error(std::to_string(in.remaining()) + " unaccounted bytes after redundant_pointers"); }
}

void load_gcsa_members(const char* path, gcsa2_view_storage& st)
{
  sdsl_file::Mapping map(path);
  sdsl_file::Cursor in(map, std::string("GCSA::load(") + path + ")");
  load_gcsa_members(in, st, true);
}

void load_lcp_members(sdsl_file::Cursor& in, gcsa2_view_storage& st, bool exact)
{
  using namespace sdsl_file;
  gcsa2_host_view& v = st.view;

  // LCPHeader (files.cpp:595-609): tag, version, size, branching, flags
  u32 tag = in.get<u32>("header.tag"), version = in.get<u32>("header.version");
  v.lcp_size = in.get<u64>("header.size"); v.lcp_branching = in.get<u64>("header.branching");
  u64 flags = in.get<u64>("header.flags");
  if(tag != 0x6C5A7C94u || version != 1 || flags != 0)
  {
    in.error("Invalid header: tag " + std::to_string(tag) + ", version " + std::to_string(version) + ", flags " + std::to_string(flags)
             + " (expected LCP version 1)");
  }
  IntVector data = read_int_vector(in, 0, "data");
  IntVector offsets = read_int_vector(in, 64, "offsets");
  if(exact && !in.at_end()) { in.error(std::to_string(in.remaining()) + " unaccounted bytes after offsets"); }
  if(data.width > 8) { in.error("LCP values wider than 8 bits are not supported"); }
  if(offsets.size() < 2 || offsets.size() - 1 > u64(MAX_LCP_LEVELS)) { in.error("offsets: number of levels out of range"); }
  v.lcp_levels = offsets.size() - 1;
  if(offsets.word(0) != 0 || offsets.word(1) != v.lcp_size || offsets.word(v.lcp_levels) != data.size()) { in.error("offsets do not match header.size / data"); }

  st.blobs.emplace_back(); offsets.copy_words(st.blobs.back());
  const u64* offsets_ptr = st.blobs.back().data();
  st.blobs.emplace_back((data.size() + 7) / 8 + 2, 0);
  uint8_t* bytes = reinterpret_cast<uint8_t*>(st.blobs.back().data());
  for(u64 i = 0; i < data.size(); i++) { bytes[i] = uint8_t(data.get(i)); }
  v.lcp_offsets = offsets_ptr; v.lcp_data = bytes;
}

void load_lcp_members(const char* path, gcsa2_view_storage& st)
{
  sdsl_file::Mapping map(path);
  sdsl_file::Cursor in(map, std::string("LCP::load(") + path + ")");
  load_lcp_members(in, st, true);
}

template<class Loader>
int parse_memory(const void* bytes, uint64_t size, uint64_t* consumed, gcsa2_view_storage** out, const char* what, Loader load)
{
  if((bytes == nullptr && size > 0) || out == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null argument"); }
  *out = nullptr;
  try
  {
    std::unique_ptr<gcsa2_view_storage> st(new gcsa2_view_storage());
    std::memset(&st->view, 0, sizeof(st->view));
    st->blobs.reserve(64);
    sdsl_file::Cursor in(bytes, size, what);          // an empty stream fails as "truncated while reading header.tag"
    load(in, *st, consumed == nullptr);
    if(consumed != nullptr) { *consumed = in.consumed(); }
    *out = st.release();
    return GCSA2_OK;
  }
  catch(const sdsl_file::FormatError& e) { return fail(GCSA2_ERR_INVALID_ARGUMENT, e.what()); }
  catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string(what) + ": " + e.what()); }
}

} // namespace

extern "C" int gcsa2_host_view_parse_gcsa(const void* bytes, uint64_t size, uint64_t* consumed, gcsa2_view_storage** out)
{
  return parse_memory(bytes, size, consumed, out, "GCSA::load()",
                      [](sdsl_file::Cursor& in, gcsa2_view_storage& st, bool exact) { load_gcsa_members(in, st, exact); });
}

extern "C" int gcsa2_host_view_parse_lcp(const void* bytes, uint64_t size, uint64_t* consumed, gcsa2_view_storage** out)
{
  return parse_memory(bytes, size, consumed, out, "LCP::load()",
                      [](sdsl_file::Cursor& in, gcsa2_view_storage& st, bool exact) { load_lcp_members(in, st, exact); });
}

// GCSA::serialize (src/gcsa.cpp:140-179): header, alphabet, fast_bwt + fast_rank, sparse_bwt + sparse_rank, edges + edge_rank,
// sampled_paths + rank, stored_samples, samples + select, extra_pointers, redundant_pointers.  The rank supports of
// bit_vector_il and sd_vector, and the select support of sd_vector, serialize to nothing.
extern "C" int gcsa2_host_view_serialize_gcsa(const gcsa2_host_view* v, gcsa2_sink sink, void* ctx, uint64_t* written)
{
  if(v == nullptr || sink == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null argument"); }
  if(v->sampled_path_bits == nullptr || v->extra_filter_bits == nullptr)
  {
    return fail(GCSA2_ERR_MISSING_COMPONENT, "GCSA::serialize() needs the samples and the counters (a .gcsa file always holds them)");
  }
  try
  {
    using namespace sdsl_file;
    Writer out(sink, ctx);
    out.put<u32>(0x6C5A6C5Au); out.put<u32>(3);                       // GCSAHeader (files.cpp:513-525)
    out.put<u64>(v->path_nodes); out.put<u64>(v->edges); out.put<u64>(v->order); out.put<u64>(0);
    // Alphabet (support.cpp:228-241): char2comp, comp2char, C, sigma, fast_chars.  comp2char travels in the view when
    // it came from a file; otherwise it is derived by the one rule the facade's Alphabet uses too.
    out.int_vector8(v->char2comp, 256, false);
    std::vector<u8> comp2char(v->sigma, 0);
    if(v->comp2char != nullptr) { std::memcpy(comp2char.data(), v->comp2char, v->sigma); }      // as loaded (or as the caller's Alphabet has it)
    else { gcsa2_derive_comp2char(v->char2comp, v->sigma, comp2char.data()); }
    out.int_vector8(comp2char.data(), v->sigma, false);
    out.int_vector64(v->C, v->sigma + 1);
    out.put<u64>(v->sigma); out.put<u64>(v->fast_chars);
    for(u64 c = 0; c < v->sigma; c++)
    {
      if(c > 0 && c <= v->fast_chars) { write_bit_vector_il(out, v->bwt[c], v->path_nodes); } else { write_empty_bit_vector_il(out); }
    }
    for(u64 c = 0; c < v->sigma; c++)
    {
      if(c > 0 && c <= v->fast_chars) { write_empty_sd_vector(out); } else { write_sd_vector(out, v->bwt[c], v->path_nodes); }
    }
    write_bit_vector_il(out, v->edge_bits, v->edges);
    write_bit_vector_il(out, v->sampled_path_bits, v->path_nodes);
    out.int_vector0_words(v->stored_samples, v->sample_count, u8(v->sample_width));
    out.bit_vector(v->sample_bits, v->sample_count);
    write_select_mcl(out, v->sample_bits, v->sample_count, true);
    write_sd_vector(out, v->extra_filter_bits, v->path_nodes);        // SadaSparse (support.cpp:493-503)
    write_sd_vector(out, v->extra_values_bits, v->extra_values_len);
    out.bit_vector(v->redundant_bits, v->redundant_len);              // SadaCount (support.cpp:401-408)
    write_select_mcl(out, v->redundant_bits, v->redundant_len, true);
    if(written != nullptr) { *written = out.written(); }
    return GCSA2_OK;
  }
  catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("GCSA::serialize(): ") + e.what()); }
}

// LCPArray::serialize (src/lcp.cpp:116-128): header, data (bit-compressed int_vector<0>, lcp.cpp:258), offsets.
extern "C" int gcsa2_host_view_serialize_lcp(const gcsa2_host_view* v, gcsa2_sink sink, void* ctx, uint64_t* written)
{
  if(v == nullptr || sink == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null argument"); }
  if(v->lcp_data == nullptr) { return fail(GCSA2_ERR_MISSING_COMPONENT, "the view holds no LCP array"); }
  try
  {
    using namespace sdsl_file;
    Writer out(sink, ctx);
    out.put<u32>(0x6C5A7C94u); out.put<u32>(1);                       // LCPHeader (files.cpp:581-593)
    out.put<u64>(v->lcp_size); out.put<u64>(v->lcp_branching); out.put<u64>(0);
    const u64 values = v->lcp_offsets[v->lcp_levels];
    u8 top = 0;
    for(u64 i = 0; i < values; i++) { top = (v->lcp_data[i] > top ? v->lcp_data[i] : top); }
    const u8 width = u8(bits_hi(top) + 1);                            // sdsl::util::bit_compress
    if(width == 8) { out.int_vector8(v->lcp_data, values, true); }
    else
    {
      std::vector<u64> wide(values);
      for(u64 i = 0; i < values; i++) { wide[i] = v->lcp_data[i]; }
      out.int_vector0(wide, width);
    }
    out.int_vector64(v->lcp_offsets, v->lcp_levels + 1);
    if(written != nullptr) { *written = out.written(); }
    return GCSA2_OK;
  }
  catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("LCP::serialize(): ") + e.what()); }
}

// An image that holds only the LCP array: what a default-constructed gcsa::LCPArray becomes after load()
// (src/lcp.cpp:130-143).  parent / depth / psv / nsv / rmq work on it; everything that needs the GCSA part fails
// with GCSA2_ERR_MISSING_COMPONENT or returns empty results.
extern "C" int gcsa2_lcp_create(const gcsa2_host_view* v, int device, gcsa2_index** out)
{
  if(v == nullptr || out == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null argument"); }
  *out = nullptr;
  if(v->lcp_data == nullptr || v->lcp_offsets == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "the view holds no LCP array"); }
  static const uint8_t c2c[256] = {0};
  static const uint64_t C[2] = {0, 0}, none[2] = {0, 0};
  static const uint64_t* const bwt[1] = { none };
  gcsa2_host_view lcp_only;
  std::memset(&lcp_only, 0, sizeof(lcp_only));
  lcp_only.sigma = 1; lcp_only.char2comp = c2c; lcp_only.C = C; lcp_only.bwt = bwt; lcp_only.edge_bits = none;
  lcp_only.lcp_size = v->lcp_size; lcp_only.lcp_branching = v->lcp_branching; lcp_only.lcp_levels = v->lcp_levels;
  lcp_only.lcp_offsets = v->lcp_offsets; lcp_only.lcp_data = v->lcp_data;
  return gcsa2_index_create(&lcp_only, device, out);
}

extern "C" int gcsa2_host_view_load_gcsa(const char* gcsa_path, const char* lcp_path, gcsa2_view_storage** out)
{
  if(gcsa_path == nullptr || out == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null argument"); }
  *out = nullptr;
  try
  {
    std::unique_ptr<gcsa2_view_storage> st(new gcsa2_view_storage());
    std::memset(&st->view, 0, sizeof(st->view));
    st->blobs.reserve(64);      // pointers into the blobs' heap buffers stay valid either way; avoids reallocation churn
    load_gcsa_members(gcsa_path, *st);
    if(lcp_path != nullptr) { load_lcp_members(lcp_path, *st); }
    *out = st.release();
    return GCSA2_OK;
  }
  catch(const sdsl_file::FormatError& e) { return fail(GCSA2_ERR_INVALID_ARGUMENT, e.what()); }
  catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_host_view_load_gcsa: ") + e.what()); }
}

extern "C" int gcsa2_index_create_from_gcsa(const char* gcsa_path, const char* lcp_path, int device, gcsa2_index** out)
{
  gcsa2_view_storage* st = nullptr;
  int rc = gcsa2_host_view_load_gcsa(gcsa_path, lcp_path, &st);
  if(rc != GCSA2_OK) { return rc; }
  rc = gcsa2_index_create(&st->view, device, out);
  gcsa2_host_view_free(st);
  return rc;
}

// ==== MEM hits: a MEM finder's count() + locate() per match in one call (kernels_mem.hpp) ==================================
namespace {

constexpr u64 MEM_SAMPLED_PART = LMAX_BATCH - 1;     // locate_max_core takes fewer than LMAX_BATCH ranges per call

int mem_hits_checks(const gcsa2_index* ix, u64 min_length, int over)
{
  if(min_length == 0)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "mem_hits: min_length must be at least 1 (a record of length 0 carries the whole index as its range)");
  }
  if(over != GCSA2_MEM_OVER_SKIP && over != GCSA2_MEM_OVER_SAMPLE)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "mem_hits: unknown over-cap policy (GCSA2_MEM_OVER_SKIP or GCSA2_MEM_OVER_SAMPLE)");
  }
  if(!ix->img.has_lcp) { return fail(GCSA2_ERR_MISSING_COMPONENT, "index was created without an LCP array"); }
  return locate_checks(ix, 0);
}

// The sampled class through locate_max_core: one CSR (d_offsets, ns + 1 entries; *d_values from `scratch`).  A class of
// LMAX_BATCH ranges or more goes in parts below that limit, whose offsets are shifted and whose values are concatenated.
int mem_sampled(const gcsa2_index* ix, const u64* d_ranges, u64 ns, u64 hit_max, u64* d_offsets, Scratch& scratch,
                u64** d_values, u64* total_out, hipStream_t st)
{
  *total_out = 0;
  *d_values = nullptr;
  if(ns <= MEM_SAMPLED_PART)
  {
    auto provide = [&scratch, d_values](u64 count, u64** out) -> int { HIP_TRY(scratch.get(*d_values, count)); *out = *d_values; return GCSA2_OK; };
    return locate_max_core(ix, d_ranges, ns, hit_max, d_offsets, provide, total_out, st);
  }
  struct Part { u64 q0 = 0, count = 0, total = 0; u64* d_off = nullptr; u64* d_val = nullptr; };
  std::vector<Part> parts;
  u64 total = 0;
  for(u64 q0 = 0; q0 < ns; q0 += MEM_SAMPLED_PART)
  {
    Part part;
    part.q0 = q0; part.count = std::min(MEM_SAMPLED_PART, ns - q0);
    HIP_TRY(scratch.get(part.d_off, part.count + 1));
    Part* self = &part;
    auto provide = [&scratch, self](u64 count, u64** out) -> int { HIP_TRY(scratch.get(self->d_val, count)); *out = self->d_val; return GCSA2_OK; };
    const int rc = locate_max_core(ix, d_ranges + 2 * q0, part.count, hit_max, part.d_off, provide, &part.total, st);
    if(rc != GCSA2_OK) { return rc; }
    total += part.total;
    parts.push_back(part);
  }
  HIP_TRY(scratch.get(*d_values, total));
  u64 base = 0;
  for(const Part& part : parts)
  {
    if(part.total > 0) { HIP_TRY(hipMemcpyAsync(*d_values + base, part.d_val, part.total * sizeof(u64), hipMemcpyDeviceToDevice, st)); }
    hipLaunchKernelGGL(k_shift_offsets, dim3(grid_for(part.count)), dim3(TPB), 0, st, part.d_off, part.count, base, d_offsets + part.q0);
    LAUNCH_CHECK("k_shift_offsets");
    base += part.total;
  }
  HIP_TRY(hipMemcpyAsync(d_offsets + ns, &total, sizeof(u64), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  *total_out = total;
  return GCSA2_OK;
}

int mem_hits_tail(const gcsa2_index* ix, const u64* brk, const u64* known, u64 m, u64 hit_max, int over, gcsa2_mem* d_mems, u64 mem_capacity,
                  u64* d_hit_offsets, u64* d_hits, u64 hit_capacity, u64* total_hits, Scratch& scratch, hipStream_t st);

// gcsa2_mem_hits_device after its argument checks (nq > 0).  Host round trips: the pattern bytes (only when the caller does
// not know them), the break total (inside gcsa2_match_breaks_device), the class totals, those of the locate passes, the end.
int mem_hits_core(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 nq, u64 total_bytes, u64 min_length, u64 max_length,
                  u64 hit_max, int over, u64* d_mem_offsets, gcsa2_mem* d_mems, u64 mem_capacity, u64* total_mems,
                  u64* d_hit_offsets, u64* d_hits, u64 hit_capacity, u64* total_hits, hipStream_t st)
{
  Scratch scratch(ix, st);
  if(total_bytes == GCSA2_UNKNOWN)
  {
    HIP_TRY(hipMemcpyAsync(&total_bytes, d_offsets + nq, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  // 1. the break records, into scratch: room for the caller's MEM capacity or one record per 8 pattern bytes (a MEM finder's
  //    minimum length keeps far fewer), never more than one per position and pattern; a batch that needs more runs again
  u64 room = std::max(total_bytes / 8 + nq + 1, mem_capacity);
  room = std::min(room, total_bytes + nq);
  u64* brk = nullptr;
  u64 m = 0;
  HIP_TRY(scratch.get(brk, 4 * room));
  int rc = gcsa2_match_breaks_bounded_device(ix, d_patterns, d_offsets, nq, total_bytes, 0, min_length, max_length, d_mem_offsets, reinterpret_cast<gcsa2_break*>(brk),
                                     room, &m, nullptr, nullptr, st);
  if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && m > room)
  {
    room = m;
    HIP_TRY(scratch.get(brk, 4 * room));
    g_error.clear();
    rc = gcsa2_match_breaks_bounded_device(ix, d_patterns, d_offsets, nq, total_bytes, 0, min_length, max_length, d_mem_offsets, reinterpret_cast<gcsa2_break*>(brk),
                                   room, &m, nullptr, nullptr, st);
  }
  if(rc != GCSA2_OK) { return rc; }
  *total_mems = m;
  if(m >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "mem_hits: 2^32 or more MEMs in one batch; split the batch"); }
  if(m == 0)
  {
    HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipStreamSynchronize(st));
    scratch.settled = true;
    return GCSA2_OK;
  }
  return mem_hits_tail(ix, brk, nullptr, m, hit_max, over, d_mems, mem_capacity, d_hit_offsets, d_hits, hit_capacity, total_hits, scratch, st);
}

// Steps 2 onward of a MEM hits call, shared by mem_hits_core and sub_mem_hits_core: m (1 <= m < 2^32) records {position,
// length, sp, ep} in device memory, with their count()s in `known` or (nullptr) computed here, become the caller's gcsa2_mem
// records and their hit CSR.  *total_hits is always set; BUFFER_TOO_SMALL (m > mem_capacity or hits > hit_capacity) writes
// nothing of the caller's.
int mem_hits_tail(const gcsa2_index* ix, const u64* brk, const u64* known, u64 m, u64 hit_max, int over, gcsa2_mem* d_mems, u64 mem_capacity,
                  u64* d_hit_offsets, u64* d_hits, u64 hit_capacity, u64* total_hits, Scratch& scratch, hipStream_t st)
{
  int rc = GCSA2_OK;
  // 2. count() and the class of every MEM, one scan for the positions in both range lists and the full class's count() sum
  u64 *mems = nullptr, *full = nullptr, *sampled = nullptr, *full_off = nullptr, *full_val = nullptr, *samp_off = nullptr, *samp_val = nullptr;
  MemScan *words = nullptr, *pos = nullptr;
  char* scan_tmp = nullptr;
  HIP_TRY(scratch.get(mems, 5 * m));
  HIP_TRY(scratch.get(words, m + 1));
  HIP_TRY(scratch.get(pos, m + 1));
  hipLaunchKernelGGL(k_mem_classify, dim3(grid_for(m + 1)), dim3(TPB), 0, st, ix->img, brk, known, m, hit_max, int(over == GCSA2_MEM_OVER_SAMPLE), mems, words);
  LAUNCH_CHECK("k_mem_classify");
  size_t scan_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveScan(nullptr, scan_bytes, words, pos, MemScanOp(), MemScan{0, 0}, size_t(m + 1), st));
  HIP_TRY(scratch.get(scan_tmp, scan_bytes));
  HIP_TRY(hipcub::DeviceScan::ExclusiveScan(scan_tmp, scan_bytes, words, pos, MemScanOp(), MemScan{0, 0}, size_t(m + 1), st));
  MemScan sums{0, 0};
  HIP_TRY(hipMemcpyAsync(&sums, pos + m, sizeof(MemScan), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const u64 nf = sums.cls & MEM_CLASS_LOW, ns = sums.cls >> 32;
  HIP_TRY(scratch.get(full, 2 * nf));
  HIP_TRY(scratch.get(sampled, 2 * ns));
  hipLaunchKernelGGL(k_mem_compact, dim3(grid_for(m)), dim3(TPB), 0, st, mems, m, pos, full, sampled);
  LAUNCH_CHECK("k_mem_compact");
  // 3. the full class: straight into the caller's hits when nothing else goes there and they are known to fit (count() bounds
  //    the distinct values of a range), otherwise into scratch
  const bool direct = (ns == 0 && m <= mem_capacity && sums.sum < MEM_SUM_CAP && sums.sum <= hit_capacity);
  u64 full_total = 0;
  HIP_TRY(scratch.get(full_off, nf + 1));
  if(direct)
  {
    ValuesProvider provide = [d_hits, hit_capacity](u64 count) -> u64* { return count <= hit_capacity ? d_hits : nullptr; };
    rc = locate_core(ix, full, nf, 1, full_off, provide, &full_total, st, d_hits, hit_capacity);
    full_val = d_hits;
  }
  else
  {
    ValuesProvider provide = [&scratch, &full_val](u64 count) -> u64*
    {
      const hipError_t e = scratch.get(full_val, count);
      if(e != hipSuccess) { fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("mem_hits: values of the full class: ") + hipGetErrorString(e)); return nullptr; }
      return full_val;
    };
    rc = locate_core(ix, full, nf, 1, full_off, provide, &full_total, st);
  }
  if(rc != GCSA2_OK) { return rc; }
  // 4. the sampled class
  u64 samp_total = 0;
  if(ns > 0)
  {
    HIP_TRY(scratch.get(samp_off, ns + 1));
    rc = mem_sampled(ix, sampled, ns, hit_max, samp_off, scratch, &samp_val, &samp_total, st);
    if(rc != GCSA2_OK) { return rc; }
  }
  const u64 h = full_total + samp_total;
  *total_hits = h;
  if(m > mem_capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "MEM buffer too small"); }
  if(h > hit_capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "hit buffer too small"); }
  // 5. the results in MEM order
  HIP_TRY(hipMemcpyAsync(d_mems, mems, m * sizeof(gcsa2_mem), hipMemcpyDeviceToDevice, st));
  if(ns == 0)
  {
    hipLaunchKernelGGL(k_mem_spread, dim3(grid_for(m + 1)), dim3(TPB), 0, st, pos, m, full_off, d_hit_offsets);
    LAUNCH_CHECK("k_mem_spread");
    if(!direct && full_total > 0) { HIP_TRY(hipMemcpyAsync(d_hits, full_val, full_total * sizeof(u64), hipMemcpyDeviceToDevice, st)); }
  }
  else
  {
    u64* sizes = nullptr;
    HIP_TRY(scratch.get(sizes, m + 1));
    hipLaunchKernelGGL(k_mem_sizes, dim3(grid_for(m + 1)), dim3(TPB), 0, st, pos, m, full_off, samp_off, sizes);
    LAUNCH_CHECK("k_mem_sizes");
    size_t sum_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, sum_bytes, sizes, d_hit_offsets, size_t(m + 1), st));
    char* sum_tmp = nullptr;
    HIP_TRY(scratch.get(sum_tmp, sum_bytes));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sum_tmp, sum_bytes, sizes, d_hit_offsets, size_t(m + 1), st));
    if(h > 0)
    {
      hipLaunchKernelGGL(k_mem_gather, dim3(grid_for(h)), dim3(TPB), 0, st, pos, m, d_hit_offsets, h, full_off, full_val, samp_off, samp_val, d_hits);
      LAUNCH_CHECK("k_mem_gather");
    }
  }
  HIP_TRY(hipStreamSynchronize(st));
  scratch.settled = true;
  return GCSA2_OK;
}

}  // namespace

extern "C" {

int gcsa2_mem_hits_bounded_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t nq, uint64_t total_pattern_bytes,
                                  uint64_t min_length, uint64_t max_length, uint64_t hit_max, int over, uint64_t* d_mem_offsets, gcsa2_mem* d_mems,
                                  uint64_t mem_capacity, uint64_t* total_mems, uint64_t* d_hit_offsets, uint64_t* d_hits, uint64_t hit_capacity,
                                  uint64_t* total_hits, void* stream)
{
  CHECK_INDEX(ix);
  CHECK_CAP(min_length, max_length);
  if(total_mems == nullptr || total_hits == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null total pointer"); }
  *total_mems = 0;
  *total_hits = 0;
  if(d_mem_offsets == nullptr || d_hit_offsets == nullptr || (d_offsets == nullptr && nq > 0) || (d_mems == nullptr && mem_capacity > 0) ||
     (d_hits == nullptr && hit_capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  int rc = mem_hits_checks(ix, min_length, over);
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  hipStream_t st = static_cast<hipStream_t>(stream);
  if(nq == 0)
  {
    HIP_TRY(hipMemsetAsync(d_mem_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipStreamSynchronize(st));
    return GCSA2_OK;
  }
  return mem_hits_core(ix, d_patterns, d_offsets, nq, total_pattern_bytes, min_length, max_length, hit_max, over, d_mem_offsets, d_mems, mem_capacity,
                       total_mems, d_hit_offsets, d_hits, hit_capacity, total_hits, st);
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_mem_hits_device: ") + e.what()); }
}

int gcsa2_mem_hits_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t nq, uint64_t total_pattern_bytes,
                          uint64_t min_length, uint64_t hit_max, int over, uint64_t* d_mem_offsets, gcsa2_mem* d_mems, uint64_t mem_capacity,
                          uint64_t* total_mems, uint64_t* d_hit_offsets, uint64_t* d_hits, uint64_t hit_capacity, uint64_t* total_hits, void* stream)
{
  return gcsa2_mem_hits_bounded_device(ix, d_patterns, d_offsets, nq, total_pattern_bytes, min_length, 0, hit_max, over, d_mem_offsets, d_mems,
                                       mem_capacity, total_mems, d_hit_offsets, d_hits, hit_capacity, total_hits, stream);
}

// The host form: pieces of tune.ms_piece_bytes pattern bytes (a batch of two pieces' worth or more; one piece otherwise), each
// copied in, run through gcsa2_mem_hits_device and copied out behind the pieces before it.  A piece's device buffers are sized
// from the caller's remaining room (one piece) or an estimate (a piece that needs more runs again with the exact sizes); once
// the caller's room is exceeded the remaining pieces only count.  Every piece runs under the same max_length.
int gcsa2_mem_hits_bounded_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t nq, uint64_t min_length,
                                 uint64_t max_length, uint64_t hit_max, int over, uint64_t* mem_offsets, gcsa2_mem* mems, uint64_t mem_capacity,
                                 uint64_t* total_mems, uint64_t* hit_offsets, uint64_t* hits, uint64_t hit_capacity, uint64_t* total_hits)
{
  CHECK_INDEX(ix);
  CHECK_CAP(min_length, max_length);
  if(total_mems == nullptr || total_hits == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null total pointer"); }
  *total_mems = 0;
  *total_hits = 0;
  if(mem_offsets == nullptr || hit_offsets == nullptr || (offsets == nullptr && nq > 0) || (mems == nullptr && mem_capacity > 0) ||
     (hits == nullptr && hit_capacity > 0) || (nq > 0 && patterns == nullptr && offsets[nq] > offsets[0]))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  int rc = mem_hits_checks(ix, min_length, over);
  if(rc != GCSA2_OK) { return rc; }
  if(nq == 0) { mem_offsets[0] = 0; hit_offsets[0] = 0; return GCSA2_OK; }
  if(offsets[0] != 0 || !offsets_ok(offsets, nq)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "pattern offsets must start at 0 and be non-decreasing"); }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  const std::vector<u64> cut = read_cut(ix, offsets, nq);
  const u64 pieces = cut.size() - 1;
  DBuf<u8> d_pat; DBuf<u64> d_off, d_mem_off, d_hit_off, d_hits; DBuf<gcsa2_mem> d_mems;
  u64 mbase = 0, hbase = 0;
  bool exceeded = false;
  std::vector<u64> local;
  for(u64 c = 0; c < pieces; c++)
  {
    const u64 b = cut[c], count = cut[c + 1] - b, first = offsets[b], bytes = offsets[b + count] - first;
    rebase_piece(offsets, b, count, local);
    const u64 mem_room = exceeded ? 0 : mem_capacity - mbase, hit_room = exceeded ? 0 : hit_capacity - hbase;
    u64 rm = std::min(mem_room, pieces == 1 ? bytes + count : bytes / 8 + count + 1);
    u64 rh = (pieces == 1 ? hit_room : std::min(hit_room, 16 * rm));
    u64 m = 0, h = 0;
    for(int attempt = 0; attempt < 2; attempt++)
    {
      d_pat.release(); d_off.release(); d_mem_off.release(); d_mems.release(); d_hit_off.release(); d_hits.release();     // the piece before, the first attempt
      HIP_TRY(d_pat.alloc(bytes + 16));
      HIP_TRY(d_off.alloc(count + 1));
      HIP_TRY(d_mem_off.alloc(count + 1));
      HIP_TRY(d_mems.alloc(rm));
      HIP_TRY(d_hit_off.alloc(rm + 1));
      HIP_TRY(d_hits.alloc(rh));
      if(bytes > 0) { HIP_TRY(hipMemcpy(d_pat.p, patterns + first, bytes, hipMemcpyHostToDevice)); }
      HIP_TRY(hipMemcpy(d_off.p, local.data(), (count + 1) * sizeof(u64), hipMemcpyHostToDevice));
      rc = gcsa2_mem_hits_bounded_device(ix, d_pat.p, d_off.p, count, bytes, min_length, max_length, hit_max, over, d_mem_off.p, d_mems.p, rm, &m, d_hit_off.p, d_hits.p, rh, &h, nullptr);
      if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && attempt == 0 && m <= mem_room && h <= hit_room && (m > rm || h > rh)) { rm = m; rh = h; continue; }
      break;
    }
    if(rc == GCSA2_ERR_BUFFER_TOO_SMALL) { exceeded = true; }
    else if(rc != GCSA2_OK) { return rc; }
    else if(!exceeded)
    {
      HIP_TRY(hipMemcpy(local.data(), d_mem_off.p, (count + 1) * sizeof(u64), hipMemcpyDeviceToHost));
      for(u64 i = 0; i <= count; i++) { mem_offsets[b + i] = local[i] + mbase; }
      if(m > 0) { HIP_TRY(hipMemcpy(mems + mbase, d_mems.p, m * sizeof(gcsa2_mem), hipMemcpyDeviceToHost)); }
      local.resize(m + 1);
      HIP_TRY(hipMemcpy(local.data(), d_hit_off.p, (m + 1) * sizeof(u64), hipMemcpyDeviceToHost));
      for(u64 i = 0; i <= m; i++) { hit_offsets[mbase + i] = local[i] + hbase; }
      if(h > 0) { HIP_TRY(hipMemcpy(hits + hbase, d_hits.p, h * sizeof(u64), hipMemcpyDeviceToHost)); }
    }
    mbase += m;
    hbase += h;
  }
  *total_mems = mbase;
  *total_hits = hbase;
  if(exceeded || mbase > mem_capacity || hbase > hit_capacity)
  {
    return fail(GCSA2_ERR_BUFFER_TOO_SMALL, mbase > mem_capacity ? "MEM buffer too small" : "hit buffer too small");
  }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_mem_hits_batch: ") + e.what()); }
}

int gcsa2_mem_hits_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t nq, uint64_t min_length,
                         uint64_t hit_max, int over, uint64_t* mem_offsets, gcsa2_mem* mems, uint64_t mem_capacity, uint64_t* total_mems,
                         uint64_t* hit_offsets, uint64_t* hits, uint64_t hit_capacity, uint64_t* total_hits)
{
  return gcsa2_mem_hits_bounded_batch(ix, patterns, offsets, nq, min_length, 0, hit_max, over, mem_offsets, mems, mem_capacity, total_mems,
                                      hit_offsets, hits, hit_capacity, total_hits);
}

}  // extern "C"

// ==== sub-MEM reseeding: the shorter, more frequent matches inside long MEMs, with count() and locate() (kernels_submem.hpp) =====
namespace {

// gcsa2_sub_mem_hits_device after its argument checks (nq > 0, 0 < n_mems < 2^32).  Host round trips: the control words
// (bounds check, reseeded MEMs), the sub-MEM total with the overrun flag, those of the shared tail, the end.
int sub_mem_hits_core(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 nq, const u64* d_mem_offsets,
                      const gcsa2_mem* d_mems, u64 n_mems, u64 min_length, u64 reseed_length, u64 hit_max, int over, u64* d_sub_offsets,
                      gcsa2_mem* d_subs, u64 sub_capacity, u64* total_subs, u64* d_hit_offsets, u64* d_hits, u64 hit_capacity,
                      u64* total_hits, hipStream_t st)
{
  Scratch scratch(ix, st);
  const u64* mems = reinterpret_cast<const u64*>(d_mems);
  unsigned long long* ctl = nullptr;
  u64 *pid = nullptr, *sizes = nullptr, *sub_off = nullptr;
  u8* flag = nullptr;
  u32* work = nullptr;
  HIP_TRY(scratch.get(ctl, SUBMEM_CTL_WORDS));
  HIP_TRY(scratch.get(pid, n_mems));
  HIP_TRY(scratch.get(flag, n_mems));
  HIP_TRY(scratch.get(work, n_mems));
  HIP_TRY(scratch.get(sizes, n_mems + 1));
  HIP_TRY(scratch.get(sub_off, n_mems + 1));
  HIP_TRY(hipMemsetAsync(ctl, 0, SUBMEM_CTL_WORDS * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(sizes, 0, (n_mems + 1) * sizeof(u64), st));
  // 1. each MEM's pattern, the bounds check, the list of reseeded MEMs
  hipLaunchKernelGGL(k_submem_prep, dim3(grid_for(n_mems)), dim3(TPB), 0, st, d_offsets, nq, d_mem_offsets, mems, n_mems, reseed_length, pid, flag, ctl);
  LAUNCH_CHECK("k_submem_prep");
  size_t sel_bytes = 0;
  hipcub::CountingInputIterator<u32> items(0);
  HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, sel_bytes, items, flag, work, reinterpret_cast<u64*>(ctl + 2), size_t(n_mems), st));
  char* sel_tmp = nullptr;
  HIP_TRY(scratch.get(sel_tmp, sel_bytes));
  HIP_TRY(hipcub::DeviceSelect::Flagged(sel_tmp, sel_bytes, items, flag, work, reinterpret_cast<u64*>(ctl + 2), size_t(n_mems), st));
  unsigned long long words[SUBMEM_CTL_WORDS];
  HIP_TRY(hipMemcpyAsync(words, ctl, sizeof(words), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if(words[0] != 0) { scratch.settled = true; return fail(GCSA2_ERR_INVALID_ARGUMENT, "sub_mem_hits: a MEM reaches beyond its pattern (position + length > pattern length)"); }
  const u64 nr = (ix->img.n == 0 ? 0 : words[2]);
  // 2. the walk, counting; the CSR offsets; the walk again, writing (persistent lanes: what the device holds at once)
  const u64 resident = ix->tune.ms_grid != 0 ? ix->tune.ms_grid : u64(ix->compute_units) * 8;
  const unsigned grid = unsigned(std::max<u64>(1, std::min<u64>((nr + TPB2 - 1) / TPB2, resident)));
  if(nr > 0)
  {
    hipLaunchKernelGGL(k_submem_walk<false>, dim3(grid), dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, mems, pid, work, nr, min_length, ctl,
                       sizes, nullptr, nullptr, nullptr);
    LAUNCH_CHECK("k_submem_walk<count>");
  }
  size_t scan_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, sizes, sub_off, size_t(n_mems + 1), st));
  char* scan_tmp = nullptr;
  HIP_TRY(scratch.get(scan_tmp, scan_bytes));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, sizes, sub_off, size_t(n_mems + 1), st));
  u64 s = 0;
  HIP_TRY(hipMemcpyAsync(&s, sub_off + n_mems, sizeof(u64), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(words, ctl, sizeof(words), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if(words[1] != 0) { scratch.settled = true; return fail(GCSA2_ERR_HIP, "sub_mem_hits: a walk did not shorten its match (parent() returned an lcp >= the match length); the index is inconsistent"); }
  *total_subs = s;
  if(s >= (u64(1) << 32)) { scratch.settled = true; return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "sub_mem_hits: 2^32 or more sub-MEMs in one batch; split the batch"); }
  if(s == 0)
  {
    HIP_TRY(hipMemcpyAsync(d_sub_offsets, sub_off, (n_mems + 1) * sizeof(u64), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipStreamSynchronize(st));
    scratch.settled = true;
    return GCSA2_OK;
  }
  u64 *recs = nullptr, *counts = nullptr;
  HIP_TRY(scratch.get(recs, 4 * s));
  HIP_TRY(scratch.get(counts, s));
  HIP_TRY(hipMemsetAsync(ctl + 3, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_submem_walk<true>, dim3(grid), dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, mems, pid, work, nr, min_length, ctl,
                     nullptr, sub_off, recs, counts);
  LAUNCH_CHECK("k_submem_walk<write>");
  // 3. count class, locate, hits in sub-MEM order (mem_hits' tail); the offsets only once everything fits
  const int rc = mem_hits_tail(ix, recs, counts, s, hit_max, over, d_subs, sub_capacity, d_hit_offsets, d_hits, hit_capacity, total_hits, scratch, st);
  if(rc != GCSA2_OK) { return rc; }
  scratch.settled = false;
  HIP_TRY(hipMemcpyAsync(d_sub_offsets, sub_off, (n_mems + 1) * sizeof(u64), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  scratch.settled = true;
  return GCSA2_OK;
}

}  // namespace

extern "C" {

int gcsa2_sub_mem_hits_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t nq, uint64_t total_pattern_bytes,
                              const uint64_t* d_mem_offsets, const gcsa2_mem* d_mems, uint64_t n_mems, uint64_t min_length, uint64_t reseed_length,
                              uint64_t hit_max, int over, uint64_t* d_sub_offsets, gcsa2_mem* d_subs, uint64_t sub_capacity, uint64_t* total_subs,
                              uint64_t* d_hit_offsets, uint64_t* d_hits, uint64_t hit_capacity, uint64_t* total_hits, void* stream)
{
  (void)total_pattern_bytes;
  CHECK_INDEX(ix);
  if(total_subs == nullptr || total_hits == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null total pointer"); }
  *total_subs = 0;
  *total_hits = 0;
  if(d_sub_offsets == nullptr || d_hit_offsets == nullptr || (nq > 0 && (d_offsets == nullptr || d_mem_offsets == nullptr)) ||
     (d_subs == nullptr && sub_capacity > 0) || (d_hits == nullptr && hit_capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  int rc = mem_hits_checks(ix, min_length, over);
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  hipStream_t st = static_cast<hipStream_t>(stream);
  if(nq > 0 && n_mems == GCSA2_UNKNOWN)
  {
    HIP_TRY(hipMemcpyAsync(&n_mems, d_mem_offsets + nq, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  if(nq == 0 || n_mems == 0 || n_mems == GCSA2_UNKNOWN)
  {
    HIP_TRY(hipMemsetAsync(d_sub_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipStreamSynchronize(st));
    return GCSA2_OK;
  }
  if(d_mems == nullptr || d_patterns == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  if(n_mems >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "sub_mem_hits: 2^32 or more MEMs in one batch; split the batch"); }
  return sub_mem_hits_core(ix, d_patterns, d_offsets, nq, d_mem_offsets, d_mems, n_mems, min_length, reseed_length, hit_max, over, d_sub_offsets,
                           d_subs, sub_capacity, total_subs, d_hit_offsets, d_hits, hit_capacity, total_hits, st);
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_sub_mem_hits_device: ") + e.what()); }
}

// The host form, in one piece: patterns, offsets, MEM offsets and MEMs copied in, gcsa2_sub_mem_hits_device on buffers of the
// caller's capacities, the results copied out.  The whole batch and both capacities must fit in device memory at once.
int gcsa2_sub_mem_hits_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t nq, const uint64_t* mem_offsets,
                             const gcsa2_mem* mems, uint64_t n_mems, uint64_t min_length, uint64_t reseed_length, uint64_t hit_max, int over,
                             uint64_t* sub_offsets, gcsa2_mem* subs, uint64_t sub_capacity, uint64_t* total_subs,
                             uint64_t* hit_offsets, uint64_t* hits, uint64_t hit_capacity, uint64_t* total_hits)
{
  CHECK_INDEX(ix);
  if(total_subs == nullptr || total_hits == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null total pointer"); }
  *total_subs = 0;
  *total_hits = 0;
  if(sub_offsets == nullptr || hit_offsets == nullptr || (nq > 0 && (offsets == nullptr || mem_offsets == nullptr)) ||
     (subs == nullptr && sub_capacity > 0) || (hits == nullptr && hit_capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  int rc = mem_hits_checks(ix, min_length, over);
  if(rc != GCSA2_OK) { return rc; }
  if(nq > 0 && n_mems == GCSA2_UNKNOWN) { n_mems = mem_offsets[nq]; }
  if(nq == 0 || n_mems == 0) { sub_offsets[0] = 0; hit_offsets[0] = 0; return GCSA2_OK; }
  if(offsets[0] != 0 || !offsets_ok(offsets, nq)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "pattern offsets must start at 0 and be non-decreasing"); }
  if(mem_offsets[0] != 0 || !offsets_ok(mem_offsets, nq) || mem_offsets[nq] != n_mems)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "MEM offsets must start at 0, be non-decreasing and end at n_mems");
  }
  if(mems == nullptr || (patterns == nullptr && offsets[nq] > 0)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  DBuf<u8> d_pat; DBuf<u64> d_off, d_mem_off, d_sub_off, d_hit_off, d_hits; DBuf<gcsa2_mem> d_mems, d_subs;
  const u64 bytes = offsets[nq];
  HIP_TRY(d_pat.alloc(bytes + 16));
  HIP_TRY(d_off.alloc(nq + 1));
  HIP_TRY(d_mem_off.alloc(nq + 1));
  HIP_TRY(d_mems.alloc(n_mems));
  HIP_TRY(d_sub_off.alloc(n_mems + 1));
  HIP_TRY(d_subs.alloc(sub_capacity));
  HIP_TRY(d_hit_off.alloc(sub_capacity + 1));
  HIP_TRY(d_hits.alloc(hit_capacity));
  if(bytes > 0) { HIP_TRY(hipMemcpy(d_pat.p, patterns, bytes, hipMemcpyHostToDevice)); }
  HIP_TRY(hipMemcpy(d_off.p, offsets, (nq + 1) * sizeof(u64), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_mem_off.p, mem_offsets, (nq + 1) * sizeof(u64), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_mems.p, mems, n_mems * sizeof(gcsa2_mem), hipMemcpyHostToDevice));
  rc = gcsa2_sub_mem_hits_device(ix, d_pat.p, d_off.p, nq, bytes, d_mem_off.p, d_mems.p, n_mems, min_length, reseed_length, hit_max, over,
                                 d_sub_off.p, d_subs.p, sub_capacity, total_subs, d_hit_off.p, d_hits.p, hit_capacity, total_hits, nullptr);
  if(rc != GCSA2_OK) { return rc; }
  const u64 s = *total_subs, h = *total_hits;
  HIP_TRY(hipMemcpy(sub_offsets, d_sub_off.p, (n_mems + 1) * sizeof(u64), hipMemcpyDeviceToHost));
  if(s > 0) { HIP_TRY(hipMemcpy(subs, d_subs.p, s * sizeof(gcsa2_mem), hipMemcpyDeviceToHost)); }
  HIP_TRY(hipMemcpy(hit_offsets, d_hit_off.p, (s + 1) * sizeof(u64), hipMemcpyDeviceToHost));
  if(h > 0) { HIP_TRY(hipMemcpy(hits, d_hits.p, h * sizeof(u64), hipMemcpyDeviceToHost)); }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_sub_mem_hits_batch: ") + e.what()); }
}

}  // extern "C"

// ==== k-mer windows: find() / count() of every window of every read, per-read profiles (kernels_windows.hpp) ================
namespace {

// what both forms refuse before any device is touched, then the one component the call may need
int kmer_windows_checks(const gcsa2_index* ix, u64 k, u64 stride, int flags, const void* counts, const u64* total_windows)
{
  CHECK_INDEX(ix);
  if(total_windows == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null total pointer"); }
  if(k == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_windows: k must be at least 1"); }
  if(stride == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_windows: stride must be at least 1"); }
  if((flags & ~GCSA2_KMER_COUNTS) != 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_windows: unknown flag"); }
  if(counts != nullptr && (flags & GCSA2_KMER_COUNTS) == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_windows: a counts buffer needs GCSA2_KMER_COUNTS"); }
  if((flags & GCSA2_KMER_COUNTS) != 0 && !ix->img.has_counters) { return fail(GCSA2_ERR_MISSING_COMPONENT, "index was created without counters"); }
  return GCSA2_OK;
}

// How every k-mer call begins: where each read's windows start (n_patterns + 1 entries, in `woff_or_null` or in scratch) and,
// after one host round trip, their number.  The stream is idle when this returns without a HIP error; a call of 2^32 or
// more windows is refused in `name`, with `total` set.
int window_plan(Scratch& scratch, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 stride, u64* woff_or_null, const char* name, hipStream_t st,
                u64*& woff, u64& total)
{
  u64* sizes = nullptr;
  char* scan_tmp = nullptr;
  woff = woff_or_null;
  HIP_TRY(scratch.get(sizes, n_patterns + 1));
  if(woff == nullptr) { HIP_TRY(scratch.get(woff, n_patterns + 1)); }
  hipLaunchKernelGGL(k_window_counts, dim3(grid_for(n_patterns + 1)), dim3(TPB), 0, st, d_offsets, n_patterns, k, stride, sizes);
  LAUNCH_CHECK("k_window_counts");
  size_t scan_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, sizes, woff, size_t(n_patterns + 1), st));
  HIP_TRY(scratch.get(scan_tmp, scan_bytes));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, sizes, woff, size_t(n_patterns + 1), st));
  HIP_TRY(hipMemcpyAsync(&total, woff + n_patterns, sizeof(u64), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if(total >= (u64(1) << 32))
  {
    scratch.settled = true;
    return fail(GCSA2_ERR_BUFFER_TOO_SMALL, std::string(name) + ": 2^32 or more windows in one call; split the batch");
  }
  return GCSA2_OK;
}

// gcsa2_kmer_windows_device after its argument checks (n_patterns > 0).  One host round trip: the number of windows.
int kmer_windows_core(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 stride, int flags,
                      u64* d_window_offsets, gcsa2_kmer_profile* d_profiles, u64* d_ranges, u64* d_counts, u64 capacity, u64* total_windows,
                      hipStream_t st)
{
  Scratch scratch(ix, st);
  u64 *woff = nullptr, total = 0;
  const int rc = window_plan(scratch, d_offsets, n_patterns, k, stride, d_window_offsets, "kmer_windows", st, woff, total);
  *total_windows = total;
  if(rc != GCSA2_OK) { return rc; }
  scratch.settled = true;
  if((d_ranges != nullptr || d_counts != nullptr) && total > capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "window buffer too small"); }
  if(d_profiles == nullptr && d_ranges == nullptr && d_counts == nullptr) { return GCSA2_OK; }
  scratch.settled = false;
  static_assert(sizeof(gcsa2_kmer_profile) == 32, "four u64");
  if(d_profiles != nullptr) { HIP_TRY(hipMemsetAsync(d_profiles, 0, n_patterns * sizeof(gcsa2_kmer_profile), st)); }
  if(total > 0)
  {
    const dim3 grid(unsigned((total + TPB2 - 1) / TPB2));
    const bool pair = ix->img.flp != nullptr, count = (flags & GCSA2_KMER_COUNTS) != 0 && (d_counts != nullptr || d_profiles != nullptr);
    // the reads of every wavefront's first window: the bracket in which a lane looks for its own read
    const u64 spans = (total + OWNER_SPAN - 1) / OWNER_SPAN;
    u64* owners = nullptr;
    HIP_TRY(scratch.get(owners, spans + 1));
    hipLaunchKernelGGL(k_block_owners, dim3(grid_for(spans + 1)), dim3(TPB), 0, st, woff, n_patterns, total, OWNER_SPAN, spans, owners);
    LAUNCH_CHECK("k_block_owners");
#define KMER_WINDOWS_LAUNCH(P, C) hipLaunchKernelGGL((k_kmer_windows<P, C>), grid, dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, k, stride, \
                                                     woff, owners, total, d_ranges, d_counts, d_profiles)
    if(pair) { if(count) { KMER_WINDOWS_LAUNCH(true, true); } else { KMER_WINDOWS_LAUNCH(true, false); } }
    else { if(count) { KMER_WINDOWS_LAUNCH(false, true); } else { KMER_WINDOWS_LAUNCH(false, false); } }
#undef KMER_WINDOWS_LAUNCH
    LAUNCH_CHECK("k_kmer_windows");
  }
  HIP_TRY(hipStreamSynchronize(st));
  scratch.settled = true;
  return GCSA2_OK;
}

// The k-mer seed search over the windows of window_plan (total > 0): the found windows as seed records with their count()s, in
// arrival order, in an area of `capacity` records; `m`: how many were found, to which the caller reacts if the area was
// short.  attempts == 2 (capacity is a caller's guess): a short area is re-made at m and the search runs again, so each
// run zeroes what it left behind (`prof`, found[spans]) and the area is taken after the owners are on their way; attempts ==
// 1 (capacity == total): the area first, one run.  One host round trip per run.
// `mins` (gcsa2_minimizer_hits_device): the windows are those of this list, woff its offsets per read; `stride` is not used.
// `wins` (gcsa2_stranded_minimizer_hits_device): the windows are the {key, position} entries of this list, woff its offsets per
// group; the patterns are not read.
int kmer_seed_search(const gcsa2_index* ix, Scratch& scratch, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 stride,
                     const u64* woff, u64 total, u64 capacity, gcsa2_kmer_profile* prof, int attempts, hipStream_t st, SeedEmit& emit, u64& m,
                     const gcsa2_minimizer* mins = nullptr, const ulonglong2* wins = nullptr)
{
  const u64 spans = (total + OWNER_SPAN - 1) / OWNER_SPAN;
  static_assert(OWNER_SPAN == 64, "one SeedEmit entry per wavefront of the search");
  u64* owners = nullptr;
  emit = SeedEmit{};
  HIP_TRY(scratch.get(owners, spans + 1));
  HIP_TRY(scratch.get(emit.cursor, 1));
  HIP_TRY(scratch.get(emit.base, spans));
  HIP_TRY(scratch.get(emit.found, spans + 1));
  HIP_TRY(scratch.get(emit.mask, spans));
  // the reads of every wavefront's first window: the bracket in which a lane looks for its own read
  auto block_owners = [&]() -> int
  {
    scratch.settled = false;
    hipLaunchKernelGGL(k_block_owners, dim3(grid_for(spans + 1)), dim3(TPB), 0, st, woff, n_patterns, total, OWNER_SPAN, spans, owners);
    LAUNCH_CHECK("k_block_owners");
    return GCSA2_OK;
  };
  const bool rerun = attempts > 1;
  if(rerun) { const int rc = block_owners(); if(rc != GCSA2_OK) { return rc; } }
  const dim3 grid(unsigned((total + TPB2 - 1) / TPB2));
  emit.capacity = capacity;
  for(int attempt = 0; attempt < attempts; attempt++)
  {
    HIP_TRY(scratch.get(emit.recs, 4 * emit.capacity));
    HIP_TRY(scratch.get(emit.counts, emit.capacity));
    if(!rerun) { const int rc = block_owners(); if(rc != GCSA2_OK) { return rc; } }
    HIP_TRY(hipMemsetAsync(emit.cursor, 0, sizeof(unsigned long long), st));
    if(rerun) { HIP_TRY(hipMemsetAsync(emit.found + spans, 0, sizeof(u32), st)); }
    if(prof != nullptr) { HIP_TRY(hipMemsetAsync(prof, 0, n_patterns * sizeof(gcsa2_kmer_profile), st)); }
    if(wins != nullptr)
    {
      if(ix->img.flp != nullptr) { hipLaunchKernelGGL((k_strand_seeds<true>), grid, dim3(TPB2), 0, st, ix->img, k, wins, woff, owners, total, prof, emit); }
      else { hipLaunchKernelGGL((k_strand_seeds<false>), grid, dim3(TPB2), 0, st, ix->img, k, wins, woff, owners, total, prof, emit); }
    }
    else if(mins != nullptr)
    {
      if(ix->img.flp != nullptr) { hipLaunchKernelGGL((k_minimizer_seeds<true>), grid, dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, k, mins, woff, owners, total, prof, emit); }
      else { hipLaunchKernelGGL((k_minimizer_seeds<false>), grid, dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, k, mins, woff, owners, total, prof, emit); }
    }
    else if(ix->img.flp != nullptr) { hipLaunchKernelGGL((k_kmer_seeds<true>), grid, dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, k, stride, woff, owners, total, prof, emit); }
    else { hipLaunchKernelGGL((k_kmer_seeds<false>), grid, dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, k, stride, woff, owners, total, prof, emit); }
    LAUNCH_CHECK("k_kmer_seeds");
    HIP_TRY(hipMemcpyAsync(&m, emit.cursor, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if(m <= emit.capacity) { break; }
    if(attempt + 1 < attempts) { emit.capacity = m; }        // the records are still needed, for the totals
  }
  return GCSA2_OK;
}

}  // namespace

extern "C" {

int gcsa2_kmer_windows_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k,
                              uint64_t stride, int flags, uint64_t* d_window_offsets, gcsa2_kmer_profile* d_profiles, uint64_t* d_ranges,
                              uint64_t* d_counts, uint64_t capacity, uint64_t* total_windows, void* stream)
{
  int rc = kmer_windows_checks(ix, k, stride, flags, d_counts, total_windows);
  if(rc != GCSA2_OK) { return rc; }
  *total_windows = 0;
  if(n_patterns > 0 && d_offsets == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "kmer_windows: 2^32 or more reads in one call; split the batch"); }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  hipStream_t st = static_cast<hipStream_t>(stream);
  if(n_patterns == 0)
  {
    if(d_window_offsets != nullptr)
    {
      HIP_TRY(hipMemsetAsync(d_window_offsets, 0, sizeof(u64), st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    return GCSA2_OK;
  }
  return kmer_windows_core(ix, d_patterns, d_offsets, n_patterns, k, stride, flags, d_window_offsets, d_profiles, d_ranges, d_counts, capacity,
                           total_windows, st);
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_kmer_windows_device: ") + e.what()); }
}

// The host form.  The window offsets are a function of the pattern offsets alone, so they -- and the total, and the refusal of
// a short buffer -- are worked out here before any device work.  A piece (for_read_pieces) travels through a Lease, which
// brings its own stream: reads and their rebased offsets in, gcsa2_kmer_windows_device with the window offsets left in
// scratch, then the piece's profiles / ranges / counts out to their places in the caller's arrays, which the host-side
// offsets name.  With profiles as the only output that is the reads in and 32 bytes per read out.
int gcsa2_kmer_windows_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k,
                             uint64_t stride, int flags, uint64_t* window_offsets, gcsa2_kmer_profile* profiles, uint64_t* ranges,
                             uint64_t* counts, uint64_t capacity, uint64_t* total_windows)
{
  int rc = kmer_windows_checks(ix, k, stride, flags, counts, total_windows);
  if(rc != GCSA2_OK) { return rc; }
  *total_windows = 0;
  if(n_patterns == 0) { if(window_offsets != nullptr) { window_offsets[0] = 0; } return GCSA2_OK; }
  if(offsets == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer"); }
  rc = reads_ok(patterns, offsets, n_patterns, nullptr);
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  g_error.clear();
  std::vector<u64> woff(n_patterns + 1);
  const u64 total = host_windows(offsets, n_patterns, k, stride, woff.data());
  *total_windows = total;
  if((ranges != nullptr || counts != nullptr) && total > capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "window buffer too small"); }
  if(window_offsets != nullptr) { std::memcpy(window_offsets, woff.data(), (n_patterns + 1) * sizeof(u64)); }
  if(profiles == nullptr && ranges == nullptr && counts == nullptr) { return GCSA2_OK; }
  return for_read_pieces(ix, offsets, read_cut(ix, offsets, n_patterns), [&](const ReadPiece& p, Outcome& out) -> bool
  {
    const u64 at = woff[p.b], windows = woff[p.b + p.count] - at;
    Lease lease(ix);
    hipError_t e = lease.begin(Lease::need(p.bytes + 16) + Lease::need((p.count + 1) * 8) + (profiles != nullptr ? Lease::need(p.count * 32) : 0) +
                               (ranges != nullptr ? Lease::need(windows * 16) : 0) + (counts != nullptr ? Lease::need(windows * 8) : 0));
    if(e != hipSuccess) { out.set(GCSA2_ERR_OUT_OF_MEMORY, std::string("staging of a piece: ") + hipGetErrorString(e)); return false; }
    u8* d_pat = lease.dev<u8>(p.bytes + 16); u64* d_off = lease.dev<u64>(p.count + 1);
    gcsa2_kmer_profile* d_prof = (profiles != nullptr ? lease.dev<gcsa2_kmer_profile>(p.count) : nullptr);
    u64* d_rng = (ranges != nullptr ? lease.dev<u64>(2 * windows) : nullptr);
    u64* d_cnt = (counts != nullptr ? lease.dev<u64>(windows) : nullptr);
    e = lease.up(d_pat, patterns + p.first, p.bytes);
    if(e == hipSuccess) { e = lease.up(d_off, p.local, (p.count + 1) * sizeof(u64)); }
    if(e != hipSuccess) { out.hip_error("upload of a piece", e); return false; }
    u64 got = 0;
    const int piece_rc = gcsa2_kmer_windows_device(ix, d_pat, d_off, p.count, k, stride, flags, nullptr, d_prof, d_rng, d_cnt, windows, &got, lease.stream());
    if(piece_rc != GCSA2_OK) { out.set(piece_rc, g_error); return false; }
    if(profiles != nullptr) { e = lease.down(profiles + p.b, d_prof, p.count * sizeof(gcsa2_kmer_profile)); }
    if(e == hipSuccess && ranges != nullptr) { e = lease.down(ranges + 2 * at, d_rng, 2 * windows * sizeof(u64)); }
    if(e == hipSuccess && counts != nullptr) { e = lease.down(counts + at, d_cnt, windows * sizeof(u64)); }
    if(e == hipSuccess) { e = lease.finish(); }
    if(e != hipSuccess) { out.hip_error("download of a piece", e); return false; }
    return true;
  }, false);
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_kmer_windows_batch: ") + e.what()); }
}

}  // extern "C"

// ==== k-mer hits: the found windows of every read as seeds with count() and locate() (kernels_windows.hpp, kernels_mem.hpp) ====
namespace {

// what both forms refuse before any device is touched, then the components the call needs (no LCP array)
int kmer_hits_checks(const gcsa2_index* ix, u64 k, u64 stride, int over, const u64* total_seeds, const u64* total_hits)
{
  CHECK_INDEX(ix);
  if(total_seeds == nullptr || total_hits == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null total pointer"); }
  if(k == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_hits: k must be at least 1"); }
  if(stride == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_hits: stride must be at least 1"); }
  if(over != GCSA2_MEM_OVER_SKIP && over != GCSA2_MEM_OVER_SAMPLE)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_hits: unknown over-cap policy (GCSA2_MEM_OVER_SKIP or GCSA2_MEM_OVER_SAMPLE)");
  }
  return locate_checks(ix, 0);
}

// gcsa2_kmer_hits_device after its argument checks (0 < n_patterns < 2^32).  Host round trips: the number of windows, the
// number of seeds (twice when the arrival area was too small for them), those of the shared tail, the end.
// Scratch: per read the window offsets and, if asked for, the profiles (the caller's only once everything fits); per 64
// windows the owner entry and 16 bytes of SeedEmit; the rest per seed.
// kmer_hits_found is everything behind the plan of the windows: `total` windows with the offsets `woff` per read, at j stride
// or, with `mins` (gcsa2_minimizer_hits_device), at the positions of that list, or, with `wins`
// (gcsa2_stranded_minimizer_hits_device), the keys of that list: the "reads" are then its groups.
int kmer_hits_found(const gcsa2_index* ix, Scratch& scratch, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 stride,
                    const u64* woff, u64 total, const gcsa2_minimizer* mins, u64 hit_max, int over,
                    gcsa2_kmer_profile* d_profiles, u64* d_seed_offsets, gcsa2_mem* d_seeds, u64 seed_capacity, u64* total_seeds,
                    u64* d_hit_offsets, u64* d_hits, u64 hit_capacity, u64* total_hits, hipStream_t st, const ulonglong2* wins = nullptr)
{
  int rc = GCSA2_OK;
  // no seed: zeroed offsets, the profiles are their window numbers
  auto nothing_found = [&](const gcsa2_kmer_profile* prof) -> int
  {
    HIP_TRY(hipMemsetAsync(d_seed_offsets, 0, (n_patterns + 1) * sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, sizeof(u64), st));
    if(d_profiles != nullptr)
    {
      if(prof != nullptr) { HIP_TRY(hipMemcpyAsync(d_profiles, prof, n_patterns * sizeof(gcsa2_kmer_profile), hipMemcpyDeviceToDevice, st)); }
      else { HIP_TRY(hipMemsetAsync(d_profiles, 0, n_patterns * sizeof(gcsa2_kmer_profile), st)); }
    }
    HIP_TRY(hipStreamSynchronize(st));
    scratch.settled = true;
    return GCSA2_OK;
  };
  if(total == 0) { return nothing_found(nullptr); }
  // 1. the search: seed records in arrival order, the profiles in scratch
  const u64 spans = (total + OWNER_SPAN - 1) / OWNER_SPAN;
  gcsa2_kmer_profile* prof = nullptr;
  SeedEmit emit{};
  u64 m = 0;
  if(d_profiles != nullptr) { HIP_TRY(scratch.get(prof, n_patterns)); }
  rc = kmer_seed_search(ix, scratch, d_patterns, d_offsets, n_patterns, k, stride, woff, total, std::min(seed_capacity, total), prof, 2, st, emit, m, mins, wins);
  if(rc != GCSA2_OK) { return rc; }
  if(m > emit.capacity) { scratch.settled = true; return fail(GCSA2_ERR_HIP, "kmer_hits: two runs of the search disagree on the number of seeds"); }
  *total_seeds = m;
  if(m == 0) { return nothing_found(prof); }
  // 2. window order: the scan of the wavefronts' found numbers, then every wavefront's records to their place
  u64 *recs = nullptr, *counts = nullptr;
  size_t scan_bytes = 0;
  char* scan_tmp = nullptr;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, emit.found, emit.found, size_t(spans + 1), st));
  HIP_TRY(scratch.get(scan_tmp, scan_bytes));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, emit.found, emit.found, size_t(spans + 1), st));
  HIP_TRY(scratch.get(recs, 4 * m));
  HIP_TRY(scratch.get(counts, m));
  hipLaunchKernelGGL(k_seed_place, dim3(grid_for(spans * 64)), dim3(TPB), 0, st, emit.base, emit.found, spans, emit.recs, emit.counts, recs, counts);
  LAUNCH_CHECK("k_seed_place");
  // 3. count class, locate, hits in seed order (mem_hits' tail); offsets and profiles only once everything fits
  rc = mem_hits_tail(ix, recs, counts, m, hit_max, over, d_seeds, seed_capacity, d_hit_offsets, d_hits, hit_capacity, total_hits, scratch, st);
  if(rc != GCSA2_OK) { return rc; }
  scratch.settled = false;
  hipLaunchKernelGGL(k_seed_offsets, dim3(grid_for(n_patterns + 1)), dim3(TPB), 0, st, woff, n_patterns, total, spans, emit.found, emit.mask, d_seed_offsets);
  LAUNCH_CHECK("k_seed_offsets");
  if(d_profiles != nullptr) { HIP_TRY(hipMemcpyAsync(d_profiles, prof, n_patterns * sizeof(gcsa2_kmer_profile), hipMemcpyDeviceToDevice, st)); }
  HIP_TRY(hipStreamSynchronize(st));
  scratch.settled = true;
  return GCSA2_OK;
}

int kmer_hits_core(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 stride, u64 hit_max, int over,
                   gcsa2_kmer_profile* d_profiles, u64* d_seed_offsets, gcsa2_mem* d_seeds, u64 seed_capacity, u64* total_seeds,
                   u64* d_hit_offsets, u64* d_hits, u64 hit_capacity, u64* total_hits, hipStream_t st)
{
  Scratch scratch(ix, st);
  u64 *woff = nullptr, total = 0;
  const int rc = window_plan(scratch, d_offsets, n_patterns, k, stride, nullptr, "kmer_hits", st, woff, total);
  if(rc != GCSA2_OK) { return rc; }
  return kmer_hits_found(ix, scratch, d_patterns, d_offsets, n_patterns, k, stride, woff, total, nullptr, hit_max, over, d_profiles, d_seed_offsets, d_seeds,
                         seed_capacity, total_seeds, d_hit_offsets, d_hits, hit_capacity, total_hits, st);
}

}  // namespace

extern "C" {

int gcsa2_kmer_hits_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k,
                           uint64_t stride, uint64_t hit_max, int over, gcsa2_kmer_profile* d_profiles, uint64_t* d_seed_offsets,
                           gcsa2_mem* d_seeds, uint64_t seed_capacity, uint64_t* total_seeds, uint64_t* d_hit_offsets, uint64_t* d_hits,
                           uint64_t hit_capacity, uint64_t* total_hits, void* stream)
{
  int rc = kmer_hits_checks(ix, k, stride, over, total_seeds, total_hits);
  if(rc != GCSA2_OK) { return rc; }
  *total_seeds = 0;
  *total_hits = 0;
  if(d_seed_offsets == nullptr || d_hit_offsets == nullptr || (n_patterns > 0 && d_offsets == nullptr) || (d_seeds == nullptr && seed_capacity > 0) ||
     (d_hits == nullptr && hit_capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "kmer_hits: 2^32 or more reads in one call; split the batch"); }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  hipStream_t st = static_cast<hipStream_t>(stream);
  if(n_patterns == 0)
  {
    HIP_TRY(hipMemsetAsync(d_seed_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipStreamSynchronize(st));
    return GCSA2_OK;
  }
  return kmer_hits_core(ix, d_patterns, d_offsets, n_patterns, k, stride, hit_max, over, d_profiles, d_seed_offsets, d_seeds, seed_capacity, total_seeds,
                        d_hit_offsets, d_hits, hit_capacity, total_hits, st);
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_kmer_hits_device: ") + e.what()); }
}

// The host form (seed_pieces_batch).  Its own: the window count refused before any device work, a first run with room for
// every window, and the profiles as the per-read output.
int gcsa2_kmer_hits_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k,
                          uint64_t stride, uint64_t hit_max, int over, gcsa2_kmer_profile* profiles, uint64_t* seed_offsets,
                          gcsa2_mem* seeds, uint64_t seed_capacity, uint64_t* total_seeds, uint64_t* hit_offsets, uint64_t* hits,
                          uint64_t hit_capacity, uint64_t* total_hits)
{
  int rc = kmer_hits_checks(ix, k, stride, over, total_seeds, total_hits);
  if(rc != GCSA2_OK) { return rc; }
  *total_seeds = 0;
  *total_hits = 0;
  if(seed_offsets == nullptr || hit_offsets == nullptr || (n_patterns > 0 && offsets == nullptr) || (seeds == nullptr && seed_capacity > 0) ||
     (hits == nullptr && hit_capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "kmer_hits: 2^32 or more reads in one call; split the batch"); }
  if(n_patterns == 0) { seed_offsets[0] = 0; hit_offsets[0] = 0; return GCSA2_OK; }
  rc = reads_ok(patterns, offsets, n_patterns, nullptr);
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  g_error.clear();
  if(host_windows(offsets, n_patterns, k, stride) >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "kmer_hits: 2^32 or more windows in one call; split the batch"); }
  // several pieces: room for every window, so that the search runs once, and an estimate of the hits
  auto estimate = [&](const ReadPiece& p) -> std::pair<u64, u64>
  {
    const u64 windows = host_windows(p.local, p.count, k, stride);
    if(p.pieces == 1) { return {std::min(seed_capacity, windows), hit_capacity}; }
    return {windows, 4 * windows};
  };
  auto run = [&](const ReadPiece& p, const u8* d_pat, const u64* d_off, u8* d_prof, u64* d_seed_off, gcsa2_mem* d_seeds, u64 rm, u64* m, u64* d_hit_off,
                 u64* d_hits, u64 rh, u64* h) -> int
  {
    return gcsa2_kmer_hits_device(ix, d_pat, d_off, p.count, k, stride, hit_max, over, reinterpret_cast<gcsa2_kmer_profile*>(d_prof), d_seed_off, d_seeds, rm, m,
                                  d_hit_off, d_hits, rh, h, p.stream);
  };
  return seed_pieces_batch(ix, patterns, offsets, n_patterns, estimate, run, sizeof(gcsa2_kmer_profile), profiles, seed_offsets, seeds, seed_capacity,
                           total_seeds, hit_offsets, hits, hit_capacity, total_hits);
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_kmer_hits_batch: ") + e.what()); }
}

}  // extern "C"

// ==== minimizers: the (w, k)-minimizers of every read, alone and as the windows of the k-mer hits (kernels_minimizers.hpp) ====
namespace {

// what all four forms refuse before any device is touched
int minimizers_checks(const gcsa2_index* ix, u64 k, u64 w, const u64* total)
{
  CHECK_INDEX(ix);
  if(total == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null total pointer"); }
  if(k == 0 || k > GCSA2_MINIMIZER_MAX_K) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "minimizers: k must be 1 .. 32"); }
  if(w == 0 || w > GCSA2_MINIMIZER_MAX_W) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "minimizers: w must be 1 .. 64"); }
  return GCSA2_OK;
}

// then the over-cap policy and the components the hits need (no LCP array)
int minimizer_hits_checks(const gcsa2_index* ix, u64 k, u64 w, int over, const u64* total_seeds, const u64* total_hits)
{
  const int rc = minimizers_checks(ix, k, w, total_seeds);
  if(rc != GCSA2_OK) { return rc; }
  if(total_hits == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null total pointer"); }
  if(over != GCSA2_MEM_OVER_SKIP && over != GCSA2_MEM_OVER_SAMPLE)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "minimizer_hits: unknown over-cap policy (GCSA2_MEM_OVER_SKIP or GCSA2_MEM_OVER_SAMPLE)");
  }
  return locate_checks(ix, 0);
}

// The selection (0 < n_patterns < 2^32): a counting pass, the scan into the offsets (n_patterns + 1 entries, in `moff_or_null` or in
// scratch), one host round trip for the number of minimizers and of stride-1 windows, then the same pass again placing the
// records -- into scratch (to_scratch), or into `out` if they fit in `capacity` (else GCSA2_ERR_BUFFER_TOO_SMALL with the
// offsets complete and no record written).  The stream is idle when this returns a refusal; after the placing pass it is not.
// Rec: gcsa2_minimizer, or gcsa2_canonical_minimizer for the canonical selection (k_canonical_minimizers).
template<class Rec>
int minimizer_select(const gcsa2_index* ix, Scratch& scratch, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 w,
                     u64 hash_seed, u64* moff_or_null, bool to_scratch, typename std::common_type<Rec*>::type out, u64 capacity, const char* name,
                     hipStream_t st, u64*& moff, Rec*& mins, u64& total)
{
  constexpr bool CANONICAL = std::is_same<Rec, gcsa2_canonical_minimizer>::value;
  u64 *sizes = nullptr, *windows = nullptr;
  char *scan_tmp = nullptr, *sum_tmp = nullptr;
  moff = moff_or_null;
  mins = out;
  total = 0;
  HIP_TRY(scratch.get(sizes, n_patterns + 1));
  HIP_TRY(scratch.get(windows, 1));
  if(moff == nullptr) { HIP_TRY(scratch.get(moff, n_patterns + 1)); }
  const dim3 grid(unsigned(std::min<u64>(n_patterns, u64(1) << 20)));
  if constexpr(CANONICAL)
  {
    hipLaunchKernelGGL((k_canonical_minimizers<false>), grid, dim3(MINI_TPB), 0, st, ix->img, d_patterns, d_offsets, n_patterns, u32(k), u32(w), hash_seed,
                       sizes, static_cast<const u64*>(nullptr), static_cast<Rec*>(nullptr));
  }
  else
  {
    hipLaunchKernelGGL((k_minimizers<false>), grid, dim3(MINI_TPB), 0, st, ix->img, d_patterns, d_offsets, n_patterns, u32(k), u32(w), hash_seed, sizes,
                       static_cast<const u64*>(nullptr), static_cast<Rec*>(nullptr));
  }
  LAUNCH_CHECK("k_minimizers");
  size_t scan_bytes = 0, sum_bytes = 0;
  hipcub::TransformInputIterator<u64, MiniWindowsOf, hipcub::CountingInputIterator<u64>> per_read(hipcub::CountingInputIterator<u64>(0), MiniWindowsOf{d_offsets, k});
  HIP_TRY(hipcub::DeviceReduce::Sum(nullptr, sum_bytes, per_read, windows, size_t(n_patterns), st));
  HIP_TRY(scratch.get(sum_tmp, sum_bytes));
  HIP_TRY(hipcub::DeviceReduce::Sum(sum_tmp, sum_bytes, per_read, windows, size_t(n_patterns), st));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, sizes, moff, size_t(n_patterns + 1), st));
  HIP_TRY(scratch.get(scan_tmp, scan_bytes));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, sizes, moff, size_t(n_patterns + 1), st));
  u64 all_windows = 0;
  HIP_TRY(hipMemcpyAsync(&total, moff + n_patterns, sizeof(u64), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&all_windows, windows, sizeof(u64), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  scratch.settled = true;
  if(all_windows >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, std::string(name) + ": 2^32 or more windows in one call; split the batch"); }
  if(to_scratch) { HIP_TRY(scratch.get(mins, total)); }
  else if(total > capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "minimizer buffer too small"); }
  if(total == 0) { return GCSA2_OK; }
  scratch.settled = false;
  if constexpr(CANONICAL)
  {
    hipLaunchKernelGGL((k_canonical_minimizers<true>), grid, dim3(MINI_TPB), 0, st, ix->img, d_patterns, d_offsets, n_patterns, u32(k), u32(w), hash_seed,
                       static_cast<u64*>(nullptr), static_cast<const u64*>(moff), mins);
  }
  else
  {
    hipLaunchKernelGGL((k_minimizers<true>), grid, dim3(MINI_TPB), 0, st, ix->img, d_patterns, d_offsets, n_patterns, u32(k), u32(w), hash_seed,
                       static_cast<u64*>(nullptr), static_cast<const u64*>(moff), mins);
  }
  LAUNCH_CHECK("k_minimizers");
  return GCSA2_OK;
}

// gcsa2_minimizer_hits_device after its argument checks (0 < n_patterns < 2^32): the selection into scratch, then what
// gcsa2_kmer_hits_device does behind its window plan, with the minimizers as the windows.
int minimizer_hits_core(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 w, u64 hash_seed,
                        u64 hit_max, int over, gcsa2_kmer_profile* d_profiles, u64* d_seed_offsets, gcsa2_mem* d_seeds, u64 seed_capacity,
                        u64* total_seeds, u64* d_hit_offsets, u64* d_hits, u64 hit_capacity, u64* total_hits, hipStream_t st)
{
  Scratch scratch(ix, st);
  u64 *moff = nullptr, total = 0;
  gcsa2_minimizer* mins = nullptr;
  const int rc = minimizer_select(ix, scratch, d_patterns, d_offsets, n_patterns, k, w, hash_seed, nullptr, true, nullptr, 0, "minimizer_hits", st,
                                  moff, mins, total);
  if(rc != GCSA2_OK) { return rc; }
  return kmer_hits_found(ix, scratch, d_patterns, d_offsets, n_patterns, k, 1, moff, total, mins, hit_max, over, d_profiles, d_seed_offsets, d_seeds,
                         seed_capacity, total_seeds, d_hit_offsets, d_hits, hit_capacity, total_hits, st);
}

// gcsa2_minimizers_device and gcsa2_canonical_minimizers_device (Rec, as minimizer_select)
template<class Rec>
int minimizers_device_form(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k, uint64_t w,
                           uint64_t hash_seed, uint64_t* d_min_offsets, Rec* d_minimizers, uint64_t capacity, uint64_t* total, void* stream,
                           const char* entry)
{
  int rc = minimizers_checks(ix, k, w, total);
  if(rc != GCSA2_OK) { return rc; }
  *total = 0;
  if(d_min_offsets == nullptr || (n_patterns > 0 && d_offsets == nullptr) || (d_minimizers == nullptr && capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "minimizers: 2^32 or more reads in one call; split the batch"); }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  hipStream_t st = static_cast<hipStream_t>(stream);
  if(n_patterns == 0)
  {
    HIP_TRY(hipMemsetAsync(d_min_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipStreamSynchronize(st));
    return GCSA2_OK;
  }
  Scratch scratch(ix, st);
  u64* moff = nullptr;
  Rec* mins = nullptr;
  u64 found = 0;
  rc = minimizer_select(ix, scratch, d_patterns, d_offsets, n_patterns, k, w, hash_seed, d_min_offsets, false, d_minimizers, capacity, "minimizers", st,
                        moff, mins, found);
  *total = found;
  if(rc != GCSA2_OK) { return rc; }
  HIP_TRY(hipStreamSynchronize(st));
  scratch.settled = true;
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string(entry) + ": " + e.what()); }
}

// The host form.  The number of minimizers of a piece (for_read_pieces) is not known before it ran, so every piece keeps its
// offsets and records in host memory and the caller's arrays are put together in read order at the end; the offsets are
// complete and *total is written whether the records fit or not.
template<class Rec>
int minimizers_batch_form(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k, uint64_t w,
                          uint64_t hash_seed, uint64_t* min_offsets, Rec* minimizers, uint64_t capacity, uint64_t* total, const char* entry)
{
  int rc = minimizers_checks(ix, k, w, total);
  if(rc != GCSA2_OK) { return rc; }
  *total = 0;
  if(min_offsets == nullptr || (n_patterns > 0 && offsets == nullptr) || (minimizers == nullptr && capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "minimizers: 2^32 or more reads in one call; split the batch"); }
  if(n_patterns == 0) { min_offsets[0] = 0; return GCSA2_OK; }
  rc = reads_ok(patterns, offsets, n_patterns, nullptr);
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  g_error.clear();
  if(host_windows(offsets, n_patterns, k, 1) >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "minimizers: 2^32 or more windows in one call; split the batch"); }
  const std::vector<u64> cut = read_cut(ix, offsets, n_patterns);
  struct Piece { std::vector<u64> off; std::vector<Rec> mins; };
  std::vector<Piece> done(cut.size() - 1);
  rc = for_read_pieces(ix, offsets, cut, [&](const ReadPiece& p, Outcome& out) -> bool
  {
    Piece& piece = done[p.c];
    DBuf<u8> d_pat; DBuf<u64> d_off;
    if(!upload_reads(p, patterns, d_pat, d_off, out)) { return false; }
    Scratch scratch(ix, p.stream);
    u64 *moff = nullptr, found = 0;
    Rec* mins = nullptr;
    const int piece_rc = minimizer_select(ix, scratch, d_pat.p, d_off.p, p.count, k, w, hash_seed, nullptr, true, nullptr, 0, "minimizers", p.stream,
                                          moff, mins, found);
    if(piece_rc != GCSA2_OK) { out.set(piece_rc, g_error); return false; }
    piece.off.resize(p.count + 1); piece.mins.resize(found);
    hipError_t e = hipMemcpyAsync(piece.off.data(), moff, (p.count + 1) * sizeof(u64), hipMemcpyDeviceToHost, p.stream);
    if(e == hipSuccess && found > 0) { e = hipMemcpyAsync(piece.mins.data(), mins, found * sizeof(Rec), hipMemcpyDeviceToHost, p.stream); }
    if(e == hipSuccess) { e = hipStreamSynchronize(p.stream); }
    if(e != hipSuccess) { out.hip_error("download of a piece", e); return false; }
    scratch.settled = true;
    return true;
  });
  if(rc != GCSA2_OK) { return rc; }
  u64 base = 0;
  for(u64 c = 0; c + 1 < cut.size(); c++)
  {
    const u64 b = cut[c], count = cut[c + 1] - b;
    for(u64 i = 0; i <= count; i++) { min_offsets[b + i] = done[c].off[i] + base; }
    base += done[c].mins.size();
  }
  *total = base;
  if(base > capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "minimizer buffer too small"); }
  base = 0;
  for(const Piece& piece : done)
  {
    if(!piece.mins.empty()) { std::memcpy(minimizers + base, piece.mins.data(), piece.mins.size() * sizeof(Rec)); }
    base += piece.mins.size();
  }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string(entry) + ": " + e.what()); }
}

}  // namespace

extern "C" {

int gcsa2_minimizers_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k, uint64_t w,
                            uint64_t hash_seed, uint64_t* d_min_offsets, gcsa2_minimizer* d_minimizers, uint64_t capacity, uint64_t* total,
                            void* stream)
{
  return minimizers_device_form(ix, d_patterns, d_offsets, n_patterns, k, w, hash_seed, d_min_offsets, d_minimizers, capacity, total, stream,
                                "gcsa2_minimizers_device");
}

int gcsa2_minimizers_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k, uint64_t w,
                           uint64_t hash_seed, uint64_t* min_offsets, gcsa2_minimizer* minimizers, uint64_t capacity, uint64_t* total)
{
  return minimizers_batch_form(ix, patterns, offsets, n_patterns, k, w, hash_seed, min_offsets, minimizers, capacity, total, "gcsa2_minimizers_batch");
}

int gcsa2_minimizer_hits_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k,
                                uint64_t w, uint64_t hash_seed, uint64_t hit_max, int over, gcsa2_kmer_profile* d_profiles,
                                uint64_t* d_seed_offsets, gcsa2_mem* d_seeds, uint64_t seed_capacity, uint64_t* total_seeds,
                                uint64_t* d_hit_offsets, uint64_t* d_hits, uint64_t hit_capacity, uint64_t* total_hits, void* stream)
{
  int rc = minimizer_hits_checks(ix, k, w, over, total_seeds, total_hits);
  if(rc != GCSA2_OK) { return rc; }
  *total_seeds = 0;
  *total_hits = 0;
  if(d_seed_offsets == nullptr || d_hit_offsets == nullptr || (n_patterns > 0 && d_offsets == nullptr) || (d_seeds == nullptr && seed_capacity > 0) ||
     (d_hits == nullptr && hit_capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "minimizer_hits: 2^32 or more reads in one call; split the batch"); }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  hipStream_t st = static_cast<hipStream_t>(stream);
  if(n_patterns == 0)
  {
    HIP_TRY(hipMemsetAsync(d_seed_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipStreamSynchronize(st));
    return GCSA2_OK;
  }
  return minimizer_hits_core(ix, d_patterns, d_offsets, n_patterns, k, w, hash_seed, hit_max, over, d_profiles, d_seed_offsets, d_seeds, seed_capacity,
                             total_seeds, d_hit_offsets, d_hits, hit_capacity, total_hits, st);
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_minimizer_hits_device: ") + e.what()); }
}

// The host form (seed_pieces_batch), as gcsa2_kmer_hits_batch: minimizers are per read, so the cut changes nothing.
int gcsa2_minimizer_hits_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k, uint64_t w,
                               uint64_t hash_seed, uint64_t hit_max, int over, gcsa2_kmer_profile* profiles, uint64_t* seed_offsets,
                               gcsa2_mem* seeds, uint64_t seed_capacity, uint64_t* total_seeds, uint64_t* hit_offsets, uint64_t* hits,
                               uint64_t hit_capacity, uint64_t* total_hits)
{
  int rc = minimizer_hits_checks(ix, k, w, over, total_seeds, total_hits);
  if(rc != GCSA2_OK) { return rc; }
  *total_seeds = 0;
  *total_hits = 0;
  if(seed_offsets == nullptr || hit_offsets == nullptr || (n_patterns > 0 && offsets == nullptr) || (seeds == nullptr && seed_capacity > 0) ||
     (hits == nullptr && hit_capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "minimizer_hits: 2^32 or more reads in one call; split the batch"); }
  if(n_patterns == 0) { seed_offsets[0] = 0; hit_offsets[0] = 0; return GCSA2_OK; }
  rc = reads_ok(patterns, offsets, n_patterns, nullptr);
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  g_error.clear();
  if(host_windows(offsets, n_patterns, k, 1) >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "minimizer_hits: 2^32 or more windows in one call; split the batch"); }
  // several pieces: room for every span's minimizer (a bound that the density 2 / (w + 1) stays far below), and an estimate of the hits
  auto estimate = [&](const ReadPiece& p) -> std::pair<u64, u64>
  {
    const u64 windows = host_windows(p.local, p.count, k, 1);
    if(p.pieces == 1) { return {std::min(seed_capacity, windows), hit_capacity}; }
    return {windows, 4 * windows};
  };
  auto run = [&](const ReadPiece& p, const u8* d_pat, const u64* d_off, u8* d_prof, u64* d_seed_off, gcsa2_mem* d_seeds, u64 rm, u64* m, u64* d_hit_off,
                 u64* d_hits, u64 rh, u64* h) -> int
  {
    return gcsa2_minimizer_hits_device(ix, d_pat, d_off, p.count, k, w, hash_seed, hit_max, over, reinterpret_cast<gcsa2_kmer_profile*>(d_prof), d_seed_off,
                                       d_seeds, rm, m, d_hit_off, d_hits, rh, h, p.stream);
  };
  return seed_pieces_batch(ix, patterns, offsets, n_patterns, estimate, run, sizeof(gcsa2_kmer_profile), profiles, seed_offsets, seeds, seed_capacity,
                           total_seeds, hit_offsets, hits, hit_capacity, total_hits);
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_minimizer_hits_batch: ") + e.what()); }
}

}  // extern "C"

// ==== stranded minimizer seeds: canonical minimizers and their hits on both strands (gcsa2_hip_strands.h, kernels_strands.hpp) ====
namespace {

// what both forms of the hits refuse before any device is touched, then the components the hits need
int stranded_hits_checks(const gcsa2_index* ix, u64 k, u64 w, int strands, int over, const u64* total_seeds, const u64* total_hits)
{
  const int rc = minimizers_checks(ix, k, w, total_seeds);
  if(rc != GCSA2_OK) { return rc; }
  if(total_hits == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null total pointer"); }
  if(strands < GCSA2_STRAND_FORWARD || strands > GCSA2_STRAND_BOTH)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "stranded_minimizer_hits: strands must be GCSA2_STRAND_FORWARD, GCSA2_STRAND_REVERSE or GCSA2_STRAND_BOTH");
  }
  if(over != GCSA2_MEM_OVER_SKIP && over != GCSA2_MEM_OVER_SAMPLE)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "stranded_minimizer_hits: unknown over-cap policy (GCSA2_MEM_OVER_SKIP or GCSA2_MEM_OVER_SAMPLE)");
  }
  if((strands & GCSA2_STRAND_REVERSE) != 0 && ix->img.sigma < 6)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "stranded_minimizer_hits: the reverse strand needs an alphabet with four codes (sigma >= 6)");
  }
  return locate_checks(ix, 0);
}

// The searched windows of a stranded call (0 < n_patterns < 2^31): the canonical selection into scratch, then the windows of the
// strands asked for as keys in group order (k_strand_windows) -- `goff` (2 n_patterns + 1) and `wins` (`searched` of them) are
// what kmer_hits_found takes as the window offsets of its "reads" and as its windows.
int stranded_windows(const gcsa2_index* ix, Scratch& scratch, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 w, u64 hash_seed,
                     int strands, const char* name, hipStream_t st, u64*& goff, ulonglong2*& wins, u64& searched)
{
  u64 *moff = nullptr, total = 0;
  gcsa2_canonical_minimizer* mins = nullptr;
  const int rc = minimizer_select(ix, scratch, d_patterns, d_offsets, n_patterns, k, w, hash_seed, nullptr, true, nullptr, 0, name, st, moff, mins, total);
  if(rc != GCSA2_OK) { return rc; }
  searched = (strands == GCSA2_STRAND_BOTH ? 2 : 1) * total;
  if(searched >= (u64(1) << 32))
  {
    HIP_TRY(hipStreamSynchronize(st));                       // the placing pass
    scratch.settled = true;
    return fail(GCSA2_ERR_BUFFER_TOO_SMALL, std::string(name) + ": 2^32 or more searched windows in one call; split the batch");
  }
  HIP_TRY(scratch.get(goff, 2 * n_patterns + 1));
  HIP_TRY(scratch.get(wins, searched));
  if(searched > 0)
  {
    scratch.settled = false;
    hipLaunchKernelGGL(k_strand_windows, dim3(grid_for((n_patterns + 1) * STRAND_LANES)), dim3(TPB), 0, st, d_offsets, n_patterns, u32(k), moff, mins,
                       u32(strands), goff, wins);
    LAUNCH_CHECK("k_strand_windows");
  }
  return GCSA2_OK;
}

// gcsa2_stranded_minimizer_hits_device after its argument checks (0 < n_patterns < 2^31): the searched windows, then what
// gcsa2_kmer_hits_device does behind its window plan with the 2 n_patterns groups as the reads and k_strand_seeds as the search.
int stranded_hits_core(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 w, u64 hash_seed,
                       int strands, u64 hit_max, int over, gcsa2_kmer_profile* d_profiles, u64* d_seed_offsets, gcsa2_mem* d_seeds, u64 seed_capacity,
                       u64* total_seeds, u64* d_hit_offsets, u64* d_hits, u64 hit_capacity, u64* total_hits, hipStream_t st)
{
  Scratch scratch(ix, st);
  u64 *goff = nullptr, searched = 0;
  ulonglong2* wins = nullptr;
  const int rc = stranded_windows(ix, scratch, d_patterns, d_offsets, n_patterns, k, w, hash_seed, strands, "stranded_minimizer_hits", st, goff, wins, searched);
  if(rc != GCSA2_OK) { return rc; }
  return kmer_hits_found(ix, scratch, nullptr, nullptr, 2 * n_patterns, k, 1, goff, searched, nullptr, hit_max, over, d_profiles, d_seed_offsets, d_seeds,
                         seed_capacity, total_seeds, d_hit_offsets, d_hits, hit_capacity, total_hits, st, wins);
}

}  // namespace

extern "C" {

int gcsa2_canonical_minimizers_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k,
                                      uint64_t w, uint64_t hash_seed, uint64_t* d_min_offsets, gcsa2_canonical_minimizer* d_minimizers,
                                      uint64_t capacity, uint64_t* total, void* stream)
{
  return minimizers_device_form(ix, d_patterns, d_offsets, n_patterns, k, w, hash_seed, d_min_offsets, d_minimizers, capacity, total, stream,
                                "gcsa2_canonical_minimizers_device");
}

int gcsa2_canonical_minimizers_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k, uint64_t w,
                                     uint64_t hash_seed, uint64_t* min_offsets, gcsa2_canonical_minimizer* minimizers, uint64_t capacity,
                                     uint64_t* total)
{
  return minimizers_batch_form(ix, patterns, offsets, n_patterns, k, w, hash_seed, min_offsets, minimizers, capacity, total,
                               "gcsa2_canonical_minimizers_batch");
}

int gcsa2_stranded_minimizer_hits_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k,
                                         uint64_t w, uint64_t hash_seed, int strands, uint64_t hit_max, int over, gcsa2_kmer_profile* d_profiles,
                                         uint64_t* d_seed_offsets, gcsa2_mem* d_seeds, uint64_t seed_capacity, uint64_t* total_seeds,
                                         uint64_t* d_hit_offsets, uint64_t* d_hits, uint64_t hit_capacity, uint64_t* total_hits, void* stream)
{
  int rc = stranded_hits_checks(ix, k, w, strands, over, total_seeds, total_hits);
  if(rc != GCSA2_OK) { return rc; }
  *total_seeds = 0;
  *total_hits = 0;
  if(d_seed_offsets == nullptr || d_hit_offsets == nullptr || (n_patterns > 0 && d_offsets == nullptr) || (d_seeds == nullptr && seed_capacity > 0) ||
     (d_hits == nullptr && hit_capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  if(n_patterns >= (u64(1) << 31)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "stranded_minimizer_hits: 2^31 or more reads in one call; split the batch"); }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  hipStream_t st = static_cast<hipStream_t>(stream);
  if(n_patterns == 0)
  {
    HIP_TRY(hipMemsetAsync(d_seed_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipStreamSynchronize(st));
    return GCSA2_OK;
  }
  return stranded_hits_core(ix, d_patterns, d_offsets, n_patterns, k, w, hash_seed, strands, hit_max, over, d_profiles, d_seed_offsets, d_seeds,
                            seed_capacity, total_seeds, d_hit_offsets, d_hits, hit_capacity, total_hits, st);
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_stranded_minimizer_hits_device: ") + e.what()); }
}

// The host form (seed_pieces_batch with two groups per read), as gcsa2_minimizer_hits_batch: the groups are per read, so the
// cut changes nothing.
int gcsa2_stranded_minimizer_hits_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k,
                                        uint64_t w, uint64_t hash_seed, int strands, uint64_t hit_max, int over, gcsa2_kmer_profile* profiles,
                                        uint64_t* seed_offsets, gcsa2_mem* seeds, uint64_t seed_capacity, uint64_t* total_seeds,
                                        uint64_t* hit_offsets, uint64_t* hits, uint64_t hit_capacity, uint64_t* total_hits)
{
  int rc = stranded_hits_checks(ix, k, w, strands, over, total_seeds, total_hits);
  if(rc != GCSA2_OK) { return rc; }
  *total_seeds = 0;
  *total_hits = 0;
  if(seed_offsets == nullptr || hit_offsets == nullptr || (n_patterns > 0 && offsets == nullptr) || (seeds == nullptr && seed_capacity > 0) ||
     (hits == nullptr && hit_capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  if(n_patterns >= (u64(1) << 31)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "stranded_minimizer_hits: 2^31 or more reads in one call; split the batch"); }
  if(n_patterns == 0) { seed_offsets[0] = 0; hit_offsets[0] = 0; return GCSA2_OK; }
  rc = reads_ok(patterns, offsets, n_patterns, nullptr);
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  g_error.clear();
  if(host_windows(offsets, n_patterns, k, 1) >= (u64(1) << 32))
  {
    return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "stranded_minimizer_hits: 2^32 or more windows in one call; split the batch");
  }
  const u64 per = (strands == GCSA2_STRAND_BOTH ? 2 : 1);
  // several pieces: room for every span's minimizer on the strands asked for, and an estimate of the hits
  auto estimate = [&](const ReadPiece& p) -> std::pair<u64, u64>
  {
    const u64 windows = per * host_windows(p.local, p.count, k, 1);
    if(p.pieces == 1) { return {std::min(seed_capacity, windows), hit_capacity}; }
    return {windows, 4 * windows};
  };
  auto run = [&](const ReadPiece& p, const u8* d_pat, const u64* d_off, u8* d_prof, u64* d_seed_off, gcsa2_mem* d_seeds, u64 rm, u64* m, u64* d_hit_off,
                 u64* d_hits, u64 rh, u64* h) -> int
  {
    return gcsa2_stranded_minimizer_hits_device(ix, d_pat, d_off, p.count, k, w, hash_seed, strands, hit_max, over,
                                                reinterpret_cast<gcsa2_kmer_profile*>(d_prof), d_seed_off, d_seeds, rm, m, d_hit_off, d_hits, rh, h, p.stream);
  };
  return seed_pieces_batch(ix, patterns, offsets, n_patterns, estimate, run, sizeof(gcsa2_kmer_profile), profiles, seed_offsets, seeds, seed_capacity,
                           total_seeds, hit_offsets, hits, hit_capacity, total_hits, 2);
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_stranded_minimizer_hits_batch: ") + e.what()); }
}

}  // extern "C"

// ==== capped seeds: the shortest matches of every read that occur at most max_count times (kernels_seeds.hpp, kernels_mem.hpp) ====
namespace {

// what both forms refuse before any device is touched, then the components the call needs (no LCP array)
int capped_seeds_checks(const gcsa2_index* ix, u64 min_length, u64 max_length, u64 max_count, int over, const u64* total_seeds, const u64* total_hits)
{
  CHECK_INDEX(ix);
  if(total_seeds == nullptr || total_hits == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "null total pointer"); }
  if(min_length == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "capped_seeds: min_length must be at least 1"); }
  if(max_count == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "capped_seeds: max_count must be at least 1"); }
  if(max_length != 0 && min_length > max_length) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "capped_seeds: min_length exceeds max_length: no seed could be reported"); }
  if(over != GCSA2_MEM_OVER_SKIP && over != GCSA2_MEM_OVER_SAMPLE)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "capped_seeds: unknown over-cap policy (GCSA2_MEM_OVER_SKIP or GCSA2_MEM_OVER_SAMPLE)");
  }
  return locate_checks(ix, 0);
}

// gcsa2_capped_seeds_device after its argument checks (0 < n_patterns < 2^32).  Host round trips: the seed total with the
// overrun flag, those of the shared tail, the end.  Scratch: two words per read, the rest per seed.
int capped_seeds_core(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 min_length, u64 max_length,
                      u64 max_count, u64 hit_max, int over, u64* d_seed_offsets, gcsa2_mem* d_seeds, u64 seed_capacity, u64* total_seeds,
                      u64* d_hit_offsets, u64* d_hits, u64 hit_capacity, u64* total_hits, hipStream_t st)
{
  Scratch scratch(ix, st);
  unsigned long long* ctl = nullptr;
  u64 *sizes = nullptr, *seed_off = nullptr;
  HIP_TRY(scratch.get(ctl, SEEDS_CTL_WORDS));
  HIP_TRY(scratch.get(sizes, n_patterns + 1));
  HIP_TRY(scratch.get(seed_off, n_patterns + 1));
  HIP_TRY(hipMemsetAsync(ctl, 0, SEEDS_CTL_WORDS * sizeof(unsigned long long), st));
  HIP_TRY(hipMemsetAsync(sizes, 0, (n_patterns + 1) * sizeof(u64), st));
  // 1. the walk, counting; the CSR offsets; the walk again, writing (persistent lanes: what the device holds at once)
  const u64 nr = (ix->img.n == 0 ? 0 : n_patterns);
  const u64 resident = ix->tune.ms_grid != 0 ? ix->tune.ms_grid : u64(ix->compute_units) * 8;
  const unsigned grid = unsigned(std::max<u64>(1, std::min<u64>((nr + TPB2 - 1) / TPB2, resident)));
  const bool pair = (ix->img.flp != nullptr);          // the start of an attempt goes two characters per request
  if(nr > 0)
  {
    if(pair) { hipLaunchKernelGGL((k_capped_seeds<false, true>), dim3(grid), dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, nr, min_length, max_length, max_count, ctl, sizes, nullptr, nullptr, nullptr); }
    else { hipLaunchKernelGGL((k_capped_seeds<false, false>), dim3(grid), dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, nr, min_length, max_length, max_count, ctl, sizes, nullptr, nullptr, nullptr); }
    LAUNCH_CHECK("k_capped_seeds<count>");
  }
  size_t scan_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, sizes, seed_off, size_t(n_patterns + 1), st));
  char* scan_tmp = nullptr;
  HIP_TRY(scratch.get(scan_tmp, scan_bytes));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, sizes, seed_off, size_t(n_patterns + 1), st));
  u64 m = 0;
  unsigned long long words[SEEDS_CTL_WORDS];
  HIP_TRY(hipMemcpyAsync(&m, seed_off + n_patterns, sizeof(u64), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(words, ctl, sizeof(words), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if(words[0] != 0) { scratch.settled = true; return fail(GCSA2_ERR_HIP, "capped_seeds: a walk took more than 2 L + 2 LF steps for a read of L characters; the index is inconsistent"); }
  *total_seeds = m;
  if(m >= (u64(1) << 32)) { scratch.settled = true; return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "capped_seeds: 2^32 or more seeds in one call; split the batch"); }
  if(m == 0)
  {
    HIP_TRY(hipMemsetAsync(d_seed_offsets, 0, (n_patterns + 1) * sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipStreamSynchronize(st));
    scratch.settled = true;
    return GCSA2_OK;
  }
  u64 *recs = nullptr, *counts = nullptr;
  HIP_TRY(scratch.get(recs, 4 * m));
  HIP_TRY(scratch.get(counts, m));
  HIP_TRY(hipMemsetAsync(ctl + 1, 0, sizeof(unsigned long long), st));
  if(pair) { hipLaunchKernelGGL((k_capped_seeds<true, true>), dim3(grid), dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, nr, min_length, max_length, max_count, ctl, nullptr, seed_off, recs, counts); }
  else { hipLaunchKernelGGL((k_capped_seeds<true, false>), dim3(grid), dim3(TPB2), 0, st, ix->img, d_patterns, d_offsets, nr, min_length, max_length, max_count, ctl, nullptr, seed_off, recs, counts); }
  LAUNCH_CHECK("k_capped_seeds<write>");
  // 2. count class, locate, hits in seed order (mem_hits' tail); the offsets only once everything fits
  const int rc = mem_hits_tail(ix, recs, counts, m, hit_max, over, d_seeds, seed_capacity, d_hit_offsets, d_hits, hit_capacity, total_hits, scratch, st);
  if(rc != GCSA2_OK) { return rc; }
  scratch.settled = false;
  HIP_TRY(hipMemcpyAsync(d_seed_offsets, seed_off, (n_patterns + 1) * sizeof(u64), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  scratch.settled = true;
  return GCSA2_OK;
}

}  // namespace

extern "C" {

int gcsa2_capped_seeds_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t min_length,
                              uint64_t max_length, uint64_t max_count, uint64_t hit_max, int over, uint64_t* d_seed_offsets, gcsa2_mem* d_seeds,
                              uint64_t seed_capacity, uint64_t* total_seeds, uint64_t* d_hit_offsets, uint64_t* d_hits, uint64_t hit_capacity,
                              uint64_t* total_hits, void* stream)
{
  int rc = capped_seeds_checks(ix, min_length, max_length, max_count, over, total_seeds, total_hits);
  if(rc != GCSA2_OK) { return rc; }
  *total_seeds = 0;
  *total_hits = 0;
  if(d_seed_offsets == nullptr || d_hit_offsets == nullptr || (n_patterns > 0 && d_offsets == nullptr) || (d_seeds == nullptr && seed_capacity > 0) ||
     (d_hits == nullptr && hit_capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "capped_seeds: 2^32 or more reads in one call; split the batch"); }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  hipStream_t st = static_cast<hipStream_t>(stream);
  if(n_patterns == 0)
  {
    HIP_TRY(hipMemsetAsync(d_seed_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, sizeof(u64), st));
    HIP_TRY(hipStreamSynchronize(st));
    return GCSA2_OK;
  }
  return capped_seeds_core(ix, d_patterns, d_offsets, n_patterns, min_length, max_length, max_count, hit_max, over, d_seed_offsets, d_seeds, seed_capacity,
                           total_seeds, d_hit_offsets, d_hits, hit_capacity, total_hits, st);
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_capped_seeds_device: ") + e.what()); }
}

// The host form (seed_pieces_batch).  Its own: the first run of a piece among several is a guess, and a refusal costs
// little, because the device form's sizing run keeps no records.
int gcsa2_capped_seeds_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t min_length,
                             uint64_t max_length, uint64_t max_count, uint64_t hit_max, int over, uint64_t* seed_offsets, gcsa2_mem* seeds,
                             uint64_t seed_capacity, uint64_t* total_seeds, uint64_t* hit_offsets, uint64_t* hits, uint64_t hit_capacity,
                             uint64_t* total_hits)
{
  int rc = capped_seeds_checks(ix, min_length, max_length, max_count, over, total_seeds, total_hits);
  if(rc != GCSA2_OK) { return rc; }
  *total_seeds = 0;
  *total_hits = 0;
  if(seed_offsets == nullptr || hit_offsets == nullptr || (n_patterns > 0 && offsets == nullptr) || (seeds == nullptr && seed_capacity > 0) ||
     (hits == nullptr && hit_capacity > 0))
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "null buffer");
  }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "capped_seeds: 2^32 or more reads in one call; split the batch"); }
  if(n_patterns == 0) { seed_offsets[0] = 0; hit_offsets[0] = 0; return GCSA2_OK; }
  rc = reads_ok(patterns, offsets, n_patterns, nullptr);
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  g_error.clear();
  // one piece: never more seeds than a read has positions for; several: one seed per eight positions, four hits per seed
  auto estimate = [&](const ReadPiece& p) -> std::pair<u64, u64>
  {
    if(p.pieces == 1) { return {std::min(seed_capacity, p.bytes / min_length), hit_capacity}; }
    const u64 rm = p.bytes / (8 * min_length) + p.count + 1;
    return {rm, 4 * rm};
  };
  auto run = [&](const ReadPiece& p, const u8* d_pat, const u64* d_off, u8*, u64* d_seed_off, gcsa2_mem* d_seeds, u64 rm, u64* m, u64* d_hit_off, u64* d_hits,
                 u64 rh, u64* h) -> int
  {
    return gcsa2_capped_seeds_device(ix, d_pat, d_off, p.count, min_length, max_length, max_count, hit_max, over, d_seed_off, d_seeds, rm, m, d_hit_off, d_hits,
                                     rh, h, p.stream);
  };
  return seed_pieces_batch(ix, patterns, offsets, n_patterns, estimate, run, 0, nullptr, seed_offsets, seeds, seed_capacity, total_seeds, hit_offsets, hits,
                           hit_capacity, total_hits);
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_capped_seeds_batch: ") + e.what()); }
}

}  // extern "C"

// ==== the calls over seed records with statistics: k-mer support, k-mer classes, seed clusters, seed chains ===============================
namespace {

// The shell of gcsa2_<name>_device after its argument checks.  `empty` (no read, no group, no record): zeroed statistics and
// nothing else.  Otherwise core(sums) runs on the index's device, `sums` holding what the arguments alone say, and the
// statistics reach the caller only with GCSA2_OK.
template<class Stats, class Core>
int stats_entry(const char* name, const gcsa2_index* ix, Stats* stats, Stats sums, bool empty, Core core)
{
  if(empty) { if(stats != nullptr) { *stats = Stats{}; } return GCSA2_OK; }
  try {   // no C++ exception may cross the C boundary
  DeviceGuard guard(ix->device);
  g_error.clear();
  const int rc = core(sums);
  if(rc == GCSA2_OK && stats != nullptr) { *stats = sums; }
  return rc;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_") + name + "_device: " + e.what()); }
}

// a += b, counter by counter, for the host forms that sum their pieces' statistics
template<class Stats>
void sum_stats(Stats& a, const Stats& b)
{
  constexpr size_t N = sizeof(Stats) / sizeof(uint64_t);
  static_assert(sizeof(Stats) == N * sizeof(uint64_t) && std::is_trivially_copyable<Stats>::value, "a struct of uint64_t counters and nothing else");
  uint64_t x[N], y[N];
  std::memcpy(x, &a, sizeof(Stats)); std::memcpy(y, &b, sizeof(Stats));
  for(size_t i = 0; i < N; i++) { x[i] += y[i]; }
  std::memcpy(&a, x, sizeof(Stats));
}
static_assert(sizeof(gcsa2_support_stats) == 7 * sizeof(uint64_t) && sizeof(gcsa2_class_stats) == 8 * sizeof(uint64_t) &&
              sizeof(gcsa2_cluster_stats) == 7 * sizeof(uint64_t) && sizeof(gcsa2_chain_stats) == 7 * sizeof(uint64_t),
              "sum_stats: a field of another type was added");

}  // namespace

// ==== seed records folded into runs of equal ranges and located chunk by chunk: what k-mer support and k-mer classes share ====
#include "host_fold.hpp"

// ==== k-mer support: read k-mers (or any seed records) summed per graph node (kernels_support.hpp) ==========================
namespace {

// what every form refuses before any device is touched, then the components the call needs (no LCP array)
int support_checks(const gcsa2_index* ix, u64 shift, int flags, const void* support, u64 n_bins, const char* support_name)
{
  CHECK_INDEX(ix);
  if(shift >= 64) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "support: shift must be below 64"); }
  if((flags & ~GCSA2_SUPPORT_PER_BIN) != 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "support: unknown flags (GCSA2_SUPPORT_PER_BIN)"); }
  if(support == nullptr && n_bins > 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, std::string("support: ") + support_name + " is NULL with n_bins > 0"); }
  return locate_checks(ix, 0);
}

int kmer_support_checks(const gcsa2_index* ix, u64 k, u64 stride, u64 shift, int flags, const void* support, u64 n_bins, const char* support_name)
{
  CHECK_INDEX(ix);
  if(k == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_support: k must be at least 1"); }
  if(stride == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_support: stride must be at least 1"); }
  return support_checks(ix, shift, flags, support, n_bins, support_name);
}

// Steps 2 onward of a support call: m (1 <= m < 2^32) records of `words` u64 with (sp, ep) at words 2 and 3, their count()s
// in `known` or (nullptr) computed here, weights or (nullptr) 1 each, are added to d_support.  Fills every field of *st_out
// but `windows`.  Host round trips: those of fold_seed_ranges, cut_chunks and for_located_chunks (host_fold.hpp), the end.
// Scratch: theirs.
int support_tail(const gcsa2_index* ix, const u64* recs, u32 words, const u64* known, const u64* weights, u64 m, u64 hit_max, u64 shift, int flags,
                 u64* d_support, u64 n_bins, gcsa2_support_stats* st_out, Scratch& scratch, hipStream_t st)
{
  unsigned long long* stat = nullptr;
  HIP_TRY(scratch.get(stat, SUP_WORDS));
  SeedFold fold;
  int rc = fold_seed_ranges(ix, recs, words, known, weights, m, hit_max, false, stat, fold, scratch, st);
  if(rc != GCSA2_OK) { return rc; }
  st_out->found = fold.found;
  st_out->counted = fold.counted;
  if(fold.counted == 0) { scratch.settled = true; return GCSA2_OK; }
  st_out->distinct = fold.distinct;
  SeedChunks chunks;
  rc = cut_chunks(ix, fold, stat + SUP_CUT, "support", chunks, scratch, st);
  if(rc != GCSA2_OK) { return rc; }
  // locate and add, chunk by chunk
  u64 values = 0;
  rc = for_located_chunks(ix, fold, chunks, "support", &values, scratch, st, []() -> int { return GCSA2_OK; },
                          [&](const SeedChunk& chunk, u64 runs, u64 total, const u64* off, const u64* val, const u64* owners, u64) -> int
  {
    hipLaunchKernelGGL(k_support_add, dim3(grid_for(total)), dim3(TPB), 0, st, off, val, owners, runs, total, fold.mult + chunk.q0, u32(shift),
                       int((flags & GCSA2_SUPPORT_PER_BIN) != 0), reinterpret_cast<unsigned long long*>(d_support), n_bins, stat);
    LAUNCH_CHECK("k_support_add");
    scratch.settled = false;
    return GCSA2_OK;
  });
  if(rc != GCSA2_OK) { return rc; }
  unsigned long long host_stat[SUP_WORDS];
  HIP_TRY(hipMemcpyAsync(host_stat, stat, sizeof(host_stat), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  scratch.settled = true;
  st_out->values = values;
  st_out->added = host_stat[SUP_ADDED];
  st_out->dropped = host_stat[SUP_DROPPED];
  return GCSA2_OK;
}

// gcsa2_kmer_support_device after its argument checks (0 < n_patterns < 2^32): the search of gcsa2_kmer_hits_device with room
// for every window, so that it runs once; its records stay in arrival order and go to support_tail with their count()s.
int kmer_support_core(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 stride, u64 hit_max,
                      u64 shift, int flags, u64* d_support, u64 n_bins, gcsa2_support_stats* st_out, hipStream_t st)
{
  Scratch scratch(ix, st);
  u64 *woff = nullptr, total = 0, m = 0;
  int rc = window_plan(scratch, d_offsets, n_patterns, k, stride, nullptr, "kmer_support", st, woff, total);
  if(rc != GCSA2_OK) { return rc; }
  scratch.settled = true;
  st_out->windows = total;
  if(total == 0) { return GCSA2_OK; }
  SeedEmit emit{};
  rc = kmer_seed_search(ix, scratch, d_patterns, d_offsets, n_patterns, k, stride, woff, total, total, nullptr, 1, st, emit, m);
  if(rc != GCSA2_OK) { return rc; }
  scratch.settled = true;
  if(m > emit.capacity) { return fail(GCSA2_ERR_HIP, "kmer_support: more seeds than windows"); }
  if(m == 0) { return GCSA2_OK; }
  scratch.settled = false;
  return support_tail(ix, emit.recs, 4, emit.counts, nullptr, m, hit_max, shift, flags, d_support, n_bins, st_out, scratch, st);
}

}  // namespace

extern "C" {

int gcsa2_kmer_support_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k,
                              uint64_t stride, uint64_t hit_max, uint64_t shift, int flags, uint64_t* d_support, uint64_t n_bins,
                              gcsa2_support_stats* stats, void* stream)
{
  int rc = kmer_support_checks(ix, k, stride, shift, flags, d_support, n_bins, "d_support");
  if(rc != GCSA2_OK) { return rc; }
  if(n_patterns > 0 && d_offsets == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_support: d_offsets is NULL"); }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "kmer_support: 2^32 or more reads in one call; split the batch"); }
  return stats_entry("kmer_support", ix, stats, gcsa2_support_stats{}, n_patterns == 0, [&](gcsa2_support_stats& sums) -> int
  {
    return kmer_support_core(ix, d_patterns, d_offsets, n_patterns, k, stride, hit_max, shift, flags, d_support, n_bins, &sums, static_cast<hipStream_t>(stream));
  });
}

int gcsa2_seed_support_device(const gcsa2_index* ix, const gcsa2_mem* d_seeds, uint64_t n_seeds, const uint64_t* d_weights, uint64_t hit_max,
                              uint64_t shift, int flags, uint64_t* d_support, uint64_t n_bins, gcsa2_support_stats* stats, void* stream)
{
  int rc = support_checks(ix, shift, flags, d_support, n_bins, "d_support");
  if(rc != GCSA2_OK) { return rc; }
  if(n_seeds > 0 && d_seeds == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "seed_support: d_seeds is NULL"); }
  if(n_seeds >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "seed_support: 2^32 or more seeds in one call; split the batch"); }
  gcsa2_support_stats pre{};
  pre.windows = n_seeds;
  return stats_entry("seed_support", ix, stats, pre, n_seeds == 0, [&](gcsa2_support_stats& sums) -> int
  {
    hipStream_t st = static_cast<hipStream_t>(stream);
    static_assert(sizeof(gcsa2_mem) == 5 * sizeof(u64), "gcsa2_mem is five words");
    Scratch scratch(ix, st);
    return support_tail(ix, reinterpret_cast<const u64*>(d_seeds), 5, nullptr, d_weights, n_seeds, hit_max, shift, flags, d_support, n_bins, &sums, scratch, st);
  });
}

// The host form.  One zeroed device array of n_bins for the whole call; each piece (for_read_pieces) is one
// gcsa2_kmer_support_device on its thread's stream -- the pieces add into the one array with atomics -- and the array is
// added into the caller's at the end.
int gcsa2_kmer_support_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k,
                             uint64_t stride, uint64_t hit_max, uint64_t shift, int flags, uint64_t* support, uint64_t n_bins,
                             gcsa2_support_stats* stats)
{
  int rc = kmer_support_checks(ix, k, stride, shift, flags, support, n_bins, "support");
  if(rc != GCSA2_OK) { return rc; }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "kmer_support: 2^32 or more reads in one call; split the batch"); }
  gcsa2_support_stats sums{};
  if(n_patterns == 0) { if(stats != nullptr) { *stats = sums; } return GCSA2_OK; }
  if(offsets == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_support: offsets is NULL"); }
  rc = reads_ok(patterns, offsets, n_patterns, "kmer_support");
  if(rc != GCSA2_OK) { return rc; }
  try {   // no C++ exception may cross the C boundary
  g_error.clear();
  if(host_windows(offsets, n_patterns, k, stride) >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "kmer_support: 2^32 or more windows in one call; split the batch"); }
  DeviceGuard guard(ix->device);
  DBuf<u64> d_sup;
  HIP_TRY(d_sup.alloc(n_bins));
  HIP_TRY(hipMemset(d_sup.p, 0, (n_bins > 0 ? n_bins : 1) * sizeof(u64)));
  const std::vector<u64> cut = read_cut(ix, offsets, n_patterns);
  std::vector<gcsa2_support_stats> done(cut.size() - 1);
  rc = for_read_pieces(ix, offsets, cut, [&](const ReadPiece& p, Outcome& out) -> bool
  {
    DBuf<u8> d_pat; DBuf<u64> d_off;
    if(!upload_reads(p, patterns, d_pat, d_off, out)) { return false; }
    const int piece_rc = gcsa2_kmer_support_device(ix, d_pat.p, d_off.p, p.count, k, stride, hit_max, shift, flags, d_sup.p, n_bins, &done[p.c], p.stream);
    if(piece_rc != GCSA2_OK) { out.set(piece_rc, g_error); return false; }
    return true;
  });
  if(rc != GCSA2_OK) { return rc; }
  for(const gcsa2_support_stats& s : done) { sum_stats(sums, s); }
  if(n_bins > 0)
  {
    std::vector<u64> got(n_bins);
    HIP_TRY(hipMemcpy(got.data(), d_sup.p, n_bins * sizeof(u64), hipMemcpyDeviceToHost));
    for(u64 i = 0; i < n_bins; i++) { support[i] += got[i]; }
  }
  if(stats != nullptr) { *stats = sums; }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string("gcsa2_kmer_support_batch: ") + e.what()); }
}

}  // extern "C"

// ==== the index-side k-mer calls: countKMers, compareKMers, the index k-mer spectrum (one walk of one search tree) ====
#include "host_kmers.hpp"

// ==== k-mer classes: per read, the votes of its k-mers (or any seed records) over classes of graph nodes (kernels_classes.hpp) ====
namespace {

// what every form refuses before any device is touched, then the components the call needs (no LCP array)
int classes_checks(const gcsa2_index* ix, u64 shift, int flags, const void* class_of_bin, u64 n_bins, u64 n_classes, const char* map_name, u64 top_n = 0,
                   bool sparse = false)
{
  CHECK_INDEX(ix);
  if(shift >= 64) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "classes: shift must be below 64"); }
  if((flags & ~(GCSA2_CLASS_PER_WINDOW | GCSA2_CLASS_UNAMBIGUOUS)) != 0)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "classes: unknown flags (GCSA2_CLASS_PER_WINDOW, GCSA2_CLASS_UNAMBIGUOUS)");
  }
  if(sparse)
  {
    if(n_classes == 0 || n_classes > 0xFFFFFFFFull) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "top_classes: n_classes must be 1 .. 0xFFFFFFFF"); }
    if(top_n == 0 || top_n > GCSA2_TOP_LIMIT) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "top_classes: top_n must be 1 .. GCSA2_TOP_LIMIT (64)"); }
  }
  else if(n_classes == 0 || n_classes > GCSA2_CLASS_LIMIT) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "classes: n_classes must be 1 .. GCSA2_CLASS_LIMIT (4096)"); }
  if(class_of_bin == nullptr && n_bins > 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, std::string("classes: ") + map_name + " is NULL with n_bins > 0"); }
  return locate_checks(ix, 0);
}

int kmer_classes_checks(const gcsa2_index* ix, u64 k, u64 stride, u64 shift, int flags, const void* class_of_bin, u64 n_bins, u64 n_classes, const char* map_name,
                        u64 top_n = 0, bool sparse = false)
{
  CHECK_INDEX(ix);
  if(k == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_classes: k must be at least 1"); }
  if(stride == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_classes: stride must be at least 1"); }
  return classes_checks(ix, shift, flags, class_of_bin, n_bins, n_classes, map_name, top_n, sparse);
}

// what a call votes with and writes: the dense form (votes, calls) or, with top_n != 0, the sparse one (top, summaries), whose
// keys and signatures are the wide ones
struct ClassesJob
{
  u64 hit_max, shift; int flags;
  const u32* class_of_bin; u64 n_bins, n_classes;
  u64* votes; gcsa2_class_call* calls;
  u64 top_n; gcsa2_class_vote* top; gcsa2_top_summary* summaries;
};

// GCSA2_TOP_SLOTS (a test knob, read per call): the slots of k_classes_top's table, a power of two (rounded down) between
// TOP_SLOTS_MIN and TOP_SLOTS_MAX.  The result never depends on it.
u32 top_slots()
{
  u64 slots = TOP_SLOTS_DEFAULT, v = 0;
  if(env_count("GCSA2_TOP_SLOTS", &v)) { slots = std::min<u64>(std::max<u64>(v, TOP_SLOTS_MIN), TOP_SLOTS_MAX); }
  u32 out = TOP_SLOTS_MIN;
  while(u64(out) * 2 <= slots) { out *= 2; }
  return out;
}

// Steps 2 onward of a classes call.  m (< 2^32) records of `words` u64 with (sp, ep) at words 2 and 3, their count()s in
// `known` or (nullptr) computed here, weights or (nullptr) 1 each.  n_groups (1 <= n_groups < 2^32) groups: with `windows`,
// group q owns the windows [group_off[q], group_off[q + 1]) of a search of `limit` windows whose wavefronts left wave_base /
// wave_mask; otherwise the records [group_off[q], group_off[q + 1]), limit = m.  Writes every row and call and fills every
// field of *st_out but `windows`.  Host round trips: those of support_tail.  Scratch: that of fold_seed_ranges with slots,
// cut_chunks and for_located_chunks (host_fold.hpp); per value that the distinct ranges count() 8 bytes (the signatures, which
// stay); per chunk -- the same buffers for every chunk -- 20 bytes per value of the largest, and hipCUB's.  A range of 2^31 or
// more values is refused (one run-length encoding per chunk).
int classes_tail(const gcsa2_index* ix, const u64* recs, u32 words, const u64* known, const u64* weights, u64 m, bool windows, const u64* group_off,
                 u64 n_groups, u64 limit, const u32* wave_base, const u64* wave_mask, const ClassesJob& job, gcsa2_class_stats* st_out,
                 Scratch& scratch, hipStream_t st)
{
  unsigned long long* stat = nullptr;
  HIP_TRY(scratch.get(stat, CLS_WORDS));
  // steps 1 and 2: the cap, every record keeping its compacted place, and the fold.  The runs' multiplicities are not needed.
  SeedFold fold;
  int rc = fold_seed_ranges(ix, recs, words, known, nullptr, m, job.hit_max, true, stat, fold, scratch, st);
  if(rc != GCSA2_OK) { return rc; }
  st_out->found = fold.found;
  st_out->counted = fold.counted;
  st_out->distinct = fold.distinct;
  u64* sig = nullptr;
  // the last step, from wherever the records run out: every row and call is written, with or without a counted record
  auto vote = [&]() -> int
  {
    const u64 resident = u64(ix->compute_units) * 32;              // one wavefront per workgroup
    const dim3 grid(unsigned(std::min<u64>(n_groups, resident)));
    if(job.top_n != 0)
    {
      const u32 slots = top_slots();
      const size_t lds = size_t(slots) * (sizeof(u64) + sizeof(u32));
      const dim3 fit(unsigned(std::min<u64>(n_groups, u64(ix->compute_units) * std::min<u64>(32, (160u << 10) / lds))));   // as many as a CU's LDS holds
      hipLaunchKernelGGL((windows ? k_classes_top<true> : k_classes_top<false>), fit, dim3(64), lds, st, group_off, n_groups, limit, wave_base, wave_mask,
                         fold.slot, fold.run_of, fold.span, sig, weights, job.flags, slots, u32(job.top_n), job.top, job.summaries, stat);
      LAUNCH_CHECK("k_classes_top");
    }
    else
    {
      const size_t lds = size_t(job.n_classes) * sizeof(u64);
      hipLaunchKernelGGL((windows ? k_classes_vote<true> : k_classes_vote<false>), grid, dim3(64), lds, st, group_off, n_groups, limit, wave_base, wave_mask,
                         fold.slot, fold.run_of, fold.span, sig, weights, job.flags, u32(job.n_classes), job.votes, job.calls, stat);
      LAUNCH_CHECK("k_classes_vote");
    }
    unsigned long long host_stat[CLS_WORDS];
    HIP_TRY(hipMemcpyAsync(host_stat, stat, sizeof(host_stat), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    scratch.settled = true;
    st_out->votes = host_stat[CLS_VOTES];
    st_out->unclassified = host_stat[CLS_UNCLASSIFIED];
    st_out->ambiguous = host_stat[CLS_AMBIGUOUS];
    return GCSA2_OK;
  };
  if(fold.counted == 0) { return vote(); }
  // 3. the chunks, as support_tail cuts them
  SeedChunks chunks;
  rc = cut_chunks(ix, fold, stat + CLS_CUT, "classes", chunks, scratch, st);
  if(rc != GCSA2_OK) { return rc; }
  // 4. locate and sign, chunk by chunk, in the same scratch; the signatures of all chunks stay, one entry per value at most
  const u64 most_raw = chunks.most_raw, most_runs = chunks.most_runs;
  u64 *keys = nullptr, *sorted = nullptr;
  u32 *lengths = nullptr, *n_entries = nullptr;
  char* cub = nullptr;
  if(most_raw >= (u64(1) << 31)) { scratch.settled = true; return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "classes: a range with 2^31 or more values; set hit_max"); }
  const bool wide = job.top_n != 0;
  int key_bits = 0;
  size_t keys_bytes = 0, rle_bytes = 0;
  rc = for_located_chunks(ix, fold, chunks, "classes", &st_out->values, scratch, st, [&]() -> int
  {
    HIP_TRY(scratch.get(keys, most_raw)); HIP_TRY(scratch.get(sorted, most_raw)); HIP_TRY(scratch.get(lengths, most_raw)); HIP_TRY(scratch.get(n_entries, 1));
    HIP_TRY(scratch.get(sig, chunks.all_raw));
    int run_bits = 1;
    while(run_bits < 50 && (most_runs >> run_bits) != 0) { run_bits++; }
    if(wide && most_runs >= (u64(1) << 31)) { scratch.settled = true; return fail(GCSA2_ERR_HIP, "top_classes: a chunk with 2^31 or more ranges"); }
    key_bits = int(wide ? WIDE_KEY_BITS : CLASS_KEY_BITS) + run_bits;
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, keys_bytes, keys, sorted, size_t(most_raw > 0 ? most_raw : 1), 0, key_bits, st));
    HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(nullptr, rle_bytes, sorted, keys, lengths, n_entries, int(most_raw > 0 ? most_raw : 1), st));
    HIP_TRY(scratch.get(cub, std::max(keys_bytes, rle_bytes)));
    return GCSA2_OK;
  },
  [&](const SeedChunk& chunk, u64, u64 total, const u64* off, const u64* val, const u64* owners, u64 values) -> int
  {
    if(wide) { hipLaunchKernelGGL(k_classes_keys<true>, dim3(grid_for(total)), dim3(TPB), 0, st, off, val, owners, total, u32(job.shift), job.class_of_bin, job.n_bins, job.n_classes, keys); }
    else { hipLaunchKernelGGL(k_classes_keys<false>, dim3(grid_for(total)), dim3(TPB), 0, st, off, val, owners, total, u32(job.shift), job.class_of_bin, job.n_bins, u32(job.n_classes), keys); }
    LAUNCH_CHECK("k_classes_keys");
    scratch.settled = false;
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(cub, keys_bytes, keys, sorted, size_t(total), 0, key_bits, st));
    HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(cub, rle_bytes, sorted, keys, lengths, n_entries, int(total), st));
    hipLaunchKernelGGL((wide ? k_classes_sign<true> : k_classes_sign<false>), dim3(grid_for(total)), dim3(TPB), 0, st, keys, lengths, n_entries, chunk.q0, values, sig, fold.span);
    LAUNCH_CHECK("k_classes_sign");
    return GCSA2_OK;
  });
  if(rc != GCSA2_OK) { return rc; }
  // 5. the votes
  return vote();
}

// gcsa2_kmer_classes_device after its argument checks (0 < n_patterns < 2^32): the search of gcsa2_kmer_support_device, with
// room for every window, so that it runs once; its records stay in arrival order, and what its wavefronts leave (SeedEmit's
// base and mask) is how a read finds them.
int kmer_classes_core(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 stride,
                      const ClassesJob& job, gcsa2_class_stats* st_out, hipStream_t st)
{
  Scratch scratch(ix, st);
  u64 *woff = nullptr, total = 0, m = 0;
  int rc = window_plan(scratch, d_offsets, n_patterns, k, stride, nullptr, "kmer_classes", st, woff, total);
  if(rc != GCSA2_OK) { return rc; }
  scratch.settled = true;
  st_out->windows = total;
  if(total == 0) { return classes_tail(ix, nullptr, 4, nullptr, nullptr, 0, true, woff, n_patterns, 0, nullptr, nullptr, job, st_out, scratch, st); }
  SeedEmit emit{};
  rc = kmer_seed_search(ix, scratch, d_patterns, d_offsets, n_patterns, k, stride, woff, total, total, nullptr, 1, st, emit, m);
  if(rc != GCSA2_OK) { return rc; }
  scratch.settled = true;
  if(m > emit.capacity) { return fail(GCSA2_ERR_HIP, "kmer_classes: more seeds than windows"); }
  return classes_tail(ix, emit.recs, 4, emit.counts, nullptr, m, true, woff, n_patterns, total, emit.base, emit.mask, job, st_out, scratch, st);
}

// gcsa2_kmer_classes_device and gcsa2_kmer_top_classes_device: `job` says which, `name` is the call's in its messages
int kmer_classes_entry(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, u64 k, u64 stride, const ClassesJob& job,
                       bool sparse, const char* name, gcsa2_class_stats* stats, void* stream)
{
  int rc = kmer_classes_checks(ix, k, stride, job.shift, job.flags, job.class_of_bin, job.n_bins, job.n_classes, "d_class_of_bin", job.top_n, sparse);
  if(rc != GCSA2_OK) { return rc; }
  if(n_patterns > 0 && d_offsets == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, std::string(name) + ": d_offsets is NULL"); }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, std::string(name) + ": 2^32 or more reads in one call; split the batch"); }
  return stats_entry(name, ix, stats, gcsa2_class_stats{}, n_patterns == 0, [&](gcsa2_class_stats& sums) -> int
  {
    return kmer_classes_core(ix, d_patterns, d_offsets, n_patterns, k, stride, job, &sums, static_cast<hipStream_t>(stream));
  });
}

// gcsa2_seed_classes_device and gcsa2_seed_top_classes_device, likewise
int seed_classes_entry(const gcsa2_index* ix, const uint64_t* d_group_offsets, u64 n_groups, const gcsa2_mem* d_seeds, u64 n_seeds, const uint64_t* d_weights,
                       const ClassesJob& job, bool sparse, const char* name, gcsa2_class_stats* stats, void* stream)
{
  int rc = classes_checks(ix, job.shift, job.flags, job.class_of_bin, job.n_bins, job.n_classes, "d_class_of_bin", job.top_n, sparse);
  if(rc != GCSA2_OK) { return rc; }
  if(n_groups > 0 && d_group_offsets == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, std::string(name) + ": d_group_offsets is NULL"); }
  if(n_seeds > 0 && d_seeds == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, std::string(name) + ": d_seeds is NULL"); }
  if(n_groups >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, std::string(name) + ": 2^32 or more groups in one call; split the batch"); }
  if(n_seeds >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, std::string(name) + ": 2^32 or more seeds in one call; split the batch"); }
  gcsa2_class_stats pre{};
  pre.windows = n_seeds;
  return stats_entry(name, ix, stats, pre, n_groups == 0, [&](gcsa2_class_stats& sums) -> int
  {
    hipStream_t st = static_cast<hipStream_t>(stream);
    static_assert(sizeof(gcsa2_mem) == 5 * sizeof(u64), "gcsa2_mem is five words");
    Scratch scratch(ix, st);
    return classes_tail(ix, reinterpret_cast<const u64*>(d_seeds), 5, nullptr, d_weights, n_seeds, false, d_group_offsets, n_groups, n_seeds, nullptr, nullptr,
                        job, &sums, scratch, st);
  });
}

// The host form.  The class map goes to the device once; each piece (for_read_pieces) is one gcsa2_kmer_classes_device on its
// thread's stream into device rows and calls of its own, which are copied to the piece's place in the caller's arrays: a row
// belongs to one read.
// Both host forms: the dense one (top_n == 0: rows = votes, n_classes u64 per read; records = calls) and the sparse one (rows =
// top, top_n gcsa2_class_vote per read; records = summaries).
int classes_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, u64 n_patterns, u64 k, u64 stride, u64 hit_max, u64 shift,
                  int flags, const uint32_t* class_of_bin, u64 n_bins, u64 n_classes, bool sparse, u64 top_n, void* rows, void* records,
                  gcsa2_class_stats* stats, const char* name)
{
  int rc = kmer_classes_checks(ix, k, stride, shift, flags, class_of_bin, n_bins, n_classes, "class_of_bin", top_n, sparse);
  if(rc != GCSA2_OK) { return rc; }
  if(n_patterns >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "kmer_classes: 2^32 or more reads in one call; split the batch"); }
  gcsa2_class_stats sums{};
  if(n_patterns == 0) { if(stats != nullptr) { *stats = sums; } return GCSA2_OK; }
  if(offsets == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "kmer_classes: offsets is NULL"); }
  rc = reads_ok(patterns, offsets, n_patterns, "kmer_classes");
  if(rc != GCSA2_OK) { return rc; }
  const u64 row_bytes = (sparse ? top_n * sizeof(gcsa2_class_vote) : n_classes * sizeof(u64));
  const u64 record_bytes = (sparse ? sizeof(gcsa2_top_summary) : sizeof(gcsa2_class_call));
  try {   // no C++ exception may cross the C boundary
  g_error.clear();
  if(host_windows(offsets, n_patterns, k, stride) >= (u64(1) << 32)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "kmer_classes: 2^32 or more windows in one call; split the batch"); }
  DeviceGuard guard(ix->device);
  DBuf<u32> d_map;
  HIP_TRY(d_map.alloc(n_bins));
  if(n_bins > 0) { HIP_TRY(hipMemcpy(d_map.p, class_of_bin, n_bins * sizeof(u32), hipMemcpyHostToDevice)); }
  const std::vector<u64> cut = read_cut(ix, offsets, n_patterns);
  std::vector<gcsa2_class_stats> done(cut.size() - 1);
  rc = for_read_pieces(ix, offsets, cut, [&](const ReadPiece& p, Outcome& out) -> bool
  {
    DBuf<u8> d_pat, d_rows, d_records; DBuf<u64> d_off;
    if(!upload_reads(p, patterns, d_pat, d_off, out)) { return false; }
    hipError_t e = (rows != nullptr ? d_rows.alloc(p.count * row_bytes) : hipSuccess);
    if(e == hipSuccess && records != nullptr) { e = d_records.alloc(p.count * record_bytes); }
    if(e != hipSuccess) { out.hip_error("upload of a piece", e); return false; }
    const int piece_rc = (sparse ? gcsa2_kmer_top_classes_device(ix, d_pat.p, d_off.p, p.count, k, stride, hit_max, shift, flags, d_map.p, n_bins, n_classes, top_n,
                                                                 reinterpret_cast<gcsa2_class_vote*>(d_rows.p), reinterpret_cast<gcsa2_top_summary*>(d_records.p),
                                                                 &done[p.c], p.stream)
                                 : gcsa2_kmer_classes_device(ix, d_pat.p, d_off.p, p.count, k, stride, hit_max, shift, flags, d_map.p, n_bins, n_classes,
                                                             reinterpret_cast<u64*>(d_rows.p), reinterpret_cast<gcsa2_class_call*>(d_records.p), &done[p.c], p.stream));
    if(piece_rc != GCSA2_OK) { out.set(piece_rc, g_error); return false; }
    if(rows != nullptr) { e = hipMemcpy(static_cast<u8*>(rows) + p.b * row_bytes, d_rows.p, p.count * row_bytes, hipMemcpyDeviceToHost); }
    if(e == hipSuccess && records != nullptr) { e = hipMemcpy(static_cast<u8*>(records) + p.b * record_bytes, d_records.p, p.count * record_bytes, hipMemcpyDeviceToHost); }
    if(e != hipSuccess) { out.hip_error("download of a piece", e); return false; }
    return true;
  });
  if(rc != GCSA2_OK) { return rc; }
  for(const gcsa2_class_stats& s : done) { sum_stats(sums, s); }
  if(stats != nullptr) { *stats = sums; }
  return GCSA2_OK;
  } catch(const std::exception& e) { return fail(GCSA2_ERR_OUT_OF_MEMORY, std::string(name) + ": " + e.what()); }
}

}  // namespace

extern "C" {

int gcsa2_kmer_classes_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k,
                              uint64_t stride, uint64_t hit_max, uint64_t shift, int flags, const uint32_t* d_class_of_bin, uint64_t n_bins,
                              uint64_t n_classes, uint64_t* d_votes, gcsa2_class_call* d_calls, gcsa2_class_stats* stats, void* stream)
{
  const ClassesJob job{hit_max, shift, flags, d_class_of_bin, n_bins, n_classes, d_votes, d_calls, 0, nullptr, nullptr};
  return kmer_classes_entry(ix, d_patterns, d_offsets, n_patterns, k, stride, job, false, "kmer_classes", stats, stream);
}

int gcsa2_seed_classes_device(const gcsa2_index* ix, const uint64_t* d_group_offsets, uint64_t n_groups, const gcsa2_mem* d_seeds, uint64_t n_seeds,
                              const uint64_t* d_weights, uint64_t hit_max, uint64_t shift, int flags, const uint32_t* d_class_of_bin,
                              uint64_t n_bins, uint64_t n_classes, uint64_t* d_votes, gcsa2_class_call* d_calls, gcsa2_class_stats* stats,
                              void* stream)
{
  const ClassesJob job{hit_max, shift, flags, d_class_of_bin, n_bins, n_classes, d_votes, d_calls, 0, nullptr, nullptr};
  return seed_classes_entry(ix, d_group_offsets, n_groups, d_seeds, n_seeds, d_weights, job, false, "seed_classes", stats, stream);
}

int gcsa2_kmer_classes_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k,
                             uint64_t stride, uint64_t hit_max, uint64_t shift, int flags, const uint32_t* class_of_bin, uint64_t n_bins,
                             uint64_t n_classes, uint64_t* votes, gcsa2_class_call* calls, gcsa2_class_stats* stats)
{
  return classes_batch(ix, patterns, offsets, n_patterns, k, stride, hit_max, shift, flags, class_of_bin, n_bins, n_classes, false, 0, votes, calls, stats,
                       "gcsa2_kmer_classes_batch");
}

// ---- the sparse form: per read the top_n classes with the most votes, for any number of classes (k_classes_top) ----
int gcsa2_kmer_top_classes_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k,
                                  uint64_t stride, uint64_t hit_max, uint64_t shift, int flags, const uint32_t* d_class_of_bin, uint64_t n_bins,
                                  uint64_t n_classes, uint64_t top_n, gcsa2_class_vote* d_top, gcsa2_top_summary* d_summaries,
                                  gcsa2_class_stats* stats, void* stream)
{
  const ClassesJob job{hit_max, shift, flags, d_class_of_bin, n_bins, n_classes, nullptr, nullptr, top_n, d_top, d_summaries};
  return kmer_classes_entry(ix, d_patterns, d_offsets, n_patterns, k, stride, job, true, "kmer_top_classes", stats, stream);
}

int gcsa2_kmer_top_classes_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k,
                                 uint64_t stride, uint64_t hit_max, uint64_t shift, int flags, const uint32_t* class_of_bin, uint64_t n_bins,
                                 uint64_t n_classes, uint64_t top_n, gcsa2_class_vote* top, gcsa2_top_summary* summaries, gcsa2_class_stats* stats)
{
  return classes_batch(ix, patterns, offsets, n_patterns, k, stride, hit_max, shift, flags, class_of_bin, n_bins, n_classes, true, top_n, top, summaries, stats,
                       "gcsa2_kmer_top_classes_batch");
}

int gcsa2_seed_top_classes_device(const gcsa2_index* ix, const uint64_t* d_group_offsets, uint64_t n_groups, const gcsa2_mem* d_seeds, uint64_t n_seeds,
                                  const uint64_t* d_weights, uint64_t hit_max, uint64_t shift, int flags, const uint32_t* d_class_of_bin,
                                  uint64_t n_bins, uint64_t n_classes, uint64_t top_n, gcsa2_class_vote* d_top, gcsa2_top_summary* d_summaries,
                                  gcsa2_class_stats* stats, void* stream)
{
  const ClassesJob job{hit_max, shift, flags, d_class_of_bin, n_bins, n_classes, nullptr, nullptr, top_n, d_top, d_summaries};
  return seed_classes_entry(ix, d_group_offsets, n_groups, d_seeds, n_seeds, d_weights, job, true, "seed_top_classes", stats, stream);
}

}  // extern "C"

// ==== groups of placed anchors: the plan, the launch shapes and the entry points that seed clusters and seed chains share ====
#include "host_anchors.hpp"

// ==== seed clusters: per read (or group of seed records) the top diagonal bands of its anchors (kernels_clusters.hpp) ====
namespace {

// what a clusters call places with and writes
struct ClustersJob
{
  u64 shift; const u64* coord_of_bin; u64 n_bins, band, top_n;
  gcsa2_cluster* top; gcsa2_cluster_summary* summaries;
};

// what every form refuses before any device is touched (`what` and `limit`: "chains" and its limit's name for the chain calls,
// which share these refusals)
int clusters_checks(const gcsa2_index* ix, u64 shift, const void* coord_of_bin, u64 n_bins, u64 top_n, const char* map_name, const char* what = "clusters",
                    const char* limit = "GCSA2_CLUSTER_TOP_LIMIT")
{
  CHECK_INDEX(ix);
  const std::string head = std::string(what) + ": ";
  if(top_n == 0 || top_n > GCSA2_CLUSTER_TOP_LIMIT) { return fail(GCSA2_ERR_INVALID_ARGUMENT, head + "top_n must be 1 .. " + limit + " (64)"); }
  if(shift >= 64) { return fail(GCSA2_ERR_INVALID_ARGUMENT, head + "shift must be below 64"); }
  if(n_bins == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, head + "n_bins must be at least 1"); }
  if(coord_of_bin == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, head + map_name + " is NULL"); }
  return GCSA2_OK;
}

// The cluster core.  n_groups >= 1; n_groups, n_seeds, n_hits < 2^32.  Writes every row and summary and fills every field of
// *out but `groups`.  One host round trip (anchors_plan: the largest group in LDS sizes the launch, the anchors above the
// capacity size the large path), then the end.  Scratch: 16 bytes per group; for the large path 8 bytes per group and 92
// bytes per anchor of a group above the capacity, and hipCUB's.
int clusters_core(const gcsa2_index* ix, const u64* goff, u64 n_groups, const gcsa2_mem* seeds, u64 n_seeds, const u64* hoff, const u64* hits, u64 n_hits,
                  const ClustersJob& job, gcsa2_cluster_stats* out, Scratch& scratch, hipStream_t st)
{
  static_assert(sizeof(gcsa2_mem) == 5 * sizeof(u64), "gcsa2_mem is five words");
  const u64* recs = reinterpret_cast<const u64*>(seeds);
  const CluMap map{u32(job.shift), job.coord_of_bin, job.n_bins};
  const u32 cap = cluster_capacity("GCSA2_CLUSTER_LDS"), top_n = u32(job.top_n);
  AnchorPlan plan;
  int rc = anchors_plan(ix, goff, n_groups, n_seeds, hoff, n_hits, cap, "clusters", plan, scratch, st);
  if(rc != GCSA2_OK) { return rc; }
  rc = anchors_lds_launches(ix, n_groups, plan.most, cap, reinterpret_cast<const void*>(&k_clusters_lds<TPB>), "k_clusters_lds",
                            [&](auto width, dim3 grid, size_t lds, u32 fit, u64 above, u64 spill)
  {
    constexpr u32 T = decltype(width)::value;
    hipLaunchKernelGGL((k_clusters_lds<T>), grid, dim3(T), lds, st, goff, n_groups, recs, hoff, hits, plan.info, map, job.band, top_n, fit, above, spill, job.top,
                       job.summaries, plan.stat);
  });
  if(rc != GCSA2_OK) { return rc; }
  // the groups above the capacity
  if(const u64 count = plan.count)
  {
    u64 *loff = nullptr, *dk = nullptr, *pe = nullptr, *gk = nullptr, *ka = nullptr, *kb = nullptr, *sdk = nullptr, *spe = nullptr, *sgk = nullptr;
    u64 *key2 = nullptr, *ends = nullptr, *reach = nullptr;
    u32 *pa = nullptr, *pb = nullptr;
    char* tmp = nullptr;
    size_t bytes = 0;
    rc = anchors_large_offsets(plan, n_groups, loff, tmp, bytes, scratch, st, [&](size_t& most) -> int
    {
      HIP_TRY(scratch.get(dk, count)); HIP_TRY(scratch.get(pe, count)); HIP_TRY(scratch.get(gk, count));
      HIP_TRY(scratch.get(ka, count)); HIP_TRY(scratch.get(kb, count));
      HIP_TRY(scratch.get(sdk, count)); HIP_TRY(scratch.get(spe, count)); HIP_TRY(scratch.get(sgk, count));
      HIP_TRY(scratch.get(key2, count)); HIP_TRY(scratch.get(ends, count)); HIP_TRY(scratch.get(reach, count));
      HIP_TRY(scratch.get(pa, count)); HIP_TRY(scratch.get(pb, count));
      size_t need = 0;
      HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need, dk, ka, pa, pb, size_t(count), 0, 64, st)); most = std::max(most, need);
      HIP_TRY(hipcub::DeviceScan::InclusiveScan(nullptr, need, ka, kb, hipcub::Max(), size_t(count), st)); most = std::max(most, need);
      HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, need, ka, kb, size_t(count), st)); most = std::max(most, need);
      return GCSA2_OK;
    });
    if(rc != GCSA2_OK) { return rc; }
    const dim3 lanes(grid_for(count));
    hipLaunchKernelGGL((k_anchors_large_gather<clu_place>), lanes, dim3(TPB), 0, st, loff, n_groups, count, goff, recs, hoff, hits, map, dk, pe, gk, pa);
    LAUNCH_CHECK("k_anchors_large_gather");
    // by (group, unplaced, diagonal): the diagonal first, then a stable sort by the group word
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, dk, ka, pa, pb, size_t(count), 0, 64, st));                     // pb: by diagonal
    hipLaunchKernelGGL(k_clusters_large_take, lanes, dim3(TPB), 0, st, gk, pb, count, ka);
    LAUNCH_CHECK("k_clusters_large_take");
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, ka, sgk, pb, pa, size_t(count), 0, 34, st));                    // sgk, pa: by (group, diagonal)
    hipLaunchKernelGGL(k_clusters_large_take, lanes, dim3(TPB), 0, st, dk, pa, count, sdk);
    LAUNCH_CHECK("k_clusters_large_take");
    hipLaunchKernelGGL(k_clusters_large_take, lanes, dim3(TPB), 0, st, pe, pa, count, spe);
    LAUNCH_CHECK("k_clusters_large_take");
    // the cluster of every anchor, then (cluster, position) order
    hipLaunchKernelGGL(k_clusters_large_heads, lanes, dim3(TPB), 0, st, sdk, sgk, count, job.band, ka);
    LAUNCH_CHECK("k_clusters_large_heads");
    HIP_TRY(hipcub::DeviceScan::InclusiveScan(tmp, bytes, ka, kb, hipcub::Max(), size_t(count), st));                       // kb: the head of every anchor
    hipLaunchKernelGGL(k_clusters_large_keys, lanes, dim3(TPB), 0, st, kb, spe, sgk, count, ka, pa);
    LAUNCH_CHECK("k_clusters_large_keys");
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, ka, key2, pa, pb, size_t(count), 0, 64, st));
    // the running end, then covered and starts as one wrapping sum
    hipLaunchKernelGGL(k_clusters_large_ends, lanes, dim3(TPB), 0, st, key2, pb, spe, sgk, count, ends);
    LAUNCH_CHECK("k_clusters_large_ends");
    HIP_TRY(hipcub::DeviceScan::InclusiveScan(tmp, bytes, ends, reach, hipcub::Max(), size_t(count), st));
    hipLaunchKernelGGL(k_clusters_large_cover, lanes, dim3(TPB), 0, st, key2, ends, reach, sgk, count, ka);
    LAUNCH_CHECK("k_clusters_large_cover");
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(tmp, bytes, ka, kb, size_t(count), st));
    const dim3 grid(unsigned(std::min<u64>(n_groups, u64(ix->compute_units) * 8)));
    hipLaunchKernelGGL(k_clusters_large_score, grid, dim3(TPB), 0, st, loff, plan.lsize, n_groups, sdk, spe, sgk, key2, kb, top_n, job.top, job.summaries, plan.stat);
    LAUNCH_CHECK("k_clusters_large_score");
  }
  return anchors_tail(plan, out, &gcsa2_cluster_stats::clusters, scratch, st);
}

// the fused cluster forms
int fused_clusters_entry(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, const AnchorWindows& win,
                         const ClustersJob& job, const char* name, gcsa2_cluster_stats* stats, void* stream)
{
  return fused_anchors_entry(ix, d_patterns, d_offsets, n_patterns, win, job, name, "clusters",
                             [&] { return clusters_checks(ix, job.shift, job.coord_of_bin, job.n_bins, job.top_n, "d_coord_of_bin"); }, clusters_core, stats, stream);
}

// both host forms: the top rows and the summaries of every piece
int clusters_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, u64 n_patterns, const AnchorWindows& win, u64 shift,
                   const uint64_t* coord_of_bin, u64 n_bins, u64 band, u64 top_n, gcsa2_cluster* top, gcsa2_cluster_summary* summaries, gcsa2_cluster_stats* stats,
                   const char* name)
{
  const PieceOutput outs[] = {{top, top_n, sizeof(gcsa2_cluster)}, {summaries, 1, sizeof(gcsa2_cluster_summary)}};
  return anchors_batch(ix, patterns, offsets, n_patterns, win, coord_of_bin, n_bins, outs, stats, name,
                       [&] { return clusters_checks(ix, shift, coord_of_bin, n_bins, top_n, "coord_of_bin"); },
                       [&](const ReadPiece& p, const u8* d_pat, const u64* d_off, const u64* d_map, void* const* d, gcsa2_cluster_stats* done) -> int
  {
    gcsa2_cluster* d_top = static_cast<gcsa2_cluster*>(d[0]);
    gcsa2_cluster_summary* d_sum = static_cast<gcsa2_cluster_summary*>(d[1]);
    return (win.minimizers ? gcsa2_minimizer_clusters_device(ix, d_pat, d_off, p.count, win.k, win.w, win.hash_seed, win.hit_max, win.over, shift, d_map, n_bins, band,
                                                             top_n, d_top, d_sum, done, p.stream)
                           : gcsa2_kmer_clusters_device(ix, d_pat, d_off, p.count, win.k, win.stride, win.hit_max, win.over, shift, d_map, n_bins, band, top_n, d_top,
                                                        d_sum, done, p.stream));
  });
}

}  // namespace

extern "C" {

int gcsa2_seed_clusters_device(const gcsa2_index* ix, const uint64_t* d_group_offsets, uint64_t n_groups, const gcsa2_mem* d_seeds, uint64_t n_seeds,
                               const uint64_t* d_hit_offsets, const uint64_t* d_hits, uint64_t n_hits, uint64_t shift, const uint64_t* d_coord_of_bin,
                               uint64_t n_bins, uint64_t band, uint64_t top_n, gcsa2_cluster* d_top, gcsa2_cluster_summary* d_summaries,
                               gcsa2_cluster_stats* stats, void* stream)
{
  int rc = clusters_checks(ix, shift, d_coord_of_bin, n_bins, top_n, "d_coord_of_bin");
  if(rc != GCSA2_OK) { return rc; }
  rc = seed_form_checks("seed_clusters", d_group_offsets, n_groups, d_seeds, n_seeds, d_hit_offsets, d_hits, n_hits);
  if(rc != GCSA2_OK) { return rc; }
  gcsa2_cluster_stats pre{};
  pre.groups = n_groups;
  return stats_entry("seed_clusters", ix, stats, pre, n_groups == 0, [&](gcsa2_cluster_stats& sums) -> int
  {
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scratch scratch(ix, st);
    const ClustersJob job{shift, d_coord_of_bin, n_bins, band, top_n, d_top, d_summaries};
    return clusters_core(ix, d_group_offsets, n_groups, d_seeds, n_seeds, d_hit_offsets, d_hits, n_hits, job, &sums, scratch, st);
  });
}

int gcsa2_kmer_clusters_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k, uint64_t stride,
                               uint64_t hit_max, int over, uint64_t shift, const uint64_t* d_coord_of_bin, uint64_t n_bins, uint64_t band, uint64_t top_n,
                               gcsa2_cluster* d_top, gcsa2_cluster_summary* d_summaries, gcsa2_cluster_stats* stats, void* stream)
{
  const ClustersJob job{shift, d_coord_of_bin, n_bins, band, top_n, d_top, d_summaries};
  return fused_clusters_entry(ix, d_patterns, d_offsets, n_patterns, AnchorWindows{k, stride, false, 0, 0, hit_max, over}, job, "kmer_clusters", stats, stream);
}

int gcsa2_minimizer_clusters_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k, uint64_t w,
                                    uint64_t hash_seed, uint64_t hit_max, int over, uint64_t shift, const uint64_t* d_coord_of_bin, uint64_t n_bins,
                                    uint64_t band, uint64_t top_n, gcsa2_cluster* d_top, gcsa2_cluster_summary* d_summaries, gcsa2_cluster_stats* stats,
                                    void* stream)
{
  const ClustersJob job{shift, d_coord_of_bin, n_bins, band, top_n, d_top, d_summaries};
  return fused_clusters_entry(ix, d_patterns, d_offsets, n_patterns, AnchorWindows{k, 1, true, w, hash_seed, hit_max, over}, job, "minimizer_clusters", stats, stream);
}

int gcsa2_kmer_clusters_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k, uint64_t stride,
                              uint64_t hit_max, int over, uint64_t shift, const uint64_t* coord_of_bin, uint64_t n_bins, uint64_t band, uint64_t top_n,
                              gcsa2_cluster* top, gcsa2_cluster_summary* summaries, gcsa2_cluster_stats* stats)
{
  return clusters_batch(ix, patterns, offsets, n_patterns, AnchorWindows{k, stride, false, 0, 0, hit_max, over}, shift, coord_of_bin, n_bins, band, top_n, top,
                        summaries, stats, "gcsa2_kmer_clusters_batch");
}

int gcsa2_minimizer_clusters_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k, uint64_t w,
                                   uint64_t hash_seed, uint64_t hit_max, int over, uint64_t shift, const uint64_t* coord_of_bin, uint64_t n_bins, uint64_t band,
                                   uint64_t top_n, gcsa2_cluster* top, gcsa2_cluster_summary* summaries, gcsa2_cluster_stats* stats)
{
  return clusters_batch(ix, patterns, offsets, n_patterns, AnchorWindows{k, 1, true, w, hash_seed, hit_max, over}, shift, coord_of_bin, n_bins, band, top_n, top,
                        summaries, stats, "gcsa2_minimizer_clusters_batch");
}

}  // extern "C"

// ==== seed chains: per read (or group of seed records) the top colinear chains of its anchors (kernels_chains.hpp) ====
namespace {

// what a chains call places with, chains with and writes
struct ChainsJob
{
  u64 shift; const u64* coord_of_bin; u64 n_bins;
  const gcsa2_chain_params* params;
  gcsa2_chain* top; gcsa2_chain_anchor* members; gcsa2_chain_summary* summaries;
};

// what every form refuses before any device is touched: the refusals of the cluster calls and those of the parameters
int chains_checks(const gcsa2_index* ix, u64 shift, const void* coord_of_bin, u64 n_bins, const gcsa2_chain_params* p, const char* map_name)
{
  CHECK_INDEX(ix);
  if(p == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chains: params is NULL"); }
  const int rc = clusters_checks(ix, shift, coord_of_bin, n_bins, p->top_n, map_name, "chains", "GCSA2_CHAIN_TOP_LIMIT");
  if(rc != GCSA2_OK) { return rc; }
  if(p->lookback == 0 || p->lookback > GCSA2_CHAIN_LOOKBACK_LIMIT) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chains: lookback must be 1 .. GCSA2_CHAIN_LOOKBACK_LIMIT (64)"); }
  if(p->match == 0 || p->match > 65536) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chains: match must be 1 .. 65536"); }
  if(p->gap > 65536) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chains: gap must be at most 65536"); }
  if(p->max_gap == 0 || p->max_gap >= (u64(1) << 32)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chains: max_gap must be 1 .. 2^32 - 1"); }
  if(p->min_score >= (u64(1) << 62)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chains: min_score must be below 2^62"); }
  return GCSA2_OK;
}

// member_cap > 0 with n_groups top_n member_cap >= 2^32 (top_n is 1 .. 64 here; no product is formed that could wrap)
int chains_member_check(const gcsa2_chain_params* p, u64 n_groups)
{
  if(p->member_cap > 0 && n_groups > 0 && p->member_cap > (u64(0xFFFFFFFF) / p->top_n) / n_groups)
  {
    return fail(GCSA2_ERR_INVALID_ARGUMENT, "chains: member_cap: n_groups x top_n x member_cap must be below 2^32");
  }
  return GCSA2_OK;
}

// The chain core, on the skeleton of clusters_core.  n_groups >= 1; n_groups, n_seeds, n_hits < 2^32.  Writes every row, member
// row and summary and fills every field of *out but `groups`.  One host round trip (anchors_plan), then the end.  Scratch:
// 16 bytes per group; for the large path 8 bytes per group and 80 bytes per anchor of a group above the capacity, and hipCUB's.
int chains_core(const gcsa2_index* ix, const u64* goff, u64 n_groups, const gcsa2_mem* seeds, u64 n_seeds, const u64* hoff, const u64* hits, u64 n_hits,
                const ChainsJob& job, gcsa2_chain_stats* out, Scratch& scratch, hipStream_t st)
{
  const u64* recs = reinterpret_cast<const u64*>(seeds);
  const CluMap map{u32(job.shift), job.coord_of_bin, job.n_bins};
  const gcsa2_chain_params& p = *job.params;
  const ChnParams P{p.band, p.max_gap, p.match, p.gap, p.min_score, p.member_cap, u32(p.lookback), u32(p.top_n)};
  gcsa2_chain_anchor* members = (p.member_cap > 0 ? job.members : nullptr);
  const u32 cap = cluster_capacity("GCSA2_CHAIN_LDS");
  AnchorPlan plan;
  int rc = anchors_plan(ix, goff, n_groups, n_seeds, hoff, n_hits, cap, "chains", plan, scratch, st);
  if(rc != GCSA2_OK) { return rc; }
  rc = anchors_lds_launches(ix, n_groups, plan.most, cap, reinterpret_cast<const void*>(&k_chains_lds<TPB>), "k_chains_lds",
                            [&](auto width, dim3 grid, size_t lds, u32 fit, u64 above, u64 spill)
  {
    constexpr u32 T = decltype(width)::value;
    hipLaunchKernelGGL((k_chains_lds<T>), grid, dim3(T), lds, st, goff, n_groups, recs, hoff, hits, plan.info, map, P, fit, above, spill, job.top, members,
                       job.summaries, plan.stat);
  });
  if(rc != GCSA2_OK) { return rc; }
  // the groups above the capacity
  if(const u64 count = plan.count)
  {
    u64 *loff = nullptr, *xs = nullptr, *pes = nullptr, *gk = nullptr, *ka = nullptr, *kb = nullptr, *sx = nullptr, *spe = nullptr, *sgk = nullptr;
    u32 *pa = nullptr, *pb = nullptr, *prd = nullptr, *mrk = nullptr;
    char* tmp = nullptr;
    size_t bytes = 0;
    rc = anchors_large_offsets(plan, n_groups, loff, tmp, bytes, scratch, st, [&](size_t& most) -> int
    {
      HIP_TRY(scratch.get(xs, count)); HIP_TRY(scratch.get(pes, count)); HIP_TRY(scratch.get(gk, count));
      HIP_TRY(scratch.get(ka, count)); HIP_TRY(scratch.get(kb, count));
      HIP_TRY(scratch.get(sx, count)); HIP_TRY(scratch.get(spe, count)); HIP_TRY(scratch.get(sgk, count));
      HIP_TRY(scratch.get(pa, count)); HIP_TRY(scratch.get(pb, count)); HIP_TRY(scratch.get(prd, count)); HIP_TRY(scratch.get(mrk, count));
      size_t need = 0;
      HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need, xs, ka, pa, pb, size_t(count), 0, 64, st)); most = std::max(most, need);
      return GCSA2_OK;
    });
    if(rc != GCSA2_OK) { return rc; }
    const dim3 lanes(grid_for(count));
    HIP_TRY(hipMemsetAsync(mrk, 0xFF, count * sizeof(u32), st));                                                           // CHN_NO: no anchor is used
    hipLaunchKernelGGL((k_anchors_large_gather<chn_place>), lanes, dim3(TPB), 0, st, loff, n_groups, count, goff, recs, hoff, hits, map, xs, pes, gk, pa);
    LAUNCH_CHECK("k_anchors_large_gather");
    // by (group, unplaced, x, q, l): q << 32 | qe first, then stable sorts by x and by the group word
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, pes, ka, pa, pb, size_t(count), 0, 64, st));                     // pb: by (q, l)
    hipLaunchKernelGGL(k_clusters_large_take, lanes, dim3(TPB), 0, st, xs, pb, count, ka);
    LAUNCH_CHECK("k_clusters_large_take");
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, ka, kb, pb, pa, size_t(count), 0, 64, st));                      // pa: by (x, q, l)
    hipLaunchKernelGGL(k_clusters_large_take, lanes, dim3(TPB), 0, st, gk, pa, count, ka);
    LAUNCH_CHECK("k_clusters_large_take");
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, ka, sgk, pa, pb, size_t(count), 0, 34, st));                     // sgk, pb: by (group, x, q, l)
    hipLaunchKernelGGL(k_clusters_large_take, lanes, dim3(TPB), 0, st, xs, pb, count, sx);
    LAUNCH_CHECK("k_clusters_large_take");
    hipLaunchKernelGGL(k_clusters_large_take, lanes, dim3(TPB), 0, st, pes, pb, count, spe);
    LAUNCH_CHECK("k_clusters_large_take");
    // f and pred, then the order of the visit: by (group, f descending, place), two stable sorts again
    const dim3 grid(unsigned(std::min<u64>(n_groups, u64(ix->compute_units) * 8)));
    hipLaunchKernelGGL(k_chains_large_dp, grid, dim3(64), 0, st, loff, plan.lsize, n_groups, sx, spe, sgk, P, ka, prd, pa);
    LAUNCH_CHECK("k_chains_large_dp");
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, ka, kb, pa, pb, size_t(count), 0, 51, st));                      // pb: by f descending
    hipLaunchKernelGGL(k_clusters_large_take, lanes, dim3(TPB), 0, st, sgk, pb, count, ka);
    LAUNCH_CHECK("k_clusters_large_take");
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, ka, kb, pb, pa, size_t(count), 0, 34, st));                      // pa: the order of the visit
    hipLaunchKernelGGL(k_chains_large_finish, grid, dim3(TPB), 0, st, loff, plan.lsize, n_groups, sx, spe, sgk, prd, mrk, pa, P, job.top, members, job.summaries,
                       plan.stat);
    LAUNCH_CHECK("k_chains_large_finish");
  }
  return anchors_tail(plan, out, &gcsa2_chain_stats::chains, scratch, st);
}

// the job's refusals of a fused or host form of n_groups reads
int chains_job_checks(const gcsa2_index* ix, u64 shift, const void* coord_of_bin, u64 n_bins, const gcsa2_chain_params* params, const char* map_name, u64 n_groups)
{
  const int rc = chains_checks(ix, shift, coord_of_bin, n_bins, params, map_name);
  return (rc != GCSA2_OK ? rc : chains_member_check(params, n_groups));
}

// the fused chain forms
int fused_chains_entry(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, u64 n_patterns, const AnchorWindows& win, const ChainsJob& job,
                       const char* name, gcsa2_chain_stats* stats, void* stream)
{
  return fused_anchors_entry(ix, d_patterns, d_offsets, n_patterns, win, job, name, "chains",
                             [&] { return chains_job_checks(ix, job.shift, job.coord_of_bin, job.n_bins, job.params, "d_coord_of_bin", n_patterns); }, chains_core,
                             stats, stream);
}

// both host forms: the top rows, the member rows (only if member_cap > 0) and the summaries of every piece
int chains_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, u64 n_patterns, const AnchorWindows& win, u64 shift,
                 const uint64_t* coord_of_bin, u64 n_bins, const gcsa2_chain_params* params, gcsa2_chain* top, gcsa2_chain_anchor* members,
                 gcsa2_chain_summary* summaries, gcsa2_chain_stats* stats, const char* name)
{
  const u64 top_n = (params != nullptr ? params->top_n : 0), member_cap = (params != nullptr ? params->member_cap : 0);
  const PieceOutput outs[] = {{top, top_n, sizeof(gcsa2_chain)}, {members, top_n * member_cap, sizeof(gcsa2_chain_anchor)}, {summaries, 1, sizeof(gcsa2_chain_summary)}};
  return anchors_batch(ix, patterns, offsets, n_patterns, win, coord_of_bin, n_bins, outs, stats, name,
                       [&] { return chains_job_checks(ix, shift, coord_of_bin, n_bins, params, "coord_of_bin", n_patterns); },
                       [&](const ReadPiece& p, const u8* d_pat, const u64* d_off, const u64* d_map, void* const* d, gcsa2_chain_stats* done) -> int
  {
    gcsa2_chain* d_top = static_cast<gcsa2_chain*>(d[0]);
    gcsa2_chain_anchor* d_mem = static_cast<gcsa2_chain_anchor*>(d[1]);
    gcsa2_chain_summary* d_sum = static_cast<gcsa2_chain_summary*>(d[2]);
    return (win.minimizers ? gcsa2_minimizer_chains_device(ix, d_pat, d_off, p.count, win.k, win.w, win.hash_seed, win.hit_max, win.over, shift, d_map, n_bins, params,
                                                           d_top, d_mem, d_sum, done, p.stream)
                           : gcsa2_kmer_chains_device(ix, d_pat, d_off, p.count, win.k, win.stride, win.hit_max, win.over, shift, d_map, n_bins, params, d_top, d_mem,
                                                      d_sum, done, p.stream));
  });
}

}  // namespace

extern "C" {

int gcsa2_seed_chains_device(const gcsa2_index* ix, const uint64_t* d_group_offsets, uint64_t n_groups, const gcsa2_mem* d_seeds, uint64_t n_seeds,
                             const uint64_t* d_hit_offsets, const uint64_t* d_hits, uint64_t n_hits, uint64_t shift, const uint64_t* d_coord_of_bin,
                             uint64_t n_bins, const gcsa2_chain_params* params, gcsa2_chain* d_top, gcsa2_chain_anchor* d_members,
                             gcsa2_chain_summary* d_summaries, gcsa2_chain_stats* stats, void* stream)
{
  int rc = chains_checks(ix, shift, d_coord_of_bin, n_bins, params, "d_coord_of_bin");
  if(rc != GCSA2_OK) { return rc; }
  rc = seed_form_checks("seed_chains", d_group_offsets, n_groups, d_seeds, n_seeds, d_hit_offsets, d_hits, n_hits);
  if(rc != GCSA2_OK) { return rc; }
  rc = chains_member_check(params, n_groups);
  if(rc != GCSA2_OK) { return rc; }
  gcsa2_chain_stats pre{};
  pre.groups = n_groups;
  return stats_entry("seed_chains", ix, stats, pre, n_groups == 0, [&](gcsa2_chain_stats& sums) -> int
  {
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scratch scratch(ix, st);
    const ChainsJob job{shift, d_coord_of_bin, n_bins, params, d_top, d_members, d_summaries};
    return chains_core(ix, d_group_offsets, n_groups, d_seeds, n_seeds, d_hit_offsets, d_hits, n_hits, job, &sums, scratch, st);
  });
}

int gcsa2_kmer_chains_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k, uint64_t stride,
                             uint64_t hit_max, int over, uint64_t shift, const uint64_t* d_coord_of_bin, uint64_t n_bins, const gcsa2_chain_params* params,
                             gcsa2_chain* d_top, gcsa2_chain_anchor* d_members, gcsa2_chain_summary* d_summaries, gcsa2_chain_stats* stats, void* stream)
{
  const ChainsJob job{shift, d_coord_of_bin, n_bins, params, d_top, d_members, d_summaries};
  return fused_chains_entry(ix, d_patterns, d_offsets, n_patterns, AnchorWindows{k, stride, false, 0, 0, hit_max, over}, job, "kmer_chains", stats, stream);
}

int gcsa2_minimizer_chains_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k, uint64_t w,
                                  uint64_t hash_seed, uint64_t hit_max, int over, uint64_t shift, const uint64_t* d_coord_of_bin, uint64_t n_bins,
                                  const gcsa2_chain_params* params, gcsa2_chain* d_top, gcsa2_chain_anchor* d_members, gcsa2_chain_summary* d_summaries,
                                  gcsa2_chain_stats* stats, void* stream)
{
  const ChainsJob job{shift, d_coord_of_bin, n_bins, params, d_top, d_members, d_summaries};
  return fused_chains_entry(ix, d_patterns, d_offsets, n_patterns, AnchorWindows{k, 1, true, w, hash_seed, hit_max, over}, job, "minimizer_chains", stats, stream);
}

int gcsa2_kmer_chains_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k, uint64_t stride,
                            uint64_t hit_max, int over, uint64_t shift, const uint64_t* coord_of_bin, uint64_t n_bins, const gcsa2_chain_params* params,
                            gcsa2_chain* top, gcsa2_chain_anchor* members, gcsa2_chain_summary* summaries, gcsa2_chain_stats* stats)
{
  return chains_batch(ix, patterns, offsets, n_patterns, AnchorWindows{k, stride, false, 0, 0, hit_max, over}, shift, coord_of_bin, n_bins, params, top, members,
                      summaries, stats, "gcsa2_kmer_chains_batch");
}

int gcsa2_minimizer_chains_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k, uint64_t w,
                                 uint64_t hash_seed, uint64_t hit_max, int over, uint64_t shift, const uint64_t* coord_of_bin, uint64_t n_bins,
                                 const gcsa2_chain_params* params, gcsa2_chain* top, gcsa2_chain_anchor* members, gcsa2_chain_summary* summaries,
                                 gcsa2_chain_stats* stats)
{
  return chains_batch(ix, patterns, offsets, n_patterns, AnchorWindows{k, 1, true, w, hash_seed, hit_max, over}, shift, coord_of_bin, n_bins, params, top, members,
                      summaries, stats, "gcsa2_minimizer_chains_batch");
}

}  // extern "C"

// ==== chain pairs: per read pair the top placements of two mates' chains under a fragment model (kernels_pairs.hpp) ====
namespace {

// what a pairs call writes
struct PairsJob { const gcsa2_pair_params* params; gcsa2_chain_pair* top; gcsa2_pair_summary* summaries; };

// what every form refuses of the pair parameters before any device is touched
int pairs_checks(const gcsa2_index* ix, const gcsa2_pair_params* p, u64 chain_top_n, u64 n_pairs)
{
  CHECK_INDEX(ix);
  if(p == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chain_pairs: params is NULL"); }
  if(p->orientation > GCSA2_PAIR_FF) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chain_pairs: orientation must be GCSA2_PAIR_FR, GCSA2_PAIR_RF or GCSA2_PAIR_FF"); }
  if(p->top_n == 0 || p->top_n > GCSA2_PAIR_TOP_LIMIT) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chain_pairs: top_n must be 1 .. GCSA2_PAIR_TOP_LIMIT (64)"); }
  if(chain_top_n == 0 || chain_top_n > GCSA2_PAIR_TOP_LIMIT) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chain_pairs: chain_top_n must be 1 .. GCSA2_PAIR_TOP_LIMIT (64)"); }
  if(p->min_fragment > p->max_fragment) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chain_pairs: min_fragment exceeds max_fragment"); }
  if(p->max_fragment >= (u64(1) << 32)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chain_pairs: max_fragment must be below 2^32"); }
  if(p->mean_fragment >= (u64(1) << 32)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chain_pairs: mean_fragment must be below 2^32"); }
  if(p->unit == 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chain_pairs: unit must be at least 1"); }
  if(p->cost > 65536) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chain_pairs: cost must be at most 65536"); }
  if(p->min_score >= (u64(1) << 62)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chain_pairs: min_score must be below 2^62"); }
  if(n_pairs >= (u64(1) << 30)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chain_pairs: 2^30 or more pairs in one call; split the batch"); }
  return GCSA2_OK;
}

// The pair core.  0 < n_pairs < 2^30; `chains` holds 4 n_pairs rows of chain_top_n.  Writes every row and summary and fills every
// field of *out but `pairs`.  One kernel; the only host round trip is the counters' at the end.  Scratch: 56 bytes.
int pairs_core(const gcsa2_index* ix, const gcsa2_chain* chains, u64 n_pairs, u64 chain_top_n, const PairsJob& job, gcsa2_pair_stats* out, Scratch& scratch,
               hipStream_t st)
{
  const gcsa2_pair_params& p = *job.params;
  const PairParams P{p.min_fragment, p.max_fragment, p.mean_fragment, p.unit, p.cost, p.min_score, u32(p.top_n), u32(chain_top_n)};
  unsigned long long* stat = nullptr;
  HIP_TRY(scratch.get(stat, PAIR_WORDS));
  HIP_TRY(hipMemsetAsync(stat, 0, PAIR_WORDS * sizeof(unsigned long long), st));
  scratch.settled = false;
  const bool aligned = ((reinterpret_cast<uintptr_t>(chains) | reinterpret_cast<uintptr_t>(job.top)) & 15) == 0;
  const dim3 grid(unsigned(std::min<u64>((n_pairs + 3) / 4, u64(ix->compute_units) * 8)));
  const u64* rows = reinterpret_cast<const u64*>(chains);
  u64 *top = reinterpret_cast<u64*>(job.top), *summaries = reinterpret_cast<u64*>(job.summaries);
  if(p.orientation == GCSA2_PAIR_FR) { hipLaunchKernelGGL(k_chain_pairs<GCSA2_PAIR_FR>, grid, dim3(TPB), 0, st, rows, n_pairs, P, aligned, top, summaries, stat); }
  else if(p.orientation == GCSA2_PAIR_RF) { hipLaunchKernelGGL(k_chain_pairs<GCSA2_PAIR_RF>, grid, dim3(TPB), 0, st, rows, n_pairs, P, aligned, top, summaries, stat); }
  else { hipLaunchKernelGGL(k_chain_pairs<GCSA2_PAIR_FF>, grid, dim3(TPB), 0, st, rows, n_pairs, P, aligned, top, summaries, stat); }
  LAUNCH_CHECK("k_chain_pairs");
  unsigned long long host_stat[PAIR_WORDS];
  HIP_TRY(hipMemcpyAsync(host_stat, stat, sizeof(host_stat), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  scratch.settled = true;
  out->candidates = host_stat[PAIR_CANDIDATES]; out->proper = host_stat[PAIR_PROPER]; out->kept = host_stat[PAIR_KEPT]; out->ignored = host_stat[PAIR_IGNORED];
  out->paired = host_stat[PAIR_PAIRED]; out->unique = host_stat[PAIR_UNIQUE]; out->unique_fragment_sum = host_stat[PAIR_FRAGMENT_SUM];
  return GCSA2_OK;
}

// what both fused forms refuse before any device is touched: the refusals of the chain calls, of the pair call and of the
// stranded hits call -- the components it needs last -- and an odd number of reads
int fused_pairs_checks(const gcsa2_index* ix, u64 n_patterns, u64 k, u64 w, int over, u64 shift, const void* coord_of_bin, u64 n_bins,
                       const gcsa2_chain_params* chain_params, const gcsa2_pair_params* pair_params, const char* map_name)
{
  CHECK_INDEX(ix);
  const u64 n_groups = (n_patterns < (u64(1) << 32) ? 2 * n_patterns : 0);          // (beyond: the refusal of the reads below)
  int rc = chains_job_checks(ix, shift, coord_of_bin, n_bins, chain_params, map_name, n_groups);
  if(rc != GCSA2_OK) { return rc; }
  rc = pairs_checks(ix, pair_params, chain_params->top_n, 0);
  if(rc != GCSA2_OK) { return rc; }
  if(n_patterns % 2 != 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "minimizer_chain_pairs: n_patterns must be even: the mates of pair p are the reads 2p and 2p + 1"); }
  const u64 unused = 0;
  rc = stranded_hits_checks(ix, k, w, GCSA2_STRAND_BOTH, over, &unused, &unused);
  if(rc != GCSA2_OK) { return rc; }
  if(n_patterns >= (u64(1) << 31)) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "minimizer_chain_pairs: 2^31 or more reads in one call; split the batch"); }
  return GCSA2_OK;
}

// the statistics of a host form's piece, summed side by side (sum_stats)
struct PairBatchStats { gcsa2_chain_stats chains; gcsa2_pair_stats pairs; };
static_assert(sizeof(PairBatchStats) == 15 * sizeof(uint64_t), "sum_stats: a struct of uint64_t counters and nothing else");

}  // namespace

extern "C" {

int gcsa2_chain_pairs_device(const gcsa2_index* ix, const gcsa2_chain* d_chains, uint64_t n_pairs, uint64_t chain_top_n, const gcsa2_pair_params* params,
                             gcsa2_chain_pair* d_top, gcsa2_pair_summary* d_summaries, gcsa2_pair_stats* stats, void* stream)
{
  const int rc = pairs_checks(ix, params, chain_top_n, n_pairs);
  if(rc != GCSA2_OK) { return rc; }
  if(n_pairs > 0 && d_chains == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "chain_pairs: d_chains is NULL"); }
  gcsa2_pair_stats pre{};
  pre.pairs = n_pairs;
  return stats_entry("chain_pairs", ix, stats, pre, n_pairs == 0, [&](gcsa2_pair_stats& sums) -> int
  {
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scratch scratch(ix, st);
    return pairs_core(ix, d_chains, n_pairs, chain_top_n, PairsJob{params, d_top, d_summaries}, &sums, scratch, st);
  });
}

int gcsa2_minimizer_chain_pairs_device(const gcsa2_index* ix, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns, uint64_t k, uint64_t w,
                                       uint64_t hash_seed, uint64_t hit_max, int over, uint64_t shift, const uint64_t* d_coord_of_bin, uint64_t n_bins,
                                       const gcsa2_chain_params* chain_params, const gcsa2_pair_params* pair_params, gcsa2_chain* d_chains,
                                       gcsa2_chain_anchor* d_members, gcsa2_chain_summary* d_chain_summaries, gcsa2_chain_pair* d_top,
                                       gcsa2_pair_summary* d_summaries, gcsa2_chain_stats* chain_stats, gcsa2_pair_stats* pair_stats, void* stream)
{
  const int rc = fused_pairs_checks(ix, n_patterns, k, w, over, shift, d_coord_of_bin, n_bins, chain_params, pair_params, "d_coord_of_bin");
  if(rc != GCSA2_OK) { return rc; }
  if(n_patterns > 0 && d_offsets == nullptr) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "minimizer_chain_pairs: d_offsets is NULL"); }
  PairBatchStats pre{}, both{};
  pre.chains.groups = 2 * n_patterns; pre.pairs.pairs = n_patterns / 2;
  const int run = stats_entry("minimizer_chain_pairs", ix, &both, pre, n_patterns == 0, [&](PairBatchStats& sums) -> int
  {
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scratch scratch(ix, st);
    const u64 n_groups = 2 * n_patterns, top_n = chain_params->top_n;
    FusedHits f;
    int step = fused_stranded_hits(ix, scratch, d_patterns, d_offsets, n_patterns, k, w, hash_seed, hit_max, over, "minimizer_chain_pairs", "chains", f, st);
    if(step != GCSA2_OK) { return step; }
    gcsa2_chain* rows = d_chains;
    if(rows == nullptr) { HIP_TRY(scratch.get(rows, n_groups * top_n)); }
    const ChainsJob job{shift, d_coord_of_bin, n_bins, chain_params, rows, d_members, d_chain_summaries};
    step = chains_core(ix, f.seed_off, n_groups, f.seeds, f.m, f.hit_off, f.hit_values, f.h, job, &sums.chains, scratch, st);
    if(step != GCSA2_OK) { return step; }
    return pairs_core(ix, rows, n_patterns / 2, top_n, PairsJob{pair_params, d_top, d_summaries}, &sums.pairs, scratch, st);
  });
  if(run != GCSA2_OK) { return run; }
  if(chain_stats != nullptr) { *chain_stats = both.chains; }
  if(pair_stats != nullptr) { *pair_stats = both.pairs; }
  return GCSA2_OK;
}

int gcsa2_minimizer_chain_pairs_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns, uint64_t k, uint64_t w,
                                      uint64_t hash_seed, uint64_t hit_max, int over, uint64_t shift, const uint64_t* coord_of_bin, uint64_t n_bins,
                                      const gcsa2_chain_params* chain_params, const gcsa2_pair_params* pair_params, gcsa2_chain* chains,
                                      gcsa2_chain_anchor* members, gcsa2_chain_summary* chain_summaries, gcsa2_chain_pair* top, gcsa2_pair_summary* summaries,
                                      gcsa2_chain_stats* chain_stats, gcsa2_pair_stats* pair_stats)
{
  const u64 chain_top_n = (chain_params != nullptr ? chain_params->top_n : 0), member_cap = (chain_params != nullptr ? chain_params->member_cap : 0);
  const u64 top_n = (pair_params != nullptr ? pair_params->top_n : 0);
  // per pair: four groups of chain rows, member rows and chain summaries, one row of placements and one summary
  const PieceOutput outs[] = {{chains, 4 * chain_top_n, sizeof(gcsa2_chain)}, {members, 4 * chain_top_n * member_cap, sizeof(gcsa2_chain_anchor)},
                              {chain_summaries, 4, sizeof(gcsa2_chain_summary)}, {top, top_n, sizeof(gcsa2_chain_pair)}, {summaries, 1, sizeof(gcsa2_pair_summary)}};
  PairBatchStats sums{};
  const int rc = anchors_batch(ix, patterns, offsets, n_patterns, AnchorWindows{k, 1, true, w, hash_seed, hit_max, over}, coord_of_bin, n_bins, outs, &sums,
                               "gcsa2_minimizer_chain_pairs_batch",
                               [&] { return fused_pairs_checks(ix, n_patterns, k, w, over, shift, coord_of_bin, n_bins, chain_params, pair_params, "coord_of_bin"); },
                               [&](const ReadPiece& p, const u8* d_pat, const u64* d_off, const u64* d_map, void* const* d, PairBatchStats* done) -> int
  {
    return gcsa2_minimizer_chain_pairs_device(ix, d_pat, d_off, p.count, k, w, hash_seed, hit_max, over, shift, d_map, n_bins, chain_params, pair_params,
                                              static_cast<gcsa2_chain*>(d[0]), static_cast<gcsa2_chain_anchor*>(d[1]), static_cast<gcsa2_chain_summary*>(d[2]),
                                              static_cast<gcsa2_chain_pair*>(d[3]), static_cast<gcsa2_pair_summary*>(d[4]), &done->chains, &done->pairs, p.stream);
  }, 2);
  if(rc != GCSA2_OK) { return rc; }
  if(chain_stats != nullptr) { *chain_stats = sums.chains; }
  if(pair_stats != nullptr) { *pair_stats = sums.pairs; }
  return GCSA2_OK;
}

}  // extern "C"
