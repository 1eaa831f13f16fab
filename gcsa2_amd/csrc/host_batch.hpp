// host_batch.hpp -- how a batch in the caller's HOST memory travels to the kernels and back: the pieces a large batch is cut
// into, the host threads that carry them, device buffers of a call, the piece loop of the read calls, and the chunked pipeline
// of the large find() batches.
// Host code only.  Part of the single translation unit gcsa2_hip.hip, which includes it once gcsa2_index, g_error / fail()
// and DeviceGuard are defined; the entry points that use it keep only what is particular to their call.
#pragma once

namespace {

// RAII device buffer for the host-pointer entry points
template<class T> struct DBuf
{
  T* p = nullptr;
  hipError_t alloc(u64 count) { return hipMalloc(reinterpret_cast<void**>(&p), (count > 0 ? count : 1) * sizeof(T)); }
  void release() { if(p) { (void)hipFree(p); p = nullptr; } }
  ~DBuf() { release(); }
};

// A caller's buffer that is already page-locked (hipHostMalloc / hipHostRegister: a pinned torch tensor, the facade's own
// arena) is handed to the copy engines where it lies; only pageable memory goes through pinned staging.
inline bool page_locked(const void* first, u64 bytes)
{
  if(bytes == 0) { return false; }
  hipPointerAttribute_t a, b;
  const bool yes = hipPointerGetAttributes(&a, first) == hipSuccess && a.type == hipMemoryTypeHost &&
                   hipPointerGetAttributes(&b, static_cast<const char*>(first) + bytes - 1) == hipSuccess && b.type == hipMemoryTypeHost;
  (void)hipGetLastError();
  return yes;
}

// ---- pieces of a batch ----------------------------------------------------------------------------------------------------

// Cut points of a batch in pieces of at most `limit` pattern bytes, at least one pattern each: piece c is patterns
// cut[c] .. cut[c + 1] - 1.  (offsets: nq + 1 entries, non-decreasing)
inline std::vector<u64> cut_pieces(const uint64_t* offsets, u64 nq, u64 limit)
{
  std::vector<u64> cut(1, 0);
  while(cut.back() < nq)
  {
    const u64 b = cut.back();
    u64 lo = b + 1, hi = nq;                               // largest e with offsets[e] - offsets[b] <= the piece size, at least one pattern
    while(lo < hi) { const u64 mid = (lo + hi + 1) / 2; if(offsets[mid] - offsets[b] <= limit) { lo = mid; } else { hi = mid - 1; } }
    cut.push_back(lo);
  }
  return cut;
}

// the offsets of patterns b .. b + count - 1 as a batch of their own (count + 1 entries from 0), in `local`
inline const u64* rebase_piece(const uint64_t* offsets, u64 b, u64 count, std::vector<u64>& local)
{
  local.resize(count + 1);
  for(u64 i = 0; i <= count; i++) { local[i] = offsets[b + i] - offsets[b]; }
  return local.data();
}

// ---- host threads of one call ---------------------------------------------------------------------------------------------

// Host worker threads of one call.  If starting one of them throws (std::system_error: thread limit), the ones already
// running are joined before the exception travels on -- destroying a joinable std::thread ends the process.
struct Workers
{
  std::vector<std::thread> threads;
  template<class... Args> void emplace_back(Args&&... args) { threads.emplace_back(std::forward<Args>(args)...); }
  void join() { for(std::thread& t : threads) { if(t.joinable()) { t.join(); } } }
  ~Workers() { join(); }
};

// What one of them has to say at the end (g_error is thread-local: the text must travel with the status).  `echo`: this
// thread only stopped because another one failed, whose report is the one the caller should see.
struct Outcome
{
  int status = GCSA2_OK; std::string message; bool echo = false;
  int set(int rc, const std::string& what) { status = rc; message = what; return rc; }
  int hip_error(const char* what, hipError_t e) { return set(GCSA2_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
};

// work(t, outcome) for t < threads, thread 0 on the caller's; thread t takes items t, t + threads, ... of whatever the call
// stripes.  Returns the first failure (through fail(); with `prefix`, as "<prefix><t>: <message>").  No exception leaves a
// worker thread (std::terminate); one from starting a thread reaches the caller after the join.
template<class Work> int fan_out(unsigned threads, const char* prefix, Work work)
{
  std::vector<Outcome> outcome(threads);
  auto run = [&](unsigned t)
  {
    try { work(t, outcome[t]); }
    catch(const std::exception& e) { outcome[t].set(GCSA2_ERR_OUT_OF_MEMORY, std::string("a piece of the batch: ") + e.what()); }
  };
  {
    Workers workers;
    for(unsigned t = 1; t < threads; t++) { workers.emplace_back(run, t); }
    run(0);
    workers.join();
  }
  for(int echoes = 0; echoes < 2; echoes++)
  {
    for(unsigned t = 0; t < threads; t++)
    {
      const Outcome& o = outcome[t];
      if(o.status != GCSA2_OK && o.echo == (echoes != 0)) { return fail(o.status, prefix != nullptr ? prefix + std::to_string(t) + ": " + o.message : o.message); }
    }
  }
  return GCSA2_OK;
}

// ---- read batches: a host form that hands pieces of whole reads to its device form -----------------------------------------
// Three layers.  fan_out starts the host threads.  for_read_pieces is what every host form of a read call does around its
// device form: a batch of two pieces' worth of read bytes or more is cut into pieces of whole reads (tune.ms_piece_bytes,
// GCSA2_MS_PIECE_MB) that tune.ms_threads host threads carry, thread t pieces t, t + threads, ..., each thread on a
// non-blocking stream of its own when there are several pieces (the null stream if it cannot be created); a smaller batch is
// one piece on the null stream.  seed_pieces_batch is the whole host form of the calls that return seeds with their hits.

// pattern offsets handed over by a host caller: non-decreasing, or the kernels would read outside the pattern buffer
inline bool offsets_ok(const uint64_t* offsets, uint64_t nq, u64* longest = nullptr)
{
  u64 bad = 0, most = 0;
  for(u64 q = 0; q < nq; q++)
  {
    const u64 len = offsets[q + 1] - offsets[q];
    bad |= u64(offsets[q + 1] < offsets[q]);
    most = (len > most ? len : most);
  }
  if(longest != nullptr) { *longest = most; }
  return bad == 0;
}

// what a host form refuses of its reads (n > 0, offsets not null); with `name` the missing argument is named
inline int reads_ok(const uint8_t* patterns, const uint64_t* offsets, u64 n, const char* name)
{
  if(offsets[0] != 0 || !offsets_ok(offsets, n)) { return fail(GCSA2_ERR_INVALID_ARGUMENT, "pattern offsets must start at 0 and be non-decreasing"); }
  if(patterns == nullptr && offsets[n] > 0) { return fail(GCSA2_ERR_INVALID_ARGUMENT, name != nullptr ? std::string(name) + ": patterns is NULL" : std::string("null buffer")); }
  return GCSA2_OK;
}

// the windows of length k at every stride-th position of n reads; with `starts`, n + 1 entries: where each read's begin
inline u64 host_windows(const uint64_t* offsets, u64 n, u64 k, u64 stride, u64* starts = nullptr)
{
  u64 total = 0;
  for(u64 q = 0; q < n; q++)
  {
    const u64 len = offsets[q + 1] - offsets[q];
    if(starts != nullptr) { starts[q] = total; }
    if(len >= k) { total += (len - k) / stride + 1; }
  }
  if(starts != nullptr) { starts[n] = total; }
  return total;
}

// one piece below two pieces' worth of read bytes, else cut_pieces
inline std::vector<u64> read_cut(const gcsa2_index* ix, const uint64_t* offsets, u64 n)
{
  return offsets[n] < 2 * ix->tune.ms_piece_bytes ? std::vector<u64>{0, n} : cut_pieces(offsets, n, ix->tune.ms_piece_bytes);
}

// piece c of `pieces`: reads b .. b + count - 1, whose `bytes` bytes begin at patterns + first; `local`: their offsets from 0
struct ReadPiece { u64 c, b, count, first, bytes; const u64* local; hipStream_t stream; u64 pieces; };

// body(piece, outcome) -> bool for every piece of `cut` (read_cut: the caller sizes what it keeps per piece from it).  false,
// or a failure in `outcome`, ends the thread's loop.  A form that brings its own stream (a Lease) asks for none.
template<class Body> int for_read_pieces(const gcsa2_index* ix, const uint64_t* offsets, const std::vector<u64>& cut, Body body, bool streams = true)
{
  const u64 pieces = cut.size() - 1;
  const unsigned threads = unsigned(pieces < ix->tune.ms_threads ? pieces : ix->tune.ms_threads);
  return fan_out(threads, nullptr, [&](unsigned t, Outcome& out)
  {
    DeviceGuard guard(ix->device);
    std::vector<u64> local;
    hipStream_t stream = nullptr;
    if(streams && pieces > 1 && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); stream = nullptr; }
    for(u64 c = t; c < pieces && out.status == GCSA2_OK; c += threads)
    {
      const u64 b = cut[c], count = cut[c + 1] - b, first = offsets[b], bytes = offsets[b + count] - first;
      rebase_piece(offsets, b, count, local);
      if(!body(ReadPiece{c, b, count, first, bytes, local.data(), stream, pieces}, out)) { break; }
    }
    if(stream != nullptr) { (void)hipStreamDestroy(stream); }
  });
}

// the piece's reads and offsets in device buffers of their own, arrived when this returns
inline bool upload_reads(const ReadPiece& piece, const uint8_t* patterns, DBuf<u8>& d_pat, DBuf<u64>& d_off, Outcome& out)
{
  hipError_t e = d_pat.alloc(piece.bytes + 16);
  if(e == hipSuccess) { e = d_off.alloc(piece.count + 1); }
  if(e == hipSuccess && piece.bytes > 0) { e = hipMemcpyAsync(d_pat.p, patterns + piece.first, piece.bytes, hipMemcpyHostToDevice, piece.stream); }
  if(e == hipSuccess) { e = hipMemcpyAsync(d_off.p, piece.local, (piece.count + 1) * sizeof(u64), hipMemcpyHostToDevice, piece.stream); }
  if(e == hipSuccess) { e = hipStreamSynchronize(piece.stream); }
  if(e != hipSuccess) { out.hip_error("upload of a piece", e); return false; }
  return true;
}

// The host form of a call that returns, per read, seeds (seed_offsets, seeds) and, per seed, hits (hit_offsets, hits), after
// the caller's checks (n > 0).  The number of seeds of a piece is not known before it ran, so every piece keeps its four
// arrays in host memory and the caller's arrays are put together from them in read order at the end, when the totals are
// known to fit; *total_seeds and *total_hits are written whatever the outcome.  The call supplies
//   estimate(piece) -> (rm, rh)     the seed and hit room of the piece's first run: with one piece the caller's capacities (a
//                                   refusal is the call's), with several a guess -- a piece that the device form refuses for
//                                   room runs once more with what the refusal asks for
//   run(piece, d_pat, d_off, d_per_read, d_seed_off, d_seeds, rm, &m, d_hit_off, d_hits, rh, &h) -> status
//                                   the device form on piece.stream
// and, if the call has one, an output of per_read_bytes per read (per_read, null: none), copied to its reads' place.
// `groups`: the seed CSR and the per-read output have this many consecutive entries per read (2: a read's two strands,
// gcsa2_stranded_minimizer_hits_batch); per_read_bytes is then the size of one entry.
template<class Estimate, class Run>
int seed_pieces_batch(const gcsa2_index* ix, const uint8_t* patterns, const uint64_t* offsets, u64 n, Estimate estimate, Run run, u64 per_read_bytes,
                      void* per_read, uint64_t* seed_offsets, gcsa2_mem* seeds, u64 seed_capacity, u64* total_seeds, uint64_t* hit_offsets,
                      uint64_t* hits, u64 hit_capacity, u64* total_hits, u64 groups = 1)
{
  const std::vector<u64> cut = read_cut(ix, offsets, n);
  struct Piece { u64 m = 0, h = 0; std::vector<u64> seed_off, hit_off, hits; std::vector<gcsa2_mem> seeds; };
  std::vector<Piece> done(cut.size() - 1);
  const int rc = for_read_pieces(ix, offsets, cut, [&](const ReadPiece& p, Outcome& out) -> bool
  {
    Piece& piece = done[p.c];
    DBuf<u8> d_pat, d_per_read; DBuf<u64> d_off, d_seed_off, d_hit_off, d_hits; DBuf<gcsa2_mem> d_seeds;
    if(!upload_reads(p, patterns, d_pat, d_off, out)) { return false; }
    hipError_t e = d_seed_off.alloc(groups * p.count + 1);
    if(e == hipSuccess && per_read != nullptr) { e = d_per_read.alloc(groups * p.count * per_read_bytes); }
    if(e != hipSuccess) { out.hip_error("upload of a piece", e); return false; }
    std::pair<u64, u64> room = estimate(p);
    u64 &rm = room.first, &rh = room.second;
    int piece_rc = GCSA2_OK;
    for(int attempt = 0; attempt < 2; attempt++)
    {
      d_seeds.release(); d_hit_off.release(); d_hits.release();
      e = d_seeds.alloc(rm);
      if(e == hipSuccess) { e = d_hit_off.alloc(rm + 1); }
      if(e == hipSuccess) { e = d_hits.alloc(rh); }
      if(e != hipSuccess) { break; }
      piece_rc = run(p, d_pat.p, d_off.p, d_per_read.p, d_seed_off.p, d_seeds.p, rm, &piece.m, d_hit_off.p, d_hits.p, rh, &piece.h);
      if(piece_rc == GCSA2_ERR_BUFFER_TOO_SMALL && p.pieces > 1 && attempt == 0 && (piece.m > rm || piece.h > rh)) { rm = piece.m; rh = piece.h; continue; }
      break;
    }
    if(e != hipSuccess) { out.set(e == hipErrorOutOfMemory ? GCSA2_ERR_OUT_OF_MEMORY : GCSA2_ERR_HIP, std::string("buffers of a piece: ") + hipGetErrorString(e)); return false; }
    if(piece_rc != GCSA2_OK) { out.set(piece_rc, g_error); return false; }
    piece.seed_off.resize(groups * p.count + 1); piece.seeds.resize(piece.m); piece.hit_off.resize(piece.m + 1); piece.hits.resize(piece.h);
    e = hipMemcpy(piece.seed_off.data(), d_seed_off.p, (groups * p.count + 1) * sizeof(u64), hipMemcpyDeviceToHost);
    if(e == hipSuccess && piece.m > 0) { e = hipMemcpy(piece.seeds.data(), d_seeds.p, piece.m * sizeof(gcsa2_mem), hipMemcpyDeviceToHost); }
    if(e == hipSuccess) { e = hipMemcpy(piece.hit_off.data(), d_hit_off.p, (piece.m + 1) * sizeof(u64), hipMemcpyDeviceToHost); }
    if(e == hipSuccess && piece.h > 0) { e = hipMemcpy(piece.hits.data(), d_hits.p, piece.h * sizeof(u64), hipMemcpyDeviceToHost); }
    if(e == hipSuccess && per_read != nullptr) { e = hipMemcpy(static_cast<u8*>(per_read) + groups * p.b * per_read_bytes, d_per_read.p, groups * p.count * per_read_bytes, hipMemcpyDeviceToHost); }
    if(e != hipSuccess) { out.hip_error("download of a piece", e); return false; }
    return true;
  });
  u64 m = 0, h = 0;
  for(const Piece& piece : done) { m += piece.m; h += piece.h; }
  *total_seeds = m;
  *total_hits = h;
  if(rc != GCSA2_OK) { return rc; }
  if(m > seed_capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "seed buffer too small"); }
  if(h > hit_capacity) { return fail(GCSA2_ERR_BUFFER_TOO_SMALL, "hit buffer too small"); }
  u64 mbase = 0, hbase = 0;
  for(u64 c = 0; c + 1 < cut.size(); c++)
  {
    const Piece& piece = done[c];
    const u64 b = groups * cut[c], count = groups * (cut[c + 1] - cut[c]);
    for(u64 i = 0; i <= count; i++) { seed_offsets[b + i] = piece.seed_off[i] + mbase; }
    if(piece.m > 0) { std::memcpy(seeds + mbase, piece.seeds.data(), piece.m * sizeof(gcsa2_mem)); }
    for(u64 i = 0; i <= piece.m; i++) { hit_offsets[mbase + i] = piece.hit_off[i] + hbase; }
    if(piece.h > 0) { std::memcpy(hits + hbase, piece.hits.data(), piece.h * sizeof(u64)); }
    mbase += piece.m;
    hbase += piece.h;
  }
  return GCSA2_OK;
}

// ---- large host batches: chunked, double-buffered host -> device -> host pipeline -----------------------------------------
// A batch of millions of patterns in pageable host memory used to go through ONE copy in, one kernel, one copy out: 10 M
// 32-mers took 25 ms, ten times the kernel (19 GB/s end to end).  Here PIPE_LANES host threads each take every
// PIPE_LANES-th chunk of PIPE_CHUNK_QUERIES patterns: copy the chunk into pinned memory (rebasing its offsets), enqueue
// H2D + k_find2 + D2H on the lane's own stream, and while that runs prepare the next chunk in the lane's other staging set;
// a set's results are copied to the caller's array when its event has fired.  Both PCIe directions, the kernel and the host
// copies overlap; what bounds the batch is the host's memcpy rate (56 bytes per 32-mer query through pinned memory).
// (lanes: tune.pipe_lanes, GCSA2_PIPE_LANES, 1..16, default 6; patterns per chunk: tune.pipe_chunk, GCSA2_PIPE_CHUNK = log2, default 18.
// Round 4 re-measured the shape on the headline index, one live image re-shaped with gcsa2_index_set_pipeline: 12 lanes x 2^17
// -- round 3's choice -- 1.4-1.8 G packed 32-mers/s, 6 lanes x 2^18 2.1-2.5 G; 0.9-1.0 -> 1.15-1.3 G for the bytes interface.  The
// boxes give a container 16 CPUs' worth of time: twelve spinning lanes plus the runtime's own threads run into that quota --
// with hipEventBlockingSync twelve lanes gain 20 %, six gain nothing; profiles/r04_host.md.)
constexpr u64 PIPE_CHUNK_BYTES = u64(8) << 20;     // per chunk: at most this many pattern bytes, and tune.pipe_chunk patterns (GCSA2_PIPE_CHUNK = log2, 15..20, default 18)
constexpr u64 PIPE_MIN_QUERIES = u64(1) << 19;                                       // smaller batches take the single-copy path
constexpr int PIPE_PATTERN_TOO_LONG = 1;                                             // internal: not a gcsa2_status

// A staging set (pinned and device alike): patterns (+ 32 bytes of phase, + slack) | offsets | ranges
inline u64 pipe_out_at(u64 PIPE_CHUNK_QUERIES) { return (PIPE_CHUNK_BYTES + 64) + (PIPE_CHUNK_QUERIES + 8) * 8; }      // where a set keeps its ranges
inline u64 pipe_set_bytes(u64 PIPE_CHUNK_QUERIES) { return pipe_out_at(PIPE_CHUNK_QUERIES) + PIPE_CHUNK_QUERIES * 16; }

int pipe_prepare(const gcsa2_index* ix)
{
  if(!ix->pipe.empty()) { return GCSA2_OK; }
  const unsigned PIPE_LANES = ix->tune.pipe_lanes;
  std::vector<gcsa2_index::PipeLane> lanes(PIPE_LANES);
  hipError_t e = hipSuccess;
  for(gcsa2_index::PipeLane& lane : lanes)
  {
    if(e == hipSuccess) { e = hipStreamCreateWithFlags(&lane.stream, hipStreamNonBlocking); }
    for(gcsa2_index::PipeSet& set : lane.set)
    {
      if(e == hipSuccess) { e = hipHostMalloc(reinterpret_cast<void**>(&set.h), pipe_set_bytes(ix->tune.pipe_chunk), hipHostMallocDefault); }
      if(e == hipSuccess) { e = hipMalloc(reinterpret_cast<void**>(&set.d), pipe_set_bytes(ix->tune.pipe_chunk)); }
      if(e == hipSuccess) { e = hipEventCreateWithFlags(&set.done, hipEventDisableTiming | (ix->tune.pipe_blocking ? hipEventBlockingSync : 0)); }
    }
  }
  if(e != hipSuccess)
  {
    for(gcsa2_index::PipeLane& lane : lanes)
    {
      for(gcsa2_index::PipeSet& set : lane.set)
      {
        if(set.h) { (void)hipHostFree(set.h); } if(set.d) { (void)hipFree(set.d); } if(set.done) { (void)hipEventDestroy(set.done); }
      }
      if(lane.stream) { (void)hipStreamDestroy(lane.stream); }
    }
    return fail(e == hipErrorOutOfMemory ? GCSA2_ERR_OUT_OF_MEMORY : GCSA2_ERR_HIP, std::string("host pipeline: ") + hipGetErrorString(e));
  }
  ix->pipe = std::move(lanes);
  return GCSA2_OK;
}

// What a pipelined call does first, holding ix->pipe_lock: the lanes exist, and PIPE_CHUNK_QUERIES is the handle's patterns
// per chunk, less for a batch too small to give every lane two chunks of that size.
inline int pipe_begin(const gcsa2_index* ix, u64 nq, u64& PIPE_CHUNK_QUERIES)
{
  PIPE_CHUNK_QUERIES = ix->tune.pipe_chunk;
  const u64 even = ((nq / (2 * u64(ix->tune.pipe_lanes)) + 63) & ~u64(63)), least = u64(1) << 15;
  if(even < PIPE_CHUNK_QUERIES) { PIPE_CHUNK_QUERIES = (even > least ? even : least); }
  return pipe_prepare(ix);
}

// The ranges of a chunk travel home as (sp, length) pairs in the narrowest exact form (comm.hpp: k_pack_ranges32 / 40): 8 bytes
// per query below 2^32 path nodes and edges, 10 below 2^40, else the 16 bytes of the u64 pairs.  A lane widens them into the
// caller's array when it retires the chunk.
inline u64 pipe_wire_bytes(const gcsa2_index* ix)
{
  const u64 top = (ix->img.n > ix->img.e ? ix->img.n : ix->img.e);
  return (top < (u64(1) << 32) ? 8 : (top < (u64(1) << 40) ? 10 : 16));
}

inline void pipe_widen(const char* h, u64 count, u64 wire, u64* dst)
{
  if(wire == 10)                     // (sp, length) as five u16
  {
    const unsigned short* w = reinterpret_cast<const unsigned short*>(h);
    for(u64 i = 0; i < count; i++, w += 5)
    {
      const u64 sp = u64(w[0]) | (u64(w[1]) << 16) | (u64(w[4] & 0xFF) << 32), len = u64(w[2]) | (u64(w[3]) << 16) | (u64(w[4] >> 8) << 32);
      dst[2 * i] = sp; dst[2 * i + 1] = sp + len - 1;
    }
  }
  else                               // (sp, length) as u32 pairs
  {
    const u32* w = reinterpret_cast<const u32*>(h);
    for(u64 i = 0; i < count; i++) { dst[2 * i] = w[2 * i]; dst[2 * i + 1] = u64(w[2 * i]) + u64(w[2 * i + 1]) - 1; }
  }
}

// The lanes of one pipelined call (ix->pipe_lock held, pipe_begin done): lane t takes chunks t, t + PIPE_LANES, ... in its two
// staging sets by turns.  The chunk SOURCE is what the bytes and the packed form differ in:
//   stage(c, lane, set, outcome) -> bool   stages chunk c on lane.stream -- its uploads and its find call, the ranges as u64
//                                          pairs at set.d + pipe_out_at() -- and names it in set.first / set.count; false
//                                          with the failure in `outcome`.
// What follows is the same for both.  wire 8 / 10: the ranges are packed over the chunk's input at the start of set.d (consumed
// by then) and that is what travels, to be widened into the caller's array when the set is retired; wire 16: the pairs travel,
// straight into `ranges` when the array is page-locked (direct_out), else through the pinned set.
template<class Stage> int pipe_run(const gcsa2_index* ix, u64 chunks, u64 PIPE_CHUNK_QUERIES, u64 wire, bool direct_out, uint64_t* ranges, Stage stage)
{
  const unsigned PIPE_LANES = ix->tune.pipe_lanes;
  const u64 out_at = pipe_out_at(PIPE_CHUNK_QUERIES);
  auto work = [&](unsigned t, Outcome& out)
  {
    DeviceGuard guard(ix->device);
    gcsa2_index::PipeLane& lane = ix->pipe[t];
    auto retire = [&](gcsa2_index::PipeSet& set) -> bool        // wait for the set's chunk and hand its ranges to the caller
    {
      if(!set.busy) { return true; }
      hipError_t e = hipEventSynchronize(set.done);
      if(e != hipSuccess) { out.hip_error("hipEventSynchronize", e); return false; }
      if(wire != 16) { pipe_widen(set.h, set.count, wire, ranges + 2 * set.first); }
      else if(!direct_out) { std::memcpy(ranges + 2 * set.first, set.h + out_at, set.count * 16); }
      set.busy = false;
      return true;
    };
    unsigned turn = 0;
    for(u64 c = t; c < chunks && out.status == GCSA2_OK; c += PIPE_LANES, turn ^= 1)
    {
      gcsa2_index::PipeSet& set = lane.set[turn];
      if(!retire(set) || !stage(c, lane, set, out)) { break; }
      u64* d_out = reinterpret_cast<u64*>(set.d + out_at);
      hipError_t err = hipSuccess;
      if(wire != 16)
      {
        const int rc_pack = (wire == 10 ? gcsa2_pack_ranges40_device(d_out, set.count, set.d, lane.stream) : gcsa2_pack_ranges32_device(d_out, set.count, reinterpret_cast<uint32_t*>(set.d), lane.stream));
        if(rc_pack != GCSA2_OK) { out.set(rc_pack, g_error); break; }
        err = hipMemcpyAsync(set.h, set.d, set.count * wire, hipMemcpyDeviceToHost, lane.stream);
      }
      else { err = hipMemcpyAsync(direct_out ? reinterpret_cast<char*>(ranges + 2 * set.first) : set.h + out_at, d_out, set.count * 16, hipMemcpyDeviceToHost, lane.stream); }
      if(err == hipSuccess) { err = hipEventRecord(set.done, lane.stream); }
      if(err != hipSuccess) { out.hip_error("hipMemcpyAsync / hipEventRecord", err); break; }
      set.busy = true;
    }
    for(gcsa2_index::PipeSet& set : lane.set) { if(out.status == GCSA2_OK) { (void)retire(set); } }
    if(out.status != GCSA2_OK)           // nothing of this call may still be in flight when it returns
    {
      (void)hipStreamSynchronize(lane.stream);
      for(gcsa2_index::PipeSet& set : lane.set) { set.busy = false; }
    }
  };
  return fan_out(unsigned(chunks < PIPE_LANES ? chunks : PIPE_LANES), "pipeline lane ", work);
}

}  // namespace
