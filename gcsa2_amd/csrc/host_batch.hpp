// host_batch.hpp -- how a batch in the caller's HOST memory travels to the kernels and back: the pieces a large batch is cut
// into, the host threads that carry them, device buffers of a call, and the chunked pipeline of the large find() batches.
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
