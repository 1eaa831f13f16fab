// kernels_clusters.hpp -- seed clusters (gcsa2_seed_clusters_device and its fused forms): per group of seed records the top_n
// diagonal bands of its anchors.  An anchor is a (seed, hit) pair; its diagonal is the coordinate of the hit minus the seed's
// position in the read.  Included by gcsa2_hip.hip after kernels_support.hpp (wave_sum).
//
// Data flow: k_clusters_plan (one wavefront per group: the group is checked against n_seeds and n_hits ONCE, here; info[g] is
// its anchor count or "invalid", lsize[g] the same count if the group is above the LDS capacity) -> k_clusters_lds (one
// workgroup per group: gather, bitonic sort by diagonal, heads, bitonic sort by (cluster, position), segment sums, top row) ->
// for the groups above the capacity the same steps device-wide: k_anchors_large_gather, two radix sorts by (group, diagonal),
// k_clusters_large_take / _heads, a max-scan for the cluster of every anchor, a radix sort by (cluster, position),
// k_clusters_large_ends and a max-scan for the running end, k_clusters_large_cover and a sum-scan for covered and starts,
// then k_clusters_large_score (one workgroup per group).  Both paths end in clu_score, over a view of LDS or of global memory.
//
// Shared with the seed chains (kernels_chains.hpp): the plan, k_anchors_large_gather<clu_place or chn_place>, clu_large_placed,
// clu_zero, clu_flush.  Not the group loop and LDS gather of the two LDS kernels: folded, the chain kernels ran slower
// (profiles/anchor_groups_refactor.md).
//
// A cluster is named by the sorted place of its first anchor (its HEAD): heads ascend with the diagonal and, in the large
// path, with the group, so "sort by (group, cluster, position)" is one 64-bit key head << 32 | position, and the running
// maximum of head << 32 | end is, inside a cluster, the running maximum of the end -- no segmented scan anywhere.
#pragma once

namespace {

// device counters of one call; CLU_LARGE and CLU_MAX_SMALL steer the host: the anchors of the groups above the capacity
// and the largest group below it (the LDS of the launch is sized by it)
enum : u32 { CLU_INVALID = 0, CLU_SEEDS = 1, CLU_ANCHORS = 2, CLU_UNPLACED = 3, CLU_CLUSTERS = 4, CLU_SPILLED = 5, CLU_LARGE = 6, CLU_MAX_SMALL = 7, CLU_WORDS = 8 };

constexpr u32 CLU_CAP_MIN = 64, CLU_CAP_DEFAULT = 4096;     // anchors of a group in LDS
constexpr u32 CLU_WAVE_MAX = 256;                           // a group of up to this many anchors is one wavefront's
constexpr u32 CLU_LDS_BYTES = 32;                           // per anchor: diagonal, position | end, second key, sums
constexpr u64 CLU_INFO_INVALID = ~u64(0);
constexpr u64 CLU_BIAS = u64(1) << 63;                      // diag ^ CLU_BIAS: signed order as unsigned order
constexpr u64 CLU_NONE = ~u64(0);                           // the key and payload of a pad; no anchor has this payload (end < 2^32)
static_assert(GCSA2_CLUSTER_TOP_LIMIT == 64, "lane j of the wavefront holds the j-th cluster of the running top row");
static_assert(sizeof(gcsa2_cluster) == 64 && sizeof(gcsa2_cluster_summary) == 24, "a cluster is eight words, a summary three");
static_assert(CLU_CAP_DEFAULT <= 4096, "the LDS keys hold a head and an anchor index of 12 bits each, the sums 13 bits of anchors");
static_assert(u64(CLU_CAP_DEFAULT) * CLU_LDS_BYTES + 4096 <= (160u << 10), "a group at full capacity fits the LDS of a CU");

struct CluMap { u32 shift; const u64* coord; u64 n_bins; };

// The diagonal key and position << 32 | end of the anchor (seed at `pos` of `len` bases, hit v), or false: unplaced.
__device__ __forceinline__ bool clu_place(const CluMap& map, u64 v, u64 pos, u64 len, u64& key, u64& pe)
{
  const u64 bin = v >> map.shift;
  if(bin >= map.n_bins) { return false; }
  const u64 c = map.coord[bin];
  if(c == GCSA2_UNKNOWN) { return false; }
  constexpr u64 LIMIT = u64(1) << 32;
  if(pos >= LIMIT || len >= LIMIT || pos + len >= LIMIT) { return false; }
  const u64 x = c + (v & ((u64(1) << map.shift) - 1));
  key = (x - pos) ^ CLU_BIAS;
  pe = (pos << 32) | (pos + len);
  return true;
}
// a placer, clu_place or the chains' chn_place: the gathers below are written once and take it as a template argument
using CluPlaceFn = bool(const CluMap&, u64, u64, u64, u64&, u64&);

// the seed of hit h: the last i in [first, last) with hoff[i] <= h (hoff[first] <= h < hoff[last], the offsets do not decrease)
__device__ __forceinline__ u64 clu_seed_of(const u64* __restrict__ hoff, u64 first, u64 last, u64 h)
{
  u64 lo = first, hi = last;
  while(hi - lo > 1)
  {
    const u64 mid = lo + (hi - lo) / 2;
    if(hoff[mid] <= h) { lo = mid; } else { hi = mid; }
  }
  return lo;
}

__device__ __forceinline__ u64 clu_max(u64 a, u64 b) { return a > b ? a : b; }

// One wavefront per group, the workgroups striding over them.  A group whose offsets decrease or reach beyond n_seeds, or
// whose hit offsets hoff[first .. last] decrease or reach beyond n_hits, is invalid; a group without a seed reads no hit
// offset.  Nothing else in this file checks a group again.  Six atomics per workgroup at most.
__global__ __launch_bounds__(TPB) void k_clusters_plan(const u64* __restrict__ goff, u64 n_groups, u64 n_seeds, const u64* __restrict__ hoff, u64 n_hits,
                                                       u64 cap, u64* __restrict__ info, u64* __restrict__ lsize, unsigned long long* __restrict__ stat)
{
  constexpr u32 WAVES = TPB / 64;
  __shared__ u64 sums[WAVES][6];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  u64 invalid = 0, seeds = 0, spilled = 0, large = 0, most = 0;
  for(u64 g = u64(blockIdx.x) * WAVES + wave; g < n_groups; g += u64(gridDim.x) * WAVES)
  {
    const u64 first = goff[g], last = goff[g + 1];
    bool ok = (first <= last && last <= n_seeds);
    u64 anchors = 0;
    if(ok && first < last)
    {
      bool bad = false;
      for(u64 i = first + lane; i < last; i += 64) { if(hoff[i] > hoff[i + 1]) { bad = true; } }      // i + 1 <= last <= n_seeds
      const u64 from = hoff[first], to = hoff[last];
      if(to > n_hits) { bad = true; }
      ok = (__any(bad) == 0);
      if(ok) { anchors = to - from; }
    }
    if(lane == 0)
    {
      info[g] = (ok ? anchors : CLU_INFO_INVALID);
      lsize[g] = (ok && anchors > cap ? anchors : 0);
      if(!ok) { invalid++; }
      else
      {
        seeds += last - first;
        if(anchors > cap) { spilled++; large += anchors; } else { most = clu_max(most, anchors); }
      }
    }
  }
  if(lane == 0) { sums[wave][0] = invalid; sums[wave][1] = seeds; sums[wave][2] = spilled; sums[wave][3] = large; sums[wave][4] = most; }
  __syncthreads();
  if(threadIdx.x == 0)
  {
    for(u32 w = 1; w < WAVES; w++)
    {
      invalid += sums[w][0]; seeds += sums[w][1]; spilled += sums[w][2]; large += sums[w][3]; most = clu_max(most, sums[w][4]);
    }
    if(invalid != 0) { atomicAdd(stat + CLU_INVALID, (unsigned long long)invalid); }
    if(seeds != 0) { atomicAdd(stat + CLU_SEEDS, (unsigned long long)seeds); }
    if(spilled != 0) { atomicAdd(stat + CLU_SPILLED, (unsigned long long)spilled); atomicAdd(stat + CLU_LARGE, (unsigned long long)large); }
    if(most != 0) { atomicMax(stat + CLU_MAX_SMALL, (unsigned long long)most); }
  }
}

// ---- the score: what both paths share ------------------------------------------------------------------------------------------

// (score, diagonal key) a ahead of b: score = covered << 32 | anchors, the larger first; then the smaller diag_min.  A lane
// without a cluster holds (0, CLU_NONE): a cluster has at least one anchor, so its score is not 0.
__device__ __forceinline__ bool clu_ahead(u64 sa, u64 da, u64 sb, u64 db) { return sa > sb || (sa == sb && da < db); }

// One wavefront holds a top row sorted by clu_ahead in its registers, lane j the j-th entry (score, key, payload): the entry
// (ns, nk, nx), the same in every lane, goes to its place and the entries behind it move down one lane; the last falls off.
__device__ __forceinline__ void clu_top_insert(u64& rs, u64& rk, u64& rx, u64 ns, u64 nk, u64 nx)
{
  const u32 lane = threadIdx.x & 63;
  const u32 at = u32(__popcll(__ballot(clu_ahead(rs, rk, ns, nk))));             // the row is sorted: those ahead are a prefix
  const u64 us = __shfl_up(rs, 1, 64), uk = __shfl_up(rk, 1, 64), ux = __shfl_up(rx, 1, 64);
  if(lane == at) { rs = ns; rk = nk; rx = nx; }
  else if(lane > at) { rs = us; rk = uk; rx = ux; }
}

struct CluShared
{
  u64 wave[TPB / 64];
  u64 win_score[64], win_key[64], win_at[64];              // the top row: score, diag_min key, head << 32 | starts
  u64 clusters;
  u32 count;
};

// View of a group's placed anchors in diagonal order (key, pe) and of its clusters: cand(i) says whether place i holds the
// sums of a cluster -- its head in LDS, its last anchor in global memory -- and which.
struct CluLdsView
{
  const u64 *dk, *pe, *acc;
  __device__ __forceinline__ u64 key(u64 i) const { return dk[i]; }
  __device__ __forceinline__ u64 pos_end(u64 i) const { return pe[i]; }
  __device__ __forceinline__ bool cand(u64 i, u64, u64& score, u64& head, u64& starts) const
  {
    const u64 a = acc[i];                                    // covered << 26 | anchors << 13 | starts
    if(a == 0) { return false; }
    score = ((a >> 26) << 32) | ((a >> 13) & 0x1FFF);
    head = i; starts = a & 0x1FFF;
    return true;
  }
};

struct CluGlobalView
{
  const u64 *dk, *pe, *key2, *sum;                           // key2: head << 32 | position, sorted; sum: covered << 32 | starts, scanned
  __device__ __forceinline__ u64 key(u64 i) const { return dk[i]; }
  __device__ __forceinline__ u64 pos_end(u64 i) const { return pe[i]; }
  __device__ __forceinline__ bool cand(u64 i, u64 end, u64& score, u64& head, u64& starts) const
  {
    const u64 h = key2[i] >> 32;
    if(i + 1 < end && (key2[i + 1] >> 32) == h) { return false; }
    const u64 delta = sum[i] - (h > 0 ? sum[h - 1] : 0);     // exact: covered and starts of one cluster are below 2^32
    score = (delta & ~u64(0xFFFFFFFF)) | (i - h + 1);
    head = h; starts = delta & 0xFFFFFFFF;
    return true;
  }
};

// The whole workgroup: the clusters of the placed anchors [begin, end) of group g are ranked by wavefront 0 (the running top
// row in its registers, lane j the j-th cluster; a candidate joins only if it is ahead of entry top_n - 1: a ballot and one
// wave-wide insertion), then every wavefront completes winners from their anchors (diag_max, ref_begin, read_begin,
// read_end), and the row -- zeros behind the last cluster -- and the summary are stored.  Returns the number of clusters.
template<u32 T, class View>
__device__ u64 clu_score(const View& view, u64 begin, u64 end, u64 anchors_all, u64 g, u32 top_n, gcsa2_cluster* __restrict__ top,
                         gcsa2_cluster_summary* __restrict__ summaries, CluShared& sh)
{
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  if(wave == 0)
  {
    u64 rs = 0, rk = CLU_NONE, rx = 0, clusters = 0;
    for(u64 i0 = begin; i0 < end; i0 += 64)
    {
      const u64 i = i0 + lane;
      u64 s = 0, head = 0, starts = 0;
      const bool valid = (i < end && view.cand(i, end, s, head, starts));
      const u64 k = (valid ? view.key(head) : CLU_NONE), x = (head << 32) | starts;
      clusters += u64(__popcll(__ballot(valid)));
      const u64 cut_s = __shfl(rs, int(top_n - 1), 64), cut_k = __shfl(rk, int(top_n - 1), 64);
      u64 fresh = __ballot(valid && clu_ahead(s, k, cut_s, cut_k));
      while(fresh != 0)
      {
        const int src = __ffsll((unsigned long long)fresh) - 1;
        fresh &= fresh - 1;
        clu_top_insert(rs, rk, rx, __shfl(s, src, 64), __shfl(k, src, 64), __shfl(x, src, 64));
      }
    }
    sh.win_score[lane] = rs; sh.win_key[lane] = rk; sh.win_at[lane] = rx;
    if(lane == 0) { sh.clusters = clusters; }
  }
  __syncthreads();
  const u64 clusters = sh.clusters;
  const u32 winners = u32(clusters < top_n ? clusters : top_n);
  if(top != nullptr)
  {
    u64* row = reinterpret_cast<u64*>(top + g * top_n);
    for(u32 w = wave; w < winners; w += T / 64)
    {
      const u64 score = sh.win_score[w], head = sh.win_at[w] >> 32, n = score & 0xFFFFFFFF;
      u64 ref = ~u64(0), from = ~u64(0), to = 0;
      for(u64 i = head + lane; i < head + n; i += 64)
      {
        const u64 p = view.pos_end(i), pos = p >> 32, x = (view.key(i) ^ CLU_BIAS) + pos;
        ref = (x < ref ? x : ref); from = (pos < from ? pos : from); to = clu_max(to, p & 0xFFFFFFFF);
      }
#pragma unroll
      for(u32 o = 32; o > 0; o >>= 1)
      {
        const u64 a = __shfl_xor(ref, o, 64), b = __shfl_xor(from, o, 64), c = __shfl_xor(to, o, 64);
        ref = (a < ref ? a : ref); from = (b < from ? b : from); to = clu_max(to, c);
      }
      if(lane == 0)
      {
        u64* dst = row + 8 * u64(w);
        dst[0] = sh.win_key[w] ^ CLU_BIAS; dst[1] = view.key(head + n - 1) ^ CLU_BIAS; dst[2] = n; dst[3] = sh.win_at[w] & 0xFFFFFFFF;
        dst[4] = score >> 32; dst[5] = from; dst[6] = to; dst[7] = ref;
      }
    }
    for(u32 word = winners * 8 + threadIdx.x; word < top_n * 8; word += T) { row[word] = 0; }
  }
  if(summaries != nullptr && threadIdx.x == 0)
  {
    u64* dst = reinterpret_cast<u64*>(summaries + g);
    dst[0] = end - begin; dst[1] = anchors_all - (end - begin); dst[2] = clusters;
  }
  __syncthreads();                                           // the top row is read before the next group writes it
  return clusters;
}

// the zero row (of clusters, or of chains) of an invalid group or one without a placed anchor, and its summary {0, unplaced, 0}
template<u32 T, class Row, class Summary>
__device__ __forceinline__ void clu_zero(u64 g, u32 top_n, Row* __restrict__ top, Summary* __restrict__ summaries, u64 unplaced)
{
  static_assert(sizeof(Row) == 64 && sizeof(Summary) == 24, "eight words a row entry, three a summary");
  if(top != nullptr)
  {
    u64* row = reinterpret_cast<u64*>(top + g * top_n);
    for(u32 word = threadIdx.x; word < top_n * 8; word += T) { row[word] = 0; }
  }
  if(summaries != nullptr && threadIdx.x == 0)
  {
    u64* dst = reinterpret_cast<u64*>(summaries + g);
    dst[0] = 0; dst[1] = unplaced; dst[2] = 0;
  }
}

// what a workgroup counted over its groups: three atomics at most, by thread 0 (the other threads' sums are not looked at)
__device__ __forceinline__ void clu_flush(unsigned long long* __restrict__ stat, u64 anchors, u64 unplaced, u64 clusters)
{
  if(threadIdx.x == 0)
  {
    if(anchors != 0) { atomicAdd(stat + CLU_ANCHORS, (unsigned long long)anchors); }
    if(unplaced != 0) { atomicAdd(stat + CLU_UNPLACED, (unsigned long long)unplaced); }
    if(clusters != 0) { atomicAdd(stat + CLU_CLUSTERS, (unsigned long long)clusters); }
  }
}

// ---- the LDS path ------------------------------------------------------------------------------------------------------------

// The exclusive maximum over the lower threads of the workgroup (0 for thread 0).  Two barriers.
__device__ __forceinline__ u64 clu_block_before(u64 v, u64* wave_max)
{
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x / 64;
#pragma unroll
  for(u32 o = 1; o < 64; o <<= 1)
  {
    const u64 t = __shfl_up(v, o, 64);
    if(lane >= o) { v = clu_max(v, t); }
  }
  if(lane == 63) { wave_max[wave] = v; }
  __syncthreads();
  u64 before = __shfl_up(v, 1, 64);
  if(lane == 0) { before = 0; }
  for(u32 w = 0; w < wave; w++) { before = clu_max(before, wave_max[w]); }
  __syncthreads();
  return before;
}

// Bitonic sort of n (a power of two) pairs by (a, b), or of the keys a alone; ascending.  Ends with a barrier.
template<u32 T, bool PAIRS>
__device__ __forceinline__ void clu_bitonic(u64* a, u64* b, u32 n)
{
  for(u32 k = 2; k <= n; k <<= 1)
  {
    for(u32 j = k >> 1; j > 0; j >>= 1)
    {
      for(u32 t = threadIdx.x; t < n / 2; t += T)
      {
        const u32 lo = 2 * t - (t & (j - 1)), hi = lo + j;
        const u64 x = a[lo], y = a[hi];
        bool above = x > y;
        if constexpr(PAIRS)
        {
          const u64 p = b[lo], q = b[hi];
          above = above || (x == y && p > q);
          if(above == ((lo & k) == 0)) { a[lo] = y; a[hi] = x; b[lo] = q; b[hi] = p; }
        }
        else if(above == ((lo & k) == 0)) { a[lo] = y; a[hi] = x; }
      }
      __syncthreads();
    }
  }
}

// One workgroup of T lanes per group, striding; dynamic LDS: four arrays of `cap` (a power of two) 64-bit words.  info[g]
// decides: the launch takes the groups of above < anchors <= spill (<= cap); the one with above == 0 also writes the zero rows
// of the invalid groups and of those without an anchor; a group above `spill` is left to the large path.  A call launches
// T = 64 for the groups of up to CLU_WAVE_MAX anchors -- one wavefront per read, whose barriers cost nothing and of which a
// CU holds many -- and T = 256 for the others.
//   1. gather: anchor a of the group is hit hoff[first] + a, its seed found by a search over the hit offsets; the placed ones
//      are packed by ballot (one LDS atomic per wavefront and turn) as dk = diag ^ 2^63, pe = position << 32 | end
//   2. bitonic sort of (dk, pe), padded with (CLU_NONE, CLU_NONE), which no anchor equals
//   3. heads by neighbour difference; a max-scan of head places gives every anchor its cluster
//   4. bitonic sort of k2 = head << 44 | position << 12 | place
//   5. every thread walks a stretch of k2 with the running maximum of head << 32 | end (carried in from the lower threads):
//      covered grows by what the anchor adds beyond that maximum, starts by a change of (head, position); per cluster and
//      thread one LDS add into acc[head] = covered << 26 | anchors << 13 | starts
//   6. clu_score
// Three atomics per workgroup for the stats (clu_flush).
template<u32 T>
__global__ __launch_bounds__(T) void k_clusters_lds(const u64* __restrict__ goff, u64 n_groups, const u64* __restrict__ seeds, const u64* __restrict__ hoff,
                                                      const u64* __restrict__ hits, const u64* __restrict__ info, CluMap map, u64 band, u32 top_n, u32 cap,
                                                      u64 above, u64 spill, gcsa2_cluster* __restrict__ top, gcsa2_cluster_summary* __restrict__ summaries,
                                                      unsigned long long* __restrict__ stat)
{
  extern __shared__ u64 clu_words[];
  __shared__ CluShared sh;
  u64 *dk = clu_words, *pe = dk + cap, *k2 = pe + cap;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(k2 + cap);
  const u32 lane = threadIdx.x & 63;
  u64 all_anchors = 0, all_unplaced = 0, all_clusters = 0;
  for(u64 g = blockIdx.x; g < n_groups; g += gridDim.x)
  {
    const u64 total = info[g];
    if(total == CLU_INFO_INVALID || total == 0)
    {
      if(above == 0) { clu_zero<T>(g, top_n, top, summaries, 0); }
      continue;
    }
    if(total <= above || total > spill) { continue; }
    // 1.
    if(threadIdx.x == 0) { sh.count = 0; }
    __syncthreads();
    const u64 first = goff[g], last = goff[g + 1], h0 = hoff[first];
    for(u64 base = 0; base < total; base += T)
    {
      const u64 a = base + threadIdx.x;
      u64 key = 0, p = 0;
      bool placed = false;
      if(a < total)
      {
        const u64 h = h0 + a, i = clu_seed_of(hoff, first, last, h);
        placed = clu_place(map, hits[h], seeds[5 * i], seeds[5 * i + 1], key, p);
      }
      const u64 mask = __ballot(placed);
      u32 at = 0;
      if(lane == 0 && mask != 0) { at = atomicAdd(&sh.count, u32(__popcll(mask))); }
      at = __shfl(at, 0, 64) + u32(__popcll(mask & ((u64(1) << lane) - 1)));
      if(placed) { dk[at] = key; pe[at] = p; }               // at < total <= cap
    }
    __syncthreads();
    const u32 n = sh.count;
    if(threadIdx.x == 0) { all_anchors += n; all_unplaced += total - n; }
    if(n == 0)
    {
      clu_zero<T>(g, top_n, top, summaries, total);
      __syncthreads();
      continue;
    }
    u32 n2 = 1;
    while(n2 < n) { n2 <<= 1; }
    for(u32 i = n + threadIdx.x; i < n2; i += T) { dk[i] = CLU_NONE; pe[i] = CLU_NONE; }
    __syncthreads();
    // 2.
    clu_bitonic<T, true>(dk, pe, n2);
    // 3.
    for(u32 i = threadIdx.x; i < n; i += T)
    {
      k2[i] = (i > 0 && dk[i] - dk[i - 1] > band ? i : 0);
      acc[i] = 0;
    }
    __syncthreads();
    const u32 per = (n + T - 1) / T, from = (threadIdx.x * per < n ? threadIdx.x * per : n), to = (from + per < n ? from + per : n);
    {
      u64 run = 0;
      for(u32 i = from; i < to; i++) { run = clu_max(run, k2[i]); k2[i] = run; }
      const u64 before = clu_block_before(run, sh.wave);
      for(u32 i = from; i < to; i++) { k2[i] = (clu_max(k2[i], before) << 44) | ((pe[i] >> 32) << 12) | i; }
    }
    for(u32 i = n + threadIdx.x; i < n2; i += T) { k2[i] = CLU_NONE; }
    __syncthreads();
    // 4.
    clu_bitonic<T, false>(k2, nullptr, n2);
    // 5.
    {
      u64 run = 0;
      for(u32 i = from; i < to; i++) { const u64 key = k2[i]; run = clu_max(run, ((key >> 44) << 32) | (pe[key & 0xFFF] & 0xFFFFFFFF)); }
      run = clu_block_before(run, sh.wave);
      u64 cluster = CLU_NONE, sums = 0, prev = (from > 0 && from < to ? k2[from - 1] >> 12 : CLU_NONE);
      for(u32 i = from; i < to; i++)
      {
        const u64 key = k2[i], head = key >> 44, pos = (key >> 12) & 0xFFFFFFFF, end = pe[key & 0xFFF] & 0xFFFFFFFF;
        const u64 reached = ((run >> 32) == head ? run & 0xFFFFFFFF : 0), lo = clu_max(pos, reached);
        if(head != cluster)
        {
          if(sums != 0) { atomicAdd(acc + cluster, (unsigned long long)sums); }
          cluster = head; sums = 0;
        }
        sums += ((end > lo ? end - lo : 0) << 26) + (u64(1) << 13) + ((key >> 12) != prev ? 1 : 0);
        prev = key >> 12;
        run = clu_max(run, (head << 32) | end);
      }
      if(sums != 0) { atomicAdd(acc + cluster, (unsigned long long)sums); }
    }
    __syncthreads();
    // 6.
    const CluLdsView view{dk, pe, reinterpret_cast<const u64*>(acc)};
    const u64 clusters = clu_score<T>(view, 0, n, total, g, top_n, top, summaries, sh);
    if(threadIdx.x == 0) { all_clusters += clusters; }
  }
  clu_flush(stat, all_anchors, all_unplaced, all_clusters);
}

// ---- the large path: the groups above the capacity, all at once ---------------------------------------------------------------
// loff (n_groups + 1): the exclusive scan of lsize; the anchors of group g are the places [loff[g], loff[g + 1]) of every
// array here, `count` (< 2^32) in all, and stay there through every sort: a sort key starts with the group.

// One lane per anchor, for the clusters (clu_place) and for the chains (chn_place): its group by a search over loff, then as
// step 1 of the LDS kernels.  (wa, wb): the two words of PLACE, CLU_NONE both for an unplaced anchor; gk = group << 1 | unplaced: the
// placed anchors of a group sort in front of the others.
template<CluPlaceFn PLACE>
__global__ __launch_bounds__(TPB) void k_anchors_large_gather(const u64* __restrict__ loff, u64 n_groups, u64 count, const u64* __restrict__ goff,
                                                              const u64* __restrict__ seeds, const u64* __restrict__ hoff, const u64* __restrict__ hits,
                                                              CluMap map, u64* __restrict__ wa, u64* __restrict__ wb, u64* __restrict__ gk,
                                                              u32* __restrict__ place)
{
  const u64 e = u64(blockIdx.x) * TPB + threadIdx.x;
  if(e >= count) { return; }
  // the last g with loff[g] <= e: loff[0] = 0, loff[n_groups] = count > e (the search of clu_seed_of over the group sizes)
  const u64 g = clu_seed_of(loff, 0, n_groups, e), first = goff[g], last = goff[g + 1], h = hoff[first] + (e - loff[g]), i = clu_seed_of(hoff, first, last, h);
  u64 key = CLU_NONE, p = CLU_NONE;
  const bool placed = PLACE(map, hits[h], seeds[5 * i], seeds[5 * i + 1], key, p);
  wa[e] = (placed ? key : CLU_NONE); wb[e] = (placed ? p : CLU_NONE); gk[e] = (g << 1) | (placed ? 0 : 1);
  place[e] = u32(e);
}

// the number of placed anchors of a large group behind the sorts: the first of its `total` places with the unplaced bit
__device__ __forceinline__ u64 clu_large_placed(const u64* __restrict__ gk, u64 begin, u64 total)
{
  u64 lo = 0, hi = total;
  while(lo < hi)
  {
    const u64 mid = lo + (hi - lo) / 2;
    if((gk[begin + mid] & 1) == 0) { lo = mid + 1; } else { hi = mid; }
  }
  return lo;
}

__global__ __launch_bounds__(TPB) void k_clusters_large_take(const u64* __restrict__ src, const u32* __restrict__ place, u64 count, u64* __restrict__ dst)
{
  const u64 e = u64(blockIdx.x) * TPB + threadIdx.x;
  if(e < count) { dst[e] = src[place[e]]; }
}

// After the sorts by (group, unplaced, diagonal): head[e] = e where a cluster starts and for every unplaced anchor (a cluster
// of its own that nothing reads), else 0; the max-scan of head is the cluster of every anchor.
__global__ __launch_bounds__(TPB) void k_clusters_large_heads(const u64* __restrict__ dk, const u64* __restrict__ gk, u64 count, u64 band, u64* __restrict__ head)
{
  const u64 e = u64(blockIdx.x) * TPB + threadIdx.x;
  if(e >= count) { return; }
  const u64 mine = gk[e];
  const bool starts = (mine & 1) != 0 || e == 0 || gk[e - 1] != mine || dk[e] - dk[e - 1] > band;
  head[e] = (starts ? e : 0);
}

// the second key, head << 32 | position (0 for an unplaced anchor, alone in its cluster)
__global__ __launch_bounds__(TPB) void k_clusters_large_keys(const u64* __restrict__ head, const u64* __restrict__ pe, const u64* __restrict__ gk, u64 count,
                                                             u64* __restrict__ key2, u32* __restrict__ place)
{
  const u64 e = u64(blockIdx.x) * TPB + threadIdx.x;
  if(e >= count) { return; }
  key2[e] = (head[e] << 32) | ((gk[e] & 1) != 0 ? 0 : pe[e] >> 32);
  place[e] = u32(e);
}

// in (cluster, position) order: head << 32 | end, whose max-scan is the running end inside a cluster
__global__ __launch_bounds__(TPB) void k_clusters_large_ends(const u64* __restrict__ key2, const u32* __restrict__ place, const u64* __restrict__ pe,
                                                             const u64* __restrict__ gk, u64 count, u64* __restrict__ ends)
{
  const u64 e = u64(blockIdx.x) * TPB + threadIdx.x;
  if(e >= count) { return; }
  const u64 at = place[e];
  ends[e] = (key2[e] & ~u64(0xFFFFFFFF)) | ((gk[at] & 1) != 0 ? 0 : pe[at] & 0xFFFFFFFF);
}

// covered << 32 | starts of every anchor, for a wrapping sum-scan: what it adds beyond the running end, and whether its
// (cluster, position) is new
__global__ __launch_bounds__(TPB) void k_clusters_large_cover(const u64* __restrict__ key2, const u64* __restrict__ ends, const u64* __restrict__ reach,
                                                              const u64* __restrict__ gk, u64 count, u64* __restrict__ cover)
{
  const u64 e = u64(blockIdx.x) * TPB + threadIdx.x;
  if(e >= count) { return; }
  if((gk[e] & 1) != 0) { cover[e] = 0; return; }             // the places of a group's unplaced anchors are the same in both orders
  const u64 key = key2[e], head = key >> 32, pos = key & 0xFFFFFFFF, end = ends[e] & 0xFFFFFFFF;
  const u64 before = (e > 0 ? reach[e - 1] : 0), reached = (e > 0 && (before >> 32) == head ? before & 0xFFFFFFFF : 0), lo = clu_max(pos, reached);
  cover[e] = ((end > lo ? end - lo : 0) << 32) | (e == 0 || key2[e - 1] != key ? 1 : 0);
}

// One workgroup per group above the capacity: its placed anchors are the first of its places; then clu_score over global
// memory.  Three atomics per workgroup for the stats.
__global__ __launch_bounds__(TPB) void k_clusters_large_score(const u64* __restrict__ loff, const u64* __restrict__ lsize, u64 n_groups,
                                                              const u64* __restrict__ dk, const u64* __restrict__ pe, const u64* __restrict__ gk,
                                                              const u64* __restrict__ key2, const u64* __restrict__ sum, u32 top_n,
                                                              gcsa2_cluster* __restrict__ top, gcsa2_cluster_summary* __restrict__ summaries,
                                                              unsigned long long* __restrict__ stat)
{
  __shared__ CluShared sh;
  u64 all_anchors = 0, all_unplaced = 0, all_clusters = 0;
  for(u64 g = blockIdx.x; g < n_groups; g += gridDim.x)
  {
    const u64 total = lsize[g];
    if(total == 0) { continue; }
    const u64 begin = loff[g], n = clu_large_placed(gk, begin, total);
    if(n == 0)
    {
      clu_zero<TPB>(g, top_n, top, summaries, total);
      if(threadIdx.x == 0) { all_unplaced += total; }
      continue;
    }
    const CluGlobalView view{dk, pe, key2, sum};
    const u64 clusters = clu_score<TPB>(view, begin, begin + n, total, g, top_n, top, summaries, sh);
    if(threadIdx.x == 0) { all_anchors += n; all_unplaced += total - n; all_clusters += clusters; }
  }
  clu_flush(stat, all_anchors, all_unplaced, all_clusters);
}

}  // namespace
