// kernels_chains.hpp -- seed chains (gcsa2_seed_chains_device and its fused forms, include/gcsa2_hip_chains.h): per group of
// seed records the top_n colinear chains of its anchors, by a dynamic program over the anchors in (x, q, l) order.  Included by
// gcsa2_hip.hip after kernels_clusters.hpp, whose plan kernel (k_clusters_plan: the groups are validated there, once), placement
// (clu_place), large gather (k_anchors_large_gather, clu_large_placed), zero rows (clu_zero), bitonic sort, top row
// (clu_top_insert, CluShared) and counters (CLU_*, clu_flush; CLU_CLUSTERS counts the chains) it uses.
//
// Data flow: k_clusters_plan -> k_chains_lds (one workgroup per group of up to `cap` anchors: gather and place, bitonic sort by
// (x, q << 32 | qe), chn_dp, bitonic sort of the places by (f descending, place), chn_finish) -> for the groups above the
// capacity k_anchors_large_gather<chn_place>, three stable radix sorts into (group, x, q, l) order, k_chains_large_dp (one wavefront per
// group: chn_dp over global memory), two stable radix sorts into (group, f descending, place) order, k_chains_large_finish (one
// workgroup per group: chn_finish over global memory).  chn_dp and chn_finish are the same code over a view of LDS or of global
// memory.
//
// An anchor is two words: x and pe = q << 32 | qe (clu_place's second word); (x, q, l) order is (x, pe) order.
#pragma once

namespace {

constexpr u32 CHN_NO = 0xFFFFFFFFu;                          // no predecessor; no mark
constexpr u64 CHN_LDS_NO = 0x1FFF;                          // the same in 13 bits of an LDS word: a place in LDS is below 4096
constexpr u64 CHN_X_LIMIT = u64(1) << 62;                   // an anchor at or beyond it is unplaced
// f(i) = match (l_first + the sum of gain over the links of the best chain into i), and gain(j, i) <= dq = qe_i - qe_j, which
// telescopes: f(i) <= match (l_first + qe_i - qe_first) <= match qe_i < 2^16 2^32 = 2^48 (match <= 65536, qe < 2^32 by the
// placement).  A link costs gap drift <= 2^16 (2^32 - 1) < 2^48 (drift <= max(dq, dx) <= max_gap < 2^32), so every candidate
// value is in (-2^48, 2^48) as a signed word, and a chosen one, being above w_i >= 0, is below 2^48 <= CHN_F_LIMIT.
constexpr u64 CHN_F_LIMIT = u64(1) << 50;
static_assert(GCSA2_CHAIN_TOP_LIMIT == GCSA2_CLUSTER_TOP_LIMIT, "the top row of CluShared and clu_top_insert: one lane per chain");
static_assert(GCSA2_CHAIN_LOOKBACK_LIMIT == 64, "lane k of one wavefront evaluates predecessor i - 1 - k");
static_assert(sizeof(gcsa2_chain) == 64 && sizeof(gcsa2_chain_anchor) == 16 && sizeof(gcsa2_chain_summary) == 24, "eight, two and three words");
static_assert((CHN_F_LIMIT << 13) != 0 && ((CHN_F_LIMIT - 1) << 13 >> 13) == CHN_F_LIMIT - 1, "f << 13 | pred is one LDS word");
static_assert(((CHN_F_LIMIT - 1) << 12 | 0xFFF) < CLU_NONE, "the second sort key (F_LIMIT - 1 - f) << 12 | place is below the pad");
static_assert(((CHN_F_LIMIT - 1) << 6 | 63) < (u64(1) << 63), "the key of the wave-wide maximum: value << 6 | 63 - k");

struct ChnParams { u64 band, max_gap, match, gap, min_score, member_cap; u32 lookback, top_n; };

// clu_place and the x < 2^62 rule: the anchor's x and q << 32 | qe, or false: unplaced
__device__ __forceinline__ bool chn_place(const CluMap& map, u64 v, u64 pos, u64 len, u64& x, u64& pe)
{
  u64 key = 0;
  if(!clu_place(map, v, pos, len, key, pe)) { return false; }
  x = (key ^ CLU_BIAS) + pos;
  return x < CHN_X_LIMIT;
}

// The link j -> i of two placed anchors (but for the distance of their places): whether it is allowed, its gain and its drift.
__device__ __forceinline__ bool chn_link(const ChnParams& P, u64 xj, u64 pej, u64 xi, u64 pei, u64& gain, u64& drift)
{
  const u64 qj = pej >> 32, qej = pej & 0xFFFFFFFF, qi = pei >> 32, qei = pei & 0xFFFFFFFF, li = qei - qi, lj = qej - qj;
  const long long dq = (long long)qei - (long long)qej, dx = (long long)(xi + li) - (long long)(xj + lj);     // x + l < 2^62 + 2^32
  const long long d = (dx > dq ? dx - dq : dq - dx);
  gain = li;
  if(dq >= 0 && u64(dq) < gain) { gain = u64(dq); }
  if(dx >= 0 && u64(dx) < gain) { gain = u64(dx); }
  drift = u64(d);
  return qj < qi && xj < xi && dq >= 1 && dx >= 1 && u64(dq) <= P.max_gap && u64(dx) <= P.max_gap && drift <= P.band;
}

__device__ __forceinline__ u64 chn_wave_max(u64 v)
{
#pragma unroll
  for(u32 o = 32; o > 0; o >>= 1) { v = clu_max(v, __shfl_xor(v, o, 64)); }
  return v;
}

// View of a group's placed anchors in (x, q, l) order, of f and pred, of the marks and of the places in (f, place) order.
// In LDS the third array holds f << 13 | pred behind the dynamic program, then pred | mark << 13 (k_chains_lds turns one into
// the other when it makes the sort keys).
struct ChnLdsView
{
  u64 *xs, *pes, *pm, *sk;
  __device__ __forceinline__ u64 x(u64 i) const { return xs[i]; }
  __device__ __forceinline__ u64 pe(u64 i) const { return pes[i]; }
  __device__ __forceinline__ void store_f(u64 i, u64 f, u32 pred) const { pm[i] = (f << 13) | (pred == CHN_NO ? CHN_LDS_NO : u64(pred)); }
  __device__ __forceinline__ u32 pred(u64 i) const { const u64 p = pm[i] & CHN_LDS_NO; return (p == CHN_LDS_NO ? CHN_NO : u32(p)); }
  __device__ __forceinline__ u32 mark(u64 i) const { const u64 m = (pm[i] >> 13) & CHN_LDS_NO; return (m == CHN_LDS_NO ? CHN_NO : u32(m)); }
  __device__ __forceinline__ void set_mark(u64 i, u64 e) const { pm[i] = (pm[i] & CHN_LDS_NO) | (e << 13); }
  __device__ __forceinline__ u64 order(u64 r) const { return sk[r] & 0xFFF; }
};

// The arrays start at the group's first anchor; `ord` holds places of the whole large path, `base` is the group's first.
struct ChnGlobalView
{
  const u64 *xs, *pes;
  u64* fkey;
  u32 *prd, *mrk;
  const u32* ord;
  u64 base;
  __device__ __forceinline__ u64 x(u64 i) const { return xs[i]; }
  __device__ __forceinline__ u64 pe(u64 i) const { return pes[i]; }
  __device__ __forceinline__ void store_f(u64 i, u64 f, u32 pred) const { fkey[i] = CHN_F_LIMIT - 1 - f; prd[i] = pred; }
  __device__ __forceinline__ u32 pred(u64 i) const { return prd[i]; }
  __device__ __forceinline__ u32 mark(u64 i) const { return mrk[i]; }
  __device__ __forceinline__ void set_mark(u64 i, u64 e) const { mrk[i] = u32(e); }
  __device__ __forceinline__ u64 order(u64 r) const { return u64(ord[r]) - base; }
};

// One wavefront: f and pred of the n anchors of the view, one after the other.  At step i lane k holds the record and f of
// anchor i - 1 - k in its registers -- every anchor is read once, by every lane at the same address, one step ahead, and what
// the program stores it does not read again --; the lanes below lookback evaluate their link, one wave-wide maximum of
// value << 6 | 63 - k picks the best value and among equal ones the nearest predecessor, and the window moves up one lane.
template<class View>
__device__ void chn_dp(const View& view, u64 n, const ChnParams& P)
{
  const u32 lane = threadIdx.x & 63;
  u64 wx = 0, wp = 0, wf = 0;                               // the window: anchor i - 1 - lane
  u64 xi = (n > 0 ? view.x(0) : 0), pei = (n > 0 ? view.pe(0) : 0);
  for(u64 i = 0; i < n; i++)
  {
    const u64 next = (i + 1 < n ? i + 1 : i), xn = view.x(next), pn = view.pe(next);
    const u64 w = P.match * ((pei & 0xFFFFFFFF) - (pei >> 32));
    u64 key = 0, gain = 0, drift = 0;
    if(lane < P.lookback && lane < i && chn_link(P, wx, wp, xi, pei, gain, drift))
    {
      const long long value = (long long)wf + (long long)(P.match * gain) - (long long)(P.gap * drift);
      if(value > (long long)w) { key = (u64(value) << 6) | (63 - lane); }
    }
    u64 f = w;
    u32 pred = CHN_NO;
    if(__ballot(key != 0) != 0)
    {
      key = chn_wave_max(key);
      f = key >> 6; pred = u32(i - 1 - (63 - (key & 63)));
    }
    if(lane == 0) { view.store_f(i, f, pred); }
    const u64 ux = __shfl_up(wx, 1, 64), up = __shfl_up(wp, 1, 64), uf = __shfl_up(wf, 1, 64);
    if(lane == 0) { wx = xi; wp = pei; wf = f; } else { wx = ux; wp = up; wf = uf; }
    xi = xn; pei = pn;
  }
}

// clu_zero -- the zero row and the summary {0, unplaced, 0} of an invalid group or one without a placed anchor -- and the
// zero member rows
template<u32 T>
__device__ __forceinline__ void chn_zero(u64 g, const ChnParams& P, gcsa2_chain* __restrict__ top, gcsa2_chain_anchor* __restrict__ members,
                                         gcsa2_chain_summary* __restrict__ summaries, u64 unplaced)
{
  clu_zero<T>(g, P.top_n, top, summaries, unplaced);
  if(members != nullptr)
  {
    u64* rows = reinterpret_cast<u64*>(members + g * P.top_n * P.member_cap);
    for(u64 word = threadIdx.x; word < 2 * P.top_n * P.member_cap; word += T) { rows[word] = 0; }
  }
}

// The whole workgroup, behind chn_dp and the sort of the places: wavefront 0 visits the ends in order -- lane 0 walks (every
// anchor is walked once) and marks with the end's place; a kept chain joins the running top row in the wavefront's registers
// (clu_top_insert: score, then (2^32 - 1 - anchors) << 32 | end) if it is ahead of entry top_n - 1 --, then one thread per
// winner walks its chain again while mark == its end for the record and the member row, and the rows -- zeros behind the last
// chain and behind the last member -- and the summary are stored.  `members` is null unless member_cap > 0.  Returns the
// number of kept chains.
template<u32 T, class View>
__device__ u64 chn_finish(const View& view, u64 n, u64 anchors_all, u64 g, const ChnParams& P, gcsa2_chain* __restrict__ top,
                          gcsa2_chain_anchor* __restrict__ members, gcsa2_chain_summary* __restrict__ summaries, CluShared& sh)
{
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  if(wave == 0)
  {
    u64 rs = 0, rk = CLU_NONE, rx = 0, kept = 0;
    for(u64 r = 0; r < n; r++)
    {
      u64 s = 0, k = CLU_NONE;
      bool keep = false;
      if(lane == 0)
      {
        const u64 e = view.order(r);
        if(view.mark(e) == CHN_NO)
        {
          u64 i = e, anchors = 0, matched = 0, drift = 0, xi = view.x(i), pei = view.pe(i);
          for(;;)
          {
            view.set_mark(i, e);
            anchors++;
            const u32 p = view.pred(i);
            if(p == CHN_NO) { matched += (pei & 0xFFFFFFFF) - (pei >> 32); break; }
            const u64 xp = view.x(p), pp = view.pe(p);
            u64 gain = 0, d = 0;
            chn_link(P, xp, pp, xi, pei, gain, d);
            matched += gain; drift += d;
            if(view.mark(p) != CHN_NO) { break; }
            i = p; xi = xp; pei = pp;
          }
          const long long score = (long long)(P.match * matched) - (long long)(P.gap * drift);
          if(score >= (long long)P.min_score) { keep = true; s = u64(score); k = ((u64(0xFFFFFFFF) - anchors) << 32) | e; }
        }
      }
      if(__ballot(keep) != 0)
      {
        kept++;
        const u64 ns = __shfl(s, 0, 64), nk = __shfl(k, 0, 64);
        const u64 cut_s = __shfl(rs, int(P.top_n - 1), 64), cut_k = __shfl(rk, int(P.top_n - 1), 64);
        if(clu_ahead(ns, nk, cut_s, cut_k)) { clu_top_insert(rs, rk, rx, ns, nk, 0); }
      }
    }
    sh.win_score[lane] = rs; sh.win_key[lane] = rk;
    if(lane == 0) { sh.clusters = kept; }
  }
  __syncthreads();
  const u64 kept = sh.clusters;
  const u32 winners = u32(kept < P.top_n ? kept : P.top_n);
  u64* row = (top != nullptr ? reinterpret_cast<u64*>(top + g * P.top_n) : nullptr);
  u64* rows = (members != nullptr ? reinterpret_cast<u64*>(members + g * P.top_n * P.member_cap) : nullptr);
  if(row != nullptr || rows != nullptr)
  {
    for(u32 w = threadIdx.x; w < winners; w += T)
    {
      const u64 e = sh.win_key[w] & 0xFFFFFFFF, xe = view.x(e), pe_e = view.pe(e);
      u64* out = (rows != nullptr ? rows + 2 * u64(w) * P.member_cap : nullptr);
      u64 i = e, anchors = 0, matched = 0, drift = 0, xi = xe, pei = pe_e;
      for(;;)
      {
        if(out != nullptr && anchors < P.member_cap)
        {
          out[2 * anchors] = xi; out[2 * anchors + 1] = (pei >> 32) | (((pei & 0xFFFFFFFF) - (pei >> 32)) << 32);      // position, length
        }
        anchors++;
        const u32 p = view.pred(i);
        if(p == CHN_NO) { matched += (pei & 0xFFFFFFFF) - (pei >> 32); break; }
        const u64 xp = view.x(p), pp = view.pe(p);
        u64 gain = 0, d = 0;
        chn_link(P, xp, pp, xi, pei, gain, d);
        matched += gain; drift += d;
        if(view.mark(p) != u32(e)) { break; }
        i = p; xi = xp; pei = pp;
      }
      if(row != nullptr)
      {
        u64* dst = row + 8 * u64(w);
        dst[0] = sh.win_score[w]; dst[1] = anchors; dst[2] = matched; dst[3] = drift;
        dst[4] = pei >> 32; dst[5] = pe_e & 0xFFFFFFFF; dst[6] = xi; dst[7] = xe + ((pe_e & 0xFFFFFFFF) - (pe_e >> 32));
      }
    }
  }
  if(row != nullptr)
  {
    for(u32 word = winners * 8 + threadIdx.x; word < P.top_n * 8; word += T) { row[word] = 0; }
  }
  if(rows != nullptr)
  {
    // what the winners' threads do not write: the entries behind min(anchors, member_cap) of a winner, every entry of an empty slot
    for(u64 at = threadIdx.x; at < u64(P.top_n) * P.member_cap; at += T)
    {
      const u64 slot = at / P.member_cap, m = at % P.member_cap;
      const u64 filled = (slot < winners ? u64(0xFFFFFFFF) - (sh.win_key[slot] >> 32) : 0);
      if(m >= filled) { rows[2 * at] = 0; rows[2 * at + 1] = 0; }
    }
  }
  if(summaries != nullptr && threadIdx.x == 0)
  {
    u64* dst = reinterpret_cast<u64*>(summaries + g);
    dst[0] = n; dst[1] = anchors_all - n; dst[2] = kept;
  }
  __syncthreads();                                           // the top row is read before the next group writes it
  return kept;
}

// ---- the LDS path ------------------------------------------------------------------------------------------------------------

// One workgroup of T lanes per group, striding, launched as k_clusters_lds is: T = 64 for the groups of up to CLU_WAVE_MAX
// anchors, T = 256 for the others; the launch with above == 0 also writes the zero rows.  Dynamic LDS: four arrays of `cap` (a
// power of two) 64-bit words.
//   1. gather: as k_clusters_lds, the placed anchors packed as xs = x, pes = q << 32 | qe
//   2. bitonic sort of (xs, pes), padded with (CLU_NONE, CLU_NONE), which no anchor equals (x < 2^62)
//   3. chn_dp by wavefront 0: pm = f << 13 | pred
//   4. sk = (F_LIMIT - 1 - f) << 12 | place and pm = pred | no mark; bitonic sort of sk
//   5. chn_finish
// Three atomics per workgroup for the stats (clu_flush).
template<u32 T>
__global__ __launch_bounds__(T) void k_chains_lds(const u64* __restrict__ goff, u64 n_groups, const u64* __restrict__ seeds, const u64* __restrict__ hoff,
                                                    const u64* __restrict__ hits, const u64* __restrict__ info, CluMap map, ChnParams P, u32 cap,
                                                    u64 above, u64 spill, gcsa2_chain* __restrict__ top, gcsa2_chain_anchor* __restrict__ members,
                                                    gcsa2_chain_summary* __restrict__ summaries, unsigned long long* __restrict__ stat)
{
  extern __shared__ u64 chn_words[];
  __shared__ CluShared sh;
  const ChnLdsView view{chn_words, chn_words + cap, chn_words + 2 * size_t(cap), chn_words + 3 * size_t(cap)};
  const u32 lane = threadIdx.x & 63;
  u64 all_anchors = 0, all_unplaced = 0, all_chains = 0;
  for(u64 g = blockIdx.x; g < n_groups; g += gridDim.x)
  {
    const u64 total = info[g];
    if(total == CLU_INFO_INVALID || total == 0)
    {
      if(above == 0) { chn_zero<T>(g, P, top, members, summaries, 0); }
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
      u64 x = 0, p = 0;
      bool placed = false;
      if(a < total)
      {
        const u64 h = h0 + a, i = clu_seed_of(hoff, first, last, h);
        placed = chn_place(map, hits[h], seeds[5 * i], seeds[5 * i + 1], x, p);
      }
      const u64 mask = __ballot(placed);
      u32 at = 0;
      if(lane == 0 && mask != 0) { at = atomicAdd(&sh.count, u32(__popcll(mask))); }
      at = __shfl(at, 0, 64) + u32(__popcll(mask & ((u64(1) << lane) - 1)));
      if(placed) { view.xs[at] = x; view.pes[at] = p; }      // at < total <= cap
    }
    __syncthreads();
    const u32 n = sh.count;
    if(threadIdx.x == 0) { all_anchors += n; all_unplaced += total - n; }
    if(n == 0)
    {
      chn_zero<T>(g, P, top, members, summaries, total);
      __syncthreads();
      continue;
    }
    u32 n2 = 1;
    while(n2 < n) { n2 <<= 1; }
    for(u32 i = n + threadIdx.x; i < n2; i += T) { view.xs[i] = CLU_NONE; view.pes[i] = CLU_NONE; }
    __syncthreads();
    // 2.
    clu_bitonic<T, true>(view.xs, view.pes, n2);
    // 3.
    if(threadIdx.x < 64) { chn_dp(view, n, P); }
    __syncthreads();
    // 4.
    for(u32 i = threadIdx.x; i < n2; i += T)
    {
      if(i < n)
      {
        const u64 v = view.pm[i];
        view.sk[i] = ((CHN_F_LIMIT - 1 - (v >> 13)) << 12) | i;
        view.pm[i] = (v & CHN_LDS_NO) | (CHN_LDS_NO << 13);
      }
      else { view.sk[i] = CLU_NONE; }
    }
    __syncthreads();
    clu_bitonic<T, false>(view.sk, nullptr, n2);
    // 5.
    const u64 chains = chn_finish<T>(view, n, total, g, P, top, members, summaries, sh);
    if(threadIdx.x == 0) { all_chains += chains; }
  }
  clu_flush(stat, all_anchors, all_unplaced, all_chains);
}

// ---- the large path: the groups above the capacity, all at once ---------------------------------------------------------------
// loff, lsize and the places [loff[g], loff[g + 1]) of a group: as in kernels_clusters.hpp, whose k_anchors_large_gather<chn_place>
// fills xs = x, pes = q << 32 | qe (CLU_NONE both for an unplaced anchor) and gk = group << 1 | unplaced.

// One wavefront per group above the capacity, behind the sorts by (group, unplaced, x, q, l): chn_dp over global memory.  It
// also sets what the next sorts take: fkey (CHN_F_LIMIT for an unplaced anchor: behind every placed one) and place = the index.
__global__ __launch_bounds__(64) void k_chains_large_dp(const u64* __restrict__ loff, const u64* __restrict__ lsize, u64 n_groups, const u64* __restrict__ xs,
                                                        const u64* __restrict__ pes, const u64* __restrict__ gk, ChnParams P, u64* __restrict__ fkey,
                                                        u32* __restrict__ prd, u32* __restrict__ place)
{
  for(u64 g = blockIdx.x; g < n_groups; g += gridDim.x)
  {
    const u64 total = lsize[g];
    if(total == 0) { continue; }
    const u64 begin = loff[g], n = clu_large_placed(gk, begin, total);
    const ChnGlobalView view{xs + begin, pes + begin, fkey + begin, prd + begin, nullptr, nullptr, begin};
    chn_dp(view, n, P);
    for(u64 i = n + threadIdx.x; i < total; i += 64) { fkey[begin + i] = CHN_F_LIMIT; }
    for(u64 i = threadIdx.x; i < total; i += 64) { place[begin + i] = u32(begin + i); }
  }
}

// One workgroup per group above the capacity, behind the sorts by (group, f descending, place): `ord` holds, at the group's
// places, its anchors in the order of the visit (the unplaced ones last).  mrk is CHN_NO everywhere.  Three atomics per
// workgroup for the stats.
__global__ __launch_bounds__(TPB) void k_chains_large_finish(const u64* __restrict__ loff, const u64* __restrict__ lsize, u64 n_groups,
                                                             const u64* __restrict__ xs, const u64* __restrict__ pes, const u64* __restrict__ gk,
                                                             u32* __restrict__ prd, u32* __restrict__ mrk, const u32* __restrict__ ord, ChnParams P,
                                                             gcsa2_chain* __restrict__ top, gcsa2_chain_anchor* __restrict__ members,
                                                             gcsa2_chain_summary* __restrict__ summaries, unsigned long long* __restrict__ stat)
{
  __shared__ CluShared sh;
  u64 all_anchors = 0, all_unplaced = 0, all_chains = 0;
  for(u64 g = blockIdx.x; g < n_groups; g += gridDim.x)
  {
    const u64 total = lsize[g];
    if(total == 0) { continue; }
    const u64 begin = loff[g], n = clu_large_placed(gk, begin, total);
    if(n == 0)
    {
      chn_zero<TPB>(g, P, top, members, summaries, total);
      if(threadIdx.x == 0) { all_unplaced += total; }
      continue;
    }
    const ChnGlobalView view{xs + begin, pes + begin, nullptr, prd + begin, mrk + begin, ord + begin, begin};
    const u64 chains = chn_finish<TPB>(view, n, total, g, P, top, members, summaries, sh);
    if(threadIdx.x == 0) { all_anchors += n; all_unplaced += total - n; all_chains += chains; }
  }
  clu_flush(stat, all_anchors, all_unplaced, all_chains);
}

}  // namespace
