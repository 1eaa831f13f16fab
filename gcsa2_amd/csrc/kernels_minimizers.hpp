// kernels_minimizers.hpp -- (w, k)-minimizers of every read (gcsa2_minimizers_device) and the k-mer seed search over the
// selected windows (gcsa2_minimizer_hits_device).  The search is the body of kernels_windows.hpp with the window taken from
// the list of minimizers instead of j * stride.
// Part of the single translation unit gcsa2_hip.hip (device code, anonymous namespace).
#pragma once

#include "kernels_windows.hpp"

using namespace g2;

namespace {

constexpr u32 MINI_TPB = 64;                   // one wavefront = one workgroup = one read at a time
constexpr u32 MINI_TILE = 64;                  // span starts per tile

// the SplitMix64 finaliser (gcsa2_hip.h)
__device__ __forceinline__ u64 mini_mix64(u64 x)
{
  u64 z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// bit i of x to bit 2 i
__device__ __forceinline__ u64 mini_spread(u32 x)
{
  u64 v = x;
  v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
  v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
  v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
  v = (v | (v << 2)) & 0x3333333333333333ull;
  v = (v | (v << 1)) & 0x5555555555555555ull;
  return v;
}

// 64 bits from bit `at` (< 64) of the 128 bits (lo, hi)
__device__ __forceinline__ u64 mini_bits(u64 lo, u64 hi, u32 at) { return at == 0 ? lo : (lo >> at) | (hi << (64 - at)); }

// The key of the window that begins at character `at` (< 32) of the 64 characters packed in (a, b): 32 characters per word,
// the first one in the top two bits.
__device__ __forceinline__ u64 mini_key(u64 a, u64 b, u32 at, u32 k)
{
  const u64 both = (at == 0 ? a : (a << (2 * at)) | (b >> (64 - 2 * at)));
  return both >> (64 - 2 * k);
}

// The minimizers of read q = blockIdx.x, blockIdx.x + gridDim.x, ...: one wavefront per read, in tiles of 64 span starts.
//
// A tile at window `base` looks at the windows base .. base + 64 + w - 2 (lane l: window base + l and, for l < w - 1, the halo
// window base + 64 + l) and so at no more than 64 + w - 1 + k - 1 <= 158 characters, which the lanes load once, one byte
// each in three rounds.  Three ballots per round turn them into a bad-character mask and the two bit planes of the 2-bit
// codes; the planes of 32 characters are bit-reversed and interleaved into one 64-bit word with the first character on top
// (wave-uniform work on five words), so that a lane builds its key from two words and a funnel shift and its validity from
// a masked test of the bad bits -- no per-character loop.  Characters behind the read's end count as bad: windows behind the
// last one are invalid without a test of their own.
//
// Spans: with V the valid windows as a bit mask, lane l owns the span that STARTS at window s = base + l.  Its length is the
// number of valid windows from s on, at most w; it exists if that is w, or if s begins its run (the run is then shorter than
// w and the span is the whole run).  The minimum over (hash, position) of every span comes from a sparse table in LDS, built in
// place: level j holds the minimum of the 2^j windows from each position on, a lane whose span has floor(log2(length)) == j takes
// its two overlapping blocks while that level is there, and the left block wins ties -- so the leftmost window does.  The
// selected windows are marked in a 128-bit LDS bitmap with atomicOr (many spans mark the same bit; the result does not
// depend on the order).  Bits 64.. belong to the next tile's windows and are carried over to it; bits 0..63 are final, since
// every later span starts behind them, and leave the tile in ascending position through a rank by popcount.
//
// PLACE == false: sizes[q] = the read's number of minimizers (entry n_patterns: the scan's closing zero).  PLACE == true: the
// same walk again, records written from min_offsets[q] on.  (The first form also added every read's number of windows to one
// global counter: a million atomics on one address took 10 of the counting pass's 12 ms; profiles/minimizer_hits.md.)
template<bool PLACE>
__global__ __launch_bounds__(MINI_TPB) void k_minimizers(DevImage img, const u8* __restrict__ patterns, const u64* __restrict__ offsets, u64 n_patterns,
                                                         u32 k, u32 w, u64 hash_seed, u64* __restrict__ sizes, const u64* __restrict__ min_offsets,
                                                         gcsa2_minimizer* __restrict__ recs)
{
  __shared__ u8 c2c[256];
  __shared__ u64 table_hash[2 * MINI_TILE];
  __shared__ u32 table_at[2 * MINI_TILE];
  __shared__ u32 marks[4];
  const u32 lane = threadIdx.x;
#pragma unroll
  for(u32 c = 0; c < 256; c += MINI_TPB) { c2c[c + lane] = img.char2comp[c + lane]; }
  __syncthreads();
  const u32 limit = (img.sigma >= 3 ? (img.sigma - 2 < 4 ? u32(img.sigma - 2) : 4u) : 0u);     // codes 0 .. limit - 1
  const u32 need = MINI_TILE + (w - 1) + (k - 1);            // characters of a tile
  const u64 kmask = (u64(1) << k) - 1;                       // k <= 32
  const u64 below = (u64(1) << lane) - 1;
  if(!PLACE && blockIdx.x == 0 && lane == 0) { sizes[n_patterns] = 0; }

  for(u64 q = blockIdx.x; q < n_patterns; q += gridDim.x)
  {
    const u64 begin = offsets[q], len = offsets[q + 1] - begin;
    const u64 W = (len >= k ? len - k + 1 : 0);
    const u64 out = (PLACE ? min_offsets[q] : 0);
    u64 count = 0, carry = 0;
    bool prev_valid = false;                                 // window base - 1
    for(u64 base = 0; base < W; base += MINI_TILE)
    {
      // 1. the tile's characters as five code words and three words of bad bits
      u64 bad[3], word[5];
#pragma unroll
      for(u32 r = 0; r < 3; r++)
      {
        const u32 c = r * 64 + lane;
        const bool there = c < need && base + c < len;
        const u32 code = (there ? u32(c2c[patterns[begin + base + c]]) - 1 : ~u32(0));
        const bool good = code < limit;
        bad[r] = __ballot(!good);
        const u64 plane0 = __ballot(good && (code & 1) != 0), plane1 = __ballot(good && (code & 2) != 0);
        word[2 * r] = mini_spread(__brev(u32(plane0))) | (mini_spread(__brev(u32(plane1))) << 1);
        if(r < 2) { word[2 * r + 1] = mini_spread(__brev(u32(plane0 >> 32))) | (mini_spread(__brev(u32(plane1 >> 32))) << 1); }
      }
      // 2. hash and validity of the lane's window and of its halo window
      const bool upper = lane >= 32;
      const u32 at = lane & 31;
      const u64 key_main = mini_key(upper ? word[1] : word[0], upper ? word[2] : word[1], at, k);
      const u64 key_halo = mini_key(upper ? word[3] : word[2], upper ? word[4] : word[3], at, k);
      const u64 hash_main = mini_mix64(key_main ^ hash_seed), hash_halo = mini_mix64(key_halo ^ hash_seed);
      const u64 valid_lo = __ballot((mini_bits(bad[0], bad[1], lane) & kmask) == 0);
      const u64 valid_hi = __ballot(lane + 1 < w && (mini_bits(bad[1], bad[2], lane) & kmask) == 0);
      // 3. the span that starts at the lane's window
      const u64 from_here = mini_bits(valid_lo, valid_hi, lane);
      u64 invalid = ~from_here;
      if(w < 64) { invalid |= u64(1) << w; }
      const u32 span = (invalid != 0 ? u32(__ffsll((unsigned long long)invalid)) - 1 : 64u);     // valid windows from here on, at most w
      const bool prev = (lane == 0 ? prev_valid : ((valid_lo >> (lane - 1)) & 1) != 0);
      const bool want = (from_here & 1) != 0 && (span == w || !prev);
      const u32 level = (want ? 31 - u32(__clz(int(span))) : ~u32(0));
      // 4. the sparse table, level by level in place
      __syncthreads();                                       // the previous tile has read its table and marks
      table_hash[lane] = hash_main; table_at[lane] = lane;
      table_hash[MINI_TILE + lane] = hash_halo; table_at[MINI_TILE + lane] = MINI_TILE + lane;
      if(lane < 4) { marks[lane] = 0; }
      __syncthreads();
      u32 best = 0;
      for(u32 j = 0; ; j++)
      {
        const u32 step = u32(1) << j;
        if(level == j)
        {
          const u32 right = lane + span - step;                // < 127: the span ends inside the halo
          const u64 a = table_hash[lane], b = table_hash[right];
          best = (a <= b ? table_at[lane] : table_at[right]);
        }
        if(2 * step > w) { break; }                            // no span needs a higher level
        const u32 hi = MINI_TILE + lane;
        const bool has = hi + step < 2 * MINI_TILE;            // entries without a right half are never asked for
        const u64 x0 = table_hash[lane], y0 = table_hash[lane + step];
        const u32 j0 = table_at[lane + step];
        const u64 x1 = table_hash[hi], y1 = (has ? table_hash[hi + step] : ~u64(0));
        const u32 j1 = (has ? table_at[hi + step] : 0);
        __syncthreads();
        if(y0 < x0) { table_hash[lane] = y0; table_at[lane] = j0; }
        if(has && y1 < x1) { table_hash[hi] = y1; table_at[hi] = j1; }
        __syncthreads();
      }
      // 5. the selected windows: bits 0..63 are final, the rest goes to the next tile
      if(want) { atomicOr(&marks[best >> 5], u32(1) << (best & 31)); }
      __syncthreads();
      const u64 final_bits = (u64(marks[0]) | (u64(marks[1]) << 32)) | carry;
      carry = u64(marks[2]) | (u64(marks[3]) << 32);
      prev_valid = (valid_lo >> 63) != 0;
      if(PLACE && ((final_bits >> lane) & 1) != 0)
      {
        const u64 to = out + count + u64(__popcll(final_bits & below));
        recs[to].position = base + lane; recs[to].hash = hash_main;
      }
      count += u64(__popcll(final_bits));
    }
    if(!PLACE && lane == 0) { sizes[q] = count; }
  }
}

// the stride-1 windows of read q, for the sum that the limit of a call is checked against
struct MiniWindowsOf
{
  const u64* offsets; u64 k;
  __host__ __device__ u64 operator()(u64 q) const { const u64 len = offsets[q + 1] - offsets[q]; return len >= k ? len - k + 1 : 0; }
};

// The k-mer seed search (k_kmer_seeds) over the windows of a position list: window g of the batch is minimizer g, the CSR over
// reads is that of the minimizers.
template<bool PAIR>
__global__ __launch_bounds__(TPB2, FIND_WAVES) void k_minimizer_seeds(DevImage img, const u8* __restrict__ patterns, const u64* __restrict__ offsets,
                                                                      u64 k, const gcsa2_minimizer* __restrict__ mins, const u64* __restrict__ window_offsets,
                                                                      const u64* __restrict__ owners, u64 total, gcsa2_kmer_profile* __restrict__ profiles,
                                                                      SeedEmit emit)
{
  constexpr bool COUNTS = true;
  u64* const out = nullptr;
  u64* const counts = nullptr;
#define KMER_WINDOWS_EMIT 1
#define KMER_WINDOWS_POSITION(g) (mins[g].position)
#include "kernels_windows_body.hpp"
#undef KMER_WINDOWS_POSITION
#undef KMER_WINDOWS_EMIT
}

}  // namespace
