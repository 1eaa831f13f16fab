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
// The body is kernels_minimizers_body.hpp, which k_canonical_minimizers (kernels_strands.hpp) shares.
template<bool PLACE>
__global__ __launch_bounds__(MINI_TPB) void k_minimizers(DevImage img, const u8* __restrict__ patterns, const u64* __restrict__ offsets, u64 n_patterns,
                                                         u32 k, u32 w, u64 hash_seed, u64* __restrict__ sizes, const u64* __restrict__ min_offsets,
                                                         gcsa2_minimizer* __restrict__ recs)
{
#define MINI_CANONICAL 0
#include "kernels_minimizers_body.hpp"
#undef MINI_CANONICAL
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
