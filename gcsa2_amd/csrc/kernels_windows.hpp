// kernels_windows.hpp -- k-mer windows: find() (and count()) of every window P_q[j stride, j stride + k) of every read of a
// pattern set, with per-read profiles (gcsa2_kmer_windows_device).  The block machinery is k_find2's (kernels_find.hpp),
// count() is count_range and the lanes' brackets are k_block_owners' (kernels_locate.hpp).
// Part of the single translation unit gcsa2_hip.hip (device code, anonymous namespace).
#pragma once

#include "kernels_find.hpp"

using namespace g2;

namespace {

// W_q of every read (gcsa2_hip.h), to be scanned into the window offsets; entry n_patterns is the scan's closing zero.
__global__ __launch_bounds__(TPB) void k_window_counts(const u64* __restrict__ offsets, u64 n_patterns, u64 k, u64 stride,
                                                       u64* __restrict__ out)
{
  const u64 q = u64(blockIdx.x) * TPB + threadIdx.x;
  if(q > n_patterns) { return; }
  u64 windows = 0;
  if(q < n_patterns)
  {
    const u64 len = offsets[q + 1] - offsets[q];
    if(len >= k) { windows = (len - k) / stride + 1; }
  }
  out[q] = windows;
}

// One lane = one window; no per-window record exists in memory.  A lane finds its read in the window offsets between the
// reads of its wavefront's first window and of the next wavefront's first window, which k_block_owners (kernels_locate.hpp)
// has found beforehand, one lane per 64 windows: at 119 windows per read that is no probe or one, and never more than the
// few of a search among 64 reads.  (The first form had two lanes of every workgroup search all reads while the others waited
// at the barrier -- twenty dependent loads in front of every workgroup's first block fetch: 18.5 ms for 119 M windows, against
// 16.9 ms in this form and 17.1 ms for k_extend over prebuilt states; profiles/kmer_windows.md.  k_locate_tab met the same.)
//
// The search is k_find2's for the pattern P_q[j stride, j stride + k): the seed-table entry of its last kmer_k characters
// (wide entries and other than fast characters start from charRange), pair steps with single-step replay where the image has
// pair blocks, single steps otherwise, all through the wave-cooperative block fetch.  The jump table is NOT consulted, on any
// image: it is pure memoisation of single steps (the ranges are the same with and without it; tests/test_kmer_windows.py
// compares with gcsa2_find_device on an image that has one), a 32-mer has 20 characters left behind a 12-character seed-table
// entry, and the table would cost this kernel a second code path.  Its effect here has not been measured.
//
// COUNTS: count() of the final range, in this kernel -- the profile-only mode then needs no per-window buffer at all.
// Profiles: the lanes of a wave hold non-decreasing reads, so a segmented inclusive scan by read (six shuffle rounds) leaves
// the wave's partial sums of a read in the last lane of its segment, which adds them to the read's profile with three u64
// atomics: one set per (wave, read), never per window.  Integer sums: the result does not depend on the order of arrival.
// The lane of a read's window 0 stores profile.windows (the library zeroes the profiles in front of the launch).
//
// Emission (k_kmer_seeds, gcsa2_kmer_hits_device; KMER_WINDOWS_EMIT in kernels_windows_body.hpp): instead of per-window
// buffers, the windows with a non-empty range leave the kernel as records, compacted.  The found lanes of a wavefront are
// ranked with a ballot, lane 0 reserves the wavefront's records with ONE atomic add on a global cursor, and the lanes write
// {position, length, sp, ep} and count() at arrival base + rank: window order inside the wavefront, arrival order between
// wavefronts.  Beyond `capacity` records a wavefront only counts, so the cursor ends as the number of seeds whatever the
// capacity was.  Every wavefront leaves its arrival base, its number of found windows and the ballot (16 bytes per 64
// windows); nothing here waits for another wavefront -- putting the records into window order is k_seed_place's job, after a
// scan of the found numbers.
struct SeedEmit
{
  unsigned long long* cursor;    // records reserved so far, in the end the number of seeds
  u64 capacity;                  // records that recs / counts hold
  u64* recs;                     // 4 per record, in arrival order
  u64* counts;                   // 1 per record
  u32* base;                     // per wavefront: where its records begin
  u32* found;                    // per wavefront: how many it has (scanned in place into the final offsets)
  u64* mask;                     // per wavefront: the lanes that found their window
};

template<bool PAIR, bool COUNTS>
__global__ __launch_bounds__(TPB2, FIND_WAVES) void k_kmer_windows(DevImage img, const u8* __restrict__ patterns, const u64* __restrict__ offsets,
                                                                   u64 k, u64 stride, const u64* __restrict__ window_offsets, const u64* __restrict__ owners,
                                                                   u64 total, u64* __restrict__ out, u64* __restrict__ counts,
                                                                   gcsa2_kmer_profile* __restrict__ profiles)
{
#define KMER_WINDOWS_EMIT 0
#include "kernels_windows_body.hpp"
#undef KMER_WINDOWS_EMIT
}

// The same search with counts, emitting seed records (above) and, if asked for, the profiles; no per-window output.
template<bool PAIR>
__global__ __launch_bounds__(TPB2, FIND_WAVES) void k_kmer_seeds(DevImage img, const u8* __restrict__ patterns, const u64* __restrict__ offsets,
                                                                 u64 k, u64 stride, const u64* __restrict__ window_offsets, const u64* __restrict__ owners,
                                                                 u64 total, gcsa2_kmer_profile* __restrict__ profiles, SeedEmit emit)
{
  constexpr bool COUNTS = true;
  u64* const out = nullptr;
  u64* const counts = nullptr;
#define KMER_WINDOWS_EMIT 1
#include "kernels_windows_body.hpp"
#undef KMER_WINDOWS_EMIT
}

// The records of every wavefront of k_kmer_seeds from their arrival place to their place in window order: one wavefront per
// wavefront of the search.  offsets: the exclusive scan of SeedEmit::found (spans + 1 entries).  All `seeds` records fit in
// the arrival area when this runs, so base + found <= seeds for every wavefront.
__global__ __launch_bounds__(TPB) void k_seed_place(const u32* __restrict__ base, const u32* __restrict__ offsets, u64 spans,
                                                    const u64* __restrict__ arrived, const u64* __restrict__ arrived_counts,
                                                    u64* __restrict__ recs, u64* __restrict__ counts)
{
  const u64 wave = (u64(blockIdx.x) * TPB + threadIdx.x) / 64;
  const u32 lane = threadIdx.x & 63;
  if(wave >= spans) { return; }
  const u64 from = base[wave], to = offsets[wave], found = offsets[wave + 1] - to;
  for(u64 x = lane; x < 4 * found; x += 64) { recs[4 * to + x] = arrived[4 * from + x]; }
  if(lane < found) { counts[to + lane] = arrived_counts[from + lane]; }
}

// Seed offsets: the seeds in front of read q's first window = the scan at its wavefront + the found lanes below it there.
// q = 0 .. n_patterns; reads behind the last window (and entry n_patterns) get the number of seeds.
__global__ __launch_bounds__(TPB) void k_seed_offsets(const u64* __restrict__ window_offsets, u64 n_patterns, u64 total, u64 spans,
                                                      const u32* __restrict__ offsets, const u64* __restrict__ mask, u64* __restrict__ seed_offsets)
{
  const u64 q = u64(blockIdx.x) * TPB + threadIdx.x;
  if(q > n_patterns) { return; }
  const u64 w = window_offsets[q];
  seed_offsets[q] = (w >= total ? u64(offsets[spans]) : u64(offsets[w / 64]) + u64(__popcll(mask[w / 64] & ((u64(1) << (w & 63)) - 1))));
}

}  // namespace
