// mt64.hpp -- std::mt19937_64 for device code (GCSA::locate(range, max_positions), src/gcsa.cpp:844-878, draws from
// std::mt19937_64(sp ^ ep)).  Everything here is __host__ __device__ so that a CPU build checks it against the standard
// library (tests/test_mt64.py); it needs nothing but <cstdint>.
//
// The device generator keeps its 312 words in LDS.  Seeding is a serial chain (word i depends on word i - 1).  The twist
// runs on a wavefront in three phases, each in chunks of up to 64 words in which every lane READS its inputs before any lane
// writes (twist_word_at gives the inputs of word k for the phase it belongs to):
//   words   0 .. 155: old words k, k + 1 and k + 156;
//   words 156 .. 310: old words k, k + 1 and the NEW word k - 156 (written by the first phase);
//   word  311       : old word 311 and the NEW words 0 and 155.
// Word k + 1 of a chunk's last lane belongs to the next chunk, which is not written yet.  Every output is tempered on its own.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MT64_HD __host__ __device__
#else
#define MT64_HD
#endif

namespace mt64 {

constexpr int N = 312, M = 156;
constexpr uint64_t MATRIX_A = 0xB5026F5AA96619E9ull;
constexpr uint64_t UPPER = 0xFFFFFFFF80000000ull, LOWER = 0x7FFFFFFFull;
constexpr uint64_t INIT_MULT = 6364136223846793005ull;

MT64_HD inline void seed(uint64_t* x, uint64_t s)
{
  x[0] = s;
  for(int i = 1; i < N; i++) { x[i] = INIT_MULT * (x[i - 1] ^ (x[i - 1] >> 62)) + uint64_t(i); }
}

MT64_HD inline uint64_t twist_word(uint64_t cur, uint64_t next, uint64_t far)
{
  const uint64_t y = (cur & UPPER) | (next & LOWER);
  return far ^ (y >> 1) ^ ((y & 1) ? MATRIX_A : 0);
}

// The new value of word k, read from x as the phase schedule above leaves it.
MT64_HD inline uint64_t twist_word_at(const uint64_t* x, int k)
{
  if(k < N - M) { return twist_word(x[k], x[k + 1], x[k + M]); }
  if(k < N - 1) { return twist_word(x[k], x[k + 1], x[k + M - N]); }
  return twist_word(x[N - 1], x[0], x[M - 1]);
}

// Word ranges of the three phases: [phase_begin(p), phase_begin(p + 1)).
MT64_HD constexpr int phase_begin(int p) { return p == 0 ? 0 : p == 1 ? N - M : p == 2 ? N - 1 : N; }

// The reference twist, one word after the other.
MT64_HD inline void twist(uint64_t* x)
{
  for(int k = 0; k < N; k++) { x[k] = twist_word_at(x, k); }
}

// The phase schedule with `lanes` lanes emulated one after the other: all reads of a chunk, then all writes.
MT64_HD inline void twist_lanes_emulated(uint64_t* x, int lanes)
{
  uint64_t v[64];
  if(lanes < 1) { lanes = 1; }
  if(lanes > 64) { lanes = 64; }
  for(int p = 0; p < 3; p++)
  {
    for(int b = phase_begin(p); b < phase_begin(p + 1); b += lanes)
    {
      const int end = (b + lanes < phase_begin(p + 1) ? b + lanes : phase_begin(p + 1));
      for(int k = b; k < end; k++) { v[k - b] = twist_word_at(x, k); }
      for(int k = b; k < end; k++) { x[k] = v[k - b]; }
    }
  }
}

MT64_HD inline uint64_t temper(uint64_t y)
{
  y ^= (y >> 29) & 0x5555555555555555ull;
  y ^= (y << 17) & 0x71D67FFFEDA60000ull;
  y ^= (y << 37) & 0xFFF7EEE000000000ull;
  y ^= (y >> 43);
  return y;
}

// A serial generator with the interface of std::mt19937_64 (seed, operator()).
struct Engine
{
  uint64_t x[N];
  int pos;
  MT64_HD explicit Engine(uint64_t s = 5489u) { seed(x, s); pos = N; }
  MT64_HD uint64_t operator()()
  {
    if(pos >= N) { twist(x); pos = 0; }
    return temper(x[pos++]);
  }
};

}  // namespace mt64
