// Host driver of gcsa2_amd/csrc/mt64.hpp for tests/test_mt64.py.
//   mt64_driver outputs SEED COUNT      COUNT outputs of mt64::Engine(SEED), then of std::mt19937_64(SEED), one per line
//   mt64_driver twist SEED LANES ROUNDS  "ok" if the phase schedule with LANES lanes equals the serial twist ROUNDS times
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../gcsa2_amd/csrc/mt64.hpp"

int main(int argc, char** argv)
{
  if(argc == 4 && std::strcmp(argv[1], "outputs") == 0)
  {
    const uint64_t seed = std::strtoull(argv[2], nullptr, 0);
    const long count = std::strtol(argv[3], nullptr, 0);
    mt64::Engine mine(seed);
    std::mt19937_64 theirs(seed);
    for(long i = 0; i < count; i++) { std::printf("%llu\n", (unsigned long long)mine()); }
    for(long i = 0; i < count; i++) { std::printf("%llu\n", (unsigned long long)theirs()); }
    return 0;
  }
  if(argc == 5 && std::strcmp(argv[1], "twist") == 0)
  {
    const uint64_t seed = std::strtoull(argv[2], nullptr, 0);
    const int lanes = std::atoi(argv[3]), rounds = std::atoi(argv[4]);
    uint64_t a[mt64::N], b[mt64::N];
    mt64::seed(a, seed);
    mt64::seed(b, seed);
    for(int r = 0; r < rounds; r++)
    {
      mt64::twist(a);
      mt64::twist_lanes_emulated(b, lanes);
      for(int k = 0; k < mt64::N; k++)
      {
        if(a[k] != b[k]) { std::printf("mismatch round %d word %d\n", r, k); return 1; }
      }
    }
    std::printf("ok\n");
    return 0;
  }
  std::fprintf(stderr, "usage: mt64_driver outputs SEED COUNT | twist SEED LANES ROUNDS\n");
  return 2;
}
