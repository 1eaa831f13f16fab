// Exercises GCSA::capped_seeds_batch of the facade.  Reads come one per line (an empty line is an empty read).  Prints
// "read q seeds" per read, "seed i position length sp ep count" per seed and "hits i n v1 .. vn" per seed;
// tests/test_capped_seeds.py compares the lines with the Python call.
//
//   capped_seeds_client index.g2hv reads.txt min_length max_length max_count hit_max sample(0|1)
#include <gcsa2_hip/gcsa.hpp>

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 8) { std::cerr << "usage: capped_seeds_client index.g2hv reads.txt min_length max_length max_count hit_max sample(0|1)" << std::endl; return 2; }
  gcsa::GCSA index(std::string(argv[1]), 0);
  std::ifstream in(argv[2]);
  std::vector<std::uint8_t> patterns;
  std::vector<gcsa::size_type> offsets(1, 0);
  std::string line;
  while(std::getline(in, line))
  {
    patterns.insert(patterns.end(), line.begin(), line.end());
    offsets.push_back(patterns.size());
  }
  const gcsa::size_type min_length = std::strtoull(argv[3], nullptr, 10), max_length = std::strtoull(argv[4], nullptr, 10);
  const gcsa::size_type max_count = std::strtoull(argv[5], nullptr, 10), hit_max = std::strtoull(argv[6], nullptr, 10);
  const bool sample = std::atoi(argv[7]) != 0;

  std::vector<gcsa::size_type> seed_offsets, hit_offsets;
  std::vector<gcsa2_mem> seeds;
  std::vector<gcsa::node_type> hits;
  index.capped_seeds_batch(patterns, offsets, min_length, max_length, max_count, hit_max, sample, seed_offsets, seeds, hit_offsets, hits);
  for(size_t q = 0; q + 1 < seed_offsets.size(); q++) { std::cout << "read " << q << " " << seed_offsets[q + 1] - seed_offsets[q] << "\n"; }
  for(size_t i = 0; i < seeds.size(); i++)
  {
    const gcsa2_mem& s = seeds[i];
    std::cout << "seed " << i << " " << s.position << " " << s.length << " " << s.sp << " " << s.ep << " " << s.count << "\n";
  }
  for(size_t i = 0; i < seeds.size(); i++)
  {
    std::cout << "hits " << i << " " << hit_offsets[i + 1] - hit_offsets[i];
    for(gcsa::size_type j = hit_offsets[i]; j < hit_offsets[i + 1]; j++) { std::cout << " " << hits[j]; }
    std::cout << "\n";
  }
  return 0;
}
