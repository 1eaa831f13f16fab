// Exercises GCSA::canonical_minimizers and GCSA::stranded_minimizer_hits_batch of the facade.  Reads come one per line (an empty
// line is an empty read).  Prints "read q minimizers" per read, "group g seeds" per group (two per read), "minimizer i position
// hash key strand" per minimizer, "seed i position length sp ep count" per seed and "hits i n v1 .. vn" per seed;
// tests/test_stranded_hits.py compares the lines with the Python calls.
//
//   stranded_hits_client index.g2hv reads.txt k w hash_seed strands(1|2|3) hit_max sample(0|1)
#include <gcsa2_hip/gcsa.hpp>

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 9) { std::cerr << "usage: stranded_hits_client index.g2hv reads.txt k w hash_seed strands(1|2|3) hit_max sample(0|1)" << std::endl; return 2; }
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
  const gcsa::size_type k = std::strtoull(argv[3], nullptr, 10), w = std::strtoull(argv[4], nullptr, 10);
  const gcsa::size_type hash_seed = std::strtoull(argv[5], nullptr, 10), hit_max = std::strtoull(argv[7], nullptr, 10);
  const int strands = std::atoi(argv[6]);
  const bool sample = std::atoi(argv[8]) != 0;

  std::vector<gcsa::size_type> min_offsets, seed_offsets, hit_offsets;
  std::vector<gcsa2_canonical_minimizer> minimizers;
  std::vector<gcsa2_mem> seeds;
  std::vector<gcsa::node_type> hits;
  index.canonical_minimizers(patterns, offsets, k, w, hash_seed, min_offsets, minimizers);
  index.stranded_minimizer_hits_batch(patterns, offsets, k, w, hash_seed, strands, hit_max, sample, seed_offsets, seeds, hit_offsets, hits);
  for(size_t q = 0; q + 1 < min_offsets.size(); q++) { std::cout << "read " << q << " " << min_offsets[q + 1] - min_offsets[q] << "\n"; }
  for(size_t g = 0; g + 1 < seed_offsets.size(); g++) { std::cout << "group " << g << " " << seed_offsets[g + 1] - seed_offsets[g] << "\n"; }
  for(size_t i = 0; i < minimizers.size(); i++)
  {
    const gcsa2_canonical_minimizer& m = minimizers[i];
    std::cout << "minimizer " << i << " " << m.position << " " << m.hash << " " << m.key << " " << m.strand << "\n";
  }
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
