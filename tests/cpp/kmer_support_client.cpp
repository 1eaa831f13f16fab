// Exercises GCSA::kmer_support_batch of the facade.  Reads come one per line (an empty line is an empty read).  The support
// array starts at 5 in every bin, to show that the call adds.  Prints "stats windows found counted distinct values added
// dropped" and "bin i value" for every bin that changed; tests/test_kmer_support.py compares the lines with the Python call.
//
//   kmer_support_client index.g2hv reads.txt k stride hit_max shift per_bin(0|1) n_bins
#include <gcsa2_hip/gcsa.hpp>

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 9) { std::cerr << "usage: kmer_support_client index.g2hv reads.txt k stride hit_max shift per_bin(0|1) n_bins" << std::endl; return 2; }
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
  const gcsa::size_type k = std::strtoull(argv[3], nullptr, 10), stride = std::strtoull(argv[4], nullptr, 10);
  const gcsa::size_type hit_max = std::strtoull(argv[5], nullptr, 10), shift = std::strtoull(argv[6], nullptr, 10);
  const bool per_bin = std::atoi(argv[7]) != 0;
  std::vector<gcsa::size_type> support(std::strtoull(argv[8], nullptr, 10), 5);
  gcsa2_support_stats stats;
  index.kmer_support_batch(patterns, offsets, k, stride, hit_max, shift, per_bin, support, &stats);
  std::cout << "stats " << stats.windows << " " << stats.found << " " << stats.counted << " " << stats.distinct << " " << stats.values << " "
            << stats.added << " " << stats.dropped << "\n";
  for(size_t i = 0; i < support.size(); i++) { if(support[i] != 5) { std::cout << "bin " << i << " " << support[i] << "\n"; } }
  return 0;
}
