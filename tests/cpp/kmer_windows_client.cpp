// Exercises GCSA::kmer_windows_batch of the facade.  Reads come one per line (an empty line is an empty read).  Prints
// "read q windows found nodes occurrences" per read, then "window w sp ep count" per window; tests/test_kmer_windows.py
// compares the lines with the Python call.
//
//   kmer_windows_client index.g2hv reads.txt k stride counts(0|1)
#include <gcsa2_hip/gcsa.hpp>

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 6) { std::cerr << "usage: kmer_windows_client index.g2hv reads.txt k stride counts(0|1)" << std::endl; return 2; }
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
  const bool counts = std::atoi(argv[5]) != 0;

  const gcsa::GCSA::KMerWindows out = index.kmer_windows_batch(patterns, offsets, k, stride, counts);
  for(size_t q = 0; q < out.profiles.size(); q++)
  {
    const gcsa2_kmer_profile& p = out.profiles[q];
    std::cout << "read " << q << " " << p.windows << " " << p.found << " " << p.nodes << " " << p.occurrences << "\n";
  }
  for(size_t w = 0; w < out.ranges.size(); w++)
  {
    std::cout << "window " << w << " " << out.ranges[w].first << " " << out.ranges[w].second << " " << (counts ? out.counts[w] : 0) << "\n";
  }
  return 0;
}
