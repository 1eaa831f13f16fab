// Exercises GCSA::kmer_top_classes_batch of the facade.  Reads come one per line (an empty line is an empty read); the class
// map is class_of_bin[b] = b % modulus over n_bins bins.  Prints "stats windows found counted distinct values votes unclassified
// ambiguous", "summary q voted total counted" for every read and "top q j class votes" for every entry of its top row;
// tests/test_kmer_top_classes.py compares the lines with the Python call.
//
//   kmer_top_classes_client index.g2hv reads.txt k stride hit_max shift flags n_bins modulus n_classes top_n
#include <gcsa2_hip/gcsa.hpp>

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 12) { std::cerr << "usage: kmer_top_classes_client index.g2hv reads.txt k stride hit_max shift flags n_bins modulus n_classes top_n" << std::endl; return 2; }
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
  const int flags = std::atoi(argv[7]);
  const gcsa::size_type n_bins = std::strtoull(argv[8], nullptr, 10), modulus = std::strtoull(argv[9], nullptr, 10);
  const gcsa::size_type n_classes = std::strtoull(argv[10], nullptr, 10), top_n = std::strtoull(argv[11], nullptr, 10);
  std::vector<std::uint32_t> class_of_bin(n_bins);
  for(gcsa::size_type b = 0; b < n_bins; b++) { class_of_bin[b] = std::uint32_t(b % modulus); }
  std::vector<gcsa2_class_vote> top;
  std::vector<gcsa2_top_summary> summaries;
  gcsa2_class_stats stats;
  index.kmer_top_classes_batch(patterns, offsets, k, stride, hit_max, shift, flags, class_of_bin, n_classes, top_n, top, summaries, &stats);
  std::cout << "stats " << stats.windows << " " << stats.found << " " << stats.counted << " " << stats.distinct << " " << stats.values << " "
            << stats.votes << " " << stats.unclassified << " " << stats.ambiguous << "\n";
  for(size_t q = 0; q < summaries.size(); q++)
  {
    std::cout << "summary " << q << " " << summaries[q].voted << " " << summaries[q].total << " " << summaries[q].counted << "\n";
  }
  for(size_t q = 0; q < summaries.size(); q++)
  {
    for(gcsa::size_type j = 0; j < top_n; j++) { std::cout << "top " << q << " " << j << " " << top[q * top_n + j].class_id << " " << top[q * top_n + j].votes << "\n"; }
  }
  return 0;
}
