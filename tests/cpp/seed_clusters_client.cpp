// Exercises GCSA::kmer_clusters_batch and GCSA::minimizer_clusters_batch of the facade.  Reads come one per line (an empty line
// is an empty read); the coordinate map is coord_of_bin[b] = b << shift over n_bins bins with every 7th bin unknown.  Prints
// "top q j diag_min diag_max anchors starts covered read_begin read_end ref_begin" for every entry of every row, "summary q
// anchors unplaced clusters" for every read and "stats groups invalid_groups seeds anchors unplaced clusters";
// tests/test_seed_clusters.py compares the lines with the restatement.
//
//   seed_clusters_client index.g2hv reads.txt kmer k stride hit_max shift n_bins band top_n
//   seed_clusters_client index.g2hv reads.txt mini k w      hit_max shift n_bins band top_n
#include <gcsa2_hip/gcsa.hpp>

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 11) { std::cerr << "usage: seed_clusters_client index.g2hv reads.txt kmer|mini k stride|w hit_max shift n_bins band top_n" << std::endl; return 2; }
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
  const std::string form(argv[3]);
  const gcsa::size_type k = std::strtoull(argv[4], nullptr, 10), step = std::strtoull(argv[5], nullptr, 10);
  const gcsa::size_type hit_max = std::strtoull(argv[6], nullptr, 10), shift = std::strtoull(argv[7], nullptr, 10);
  const gcsa::size_type n_bins = std::strtoull(argv[8], nullptr, 10), band = std::strtoull(argv[9], nullptr, 10);
  const gcsa::size_type top_n = std::strtoull(argv[10], nullptr, 10);
  std::vector<gcsa::size_type> coord_of_bin(n_bins);
  for(gcsa::size_type b = 0; b < n_bins; b++) { coord_of_bin[b] = (b % 7 == 0 ? GCSA2_UNKNOWN : b << shift); }
  std::vector<gcsa2_cluster> top;
  std::vector<gcsa2_cluster_summary> summaries;
  gcsa2_cluster_stats stats;
  if(form == "kmer") { index.kmer_clusters_batch(patterns, offsets, k, step, hit_max, false, shift, coord_of_bin, band, top_n, top, summaries, &stats); }
  else if(form == "mini") { index.minimizer_clusters_batch(patterns, offsets, k, step, 0, hit_max, false, shift, coord_of_bin, band, top_n, top, summaries, &stats); }
  else { std::cerr << "unknown form " << form << std::endl; return 2; }
  for(size_t q = 0; q < summaries.size(); q++)
  {
    for(gcsa::size_type j = 0; j < top_n; j++)
    {
      const gcsa2_cluster& c = top[q * top_n + j];
      std::cout << "top " << q << " " << j << " " << c.diag_min << " " << c.diag_max << " " << c.anchors << " " << c.starts << " " << c.covered << " "
                << c.read_begin << " " << c.read_end << " " << c.ref_begin << "\n";
    }
  }
  for(size_t q = 0; q < summaries.size(); q++)
  {
    std::cout << "summary " << q << " " << summaries[q].anchors << " " << summaries[q].unplaced << " " << summaries[q].clusters << "\n";
  }
  std::cout << "stats " << stats.groups << " " << stats.invalid_groups << " " << stats.seeds << " " << stats.anchors << " " << stats.unplaced << " "
            << stats.clusters << "\n";
  return 0;
}
