// Exercises GCSA::kmer_chains_batch and GCSA::minimizer_chains_batch of the facade.  Reads come one per line (an empty line is
// an empty read); the coordinate map is coord_of_bin[b] = b << shift over n_bins bins with every 7th bin unknown.  Prints
// "top q j score anchors matched drift read_begin read_end ref_begin ref_end" for every entry of every row, "member q j m x
// position length" for every entry of every member row, "summary q anchors unplaced chains" for every read and "stats groups
// invalid_groups seeds anchors unplaced chains"; tests/test_seed_chains.py compares the lines with the restatement.
//
//   seed_chains_client index.g2hv reads.txt kmer k stride hit_max shift n_bins band max_gap lookback match gap min_score top_n member_cap
//   seed_chains_client index.g2hv reads.txt mini k w      hit_max shift n_bins band max_gap lookback match gap min_score top_n member_cap
#include <gcsa2_hip/gcsa.hpp>

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 17)
  {
    std::cerr << "usage: seed_chains_client index.g2hv reads.txt kmer|mini k stride|w hit_max shift n_bins band max_gap lookback match gap min_score top_n member_cap"
              << std::endl;
    return 2;
  }
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
  std::vector<gcsa::size_type> arg;
  for(int i = 4; i < 17; i++) { arg.push_back(std::strtoull(argv[i], nullptr, 10)); }
  const gcsa::size_type k = arg[0], step = arg[1], hit_max = arg[2], shift = arg[3], n_bins = arg[4];
  gcsa::ChainParameters parameters;
  parameters.band = arg[5]; parameters.max_gap = arg[6]; parameters.lookback = arg[7]; parameters.match = arg[8]; parameters.gap = arg[9];
  parameters.min_score = arg[10]; parameters.top_n = arg[11]; parameters.member_cap = arg[12];
  std::vector<gcsa::size_type> coord_of_bin(n_bins);
  for(gcsa::size_type b = 0; b < n_bins; b++) { coord_of_bin[b] = (b % 7 == 0 ? GCSA2_UNKNOWN : b << shift); }
  std::vector<gcsa2_chain> top;
  std::vector<gcsa2_chain_anchor> members;
  std::vector<gcsa2_chain_summary> summaries;
  gcsa2_chain_stats stats;
  if(form == "kmer") { index.kmer_chains_batch(patterns, offsets, k, step, hit_max, false, shift, coord_of_bin, parameters, top, members, summaries, &stats); }
  else if(form == "mini") { index.minimizer_chains_batch(patterns, offsets, k, step, 0, hit_max, false, shift, coord_of_bin, parameters, top, members, summaries, &stats); }
  else { std::cerr << "unknown form " << form << std::endl; return 2; }
  const gcsa::size_type top_n = parameters.top_n, cap = parameters.member_cap;
  for(size_t q = 0; q < summaries.size(); q++)
  {
    for(gcsa::size_type j = 0; j < top_n; j++)
    {
      const gcsa2_chain& c = top[q * top_n + j];
      std::cout << "top " << q << " " << j << " " << c.score << " " << c.anchors << " " << c.matched << " " << c.drift << " " << c.read_begin << " "
                << c.read_end << " " << c.ref_begin << " " << c.ref_end << "\n";
    }
  }
  for(size_t q = 0; q < summaries.size(); q++)
  {
    for(gcsa::size_type j = 0; j < top_n; j++)
    {
      for(gcsa::size_type m = 0; m < cap; m++)
      {
        const gcsa2_chain_anchor& a = members[(q * top_n + j) * cap + m];
        std::cout << "member " << q << " " << j << " " << m << " " << a.x << " " << a.position << " " << a.length << "\n";
      }
    }
  }
  for(size_t q = 0; q < summaries.size(); q++)
  {
    std::cout << "summary " << q << " " << summaries[q].anchors << " " << summaries[q].unplaced << " " << summaries[q].chains << "\n";
  }
  std::cout << "stats " << stats.groups << " " << stats.invalid_groups << " " << stats.seeds << " " << stats.anchors << " " << stats.unplaced << " "
            << stats.chains << "\n";
  return 0;
}
