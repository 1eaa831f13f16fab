// Exercises GCSA::minimizer_chain_pairs_batch of the facade.  Reads come one per line, the mates of a pair on consecutive lines;
// the coordinate map is coord_of_bin[b] = b << shift over n_bins bins (no bin is unknown: a fragment spans bins).  Prints
// "chain g j score anchors matched drift read_begin read_end ref_begin ref_end" for every entry of every chain row, "pair p r
// score fragment penalty chain_score left_group left_chain right_group right_chain" for every entry of every pair row, "summary
// p candidates proper kept ignored mate1_score mate1_at mate2_score mate2_at" for every pair and "stats pairs candidates proper
// kept ignored paired unique unique_fragment_sum"; tests/test_chain_pairs.py compares the lines with the binding's.
//
//   chain_pairs_client index.g2hv reads.txt k w hit_max shift n_bins  band max_gap lookback match gap min_score top_n member_cap
//                      orientation min_fragment max_fragment mean_fragment unit cost min_score top_n
#include <gcsa2_hip/gcsa.hpp>

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 24)
  {
    std::cerr << "usage: chain_pairs_client index.g2hv reads.txt k w hit_max shift n_bins band max_gap lookback match gap min_score top_n member_cap "
              << "orientation min_fragment max_fragment mean_fragment unit cost min_score top_n" << std::endl;
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
  std::vector<gcsa::size_type> arg;
  for(int i = 3; i < 24; i++) { arg.push_back(std::strtoull(argv[i], nullptr, 10)); }
  const gcsa::size_type k = arg[0], w = arg[1], hit_max = arg[2], shift = arg[3], n_bins = arg[4];
  gcsa::ChainParameters parameters;
  parameters.band = arg[5]; parameters.max_gap = arg[6]; parameters.lookback = arg[7]; parameters.match = arg[8]; parameters.gap = arg[9];
  parameters.min_score = arg[10]; parameters.top_n = arg[11]; parameters.member_cap = arg[12];
  gcsa::PairParameters pairing;
  pairing.orientation = arg[13]; pairing.min_fragment = arg[14]; pairing.max_fragment = arg[15]; pairing.mean_fragment = arg[16]; pairing.unit = arg[17];
  pairing.cost = arg[18]; pairing.min_score = arg[19]; pairing.top_n = arg[20];
  std::vector<gcsa::size_type> coord_of_bin(n_bins);
  for(gcsa::size_type b = 0; b < n_bins; b++) { coord_of_bin[b] = b << shift; }
  std::vector<gcsa2_chain> chains;
  std::vector<gcsa2_chain_anchor> members;
  std::vector<gcsa2_chain_summary> chain_summaries;
  std::vector<gcsa2_chain_pair> top;
  std::vector<gcsa2_pair_summary> summaries;
  gcsa2_chain_stats chain_stats;
  gcsa2_pair_stats stats;
  index.minimizer_chain_pairs_batch(patterns, offsets, k, w, 0, hit_max, false, shift, coord_of_bin, parameters, pairing, chains, members, chain_summaries, top,
                                    summaries, &chain_stats, &stats);
  for(size_t g = 0; g < chain_summaries.size(); g++)
  {
    for(gcsa::size_type j = 0; j < parameters.top_n; j++)
    {
      const gcsa2_chain& c = chains[g * parameters.top_n + j];
      std::cout << "chain " << g << " " << j << " " << c.score << " " << c.anchors << " " << c.matched << " " << c.drift << " " << c.read_begin << " "
                << c.read_end << " " << c.ref_begin << " " << c.ref_end << "\n";
    }
  }
  for(size_t p = 0; p < summaries.size(); p++)
  {
    for(gcsa::size_type r = 0; r < pairing.top_n; r++)
    {
      const gcsa2_chain_pair& c = top[p * pairing.top_n + r];
      std::cout << "pair " << p << " " << r << " " << c.score << " " << c.fragment << " " << c.penalty << " " << c.chain_score << " " << c.left_group << " "
                << c.left_chain << " " << c.right_group << " " << c.right_chain << "\n";
    }
  }
  for(size_t p = 0; p < summaries.size(); p++)
  {
    const gcsa2_pair_summary& s = summaries[p];
    std::cout << "summary " << p << " " << s.candidates << " " << s.proper << " " << s.kept << " " << s.ignored << " " << s.mate1_score << " " << s.mate1_at << " "
              << s.mate2_score << " " << s.mate2_at << "\n";
  }
  std::cout << "stats " << stats.pairs << " " << stats.candidates << " " << stats.proper << " " << stats.kept << " " << stats.ignored << " " << stats.paired << " "
            << stats.unique << " " << stats.unique_fragment_sum << "\n";
  return 0;
}
