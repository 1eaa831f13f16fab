// Exercises GCSA::extend_batch of the facade.  Patterns come one per line (an empty line is an empty pattern), states one per
// line as "pattern begin end sp ep".  Prints "state i matched sp ep last_sp last_ep" per state; tests/test_extend.py compares
// the lines with the walk of the contract (include/gcsa2_hip.h).
//
//   extend_client index.g2hv patterns.txt states.txt
#include <gcsa2_hip/gcsa.hpp>

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 4) { std::cerr << "usage: extend_client index.g2hv patterns.txt states.txt" << std::endl; return 2; }
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
  std::ifstream state_file(argv[3]);
  std::vector<gcsa2_search_state> states;
  gcsa2_search_state s;
  while(state_file >> s.pattern >> s.begin >> s.end >> s.sp >> s.ep) { states.push_back(s); }

  const std::vector<gcsa2_extension> out = index.extend_batch(patterns, offsets, states);
  for(size_t i = 0; i < out.size(); i++)
  {
    const gcsa2_extension& x = out[i];
    std::cout << "state " << i << " " << x.matched << " " << x.sp << " " << x.ep << " " << x.last_sp << " " << x.last_ep << "\n";
  }
  return 0;
}
