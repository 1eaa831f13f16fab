// Exercises the bounded overloads of the facade with max_length = order(), what a mapper passes:
// GCSA::match_breaks_batch(patterns, offsets, min_length, max_length, ...) and
// GCSA::mem_hits_batch(patterns, offsets, min_length, max_length, hit_max, sample, ...).
// Patterns come one per line (an empty line is an empty pattern).  Prints "order k", then "breaks q n" per pattern and
// "break i position length sp ep" per record, then "pattern q mems" per pattern, "mem i position length sp ep count" per MEM
// and "hits i size v..." per MEM; tests/test_bounded_mems.py compares the lines with the Python calls.
//
//   bounded_mems_client index.g2hv patterns.txt min_length hit_max sample
#include <gcsa2_hip/gcsa.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 6) { std::cerr << "usage: bounded_mems_client index.g2hv patterns.txt min_length hit_max sample" << std::endl; return 2; }
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
  const gcsa::size_type min_length = std::strtoull(argv[3], nullptr, 0);
  const gcsa::size_type hit_max = std::strtoull(argv[4], nullptr, 0);
  const bool sample = std::atoi(argv[5]) != 0;
  const gcsa::size_type max_length = index.order();
  std::cout << "order " << max_length << "\n";

  std::vector<gcsa::size_type> break_offsets;
  std::vector<gcsa2_break> breaks;
  index.match_breaks_batch(patterns, offsets, min_length, max_length, break_offsets, breaks);
  for(size_t q = 0; q + 1 < offsets.size(); q++) { std::cout << "breaks " << q << " " << (break_offsets[q + 1] - break_offsets[q]) << "\n"; }
  for(size_t i = 0; i < breaks.size(); i++)
  {
    const gcsa2_break& b = breaks[i];
    std::cout << "break " << i << " " << b.position << " " << b.length << " " << b.sp << " " << b.ep << "\n";
  }

  std::vector<gcsa::size_type> mem_offsets, hit_offsets;
  std::vector<gcsa2_mem> mems;
  std::vector<gcsa::node_type> hits;
  index.mem_hits_batch(patterns, offsets, min_length, max_length, hit_max, sample, mem_offsets, mems, hit_offsets, hits);
  for(size_t q = 0; q + 1 < offsets.size(); q++) { std::cout << "pattern " << q << " " << (mem_offsets[q + 1] - mem_offsets[q]) << "\n"; }
  for(size_t i = 0; i < mems.size(); i++)
  {
    const gcsa2_mem& m = mems[i];
    std::cout << "mem " << i << " " << m.position << " " << m.length << " " << m.sp << " " << m.ep << " " << m.count << "\n";
  }
  for(size_t i = 0; i < mems.size(); i++)
  {
    std::cout << "hits " << i << " " << (hit_offsets[i + 1] - hit_offsets[i]);
    for(gcsa::size_type j = hit_offsets[i]; j < hit_offsets[i + 1]; j++) { std::cout << " " << hits[j]; }
    std::cout << "\n";
  }
  return 0;
}
