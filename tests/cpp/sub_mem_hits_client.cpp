// Exercises GCSA::sub_mem_hits_batch(patterns, offsets, mem_offsets, mems, min_length, reseed_length, hit_max, sample, ...):
// the MEMs of GCSA::mem_hits_batch (no cap) reseeded.  Patterns come one per line (an empty line is an empty pattern).  Prints
// "mem k subs" per MEM, "sub i position length sp ep count" per sub-MEM and "hits i size v..." per sub-MEM;
// tests/test_sub_mems.py compares the lines with GCSA.sub_mem_hits_batch from Python.
//
//   sub_mem_hits_client index.g2hv patterns.txt min_length reseed_length hit_max sample
#include <gcsa2_hip/gcsa.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 7) { std::cerr << "usage: sub_mem_hits_client index.g2hv patterns.txt min_length reseed_length hit_max sample" << std::endl; return 2; }
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
  const gcsa::size_type reseed_length = std::strtoull(argv[4], nullptr, 0);
  const gcsa::size_type hit_max = std::strtoull(argv[5], nullptr, 0);
  const bool sample = std::atoi(argv[6]) != 0;

  std::vector<gcsa::size_type> mem_offsets, mem_hit_offsets, sub_offsets, hit_offsets;
  std::vector<gcsa2_mem> mems, subs;
  std::vector<gcsa::node_type> mem_hits, hits;
  index.mem_hits_batch(patterns, offsets, min_length, 0, false, mem_offsets, mems, mem_hit_offsets, mem_hits);
  index.sub_mem_hits_batch(patterns, offsets, mem_offsets, mems, min_length, reseed_length, hit_max, sample, sub_offsets, subs, hit_offsets, hits);
  for(size_t k = 0; k < mems.size(); k++) { std::cout << "mem " << k << " " << (sub_offsets[k + 1] - sub_offsets[k]) << "\n"; }
  for(size_t i = 0; i < subs.size(); i++)
  {
    const gcsa2_mem& m = subs[i];
    std::cout << "sub " << i << " " << m.position << " " << m.length << " " << m.sp << " " << m.ep << " " << m.count << "\n";
  }
  for(size_t i = 0; i < subs.size(); i++)
  {
    std::cout << "hits " << i << " " << (hit_offsets[i + 1] - hit_offsets[i]);
    for(gcsa::size_type j = hit_offsets[i]; j < hit_offsets[i + 1]; j++) { std::cout << " " << hits[j]; }
    std::cout << "\n";
  }
  return 0;
}
