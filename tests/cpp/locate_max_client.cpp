// Exercises GCSA::locate_batch(ranges, max_positions, offsets, values), the batch form of
// GCSA::locate(range, max_positions, results), next to the per-range call.
// Prints "range q size v..." for the batch and "single q size v..." for the per-range call;
// tests/test_locate_max_batch.py compares both with the oracle.
//
//   locate_max_client index.g2hv ranges.txt max_positions
#include <gcsa2_hip/gcsa.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 4) { std::cerr << "usage: locate_max_client index.g2hv ranges.txt max_positions" << std::endl; return 2; }
  gcsa::GCSA index(std::string(argv[1]), 0);
  std::ifstream in(argv[2]);
  std::vector<gcsa::range_type> ranges;
  gcsa::size_type sp = 0, ep = 0;
  while(in >> sp >> ep) { ranges.push_back(gcsa::range_type(sp, ep)); }
  const gcsa::size_type max_positions = std::strtoull(argv[3], nullptr, 0);

  std::vector<gcsa::size_type> offsets;
  std::vector<gcsa::node_type> values;
  index.locate_batch(ranges, max_positions, offsets, values);
  for(size_t q = 0; q < ranges.size(); q++)
  {
    std::cout << "range " << q << " " << (offsets[q + 1] - offsets[q]);
    for(gcsa::size_type i = offsets[q]; i < offsets[q + 1]; i++) { std::cout << " " << values[i]; }
    std::cout << "\n";
  }
  std::vector<gcsa::node_type> results;
  for(size_t q = 0; q < ranges.size(); q++)
  {
    index.locate(ranges[q], max_positions, results);
    std::cout << "single " << q << " " << results.size();
    for(gcsa::node_type v : results) { std::cout << " " << v; }
    std::cout << "\n";
  }
  return 0;
}
