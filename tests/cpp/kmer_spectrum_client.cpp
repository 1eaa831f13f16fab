// Exercises kmerSpectrum and listKMers of the facade.  Prints "stats kmers nodes occurrences unique max_value", "bin i value"
// for every histogram bin that is not zero, and "listed m nodes occurrences" for the k-mers of listKMers within [min_value,
// max_value] (m records, the sums of their `nodes` and `count` fields); tests/test_kmer_spectrum.py compares the lines with
// the oracle.
//
//   kmer_spectrum_client index.g2hv k include_ns(0|1) force(0|1) n_hist counts(0|1) min_value max_value
#include <gcsa2_hip/gcsa.hpp>

#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
  if(argc < 9) { std::cerr << "usage: kmer_spectrum_client index.g2hv k include_ns(0|1) force(0|1) n_hist counts(0|1) min_value max_value" << std::endl; return 2; }
  gcsa::GCSA index(std::string(argv[1]), 0);
  const gcsa::size_type k = std::strtoull(argv[2], nullptr, 10);
  gcsa::KMerSearchParameters parameters;
  parameters.include_Ns = std::atoi(argv[3]) != 0;
  parameters.force = std::atoi(argv[4]) != 0;
  std::vector<gcsa::size_type> histogram(std::strtoull(argv[5], nullptr, 10), 7);     // overwritten, not added to
  const bool counts = std::atoi(argv[6]) != 0;
  const gcsa::size_type min_value = std::strtoull(argv[7], nullptr, 10), max_value = std::strtoull(argv[8], nullptr, 10);
  const gcsa2_spectrum_stats stats = gcsa::kmerSpectrum(index, k, parameters, histogram, counts);
  std::cout << "stats " << stats.kmers << " " << stats.nodes << " " << stats.occurrences << " " << stats.unique << " " << stats.max_value << "\n";
  for(size_t i = 0; i < histogram.size(); i++) { if(histogram[i] != 0) { std::cout << "bin " << i << " " << histogram[i] << "\n"; } }
  const std::vector<gcsa2_index_kmer> listed = gcsa::listKMers(index, k, parameters, min_value, max_value, counts);
  gcsa::size_type nodes = 0, occurrences = 0;
  for(const gcsa2_index_kmer& r : listed) { nodes += r.nodes; occurrences += r.count; }
  std::cout << "listed " << listed.size() << " " << nodes << " " << occurrences << "\n";
  return (stats.kmers == gcsa::countKMers(index, k, parameters) ? 0 : 1);
}
