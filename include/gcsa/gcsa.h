// <gcsa/gcsa.h> of the MI355X engine: class gcsa::GCSA with the reference's public query interface
// (reference include/gcsa/gcsa.h:40-277), every call forwarded to the device image behind the C ABI
// (include/gcsa2_hip.h).  Names, argument meaning, result types and error behaviour are the reference's
// (citations on each method), so a caller such as vg's MEM finder or the reference's own query_gcsa /
// count_kmers tools compiles against this header unchanged; `*_batch` methods are the additional,
// throughput-oriented entry points.  Header-only; link with -lgcsa2_hip.
//
// What differs, by design: an index is a device image, not SDSL members in host memory.  It is immutable and
// shared by copies (copying a GCSA copies a reference).  The SDSL-typed data members of the reference
// (gcsa.h:214-240) do not exist; `header` and `alpha` do.  Construction from an InputGraph is out of scope.
#ifndef GCSA2_HIP_GCSA_GCSA_H
#define GCSA2_HIP_GCSA_GCSA_H

#include "files.h"
#include "support.h"
#include "../gcsa2_hip_chains.h"
#include "../gcsa2_hip_strands.h"
#include "../gcsa2_hip_pairs.h"

namespace gcsa
{

// The parameters of the seed-chain calls (gcsa2_chain_params), with the defaults of the Python binding.
struct ChainParameters
{
  size_type band = 64, max_gap = 5000, lookback = 16, match = 1, gap = 1, min_score = 0, top_n = 5, member_cap = 0;
  gcsa2_chain_params c() const { return gcsa2_chain_params{band, max_gap, lookback, match, gap, min_score, top_n, member_cap}; }
};

// The parameters of the chain-pair calls (gcsa2_pair_params), with the defaults of the Python binding.
struct PairParameters
{
  size_type orientation = GCSA2_PAIR_FR, min_fragment = 0, max_fragment = 1000, mean_fragment = 400, unit = 16, cost = 1, min_score = 0, top_n = 2;
  gcsa2_pair_params c() const { return gcsa2_pair_params{orientation, min_fragment, max_fragment, mean_fragment, unit, cost, min_score, top_n}; }
};

class GCSA
{
public:
  typedef gcsa::size_type size_type;

  GCSA() : handle(nullptr) {}                                                // gcsa.cpp:56-58: an empty index
  GCSA(const GCSA& source) = default;                                        // copies share the immutable device image
  GCSA(GCSA&& source) noexcept { this->take(source); }
  ~GCSA() = default;
  void swap(GCSA& another)
  {
    std::swap(header, another.header); alpha.swap(another.alpha); std::swap(handle, another.handle);
    owner.swap(another.owner); host.swap(another.host);
  }
  GCSA& operator=(const GCSA& source) = default;
  GCSA& operator=(GCSA&& source) noexcept { if(this != &source) { this->take(source); } return *this; }

  inline static const std::string EXTENSION = ".gcsa";                       // gcsa.cpp:51

  // GCSA::load (gcsa.cpp:184-216): reads one serialized index from the stream, builds the device image on
  // Device::current().  Throws std::runtime_error("GCSA::load(): Invalid header: ...") like the reference on a
  // bad header, and on any other inconsistency.  Bytes of the stream after the index are left unread when the
  // stream is seekable.
  void load(std::istream& in)
  {
    const std::streampos start = in.tellg();
    std::vector<char> data = readRest(in);
    gcsa2_view_storage* storage = nullptr;
    std::uint64_t consumed = 0;
    if(gcsa2_host_view_parse_gcsa(data.data(), data.size(), &consumed, &storage) != GCSA2_OK) { throw std::runtime_error(gcsa2_last_error()); }
    std::shared_ptr<gcsa2_view_storage> keep(storage, gcsa2_host_view_free);
    in.clear();
    if(start != std::streampos(-1)) { in.seekg(start + std::streamoff(consumed)); }
    this->adopt(*gcsa2_host_view_get(storage), Device::current(), keep);
  }

  // GCSA::serialize (gcsa.cpp:140-179): the reference's byte stream.  The device image does not keep the host-side
  // arrays, so this works on an index whose host view was retained (retainHostView(true) before it was loaded or
  // created); otherwise it throws.  Returns the number of bytes written; the structure tree is not filled in.
  // EXPERIMENTAL: the SDSL container encodings inside the stream (bit_vector_il rank samples, sd_vector, the stored
  // select_support_mcl directories) are restated from sdsl-lite and have never met a file written by the real library.
  // The reference LOADS stored select directories without checking them, so a mismatch there would surface as wrong
  // select() / locate() answers in reference tools, not as a load error: do not feed files written here to reference tools
  // before one has been compared with the real library's output for the same index.
  size_type serialize(std::ostream& out, sdsl::structure_tree_node* = nullptr, std::string = "") const
  {
    if(!host) { throw std::runtime_error("GCSA::serialize(): the host view of this index was not retained (GCSA::retainHostView)"); }
    std::uint64_t written = 0;
    check(gcsa2_host_view_serialize_gcsa(gcsa2_host_view_get(host.get()), &GCSA::write_to, &out, &written), "GCSA::serialize()");
    return written;
  }
  const std::shared_ptr<gcsa2_index>& shared() const { return owner; }      // for LCPArray(const GCSA&): keeps the image alive
  static bool& retainHostView() { static bool retain = false; return retain; }
  static void retainHostView(bool retain) { retainHostView() = retain; }

  // ---- engine-specific construction ----
  // From the plain arrays of a loaded reference index, onto HIP device `device`.
  explicit GCSA(const gcsa2_host_view& view, int device = 0) : handle(nullptr) { this->adopt(view, device, nullptr); }
  // From a G2HV container file (gcsa2_host_view_save); throws on an invalid header.
  explicit GCSA(const std::string& container_file, int device = 0) : handle(nullptr)
  {
    gcsa2_index* raw = nullptr;
    check(gcsa2_index_create_from_file(container_file.c_str(), device, &raw), "GCSA::GCSA()");
    this->own(raw);
  }
  // From the reference's own files, base.gcsa + (optionally) its .lcp IN ONE IMAGE, which the fused
  // LF + parent kernels need (matching statistics); as query_gcsa opens them (benchmark/query_gcsa.cpp:53-63).
  GCSA(const std::string& gcsa_file, const std::string& lcp_file, int device) : handle(nullptr)
  {
    gcsa2_index* raw = nullptr;
    check(gcsa2_index_create_from_gcsa(gcsa_file.c_str(), lcp_file.empty() ? nullptr : lcp_file.c_str(), device, &raw), "GCSA::load()");
    this->own(raw);
  }

  // ---- high-level interface (gcsa.h:96-128) ----
  template<class Iterator>
  range_type find(Iterator begin, Iterator end) const                       // gcsa.h:96-110
  {
    if(handle == nullptr) { return range_type(0, size_type(0) - 1); }        // empty index: (0, size() - 1), gcsa.h:99
    std::vector<std::uint8_t> pattern(begin, end);
    size_type offsets[2] = { 0, pattern.size() };
    std::uint8_t dummy = 0;
    size_type range[2];
    check(gcsa2_find_batch(handle, pattern.empty() ? &dummy : pattern.data(), offsets, 1, range), "GCSA::find()");
    return range_type(range[0], range[1]);
  }
  template<class Container>
  range_type find(const Container& pattern) const { return find(pattern.begin(), pattern.end()); }   // gcsa.h:112-116
  template<class Element>
  range_type find(const Element* pattern, size_type length) const { return find(pattern, pattern + length); }  // gcsa.h:118-122

  // Batched find: patterns concatenated, pattern q = [offsets[q], offsets[q + 1]).
  std::vector<range_type> find_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets) const
  {
    size_type nq = offsets.empty() ? 0 : offsets.size() - 1;
    std::vector<range_type> result(nq);
    static_assert(sizeof(range_type) == 2 * sizeof(size_type), "range_type must be two packed u64");
    std::uint8_t dummy = 0;
    check(gcsa2_find_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.data(), nq,
                           reinterpret_cast<size_type*>(result.data())), "GCSA::find_batch()");
    return result;
  }

  // Batched extend (gcsa2_extend_batch): state s continues the loop of find() from the range (sp, ep) over
  // P[begin, end) of pattern s.pattern -- what a caller's loop of LF(range, comp) from a stored range does, for many
  // states and without copying substrings out.  An invalid state comes back with matched = GCSA2_UNKNOWN.
  std::vector<gcsa2_extension> extend_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets,
                                            const std::vector<gcsa2_search_state>& states) const
  {
    size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    std::vector<gcsa2_extension> result(states.size());
    std::uint8_t dummy = 0;
    check(gcsa2_extend_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.data(), np, states.data(), states.size(),
                             result.data()), "GCSA::extend_batch()");
    return result;
  }

  // Batched k-mer windows (gcsa2_kmer_windows_batch): find() -- and with `counts` count() -- of every window
  // P_q[j stride, j stride + k) of every read, without copying the windows out.  window_offsets (reads + 1) is the exclusive
  // prefix sum of the windows per read; profiles[q] = { windows, found, nodes, occurrences } of read q (occurrences only
  // with `counts`); ranges / counts are per window, in read order.  What was not asked for stays empty.
  struct KMerWindows
  {
    std::vector<size_type> window_offsets;
    std::vector<gcsa2_kmer_profile> profiles;
    std::vector<range_type> ranges;
    std::vector<size_type> counts;
  };
  KMerWindows kmer_windows_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k,
                                 size_type stride = 1, bool counts = false, bool ranges = true, bool profiles = true) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    const int flags = (counts ? GCSA2_KMER_COUNTS : 0);
    const std::uint8_t dummy = 0;
    const std::uint8_t* data = patterns.empty() ? &dummy : patterns.data();
    KMerWindows result;
    result.window_offsets.assign(np + 1, 0);
    size_type total = 0;      // the offsets alone first: they size the per-window arrays (host arithmetic, no device work)
    check(gcsa2_kmer_windows_batch(handle, data, offsets.data(), np, k, stride, flags, result.window_offsets.data(), nullptr, nullptr,
                                   nullptr, 0, &total), "GCSA::kmer_windows_batch()");
    if(profiles) { result.profiles.resize(np); }
    if(ranges) { result.ranges.resize(total); }
    if(counts) { result.counts.resize(total); }
    if(!profiles && !ranges && !counts) { return result; }
    static_assert(sizeof(range_type) == 2 * sizeof(size_type), "range_type must be two packed u64");
    check(gcsa2_kmer_windows_batch(handle, data, offsets.data(), np, k, stride, flags, nullptr, profiles ? result.profiles.data() : nullptr,
                                   ranges ? reinterpret_cast<size_type*>(result.ranges.data()) : nullptr,
                                   counts ? result.counts.data() : nullptr, total, &total), "GCSA::kmer_windows_batch()");
    return result;
  }

  // Batched find of k-mers handed over as 2-bit codes (gcsa2_find_batch_packed: `length` characters each, last character
  // first, comp - 1 in two bits, ceil(length / 32) words per pattern): 8 instead of 40 bytes per 32-mer over the link.
  std::vector<range_type> find_packed_batch(const std::vector<std::uint64_t>& codes, size_type length) const
  {
    const size_type words = (length + 31) / 32, nq = (words == 0 ? 0 : codes.size() / words);
    std::vector<range_type> result(nq);
    if(nq > 0) { check(gcsa2_find_batch_packed(handle, codes.data(), length, nq, reinterpret_cast<size_type*>(result.data())), "GCSA::find_packed_batch()"); }
    return result;
  }
  // codes of `count` patterns of `length` bytes each, through THIS index's alphabet: comp - 1 of the fast characters
  // (char2comp values 1..4); any other byte throws.  The packing a caller does.
  std::vector<std::uint64_t> packKMers(const std::uint8_t* patterns, size_type count, size_type length) const
  {
    std::uint8_t code_of[256];
    for(size_type c = 0; c < 256; c++) { const size_type comp = alpha.char2comp[c]; code_of[c] = (comp >= 1 && comp <= 4 ? std::uint8_t(comp - 1) : 0xFF); }
    return pack_with(code_of, patterns, count, length);
  }
  // the same for the default alphabet "$ACGTN#" (A C G T in either case): no index needed
  static std::vector<std::uint64_t> pack_kmers(const std::uint8_t* patterns, size_type count, size_type length)
  {
    std::uint8_t code_of[256];
    for(size_type c = 0; c < 256; c++) { code_of[c] = 0xFF; }
    code_of['A'] = code_of['a'] = 0; code_of['C'] = code_of['c'] = 1; code_of['G'] = code_of['g'] = 2; code_of['T'] = code_of['t'] = 3;
    return pack_with(code_of, patterns, count, length);
  }
  static std::vector<std::uint64_t> pack_with(const std::uint8_t* code_of, const std::uint8_t* patterns, size_type count, size_type length)
  {
    const size_type words = (length + 31) / 32;
    std::vector<std::uint64_t> codes(count * words, 0);
    for(size_type q = 0; q < count; q++)
    {
      for(size_type t = 0; t < length; t++)                  // distance t from the pattern's end
      {
        const std::uint64_t code = code_of[patterns[q * length + (length - 1 - t)]];
        if(code > 3) { throw std::invalid_argument("GCSA::pack_kmers(): a pattern holds a character that is not one of the index's four fast characters"); }
        codes[q * words + (t >> 5)] |= code << (2 * (t & 31));
      }
    }
    return codes;
  }

  // The LF + parent() loop of a MEM finder for a whole batch (gcsa2_match_breaks_batch; the reference's caller shape:
  // src/algorithms.cpp:146-167): the left-maximal matches of every pattern, of at least min_length characters, as
  // {position, length, sp, ep} with (sp, ep) = find() of the match.  Needs an index created together with its LCP array
  // (the two-file constructor / load of base.gcsa + base.lcp).  breaks of pattern q: [offsets_out[q], offsets_out[q + 1]).
  void match_breaks_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type min_length,
                          std::vector<size_type>& offsets_out, std::vector<gcsa2_break>& breaks) const
  {
    match_breaks_batch(patterns, offsets, min_length, 0, offsets_out, breaks);
  }

  // The same with a maximum match length (gcsa2_match_breaks_bounded_batch): a match that has reached max_length characters
  // is cut as if the next character had failed, and the search goes on from parent().  The index answers for patterns up to
  // its order (a longer one "may result in false positives"), so a mapper passes order(); 0 means no cap.
  void match_breaks_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type min_length,
                          size_type max_length, std::vector<size_type>& offsets_out, std::vector<gcsa2_break>& breaks) const
  {
    const size_type nq = offsets.empty() ? 0 : offsets.size() - 1;
    offsets_out.assign(nq + 1, 0);
    if(nq == 0) { breaks.clear(); return; }                    // an empty batch: no records
    breaks.assign(4 * nq + 16, gcsa2_break());
    std::uint8_t dummy = 0;
    size_type total = 0;
    for(int attempt = 0; attempt < 2; attempt++)
    {
      const int rc = gcsa2_match_breaks_bounded_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.data(), nq, min_length, max_length,
                                                      offsets_out.data(), breaks.data(), breaks.size(), &total, nullptr, nullptr);
      if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && total > breaks.size()) { breaks.assign(total, gcsa2_break()); continue; }
      check(rc, "GCSA::match_breaks_batch()");
      break;
    }
    breaks.resize(total);
  }

  // A MEM finder's seeds in one call (gcsa2_mem_hits_batch): the MEMs of match_breaks_batch with count(range), and for each
  // MEM its locate(range) values when hit_max == 0 or count <= hit_max; above the cap none (sample == false) or
  // locate(range, hit_max) (sample == true).  MEMs of pattern q: [mem_offsets[q], mem_offsets[q + 1]); hits of MEM i:
  // [hit_offsets[i], hit_offsets[i + 1]).
  void mem_hits_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type min_length,
                      size_type hit_max, bool sample, std::vector<size_type>& mem_offsets, std::vector<gcsa2_mem>& mems,
                      std::vector<size_type>& hit_offsets, std::vector<node_type>& hits) const
  {
    mem_hits_batch(patterns, offsets, min_length, 0, hit_max, sample, mem_offsets, mems, hit_offsets, hits);
  }

  // The same with a maximum match length (gcsa2_mem_hits_bounded_batch): the MEMs of the bounded match_breaks_batch.  A
  // mapper passes order() -- beyond it the index may report matches the graph does not have; 0 means no cap.
  void mem_hits_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type min_length,
                      size_type max_length, size_type hit_max, bool sample, std::vector<size_type>& mem_offsets, std::vector<gcsa2_mem>& mems,
                      std::vector<size_type>& hit_offsets, std::vector<node_type>& hits) const
  {
    const size_type nq = offsets.empty() ? 0 : offsets.size() - 1;
    mem_offsets.assign(nq + 1, 0);
    mems.assign(4 * nq + 16, gcsa2_mem());
    hits.resize(16 * nq + 64);
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0, total_mems = 0, total_hits = 0;
    for(int attempt = 0; attempt < 2; attempt++)
    {
      hit_offsets.assign(mems.size() + 1, 0);
      const int rc = gcsa2_mem_hits_bounded_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), nq,
                                          min_length, max_length, hit_max, sample ? GCSA2_MEM_OVER_SAMPLE : GCSA2_MEM_OVER_SKIP, mem_offsets.data(), mems.data(),
                                          mems.size(), &total_mems, hit_offsets.data(), hits.data(), hits.size(), &total_hits);
      if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && attempt == 0)
      {
        if(total_mems > mems.size()) { mems.assign(total_mems, gcsa2_mem()); }
        if(total_hits > hits.size()) { hits.resize(total_hits); }
        continue;
      }
      check(rc, "GCSA::mem_hits_batch()");
      break;
    }
    mems.resize(total_mems);
    hit_offsets.resize(total_mems + 1);
    hits.resize(total_hits);
  }

  // A k-mer seeder's lookup in one call (gcsa2_kmer_hits_batch): the windows P_q[j stride, j stride + k) of every read that
  // find() finds, in window order, as records {position = j stride, length = k, sp, ep, count(range)}, with their hits by the
  // rules of mem_hits_batch.  Seeds of read q: [seed_offsets[q], seed_offsets[q + 1]); hits of seed i: [hit_offsets[i],
  // hit_offsets[i + 1]).  (seed_offsets, seeds) is a MEM CSR: sub_mem_hits_batch takes it as it is.
  void kmer_hits_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type stride,
                       size_type hit_max, bool sample, std::vector<size_type>& seed_offsets, std::vector<gcsa2_mem>& seeds,
                       std::vector<size_type>& hit_offsets, std::vector<node_type>& hits) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    seed_offsets.assign(np + 1, 0);
    seeds.clear();
    hits.clear();
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0, total_seeds = 0, total_hits = 0;
    for(int attempt = 0; attempt < 2; attempt++)           // the first call sizes the buffers, unless nothing is found
    {
      hit_offsets.assign(seeds.size() + 1, 0);
      const int rc = gcsa2_kmer_hits_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), np,
                                           k, stride, hit_max, sample ? GCSA2_MEM_OVER_SAMPLE : GCSA2_MEM_OVER_SKIP, nullptr, seed_offsets.data(),
                                           seeds.data(), seeds.size(), &total_seeds, hit_offsets.data(), hits.data(), hits.size(), &total_hits);
      if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && attempt == 0 && (total_seeds > seeds.size() || total_hits > hits.size()))
      {
        seeds.assign(total_seeds, gcsa2_mem());
        hits.assign(total_hits, 0);
        continue;
      }
      check(rc, "GCSA::kmer_hits_batch()");
      break;
    }
    seeds.resize(total_seeds);
    hit_offsets.resize(total_seeds + 1);
    hits.resize(total_hits);
  }

  // The (w, k)-minimizers of every read (gcsa2_minimizers_batch): of every w consecutive valid k-mers the one with the smallest
  // (hash, position), as records {position, hash}; a run of fewer than w valid k-mers gives one.  Minimizers of read q:
  // [min_offsets[q], min_offsets[q + 1]).  1 <= k <= 32, 1 <= w <= 64; forward strand only.
  void minimizers(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type w, size_type hash_seed,
                  std::vector<size_type>& min_offsets, std::vector<gcsa2_minimizer>& minimizers) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    min_offsets.assign(np + 1, 0);
    minimizers.clear();
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0, total = 0;
    for(int attempt = 0; attempt < 2; attempt++)           // the first call sizes the records, unless there are none
    {
      const int rc = gcsa2_minimizers_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), np,
                                            k, w, hash_seed, min_offsets.data(), minimizers.data(), minimizers.size(), &total);
      if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && attempt == 0 && total > minimizers.size())
      {
        minimizers.assign(total, gcsa2_minimizer());
        continue;
      }
      check(rc, "GCSA::minimizers()");
      break;
    }
    minimizers.resize(total);
  }

  // kmer_hits_batch over the minimizers of every read in the place of every stride-th window (gcsa2_minimizer_hits_batch): the
  // seeds of a read are its (w, k)-minimizers that find() finds, in ascending position.
  void minimizer_hits_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type w,
                            size_type hash_seed, size_type hit_max, bool sample, std::vector<size_type>& seed_offsets,
                            std::vector<gcsa2_mem>& seeds, std::vector<size_type>& hit_offsets, std::vector<node_type>& hits) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    seed_offsets.assign(np + 1, 0);
    seeds.clear();
    hits.clear();
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0, total_seeds = 0, total_hits = 0;
    for(int attempt = 0; attempt < 2; attempt++)           // the first call sizes the buffers, unless nothing is found
    {
      hit_offsets.assign(seeds.size() + 1, 0);
      const int rc = gcsa2_minimizer_hits_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), np,
                                                k, w, hash_seed, hit_max, sample ? GCSA2_MEM_OVER_SAMPLE : GCSA2_MEM_OVER_SKIP, nullptr,
                                                seed_offsets.data(), seeds.data(), seeds.size(), &total_seeds, hit_offsets.data(), hits.data(),
                                                hits.size(), &total_hits);
      if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && attempt == 0 && (total_seeds > seeds.size() || total_hits > hits.size()))
      {
        seeds.assign(total_seeds, gcsa2_mem());
        hits.assign(total_hits, 0);
        continue;
      }
      check(rc, "GCSA::minimizer_hits_batch()");
      break;
    }
    seeds.resize(total_seeds);
    hit_offsets.resize(total_seeds + 1);
    hits.resize(total_hits);
  }

  // The canonical (w, k)-minimizers of every read (gcsa2_canonical_minimizers_batch, gcsa2_hip_strands.h): minimizers() with the
  // smaller one of the hashes of a window and of its reverse complement as the window's hash, so that a read and its reverse
  // complement select the same k-mers; records {position, hash, key, strand}.
  void canonical_minimizers(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type w,
                            size_type hash_seed, std::vector<size_type>& min_offsets, std::vector<gcsa2_canonical_minimizer>& minimizers) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    min_offsets.assign(np + 1, 0);
    minimizers.clear();
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0, total = 0;
    for(int attempt = 0; attempt < 2; attempt++)           // the first call sizes the records, unless there are none
    {
      const int rc = gcsa2_canonical_minimizers_batch(handle, patterns.empty() ? &dummy : patterns.data(),
                                                      offsets.empty() ? &dummy_offset : offsets.data(), np, k, w, hash_seed, min_offsets.data(),
                                                      minimizers.data(), minimizers.size(), &total);
      if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && attempt == 0 && total > minimizers.size())
      {
        minimizers.assign(total, gcsa2_canonical_minimizer());
        continue;
      }
      check(rc, "GCSA::canonical_minimizers()");
      break;
    }
    minimizers.resize(total);
  }

  // minimizer_hits_batch over the canonical minimizers, on both strands (gcsa2_stranded_minimizer_hits_batch): two groups of seeds
  // per read, [seed_offsets[2q], seed_offsets[2q + 1]) the minimizers of read q found as written, [seed_offsets[2q + 1],
  // seed_offsets[2q + 2]) the same windows found in its reverse complement, in that read's coordinates.  strands:
  // GCSA2_STRAND_FORWARD, GCSA2_STRAND_REVERSE or GCSA2_STRAND_BOTH; the groups of a strand not asked for are empty.
  void stranded_minimizer_hits_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type w,
                                     size_type hash_seed, int strands, size_type hit_max, bool sample, std::vector<size_type>& seed_offsets,
                                     std::vector<gcsa2_mem>& seeds, std::vector<size_type>& hit_offsets, std::vector<node_type>& hits) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    seed_offsets.assign(2 * np + 1, 0);
    seeds.clear();
    hits.clear();
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0, total_seeds = 0, total_hits = 0;
    for(int attempt = 0; attempt < 2; attempt++)           // the first call sizes the buffers, unless nothing is found
    {
      hit_offsets.assign(seeds.size() + 1, 0);
      const int rc = gcsa2_stranded_minimizer_hits_batch(handle, patterns.empty() ? &dummy : patterns.data(),
                                                         offsets.empty() ? &dummy_offset : offsets.data(), np, k, w, hash_seed, strands, hit_max,
                                                         sample ? GCSA2_MEM_OVER_SAMPLE : GCSA2_MEM_OVER_SKIP, nullptr, seed_offsets.data(),
                                                         seeds.data(), seeds.size(), &total_seeds, hit_offsets.data(), hits.data(), hits.size(),
                                                         &total_hits);
      if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && attempt == 0 && (total_seeds > seeds.size() || total_hits > hits.size()))
      {
        seeds.assign(total_seeds, gcsa2_mem());
        hits.assign(total_hits, 0);
        continue;
      }
      check(rc, "GCSA::stranded_minimizer_hits_batch()");
      break;
    }
    seeds.resize(total_seeds);
    hit_offsets.resize(total_seeds + 1);
    hits.resize(total_hits);
  }

  // Frequency-bounded seeds in one call (gcsa2_capped_seeds_batch): from the end of every read the match is extended until it
  // has min_length characters and count(range) <= max_count, emitted as {position, length, sp, ep, count}, and the search
  // starts again behind it; max_length (0: none, a mapper passes order()) cuts an attempt short.  The seeds of a read do not
  // overlap and come in descending position; their hits follow the rules of mem_hits_batch.  Seeds of read q:
  // [seed_offsets[q], seed_offsets[q + 1]); hits of seed i: [hit_offsets[i], hit_offsets[i + 1]).  (seed_offsets, seeds) is a MEM
  // CSR: sub_mem_hits_batch takes it as it is.  Needs no LCP array.
  void capped_seeds_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type min_length,
                          size_type max_length, size_type max_count, size_type hit_max, bool sample, std::vector<size_type>& seed_offsets,
                          std::vector<gcsa2_mem>& seeds, std::vector<size_type>& hit_offsets, std::vector<node_type>& hits) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    seed_offsets.assign(np + 1, 0);
    seeds.clear();
    hits.clear();
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0, total_seeds = 0, total_hits = 0;
    for(int attempt = 0; attempt < 2; attempt++)           // the first call sizes the buffers, unless nothing is found
    {
      hit_offsets.assign(seeds.size() + 1, 0);
      const int rc = gcsa2_capped_seeds_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), np,
                                              min_length, max_length, max_count, hit_max, sample ? GCSA2_MEM_OVER_SAMPLE : GCSA2_MEM_OVER_SKIP,
                                              seed_offsets.data(), seeds.data(), seeds.size(), &total_seeds, hit_offsets.data(), hits.data(),
                                              hits.size(), &total_hits);
      if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && attempt == 0 && (total_seeds > seeds.size() || total_hits > hits.size()))
      {
        seeds.assign(total_seeds, gcsa2_mem());
        hits.assign(total_hits, 0);
        continue;
      }
      check(rc, "GCSA::capped_seeds_batch()");
      break;
    }
    seeds.resize(total_seeds);
    hit_offsets.resize(total_seeds + 1);
    hits.resize(total_hits);
  }

  // A genotyper's or a coverage screen's lookup in one call (gcsa2_kmer_support_batch): every window P_q[j stride, j stride + k)
  // with a non-empty find() and hit_max == 0 or count(range) <= hit_max adds 1 to support[v >> shift] for every located value v
  // of its range (per_bin: once per distinct bin).  shift = 11 (Node::ID_OFFSET) gives node ids.  ADDS into `support`, whose
  // size is the number of bins: contributions beyond it are counted in stats->dropped.  Needs no LCP array.
  void kmer_support_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type stride,
                          size_type hit_max, size_type shift, bool per_bin, std::vector<size_type>& support,
                          gcsa2_support_stats* stats = nullptr) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0;
    const int rc = gcsa2_kmer_support_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), np,
                                            k, stride, hit_max, shift, per_bin ? GCSA2_SUPPORT_PER_BIN : 0,
                                            support.empty() ? nullptr : support.data(), support.size(), stats);
    check(rc, "GCSA::kmer_support_batch()");
  }

  // The denominator of kmer_support_batch (gcsa2_index_kmer_support_device): every k-mer of the INDEX with hit_max == 0 or
  // count(range) <= hit_max adds 1 to d_support[v >> shift] for every located value v of its range (per_bin: once per distinct
  // bin).  d_support is DEVICE memory of n_bins words that is added into (nullptr with n_bins == 0: the statistics alone).
  void index_kmer_support_device(size_type k, bool include_Ns, bool force, size_type hit_max, size_type shift, bool per_bin,
                                 size_type* d_support, size_type n_bins, gcsa2_support_stats* stats = nullptr, void* stream = nullptr) const
  {
    const int rc = gcsa2_index_kmer_support_device(handle, k, include_Ns ? 1 : 0, force ? 1 : 0, hit_max, shift, per_bin ? GCSA2_SUPPORT_PER_BIN : 0,
                                                   d_support, n_bins, stats, stream);
    check(rc, "GCSA::index_kmer_support_device()");
  }

  // A read classifier's or binner's lookup in one call (gcsa2_kmer_classes_batch): every window P_q[j stride, j stride + k) with
  // a non-empty find() and hit_max == 0 or count(range) <= hit_max votes, in the row of its read, for the class
  // class_of_bin[v >> shift] of every located value v of its range (GCSA2_CLASS_NONE, an id >= n_classes or a bin beyond the
  // map: no class).  flags: GCSA2_CLASS_PER_WINDOW, GCSA2_CLASS_UNAMBIGUOUS.  votes (reads x n_classes, row-major) and calls
  // (one per read) are resized and WRITTEN.  Needs no LCP array.
  void kmer_classes_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type stride,
                          size_type hit_max, size_type shift, int flags, const std::vector<std::uint32_t>& class_of_bin, size_type n_classes,
                          std::vector<size_type>& votes, std::vector<gcsa2_class_call>& calls, gcsa2_class_stats* stats = nullptr) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0;
    votes.assign(np * n_classes, 0);
    calls.assign(np, gcsa2_class_call{GCSA2_UNKNOWN, 0, GCSA2_UNKNOWN, 0, 0, 0});
    const int rc = gcsa2_kmer_classes_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), np,
                                            k, stride, hit_max, shift, flags, class_of_bin.empty() ? nullptr : class_of_bin.data(),
                                            class_of_bin.size(), n_classes, votes.empty() ? nullptr : votes.data(),
                                            calls.empty() ? nullptr : calls.data(), stats);
    check(rc, "GCSA::kmer_classes_batch()");
  }

  // The sparse form for any number of classes (gcsa2_kmer_top_classes_batch): the same votes, n_classes up to 0xFFFFFFFF, and
  // per read the top_n (1 .. GCSA2_TOP_LIMIT) classes with the most votes -- more votes first, the lower id on a tie,
  // {GCSA2_UNKNOWN, 0} behind the voted classes -- and {voted, total, counted}.  top (reads x top_n, row-major) and summaries
  // (one per read) are resized and WRITTEN.  Needs no LCP array.
  void kmer_top_classes_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type stride,
                              size_type hit_max, size_type shift, int flags, const std::vector<std::uint32_t>& class_of_bin, size_type n_classes,
                              size_type top_n, std::vector<gcsa2_class_vote>& top, std::vector<gcsa2_top_summary>& summaries,
                              gcsa2_class_stats* stats = nullptr) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0;
    top.assign(np * (top_n <= GCSA2_TOP_LIMIT ? top_n : 0), gcsa2_class_vote{GCSA2_UNKNOWN, 0});
    summaries.assign(np, gcsa2_top_summary{0, 0, 0});
    const int rc = gcsa2_kmer_top_classes_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), np,
                                                k, stride, hit_max, shift, flags, class_of_bin.empty() ? nullptr : class_of_bin.data(),
                                                class_of_bin.size(), n_classes, top_n, top.empty() ? nullptr : top.data(),
                                                summaries.empty() ? nullptr : summaries.data(), stats);
    check(rc, "GCSA::kmer_top_classes_batch()");
  }

  // Seed clusters (gcsa2_kmer_clusters_batch): per read the top_n (1 .. GCSA2_CLUSTER_TOP_LIMIT) diagonal bands of the hits of
  // its k-mers -- larger covered first, then more anchors, then the smaller diag_min; all zero behind the last cluster -- and
  // {anchors, unplaced, clusters}.  coord_of_bin[value >> shift] is the coordinate of a hit (GCSA2_UNKNOWN: none); anchors whose
  // diagonals differ by at most `band` join.  top (reads x top_n, row-major) and summaries (one per read) are resized and
  // WRITTEN.  Needs no LCP array.
  void kmer_clusters_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type stride,
                           size_type hit_max, bool sample, size_type shift, const std::vector<size_type>& coord_of_bin, size_type band,
                           size_type top_n, std::vector<gcsa2_cluster>& top, std::vector<gcsa2_cluster_summary>& summaries,
                           gcsa2_cluster_stats* stats = nullptr) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0;
    top.assign(np * (top_n <= GCSA2_CLUSTER_TOP_LIMIT ? top_n : 0), gcsa2_cluster{0, 0, 0, 0, 0, 0, 0, 0});
    summaries.assign(np, gcsa2_cluster_summary{0, 0, 0});
    const int rc = gcsa2_kmer_clusters_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), np,
                                             k, stride, hit_max, sample ? GCSA2_MEM_OVER_SAMPLE : GCSA2_MEM_OVER_SKIP, shift,
                                             coord_of_bin.empty() ? nullptr : coord_of_bin.data(), coord_of_bin.size(), band, top_n,
                                             top.empty() ? nullptr : top.data(), summaries.empty() ? nullptr : summaries.data(), stats);
    check(rc, "GCSA::kmer_clusters_batch()");
  }

  // The same over the (w, k)-minimizers of every read (gcsa2_minimizer_clusters_batch).
  void minimizer_clusters_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type w,
                                size_type hash_seed, size_type hit_max, bool sample, size_type shift, const std::vector<size_type>& coord_of_bin,
                                size_type band, size_type top_n, std::vector<gcsa2_cluster>& top, std::vector<gcsa2_cluster_summary>& summaries,
                                gcsa2_cluster_stats* stats = nullptr) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0;
    top.assign(np * (top_n <= GCSA2_CLUSTER_TOP_LIMIT ? top_n : 0), gcsa2_cluster{0, 0, 0, 0, 0, 0, 0, 0});
    summaries.assign(np, gcsa2_cluster_summary{0, 0, 0});
    const int rc = gcsa2_minimizer_clusters_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), np,
                                                  k, w, hash_seed, hit_max, sample ? GCSA2_MEM_OVER_SAMPLE : GCSA2_MEM_OVER_SKIP, shift,
                                                  coord_of_bin.empty() ? nullptr : coord_of_bin.data(), coord_of_bin.size(), band, top_n,
                                                  top.empty() ? nullptr : top.data(), summaries.empty() ? nullptr : summaries.data(), stats);
    check(rc, "GCSA::minimizer_clusters_batch()");
  }

  // The clusters of a seed CSR that is already in device memory with its hit offsets and hits, as any hits call of the C
  // interface leaves them (gcsa2_seed_clusters_device): raw device pointers, d_top and d_summaries may be null.
  void seed_clusters_device(const size_type* d_group_offsets, size_type n_groups, const gcsa2_mem* d_seeds, size_type n_seeds,
                            const size_type* d_hit_offsets, const node_type* d_hits, size_type n_hits, size_type shift,
                            const size_type* d_coord_of_bin, size_type n_bins, size_type band, size_type top_n, gcsa2_cluster* d_top,
                            gcsa2_cluster_summary* d_summaries, gcsa2_cluster_stats* stats = nullptr, void* stream = nullptr) const
  {
    const int rc = gcsa2_seed_clusters_device(handle, d_group_offsets, n_groups, d_seeds, n_seeds, d_hit_offsets, d_hits, n_hits, shift, d_coord_of_bin,
                                              n_bins, band, top_n, d_top, d_summaries, stats, stream);
    check(rc, "GCSA::seed_clusters_device()");
  }

  // Seed chains (gcsa2_kmer_chains_batch): per read the top_n (1 .. GCSA2_CHAIN_TOP_LIMIT) colinear chains of the hits of its
  // k-mers -- larger score first, then more anchors, then the smaller place of the end; all zero behind the last chain --, of
  // every chain its first member_cap anchors from its end backwards, and {anchors, unplaced, chains}.  coord_of_bin as for the
  // clusters.  top (reads x top_n), members (reads x top_n x member_cap; empty with member_cap == 0) and summaries (one per
  // read) are resized and WRITTEN.  Needs no LCP array.
  void kmer_chains_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type stride,
                         size_type hit_max, bool sample, size_type shift, const std::vector<size_type>& coord_of_bin, const ChainParameters& parameters,
                         std::vector<gcsa2_chain>& top, std::vector<gcsa2_chain_anchor>& members, std::vector<gcsa2_chain_summary>& summaries,
                         gcsa2_chain_stats* stats = nullptr) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0;
    const gcsa2_chain_params params = parameters.c();
    this->chain_outputs(np, params, top, members, summaries);
    const int rc = gcsa2_kmer_chains_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), np,
                                           k, stride, hit_max, sample ? GCSA2_MEM_OVER_SAMPLE : GCSA2_MEM_OVER_SKIP, shift,
                                           coord_of_bin.empty() ? nullptr : coord_of_bin.data(), coord_of_bin.size(), &params,
                                           top.empty() ? nullptr : top.data(), members.empty() ? nullptr : members.data(),
                                           summaries.empty() ? nullptr : summaries.data(), stats);
    check(rc, "GCSA::kmer_chains_batch()");
  }

  // The same over the (w, k)-minimizers of every read (gcsa2_minimizer_chains_batch).
  void minimizer_chains_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type w,
                              size_type hash_seed, size_type hit_max, bool sample, size_type shift, const std::vector<size_type>& coord_of_bin,
                              const ChainParameters& parameters, std::vector<gcsa2_chain>& top, std::vector<gcsa2_chain_anchor>& members,
                              std::vector<gcsa2_chain_summary>& summaries, gcsa2_chain_stats* stats = nullptr) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0;
    const gcsa2_chain_params params = parameters.c();
    this->chain_outputs(np, params, top, members, summaries);
    const int rc = gcsa2_minimizer_chains_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), np,
                                                k, w, hash_seed, hit_max, sample ? GCSA2_MEM_OVER_SAMPLE : GCSA2_MEM_OVER_SKIP, shift,
                                                coord_of_bin.empty() ? nullptr : coord_of_bin.data(), coord_of_bin.size(), &params,
                                                top.empty() ? nullptr : top.data(), members.empty() ? nullptr : members.data(),
                                                summaries.empty() ? nullptr : summaries.data(), stats);
    check(rc, "GCSA::minimizer_chains_batch()");
  }

  // The chains of a seed CSR that is already in device memory with its hit offsets and hits (gcsa2_seed_chains_device): raw
  // device pointers; d_top, d_members and d_summaries may be null.
  void seed_chains_device(const size_type* d_group_offsets, size_type n_groups, const gcsa2_mem* d_seeds, size_type n_seeds,
                          const size_type* d_hit_offsets, const node_type* d_hits, size_type n_hits, size_type shift,
                          const size_type* d_coord_of_bin, size_type n_bins, const ChainParameters& parameters, gcsa2_chain* d_top,
                          gcsa2_chain_anchor* d_members, gcsa2_chain_summary* d_summaries, gcsa2_chain_stats* stats = nullptr,
                          void* stream = nullptr) const
  {
    const gcsa2_chain_params params = parameters.c();
    const int rc = gcsa2_seed_chains_device(handle, d_group_offsets, n_groups, d_seeds, n_seeds, d_hit_offsets, d_hits, n_hits, shift, d_coord_of_bin,
                                            n_bins, &params, d_top, d_members, d_summaries, stats, stream);
    check(rc, "GCSA::seed_chains_device()");
  }

  // Chain pairs (gcsa2_minimizer_chain_pairs_batch): the reads are interleaved mates, pair p the reads 2p and 2p + 1 (an odd
  // number of reads is refused).  Both strands of every read are seeded at its canonical (w, k)-minimizers and chained -- chains
  // (2 reads x chain top_n; group 2q + s is strand s of read q), members and chain_summaries (one per group) as for
  // minimizer_chains_batch --, and per pair the top_n (1 .. GCSA2_PAIR_TOP_LIMIT) placements of a chain of one mate and a chain of
  // the other under the fragment model of pair_parameters -- larger score first, then the smaller deviation from the mean
  // fragment; all zero behind the last placement -- go to top (pairs x top_n), {candidates, proper, kept, ignored, the best chain
  // of each mate} to summaries (one per pair).  All five are resized and WRITTEN.  Needs no LCP array.
  void minimizer_chain_pairs_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets, size_type k, size_type w,
                                   size_type hash_seed, size_type hit_max, bool sample, size_type shift, const std::vector<size_type>& coord_of_bin,
                                   const ChainParameters& chain_parameters, const PairParameters& pair_parameters, std::vector<gcsa2_chain>& chains,
                                   std::vector<gcsa2_chain_anchor>& members, std::vector<gcsa2_chain_summary>& chain_summaries,
                                   std::vector<gcsa2_chain_pair>& top, std::vector<gcsa2_pair_summary>& summaries,
                                   gcsa2_chain_stats* chain_stats = nullptr, gcsa2_pair_stats* pair_stats = nullptr) const
  {
    const size_type np = offsets.empty() ? 0 : offsets.size() - 1;
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0;
    const gcsa2_chain_params params = chain_parameters.c();
    const gcsa2_pair_params pair_params = pair_parameters.c();
    this->chain_outputs(2 * np, params, chains, members, chain_summaries);
    top.assign((np / 2) * (pair_params.top_n <= GCSA2_PAIR_TOP_LIMIT ? pair_params.top_n : 0), gcsa2_chain_pair{0, 0, 0, 0, 0, 0, 0, 0});
    summaries.assign(np / 2, gcsa2_pair_summary{0, 0, 0, 0, 0, 0, 0, 0});
    const int rc = gcsa2_minimizer_chain_pairs_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), np,
                                                     k, w, hash_seed, hit_max, sample ? GCSA2_MEM_OVER_SAMPLE : GCSA2_MEM_OVER_SKIP, shift,
                                                     coord_of_bin.empty() ? nullptr : coord_of_bin.data(), coord_of_bin.size(), &params, &pair_params,
                                                     chains.empty() ? nullptr : chains.data(), members.empty() ? nullptr : members.data(),
                                                     chain_summaries.empty() ? nullptr : chain_summaries.data(), top.empty() ? nullptr : top.data(),
                                                     summaries.empty() ? nullptr : summaries.data(), chain_stats, pair_stats);
    check(rc, "GCSA::minimizer_chain_pairs_batch()");
  }

  // The placements of chain rows that are already in device memory (gcsa2_chain_pairs_device): d_chains holds the four rows of
  // every pair, 4 n_pairs x chain_top_n, in the group order of the stranded hits of interleaved mates; raw device pointers;
  // d_top and d_summaries may be null.
  void chain_pairs_device(const gcsa2_chain* d_chains, size_type n_pairs, size_type chain_top_n, const PairParameters& parameters, gcsa2_chain_pair* d_top,
                          gcsa2_pair_summary* d_summaries, gcsa2_pair_stats* stats = nullptr, void* stream = nullptr) const
  {
    const gcsa2_pair_params params = parameters.c();
    const int rc = gcsa2_chain_pairs_device(handle, d_chains, n_pairs, chain_top_n, &params, d_top, d_summaries, stats, stream);
    check(rc, "GCSA::chain_pairs_device()");
  }

  // Sub-MEM reseeding (gcsa2_sub_mem_hits_batch): inside every MEM of mem_hits_batch (mem_offsets, mems) of at least
  // reseed_length bases, the matches of at least min_length that occur more often than the MEM, with their hits by the rules of
  // mem_hits_batch.  Sub-MEMs of MEM k: [sub_offsets[k], sub_offsets[k + 1]); hits of sub-MEM i: [hit_offsets[i], hit_offsets[i + 1]).
  void sub_mem_hits_batch(const std::vector<std::uint8_t>& patterns, const std::vector<size_type>& offsets,
                          const std::vector<size_type>& mem_offsets, const std::vector<gcsa2_mem>& mems, size_type min_length,
                          size_type reseed_length, size_type hit_max, bool sample, std::vector<size_type>& sub_offsets,
                          std::vector<gcsa2_mem>& subs, std::vector<size_type>& hit_offsets, std::vector<node_type>& hits) const
  {
    const size_type nq = offsets.empty() ? 0 : offsets.size() - 1;
    sub_offsets.assign(mems.size() + 1, 0);
    subs.assign(4 * mems.size() + 16, gcsa2_mem());
    hits.resize(16 * mems.size() + 64);
    std::uint8_t dummy = 0;
    size_type dummy_offset = 0, total_subs = 0, total_hits = 0;
    gcsa2_mem dummy_mem = gcsa2_mem();
    for(int attempt = 0; attempt < 2; attempt++)
    {
      hit_offsets.assign(subs.size() + 1, 0);
      const int rc = gcsa2_sub_mem_hits_batch(handle, patterns.empty() ? &dummy : patterns.data(), offsets.empty() ? &dummy_offset : offsets.data(), nq,
                                              mem_offsets.empty() ? &dummy_offset : mem_offsets.data(), mems.empty() ? &dummy_mem : mems.data(),
                                              mems.size(), min_length, reseed_length, hit_max, sample ? GCSA2_MEM_OVER_SAMPLE : GCSA2_MEM_OVER_SKIP,
                                              sub_offsets.data(), subs.data(), subs.size(), &total_subs, hit_offsets.data(), hits.data(), hits.size(),
                                              &total_hits);
      if(rc == GCSA2_ERR_BUFFER_TOO_SMALL && attempt == 0)
      {
        if(total_subs > subs.size()) { subs.assign(total_subs, gcsa2_mem()); }
        if(total_hits > hits.size()) { hits.resize(total_hits); }
        continue;
      }
      check(rc, "GCSA::sub_mem_hits_batch()");
      break;
    }
    subs.resize(total_subs);
    hit_offsets.resize(total_subs + 1);
    hits.resize(total_hits);
  }

  // Memory pressure (gcsa2_index_set_tables / gcsa2_index_trim): drop (0), build (1) or leave (-1) the pair blocks and the
  // locate table, resize the seed table (kmer_k: -1 leaves it, 0 drops it); give back staging and scratch memory.  Results
  // never change.  Not to be called while queries run on this index or on copies of it (copies share the device image).
  void setTables(int pair_blocks, int kmer_k, int locate_table) { check(gcsa2_index_set_tables(owner.get(), pair_blocks, kmer_k, locate_table), "GCSA::setTables()"); }
  void trim() { check(gcsa2_index_trim(owner.get()), "GCSA::trim()"); }
  // Shape of the host pipeline behind find_batch / find_packed_batch (gcsa2_index_set_pipeline): host threads, log2 of the
  // patterns per chunk, spinning (0) or sleeping (1) waits; 0 / 0 / -1 leave a value as it is.
  void setPipeline(int lanes, int chunk_log2, int blocking = -1) { check(gcsa2_index_set_pipeline(owner.get(), lanes, chunk_log2, blocking), "GCSA::setPipeline()"); }
  size_type deviceBytes() const { return gcsa2_device_bytes(handle); }

  size_type count(range_type range) const                                   // src/gcsa.cpp:802-809
  {
    size_type in[2] = { range.first, range.second }, out = 0;
    if(handle == nullptr) { return 0; }
    check(gcsa2_count_batch(handle, in, 1, &out), "GCSA::count()");
    return out;
  }

  std::vector<size_type> count_batch(const std::vector<range_type>& ranges) const
  {
    std::vector<size_type> out(ranges.size());
    size_type dummy_in[2] = { 1, 0 }, dummy_out = 0;
    check(gcsa2_count_batch(handle, ranges.empty() ? dummy_in : reinterpret_cast<const size_type*>(ranges.data()), ranges.size(),
                            ranges.empty() ? &dummy_out : out.data()), "GCSA::count_batch()");
    return out;
  }

  void locate(size_type path, std::vector<node_type>& results, bool append = false, bool sort = true) const  // gcsa.cpp:813-825
  {
    locate(range_type(path, path), results, append, sort);
  }

  // gcsa.cpp:827-842: sort == false keeps path order and duplicates, as the reference does.
  void locate(range_type range, std::vector<node_type>& results, bool append = false, bool sort = true) const
  {
    if(!append) { results.clear(); }
    if(handle == nullptr) { return; }
    size_type in[2] = { range.first, range.second }, offsets[2] = { 0, 0 };
    gcsa2_locate_job* job = nullptr;
    check(gcsa2_locate_run(handle, in, 1, sort ? 1 : 0, offsets, &job), "GCSA::locate()");
    size_type old = results.size();
    results.resize(old + offsets[1]);
    node_type dummy = 0;
    check(gcsa2_locate_fetch(job, offsets[1] ? results.data() + old : &dummy, offsets[1] ? offsets[1] : 1), "GCSA::locate()");
    if(append && sort && old > 0) { sort_unique(results); }
  }

  void locate(range_type range, size_type max_positions, std::vector<node_type>& results) const   // gcsa.cpp:844-878
  {
    results.clear();
    size_type total = count(range);
    if(total == 0) { return; }
    results.resize(max_positions < total ? max_positions : total);
    size_type got = 0;
    check(gcsa2_locate_max(handle, range.first, range.second, max_positions, results.data(), results.size(), &got), "GCSA::locate()");
    results.resize(got);
  }

  // CSR batch: offsets[q] .. offsets[q + 1] index the sorted distinct values of ranges[q].
  void locate_batch(const std::vector<range_type>& ranges, std::vector<size_type>& offsets, std::vector<node_type>& values) const
  {
    offsets.assign(ranges.size() + 1, 0);
    gcsa2_locate_job* job = nullptr;
    check(gcsa2_locate_run(handle, reinterpret_cast<const size_type*>(ranges.data()), ranges.size(), 1, offsets.data(), &job), "GCSA::locate_batch()");
    values.resize(offsets.back() ? offsets.back() : 1);
    check(gcsa2_locate_fetch(job, values.data(), values.size()), "GCSA::locate_batch()");
    values.resize(offsets.back());
  }

  // CSR batch of locate(range, max_positions, results): offsets[q] .. offsets[q + 1] index the values of ranges[q], as the
  // per-range call returns them; offsets[q + 1] - offsets[q] == min(max_positions, count(ranges[q])).
  void locate_batch(const std::vector<range_type>& ranges, size_type max_positions, std::vector<size_type>& offsets,
                    std::vector<node_type>& values) const
  {
    offsets.assign(ranges.size() + 1, 0);
    std::vector<size_type> counts(ranges.size());
    if(!ranges.empty())
    {
      check(gcsa2_count_batch(handle, reinterpret_cast<const size_type*>(ranges.data()), ranges.size(), counts.data()), "GCSA::locate_batch()");
    }
    // room for min(max_positions, count) per range; a count() that wrapped below zero says nothing of the range's size,
    // so the call is repeated with the size it asks for when this is not enough
    size_type capacity = 0;
    for(size_type c : counts) { if(c < (size_type(1) << 40)) { capacity += (max_positions < c ? max_positions : c); } }
    size_type total = 0;
    int rc = GCSA2_OK;
    for(int attempt = 0; attempt < 2; attempt++)
    {
      values.resize(capacity ? capacity : 1);
      rc = gcsa2_locate_max_batch(handle, reinterpret_cast<const size_type*>(ranges.data()), ranges.size(), max_positions,
                                  offsets.data(), values.data(), capacity, &total);
      if(rc != GCSA2_ERR_BUFFER_TOO_SMALL || total <= capacity) { break; }
      capacity = total;
    }
    check(rc, "GCSA::locate_batch()");
    values.resize(total);
  }

  // ---- low-level interface (gcsa.h:137-210) ----
  size_type size() const { return header.path_nodes; }                      // gcsa.h:137-148
  bool empty() const { return size() == 0; }
  size_type edgeCount() const { return header.edges; }
  size_type order() const { return header.order; }
  size_type sampleCount() const { return handle != nullptr ? gcsa2_sample_count(handle) : 0; }
  size_type sampleBits() const { return handle != nullptr ? gcsa2_sample_bits(handle) : 0; }
  size_type sampledPositions() const { return handle != nullptr ? gcsa2_sampled_positions(handle) : 0; }

  range_type charRange(comp_type comp) const                                // gcsa.h:150-153
  {
    range_type r;
    check(gcsa2_char_range(handle, comp, &r.first, &r.second), "GCSA::charRange()");
    return r;
  }

  range_type LF(range_type range, comp_type comp) const                     // gcsa.h:155-162
  {
    size_type in[2] = { range.first, range.second }, out[2];
    check(gcsa2_lf_batch(handle, in, &comp, 1, out), "GCSA::LF()");
    return range_type(out[0], out[1]);
  }

  std::vector<range_type> LF_batch(const std::vector<range_type>& ranges, const std::vector<comp_type>& comps) const
  {
    std::vector<range_type> out(ranges.size());
    check(gcsa2_lf_batch(handle, reinterpret_cast<const size_type*>(ranges.data()), comps.data(), ranges.size(),
                         reinterpret_cast<size_type*>(out.data())), "GCSA::LF_batch()");
    return out;
  }

  size_type LF(size_type path_node) const                                   // gcsa.h:165-183
  {
    size_type out = 0;
    check(gcsa2_lf_node_batch(handle, &path_node, 1, &out), "GCSA::LF()");
    return out;
  }

  // results must hold sigma entries, as in the reference (gcsa.cpp:742-798)
  void LF_fast(range_type range, std::vector<range_type>& results) const { lf_all(range, results, 0); }
  void LF_all(range_type range, std::vector<range_type>& results) const { lf_all(range, results, 1); }

  bool sampled(size_type path_node) const { return sample_info(path_node)[0] != 0; }              // gcsa.h:191
  range_type sampleRange(size_type path_node) const                                                // gcsa.h:193-200
  { std::vector<size_type> s = sample_info(path_node); return range_type(s[1], s[2]); }
  size_type firstSample(size_type path_node) const { return sample_info(path_node)[1]; }           // gcsa.h:202-206
  bool lastSample(size_type i) const { size_type v; std::uint8_t l; check(gcsa2_sample_batch(handle, &i, 1, &v, &l), "GCSA::lastSample()"); return l != 0; }  // gcsa.h:208
  node_type sample(size_type i) const { size_type v; std::uint8_t l; check(gcsa2_sample_batch(handle, &i, 1, &v, &l), "GCSA::sample()"); return v; }          // gcsa.h:210

  GCSAHeader header;         // gcsa.h:214
  Alphabet   alpha;          // gcsa.h:215: alpha.char2comp / comp2char / C / sigma / fast_chars
  gcsa2_index* handle;       // the device image, for the C ABI (nullptr: empty index)

private:
  static void sort_unique(std::vector<node_type>& v) { removeDuplicates(v); }     // utils.h:350-357, for append == true
  void lf_all(range_type range, std::vector<range_type>& results, int all) const
  {
    std::vector<size_type> out(2 * alpha.sigma);
    size_type in[2] = { range.first, range.second };
    check(gcsa2_lf_all_batch(handle, in, 1, all, out.data()), "GCSA::LF_all()");
    size_type limit = all ? alpha.sigma - 2 : alpha.fast_chars;
    for(size_type c = 1; c <= limit && c < results.size(); c++) { results[c] = range_type(out[2 * c], out[2 * c + 1]); }
  }
  // the outputs of a chains call for np reads, zeroed; nothing for parameters that the call will refuse
  static void chain_outputs(size_type np, const gcsa2_chain_params& p, std::vector<gcsa2_chain>& top, std::vector<gcsa2_chain_anchor>& members,
                            std::vector<gcsa2_chain_summary>& summaries)
  {
    const size_type rows = np * (p.top_n <= GCSA2_CHAIN_TOP_LIMIT ? p.top_n : 0);
    const bool fits = (p.member_cap == 0 || rows == 0 || p.member_cap <= 0xFFFFFFFFull / rows);
    top.assign(rows, gcsa2_chain{0, 0, 0, 0, 0, 0, 0, 0});
    members.assign(fits ? rows * p.member_cap : 0, gcsa2_chain_anchor{0, 0, 0});
    summaries.assign(np, gcsa2_chain_summary{0, 0, 0});
  }
  std::vector<size_type> sample_info(size_type node) const
  {
    std::vector<size_type> out(3);
    check(gcsa2_sample_range_batch(handle, &node, 1, out.data()), "GCSA::sampleRange()");
    return out;
  }

  void own(gcsa2_index* raw)
  {
    owner.reset(raw, gcsa2_index_destroy);
    handle = raw;
    header = GCSAHeader();
    header.path_nodes = gcsa2_size(raw); header.edges = gcsa2_edge_count(raw); header.order = gcsa2_order(raw);
    alpha.read(raw);
  }
  void adopt(const gcsa2_host_view& view, int device, std::shared_ptr<gcsa2_view_storage> storage)
  {
    gcsa2_index* raw = nullptr;
    check(gcsa2_index_create(&view, device, &raw), "GCSA::GCSA()");
    this->own(raw);
    host = (retainHostView() ? storage : nullptr);
  }
  void take(GCSA& source)
  {
    header = source.header; alpha = std::move(source.alpha); handle = source.handle;
    owner = std::move(source.owner); host = std::move(source.host);
    source.handle = nullptr; source.header = GCSAHeader(); source.alpha = Alphabet();
  }
  static void write_to(void* stream, const void* data, std::uint64_t bytes)
  {
    static_cast<std::ostream*>(stream)->write(static_cast<const char*>(data), std::streamsize(bytes));
  }

  std::shared_ptr<gcsa2_index> owner;
  std::shared_ptr<gcsa2_view_storage> host;
};

} // namespace gcsa

#endif // GCSA2_HIP_GCSA_GCSA_H
