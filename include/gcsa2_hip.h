/*
 * gcsa2_hip.h -- C ABI of the MI355X batched backward-search engine for GCSA2 indexes.
 *
 * This is the drop-in boundary for the query hot path of jltsiren/gcsa2: every entry point
 * below replaces a method of `gcsa::GCSA` / `gcsa::LCPArray` that the reference implements as
 * header-inline C++ over SDSL bitvectors (citations are relative to the reference tree).
 * The reference has no FFI of its own -- its boundary is a C++ class API -- so this header is
 * what a C++ facade (include/gcsa2_hip/gcsa.hpp), a cgo/JNI stub or the ctypes binding in
 * gcsa2_amd/binding.py binds.  Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *   - All index data are described by plain LSB-first bit arrays (bit i of a vector lives in
 *     word i >> 6 at position i & 63, as in SDSL) and plain integer arrays.  The engine builds
 *     its own device image from them; nothing is kept by reference after create() returns.
 *   - Every bit array must be readable for ceil(bits / 64) whole words.
 *   - Ranges are closed [sp, ep] pairs of uint64 as in `gcsa::range_type`
 *     (include/gcsa/utils.h:84); a range is empty iff sp + 1 > ep + 1 (utils.h:93-96).
 *   - `*_batch` entry points take HOST pointers, copy in, run the kernels, copy out and
 *     synchronise.  `*_device` entry points take DEVICE pointers on the handle's device, only
 *     enqueue work on `stream` (a hipStream_t passed as void*, NULL = default stream) and do
 *     not synchronise -- they are what the benchmark and the multi-GPU driver use.
 *   - Device buffers of the `*_device` entry points: d_patterns is read in aligned 8-byte words, so the
 *     allocation must extend to the 8-byte boundary at or after its last pattern byte and start at or before the
 *     8-byte boundary at or before its first one (any hipMalloc'd buffer of `total bytes + 8` starting with the
 *     first pattern satisfies both); d_offsets, d_ranges and every other u64 array must be 8-byte aligned, range
 *     pairs 16-byte aligned; d_ms of gcsa2_match_stats_device must be 8-byte aligned and hold 4 spare entries.
 *     The host-pointer entry points have no such requirements (they stage into padded buffers).
 *   - Return value: GCSA2_OK (0) or a negative gcsa2_status.  Query entry points do not
 *     validate ranges or comps, exactly like the reference's low-level interface
 *     (include/gcsa/gcsa.h:133-135); count/locate apply the reference's `ep >= size()` guard.
 *   - A handle is immutable after creation and may be used from several host threads.
 */
#ifndef GCSA2_HIP_H
#define GCSA2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gcsa2_status {
  GCSA2_OK = 0,
  GCSA2_ERR_INVALID_ARGUMENT = -1,
  GCSA2_ERR_NO_DEVICE = -2,     /* no HIP device / runtime failure at init */
  GCSA2_ERR_OUT_OF_MEMORY = -3,
  GCSA2_ERR_HIP = -4,           /* any other HIP runtime error; see gcsa2_last_error() */
  GCSA2_ERR_MISSING_COMPONENT = -5, /* e.g. count() without counters, parent() without LCP */
  GCSA2_ERR_BUFFER_TOO_SMALL = -6
} gcsa2_status;

/*
 * Host-side description of one index = the data members of gcsa::GCSA
 * (include/gcsa/gcsa.h:214-240) and gcsa::LCPArray (include/gcsa/lcp.h:188-190) as plain arrays.
 */
typedef struct gcsa2_host_view {
  /* GCSAHeader (include/gcsa/files.h:135-156) */
  uint64_t path_nodes;            /* header.path_nodes = size() */
  uint64_t edges;                 /* header.edges */
  uint64_t order;                 /* header.order */

  /* Alphabet (include/gcsa/support.h:93-155) */
  uint64_t sigma;                 /* alpha.sigma, 1..GCSA2_MAX_SIGMA */
  uint64_t fast_chars;            /* alpha.fast_chars (informational: every comp is stored densely) */
  const uint8_t*  char2comp;      /* alpha.char2comp, 256 entries */
  const uint64_t* C;              /* alpha.C, sigma + 1 entries */

  /* fast_bwt[1..fast_chars] / sparse_bwt[0, fast_chars+1..] as plain bits: bwt[c], path_nodes bits */
  const uint64_t* const* bwt;     /* sigma pointers */
  const uint64_t* edge_bits;      /* edges, `edges` bits */
  const uint64_t* sampled_path_bits; /* sampled_paths, path_nodes bits; NULL = no locate support */

  /* stored_samples (sdsl::int_vector<0>) and samples (bit_vector) */
  uint64_t sample_count;          /* stored_samples.size() */
  uint64_t sample_width;          /* stored_samples.width(), 1..64 */
  const uint64_t* stored_samples; /* packed: element i = bits [i*w, (i+1)*w) */
  const uint64_t* sample_bits;    /* samples, sample_count bits */

  /* extra_pointers (SadaSparse, include/gcsa/support.h:298-364); NULL filter = no count support */
  const uint64_t* extra_filter_bits; /* filter, path_nodes bits */
  uint64_t extra_values_len;         /* values.size() */
  const uint64_t* extra_values_bits; /* values as plain bits */
  /* redundant_pointers (SadaCount, include/gcsa/support.h:231-279) */
  uint64_t redundant_len;            /* data.size() */
  const uint64_t* redundant_bits;    /* data */

  /* LCPArray (include/gcsa/lcp.h:182-190); lcp_data NULL = no parent/depth support */
  uint64_t lcp_size;              /* header.size = number of leaves */
  uint64_t lcp_branching;         /* header.branching */
  uint64_t lcp_levels;            /* offsets.size() - 1 */
  const uint64_t* lcp_offsets;    /* lcp_levels + 1 entries */
  const uint8_t*  lcp_data;       /* data widened to bytes, lcp_offsets[lcp_levels] entries */

  /* alpha.comp2char, sigma entries, or NULL (round 3; appended).  The query path never reads it; it is kept so that
   * load + serialize reproduces a file's alphabet.  NULL = derived from char2comp (gcsa2_derive_comp2char). */
  const uint8_t*  comp2char;
} gcsa2_host_view;

#define GCSA2_MAX_SIGMA 16

typedef struct gcsa2_index gcsa2_index;   /* opaque; owns the device image */

/* Suffix-tree node, field for field gcsa::STNode (include/gcsa/lcp.h:40-79). */
typedef struct gcsa2_stnode {
  uint64_t sp, ep;
  uint64_t left_lcp, right_lcp;
  uint64_t node_lcp;              /* GCSA2_UNKNOWN = STNode::UNKNOWN */
} gcsa2_stnode;

#define GCSA2_UNKNOWN (~(uint64_t)0)

/* ---- lifetime ----------------------------------------------------------------------------- */

/* Number of visible HIP devices, or a negative status. */
int gcsa2_device_count(void);

/* Build the device image of `view` on HIP device `device`.  Replaces GCSA::load + LCPArray::load
 * followed by nothing: the reference queries host RAM in place (benchmark/query_gcsa.cpp:55,63).
 * The image (rank blocks, select hints, fused LF blocks) is built ON the device: every bulk array of the view (bwt[c],
 * edge_bits, the sample and counter bit arrays, stored_samples, lcp_data) is copied to HBM once, 1/8 byte per bit, and
 * may itself be in host, pinned or device memory (hipMemcpyDefault).  char2comp, C, lcp_offsets, comp2char and the
 * pointer table `bwt` are read by the host.  No host copy of the image is made. */
int gcsa2_index_create(const gcsa2_host_view* view, int device, gcsa2_index** out);
void gcsa2_index_destroy(gcsa2_index* index);

/* The optional tables of an image -- memoisations of reference functions that change no result: the two-character pair
 * blocks (10.7 bytes per path node; two LF steps of gcsa.h:155-162 per memory request), the k-mer seed table (8 * 4^k bytes;
 * find() of every k-mer, gcsa.h:96-110) and the locate table (8 bytes per path node; the walk of locateInternal,
 * src/gcsa.cpp:880-896).  gcsa2_index_create builds what the free device memory allows, or what the environment says, read
 * once at create time: GCSA2_PAIR_BLOCKS=0, GCSA2_KMER_TABLE=k, GCSA2_LOCATE_TABLE=0, and GCSA2_MEMORY_BUDGET_MB=m, a cap on
 * the whole image under which the tables are taken in the order seed table (small) / pair blocks / seed table (grown) /
 * locate table.  gcsa2_index_set_tables re-shapes an existing image, e.g. to give memory back under pressure:
 * pair_blocks and locate_table: 0 = drop, 1 = build if absent, -1 = leave; kmer_k: 0 = drop, 1..16 = exactly that size,
 * -1 = leave.  It waits for the device to idle first; the caller must not run queries on this handle (or on facade copies
 * sharing it) during the call.  On failure the table in question is absent and every query still works. */
int gcsa2_index_set_tables(gcsa2_index* index, int pair_blocks, int kmer_k, int locate_table);
/* A handle keeps what its host-pointer entry points have grown to: the pipeline of gcsa2_find_batch (6 lanes x 2 sets of
 * ~14 MB: about 170 MB of page-locked host memory and as much device memory, made at the first batch of 2^19 or more
 * patterns), the staging objects of the small calls (8 MB pinned + a grow-only device arena each) and the stream-ordered
 * scratch pool of the queries.  gcsa2_index_trim gives all of it back (the next call builds what it needs again); like
 * set_tables it waits for the device and must not run beside queries on the same handle. */
int gcsa2_index_trim(gcsa2_index* index);
/* Shape of that pipeline: `lanes` host threads, each with its stream and two staging sets (1..16; default 6, or
 * GCSA2_PIPE_LANES at create time), 2^chunk_log2 patterns per chunk (15..20; default 18, GCSA2_PIPE_CHUNK); 0 leaves a value
 * as it is; blocking: 1 = the lanes sleep while they wait for a chunk (hipEventBlockingSync), 0 = they spin, -1 = as it is.
 * Trims the handle first (same rules as gcsa2_index_trim).  What is best depends on the host: tests/perf/
 * packed_pipeline.py sweeps both on a live image. */
int gcsa2_index_set_pipeline(gcsa2_index* index, int lanes, int chunk_log2, int blocking);

/* Thread-local description of the last failing call. */
const char* gcsa2_last_error(void);

/* GCSAHeader accessors (include/gcsa/gcsa.h:137-148). */
uint64_t gcsa2_size(const gcsa2_index* index);
uint64_t gcsa2_edge_count(const gcsa2_index* index);
uint64_t gcsa2_order(const gcsa2_index* index);
uint64_t gcsa2_sample_count(const gcsa2_index* index);
uint64_t gcsa2_sample_bits(const gcsa2_index* index);
int      gcsa2_device(const gcsa2_index* index);
/* Bytes of HBM held by the image. */
uint64_t gcsa2_device_bytes(const gcsa2_index* index);
/* Payload bits per rank block of the device layout (the unit of the roofline model). */
uint64_t gcsa2_block_bits(const gcsa2_index* index);

/* ---- find: GCSA::find(begin, end)  (include/gcsa/gcsa.h:96-122) ---------------------------- */

/* patterns = concatenated pattern bytes, pattern q = patterns[offsets[q] .. offsets[q+1]).
 * ranges[2q], ranges[2q+1] = (sp, ep), including the edge-space integers the reference returns
 * for a range that empties inside LF (gcsa.h:160).  */
int gcsa2_find_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets,
                     uint64_t n_queries, uint64_t* ranges);
int gcsa2_find_device(const gcsa2_index* index, const uint8_t* d_patterns,
                      const uint64_t* d_offsets, uint64_t n_queries, uint64_t* d_ranges,
                      void* stream);

/* find() of n_queries patterns of ONE length (k-mer batches) handed over as 2-bit codes: 8 bytes per 32 characters over the link
 * instead of 32 pattern bytes + an 8-byte offset.  Pattern q occupies W = ceil(pattern_length / 32) u64 words at codes[q W ..];
 * word j holds the characters at distance 32 j .. 32 j + 31 from the pattern's END, the character at distance t in bits
 * [2 (t & 31), 2 (t & 31) + 2) as comp - 1 (A C G T = 0 1 2 3 with the default alphabet; unused high bits zero) -- the order
 * the backward search of gcsa.h:96-110 consumes them.  Only comps 1..4 can be written: a pattern with any other character
 * goes through gcsa2_find_batch.  Same ranges as the byte interface (the parity suite compares the two). */
int gcsa2_find_batch_packed(const gcsa2_index* index, const uint64_t* codes, uint64_t pattern_length, uint64_t n_queries, uint64_t* ranges);
int gcsa2_find_packed_device(const gcsa2_index* index, const uint64_t* d_codes, uint64_t pattern_length, uint64_t n_queries,
                             uint64_t* d_ranges, void* stream);

/* Launch shape.  variant 2 = the default (k_find2, fused 128-byte blocks, what
 * gcsa2_find_device runs); variant 4 = the same kernel behind a device-side sort of the queries by
 * pattern length, for batches of very uneven lengths (the 64 chains of a wavefront then finish
 * together; results are written in query order as always; stream-ordered scratch, no host sync).
 * Any other value is refused (rounds 1-2 also shipped a first-generation kernel and persistent
 * wavefronts as variants 1 and 5; neither won anywhere, both are gone). */
int gcsa2_find_device_variant(const gcsa2_index* index, int variant, const uint8_t* d_patterns,
                              const uint64_t* d_offsets, uint64_t n_queries, uint64_t* d_ranges,
                              void* stream);

/* Instrumented find for the roofline model (not the timed path): same results in d_ranges, and
 * d_stats[0] += number of distinct fused LF blocks fetched (gcsa2_find_block_bytes() each),
 * d_stats[1] += LF steps executed, d_stats[2] += seed-table lookups (8 bytes each), d_stats[3] += jump-table
 * lookups (16 bytes each).  A step whose two endpoints fall into one block counts once; a
 * two-character step counts as two LF steps and one block per distinct endpoint block, and a replayed pair
 * counts every block it fetched.  d_stats[4] += fetch rounds taken by lanes (one per single or pair step attempted),
 * d_stats[5] += those whose two endpoints lay in different blocks (a second fetch round for the whole wavefront),
 * d_stats[6] += seed-table entries that were marked "wide" (the range is then searched from scratch).
 * d_stats holds EIGHT words (rounds 1-2: four; an ABI change of round 3), zeroed by the caller.  d_stats[7] is an INPUT: 0, or
 * the device address of a bitmap of uint32 words, zeroed by the caller, with one bit per block of the image -- sigma x
 * (path_nodes / 384 + 1) FLB128 blocks, then 16 x (path_nodes / 192 + 1) FLP128 blocks; the kernel sets the bit of every
 * block it fetches, so that the set bits are the batch's working set in blocks (bench.py reports it). */
uint64_t gcsa2_find_block_bytes(const gcsa2_index* index);
/* Length k of the k-mer seed table built at create time (find() of every k-mer over comps 1..4,
 * memoised: a pattern whose last k characters are fast characters starts at step k).  0 = none.
 * One entry is 8 bytes (sp in 40 bits, range length in 24; the few ranges of 2^24 - 1 or more path nodes are
 * marked and searched from scratch).  Environment variable GCSA2_KMER_TABLE sets k (0 disables). */
uint64_t gcsa2_kmer_table_k(const gcsa2_index* index);
/* Bytes of the memoised locate table (0 = none): the walk of locateInternal (src/gcsa.cpp:880-896)
 * depends on the start node only, so it is run once per path node at create time and locate() reads
 * one 8-byte entry per path node instead of walking.  Needs samples; skipped when it would take
 * more than a third of the free device memory or when GCSA2_LOCATE_TABLE=0. */
uint64_t gcsa2_locate_table_bytes(const gcsa2_index* index);
/* Bytes of the jump table (0 = none): for every path node the chain of
 * up to 8 LF steps that is forced because each node on it has a single incoming label (a fast
 * character), with the node it ends in.  find() on a range of one path node whose next pattern
 * characters spell that chain moves there with one 16-byte lookup instead of one block fetch per
 * character; any other case steps as usual, so results (including the edge-space empty ranges of
 * include/gcsa/gcsa.h:160) are unchanged.  16 bytes per path node.
 * GCSA2_JUMP_TABLE (read at create time): unset -- built for a find-only image (one created without samples: no
 * locate(), no locate table; the jump table takes that table's place, last under GCSA2_MEMORY_BUDGET_MB) and not for an
 * image with samples; 1 -- attempted on any image; 0 -- never.  In every case only where the table leaves a sixteenth of
 * the device's memory free; an image that cannot have it is created without it, with no error.
 * GCSA2_JUMP_BUILD=double|walk (tests) forces one of the two builders, whose tables are identical: doubling through a
 * second buffer of the table's size (the default where both buffers pass the free-memory test), or one pass of chain
 * walks that needs no second buffer. */
uint64_t gcsa2_jump_table_bytes(const gcsa2_index* index);
/* An entry also holds the nodes after 4 and after `mid` steps of its chain, for patterns that end inside it.  mid is 2, or
 * 6 on an image with pair blocks whose table is larger than the 256 MiB last-level cache: there every lookup is a memory
 * request, a tail of 6 or 7 characters becomes one lookup instead of two, and a tail of 2 or 3 is left to the pair step.
 * Ranges are the same either way.  GCSA2_JUMP_MID=2|6 (read at create time; any other value is ignored) overrides the rule.
 * gcsa2_jump_mid: the value of this image (2 without a table); gcsa2_jump_mid_default: what the rule gives for an image of
 * `nodes` path nodes with (1) or without (0) pair blocks. */
int gcsa2_jump_mid(const gcsa2_index* index);
int gcsa2_jump_mid_default(uint64_t nodes, int pair_blocks);
/* Branch records: with mid = 6 the entry of a chain of at most 3 steps has two unused node slots.  Where that chain stops in
 * front of a node with exactly two incoming labels, both fast characters, the slots hold the two predecessors of that node
 * and a lookup carries a pattern that continues with either label one step past it, without the block fetch of that step.
 * Ranges are the same either way; the table's size does not change.  Built by default under the rule that gives mid = 6,
 * and never with mid = 2; GCSA2_JUMP_BRANCH=0|1 (read at create time; any other value is ignored) overrides the rule, so 1
 * together with GCSA2_JUMP_MID=6 builds them on a small image, which GCSA2_JUMP_MID=6 alone does not.
 * gcsa2_jump_branch: 1 when this image's table holds records; gcsa2_jump_branch_default: what the rule gives. */
int gcsa2_jump_branch(const gcsa2_index* index);
int gcsa2_jump_branch_default(uint64_t nodes, int pair_blocks);
/* Bytes of the two-characters-per-step blocks (0 = none).  For every ordered pair of fast characters the
 * composition of two LF steps (gcsa.h:155-162 applied twice) is stored as one rank structure of 128-byte
 * blocks over 192 path nodes each (gcsa2_amd/csrc/layout.hpp "FLP128"): find() then consumes two pattern
 * characters per memory request.  A block also tells which of its two steps empties, if any: an emptying second
 * step yields the edge-space integers of gcsa.h:160 directly, an emptying first step is replayed through the
 * single-character blocks, so every range is unchanged.  10.7 bytes per path node, built on the device at create
 * time; GCSA2_PAIR_BLOCKS=0 disables. */
uint64_t gcsa2_pair_block_bytes(const gcsa2_index* index);
int gcsa2_find_stats_device(const gcsa2_index* index, const uint8_t* d_patterns,
                            const uint64_t* d_offsets, uint64_t n_queries, uint64_t* d_ranges,
                            uint64_t* d_stats, void* stream);

/* ---- LF: GCSA::LF(range, comp) (gcsa.h:155-162), GCSA::LF(path_node) (gcsa.h:165-183),
 *      GCSA::charRange(comp) (gcsa.h:150-153) ------------------------------------------------- */
int gcsa2_lf_batch(const gcsa2_index* index, const uint64_t* ranges_in, const uint8_t* comps,
                   uint64_t n_queries, uint64_t* ranges_out);
int gcsa2_lf_device(const gcsa2_index* index, const uint64_t* d_ranges_in, const uint8_t* d_comps,
                    uint64_t n_queries, uint64_t* d_ranges_out, void* stream);
int gcsa2_lf_node_batch(const gcsa2_index* index, const uint64_t* nodes_in, uint64_t n_queries,
                        uint64_t* nodes_out);
int gcsa2_char_range(const gcsa2_index* index, uint8_t comp, uint64_t* sp, uint64_t* ep);
/* GCSA::LF_fast / LF_all (src/gcsa.cpp:742-798): ranges_out holds sigma ranges per query,
 * entries the reference leaves untouched are written as the empty range (1, 0).
 * all = 0: comps 1..fast_chars; all = 1: comps 1..sigma-2. */
int gcsa2_lf_all_batch(const gcsa2_index* index, const uint64_t* ranges_in, uint64_t n_queries,
                       int all, uint64_t* ranges_out);

/* ---- extend: the loop of GCSA::find (gcsa.h:96-110) continued from caller ranges ------------------------------------------
 * The reference's low-level interface (LF(range, comp), gcsa.h:133-162) is public so that a caller can keep a SEARCH STATE --
 * a range plus a cursor into a read -- and carry it on later: a branch of a fan-out over the bases at a low-quality position,
 * a seed resumed from a stored range, find() of a substring of a read.  One call continues n_states such searches, each over
 * a substring of one pattern of a shared pattern set, in one launch.  (d_patterns, d_offsets) is the pattern CSR of
 * gcsa2_find_device: n_patterns + 1 offsets, alignment and padding as under "Conventions"; many states may name one pattern.
 *
 * For one state s, with P = pattern s.pattern, the result is DEFINED by this walk:
 *
 *   r = (s.sp, s.ep); last = r; matched = 0; i = s.end
 *   while i > s.begin and not empty(r):            (Range::empty, utils.h:93-96)
 *     i -= 1; r = LF(r, char2comp[P[i]])           (gcsa.h:155-162)
 *     if not empty(r): matched += 1; last = r
 *   out = { matched, r.sp, r.ep, last.sp, last.ep }
 *
 * What follows from it:
 *   - (sp, ep) is exactly what the reference's loop `while(!empty(range) && end != begin) range = LF(range, *--end)` leaves:
 *     when a step empties the range, that step's edge-space integers (gcsa.h:160), as find() returns them.
 *   - (last_sp, last_ep) is the range of the longest matched suffix P[end - matched, end) extended from the start range; it
 *     equals (sp, ep) when no step emptied.
 *   - An empty start range, begin == end or an index of size 0: the start range in both places, matched = 0.
 *   - A state that starts at (0, size() - 1) gives find(P[begin, end)) whenever that is non-empty; both are empty otherwise
 *     (find() starts from charRange of the last character, whose empty form differs from the edge-space pair of an LF step).
 *   - find(P) == extend(find(P[c:]), P[:c]) for every cut c < |P|, empty results included, bit for bit (c = |P| is the
 *     start at the root of the line above).
 *   - An INVALID state -- pattern >= n_patterns, begin > end, or end beyond the pattern's length -- is not searched and no
 *     pattern byte is read for it: out = { GCSA2_UNKNOWN, s.sp, s.ep, s.sp, s.ep }.  So the device form needs no read-back
 *     to refuse a state, and a bad cursor cannot fault the GPU.
 *   - The ranges themselves are not validated, like the rest of the low-level interface.
 *
 * gcsa2_extend_device only enqueues on `stream`.  n_states == 0 is GCSA2_OK; a NULL index is GCSA2_ERR_INVALID_ARGUMENT before
 * any device is touched.  gcsa2_extend_batch takes host pointers, requires offsets[0] == 0, runs in one piece (patterns,
 * offsets, states and results must fit in device memory together) and is complete on return.  Where the image has pair
 * blocks (gcsa2_pair_block_bytes) two characters cost one memory request per endpoint whenever both steps stay non-empty;
 * anything else is stepped singly, so every field is the walk's. */
typedef struct gcsa2_search_state { uint64_t pattern, begin, end, sp, ep; } gcsa2_search_state;
typedef struct gcsa2_extension    { uint64_t matched, sp, ep, last_sp, last_ep; } gcsa2_extension;
int gcsa2_extend_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                        const gcsa2_search_state* d_states, uint64_t n_states, gcsa2_extension* d_out, void* stream);
int gcsa2_extend_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                       const gcsa2_search_state* states, uint64_t n_states, gcsa2_extension* out);

/* ---- k-mer windows: find() and count() of every k-mer of every read, with per-read profiles --------------------------------
 * A pattern set of gcsa2_find_device cannot hold overlapping patterns, so a k-mer user (genotyping, read screening, seed
 * weighting) would have to copy every window out.  Here the reads are the pattern set and the windows are implied.
 * (d_patterns, d_offsets, n_patterns) is the pattern CSR of gcsa2_find_device; k >= 1 is the window length, stride >= 1.
 *
 * DEFINITION.  For read q = P_q of length L:
 *   - W_q = 0 windows if L < k, else (L - k) / stride + 1; window j of read q is P_q[j stride, j stride + k).
 *   - Its global index is w = window_offsets[q] + j, window_offsets being the exclusive prefix sum of W_q (n_patterns + 1
 *     entries; the last one is the total).
 *   - range(w) = (d_ranges[2w], d_ranges[2w + 1]) is exactly what gcsa2_find_device returns for that substring handed over as
 *     a pattern of its own, bit for bit, both empty forms included: the empty charRange of the last character, and the
 *     edge-space integers of the LF step that emptied the range (gcsa.h:160).
 *   - count(w) = d_counts[w] = GCSA::count(range(w)) (src/gcsa.cpp:802-809; 0 for an empty range).
 *   - profile(q) = { windows = W_q, found = the number of non-empty ranges among the read's windows, nodes = the sum of
 *     Range::length over those, occurrences = the sum of count(w) }; occurrences is 0 without GCSA2_KMER_COUNTS.
 * k may exceed gcsa2_order(): the results are find()'s, false positives included (a path of the graph need not spell a
 * k-mer longer than the order), exactly as for gcsa2_find_device.
 *
 * Outputs.  Any of d_window_offsets, d_profiles, d_ranges, d_counts may be NULL; the library keeps the window offsets in
 * stream-ordered scratch when the caller does not want them, and zeroes the profiles itself.  `capacity` is the number of
 * windows d_ranges / d_counts hold (ignored when both are NULL).  *total_windows is always the number needed; when d_ranges
 * or d_counts is given and it exceeds capacity the call fails with GCSA2_ERR_BUFFER_TOO_SMALL: d_window_offsets (if given)
 * is complete then, and nothing is written into d_ranges, d_counts or d_profiles.  Nothing is ever written behind a capacity.
 * GCSA2_ERR_INVALID_ARGUMENT, with nothing written and before any device is touched: k == 0, stride == 0, d_counts without
 * GCSA2_KMER_COUNTS, an unknown flag, a NULL index (or a NULL total_windows).  GCSA2_KMER_COUNTS on an image without counters:
 * GCSA2_ERR_MISSING_COMPONENT, likewise.
 *
 * The device form follows the buffer conventions at the top of this header; no pattern byte outside the 8-byte words that
 * hold [d_offsets[0], d_offsets[n_patterns]) is read, whatever k and the read lengths are.  It reads *total_windows back
 * once, so it is enqueued on `stream` and complete on return, like gcsa2_mem_hits_device.  One call takes fewer than 2^32
 * windows: more is refused with GCSA2_ERR_BUFFER_TOO_SMALL ("split the batch"; *total_windows is still the number,
 * d_window_offsets complete, nothing else written), and 2^32 reads or more likewise, before any work (*total_windows = 0,
 * nothing written).  The jump table of a find-only image is not
 * consulted (the ranges are find()'s either way); pair blocks and the seed table are used as find() uses them.
 *
 * The host form requires offsets[0] == 0 and refuses decreasing offsets (GCSA2_ERR_INVALID_ARGUMENT).  It knows the total
 * before any device work, so on GCSA2_ERR_BUFFER_TOO_SMALL it writes nothing at all but *total_windows.  A batch of 64 MB of
 * reads or more travels in pieces of whole reads (GCSA2_MS_PIECE_MB, GCSA2_MS_THREADS, as the MEM calls); windows, counts and
 * profiles keep the order of the reads.  With profiles as the only output a piece moves its reads (bytes and offsets) in and
 * 32 bytes per read out, and nothing else. */
typedef struct gcsa2_kmer_profile { uint64_t windows, found, nodes, occurrences; } gcsa2_kmer_profile;
#define GCSA2_KMER_COUNTS 1   /* evaluate count(): d_counts and profile.occurrences; needs the counters */
int gcsa2_kmer_windows_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                              uint64_t k, uint64_t stride, int flags,
                              uint64_t* d_window_offsets,        /* n_patterns + 1, or NULL */
                              gcsa2_kmer_profile* d_profiles,    /* n_patterns, or NULL */
                              uint64_t* d_ranges,                /* 2 per window, or NULL */
                              uint64_t* d_counts,                /* 1 per window, or NULL */
                              uint64_t capacity,                 /* windows that d_ranges / d_counts hold */
                              uint64_t* total_windows, void* stream);
int gcsa2_kmer_windows_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                             uint64_t k, uint64_t stride, int flags, uint64_t* window_offsets, gcsa2_kmer_profile* profiles,
                             uint64_t* ranges, uint64_t* counts, uint64_t capacity, uint64_t* total_windows);

/* ---- count: GCSA::count(range) (src/gcsa.cpp:802-809) -------------------------------------- */
int gcsa2_count_batch(const gcsa2_index* index, const uint64_t* ranges, uint64_t n_queries,
                      uint64_t* counts);
int gcsa2_count_device(const gcsa2_index* index, const uint64_t* d_ranges, uint64_t n_queries,
                       uint64_t* d_counts, void* stream);

/* ---- scalar calls: the per-character caller (include/gcsa/gcsa.h:155-162 in a loop; vg's MEM finder) ---------------------
 * A one-query call of gcsa2_lf_batch / gcsa2_lf_node_batch / gcsa2_count_batch / gcsa2_parent_batch -- what the facade's
 * scalar LF() / count() / parent() make -- does not launch a kernel: the request goes through a page-locked slot to ONE
 * resident wavefront of the index's device, which answers in the same slot (4 us per call instead of 12-17 through a launch;
 * a CPU LF step takes 0.35 us, paper.tex:408: batches remain the way to throughput).  The wavefront is launched by the first
 * such call, leaves by itself after GCSA2_MAILBOX_PARK_US (default 200) microseconds without a request -- that is how long a
 * device-wide synchronisation elsewhere in the process may wait for it -- and after GCSA2_MAILBOX_LIFE_MS (20) in any case; the
 * next call launches it again.  It occupies one wavefront slot of one CU while it lives.  One host thread at a time uses it;
 * a second thread's call takes the launch path meanwhile.  GCSA2_MAILBOX=0 (read at create time) switches it off.  Results
 * are those of the batch kernels bit for bit (the same device functions).  gcsa2_mailbox_stats: calls answered, launches. */
int gcsa2_mailbox_stats(const gcsa2_index* index, uint64_t* calls, uint64_t* launches);

/* ---- locate: GCSA::locate(range, results, append=false, sort) (src/gcsa.cpp:827-842) -------
 * Two calls, CSR output.  locate_run runs the whole query and keeps the result on the device
 * inside `*job`; locate_fetch copies the values (offsets[n_queries] of them) and frees the job.
 * Both, and gcsa2_locate_device below, are complete on return: *total_values is read back, and the job's
 * buffers are plain allocations (a device-wide wait), so nothing is left on `stream`.
 * sort != 0: sorted distinct values per query (removeDuplicates, utils.h:350-357), so
 *            offsets[q+1] - offsets[q] == count(range q).
 * sort == 0: values in path order, duplicates kept, exactly as the reference pushes them.
 * A batch of any size: one pass of the pipeline takes fewer than 2^31 values before deduplication (its library scans and
 * segmented sort count in int); a larger batch -- the paper's 16-mer batch has 2.5 G values -- is cut into consecutive
 * sub-batches of queries whose results are concatenated.  Only a single range with that many values is refused
 * (GCSA2_ERR_BUFFER_TOO_SMALL). */
typedef struct gcsa2_locate_job gcsa2_locate_job;
int gcsa2_locate_run(const gcsa2_index* index, const uint64_t* ranges, uint64_t n_queries,
                     int sort, uint64_t* offsets /* n_queries + 1 */, gcsa2_locate_job** job);
int gcsa2_locate_fetch(gcsa2_locate_job* job, uint64_t* values, uint64_t capacity);
void gcsa2_locate_discard(gcsa2_locate_job* job);
/* Device-resident form for pipelines and the benchmark: d_ranges in HBM; on return
 * *d_offsets / *d_values point into memory owned by the job (valid until discard). */
int gcsa2_locate_device(const gcsa2_index* index, const uint64_t* d_ranges, uint64_t n_queries,
                        int sort, gcsa2_locate_job** job, const uint64_t** d_offsets,
                        const uint64_t** d_values, uint64_t* total_values, void* stream);
/* The same query into caller-owned device buffers (no allocation of results, for pipelines that
 * reuse their buffers): d_offsets has n_queries + 1 entries, d_values room for `capacity` values.
 * *total_values = number of values; if that exceeds capacity the call fails with
 * GCSA2_ERR_BUFFER_TOO_SMALL (*total_values tells how much is needed) and nothing has been written
 * behind d_values + capacity -- the buffer itself may hold a prefix of the result by then: the values
 * are compacted into it before the host has seen their number.  On success d_values[0, *total_values)
 * is the result; what lies between *total_values and capacity is unspecified: a buffer with room for
 * the values BEFORE deduplication (sum of the ranges' value counts, >= *total_values) is used as the
 * sorts' work space and compacted in place, and when no range repeats a value -- a text index -- nothing
 * is compacted at all.  Complete on return. */
int gcsa2_locate_into(const gcsa2_index* index, const uint64_t* d_ranges, uint64_t n_queries, int sort,
                      uint64_t* d_offsets, uint64_t* d_values, uint64_t capacity,
                      uint64_t* total_values, void* stream);

/* GCSA::locate(range, max_positions, results) (src/gcsa.cpp:844-878): at most max_positions
 * distinct values, chosen with the reference's std::mt19937_64(sp ^ ep) draws, sorted.
 * *count = number of values written (or needed, with GCSA2_ERR_BUFFER_TOO_SMALL). */
int gcsa2_locate_max(const gcsa2_index* index, uint64_t sp, uint64_t ep, uint64_t max_positions,
                     uint64_t* values, uint64_t capacity, uint64_t* count);

/* The same for a batch of ranges with one max_positions, one wavefront per range on the device, value for value and in
 * the same order as gcsa2_locate_max.  CSR output: values[offsets[q], offsets[q + 1]) are the sorted values of range q,
 * min(max_positions, count(range q)) of them -- fewer only where count() overstates a range's distinct values, as the
 * reference allows (the slots are sized by count() and closed up afterwards then).  A count() of 2^40 or more (one that
 * wrapped below zero) does not size a slot: such a range is answered first and its slot is its result.  The values need room
 * for the sum of the slots; if that exceeds capacity the call fails with GCSA2_ERR_BUFFER_TOO_SMALL (*total tells how much
 * is needed) and no value is written.  Otherwise *total = offsets[n_queries].  Where the reference would draw forever (fewer
 * distinct values than it waits for), the call fails with GCSA2_ERR_INVALID_ARGUMENT, at the latest after
 * 64 max_positions + 64 draws of a range.  Batches of fewer than 2^24 ranges (GCSA2_ERR_BUFFER_TOO_SMALL otherwise: split
 * the batch).  Host arrays; complete on return. */
int gcsa2_locate_max_batch(const gcsa2_index* index, const uint64_t* ranges, uint64_t n_queries, uint64_t max_positions,
                           uint64_t* offsets /* n_queries + 1 */, uint64_t* values, uint64_t capacity, uint64_t* total);
/* Into caller-owned device buffers (d_ranges, d_offsets with n_queries + 1 entries, d_values with room for `capacity`
 * values), with the GCSA2_ERR_BUFFER_TOO_SMALL contract of gcsa2_locate_into: nothing is written behind
 * d_values + capacity.  Enqueued on `stream`, complete on return. */
int gcsa2_locate_max_into(const gcsa2_index* index, const uint64_t* d_ranges, uint64_t n_queries, uint64_t max_positions,
                          uint64_t* d_offsets, uint64_t* d_values, uint64_t capacity, uint64_t* total, void* stream);

/* sampled / sampleRange / firstSample (gcsa.h:191-206): out[3q] = sampled(node),
 * out[3q+1] = sampleRange(node).first (= firstSample(node)), out[3q+2] = sampleRange(node).second. */
int gcsa2_sample_range_batch(const gcsa2_index* index, const uint64_t* nodes, uint64_t n_queries,
                             uint64_t* out);
/* sample(i) and lastSample(i) (gcsa.h:208-210). */
int gcsa2_sample_batch(const gcsa2_index* index, const uint64_t* sample_indexes, uint64_t n_queries,
                       uint64_t* values, uint8_t* last_flags);
/* sampledPositions() (gcsa.h:143-148) and the Alphabet members callers read (support.h:150-151). */
uint64_t gcsa2_sampled_positions(const gcsa2_index* index);
uint64_t gcsa2_sigma(const gcsa2_index* index);
uint64_t gcsa2_fast_chars(const gcsa2_index* index);
void gcsa2_alphabet(const gcsa2_index* index, uint8_t* char2comp /* 256 */, uint64_t* C /* sigma + 1 */);
/* comp2char of an alphabet given by char2comp alone: per comp the first byte that is not a lower-case letter and not NUL
 * (else the first byte), and the reference's "$ACGTN#" for its default alphabet (src/support.cpp:69-92).  The one rule behind
 * the facade's Alphabet and GCSA::serialize when a view carries no comp2char.  Host only. */
void gcsa2_derive_comp2char(const uint8_t* char2comp /* 256 */, uint64_t sigma, uint8_t* comp2char /* sigma */);

/* ---- suffix-tree operations: LCPArray::parent / depth / psv / psev / nsv / nsev / rmq
 *      (include/gcsa/lcp.h:137-178, src/lcp.cpp:276-519) -------------------------------------- */
int gcsa2_parent_batch(const gcsa2_index* index, const uint64_t* ranges, uint64_t n_queries,
                       gcsa2_stnode* nodes);
int gcsa2_parent_device(const gcsa2_index* index, const uint64_t* d_ranges, uint64_t n_queries,
                        gcsa2_stnode* d_nodes, void* stream);
int gcsa2_depth_batch(const gcsa2_index* index, const uint64_t* ranges, uint64_t n_queries,
                      uint64_t* depths);
/* op: 0 psv, 1 psev, 2 nsv, 3 nsev.  results[2q], results[2q+1] = (position, LCP value) or
 * notFound() = (values(), values()). */
int gcsa2_sv_batch(const gcsa2_index* index, int op, const uint64_t* positions,
                   uint64_t n_queries, uint64_t* results);
/* rmq(sp, ep): leftmost minimum of LCP[sp..ep] as (position, value), or notFound(). */
int gcsa2_rmq_batch(const gcsa2_index* index, const uint64_t* ranges, uint64_t n_queries,
                    uint64_t* results);

/* LCPArray::size / values / levels / branching / operator[] (lcp.h:124-129). */
uint64_t gcsa2_lcp_size(const gcsa2_index* index);
uint64_t gcsa2_lcp_values(const gcsa2_index* index);
uint64_t gcsa2_lcp_levels(const gcsa2_index* index);
uint64_t gcsa2_lcp_branching(const gcsa2_index* index);
int gcsa2_lcp_access_batch(const gcsa2_index* index, const uint64_t* positions, uint64_t n_queries,
                           uint64_t* out);

/* ---- countKMers(index, k, parameters) (include/gcsa/algorithms.h:73-84, src/algorithms.cpp:387-421):
 * number of distinct k-mers in the index = non-empty states at depth k of the search tree,
 * expanding with LF_fast (bases only) or, include_ns != 0, LF_all.  k > order() yields 0 unless
 * force != 0, k == 0 yields 1, as in the reference. */
int gcsa2_count_kmers(const gcsa2_index* index, uint64_t k, int include_ns, int force, uint64_t* result);

/* compareKMers(left, right, k, parameters) (include/gcsa/algorithms.h:86-92, src/algorithms.cpp:534-616):
 * result[0..2] = number of k-mers in both indexes, only in the left, only in the right one.  Same early exits as the
 * reference (k == 0 -> {1,0,0}; k > order without force, k > 64, incompatible alphabets -> zeros).
 * Both indexes must be on the same device. */
int gcsa2_compare_kmers(const gcsa2_index* left, const gcsa2_index* right, uint64_t k, int include_ns,
                        int force, uint64_t* result);
/* The same, also returning the search states of the k-mers found in one index only, as the reference
 * writes them to parameters.output + ".left" / ".right" (src/algorithms.cpp:425-457, 606-610): 8 u64
 * per state = left range, right range, k, kmer[3] (3 bits per comp, extension step i at bits
 * [3i, 3i+3), i.e. the LAST character of the k-mer first).  Order within a buffer is unspecified (the
 * reference's depends on its OpenMP schedule).  Capacities are in states; if result[1] / result[2]
 * exceed them the call fails with GCSA2_ERR_BUFFER_TOO_SMALL and result[] holds the sizes needed. */
int gcsa2_compare_kmers_records(const gcsa2_index* left, const gcsa2_index* right, uint64_t k,
                                int include_ns, int force, uint64_t* result,
                                uint64_t* left_records, uint64_t left_capacity,
                                uint64_t* right_records, uint64_t right_capacity);

/* ---- matching statistics: the LF + parent interplay of vg's MEM finder, fused ---------------
 * (paper/paper.tex:344 "maximal exact matches by using LF-mapping and parent
 * queries").  Composition of GCSA::LF(range, comp) (gcsa.h:155-162) and LCPArray::parent(range)
 * (src/lcp.cpp:276-301), scanning each pattern right to left: on an empty LF result the range is
 * replaced by its parent and the character retried; at the root the character is skipped.
 * ms[offsets[q] + i] = length of the longest match starting at byte i of pattern q that the
 * index reports (capped at 65535; exact for lengths <= order()), ranges[2q..] = range of that
 * match for i = 0, fallbacks[q] = number of parent() calls (may be NULL).  Needs the LCP array.
 * The dense calls take no maximum match length (gcsa2_match_breaks_bounded_device below): after a cut the search goes on from
 * the parent of the capped range, and one statistic per position does not follow from the capped records. */
int gcsa2_match_stats_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets,
                            uint64_t n_queries, uint16_t* ms, uint64_t* ranges, uint64_t* fallbacks);
int gcsa2_match_stats_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets,
                             uint64_t n_queries, uint16_t* d_ms, uint64_t* d_ranges, uint64_t* d_fallbacks,
                             void* stream);
/* Launch shape, same results.  variant 2 = one lane per pattern (wave-cooperative block fetch); variant 5 = the same kernel
 * as persistent wavefronts whose idle lanes draw the next pattern from a counter -- for batches of ragged pattern lengths
 * or of uneven difficulty (a pattern with mismatches takes three times the rounds of one without); variant 0 = the
 * library chooses (what gcsa2_match_stats_device runs): persistent lanes when the batch is more than two generations of
 * resident workgroups, and gcsa2_match_stats_batch also when the longest pattern exceeds 1.25 x the mean.  Any other
 * value is refused.
 * The kernel reads the patterns as 2-bit codes prepared by a pre-pass into stream-ordered scratch, whose size depends on
 * d_offsets[n_queries]: gcsa2_match_stats_device and _variant read that value back (ONE wait for `stream` per call);
 * gcsa2_match_stats_device_sized takes it from the caller (total_pattern_bytes) and only enqueues. */
int gcsa2_match_stats_device_variant(const gcsa2_index* index, int variant, const uint8_t* d_patterns,
                                     const uint64_t* d_offsets, uint64_t n_queries, uint16_t* d_ms,
                                     uint64_t* d_ranges, uint64_t* d_fallbacks, void* stream);
int gcsa2_match_stats_device_sized(const gcsa2_index* index, int variant, const uint8_t* d_patterns,
                                   const uint64_t* d_offsets, uint64_t n_queries, uint64_t total_pattern_bytes,
                                   uint16_t* d_ms, uint64_t* d_ranges, uint64_t* d_fallbacks, void* stream);
/* The same backward search with parent() on failure, reported as BREAK POINTS instead of one statistic per position: the
 * left-maximal matches a MEM finder collects (vg's caller shape; the reference exercises the LF + parent interplay in
 * verifyIndex, src/algorithms.cpp:146-167).  A record {position p, length, sp, ep} says that P[p, p + length) occurs with
 * path-node range (sp, ep) = find() of that substring (include/gcsa/gcsa.h:96-110) and cannot be extended by P[p - 1];
 * exactly the positions p with p == 0 or ms[p - 1] != ms[p] + 1 have a record (an empty pattern has none; a record of length 0
 * -- no character of the index at p, nor at p - 1 -- carries the whole index as its range).  Records of pattern q: d_breaks[d_break_offsets[q] .. d_break_offsets[q + 1]), in the order
 * of discovery (descending position).  The dense statistics follow from them: ms[i] = length - (i - p) for the record with the
 * largest p <= i.  d_break_offsets: n_queries + 1 entries; capacity: records d_breaks holds; *total_breaks: records found --
 * GCSA2_ERR_BUFFER_TOO_SMALL with that number when it exceeds capacity (nothing is written then).  d_ranges (final ranges) and
 * d_fallbacks (parent() calls per pattern) may be NULL.  variant as in gcsa2_match_stats_device_variant.  min_length > 0 keeps
 * only the records of at least that length -- a MEM finder's minimum match length: right after a mismatch the matches are as
 * short as any string of log4(n) characters and every position is a break point, which on a whole-genome index makes more
 * bytes of records than the dense statistics have; the dense form no longer follows from the records then.  Complete on return. */
typedef struct gcsa2_break { uint64_t position, length, sp, ep; } gcsa2_break;
int gcsa2_match_breaks_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_queries,
                              uint64_t total_pattern_bytes, int variant, uint64_t min_length, uint64_t* d_break_offsets, gcsa2_break* d_breaks,
                              uint64_t capacity, uint64_t* total_breaks, uint64_t* d_ranges, uint64_t* d_fallbacks, void* stream);
/* The same for a batch in host memory (offsets[0] == 0): copies in, runs, copies the CSR out.  ranges / fallbacks may be NULL.
 * A batch of two pieces' worth of pattern bytes or more goes in pieces (32 MB each, GCSA2_MS_PIECE_MB; four host threads with a stream each)
 * whose records are committed in pattern order; with GCSA2_ERR_BUFFER_TOO_SMALL (*total_breaks = the records of the whole batch)
 * the contents of the result arrays are unspecified. */
int gcsa2_match_breaks_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_queries,
                             uint64_t min_length, uint64_t* break_offsets, gcsa2_break* breaks, uint64_t capacity,
                             uint64_t* total_breaks, uint64_t* ranges, uint64_t* fallbacks);
/* The break points with a MAXIMUM MATCH LENGTH.  The index answers for patterns up to its order: "the pattern may be longer
 * than the order of the index, but this may result in false positives" (the reference, include/gcsa/gcsa.h:91, and its
 * README), so a record longer than gcsa2_order() may describe a path the graph does not have.  A mapper bounds its matches:
 * one that has reached max_length characters is cut as if the next character had failed, and the search goes on from
 * parent().  This is not a filter of the unbounded records -- after a cut the walk continues from the parent of the CAPPED
 * range, and the records that follow differ in position, length and range.  The definition is this walk over
 * GCSA::LF(range, comp) (gcsa.h:155-162) and LCPArray::parent(range) (src/lcp.cpp:276-301), per pattern P, right to left,
 * n = gcsa2_size():
 *
 *   i = |P|; r = (0, n - 1); depth = 0; last = none; parents = 0
 *   while i > 0:
 *     if not (max_length > 0 and depth >= max_length):
 *       r2 = LF(r, char2comp[P[i - 1]])
 *       if r2 is not empty: r = r2; depth += 1; i -= 1; continue
 *     if r == (0, n - 1):                                   (the root: reached through a failed LF only)
 *       depth = 0; i -= 1
 *       if i + 1 < |P| and last != i + 1: record {i + 1, 0, 0, n - 1}; last = i + 1
 *       continue
 *     if last != i: record {i, depth, r.sp, r.ep}; last = i
 *     p = parent(r); r = (p.sp, p.ep); depth = p.lcp; parents += 1
 *   if |P| > 0 and last != 0: record {0, depth, r.sp, r.ep}
 *
 * The records of length >= min_length are kept, in this order (descending position); d_fallbacks[q] = parents, the parent()
 * calls forced by the cap included; d_ranges[2q..] = r at the end.  Every record has length <= max_length and (sp, ep) =
 * find(P[position, position + length)).  max_length == 0: no cap -- the walk is then the contract of gcsa2_match_breaks_device,
 * and the results are the same bit for bit; a max_length of 2^32 or more can never be reached and means the same.  A mapper
 * passes gcsa2_order().  max_length != 0 && min_length > max_length: GCSA2_ERR_INVALID_ARGUMENT, nothing is written.
 * Everything else -- buffers, capacity, *total_breaks, variant, pieces of the host form -- as the unbounded calls, which are
 * these with max_length = 0. */
int gcsa2_match_breaks_bounded_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_queries,
                                      uint64_t total_pattern_bytes, int variant, uint64_t min_length, uint64_t max_length,
                                      uint64_t* d_break_offsets, gcsa2_break* d_breaks, uint64_t capacity, uint64_t* total_breaks,
                                      uint64_t* d_ranges, uint64_t* d_fallbacks, void* stream);
int gcsa2_match_breaks_bounded_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_queries,
                                     uint64_t min_length, uint64_t max_length, uint64_t* break_offsets, gcsa2_break* breaks,
                                     uint64_t capacity, uint64_t* total_breaks, uint64_t* ranges, uint64_t* fallbacks);
/* MEM hits: the break records of gcsa2_match_breaks_device with count() and their positions, a MEM finder's seeds in one
 * call.  MEMs of pattern q: d_mems[d_mem_offsets[q] .. d_mem_offsets[q + 1]), exactly the records gcsa2_match_breaks_device
 * returns for min_length (min_length >= 1, GCSA2_ERR_INVALID_ARGUMENT otherwise), in the same order, each with
 * count = GCSA::count(sp, ep).  Hits of MEM i: d_hits[d_hit_offsets[i] .. d_hit_offsets[i + 1]):
 *   count == 0: none;
 *   hit_max == 0 (no cap) or count <= hit_max: the sorted distinct values of gcsa2_locate_into(sort = 1);
 *   otherwise, over == GCSA2_MEM_OVER_SKIP: none (the MEM and its count are still reported);
 *   otherwise, over == GCSA2_MEM_OVER_SAMPLE: the values of gcsa2_locate_max(range, hit_max), value for value and in order
 *   (src/gcsa.cpp:844-878); its INVALID_ARGUMENT for a range the reference would draw forever on is passed through.
 * d_mem_offsets: n_queries + 1 entries; d_hit_offsets: mem_capacity + 1.  *total_mems and *total_hits are always the sizes
 * needed; if either exceeds its capacity the call fails with GCSA2_ERR_BUFFER_TOO_SMALL and writes nothing into d_mems,
 * d_hit_offsets or d_hits.  Nothing is ever written behind d_mems + mem_capacity or d_hits + hit_capacity.  Needs the LCP
 * array, the samples and the counters (GCSA2_ERR_MISSING_COMPONENT).  total_pattern_bytes = d_offsets[n_queries] or
 * GCSA2_UNKNOWN (read back).  Enqueued on `stream`, complete on return. */
typedef struct gcsa2_mem { uint64_t position, length, sp, ep, count; } gcsa2_mem;
#define GCSA2_MEM_OVER_SKIP   0   /* count > hit_max: record the MEM and its count, no hits      */
#define GCSA2_MEM_OVER_SAMPLE 1   /* count > hit_max: hits = locate(range, hit_max) (gcsa.cpp:844-878) */
int gcsa2_mem_hits_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_queries,
                          uint64_t total_pattern_bytes, uint64_t min_length, uint64_t hit_max, int over,
                          uint64_t* d_mem_offsets, gcsa2_mem* d_mems, uint64_t mem_capacity, uint64_t* total_mems,
                          uint64_t* d_hit_offsets, uint64_t* d_hits, uint64_t hit_capacity, uint64_t* total_hits, void* stream);
/* The same for a batch in host memory (offsets[0] == 0): copies in, runs, copies out.  A batch of two pieces' worth of pattern
 * bytes or more (32 MB pieces, as gcsa2_match_breaks_batch) goes in pieces whose MEMs and hits keep their order; a batch in one
 * piece writes nothing into mems, hit_offsets or hits on GCSA2_ERR_BUFFER_TOO_SMALL, one in pieces leaves their contents
 * unspecified then.  Complete on return. */
int gcsa2_mem_hits_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_queries,
                         uint64_t min_length, uint64_t hit_max, int over,
                         uint64_t* mem_offsets, gcsa2_mem* mems, uint64_t mem_capacity, uint64_t* total_mems,
                         uint64_t* hit_offsets, uint64_t* hits, uint64_t hit_capacity, uint64_t* total_hits);
/* MEM hits with a maximum match length: the MEMs are exactly the records gcsa2_match_breaks_bounded_device returns for
 * (min_length, max_length) -- the walk stated there --, counts and hits by the rules of gcsa2_mem_hits_device.  max_length == 0
 * (or >= 2^32): no cap, the unbounded calls; max_length != 0 && min_length > max_length: GCSA2_ERR_INVALID_ARGUMENT, nothing is
 * written.  The pieces of the host form all run under the same max_length.  Sub-MEM reseeding (below) needs no cap of its own:
 * its matches lie inside the MEMs it is given. */
int gcsa2_mem_hits_bounded_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_queries,
                                  uint64_t total_pattern_bytes, uint64_t min_length, uint64_t max_length, uint64_t hit_max, int over,
                                  uint64_t* d_mem_offsets, gcsa2_mem* d_mems, uint64_t mem_capacity, uint64_t* total_mems,
                                  uint64_t* d_hit_offsets, uint64_t* d_hits, uint64_t hit_capacity, uint64_t* total_hits, void* stream);
int gcsa2_mem_hits_bounded_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_queries,
                                 uint64_t min_length, uint64_t max_length, uint64_t hit_max, int over,
                                 uint64_t* mem_offsets, gcsa2_mem* mems, uint64_t mem_capacity, uint64_t* total_mems,
                                 uint64_t* hit_offsets, uint64_t* hits, uint64_t hit_capacity, uint64_t* total_hits);
/* Sub-MEM reseeding: inside every MEM of at least reseed_length bases, the shorter matches that occur MORE OFTEN than the MEM
 * (vg's GCSA mapper reseeds such MEMs: a long, nearly unique match may cross a SNP or come from a paralog), with count() and
 * hits.  Input: the patterns and a MEM CSR as gcsa2_mem_hits_device returns it -- MEMs of pattern q are
 * d_mems[d_mem_offsets[q] .. d_mem_offsets[q + 1]) (n_queries + 1 offsets; n_mems = d_mem_offsets[n_queries], or GCSA2_UNKNOWN:
 * read back).  Of each MEM only {position b, length l, count c} are read.  A MEM with l < reseed_length gets no sub-MEMs;
 * the sub-MEMs of the others are what this walk emits, in its order (descending position, as match_breaks lists breaks):
 *
 *   E = b + l;  x = e = E;  r = (0, n - 1)            r is the range of P[x .. e)
 *   last_x = infinity
 *   while e >= b + min_length:
 *     if x > b:
 *       r2 = LF(r, char2comp[P[x - 1]])
 *       if r2 is not empty and count(r2) > c: x -= 1; r = r2; continue
 *     the match ending at e cannot be extended -- candidate [x, e):
 *     if e - x >= min_length and x < last_x: emit {x, e - x, r.sp, r.ep, count(r)}; last_x = x
 *     if x == b: stop
 *     if e == x: e -= 1; x = e; r = (0, n - 1); continue
 *     p = parent(r);  e = x + p.lcp;  r = p.range         (LCPArray::parent)
 *
 * This is the LF + parent() interplay of the matching statistics, where a step also fails when count() drops to c or below,
 * kept inside [b, E).  An emitted count is the one computed when the walk extended to that range (after a parent() jump x is
 * unchanged, so nothing is emitted before the next successful step).  Meaning: count(find(.)) never drops when a match is
 * shortened on the right, so while matches are no longer than the index's order the walk emits exactly the intervals [s, e)
 * where s is the leftmost start with count(find(P[s' .. e))) > c for all s <= s' < e, of length >= min_length and not
 * contained in one taken for a larger e -- the "backward search restarted at every end position" form of reseeding, in linear
 * rather than quadratic time.  c = 0 gives the maximal matches inside the interval.
 * Sub-MEMs of MEM k: d_subs[d_sub_offsets[k] .. d_sub_offsets[k + 1]) (n_mems + 1 offsets).  Hits of sub-MEM i:
 * d_hits[d_hit_offsets[i] .. d_hit_offsets[i + 1]) (sub_capacity + 1 offsets), by the rules of gcsa2_mem_hits_device (hit_max,
 * over).  *total_subs and *total_hits are always the sizes needed; if either exceeds its capacity the call fails with
 * GCSA2_ERR_BUFFER_TOO_SMALL and writes nothing into d_sub_offsets, d_subs, d_hit_offsets or d_hits.  Nothing is ever written
 * behind a capacity.  GCSA2_ERR_INVALID_ARGUMENT, with nothing written: min_length 0, an unknown `over`, a MEM with
 * position + length beyond its pattern.  A walk that does not shorten its match (an inconsistent index) fails with
 * GCSA2_ERR_HIP instead of spinning: a walk is bounded at 2 l + 2 rounds.  Needs the LCP array, the samples and the counters
 * (GCSA2_ERR_MISSING_COMPONENT).  total_pattern_bytes is not needed (GCSA2_UNKNOWN is fine).  Fewer than 2^32 MEMs and
 * sub-MEMs per call.  Enqueued on `stream`, complete on return. */
int gcsa2_sub_mem_hits_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_queries,
                              uint64_t total_pattern_bytes, const uint64_t* d_mem_offsets, const gcsa2_mem* d_mems, uint64_t n_mems,
                              uint64_t min_length, uint64_t reseed_length, uint64_t hit_max, int over,
                              uint64_t* d_sub_offsets, gcsa2_mem* d_subs, uint64_t sub_capacity, uint64_t* total_subs,
                              uint64_t* d_hit_offsets, uint64_t* d_hits, uint64_t hit_capacity, uint64_t* total_hits, void* stream);
/* The same for a batch in host memory (offsets[0] == 0, mem_offsets[0] == 0, mem_offsets[n_queries] == n_mems or n_mems ==
 * GCSA2_UNKNOWN): copies in, runs, copies out, in one piece -- the patterns, the MEMs and buffers of both capacities must fit
 * in device memory at once.  Writes nothing on GCSA2_ERR_BUFFER_TOO_SMALL.  Complete on return. */
int gcsa2_sub_mem_hits_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_queries,
                             const uint64_t* mem_offsets, const gcsa2_mem* mems, uint64_t n_mems,
                             uint64_t min_length, uint64_t reseed_length, uint64_t hit_max, int over,
                             uint64_t* sub_offsets, gcsa2_mem* subs, uint64_t sub_capacity, uint64_t* total_subs,
                             uint64_t* hit_offsets, uint64_t* hits, uint64_t hit_capacity, uint64_t* total_hits);
/* ---- k-mer hits: the k-mers of every read that occur, as seeds with count() and their positions ----------------------------
 * What lies between gcsa2_kmer_windows_device (every window, found or not, 24 bytes each) and gcsa2_mem_hits_device (seeds
 * with hits, but MEMs): the found windows only, compacted, in read order, with count() and hits, in one call -- a k-mer
 * seeding mapper's or a genotyper's lookup.  (d_patterns, d_offsets, n_patterns), k and stride are those of
 * gcsa2_kmer_windows_device; hit_max and over those of gcsa2_mem_hits_device.
 *
 * DEFINITION.
 *   - The windows are exactly those of gcsa2_kmer_windows_device for (k, stride): window j of read q is P_q[j stride, j stride + k).
 *   - The seeds of read q are its windows with a non-empty range, in ascending window order:
 *     d_seeds[d_seed_offsets[q] .. d_seed_offsets[q + 1]) (n_patterns + 1 offsets; the last one is the total).
 *   - Each seed is the record { position = j stride (within the read), length = k, sp, ep, count }: (sp, ep) is bit for bit
 *     what gcsa2_find_device returns for that substring, count = GCSA::count(sp, ep).  A window with an empty range -- either
 *     empty form -- makes no record.
 *   - The record type is gcsa2_mem on purpose: a seed CSR is a valid input to gcsa2_sub_mem_hits_device and to everything else
 *     a caller has for MEMs.
 *   - Hits of seed i: d_hits[d_hit_offsets[i] .. d_hit_offsets[i + 1]) (seed_capacity + 1 offsets), by the rules of
 *     gcsa2_mem_hits_device, word for word: hit_max == 0 (no cap) or count <= hit_max: the sorted distinct values of
 *     gcsa2_locate_into(sort = 1); otherwise GCSA2_MEM_OVER_SKIP: none (the seed and its count are still reported), or
 *     GCSA2_MEM_OVER_SAMPLE: the values of gcsa2_locate_max(range, hit_max), value for value and in order; its
 *     INVALID_ARGUMENT for a range the reference would draw forever on is passed through.
 *   - d_profiles, if given (n_patterns entries), equals what gcsa2_kmer_windows_device returns with GCSA2_KMER_COUNTS.
 *
 * *total_seeds and *total_hits are always the sizes needed; if either exceeds its capacity the call fails with
 * GCSA2_ERR_BUFFER_TOO_SMALL and writes nothing into d_seeds, d_hit_offsets, d_hits or d_profiles (nor, as it stands, into
 * d_seed_offsets).  Nothing is ever written behind a capacity.  seed_capacity equal to the number of windows always suffices.
 * Limits and refusals are those of gcsa2_kmer_windows_device: 2^32 windows or reads, GCSA2_ERR_BUFFER_TOO_SMALL ("split the
 * batch"), nothing written.  GCSA2_ERR_INVALID_ARGUMENT, with nothing written and before any device is touched: k == 0,
 * stride == 0, an unknown `over`, a NULL index (or a NULL total pointer).  Needs the samples and the counters
 * (GCSA2_ERR_MISSING_COMPONENT, likewise); unlike MEM hits it does not need the LCP array.  n_patterns == 0, no window at all
 * and no found window are GCSA2_OK: the seed offsets are zeroed and d_hit_offsets[0] = 0.  d_seeds / d_hits may be NULL with a
 * capacity of 0 (a sizing call).  Enqueued on `stream`, complete on return.
 *
 * No per-window range or count buffer exists: the search kernel ranks the found lanes of a wavefront, reserves their records
 * with one atomic add and writes them in arrival order; a scan and a second small kernel put them into window order.  Device
 * scratch per call: the window offsets (and the profiles, if asked for) per read, 8 + 16 bytes per 64 windows, the rest per
 * seed.  A seed_capacity below *total_seeds makes the call search twice (the records are needed for *total_hits). */
int gcsa2_kmer_hits_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                           uint64_t k, uint64_t stride, uint64_t hit_max, int over,
                           gcsa2_kmer_profile* d_profiles,                 /* n_patterns, or NULL */
                           uint64_t* d_seed_offsets,                       /* n_patterns + 1 */
                           gcsa2_mem* d_seeds, uint64_t seed_capacity, uint64_t* total_seeds,
                           uint64_t* d_hit_offsets,                        /* seed_capacity + 1 */
                           uint64_t* d_hits, uint64_t hit_capacity, uint64_t* total_hits, void* stream);
/* The same for a batch in host memory: offsets[0] == 0, decreasing offsets are refused (GCSA2_ERR_INVALID_ARGUMENT).  A batch
 * of two pieces' worth of read bytes or more travels in pieces of whole reads (GCSA2_MS_PIECE_MB, GCSA2_MS_THREADS, as the MEM
 * calls); seeds, hit offsets and hits keep read order across pieces.  On GCSA2_ERR_BUFFER_TOO_SMALL a batch in one piece
 * writes nothing; one in pieces leaves the result arrays unspecified, as gcsa2_mem_hits_batch.  Complete on return. */
int gcsa2_kmer_hits_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                          uint64_t k, uint64_t stride, uint64_t hit_max, int over, gcsa2_kmer_profile* profiles,
                          uint64_t* seed_offsets, gcsa2_mem* seeds, uint64_t seed_capacity, uint64_t* total_seeds,
                          uint64_t* hit_offsets, uint64_t* hits, uint64_t hit_capacity, uint64_t* total_hits);
/* ---- minimizers: the sampled k-mers of every read, alone and as seeds with count() and their positions ----------------------
 * The k-mer calls above search every stride-th window, and a fixed stride is not shift-invariant: two reads over the same locus
 * at different offsets pick different k-mers, and an indel moves every later pick.  (w, k)-minimizers -- of every w
 * consecutive k-mers the one with the smallest hash -- are what k-mer seeders use instead: overlapping reads pick the same
 * k-mers, and about 2 / (w + 1) of the windows survive.  gcsa2_minimizers_device is the selection alone; it needs nothing of
 * the index but its alphabet (any image, with or without samples, counters or LCP array).  gcsa2_minimizer_hits_device is
 * gcsa2_kmer_hits_device with (w, hash_seed) in the place of stride: selection, search, count() and hits in one call.
 *
 * DEFINITION.  For read q = P of length L the windows are the stride-1 windows of gcsa2_kmer_windows_device: window j is
 * P[j, j + k) for 0 <= j < W, W = L - k + 1 (W = 0 if L < k).
 *   - Codes: code(c) = char2comp[c] - 1 if 1 <= char2comp[c] <= min(4, sigma - 2), else invalid.  A window is VALID if all its k
 *     characters have a code: with the default alphabet A, C, G, T and their lower-case forms; N, '$', '#' and unknown bytes
 *     make a window invalid.
 *   - key(j) = sum over i of code(P[j + i]) << 2 (k - 1 - i): the first character is the most significant, 2 k bits.
 *     hash(j) = mix64(key(j) ^ hash_seed), mix64 being the SplitMix64 finaliser on 64-bit wrapping arithmetic:
 *       z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *       return z ^ (z >> 31).
 *     mix64 is a bijection: distinct k-mers never tie.
 *   - Spans: of every maximal run [a, b) of consecutive valid windows, r = b - a: if r >= w the spans [s, s + w) for
 *     a <= s <= b - w; if 1 <= r < w the single span [a, b) -- a short read, or a short stretch between two Ns, still gets one
 *     minimizer.
 *   - Selection: each span selects its window with the smallest (hash, position): the leftmost wins a tie.  The minimizers of
 *     the read are the distinct selected windows in ascending position.  w == 1 selects every valid window.
 *
 * gcsa2_minimizers_device: d_min_offsets (n_patterns + 1 entries, the last one *total) is the CSR over reads, the records are
 * { position = j, hash = hash(j) }.  *total is always the number needed; above `capacity` the call returns
 * GCSA2_ERR_BUFFER_TOO_SMALL with the offsets complete and nothing written into the records.  d_minimizers == NULL with a
 * capacity of 0 is a sizing call.
 *
 * gcsa2_minimizer_hits_device: the contract of gcsa2_kmer_hits_device, word for word, over the selected windows instead of the
 * stride windows.  The seeds of a read are its minimizers with a non-empty find(), in ascending position, as { position,
 * length = k, sp, ep, count }, (sp, ep) bit for bit what gcsa2_find_device returns for the window; the hits follow the hit_max
 * / GCSA2_MEM_OVER_SKIP / GCSA2_MEM_OVER_SAMPLE rules of gcsa2_mem_hits_device; d_profiles[q] = { windows = the minimizers of
 * the read, found, nodes, occurrences } over those windows.  Capacities, sizing calls, "nothing written on refusal" and the
 * limits (fewer than 2^32 reads and fewer than 2^32 stride-1 windows per call) are those of gcsa2_kmer_hits_device; so is the
 * need for the samples and the counters (GCSA2_ERR_MISSING_COMPONENT) but not for the LCP array.
 *
 * GCSA2_ERR_INVALID_ARGUMENT, before any device is touched and with nothing written: k == 0 or k > GCSA2_MINIMIZER_MAX_K,
 * w == 0 or w > GCSA2_MINIMIZER_MAX_W, an unknown `over`, a NULL index or a NULL total pointer.  n_patterns == 0, no window, no
 * valid window and no found minimizer are GCSA2_OK: the offsets are zeroed (and d_hit_offsets[0] = 0).  No pattern byte outside
 * the 8-byte words that hold [d_offsets[0], d_offsets[n_patterns]) is read.  Enqueued on `stream`, complete on return.
 *
 * The selection is one wavefront per read in tiles of 64 spans: ballots pack the tile's characters into 2-bit code words and
 * a bad-character mask, a lane builds its key from two words, and the span minima come from a sparse table in LDS.  It runs
 * twice (count, scan, place).  The search is the kernel of gcsa2_kmer_hits_device over the list of selected positions.
 * Device scratch: per read 16 bytes, per minimizer 16 bytes, then that of gcsa2_kmer_hits_device with the minimizers as the windows.
 *
 * Canonical (both-strand) minimizers and their hits on both strands: gcsa2_hip_strands.h.
 * Out of scope: syncmers, w > 64, k > 32, and minimizer forms of the support and class calls. */
#define GCSA2_MINIMIZER_MAX_K 32
#define GCSA2_MINIMIZER_MAX_W 64
typedef struct gcsa2_minimizer { uint64_t position, hash; } gcsa2_minimizer;
int gcsa2_minimizers_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                            uint64_t k, uint64_t w, uint64_t hash_seed,
                            uint64_t* d_min_offsets,                       /* n_patterns + 1 */
                            gcsa2_minimizer* d_minimizers, uint64_t capacity, uint64_t* total, void* stream);
/* The same for a batch in host memory: offsets[0] == 0, decreasing offsets are refused (GCSA2_ERR_INVALID_ARGUMENT).  A batch
 * of two pieces' worth of read bytes or more travels in pieces of whole reads (GCSA2_MS_PIECE_MB, GCSA2_MS_THREADS); minimizers
 * are per read, so the result does not depend on the cut.  Complete on return. */
int gcsa2_minimizers_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                           uint64_t k, uint64_t w, uint64_t hash_seed, uint64_t* min_offsets, gcsa2_minimizer* minimizers,
                           uint64_t capacity, uint64_t* total);
int gcsa2_minimizer_hits_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                                uint64_t k, uint64_t w, uint64_t hash_seed, uint64_t hit_max, int over,
                                gcsa2_kmer_profile* d_profiles,            /* n_patterns, or NULL */
                                uint64_t* d_seed_offsets,                  /* n_patterns + 1 */
                                gcsa2_mem* d_seeds, uint64_t seed_capacity, uint64_t* total_seeds,
                                uint64_t* d_hit_offsets,                   /* seed_capacity + 1 */
                                uint64_t* d_hits, uint64_t hit_capacity, uint64_t* total_hits, void* stream);
/* The host form, as gcsa2_kmer_hits_batch: pieces of whole reads, read order kept; on GCSA2_ERR_BUFFER_TOO_SMALL a batch in
 * one piece writes nothing, one in pieces leaves the result arrays unspecified.  Complete on return. */
int gcsa2_minimizer_hits_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                               uint64_t k, uint64_t w, uint64_t hash_seed, uint64_t hit_max, int over, gcsa2_kmer_profile* profiles,
                               uint64_t* seed_offsets, gcsa2_mem* seeds, uint64_t seed_capacity, uint64_t* total_seeds,
                               uint64_t* hit_offsets, uint64_t* hits, uint64_t hit_capacity, uint64_t* total_hits);
/* ---- capped seeds: the shortest matches of every read that occur at most max_count times, with their positions -------------
 * A frequency-bounded seed (BWA-MEM's third seeding round, LAST's adaptive seeds): where a read crosses a repeat, MEMs and
 * k-mers end above hit_max and get no positions (GCSA2_MEM_OVER_SKIP) or a sample of them; here the match is extended until it
 * occurs at most max_count times, emitted, and the search starts again behind it.  No composition of the other calls gives
 * this: it needs count() of the range after every step.  (d_patterns, d_offsets, n_patterns) are those of gcsa2_find_device;
 * hit_max and over those of gcsa2_mem_hits_device.  min_length >= 1; max_length: 0 means none, a mapper passes gcsa2_order();
 * max_count >= 1.
 *
 * DEFINITION.  The seeds of read P of length L, over an index of n path nodes, are what this walk emits, in its order:
 *
 *   e = L
 *   while e > 0:
 *     r = (0, n - 1); i = e; fail = none                    r is the range of P[i .. e)
 *     loop:
 *       if i == 0: fail = -1; break                                              (the read's start)
 *       if max_length != 0 and e - i == max_length: fail = i - 1; break          (cut: the step is not taken)
 *       r2 = LF(r, char2comp[P[i - 1]])
 *       if r2 is empty: fail = i - 1; break
 *       i -= 1; r = r2
 *       if e - i >= min_length and count(r) <= max_count:
 *         emit {position = i, length = e - i, sp = r.sp, ep = r.ep, count = count(r)}; break
 *     e = i if a seed was emitted, else max(0, min(e - 1, fail + 1))
 *
 * What follows from it:
 *   - The seeds of a read do not overlap, and they come in descending position -- the order in which gcsa2_match_breaks_device
 *     lists its records.
 *   - count() is evaluated only once the match has min_length characters.
 *   - A walk takes at most 2 L LF steps: a failed attempt of s steps moves e by at least max(1, s - 1).
 *   - After a failure the next attempt ends with the character that failed (BWA's skip).  This is greedy on purpose: the
 *     contract is the walk itself, not "every shortest match under the cap".
 *   - Only non-empty ranges are emitted, so neither of find()'s empty forms appears.
 *   - A read shorter than min_length and an index of size 0 give no seed.
 *   - (sp, ep) of a seed is bit for bit what gcsa2_find_device returns for P[position, position + length); count =
 *     GCSA::count(sp, ep).  With max_length == 0 a length may exceed gcsa2_order(), with find()'s false positives.
 *   - The record type is gcsa2_mem, so that a seed CSR is a valid input to gcsa2_sub_mem_hits_device as it is.
 *
 * Seeds of read q: d_seeds[d_seed_offsets[q] .. d_seed_offsets[q + 1]) (n_patterns + 1 offsets; the last one is the total).
 * Hits of seed i: d_hits[d_hit_offsets[i] .. d_hit_offsets[i + 1]) (seed_capacity + 1 offsets), by the rules of
 * gcsa2_mem_hits_device, word for word: hit_max == 0 (no cap) or count <= hit_max: the sorted distinct values of
 * gcsa2_locate_into(sort = 1); otherwise GCSA2_MEM_OVER_SKIP: none (the seed and its count are still reported), or
 * GCSA2_MEM_OVER_SAMPLE: the values of gcsa2_locate_max(range, hit_max), value for value and in order; its INVALID_ARGUMENT for a
 * range the reference would draw forever on is passed through.  A caller who wants every seed placed passes hit_max = 0 or
 * hit_max >= max_count.
 *
 * *total_seeds and *total_hits are always the sizes needed; if either exceeds its capacity the call fails with
 * GCSA2_ERR_BUFFER_TOO_SMALL and writes nothing into d_seed_offsets, d_seeds, d_hit_offsets or d_hits.  Nothing is ever written
 * behind a capacity.  d_seeds / d_hits may be NULL with a capacity of 0 (a sizing call).  GCSA2_ERR_INVALID_ARGUMENT, with
 * nothing written and before any device is touched: min_length == 0, max_count == 0, max_length != 0 && min_length > max_length,
 * an unknown `over`, a NULL index or a NULL total pointer.  Needs the samples and the counters (GCSA2_ERR_MISSING_COMPONENT,
 * likewise); it does NOT need the LCP array -- the first seed finder with positions that works on an image created without one.
 * 2^32 or more reads or seeds: GCSA2_ERR_BUFFER_TOO_SMALL ("split the batch").  n_patterns == 0 and no seed at all are GCSA2_OK:
 * the seed offsets are zeroed and d_hit_offsets[0] = 0.  A walk that takes more than 2 L + 2 LF steps (an inconsistent index) fails
 * with GCSA2_ERR_HIP instead of spinning.  Enqueued on `stream`, complete on return.
 *
 * One lane per read, persistent lanes, two passes of the same walk (sizes, a scan, then the records at their slots): device
 * scratch per call is two words per read, the rest per seed.  The counts the walk computed go to the classify / locate / gather
 * tail of the MEM hits; count() is not evaluated twice.  Neither the seed table nor the jump table is read.  Where the image has
 * pair blocks, the steps of an attempt that is still two characters or more short of min_length -- whose ranges and counts the
 * walk does not look at -- go two per request when both are non-empty, and are replayed one by one when not, so that `fail`
 * is exact: the results are the same bit for bit with and without pair blocks. */
int gcsa2_capped_seeds_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                              uint64_t min_length, uint64_t max_length, uint64_t max_count, uint64_t hit_max, int over,
                              uint64_t* d_seed_offsets,                    /* n_patterns + 1 */
                              gcsa2_mem* d_seeds, uint64_t seed_capacity, uint64_t* total_seeds,
                              uint64_t* d_hit_offsets,                     /* seed_capacity + 1 */
                              uint64_t* d_hits, uint64_t hit_capacity, uint64_t* total_hits, void* stream);
/* The same for a batch in host memory: offsets[0] == 0, decreasing offsets are refused (GCSA2_ERR_INVALID_ARGUMENT).  A batch
 * of two pieces' worth of read bytes or more travels in pieces of whole reads (GCSA2_MS_PIECE_MB, GCSA2_MS_THREADS, as the MEM
 * calls); seeds, hit offsets and hits keep read order across pieces.  On GCSA2_ERR_BUFFER_TOO_SMALL a batch in one piece
 * writes nothing; one in pieces leaves the result arrays unspecified, as gcsa2_mem_hits_batch.  Complete on return. */
int gcsa2_capped_seeds_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                             uint64_t min_length, uint64_t max_length, uint64_t max_count, uint64_t hit_max, int over,
                             uint64_t* seed_offsets, gcsa2_mem* seeds, uint64_t seed_capacity, uint64_t* total_seeds,
                             uint64_t* hit_offsets, uint64_t* hits, uint64_t hit_capacity, uint64_t* total_hits);
/* ---- k-mer support: the k-mers of every read (or any seed records), summed per graph node -----------------------------------
 * The call of the second caller named under k-mer windows and k-mer hits: a k-mer genotyper or a coverage screen wants no seed
 * lists but, per graph node, how many read k-mers landed on it, summed over all reads.  With gcsa2_kmer_hits_batch it would
 * pull every hit of every window across the link and bin them itself; here find, count, locate and the binning stay on the
 * device, every distinct range of a call is located ONCE however many reads carry its k-mer, and what leaves the device is one
 * counter per bin.  (d_patterns, d_offsets, n_patterns), k and stride are those of gcsa2_kmer_windows_device.
 *
 * DEFINITION.
 *   - The windows are exactly those of gcsa2_kmer_windows_device for (k, stride).  A window is FOUND if its find() range is
 *     non-empty.
 *   - A found window is COUNTED if hit_max == 0 or count(range) <= hit_max: the GCSA2_MEM_OVER_SKIP rule of the MEM hits.  There
 *     is no sampling policy here: a random sample has no place in a sum.  (A seed record whose range reaches beyond the index
 *     has count() == 0, GCSA::count's answer, and is not counted: there is nothing to locate.)
 *   - A counted window of weight w (1 for k-mer windows) adds w to d_support[v >> shift] for every value v of
 *     gcsa2_locate_into(range, sort = 1), the sorted distinct values.  With GCSA2_SUPPORT_PER_BIN it adds w once per distinct
 *     v >> shift among those values.
 *   - shift = 11 (Node::ID_OFFSET) gives node ids, shift = 0 exact positions.
 *   - A contribution whose bin is >= n_bins is not written anywhere; its weight goes to stats.dropped.
 *   - The call ADDS and never zeroes: support accumulates over calls, and the caller clears it.
 *   - stats (host, may be NULL): windows and found as in the profiles of gcsa2_kmer_windows_device, summed over the reads;
 *     counted as above; distinct = the number of distinct (sp, ep) among the counted windows; values = the sum over those
 *     distinct ranges of the number of their distinct located values; added = the total weight added to d_support; dropped as
 *     above.  Without GCSA2_SUPPORT_PER_BIN and with weights 1, added + dropped is the sum over the counted windows of
 *     |locate(range)|.
 *
 * GCSA2_ERR_INVALID_ARGUMENT, with nothing written (stats included) and before any device is touched: a NULL index, k == 0,
 * stride == 0, shift >= 64, an unknown flag, d_support == NULL with n_bins > 0.  n_bins == 0 is valid: everything is dropped, a
 * statistics run.  Needs the samples and the counters (GCSA2_ERR_MISSING_COMPONENT, likewise), not the LCP array.  2^32 or more
 * reads, windows or seeds: GCSA2_ERR_BUFFER_TOO_SMALL ("split the batch"), as gcsa2_kmer_hits_device.  n_patterns == 0, no window
 * and nothing found are GCSA2_OK with zero stats (but `windows`).  The sum is NOT transactional: on an error after work has begun
 * d_support may hold a partial sum, and stats is not written.  Enqueued on `stream`, complete on return.
 *
 * The search is that of gcsa2_kmer_hits_device; its records stay in arrival order -- no window order, no seed offsets, no
 * profiles.  The cap is applied first, the counted records are sorted by (sp, ep), runs become {range, multiplicity}, and the
 * distinct ranges are located in chunks whose count() sum stays within a value budget (a chunk always holds one range at
 * least), so that device scratch does not grow with the call's total hits; every chunk's values are added with 64-bit vector
 * atomics, neighbouring lanes of one bin as one add.  GCSA2_SUPPORT_CHUNK (values, read per call; default 2^22, the smallest
 * budget within 2.5 % of the best time measured, profiles/kmer_support.md) is a test knob: no result depends on it. */
typedef struct gcsa2_support_stats { uint64_t windows, found, counted, distinct, values, added, dropped; } gcsa2_support_stats;
#define GCSA2_SUPPORT_PER_BIN 1   /* a window adds to a bin once, however many of its positions fall into it */
int gcsa2_kmer_support_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                              uint64_t k, uint64_t stride, uint64_t hit_max, uint64_t shift, int flags,
                              uint64_t* d_support, uint64_t n_bins, gcsa2_support_stats* stats /* host, may be NULL */, void* stream);
/* The same for reads in host memory, into a host array: offsets[0] == 0, decreasing offsets are refused
 * (GCSA2_ERR_INVALID_ARGUMENT).  A batch of two pieces' worth of read bytes or more travels in pieces of whole reads
 * (GCSA2_MS_PIECE_MB, GCSA2_MS_THREADS, as the MEM calls).  One zeroed device array of n_bins serves the whole call and is added
 * into `support` at the end (on an error `support` is untouched).  stats are summed over the pieces: distinct and values are then
 * per-piece sums, an upper bound of the whole-batch figures; everything else is exact.  Complete on return. */
int gcsa2_kmer_support_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                             uint64_t k, uint64_t stride, uint64_t hit_max, uint64_t shift, int flags,
                             uint64_t* support /* host, n_bins */, uint64_t n_bins, gcsa2_support_stats* stats);
/* The same sum over seed records the caller already has on the device -- MEMs, sub-MEMs, k-mer or capped seeds, as the other
 * calls emit them -- with a weight per record (d_weights, n_seeds entries, or NULL = 1 each; 0 is allowed).  Only sp and ep of a
 * record are read: count() is evaluated again and the record's count field is ignored.  A record with an empty range (either
 * form) contributes nothing.  stats.windows = n_seeds, stats.found = the records with a non-empty range; a run's multiplicity
 * is the sum of its records' weights.  n_seeds == 0 is GCSA2_OK.  Refusals, limits and everything else as above. */
int gcsa2_seed_support_device(const gcsa2_index* index, const gcsa2_mem* d_seeds, uint64_t n_seeds,
                              const uint64_t* d_weights /* or NULL = 1 each */, uint64_t hit_max, uint64_t shift, int flags,
                              uint64_t* d_support, uint64_t n_bins, gcsa2_support_stats* stats, void* stream);
/* ---- index k-mer spectrum: the k-mers of the INDEX, binned by occurrence, listed, or summed per graph node -------------------
 * Every read-side call above takes a threshold that is a property of the index, not of the reads: hit_max of the MEM, k-mer
 * and capped-seed hits, max_count of the capped seeds, the hit_max cap of k-mer support, classes and top classes.  These three
 * calls are what a caller chooses them by.  They share one walk of the search tree of countKMers (src/algorithms.cpp:364-421).
 *
 * DEFINITION.
 *   - K(k, include_ns) is the multiset of states at depth k of that tree: the root is (0, size() - 1); the children of a state
 *     are LF_fast(range) (comps 1 .. fast_chars) when include_ns == 0, LF_all(range) (comps 1 .. sigma - 2) otherwise; only
 *     non-empty children survive.  There is one state per distinct k-mer.  Distinct k-mers need NOT have distinct ranges: a
 *     path node whose label is shorter than k starts several k-mers, and all of them end in its range.
 *   - Every state carries its key in the packing of gcsa2_compare_kmers_records: the comp of extension step i at bits
 *     [3i, 3i + 3) of kmer[3], step 0 being the LAST character of the k-mer.
 *   - value(state) = GCSA::count(range) with GCSA2_SPECTRUM_COUNTS, Range::length(range) without it; count() is then never
 *     evaluated, and the call works on an image without counters.
 *
 * gcsa2_kmer_spectrum: histogram (host, n_hist words, or NULL with n_hist == 0) is OVERWRITTEN: histogram[min(value, n_hist - 1)]
 * is the number of states of K with that value, so the last bin collects everything at or above it and the bins sum to
 * stats.kmers.  stats (host, may be NULL): kmers = |K| = gcsa2_count_kmers for the same (k, include_ns, force); nodes = the sum
 * of Range::length; occurrences = the sum of count(), 0 without GCSA2_SPECTRUM_COUNTS (as in the k-mer windows profile);
 * unique = the states of value 1; max_value = the largest value.
 *
 * gcsa2_list_kmers: records (host) receives the states with min_value <= value and (max_value == 0 or value <= max_value), in
 * no specified order; `count` is 0 without GCSA2_SPECTRUM_COUNTS, `nodes` is Range::length.  *total is always the number
 * needed.  If it exceeds capacity the call fails with GCSA2_ERR_BUFFER_TOO_SMALL; nothing is ever written behind capacity, and
 * what lies before it is unspecified.  records == NULL with capacity == 0 is a sizing call.
 *
 * gcsa2_index_kmer_support_device: by composition, the records {position 0, length k, sp, ep} of K, weight 1 each, piece of
 * the walk by piece, through the core of gcsa2_seed_support_device.  It ADDS and never zeroes.  d_support, windows, found,
 * counted, added and dropped are exact, and windows == found == the stats.kmers of gcsa2_kmer_spectrum; distinct and values are
 * per-piece sums -- equal ranges fold within a piece only -- exact when the walk is one piece and upper bounds otherwise, the
 * rule of gcsa2_kmer_support_batch (which states share a piece depends on the arrival order of the levels above, so these two
 * figures may differ from run to run when there are several pieces).  d_support[node] over the k-mers with count() <= hit_max is the denominator of
 * gcsa2_kmer_support_device's per-node sums: the k-mers a node can be seen by under the same cap.  Needs the samples and the
 * counters.  Enqueued on `stream`, complete on return; not transactional, as gcsa2_kmer_support_device.
 *
 * All three: k > order() without force, or an index of size 0, is GCSA2_OK with every output zero, as countKMers.
 * GCSA2_ERR_INVALID_ARGUMENT, with nothing written and before any device is touched: a NULL index, k == 0, an unknown flag,
 * sigma < 3, histogram == NULL with n_hist > 0, min_value > max_value != 0, k > 64 for the list (the key holds 64 steps),
 * records == NULL with capacity > 0, shift >= 64, d_support == NULL with n_bins > 0, a NULL total.  GCSA2_ERR_MISSING_COMPONENT,
 * likewise: GCSA2_SPECTRUM_COUNTS on an image without counters; support on an image without samples or counters.
 *
 * The walk is depth-first over pieces of the frontier (GCSA2_KMER_PIECE, as gcsa2_count_kmers): no result but distinct and
 * values depends on the cut.  The histogram call never stores the last level; the other two cut it so that a piece holds at
 * most 2^24 records.  GCSA2_SPECTRUM_GROUPS (workgroups of the last level's kernel, read per call; default 12 per compute unit)
 * is a test knob: no result depends on it.  profiles/kmer_spectrum.md. */
#define GCSA2_SPECTRUM_COUNTS 1   /* value = count(range), not Range::length(range) */
typedef struct gcsa2_spectrum_stats { uint64_t kmers, nodes, occurrences, unique, max_value; } gcsa2_spectrum_stats;
typedef struct gcsa2_index_kmer { uint64_t sp, ep, count, nodes, k, kmer[3]; } gcsa2_index_kmer;   /* 64 bytes */
int gcsa2_kmer_spectrum(const gcsa2_index* index, uint64_t k, int include_ns, int force, int flags,
                        uint64_t* histogram /* host, n_hist, or NULL */, uint64_t n_hist,
                        gcsa2_spectrum_stats* stats /* host, or NULL */);
int gcsa2_list_kmers(const gcsa2_index* index, uint64_t k, int include_ns, int force, int flags,
                     uint64_t min_value, uint64_t max_value /* 0 = none */,
                     gcsa2_index_kmer* records /* host */, uint64_t capacity, uint64_t* total);
int gcsa2_index_kmer_support_device(const gcsa2_index* index, uint64_t k, int include_ns, int force,
                                    uint64_t hit_max, uint64_t shift, int flags /* GCSA2_SUPPORT_PER_BIN */,
                                    uint64_t* d_support, uint64_t n_bins, gcsa2_support_stats* stats, void* stream);
/* ---- k-mer classes: per read, the votes of its k-mers (or any seed records) over classes of graph nodes -----------------------
 * The transpose of k-mer support, for a read classifier or binner: per READ, on which class of graph nodes -- chromosome,
 * contig, subgraph, host or contaminant -- do its k-mers land?  With gcsa2_kmer_hits_batch the caller would pull every hit of
 * every window across the link, map hit >> shift through its node -> class table, remove duplicate classes per window and
 * scatter-add into a reads x classes matrix; here the search, the fold of equal ranges and the locate of every distinct range
 * (ONCE, however many reads carry its k-mer) are those of k-mer support, and what leaves the device is one row of n_classes
 * counters per read, or only the call.  (d_patterns, d_offsets, n_patterns), k and stride are those of gcsa2_kmer_windows_device.
 *
 * DEFINITION.
 *   - The windows, FOUND and COUNTED are exactly those of gcsa2_kmer_support_device for (k, stride, hit_max): a found window is
 *     counted if hit_max == 0 or count(range) <= hit_max; a range with count() == 0 is not counted; there is no sampling.
 *   - class(v) of a located value v: b = v >> shift (unsigned); if b < n_bins and d_class_of_bin[b] < n_classes it is
 *     d_class_of_bin[b], otherwise v has NO CLASS: GCSA2_CLASS_NONE, any id >= n_classes and a bin beyond the map mean the same.
 *   - Per range R with V(R) = the sorted distinct values of gcsa2_locate_into(R, sort = 1): n_c(R) = the values of V(R) with
 *     class c, none(R) = those without a class, classes(R) = the number of classes with n_c(R) > 0.
 *   - A counted record of weight w (1 for k-mer windows) and range R adds x_c to votes[q][c] of its read or group q: by default
 *     x_c = w n_c(R); with GCSA2_CLASS_PER_WINDOW x_c = w for every c with n_c(R) > 0; with GCSA2_CLASS_UNAMBIGUOUS x_c = 0 for
 *     all c unless classes(R) == 1.  Sums are taken in 64-bit arithmetic.
 *   - Rows are WRITTEN, not added to: the call writes every entry of d_votes[0 .. n_patterns n_classes) (row-major) and of
 *     d_calls[0 .. n_patterns), and nothing behind them.
 *   - call(q): total = the row's sum; best = the class with the most votes, the lowest id on a tie, or GCSA2_UNKNOWN (with
 *     best_votes = 0) when no class has a vote; second = the class with the most votes among the others that has at least one
 *     vote, the lowest id on a tie, or GCSA2_UNKNOWN with second_votes = 0 when there is none; counted = the number of counted
 *     records of q, unweighted.
 *   - stats (host, may be NULL): windows, found, counted, distinct and values as in gcsa2_support_stats; votes = the sum of all
 *     row totals; unclassified = the sum of none(R) over the counted records, unweighted; ambiguous = the number of counted
 *     records with classes(R) >= 2 -- with and without GCSA2_CLASS_UNAMBIGUOUS; with it these are the records that did not vote.
 *   - d_votes, d_calls and stats may each be NULL; all three NULL is valid and does the work.  Without d_votes the matrix does
 *     not exist in device memory either: a row lives in on-chip memory while its read is summed.
 *
 * GCSA2_ERR_INVALID_ARGUMENT, with nothing written (stats included) and before any device is touched: a NULL index, k == 0,
 * stride == 0, shift >= 64, an unknown flag, n_classes == 0 or n_classes > GCSA2_CLASS_LIMIT, d_class_of_bin == NULL with
 * n_bins > 0.  n_bins == 0 is valid: everything is unclassified.  Needs the samples and the counters
 * (GCSA2_ERR_MISSING_COMPONENT, likewise), not the LCP array.  2^32 or more reads, windows, groups or seeds:
 * GCSA2_ERR_BUFFER_TOO_SMALL ("split the batch"); likewise a single counted range with 2^31 or more values (set hit_max).
 * n_patterns == 0 or n_groups == 0 is GCSA2_OK with zero stats.  On an error
 * after work has begun rows and calls are unspecified and stats is not written.  Enqueued on `stream`, complete on return.
 *
 * The records of the search stay where they arrived; a read finds the record of a window through the 16 bytes that every
 * wavefront of the search leaves.  The cap, the sorts, the runs and the chunks (GCSA2_SUPPORT_CHUNK) are those of k-mer
 * support.  Every chunk's values become keys (run, class) that are sorted and run-length encoded into the runs' signatures --
 * equal classes are NOT neighbours in value order -- which are kept for all runs: scratch of 8 bytes per located value of the
 * distinct ranges, not per hit.  Then one wavefront per read adds its records' signatures into n_classes 64-bit counters in
 * LDS (at most 32 KB), stores the row with plain stores and reduces best and second: no global atomic but three per workgroup
 * for the stats. */
#define GCSA2_CLASS_NONE        0xFFFFFFFFu   /* a bin without a class */
#define GCSA2_CLASS_LIMIT       4096          /* n_classes may be 1 .. GCSA2_CLASS_LIMIT */
#define GCSA2_CLASS_PER_WINDOW  1   /* a record votes once per class, however many of its values fall into it */
#define GCSA2_CLASS_UNAMBIGUOUS 2   /* only records whose values fall into exactly one class vote */
typedef struct gcsa2_class_call  { uint64_t best, best_votes, second, second_votes, total, counted; } gcsa2_class_call;
typedef struct gcsa2_class_stats { uint64_t windows, found, counted, distinct, values, votes, unclassified, ambiguous; } gcsa2_class_stats;
int gcsa2_kmer_classes_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                              uint64_t k, uint64_t stride, uint64_t hit_max, uint64_t shift, int flags,
                              const uint32_t* d_class_of_bin, uint64_t n_bins, uint64_t n_classes,
                              uint64_t* d_votes /* n_patterns x n_classes, row-major, or NULL */,
                              gcsa2_class_call* d_calls /* n_patterns, or NULL */,
                              gcsa2_class_stats* stats /* host, may be NULL */, void* stream);
/* The same for reads and the class map in host memory, into host arrays: offsets[0] == 0, decreasing offsets are refused
 * (GCSA2_ERR_INVALID_ARGUMENT).  A batch of two pieces' worth of read bytes or more travels in pieces of whole reads
 * (GCSA2_MS_PIECE_MB, GCSA2_MS_THREADS, as the MEM calls); the class map is uploaded once per call.  Rows and calls are exact
 * whatever the pieces (a row belongs to one read); stats are summed over the pieces: distinct and values are then per-piece
 * sums, an upper bound of the whole-batch figures.  On an error votes and calls may be partly written.  Complete on return. */
int gcsa2_kmer_classes_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                             uint64_t k, uint64_t stride, uint64_t hit_max, uint64_t shift, int flags,
                             const uint32_t* class_of_bin, uint64_t n_bins, uint64_t n_classes,
                             uint64_t* votes /* host, n_patterns x n_classes, or NULL */, gcsa2_class_call* calls /* host, or NULL */,
                             gcsa2_class_stats* stats);
/* The same votes over seed records the caller already has on the device, in groups: group g owns the records
 * [d_group_offsets[g], d_group_offsets[g + 1]) -- the seed CSRs that the MEM hits, k-mer hits and capped seeds emit, as they
 * are -- with a weight per record (d_weights, n_seeds entries, or NULL = 1 each; 0 is allowed).  Only sp and ep of a record are
 * read: count() is evaluated again.  A record with an empty range (either form) contributes nothing.  A group whose offsets
 * decrease or reach beyond n_seeds is NOT READ: its row is zero and its call {GCSA2_UNKNOWN, 0, GCSA2_UNKNOWN, 0, 0, 0} -- the
 * rule of gcsa2_extend_device for an invalid state, so that no read-back is needed to refuse it and a bad cursor cannot fault.
 * stats.windows = n_seeds; found, counted, distinct and values are taken over all n_seeds records, as gcsa2_seed_support_device
 * does; votes, unclassified and ambiguous over the records as their groups own them (the same thing when the groups are a
 * CSR over the records).  n_groups == 0 is GCSA2_OK with zero stats; d_group_offsets == NULL with n_groups > 0 and d_seeds ==
 * NULL with n_seeds > 0 are GCSA2_ERR_INVALID_ARGUMENT.  Refusals, limits and everything else as above. */
int gcsa2_seed_classes_device(const gcsa2_index* index, const uint64_t* d_group_offsets, uint64_t n_groups,
                              const gcsa2_mem* d_seeds, uint64_t n_seeds, const uint64_t* d_weights /* or NULL = 1 each */,
                              uint64_t hit_max, uint64_t shift, int flags, const uint32_t* d_class_of_bin, uint64_t n_bins,
                              uint64_t n_classes, uint64_t* d_votes, gcsa2_class_call* d_calls, gcsa2_class_stats* stats, void* stream);
/* ---- k-mer top classes: the sparse form of k-mer classes, for any number of classes ---------------------------------------------
 * A metagenomic binner votes over 10^5 contigs, a taxonomic classifier over 10^4 to 10^5 taxa, a pangenome user over every node:
 * far beyond GCSA2_CLASS_LIMIT, and a dense row per read does not scale.  What leaves the device here is, per read, the top_n
 * classes with the most votes and a summary of the row -- no matrix, no hit list.
 *
 * DEFINITION.
 *   - The windows, FOUND, COUNTED, class(v), n_c(R), none(R), classes(R) and the vote x_c of a counted record are exactly those
 *     of gcsa2_kmer_classes_device; GCSA2_CLASS_PER_WINDOW and GCSA2_CLASS_UNAMBIGUOUS mean the same; votes[q][c] is the same
 *     64-bit sum.  The only difference: n_classes may be 1 .. 0xFFFFFFFF.  Class ids are < n_classes; GCSA2_CLASS_NONE and any
 *     id >= n_classes mean "no class", as before.
 *   - summary(q): voted = the number of classes c with votes[q][c] > 0 (a class whose records all have weight 0 has no vote and
 *     is not voted); total = the row's sum; counted = the number of counted records of q, unweighted.
 *   - The top row: order the voted classes by more votes first, the lower id on a tie.  d_top[q top_n + j] for
 *     j < min(top_n, voted(q)) is the j-th class in that order with its votes; every later entry of the row is
 *     {GCSA2_UNKNOWN, 0}.
 *   - Rows and summaries are WRITTEN, not added to: the call writes every entry of d_top[0 .. n_patterns top_n) and of
 *     d_summaries[0 .. n_patterns), and nothing behind them.
 *   - stats is gcsa2_class_stats, every field as for gcsa2_kmer_classes_device.
 *   - d_top, d_summaries and stats may each be NULL; all three NULL is valid and does the work.
 *   - LAW: for n_classes <= GCSA2_CLASS_LIMIT and equal arguments, d_top[q][0] = {best, best_votes} and d_top[q][1] = {second,
 *     second_votes} of gcsa2_kmer_classes_device (gcsa2_seed_classes_device for the seed form), total, counted and every field
 *     of stats are equal, and the whole top row is the sorted non-zero entries of the dense row.
 *
 * GCSA2_ERR_INVALID_ARGUMENT, with nothing written (stats included) and before any device is touched: the refusals of
 * gcsa2_kmer_classes_device with the bound on n_classes replaced by n_classes == 0 or n_classes > 0xFFFFFFFF, and top_n == 0 or
 * top_n > GCSA2_TOP_LIMIT.  Missing components, the 2^32 limits, the limit of 2^31 values per range, n_bins == 0,
 * n_patterns == 0 and "enqueued on `stream`, complete on return" are those of gcsa2_kmer_classes_device.
 *
 * The search, the cap, the fold, the chunks (GCSA2_SUPPORT_CHUNK) and the locate are those of k-mer classes; the keys are
 * run << 33 | class with "no class" = 2^32, the signature entries n_c << 32 | class.  Then one wavefront per read adds its
 * records' signatures into a hash table in LDS (32-bit key, 64-bit counter, open addressing) and keeps the top row in its
 * registers.  A read that votes for more classes than the table holds is processed again in 2, 4, ... passes over a partition
 * of the class ids by hash, whose top rows merge and whose voted and total add up: the result is exact whatever the number of
 * classes.  GCSA2_TOP_SLOTS (a test knob, read per call; a power of two, 64 .. 4096, default 512) is the table's size; no
 * result depends on it.  No global atomic but three per workgroup for the stats. */
#define GCSA2_TOP_LIMIT 64                       /* top_n may be 1 .. GCSA2_TOP_LIMIT */
typedef struct gcsa2_class_vote  { uint64_t class_id, votes; } gcsa2_class_vote;
typedef struct gcsa2_top_summary { uint64_t voted, total, counted; } gcsa2_top_summary;
int gcsa2_kmer_top_classes_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                                  uint64_t k, uint64_t stride, uint64_t hit_max, uint64_t shift, int flags,
                                  const uint32_t* d_class_of_bin, uint64_t n_bins, uint64_t n_classes, uint64_t top_n,
                                  gcsa2_class_vote* d_top /* n_patterns x top_n, row-major, or NULL */,
                                  gcsa2_top_summary* d_summaries /* n_patterns, or NULL */,
                                  gcsa2_class_stats* stats /* host, may be NULL */, void* stream);
/* The same for reads and the class map in host memory, into host arrays: pieces, the map upload, the refusal of offsets that
 * do not start at 0 or decrease, and stats summed over the pieces are exactly those of gcsa2_kmer_classes_batch. */
int gcsa2_kmer_top_classes_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                                 uint64_t k, uint64_t stride, uint64_t hit_max, uint64_t shift, int flags,
                                 const uint32_t* class_of_bin, uint64_t n_bins, uint64_t n_classes, uint64_t top_n,
                                 gcsa2_class_vote* top /* host, n_patterns x top_n, or NULL */,
                                 gcsa2_top_summary* summaries /* host, or NULL */, gcsa2_class_stats* stats);
/* The same over seed records in groups: groups, weights, invalid groups and what stats counts are exactly those of
 * gcsa2_seed_classes_device.  An invalid group is NOT READ: its row is all {GCSA2_UNKNOWN, 0} and its summary is zero. */
int gcsa2_seed_top_classes_device(const gcsa2_index* index, const uint64_t* d_group_offsets, uint64_t n_groups,
                                  const gcsa2_mem* d_seeds, uint64_t n_seeds, const uint64_t* d_weights /* or NULL = 1 each */,
                                  uint64_t hit_max, uint64_t shift, int flags, const uint32_t* d_class_of_bin, uint64_t n_bins,
                                  uint64_t n_classes, uint64_t top_n, gcsa2_class_vote* d_top, gcsa2_top_summary* d_summaries,
                                  gcsa2_class_stats* stats, void* stream);
/* ---- seed clusters: per read the top diagonal bands of its seed hits -----------------------------------------------------------
 * Where does the read go, and do its seeds agree?  A mapper groups the hits of a read's seeds into collinear clusters by anchor
 * diagonal (reference coordinate minus read position) before it chains or extends anything.  The hits calls above return the
 * whole hit CSR, which has no per-read size bound; here the hits stay on the device and what leaves is, per read (or group of
 * seed records), the top_n clusters of 64 bytes each and a summary.  The geometry is the caller's: a map from bins of located
 * values to coordinates.
 *
 * DEFINITION (gcsa2_seed_clusters_device).
 *   - Inputs: a seed CSR, hit offsets and hits exactly as every hits call emits them (gcsa2_kmer_hits_device,
 *     gcsa2_minimizer_hits_device, gcsa2_mem_hits_device, gcsa2_sub_mem_hits_device, gcsa2_capped_seeds_device); a seed-offset
 *     array serves as d_group_offsets (n_groups + 1 entries).  Of a seed only `position` and `length` are read.  d_hit_offsets
 *     has n_seeds + 1 entries, d_hits n_hits.
 *   - ANCHORS of group g: every pair (seed i of the group, hit v = d_hits[h]) with h in [d_hit_offsets[i], d_hit_offsets[i + 1]).
 *     Anchors are a multiset: GCSA2_MEM_OVER_SAMPLE hit lists may repeat a value.
 *   - Placement: bin = v >> shift.  The anchor is UNPLACED if bin >= n_bins, if d_coord_of_bin[bin] == GCSA2_UNKNOWN, or if
 *     position >= 2^32, length >= 2^32 or position + length >= 2^32.  Otherwise x = d_coord_of_bin[bin] + (v & (2^shift - 1))
 *     and diag = x - position, both in 64-bit wrapping arithmetic; diagonals are ordered as SIGNED 64-bit integers.
 *     Node values are id << 11 | rc << 10 | offset: shift = 10 gives one coordinate per oriented node, shift = 11 one per node,
 *     shift = 0 one per value.
 *   - Clusters of a group: sort the placed anchors by diag; a new cluster starts wherever the unsigned difference between two
 *     sorted neighbours exceeds `band`.  band = 0 gives exact diagonals, band = 2^64 - 1 one cluster.
 *   - The record of a cluster: diag_min, diag_max = its extreme diagonals (signed order); anchors = the number of its anchors;
 *     starts = the number of distinct seed positions; covered = the size of the union of [position, position + length) over its
 *     anchors (the read bases it explains); read_begin = the smallest position; read_end = the largest position + length;
 *     ref_begin = the unsigned minimum of x.
 *   - The top row: order the clusters by larger covered first, then larger anchors, then smaller diag_min (signed): a total
 *     order within a group.  d_top[g top_n + j] for j < min(top_n, clusters) is the j-th cluster; every later entry of the row
 *     is all zero (anchors == 0 marks an empty entry).
 *   - summary(g) = { anchors = the placed anchors, unplaced = the others, clusters = the clusters of the group }.
 *   - Rows and summaries are WRITTEN, not added to: the call writes every entry of d_top[0 .. n_groups top_n) and of
 *     d_summaries[0 .. n_groups), and nothing behind them.
 *   - INVALID groups: one whose group offsets decrease or reach beyond n_seeds, or whose hit offsets over its seeds
 *     (d_hit_offsets[first .. last]) decrease or reach beyond n_hits, is NOT READ any further -- no seed and no hit of it is
 *     touched --; its row and summary are zero and it counts in stats.invalid_groups (the rule of gcsa2_seed_classes_device).
 *     A group without a seed reads no hit offset and is valid.
 *   - stats: groups = n_groups; seeds, anchors, unplaced, clusters = the sums over the valid groups; spilled = the number of
 *     groups that took the large path (below), the only field that may depend on GCSA2_CLUSTER_LDS.
 *   - d_top, d_summaries and stats may each be NULL; all three NULL is valid and does the work.
 *
 * GCSA2_ERR_INVALID_ARGUMENT, before any device is touched, with nothing written and stats untouched: a NULL index, top_n == 0
 * or top_n > GCSA2_CLUSTER_TOP_LIMIT, shift >= 64, n_bins == 0 or a NULL map, NULL d_group_offsets with n_groups > 0, NULL
 * d_seeds or d_hit_offsets with n_seeds > 0, NULL d_hits with n_hits > 0, and n_groups, n_seeds or n_hits >= 2^32.
 * n_groups == 0 is GCSA2_OK with zero stats.  The call needs no component of the image (no samples, counters or LCP array).
 * Enqueued on `stream`, complete on return.
 *
 * The fused forms gcsa2_kmer_clusters_device and gcsa2_minimizer_clusters_device: the hits never leave the device.  LAW: their
 * rows, summaries and stats equal gcsa2_kmer_hits_device (gcsa2_minimizer_hits_device) with the same arguments into large
 * enough buffers followed by gcsa2_seed_clusters_device with the seed offsets as the groups, word for word.  Refusals, limits
 * and missing components (samples and counters) are those of the hits call plus those above.  They run the hits call's own
 * core into scratch of the call and then the cluster core: there is no second search kernel.
 *
 * One workgroup owns a group of up to 4096 anchors, 32 bytes of LDS per anchor: a single wavefront for a group of up to 256
 * anchors (8 KiB at most, so a CU holds sixteen and more of them), 256 lanes above (the launch takes what the largest group of
 * the call needs, 128 KiB at the capacity).  It packs the placed anchors into
 * LDS, sorts them by diagonal (bitonic), marks the cluster heads, sorts again by (cluster, position), sums covered and starts
 * along the running end, and keeps the top row in the registers of one wavefront.  Groups above the capacity take the LARGE
 * path -- the same steps device-wide with hipCUB radix sorts and scans, then the same scoring code over global memory --, exact
 * for any number of anchors.  GCSA2_CLUSTER_LDS (a test knob, read per call; a power of two, 64 .. 4096, anything else is
 * ignored) sets the capacity; no result but stats.spilled depends on it.  Global atomics serve the stats only. */
#define GCSA2_CLUSTER_TOP_LIMIT 64               /* top_n may be 1 .. GCSA2_CLUSTER_TOP_LIMIT */
typedef struct gcsa2_cluster { uint64_t diag_min, diag_max, anchors, starts, covered, read_begin, read_end, ref_begin; } gcsa2_cluster;
typedef struct gcsa2_cluster_summary { uint64_t anchors, unplaced, clusters; } gcsa2_cluster_summary;
typedef struct gcsa2_cluster_stats { uint64_t groups, invalid_groups, seeds, anchors, unplaced, clusters, spilled; } gcsa2_cluster_stats;
int gcsa2_seed_clusters_device(const gcsa2_index* index, const uint64_t* d_group_offsets, uint64_t n_groups /* n_groups + 1 offsets */,
                               const gcsa2_mem* d_seeds, uint64_t n_seeds,
                               const uint64_t* d_hit_offsets /* n_seeds + 1 */, const uint64_t* d_hits, uint64_t n_hits,
                               uint64_t shift, const uint64_t* d_coord_of_bin, uint64_t n_bins, uint64_t band, uint64_t top_n,
                               gcsa2_cluster* d_top /* n_groups x top_n, row-major, or NULL */,
                               gcsa2_cluster_summary* d_summaries /* n_groups, or NULL */,
                               gcsa2_cluster_stats* stats /* host, or NULL */, void* stream);
int gcsa2_kmer_clusters_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                               uint64_t k, uint64_t stride, uint64_t hit_max, int over,
                               uint64_t shift, const uint64_t* d_coord_of_bin, uint64_t n_bins, uint64_t band, uint64_t top_n,
                               gcsa2_cluster* d_top, gcsa2_cluster_summary* d_summaries, gcsa2_cluster_stats* stats, void* stream);
int gcsa2_minimizer_clusters_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets, uint64_t n_patterns,
                                    uint64_t k, uint64_t w, uint64_t hash_seed, uint64_t hit_max, int over,
                                    uint64_t shift, const uint64_t* d_coord_of_bin, uint64_t n_bins, uint64_t band, uint64_t top_n,
                                    gcsa2_cluster* d_top, gcsa2_cluster_summary* d_summaries, gcsa2_cluster_stats* stats, void* stream);
/* The same for reads and the coordinate map in host memory, into host arrays: offsets[0] == 0, decreasing offsets are refused.
 * A batch of two pieces' worth of read bytes or more travels in pieces of whole reads (GCSA2_MS_PIECE_MB, GCSA2_MS_THREADS);
 * the map is uploaded once, a row belongs to one read and so does not depend on the cut, stats are summed over the pieces. */
int gcsa2_kmer_clusters_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                              uint64_t k, uint64_t stride, uint64_t hit_max, int over,
                              uint64_t shift, const uint64_t* coord_of_bin, uint64_t n_bins, uint64_t band, uint64_t top_n,
                              gcsa2_cluster* top /* host, n_patterns x top_n, or NULL */,
                              gcsa2_cluster_summary* summaries /* host, or NULL */, gcsa2_cluster_stats* stats);
int gcsa2_minimizer_clusters_batch(const gcsa2_index* index, const uint8_t* patterns, const uint64_t* offsets, uint64_t n_patterns,
                                   uint64_t k, uint64_t w, uint64_t hash_seed, uint64_t hit_max, int over,
                                   uint64_t shift, const uint64_t* coord_of_bin, uint64_t n_bins, uint64_t band, uint64_t top_n,
                                   gcsa2_cluster* top, gcsa2_cluster_summary* summaries, gcsa2_cluster_stats* stats);
/* Diagnostic (not the timed path): the default kernel instrumented with shader-clock counters, same results.  d_prof[16],
 * zeroed by the caller: [0..7] cycles summed over the wavefronts for the phases of a round (loop head / pattern window, step
 * setup, first block fetch, first evaluation, second fetch + evaluation, outcome + statistics, parent() from the LCP chunks,
 * parent() tree walk); [8..15] events: rounds, rounds with a second fetch, lane steps, pair attempts, failed pair attempts,
 * parent() calls, tree walks, second fetches of lanes.  Needs the pair blocks. */
int gcsa2_match_stats_profile_device(const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets,
                                     uint64_t n_queries, uint64_t total_pattern_bytes, uint16_t* d_ms, uint64_t* d_ranges,
                                     uint64_t* d_fallbacks, uint64_t* d_prof, void* stream);

/* ---- host-view container file ("G2HV") ---------------------------------------------------
 * Interchange between a process that can read .gcsa / .lcp files (the reference linked with SDSL:
 * GCSA::load, src/gcsa.cpp:184-216; LCPArray::load, src/lcp.cpp:130-143; exporter stub in
 * INTEGRATION.md) and GPU nodes that cannot.  The file is the gcsa2_host_view verbatim: header
 * fields, then every array with its byte length.  A bad tag or version fails like the reference's
 * load() does ("Invalid header", src/gcsa.cpp:188-193), as an error code.  These three functions
 * are host-only (no device needed). */
typedef struct gcsa2_view_storage gcsa2_view_storage;   /* owns the arrays of a loaded view */
int gcsa2_host_view_save(const gcsa2_host_view* view, const char* path);
int gcsa2_host_view_load(const char* path, gcsa2_view_storage** out);
const gcsa2_host_view* gcsa2_host_view_get(const gcsa2_view_storage* storage);
void gcsa2_host_view_free(gcsa2_view_storage* storage);
/* load + gcsa2_index_create in one call */
int gcsa2_index_create_from_file(const char* path, int device, gcsa2_index** out);

/* ---- the reference's own files ----------------------------------------------------------------
 * GCSA::load (src/gcsa.cpp:184-216) and LCPArray::load (src/lcp.cpp:130-143) for `.gcsa` / `.lcp`
 * files written by GCSA::serialize / LCPArray::serialize (GCSA version 3, LCP version 1), without
 * SDSL: each serialized SDSL container is decoded into the plain arrays of a gcsa2_host_view and the
 * rank / select supports are skipped.  lcp_path may be NULL (no parent / depth support then).
 * An invalid header fails like the reference's load() ("Invalid header", src/gcsa.cpp:188-193), as
 * GCSA2_ERR_INVALID_ARGUMENT; so does any structural inconsistency or any unaccounted byte.
 * FORMAT PARITY UNPINNED: the container encodings follow sdsl-lite 2.1.1 as recalled in SURVEY.md
 * section 8(f)-1; no real file was available to validate against (gcsa2_amd/csrc/sdsl_reader.hpp). */
int gcsa2_host_view_load_gcsa(const char* gcsa_path, const char* lcp_path, gcsa2_view_storage** out);
int gcsa2_index_create_from_gcsa(const char* gcsa_path, const char* lcp_path, int device, gcsa2_index** out);

/* The same from memory (what GCSA::load(std::istream&) / LCPArray::load(std::istream&) of the facade call after
 * reading the stream): parses one serialized structure at the start of `bytes`.  consumed != NULL: receives the
 * number of bytes the structure occupies, trailing bytes are left alone; consumed == NULL: the buffer must end
 * with the structure.  parse_lcp yields a view in which only the lcp_* fields are set. */
int gcsa2_host_view_parse_gcsa(const void* bytes, uint64_t size, uint64_t* consumed, gcsa2_view_storage** out);
int gcsa2_host_view_parse_lcp(const void* bytes, uint64_t size, uint64_t* consumed, gcsa2_view_storage** out);
/* GCSA::serialize (src/gcsa.cpp:140-179) / LCPArray::serialize (src/lcp.cpp:116-128) of a host view: the byte
 * stream is handed to `sink` piece by piece (an std::ostream::write in the facade).  Same caveat as for the
 * reader: the SDSL container encodings are restated from sdsl-lite 2.1.1, format parity is unpinned.
 * serialize_gcsa needs a view with samples and counters, serialize_lcp one with an LCP array. */
typedef void (*gcsa2_sink)(void* ctx, const void* data, uint64_t bytes);
int gcsa2_host_view_serialize_gcsa(const gcsa2_host_view* view, gcsa2_sink sink, void* ctx, uint64_t* written);
int gcsa2_host_view_serialize_lcp(const gcsa2_host_view* view, gcsa2_sink sink, void* ctx, uint64_t* written);
/* A device image holding only the LCP array of `view` (its GCSA fields are ignored): a stand-alone
 * gcsa::LCPArray as LCPArray::load (src/lcp.cpp:130-143) produces it.  Serves gcsa2_parent_* / depth / sv / rmq /
 * lcp_* ; the GCSA queries find nothing on it. */
int gcsa2_lcp_create(const gcsa2_host_view* view, int device, gcsa2_index** out);

/* ---- single-process multi-GPU -------------------------------------------------------------
 * A group holds one replica of the index per listed device (a device may be listed more than
 * once).  group_find_batch splits the batch into contiguous shards (sizes differ by at most one,
 * the static split of verifyIndex, src/algorithms.cpp:106-114), runs every shard on its device
 * from its own host thread and writes the ranges in query order.  Multi-process deployments
 * (one rank per GPU + one RCCL gather) use gcsa2_find_device from each rank instead. */
typedef struct gcsa2_group gcsa2_group;
int gcsa2_group_create(const gcsa2_host_view* view, const int* devices, int n_devices, gcsa2_group** out);
void gcsa2_group_destroy(gcsa2_group* group);
int gcsa2_group_size(const gcsa2_group* group);
const gcsa2_index* gcsa2_group_index(const gcsa2_group* group, int i);
int gcsa2_group_find_batch(const gcsa2_group* group, const uint8_t* patterns, const uint64_t* offsets,
                           uint64_t n_queries, uint64_t* ranges);

/* The same split with every shard already in the HBM of its device: d_patterns[r] / d_offsets[r] (offsets
 * rebased to 0, counts[r] + 1 entries) live on the device of replica r, d_ranges_root (2 x sum of counts words)
 * on the device of replica 0.  Every replica searches its shard on its own stream; the ranges are then gathered
 * in the root's HBM, in query order, by one grouped RCCL send / recv over xGMI (ncclCommInitAll over the device
 * list, created at the first call) -- or by peer copies when the group lists a device twice or RCCL is not
 * available (gcsa2_group_uses_rccl tells which).  Complete on return. */
int gcsa2_group_find_device(gcsa2_group* group, const uint8_t* const* d_patterns, const uint64_t* const* d_offsets,
                            const uint64_t* counts, uint64_t* d_ranges_root);
int gcsa2_group_uses_rccl(const gcsa2_group* group);

/* BASELINE configs[4] over the group -- the two queries of benchmark/query_gcsa.cpp:143-179 whose results are ragged or
 * long -- with the same contiguous split.  Both are complete on return.
 * group_match_stats_device: replica r computes the matching statistics of its shard (d_patterns[r], d_offsets[r] rebased
 *   to 0, counts[r] patterns of pattern_bytes[r] bytes in all); the statistics (sum of pattern_bytes entries + 4 spare,
 *   8-byte aligned), ranges and parent() counts (may be NULL) are gathered on replica 0's device in query order.
 * group_locate_device: replica r locates d_ranges[r] (counts[r] ranges); the per-replica totals come first, then the CSR
 *   offsets (rebased; d_offsets_root has sum of counts + 1 entries) and the values are gathered.  *job owns
 *   the values on replica 0's device (gcsa2_locate_discard). */
int gcsa2_group_match_stats_device(gcsa2_group* group, const uint8_t* const* d_patterns, const uint64_t* const* d_offsets,
                                   const uint64_t* counts, const uint64_t* pattern_bytes, uint16_t* d_ms_root,
                                   uint64_t* d_ranges_root, uint64_t* d_fallbacks_root);
int gcsa2_group_locate_device(gcsa2_group* group, const uint64_t* const* d_ranges, const uint64_t* counts, int sort,
                              uint64_t* d_offsets_root, gcsa2_locate_job** job, const uint64_t** d_values_root,
                              uint64_t* total_values);

/* ---- multi-process multi-GPU: one rank per GPU, one gather of hit ranges ----------------------
 * The single collective of the path: every rank searches its shard with gcsa2_find_device and
 * the (sp, ep) pairs are gathered in the root's HBM with grouped ncclSend / ncclRecv -- every peer uses its own
 * xGMI link into the root.  The communicator is RCCL's (ncclCommInitRank); the 128-byte id is created on one
 * rank and handed to the others by whatever launcher the application has (bench.py: the torch.distributed store).
 * RCCL is bound at run time; without it these calls fail with GCSA2_ERR_MISSING_COMPONENT. */
#define GCSA2_COMM_ID_BYTES 128
typedef struct gcsa2_comm gcsa2_comm;
int gcsa2_comm_unique_id(uint8_t* id /* GCSA2_COMM_ID_BYTES */);
int gcsa2_comm_create(const uint8_t* id, int rank, int world, int device, gcsa2_comm** out);
/* A communicator over the APPLICATION's transport instead of RCCL (MPI, a gather through host memory on hosts without RCCL,
 * the world-size-2 tests of this repository on one GPU): `gather` has the contract of gcsa2_comm_gather below -- rank r
 * contributes bytes[r] bytes of device memory at d_send, the root receives all parts back to back, in rank order, in device
 * memory at d_recv (its own part included) -- and is called by gcsa2_comm_gather / _match_stats / _locate wherever they would
 * use RCCL.  It may work asynchronously on `stream` or complete before it returns (after waiting for `stream`, on which the
 * data it sends was produced); 0 = success.  `user` is passed through.  gcsa2_comm_rccl_ranks reports 0 for such a
 * communicator.  d_send is always a valid device address, also when bytes[rank] == 0 (nothing is to be read from it then). */
typedef int (*gcsa2_gather_fn)(void* user, const void* d_send, const uint64_t* bytes, void* d_recv, int root, void* stream);
int gcsa2_comm_create_custom(int rank, int world, int device, gcsa2_gather_fn gather, void* user, gcsa2_comm** out);
void gcsa2_comm_destroy(gcsa2_comm* comm);
int gcsa2_comm_rank(const gcsa2_comm* comm);
int gcsa2_comm_world(const gcsa2_comm* comm);
/* The number of ranks RCCL itself reports for the communicator (ncclCommCount): what a benchmark prints to show that the
 * gather really spanned `world` devices. */
int gcsa2_comm_rccl_ranks(const gcsa2_comm* comm, int* ranks);
/* Rank r contributes bytes[r] bytes from d_send (bytes[] has `world` entries and is the same on every rank);
 * the root receives them back to back in rank order in d_recv (its own part by a device copy; d_recv may be
 * NULL elsewhere).  Enqueues on `stream` of the communicator's device and does not synchronise. */
int gcsa2_comm_gather(gcsa2_comm* comm, const void* d_send, const uint64_t* bytes, void* d_recv, int root, void* stream);
/* The same two queries with one rank per GPU: every rank passes its shard and the per-rank sizes (counts[r] queries and, for
 * the matching statistics, pattern_bytes[r] pattern bytes of rank r: the same arrays on every rank); the results land on
 * `root` in query order through gcsa2_comm_gather's grouped send / recv.  The *_root arguments are read on the root only.
 * comm_match_stats only enqueues on `stream` (all three result arrays are required on the root); comm_locate is complete on
 * return: the per-rank totals travel first, the root sizes the value buffer from them ("all-gather of
 * per-rank counts, then gatherv of the CSR values"). */
int gcsa2_comm_match_stats(gcsa2_comm* comm, const gcsa2_index* index, const uint8_t* d_patterns, const uint64_t* d_offsets,
                           const uint64_t* counts, const uint64_t* pattern_bytes, int root, uint16_t* d_ms_root,
                           uint64_t* d_ranges_root, uint64_t* d_fallbacks_root, void* stream);
int gcsa2_comm_locate(gcsa2_comm* comm, const gcsa2_index* index, const uint64_t* d_ranges, const uint64_t* counts, int sort,
                      int root, uint64_t* d_offsets_root, gcsa2_locate_job** job_root, const uint64_t** d_values_root,
                      uint64_t* total_values, void* stream);
/* Wire format for indexes whose path node and edge numbers are all below 2^32: (sp, ep) u64 pairs <->
 * (sp, ep + 1 - sp) u32 pairs, exact for every range find() returns (an empty range is (x, x - 1),
 * include/gcsa/utils.h:93-96).  Halves the bytes of the gather.  Launch on the current device. */
int gcsa2_pack_ranges32_device(const uint64_t* d_ranges, uint64_t n_queries, uint32_t* d_packed, void* stream);
int gcsa2_unpack_ranges32_device(const uint32_t* d_packed, uint64_t n_queries, uint64_t* d_ranges, void* stream);
/* The same for indexes whose path node and edge numbers are below 2^40 (BASELINE configs[3]: 5.7 G path nodes): 10 bytes per
 * range (sp and length, 40 bits each) instead of 16; d_packed holds 10 * n_queries bytes, 2-byte aligned. */
int gcsa2_pack_ranges40_device(const uint64_t* d_ranges, uint64_t n_queries, void* d_packed, void* stream);
int gcsa2_unpack_ranges40_device(const void* d_packed, uint64_t n_queries, uint64_t* d_ranges, void* stream);
/* Six bytes per range for the common case (same indexes): sp in 40 bits, the length in one byte, and behind the shard's ranges
 * a list of (query, length) pairs, `capacity` of them at most, for the ranges of 255 and more path nodes.  A shard's block has
 * gcsa2_wire48_bytes(n_queries, capacity) bytes whatever the ranges are -- the gather (src/algorithms.cpp:106-114 is the static
 * split it serves) keeps fixed sizes --, 16-byte aligned.  *d_overflow_count (optional, device memory) receives the number of
 * long ranges the shard had: a value beyond `capacity` means the block does not hold the batch (the ranges that did not fit
 * come out 255 path nodes long) and the caller must use the 40-bit pairs; nothing is truncated silently. */
uint64_t gcsa2_wire48_bytes(uint64_t n_queries, uint64_t capacity);
int gcsa2_pack_ranges48_device(const uint64_t* d_ranges, uint64_t n_queries, void* d_packed, uint64_t capacity, void* stream);
int gcsa2_unpack_ranges48_device(const void* d_packed, uint64_t n_queries, uint64_t capacity, uint64_t* d_ranges,
                                 uint64_t* d_overflow_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GCSA2_HIP_H */
