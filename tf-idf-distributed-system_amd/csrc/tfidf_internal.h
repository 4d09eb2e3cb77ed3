// tfidf_internal.h — kernel parameter blocks and launch wrappers (host side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>
#include <string>
#include <vector>

#include "tfidf_common.h"

namespace tfidf {

// Debug, test and A/B knobs (TFIDF_* environment variables other than
// TFIDF_DEBUG): read only while TFIDF_DEBUG is set, so a stray variable in a
// host process's environment (a JVM inherits its parent's) never changes the
// kernel path of the library.  Without TFIDF_DEBUG every knob is unset.
inline const char *knob(const char *name) {
  const char *d = getenv("TFIDF_DEBUG");
  if (!d || !*d || (d[0] == '0' && !d[1])) return nullptr;
  return getenv(name);
}

// Error flags raised by kernels (device word err[0]; err[1] = first doc).
constexpr uint32_t kErrCapacity = 4u;
constexpr uint32_t kErrTfTooLarge = 8u;
constexpr uint32_t kErrLongScratch = 16u;
constexpr uint32_t kErrCollision = 32u;   // two different terms under one hashed key: rebuild with another seed

// Long-document path: chunks of kChunk bytes, global per-document table.
constexpr uint32_t kChunk = 2048;
constexpr uint32_t kPreMargin = 64;
constexpr uint32_t kPostMargin = 320;
constexpr uint64_t kLongScratchBudget = 8ull << 30;   // per-document tables of the concurrent long-path workgroups

struct BuildParams {
  const uint8_t *text;        // corpus base (device)
  const uint64_t *offsets;    // staged doc offsets [n_staged + 1]
  const uint32_t *live_map;   // committed doc -> staged doc (nullptr = identity)
  uint64_t n_docs;            // committed docs
  uint64_t *dict;             // 3*C u64: lo[C] (key lo per slot), hi[C], ref[C] (dict_device.h)
  uint64_t hash_seed;         // KeyBuilder seed of this build (tfidf_common.h)
  uint64_t *verify_defer;     // hashed-key checks whose reference was not visible yet: (slot, ref word)
  uint32_t *verify_count;
  uint32_t verify_cap;
  uint32_t cap_mask;          // C - 1
  uint32_t range_shift;       // log2(range size)
  uint32_t n_ranges;          // R = C >> range_shift
  uint32_t *csr;              // padded CSR rows, one packed word per entry (csr_pack)
  uint64_t *csr_esc;          // escape list: (entry index << 24) | tf for tfs the packed field cannot hold
  uint32_t *esc_count;
  uint64_t esc_cap;
  uint32_t *doc_len;          // tokens per doc (field length)
  uint32_t *doc_nuniq;        // distinct terms per doc
  uint8_t *doc_norm;          // SmallFloat.intToByte4(len)
  uint32_t *rsplit;           // [n_docs][R] inclusive end of each range segment in the row
  uint32_t *long_list;        // docs deferred to the long path
  uint32_t *long_count;
  uint32_t *uni_list;         // per document: 1 = the ASCII wave path found non-ASCII bytes (Unicode wave path)
  uint32_t *uni_count;        // flagged documents
  uint32_t *uni_wave_count;   // flagged documents k_tokenize_wave<UNI> took (the rest: k_tokenize_uwave)
  uint32_t *bad_list;         // docs that are not valid UTF-8 (indexed empty; tfidf_malformed_docs)
  uint32_t *bad_count;
  unsigned long long *stats;  // [0] docCount, [1] sumTotalTermFreq, [2] nnz
  uint32_t *err;              // [0] flags, [1] first offending doc
  // long path scratch (one table region per workgroup)
  uint64_t *lt_keys;          // 2 * lt_slots per workgroup
  uint64_t *lt_pos;           // lt_slots per workgroup: first occurrence (dict_ref_word, document-relative)
  uint32_t *lt_cnt;           // lt_slots per workgroup
  uint32_t *lt_g;             // lt_slots per workgroup
  uint32_t lt_slots_log2;     // table slots per workgroup (max)
  uint32_t debug_stop;        // profiling only (TFIDF_DEBUG_STOP): end each document after phase N
  uint32_t debug_uw_full;     // A/B only (TFIDF_UW_FULL): the Unicode wave path always scans whole documents
  // wave path units: pack > 1 = packs of `pack` consecutive documents per
  // window (short-document corpora); documents a pack cannot take go to
  // retry_list.  doc_list (pack <= 1): process these documents only
  // (*doc_list_count of them) instead of 0..n_docs-1.
  uint32_t pack;
  uint32_t *retry_list;
  uint32_t *retry_count;
  const uint32_t *doc_list;
  const uint32_t *doc_list_count;
  // book-sized documents, chunk-parallel (k_tokenize_chunk / k_long_rows):
  // the group's documents, their first unit (chunk_pre[n_group_docs + 1],
  // unit = (document, core)), each unit's pair list (kWaveTerms u32 words:
  // (slot & (2^pair_bshift - 1)) << kPairTfBits | tf, grouped by bucket
  // slot >> pair_bshift) with its pair_nb + 1 bucket starts, failure flags
  const uint32_t *chunk_pre;
  uint32_t n_group_docs;
  uint64_t n_chunks;
  const uint32_t *chunk_docs;
  uint32_t *pairs;
  uint32_t *pair_ub;
  uint32_t pair_bshift, pair_nb;
  uint32_t *chunk_fail;
  // units whose window holds non-ASCII text: k_tokenize_chunk lists them for
  // k_tokenize_uchunk (nullptr: such a unit fails its document)
  uint32_t *uchunk_list;
  uint32_t *uchunk_count;
  // incremental commit: the packed wave path's units start at this document
  // (the rows and dictionary entries of documents below it are kept; 0 = a
  // full build; the one-document pass takes a doc_list instead).  Last, so no
  // other field's kernarg offset moves; read cold.
  uint64_t first_doc;
};

__host__ __device__ inline uint64_t csr_row_base(const uint64_t *offsets, uint64_t src) {
  // A document of L bytes holds at most ceil(L/2) tokens, so rows laid out at
  // floor((offset + src) / 2) never overlap.
  return (offsets[src] + src) >> 1;
}

// Packed CSR entry, one u32 per (document, distinct term): bits [0,
// range_shift) = the term's dictionary slot minus its range base (the row
// segment it sits in names the range, rsplit), bits [range_shift, 32) = tf.
// A tf the field cannot hold stores the all-ones escape there and the exact
// value goes to the escape list ((entry index << 24) | tf, sorted by the host
// after the build, binary-searched).  Block-major ranges are 2^16 slots
// (kRangeSlots; the whole dictionary when it is smaller), so the field is 16
// bits, escapes at tf >= 65 535 and only book-sized documents can escape;
// term-major rows keep the whole slot (range_shift = log2 C), so their field
// is 32 - log2 C bits (escape 16 383 at 2^18 slots, 511 at 2^23).  A word is
// never 0 (tf >= 1).
__host__ __device__ inline uint32_t csr_esc_value(uint32_t range_shift) { return 0xFFFFFFFFu >> range_shift; }
__host__ __device__ inline uint32_t csr_local(uint32_t e, uint32_t range_shift) {
  return e & ((1u << range_shift) - 1u);
}
__host__ __device__ inline uint32_t csr_tf_field(uint32_t e, uint32_t range_shift) { return e >> range_shift; }

// tf of escaped entry idx (0 if absent)
__host__ __device__ inline uint32_t csr_esc_tf(const uint64_t *esc, uint64_t n, uint64_t idx) {
  uint64_t a = 0, z = n;
  while (a < z) {
    const uint64_t m = (a + z) >> 1;
    if ((esc[m] >> 24) < idx) a = m + 1; else z = m;
  }
  return a < n && (esc[a] >> 24) == idx ? (uint32_t)(esc[a] & 0xFFFFFFu) : 0u;
}

}  // namespace tfidf
#if defined(__HIPCC__)
#include "dict_device.h"
#include "unicode_scan.h"
#endif
namespace tfidf {
#if defined(__HIPCC__)
// Cold parameters of the BuildParams kernels (every one takes the block as its
// only argument, so it sits at offset 0 of the kernarg segment): read at the
// point of use.  The asm makes the pointer opaque, so the scalar load is not
// hoisted out of the document loop and its value not kept live in SGPRs (the
// wave tokenizer used to spill ~100 of them to VGPR lanes and restore them
// with v_readlane in its hot loops).
typedef const BuildParams __attribute__((address_space(4))) KBuildParams;
__device__ __forceinline__ KBuildParams *cold_args() {
  KBuildParams *q = (KBuildParams *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(q));
  return q;
}
#define TFIDF_COLD(f) (cold_args()->f)

__device__ inline void set_build_err(uint32_t *err, uint32_t flag, uint32_t doc) {
  const uint32_t old = atomicOr(err, flag);
  if (old == 0) atomicExch(err + 1, doc);
}
// Exact identity of a hashed term that resolved to global dictionary slot
// `slot` without claiming it: its occurrence `mine` (dict_ref_word) must
// spell the same term as the slot's reference occurrence.  A reference not
// visible yet (claimed by another wave just now) defers the check to
// k_verify_deferred after the tokenizers.
__device__ inline void dict_verify(const BuildParams &p, uint32_t slot, uint64_t mine, uint32_t doc) {
  const uint64_t r = __hip_atomic_load(p.dict + 2 * ((size_t)p.cap_mask + 1) + slot, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  if (r == mine) return;
  if (r == 0) {
    const uint32_t at = atomicAdd(TFIDF_COLD(verify_count), 1u);
    if (at < TFIDF_COLD(verify_cap)) {
      uint64_t *vd = TFIDF_COLD(verify_defer);
      vd[2 * (size_t)at] = slot;
      vd[2 * (size_t)at + 1] = mine;
    } else {
      set_build_err(TFIDF_COLD(err), kErrCollision, doc);   // cannot defer: treated as a collision (rebuild)
    }
    return;
  }
  if (!uc_same_term(p.text + dict_ref_off(r), dict_ref_len(r), p.text + dict_ref_off(mine), dict_ref_len(mine)))
    set_build_err(TFIDF_COLD(err), kErrCollision, doc);
}

// write CSR entry idx of document doc (dictionary slot, tf)
__device__ inline void csr_put(const BuildParams &p, uint64_t idx, uint32_t slot, uint32_t tf, uint32_t doc) {
  const uint32_t esc = csr_esc_value(p.range_shift);
  uint32_t f = tf;
  if (tf >= esc) {
    f = esc;
    if (tf > kMaxTf) set_build_err(TFIDF_COLD(err), kErrTfTooLarge, doc);
    const uint32_t at = atomicAdd(TFIDF_COLD(esc_count), 1u);
    if (at < TFIDF_COLD(esc_cap)) TFIDF_COLD(csr_esc)[at] = (idx << 24) | (tf > kMaxTf ? kMaxTf : tf);
  }
  __builtin_nontemporal_store(csr_local(slot, p.range_shift) | (f << p.range_shift), p.csr + idx);   // read by the next kernel
}
#endif

// Block-major posting (one u32): document within its 8192-doc block (13
// bits) | min(tf, kPostTfEsc) << 13 | norm byte << 24.  tf >= kPostTfEsc
// (2047 occurrences of a term in one document) is an escape: the exact value
// is in the sorted posting escape list (csr_esc_tf format, keyed by posting
// index).  Term-major postings stay u64: doc | (tf << 8 | norm) << 32.
constexpr uint32_t kPostTfEsc = 2047;
__host__ __device__ inline uint32_t post_word(uint32_t doc_local, uint32_t tf, uint32_t norm) {
  return doc_local | ((tf < kPostTfEsc ? tf : kPostTfEsc) << 13) | (norm << 24);
}

struct PostingParams {
  const uint64_t *offsets;
  const uint32_t *live_map;
  uint64_t n_docs;
  uint32_t C;                 // dictionary slots
  uint32_t range_shift, n_ranges;
  uint32_t n_blocks;          // ceil(n_docs / kBlockDocs)
  const uint32_t *csr, *rsplit;
  const uint64_t *csr_esc;    // sorted escape list (csr_put)
  uint64_t n_esc;
  const uint8_t *doc_norm;
  uint32_t NC;                // columns: occupied dictionary slots (block-major: num_terms)
  const uint2 *crank;         // [C / 32 + 1] {occupancy bits, occupied slots before} per 32 slots (col_rank)
  uint32_t *blk;              // [(n_blocks + 1) * NC]: per-block term counts -> per-block exclusive
                              // offsets over columns; row n_blocks = df per column
  uint64_t *bbase;            // [n_blocks + 1]: first posting of each block (block-major postings)
  uint32_t *post;             // [nnz] block-major postings (post_word); block b, column c at
                              // bbase[b] + blk[b][c]
  uint64_t *post_esc;         // (posting index << 24) | tf for tf >= kPostTfEsc
  uint32_t *post_esc_count;
  uint64_t post_esc_cap;
  uint32_t *err;
  uint32_t *post_tmp;         // [nnz] scatter pass 1 output (sub-range streams, same regions)
  uint32_t sort_spw;          // scatter pass 2: sub-range streams per workgroup
  uint32_t first_block;       // incremental inversion (commit_plan.h): blocks [first_block, n_blocks) are built;
                              // the rows of blk (offset form), bbase and post of the blocks before are kept
  // launch shape of a few-block inversion (commit_plan.h slice_plan); 1 / 1: the unsliced kernels, which read none of these
  uint32_t slices, slice_docs;      // document slices per (block, range) tile, documents per slice
  uint32_t scan_parts, scan_width;  // workgroups per block row in the row scan, columns per part
  uint32_t *slice_cur;        // [(n_blocks - first_block) * n_ranges * 64] postings appended per (block, range, stream); zeroed per commit
  uint32_t *part_tot;         // [(n_blocks - first_block) * ceil(NC / 256)] row totals per k_df_sum workgroup (scan_parts > 1)
  // the kept df base (commit_plan.h df_base_plan)
  uint32_t *df_base;          // [NC] counts of blocks [0, first_block) per column; k_df_sum adds rows [first_block, df_fold_end)
  uint32_t df_fold_end;       // the blocks that are full now (n_docs / kBlockDocs), >= first_block
  uint32_t df_from_rows;      // A/B: df of the kept blocks from their rows (the base is kept up all the same)
  // a lone inverted block in one launch (commit_plan.h fuse_plan; k_df_fused alone reads these)
  uint32_t *fuse;             // [fuse_scratch_words(n_ranges, NC)] tickets, first offsets, block total; counts.  Zero between launches
  uint32_t fuse_tickets;      // the block's slices that hold documents (fuse_tickets())
};

// Raise a kernel's dynamic-LDS limit on the current device, once per device:
// the attribute applies to the device current at the call, so a process with
// indices on several GPUs sets it on each (idempotent, so concurrent first
// calls are harmless).
inline void allow_dyn_lds(const void *fn, int bytes, std::atomic<uint64_t> &done_mask) {
  int dev = 0;
  hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  if (done_mask.load(std::memory_order_acquire) & bit) return;
  hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  done_mask.fetch_or(bit, std::memory_order_acq_rel);
}

// --- launch wrappers (kernels_index.hip) ---
hipError_t launch_tokenize_wave(const BuildParams &p, int grid, hipStream_t s);
hipError_t launch_doc_range(uint32_t *list, uint32_t *count, uint32_t first, uint32_t n, hipStream_t s);
hipError_t launch_tokenize_wave_uni(const BuildParams &p, int grid, hipStream_t s);   // flagged non-ASCII documents
hipError_t launch_tokenize_chunks_uni(const BuildParams &p, int grid, hipStream_t s);  // flagged non-ASCII book units
constexpr uint32_t kWaveWGsPerCU = 8;       // 64-thread workgroups per CU (2 waves/SIMD: VGPR- and LDS-bound)
constexpr uint32_t kWaveGroups = 128;     // CSR row groups per wave unit (documents x ranges, k_tokenize_wave)
constexpr uint32_t kPackMaxDocs = 16;     // documents per packed window (<= kPackMax, kernels_index.hip)
constexpr uint64_t kPackBytes = 2560;     // text per packed window (auto pack size): ~450 tokens, under the
                                          // wave table's 512 distinct terms (cfg 5: 7 docs, tokenize 16.3 -> 14.9 ms)
hipError_t launch_tokenize_long(const BuildParams &p, int grid, hipStream_t s);
constexpr uint32_t kLongCoreBytes = 2048;              // = kCoreBytes (kernels_index.hip)
constexpr uint64_t kPairBudget = 2ull << 30;           // per-group unit pair lists (book-sized documents)
constexpr uint32_t kPairWords = 512;                    // pair list capacity per unit (= kWaveTerms)
#ifndef TFIDF_LR_WIN_BITS
#define TFIDF_LR_WIN_BITS 15
#define TFIDF_LR_THREADS 1024
#endif
#ifndef TFIDF_LR_IN
#define TFIDF_LR_IN 16
#define TFIDF_LR_UPT 2
#endif
#ifdef TFIDF_LR_WPE
#define TFIDF_LR_ATTR __attribute__((amdgpu_waves_per_eu(TFIDF_LR_WPE)))
#else
#define TFIDF_LR_ATTR
#endif
constexpr uint32_t kLrWinBits = TFIDF_LR_WIN_BITS;      // k_long_rows: LDS window of 2^kLrWinBits u32 counters (<= a range)
constexpr uint32_t kLrWin = 1u << kLrWinBits;
constexpr uint32_t kLrThreads = TFIDF_LR_THREADS;       // k_long_rows workgroup (kLrWin / kLrThreads <= 32)
static_assert(kLrWinBits <= kRangeBits && kLrWin / kLrThreads <= 32 && kLrWin / kLrThreads >= 4, "k_long_rows window");
constexpr uint32_t kPairTfBits = 12;                    // tf field of a pair word (a 2 KB core holds < 2^11 tokens)
hipError_t launch_tokenize_chunks(const BuildParams &p, int grid, hipStream_t s);
hipError_t launch_long_rows(const BuildParams &p, uint32_t n_docs, hipStream_t s);
hipError_t launch_tokenize_uwave(const BuildParams &p, int grid, hipStream_t s);   // kernels_unicode.hip
hipError_t launch_tokenize_uchunk(const BuildParams &p, int grid, hipStream_t s);  // kernels_unicode.hip
constexpr uint32_t kUwaveWGsPerCU = 7;    // 64-thread workgroups, ~22 KB LDS each (two waves per SIMD)
constexpr uint32_t kUchunkWGsPerCU = 8;   // k_tokenize_uchunk: ~19 KB LDS each
hipError_t launch_verify_deferred(const BuildParams &p, hipStream_t s);           // kernels_index.hip
// sliced shape: zeroes the rows the slices add into and slice_cur (one launch; before launch_df_partial)
hipError_t launch_inv_zero(const PostingParams &p, hipStream_t s);
hipError_t launch_df_partial(const PostingParams &p, hipStream_t s);
hipError_t launch_df_sum(const PostingParams &p, hipStream_t s);
hipError_t launch_df_fused(const PostingParams &p, hipStream_t s);   // a lone sliced block: count, df, row scan, block base
hipError_t launch_row_scan(const PostingParams &p, hipStream_t s);
hipError_t launch_block_base(const PostingParams &p, hipStream_t s);
hipError_t launch_count_nonzero(const uint64_t *a, uint32_t n, unsigned long long *out, hipStream_t s);
// block-major columns: crank over the final dictionary (total -> *n_cols), per-slot df from the column df
hipError_t launch_col_rank(const uint64_t *dict_lo, uint32_t C, uint2 *crank, unsigned long long *n_cols, hipStream_t s);
hipError_t launch_df_slots(const uint2 *crank, const uint32_t *df_col, uint32_t C, uint32_t *df_slot, hipStream_t s);
// ... and, for the host mirrors' deltas (commit_plan.h), the slots whose df changed and the new slots' keys
struct DictDelta;
struct DfDelta;
struct MirrorDeltaParams {
  const uint2 *crank, *crank_inv;      // now / at the snapshot's last build (crank_inv: read for dict_list only)
  const uint32_t *df_col;
  uint32_t C;
  uint32_t *df_slot;                   // read (the last build's values), then written
  const uint64_t *dict;                // lo plane [0, C), hi plane [C, 2 C)
  DictDelta *dict_list;                // nullptr: not built
  uint32_t dict_cap;
  uint32_t *dict_count;
  DfDelta *df_list;                    // nullptr: not built
  uint32_t df_cap;
  uint32_t *df_count;
};
hipError_t launch_df_slots_delta(const MirrorDeltaParams &p, hipStream_t s);
hipError_t launch_scatter(const PostingParams &p, hipStream_t s);
// kept blk rows [0, rows) from the column layout of crank_inv (stride NC_inv) to that of p.crank (p.blk, stride p.NC),
// and the df base with them (df_old -> p.df_base, count form)
hipError_t launch_blk_remap(const PostingParams &p, const uint32_t *blk_old, const uint32_t *df_old,
                            const uint2 *crank_inv, uint32_t NC_inv, hipStream_t s);

// --- term-major inversion for large vocabularies (kernels_term.hip) ---
// (hand-written LSD radix sort of packed words slot | doc | tf | norm)
constexpr uint64_t kTermMaxDocs = 1ull << 26;   // documents per shard in the term-major layout
struct TermParams {
  const uint64_t *offsets;
  const uint32_t *live_map;
  uint64_t n_docs, nnz;
  uint32_t C, slot_bits;      // C = 2^slot_bits
  uint32_t doc_bits, tf_bits; // packed word layout (kernels_term.hip TermLayout)
  const uint32_t *csr, *doc_nuniq;
  const uint64_t *csr_esc;
  uint64_t n_esc;
  const uint8_t *doc_norm;
  uint32_t *row_off;          // [n_docs] compact row offsets (exclusive sum of doc_nuniq)
  uint64_t *keys, *keys_alt;  // [nnz] each: packed words (ping-pong)
  uint64_t *tesc;             // tf >= 4095: (slot << 26 | doc, tf) u64 pairs, sorted by the host
  uint32_t *tesc_count;
  uint64_t tesc_cap, n_tesc;
  uint32_t *scratch;          // term_invert_scratch_words(n_docs, nnz) u32
  uint64_t *post;             // [nnz] out: doc | (tf << 8 | norm) << 32, term-major, docs ascending
  uint64_t *toff;             // [C + 1] out: first posting of each slot
  uint32_t *df;               // [C] out
  uint32_t *err;
};
uint64_t term_invert_scratch_words(uint64_t n_docs, uint64_t nnz, uint32_t C);
hipError_t launch_term_pairs(const TermParams &p, hipStream_t s);
hipError_t launch_term_sort(const TermParams &p, hipStream_t s);

// --- query scoring (kernels_query.hip) ---
constexpr uint32_t kInlTerms = 32;          // query terms carried in QueryParams (fused single query)
constexpr uint32_t kFusedMaxK = 64;         // tfidf_search top-k through the fused single-query launch up to this k
struct QueryParams {
  const uint64_t *post;       // term-major postings (toff != nullptr)
  const uint32_t *post32;     // block-major postings (post_word)
  const uint64_t *post_esc;   // block-major tf escapes, sorted
  uint64_t n_post_esc;
  const uint64_t *bbase;      // [n_blocks + 1] first posting of each block
  const uint32_t *blk;        // per-block exclusive offsets over columns [n_blocks * C]
  const uint64_t *toff;       // term-major layout: [C + 1] first posting per slot (nullptr = block-major)
  uint32_t C;                 // block-major: columns (num_terms); term-major: dictionary slots
  uint32_t n_blocks;
  uint64_t n_docs;
  const float *cache;         // 256 floats (BM25 norm cache)
  const uint32_t *q_off;      // [n_q + 1] into q_slot / q_w
  const uint32_t *q_slot;     // per query term: block-major column / term-major slot (kInvalidSlot = absent)
  const float *q_w;           // BM25 weight per query term (boost * idf)
  const uint32_t *q_role;     // per query term: role << 24 | MUST clause index (kRole*, tfidf_common.h)
  const uint32_t *q_meta;     // per query: MUST clause count | has MUST_NOT << 31 (0 = plain disjunction)
  uint32_t ops;               // k_score_blocks: the operator-query variant (MUST / MUST_NOT clauses)
  uint32_t n_q;
  uint32_t q_chunk;           // queries per score_blocks workgroup
  uint32_t k;                 // top-k (1..1024); 0 = all hits
  // outputs
  uint64_t *cand;             // [n_q][n_blocks][k] candidate keys (score bits << 32 | ~doc)
  uint32_t *cand_n;           // [n_q][n_blocks]
  uint32_t *out_doc;          // [n_q][k]
  float *out_score;           // [n_q][k]
  uint32_t *out_n;            // [n_q]
  // all-hits mode
  uint64_t *hits;             // [n_blocks * kBlockDocs] keys (score bits << 32 | ~doc)
  uint32_t *hits_n;           // [n_blocks]
  uint32_t hits_R2;           // batched all hits: query q's block b is run q * hits_R2 + b (0: one query)
  // wave-per-pair path (k > 0): pairs it leaves to k_score_blocks (nullptr = dense grid mode)
  uint32_t *ovf_list;         // pair ids q * n_blocks + b
  uint32_t *ovf_count;        // zeroed before k_score_pairs
  uint32_t *ovf2_list;        // pairs of operator queries (q_meta != 0), for k_score_blocks<true>
  uint32_t *ovf2_count;
  uint32_t list_grid;         // k_score_blocks workgroups in list mode
  // single query, one launch (tfidf_search, k <= 64): the query terms ride in
  // the kernel arguments (inl_n > 0: no upload) and the blocks' candidates go
  // to pinned host memory (cand / cand_n), merged by the host
  uint32_t inl_n;
  uint32_t inl_meta;
  uint32_t inl_slot[kInlTerms];
  float inl_w[kInlTerms];
  uint32_t inl_role[kInlTerms];
};
hipError_t launch_score_pairs(const QueryParams &p, int grid, hipStream_t s);
constexpr uint32_t kPairWavesPerWG = 2;   // k_score_pairs workgroup = 2 waves (30 KB LDS: 5 per CU)
hipError_t launch_score_blocks(const QueryParams &p, hipStream_t s);
// batched top-k (k <= kUnitMaxK, plain disjunctions, block-major): workgroup
// per (query, block range) unit {q, b0, b1, 0}; units of one query cover
// [0, n_blocks); unit_ctr zeroed before the launch
constexpr uint32_t kUnitMaxK = 64;
constexpr uint32_t kUnitMaxTerms = 64;
constexpr uint32_t kUnitWGsPerCU = 2;     // 71 KiB LDS each
hipError_t launch_score_units(const QueryParams &p, const uint4 *units, uint32_t n_units, uint32_t *unit_ctr, int grid,
                              hipStream_t s);
// light queries of such batches: wave per unit (hash table per block)
constexpr uint32_t kWunitWavesPerWG = kPairWavesPerWG;
constexpr uint32_t kWunitWGsPerCU = 6;    // 25 KiB LDS each (round 6: no claim list; 5 at 29 KiB before)
constexpr uint32_t kWunitLightPost = 550; // postings per block (query average) up to which a query is light (400: batch 5.80 ms, 500: 5.62, 600: 5.53, 700: 6.6 — past kWunitPassPost blocks take 16 passes;
                                          // round 5, 10 k queries at cfg 2: 450 / 500 / 550 / 600 / 650 / 700 = 5.95 / 5.94 / 5.52 / 5.53 / 5.69 / 6.53 ms device; 550 keeps a margin from the cliff)
hipError_t launch_score_wunits(const QueryParams &p, const uint4 *units, uint32_t n_units, uint32_t *unit_ctr, int grid,
                               hipStream_t s);
hipError_t launch_merge_topk(const QueryParams &p, hipStream_t s);
// all hits: per-block sorted runs (k_score_blocks, k == 0) -> one ordered list:
// (doc, score) split into out_doc / out_score, or packed keys with doc_base
// added into keys_out (when non-null).  P: R + 1 u64; tmp0 / tmp1: n_blocks *
// kBlockDocs u64 each (tmp1 may alias hits).
hipError_t launch_pack_keys(const uint32_t *out_doc, const float *out_score, const uint32_t *out_n, uint32_t n_q,
                            uint32_t k, uint64_t doc_base, uint64_t *keys, hipStream_t s);
hipError_t launch_hits_order(const uint64_t *hits, const uint32_t *hits_n, uint32_t R, uint64_t *P, uint64_t *tmp0,
                             uint64_t *tmp1, uint64_t *tmp2, uint32_t *out_doc, float *out_score, uint64_t *keys_out,
                             uint64_t doc_base, uint64_t hits_bound, int grid, hipStream_t s);
constexpr uint64_t kHitsGroupAvg = 6144;   // all hits: 8-run LDS group merge when hits per group average <= this
// all hits of a chunk of n_q queries: runs indexed q * R2 + b (R2 = hits_runs_per_query(R):
// a power of two >= 2, the padding runs empty with hits_n = 0), so no merge level spans two
// queries.  P: n_q * R2 + 1 u64; q_off [n_q + 1]: each query's offset in out_doc / out_score
// (q_off[n_q] = the chunk's hits).  hits holds n_q * R2 * kBlockDocs u64 (gapped runs) and is
// reused as a merge buffer; tmp0 / tmp2 hold the chunk's hits (hits_bound: an upper bound of
// them, summed over the chunk's queries).  keys_out (when non-null): the last level writes
// packed merge keys with doc_base added there instead of out_doc / out_score, as
// launch_hits_order does.
constexpr uint32_t hits_runs_per_query(uint32_t R) {
  uint32_t r2 = 2;
  while (r2 < R) r2 <<= 1;
  return r2;
}
hipError_t launch_hits_order_batch(uint64_t *hits, const uint32_t *hits_n, uint32_t n_q, uint32_t R, uint64_t *P,
                                   uint64_t *tmp0, uint64_t *tmp2, uint32_t *out_doc, float *out_score,
                                   uint64_t *q_off, uint64_t *keys_out, uint64_t doc_base, uint64_t hits_bound,
                                   int grid, hipStream_t s);

// --- compound queries (kernels_compound.hip; rules in compound_plan.h) ---
// One chunk of queries: their clauses' rows flattened clause after clause (rows:
// (doc, score bits); c_off: n_c + 1), binned by (clause, doc block) and combined
// per (query, block) into sorted runs in the batched all-hits layout (run
// q * R2 + b of hits / hits_n; n_q * n_blocks < 2^31).  bin_cnt / bin_off:
// n_c * n_blocks + 1 u64 each; binned: n_e entries.
// A nested chunk (tfidf_search_nested*; rules in compound_tree_plan.h) is the
// same with one "clause" per node of its queries' trees, a group's row empty,
// and the node table beside the occurs: c_parent is set, and levels is the most
// groups any query of the chunk has open at once.  launch_compound_pass then
// combines with k_cqn_combine.
struct CqPass {
  const uint2 *rows;
  const uint64_t *c_off;
  const uint32_t *c_occur;    // per clause of the chunk: TFIDF_OCCUR_*; nested: | 0x100 for a group
  const uint32_t *q_coff;     // [n_q + 1] first clause of each query
  const uint32_t *c_parent;   // nested only: per node its parent within the query
  const uint32_t *c_msm;      // nested only: per node min_should_match
  uint64_t *bin_cnt, *bin_off;
  uint2 *binned;
  uint64_t *hits;
  uint32_t *hits_n;
  uint64_t n_e;
  uint32_t n_c, n_q, n_blocks, R2, n_docs;
  uint32_t levels;            // nested only: 1 .. kCqnMaxDepth
};
hipError_t launch_compound_pass(const CqPass &p, int grid, hipStream_t s);

// --- GLOBAL statistics by term ownership (kernels_vocab.hip) ---
hipError_t vocab_count(const uint64_t *dict, uint32_t C, uint32_t G, uint32_t *counts, hipStream_t s);
hipError_t vocab_starts(const uint32_t *counts, uint32_t G, uint32_t *cursor, uint64_t *counts_out, hipStream_t s);
hipError_t vocab_scatter(const uint64_t *dict, const uint32_t *df, uint32_t C, uint32_t G, uint32_t *cursor,
                         uint64_t *records, uint32_t *sent_slot, hipStream_t s);
hipError_t vocab_reduce(const uint64_t *records, uint64_t n, uint64_t *table, uint32_t tmask, uint32_t *sums,
                        uint32_t *rslot, uint32_t *out, unsigned long long *n_unique, hipStream_t s);
hipError_t vocab_import(const uint32_t *sent_slot, const uint32_t *gdf_in, uint64_t n, uint32_t *gdf, hipStream_t s);

// --- hit highlighting (kernels_highlight.hip; rules in snippet_plan.h) ---
struct HlItem;
struct HlKey;
hipError_t launch_hl_extents(const uint64_t *offsets, const uint32_t *staged, uint64_t n, uint64_t *ext,
                             hipStream_t s);
hipError_t launch_hl_scan(bool fill, const uint8_t *text, const uint64_t *ext, const HlItem *items, uint32_t n_items,
                          const HlKey *keys, const uint32_t *key_off, const uint32_t *row_q, uint64_t seed,
                          uint64_t *counts, uint64_t m_base, uint64_t *starts, uint32_t *lens, uint32_t *ords,
                          hipStream_t s);
hipError_t launch_hl_row_offsets(const uint64_t *scanned, const uint64_t *first, uint64_t n, uint64_t base,
                                 uint64_t *row_off, hipStream_t s);
hipError_t launch_hl_rank(const uint8_t *text, const uint64_t *ext, const uint64_t *row_off, const uint64_t *starts,
                          const uint32_t *lens, const uint32_t *ords, uint32_t W, uint64_t n, uint64_t *sn_a,
                          uint64_t *sn_len, uint64_t *in_first, uint64_t *in_cnt, hipStream_t s);
hipError_t launch_hl_pack(const uint8_t *text, const uint64_t *ext, const uint64_t *sn_a, const uint64_t *text_off,
                          uint8_t *out, const uint64_t *starts, const uint32_t *lens, const uint32_t *ords,
                          const uint64_t *in_first, const uint64_t *m_off, uint64_t *o_starts, uint32_t *o_lens,
                          uint32_t *o_ords, uint64_t n, hipStream_t s);

// --- fuzzy term lookup (kernels_fuzzy.hip; rules in fuzzy_plan.h) ---
// One pass of a chunk of staged input terms over the dictionary.  t_off[i] ..
// t_off[i + 1] index t_cps (lower-cased code points; an empty range = a term
// without candidates); n_terms <= kFzChunkTerms, t_off[n_terms] <= kFzChunkCps.
struct FzScan {
  const uint64_t *dict;       // lo[C], hi[C], ref[C]
  const uint32_t *df;         // per slot (Snapshot::df_dev)
  uint32_t C;
  const uint32_t *t_off, *t_cps;
  uint32_t n_terms, max_edits, prefix_len;
  uint32_t search;            // fuzzy search: candidates need fzs_keep, keys are fzs_sort_key (fuzzy_search_plan.h)
  uint32_t *counts;           // count pass: survivors per staged term (zeroed before)
  uint64_t *keys;             // fill pass: fz_sort_key per survivor, its slot, the append cursor (zeroed
  uint32_t *slots;            // before) and the capacity the counts gave
  uint32_t *cursor;
  uint32_t cap;
  uint32_t *hs_list;          // hashed slots: compacted by the count scan (hs_count zeroed before; entries
  uint32_t *hs_count;         // past hs_cap are counted, not stored), read by k_fz_hashed (hs_n of them)
  uint32_t hs_cap, hs_n;
};
hipError_t launch_fz_scan(bool fill, const FzScan &a, int max_grid, hipStream_t s);
hipError_t launch_fz_hashed(bool fill, const FzScan &a, const uint8_t *text, uint64_t text_bytes, int max_grid,
                            hipStream_t s);
hipError_t fz_sort(void *tmp, size_t *tmp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *slots_in,
                   uint32_t *slots_out, uint32_t n, hipStream_t s);
hipError_t launch_fz_select(const uint64_t *keys, const uint32_t *seg, uint32_t n_terms, uint32_t max_out,
                            uint32_t *take, hipStream_t s);
hipError_t launch_fz_gather(const uint64_t *keys, const uint32_t *slots, const uint32_t *seg, const uint32_t *out_off,
                            uint32_t n_terms, uint64_t *o_keys, uint32_t *o_slots, hipStream_t s);

// --- fuzzy search (kernels_fuzzy_search.hip; rules in fuzzy_search_plan.h) ---
// The expansion of each of n_terms input terms from its sorted candidates
// (keys / slots of term t: [seg[t], seg[t + 1]), fzs_sort_key order): the first
// E <= kFzsMaxExpansions in (boost descending, term bytes ascending) order, in
// that order: out_n[t] entries at out_keys / out_slots [t * kFzsMaxExpansions].
struct FzsSelect {
  const uint64_t *keys;
  const uint32_t *slots, *seg;
  uint32_t n_terms, E;
  const uint64_t *dict;       // lo[C], hi[C], ref[C]
  uint32_t C;
  const uint8_t *text;        // the corpus: a hashed key is read from its reference occurrence
  uint64_t text_bytes;
  uint32_t *out_n;
  uint64_t *out_keys;
  uint32_t *out_slots;
};
hipError_t launch_fzs_select(const FzsSelect &a, hipStream_t s);

// --- wildcard and prefix search (kernels_wildcard.hip; rules in wildcard_plan.h) ---
// The scan takes an FzScan: t_cps holds pattern elements (wc_parse), n_terms <=
// kWcChunkPatterns patterns of t_off[n_terms] - t_off[0] <= kWcChunkElems
// elements; max_edits and prefix_len are not read.
hipError_t launch_wc_scan(bool fill, const FzScan &a, int max_grid, hipStream_t s);
hipError_t launch_wc_hashed(bool fill, const FzScan &a, const uint8_t *text, uint64_t text_bytes, int max_grid,
                            hipStream_t s);
// The union of the matched terms' postings for n_pat patterns: pattern p's
// matched slots are slots[seg[p]] .. slots[seg[p + 1]].  bits: n_pat bitmaps of
// n_blocks * kBlockDocs bits; cnt: n_pat * n_blocks + 1 words (bits per
// (pattern, block), then scanned in place); out: the ascending doc ids.
struct WcUnion {
  const uint32_t *slots, *seg;
  uint32_t n_pat, C;          // C: dictionary slots
  uint32_t n_blocks, NC;
  uint64_t n_docs, post_words;  // post_words: postings the layout's buffer holds
  const uint2 *crank;         // block-major (toff == nullptr): col_rank, blk, bbase, post_word postings
  const uint32_t *blk;
  const uint64_t *bbase;
  const uint32_t *post32;
  const uint64_t *toff, *post;  // term-major
  uint64_t *row_off;          // term-major: [M + 1] the matched rows' lengths, then scanned in place
  uint32_t *bits;
  uint64_t *cnt;
  uint32_t *out;
  uint64_t out_cap;
};
// --- regular-expression search (kernels_regex.hip; rules in regex_plan.h) ---
// The scan takes an FzScan: t_cps holds the words of the patterns' DFA tables,
// n_terms <= kWcChunkPatterns tables of t_off[n_terms] - t_off[0] <=
// kRxStageWords words; max_edits and prefix_len are not read.
hipError_t launch_rx_scan(bool fill, const FzScan &a, int max_grid, hipStream_t s);
hipError_t launch_rx_hashed(bool fill, const FzScan &a, const uint8_t *text, uint64_t text_bytes, int max_grid,
                            hipStream_t s);
hipError_t launch_wc_union_block(const WcUnion &a, hipStream_t s);
hipError_t launch_wc_rows(const WcUnion &a, uint32_t M, hipStream_t s);
hipError_t launch_wc_union_term(const WcUnion &a, uint32_t M, uint64_t n_post_bound, int max_grid, hipStream_t s);
hipError_t launch_wc_count(const WcUnion &a, hipStream_t s);
hipError_t launch_wc_expand(const WcUnion &a, hipStream_t s);

// --- exact phrase search (kernels_phrase.hip; rules in phrase_plan.h) ---
hipError_t launch_ph_scan(bool fill, const uint8_t *text, const uint64_t *ext, const HlItem *items, uint32_t i0,
                          uint32_t ni, const HlKey *keys, const uint32_t *key_off, const uint32_t *row_q,
                          uint64_t seed, const uint64_t *first, uint64_t *all, uint64_t *listed, uint64_t m_base,
                          uint32_t *o_pos, uint32_t *o_ord, hipStream_t s);
hipError_t launch_ph_freq(const uint64_t *row_off, uint64_t m_base, const uint32_t *pos, const uint32_t *ord,
                          const uint32_t *row_q, const uint32_t *seq, const uint32_t *seq_off, uint64_t n,
                          uint32_t *freq, hipStream_t s);
hipError_t launch_ph_score(const uint32_t *freq, const uint32_t *docs, const uint32_t *row_q, const float *w,
                           const float *cache, const uint8_t *norm, uint64_t n, uint64_t *key, uint64_t *flag,
                           hipStream_t s);
// sloppy phrases: slop[phrase]; freq as a float (count of the exact rule at slop 0 or for one term)
hipError_t launch_ph_sloppy_freq(const uint64_t *row_off, uint64_t m_base, const uint32_t *pos, const uint32_t *ord,
                                 const uint32_t *row_q, const uint32_t *seq, const uint32_t *seq_off,
                                 const uint32_t *slop, uint64_t n, float *freq, hipStream_t s);
hipError_t launch_ph_score_f(const float *freq, const uint32_t *docs, const uint32_t *row_q, const float *w,
                             const float *cache, const uint8_t *norm, uint64_t n, uint64_t *key, uint64_t *flag,
                             hipStream_t s);
// freq: a count, or a float frequency's word (never negative: 0 is "no hit" for both); emit copies it
hipError_t launch_ph_compact(const uint64_t *key, const uint32_t *freq, const uint64_t *at, uint64_t n,
                             uint64_t *o_key, uint32_t *o_row, hipStream_t s);
hipError_t ph_sort_bytes(size_t *tmp_bytes, uint32_t n);
hipError_t ph_sort(void *tmp, size_t tmp_bytes, const uint64_t *key_in, uint64_t *key_a, uint32_t *row_in,
                   uint32_t *row_a, uint32_t *q_a, uint32_t *q_b, const uint32_t *row_q, uint32_t q0, uint32_t n_q,
                   uint32_t n, const uint32_t **rows_out, hipStream_t s);
hipError_t launch_ph_emit(const uint32_t *rows, const uint64_t *key, const uint32_t *freq, uint64_t n, uint32_t *o_doc,
                          float *o_score, uint32_t *o_freq, hipStream_t s);

// --- more-like-this (kernels_mlt.hip; rules in mlt_plan.h) ---
// One pass over the forward rows of seeds [s0, s1) of a staged batch: the
// flattened entries row_off[s0] .. row_off[s1] (row_off: exclusive scan of the
// rows' lengths over all n_seeds seeds, n_seeds + 1 words).
struct MltScan {
  const uint32_t *csr;        // packed CSR entries (csr_pack) and the words the buffer holds
  uint64_t csr_words;
  const uint32_t *rsplit;     // [n_docs][R] row range segments
  uint32_t R, range_shift, C;
  const uint64_t *csr_esc;    // sorted tf escapes
  uint64_t n_esc;
  const uint32_t *df;         // per slot (Snapshot::df_dev)
  const float *idf;           // mlt_idf_table: [n_docs + 1]
  uint64_t n_docs;
  const uint32_t *seed_doc;   // [n_seeds] committed ids
  const uint64_t *row_base;   // [n_seeds] first CSR entry of each seed's row
  const uint64_t *row_off;    // [n_seeds + 1]
  uint32_t s0, s1;
  uint32_t min_tf, min_df, max_df;
  uint32_t *counts;           // count pass: survivors per seed (zeroed before)
  uint64_t *keys, *vals;      // fill pass: mlt_key (seed relative to s0) / mlt_val per survivor, the
  uint32_t *cursor;           // append cursor (zeroed before) and the capacity the counts gave
  uint32_t cap;
};
hipError_t launch_mlt_extents(const uint64_t *offsets, const uint32_t *doc_nuniq, const uint32_t *seed_doc,
                              const uint32_t *seed_staged, uint32_t n, uint64_t *row_base, uint64_t *row_len,
                              hipStream_t s);
hipError_t launch_mlt_scan(bool fill, const MltScan &a, uint64_t n_entries, int max_grid, hipStream_t s);
hipError_t mlt_sort(void *tmp, size_t *tmp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint64_t *vals_in,
                    uint64_t *vals_out, uint32_t n, int end_bit, hipStream_t s);
hipError_t launch_mlt_select(const uint64_t *keys, const uint32_t *seg, uint32_t n_seeds, uint32_t max_terms,
                             uint32_t *take, hipStream_t s);
hipError_t launch_mlt_gather(const uint64_t *keys, const uint64_t *vals, const uint32_t *seg, const uint32_t *out_off,
                             uint32_t n_seeds, uint64_t *o_keys, uint64_t *o_vals, hipStream_t s);

// --- index internals the node-level orchestration reads (tfidf_capi.hip) ---
}  // namespace tfidf
struct tfidf_index;
struct tfidf_reader;
namespace tfidf {
hipStream_t index_stream(tfidf_index *ix);
int index_device(const tfidf_index *ix);
bool index_committed(const tfidf_index *ix);
uint64_t index_num_docs(const tfidf_index *ix);
uint64_t index_generation(const tfidf_index *ix);   // successful commits so far
int set_error(int code, const char *msg);       // sets tfidf_last_error() of the calling thread
// fuzzy term lookup on the snapshot published now: per input term its ordered
// candidates (at most max_out; 0 = all of them) and their count before truncation
struct FuzzyCand {
  std::string term;
  uint64_t df;
  uint32_t dist;
};
struct FuzzyLists {
  std::vector<std::vector<FuzzyCand>> cands;
  std::vector<uint64_t> n_within;
  float ms_device = 0.0f;
};
int index_fuzzy_terms(tfidf_index *ix, const uint8_t *t_utf8, const uint64_t *t_offsets, uint32_t n_terms,
                      uint32_t max_edits, uint32_t prefix_len, uint32_t max_out, FuzzyLists *out);
// wildcard search on the snapshot published now.  docs == false: per pattern its
// matching terms in (df descending, bytes) order (at most max_out; 0 = all of
// them; dist is 0).  docs == true: the patterns' ascending hit lists, one after
// the other (hit_off: n_p + 1).  n_matched: matching terms before truncation.
struct WildcardLists {
  std::vector<std::vector<FuzzyCand>> terms;
  std::vector<uint64_t> n_matched;
  std::vector<uint32_t> docs;
  std::vector<uint64_t> hit_off;
  float ms_device = 0.0f;
};
int index_wildcard(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p, bool docs,
                   uint32_t max_out, WildcardLists *out);
// the same for regular expressions, from compiled tables (a node compiles once for all its
// shards).  regex_compile_all: the patterns' DFA tables (empty: matches nothing), or the first
// pattern's error (TFIDF_E_QUERY_SYNTAX / TFIDF_E_UNSUPPORTED_QUERY).
int index_regex(tfidf_index *ix, const std::vector<std::vector<uint32_t>> &tabs, bool docs, uint32_t max_out,
                WildcardLists *out);
int regex_compile_all(const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                      std::vector<std::vector<uint32_t>> *tabs);
// more-like-this on the snapshot published now: per seed (a committed doc id)
// its interesting terms in selection order and the candidates before truncation
struct MltRules;
struct MltTerm {
  std::string term;
  uint32_t slot, tf, df;
  float score;
};
struct MltLists {
  std::vector<std::vector<MltTerm>> terms;
  std::vector<uint64_t> n_cand;
};
int index_mlt_terms(tfidf_index *ix, const uint32_t *seeds, uint32_t n, const MltRules &rules, MltLists *out);
// top k of one disjunction per term list (SHOULD clauses in list order, boost
// 1; a term this shard lacks has no scorer) in the layout of tfidf_search_batch
int index_search_term_lists(tfidf_index *ix, const std::vector<std::vector<std::string>> &lists, uint32_t k,
                            uint32_t *doc_ids, float *scores, uint32_t *counts);
// device-key searches on a reader's pinned snapshot (tfidf_reader_open)
int reader_batch_keys_device(tfidf_reader *rd, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                             uint32_t k, uint64_t doc_base, void *d_keys);
int reader_all_keys_device(tfidf_reader *rd, const uint8_t *q, uint64_t q_len, uint64_t doc_base, void *d_keys,
                           uint64_t cap, uint64_t *n_out);
// All hits of a batch as device merge keys (the node-level all-hits batches):
// the batch is prepared once (bounds[i] = query i's local hit bound: the sum of
// its scoring terms' df, at most num_docs; 0 for a query that does not parse),
// then any query range [a, z) of it is scored: the range's hits as merge keys
// (score bits << 32 | ~(doc + doc_base)), query-major and contiguous, each
// query's run in descending key order, appended into d_keys (cap >= the sum of
// the range's bounds) by local chunks whose scratch stays in the single-index
// all-hits budget; counts[i] = hits of query a + i, *n_out their sum.
struct PreparedAllHits;
int reader_prepare_all_hits(tfidf_reader *rd, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                            PreparedAllHits **out, uint64_t *bounds);
void free_prepared_all_hits(PreparedAllHits *pb);
int reader_batch_all_keys_device(tfidf_reader *rd, const PreparedAllHits *pb, uint32_t a, uint32_t z,
                                 uint64_t doc_base, void *d_keys, uint64_t cap, uint64_t *counts, uint64_t *n_out);
// GLOBAL exchange steps without the public calls' host synchronisation (every
// buffer is the communicator's, ordered on the index's stream)
int vocab_partition_async(tfidf_index *ix, uint32_t n_ranks, void *d_records, uint64_t cap, void *d_counts,
                          uint64_t *n_out);
int vocab_reduce_async(tfidf_index *ix, const void *d_records, uint64_t n, void *d_df_out, void *d_n_unique);
int set_global_df_async(tfidf_index *ix, const void *d_df, uint64_t n, uint64_t doc_count, uint64_t sum_ttf,
                        uint64_t *generation);
// String.compareTo order of two UTF-8 names (UTF-16 code units; Leader.java:80-88 TreeMap)
int utf16_compare(const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb);

// --- node-level merges (tfidf_dist.hip) ---
// lists (q, r) of `len` merge keys at keys + r * rstride + q * qstride, each
// sorted descending (0 = empty, last): out[q * k_out + i] = the i-th largest
// key of query q over all n_lists lists (i < k_out), 0 past the last one
hipError_t launch_merge_lists(const uint64_t *keys, uint32_t n_lists, uint64_t rstride, uint64_t qstride, uint64_t len,
                              uint32_t n_q, uint64_t *out, uint64_t k_out, hipStream_t s);

// --- synthetic corpus (kernels_synth.hip) ---
hipError_t synth_doc_lengths(uint64_t seed, uint64_t n_docs, uint64_t doc_base, const double *cdf,
                             const uint32_t *guide, uint32_t V, uint32_t len_min, uint32_t len_max,
                             uint64_t *bytes_out, hipStream_t s);
hipError_t synth_doc_text(uint64_t seed, uint64_t n_docs, uint64_t doc_base, const double *cdf,
                          const uint32_t *guide, uint32_t V, uint32_t len_min, uint32_t len_max,
                          const uint64_t *offsets, uint8_t *text, hipStream_t s);
hipError_t exclusive_scan_u64(const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t s);

#if defined(__HIPCC__)
// Book-sized documents: unit = (document, kCoreBytes core) with context
// margins (k_tokenize_chunk, k_tokenize_uchunk).
constexpr uint32_t kCoreBytes = kLongCoreBytes;
constexpr uint32_t kPreBytes = 64;
constexpr uint32_t kPostBytes = 320;
static_assert(kPreBytes + kCoreBytes + kPostBytes + 16 <= 4096, "chunk window: a wave window holds it");

struct ChunkMeta {
  uint64_t s0, L;                 // window: corpus bytes [s0, s0 + L)
  uint32_t shift, core_lo, core_hi, gi;
  uint64_t d;
};

__device__ __forceinline__ ChunkMeta chunk_meta(const BuildParams &p, uint64_t u) {
  // group document holding unit u: chunk_pre[gi] <= u < chunk_pre[gi + 1] (binary search, scalar loads)
  uint32_t lo = 0, hi = p.n_group_docs;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (p.chunk_pre[mid] <= u) lo = mid; else hi = mid;
  }
  const uint2 e = make_uint2(lo, (uint32_t)(u - p.chunk_pre[lo]));
  ChunkMeta m;
  m.gi = e.x;
  m.d = p.chunk_docs[e.x];
  const uint64_t src = p.live_map ? p.live_map[m.d] : m.d;
  const uint64_t dlo = p.offsets[src], dl = p.offsets[src + 1] - dlo;
  const uint64_t clo = (uint64_t)e.y * kCoreBytes, chi = min(dl, clo + kCoreBytes);
  const uint64_t ws = clo > kPreBytes ? clo - kPreBytes : 0, we = min(dl, chi + kPostBytes);
  m.s0 = dlo + ws;
  m.L = we - ws;
  m.core_lo = (uint32_t)(clo - ws);
  m.core_hi = (uint32_t)(chi - ws);
  m.shift = (uint32_t)(reinterpret_cast<uintptr_t>(p.text + m.s0) & 15);
  return m;
}


#endif

}  // namespace tfidf
