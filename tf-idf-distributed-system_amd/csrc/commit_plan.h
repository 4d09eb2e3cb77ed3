// commit_plan.h — the host side of an incremental tfidf_commit: whether the
// build target's rows and dictionary can be kept (and from which document the
// tokenizers then start), how the kept host lists take the new entries, and
// how the host mirrors of the dictionary and df follow, the launch shape
// of a few-block inversion, when a lone block is inverted in one launch, and
// the df base a snapshot keeps for its kept blocks.  Plain C++ (no HIP), so the
// decisions are tested on their own
// (tests/commit_plan_check.cpp, tests/mirror_plan_check.cpp,
// tests/slice_plan_check.cpp, tests/df_base_plan_check.cpp,
// tests/fuse_plan_check.cpp).
#pragma once

#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

namespace tfidf {

// Every knob commit_once reads before the inversion, the A/B switch, and
// TFIDF_TEST_G4_BITS, which the tokenizer launchers read to choose the
// dictionary's probe form (kept entries must be found by the form that
// inserted them).  A snapshot's rows are kept only under the knob values they
// were built with, so a test that re-commits one index under another knob
// still runs the path it names.
constexpr int kCommitKnobs = 11;
inline const char *const *commit_knob_names() {
  static const char *const names[kCommitKnobs] = {
      "TFIDF_NO_UNIWAVE", "TFIDF_NO_UNIFIRST",    "TFIDF_PACK_DOCS",  "TFIDF_NO_UCHUNK",       "TFIDF_TEST_PAIR_UNITS",
      "TFIDF_UW_FULL",    "TFIDF_TEST_WEAK_HASH", "TFIDF_DEBUG_STOP", "TFIDF_WAVE_WGS_PER_CU", "TFIDF_FULL_COMMIT",
      "TFIDF_TEST_G4_BITS"};
  return names;
}
constexpr int kKnobFullCommit = 9;

// a knob's value as one word: 0 = unset, else FNV-1a of the string with the top bit set
inline uint64_t knob_sig(const char *v) {
  if (!v) return 0;
  uint64_t h = 1469598103934665603ull;
  for (; *v; v++) h = (h ^ (uint8_t)*v) * 1099511628211ull;
  return h | (1ull << 63);
}

// What a snapshot's rows, per-document words and dictionary depend on besides
// the documents' own text.
struct CommitSig {
  uint64_t epoch = 0;        // tfidf_index::corpus_epoch: clear, load, a moving compaction, any live -> dead
  uint64_t hash_seed = 0;    // KeyBuilder seed the build ran under
  uint64_t n_dead = 0;       // rows are kept only without dead documents (csr_row_base by staged id == committed id)
  uint32_t cap_log2 = 0, C = 0, range_shift = 0, R = 0;
  bool term_major = false;
  uint64_t knobs[kCommitKnobs] = {};
};

inline bool commit_sig_equal(const CommitSig &a, const CommitSig &b) {
  if (a.epoch != b.epoch || a.hash_seed != b.hash_seed || a.n_dead != b.n_dead || a.cap_log2 != b.cap_log2 ||
      a.C != b.C || a.range_shift != b.range_shift || a.R != b.R || a.term_major != b.term_major)
    return false;
  for (int i = 0; i < kCommitKnobs; i++)
    if (a.knobs[i] != b.knobs[i]) return false;
  return true;
}

struct CommitPlan {
  bool full = true;
  uint64_t d_first = 0;      // the tokenizers take documents [d_first, n_staged)
};

// built / tok_docs: the build target's signature and the staged documents its
// rows cover (0: nothing kept — a new snapshot, or one a failed commit left);
// now: this commit's, with the seed of its first attempt.  full_knob: the value
// of TFIDF_FULL_COMMIT (nullptr = unset).
inline CommitPlan commit_plan(const CommitSig &built, uint64_t tok_docs, const CommitSig &now, uint64_t n_staged,
                              const char *full_knob) {
  CommitPlan p;
  const bool forced = full_knob && *full_knob && !(full_knob[0] == '0' && !full_knob[1]);
  if (forced || tok_docs == 0 || tok_docs > n_staged || now.n_dead != 0 || built.n_dead != 0 ||
      !commit_sig_equal(built, now))
    return p;
  p.full = false;
  p.d_first = tok_docs;
  return p;
}

// Malformed document ids: the kept ascending list takes the new build's
// (any order; in practice all above the kept ones) and stays ascending.
inline void merge_malformed(std::vector<uint32_t> *kept, const uint32_t *fresh, uint64_t n) {
  const size_t k = kept->size();
  kept->insert(kept->end(), fresh, fresh + n);
  std::sort(kept->begin() + k, kept->end());
  std::inplace_merge(kept->begin(), kept->begin() + k, kept->end());
}

// CSR escape list: the device counter starts at the kept count, so the new
// entries land behind the kept sorted ones.  counter = its value after the
// tokenizers (it keeps counting past cap; entries past cap were not written).
struct EscAppend {
  uint64_t first = 0, count = 0;   // new entries: [first, first + count) of the device list
  bool overflow = false;
};
inline EscAppend esc_append_bounds(uint64_t kept, uint64_t counter, uint64_t cap) {
  EscAppend a;
  a.first = kept;
  a.overflow = counter > cap || counter < kept;
  a.count = a.overflow ? 0 : counter - kept;
  return a;
}

// the kept sorted escapes with the new ones behind them (already in list[kept ..]): sorted as a whole
inline void esc_merge(std::vector<uint64_t> *list, uint64_t kept) {
  std::sort(list->begin() + std::min<uint64_t>(kept, list->size()), list->end());
  std::inplace_merge(list->begin(), list->begin() + std::min<uint64_t>(kept, list->size()), list->end());
}

// ---------------------------------------------------------------------------
// Incremental inversion (block-major): the blocks a snapshot's kept blk rows,
// bbase and post cover, and how those rows move to a wider column layout.

#if defined(__HIPCC__) || defined(__HIP__)
#define TFIDF_PLAN_HD __host__ __device__ __forceinline__
#else
#define TFIDF_PLAN_HD inline
#endif

constexpr uint64_t kPlanBlockDocs = 8192;     // = kBlockDocs (tfidf_common.h; checked where both are seen)

struct InversionPlan {
  uint32_t first_block = 0;   // blocks [first_block, n_blocks) are inverted; [0, first_block) are kept
  bool remap = false;         // the kept blk rows were laid out for another column count
};

// full: the commit plan's (a full build keeps nothing).  inv_docs / NC_inv:
// the staged documents the target's blk / bbase / post were built from (0:
// nothing kept) and the column count its blk rows were laid out for.  N, NC:
// this commit's.  full_knob: the value of TFIDF_FULL_INVERSION (nullptr =
// unset; an A/B switch outside the CommitSig: nothing kept depends on it).
// Only blocks every document of which was inverted before are kept; a partial
// tail block is inverted again even when no document was added.
inline InversionPlan inversion_plan(bool full, bool term_major, uint64_t inv_docs, uint64_t N, uint32_t NC,
                                    uint32_t NC_inv, const char *full_knob) {
  InversionPlan p;
  const bool forced = full_knob && *full_knob && !(full_knob[0] == '0' && !full_knob[1]);
  if (full || term_major || forced || inv_docs > N) return p;
  p.first_block = (uint32_t)(inv_docs / kPlanBlockDocs);
  // under a kept signature the dictionary only gains slots: the occupied-slot
  // set changed if and only if its size did
  p.remap = p.first_block > 0 && NC != NC_inv;
  return p;
}

// A kept row in the new column layout.  Slot s = 32 w + bit is occupied now
// and is new column c; (old_bits, old_base) = the crank word w the row was
// laid out by.  old = the occupied old slots below s: the slot's old column
// when it was occupied then, else the old column that follows it.
TFIDF_PLAN_HD uint32_t remap_old_col(uint32_t old_bits, uint32_t old_base, uint32_t bit) {
  return old_base + (uint32_t)__builtin_popcount(old_bits & ((1u << bit) - 1u));
}
// ... and the row's value at c: the old offset, or for a slot behind the last
// old column the block's posting total.  A column new to the block is an
// empty segment at the offset of the next old column.
TFIDF_PLAN_HD uint32_t remap_row_value(const uint32_t *old_row, uint32_t NC_inv, uint32_t block_total, uint32_t old) {
  return old < NC_inv ? old_row[old] : block_total;
}

// The kept df base (Snapshot::df_base): per column the sum of the counts of
// the blocks that were full at the snapshot's last inversion, so that a
// commit's df is the base plus the rows it inverts and no kept row is read.
// The base is valid exactly when the kept rows are: it is trusted if and only
// if inversion_plan keeps blocks (first_block > 0), and it then covers blocks
// [0, first_block), because the last successful commit left it at
// inv_docs / 8192 blocks and first_block is that number.  Every path that
// inverts from block 0 (a failed build before, TFIDF_FULL_COMMIT,
// TFIDF_FULL_INVERSION, dead documents, an epoch change, a seed retry, a new
// snapshot) rebuilds it from nothing in the same pass.
struct DfBasePlan {
  bool trusted = false;       // df_base holds blocks [0, base_before) (after the remap, in this commit's columns)
  uint32_t base_before = 0;   // blocks the base covers when the commit begins (0: untrusted, it starts from 0)
  uint32_t base_after = 0;    // ... and when it ends: the blocks that are full now, N / 8192
  uint32_t fold_first = 0, fold_end = 0;   // the inverted rows [fold_first, fold_end) are added to the base
  bool remap = false;         // the base moves to the new column layout with the kept rows
  bool from_rows = false;     // df of the kept blocks summed from their rows, as before the base (A/B); the base is kept up all the same
};

// inv: this commit's inversion plan; N: its documents; rows_knob: the value of
// TFIDF_DF_FROM_ROWS (nullptr = unset; an A/B switch outside the CommitSig:
// the base is maintained under either value, so nothing kept depends on it).
inline DfBasePlan df_base_plan(const InversionPlan &inv, bool term_major, uint64_t N, const char *rows_knob) {
  DfBasePlan p;
  if (term_major) return p;
  p.trusted = inv.first_block > 0;
  p.base_before = inv.first_block;
  p.base_after = (uint32_t)(N / kPlanBlockDocs);
  p.fold_first = inv.first_block;
  p.fold_end = std::max(p.base_after, inv.first_block);   // (first_block <= N / 8192: inversion_plan keeps nothing when inv_docs > N)
  p.remap = inv.remap;
  p.from_rows = p.trusted && rows_knob && *rows_knob && !(rows_knob[0] == '0' && !rows_knob[1]);
  return p;
}

// The base in the new column layout (arguments as remap_old_col's).  It is in
// count form: a column new to the layout has no posting in a kept block and
// gets 0, where a kept row takes the offset of the next old column.
TFIDF_PLAN_HD uint32_t remap_base_value(const uint32_t *old_base, uint32_t old_bits, uint32_t old_base_col, uint32_t bit) {
  return (old_bits >> bit) & 1u ? old_base[remap_old_col(old_bits, old_base_col, bit)] : 0u;
}

// Posting escapes ((posting index << 24) | tf, sorted): the entries of the
// kept blocks are those with a posting index below post_base = bbase[first_block].
inline uint64_t post_esc_keep(const std::vector<uint64_t> &sorted, uint64_t post_base) {
  return (uint64_t)(std::lower_bound(sorted.begin(), sorted.end(), post_base << 24) - sorted.begin());
}

// ---------------------------------------------------------------------------
// The inversion's launch shape when few blocks are inverted (an incremental
// commit's tail block, a small shard).  One workgroup per (block, range) tile
// and one per block row leave a 256-CU device idle, so a tile's documents are
// cut into slices (one workgroup each: k_df_partial<true>, k_scatter_part<true>)
// and a row's columns into parts (k_row_scan_parts).  Nothing that is kept
// depends on the shape: the published index is the same under every one.

constexpr uint32_t kSliceGroupDocs = 48;      // a slice is a multiple of every loader's document group (4 Q, Q = 1 .. 4)
// Documents per slice, at least (DESIGN.md §6 "Sliced tiles" has the sweep):
// one round of k_scatter_part's sixteen waves (16 x 12 documents).  Below it a
// slice's fixed cost (LDS clear, stream bases, the walk over the range's crank
// words) is no longer paid for by the shorter document loop.
constexpr uint32_t kSliceMinDocs = 192;
constexpr uint32_t kSliceWgsPerCu = 2;        // k_scatter_part (60 KiB of LDS); k_df_partial at 128 KiB runs one
constexpr uint32_t kScanPartCols = 16384;     // columns of one k_row_scan round: a part is never narrower (unless forced)
constexpr uint32_t kScanPartAlign = 256;      // a part starts on a k_df_sum workgroup's first column
constexpr uint32_t kSliceKnobMax = 256, kScanKnobMax = 64;
// k_scatter_sort takes kSortSpw of a range's 64 streams per workgroup in turn (its regions stay L2-resident in
// a full build); with few blocks that leaves 16 workgroups per (block, range), so it takes fewer, down to one,
// until the grid holds two workgroups per CU (1 / 2 / 4 measured on a lone tail block)
constexpr uint32_t kSortSpw = 4, kSortStreams = 64, kSortWgsPerCu = 2;

struct SlicePlan {
  uint32_t slices = 1;                        // document slices per (block, range) tile
  uint32_t slice_docs = (uint32_t)kPlanBlockDocs;   // slice i of block b: documents [b 8192 + i slice_docs, + slice_docs) of the block
  uint32_t scan_parts = 1;                    // workgroups per block row in the row scan
  uint32_t scan_width = 0;                    // part j: columns [j scan_width, + scan_width) below NC (scan_parts > 1)
  uint32_t sort_spw = 4;                      // k_scatter_sort: sub-range streams per workgroup (TFIDF_SORT_SPW overrides)
};

// blocks: the blocks to invert (n_blocks - first_block); max_docs: the
// documents of the largest of them; cus: the device's compute units.
// slices_knob / parts_knob: TFIDF_TEST_INV_SLICES / TFIDF_TEST_SCAN_PARTS
// (nullptr = unset), which force either number (a forced slice count may
// leave slices without documents, a forced part count parts without columns).
inline SlicePlan slice_plan(uint32_t blocks, uint32_t R, uint64_t max_docs, uint32_t NC, uint32_t cus,
                            const char *slices_knob, const char *parts_knob) {
  SlicePlan p;
  if (blocks == 0 || R == 0) return p;        // nothing is inverted: no tile kernel, no row scan
  while (p.sort_spw > 1 && (uint64_t)blocks * R * (kSortStreams / p.sort_spw) < (uint64_t)cus * kSortWgsPerCu)
    p.sort_spw /= 2;
  max_docs = std::min<uint64_t>(std::max<uint64_t>(max_docs, 1), kPlanBlockDocs);
  auto docs_for = [&](uint32_t s) {
    const uint64_t per = (max_docs + s - 1) / s;
    return (uint32_t)((per + kSliceGroupDocs - 1) / kSliceGroupDocs * kSliceGroupDocs);
  };
  if (slices_knob && *slices_knob) {
    p.slices = (uint32_t)std::max(1, std::min(atoi(slices_knob), (int)kSliceKnobMax));
    p.slice_docs = p.slices > 1 ? docs_for(p.slices) : (uint32_t)kPlanBlockDocs;
  } else {
    // a grid that fills the device stays as it is; else slices until it does, each of kSliceMinDocs or more
    const uint64_t tiles = (uint64_t)blocks * R;
    const uint64_t by_grid = tiles >= cus ? 1 : (uint64_t)cus * kSliceWgsPerCu / tiles;
    const uint64_t by_docs = std::max<uint64_t>(1, max_docs / kSliceMinDocs);
    const uint32_t s = (uint32_t)std::min(by_grid, by_docs);
    if (s > 1) {
      p.slice_docs = docs_for(s);
      p.slices = (uint32_t)((max_docs + p.slice_docs - 1) / p.slice_docs);   // (rounding up to groups may have emptied the last ones)
      if (p.slices == 1) p.slice_docs = (uint32_t)kPlanBlockDocs;
    }
  }
  const uint32_t max_parts = std::max(1u, (uint32_t)(((uint64_t)NC + kScanPartCols - 1) / kScanPartCols));
  if (parts_knob && *parts_knob)
    p.scan_parts = (uint32_t)std::max(1, std::min(atoi(parts_knob), (int)kScanKnobMax));
  else
    p.scan_parts = std::min(max_parts, std::max(1u, cus / (2 * blocks)));     // many rows: one workgroup each, as ever
  if (p.scan_parts > 1) {
    const uint64_t per = std::max<uint64_t>(1, ((uint64_t)NC + p.scan_parts - 1) / p.scan_parts);
    p.scan_width = (uint32_t)((per + kScanPartAlign - 1) / kScanPartAlign * kScanPartAlign);
  }
  return p;
}

// documents [*lo, *hi) of slice i of a block that holds documents [d0, d1) (empty: *lo == *hi)
inline void slice_range(const SlicePlan &p, uint32_t i, uint64_t d0, uint64_t d1, uint64_t *lo, uint64_t *hi) {
  const uint64_t a = d0 + (uint64_t)i * p.slice_docs;
  *lo = std::min(a, d1);
  *hi = std::min(a + p.slice_docs, d1);
}
// columns [*lo, *hi) of part j of a row of NC columns
inline void scan_part_range(const SlicePlan &p, uint32_t j, uint32_t NC, uint64_t *lo, uint64_t *hi) {
  if (p.scan_parts <= 1) { *lo = 0; *hi = NC; return; }
  const uint64_t a = (uint64_t)j * p.scan_width;
  *lo = std::min<uint64_t>(a, NC);
  *hi = std::min<uint64_t>(a + p.scan_width, NC);
}

// ---------------------------------------------------------------------------
// A lone inverted block (an incremental commit's tail): count, df, row scan
// and block base in one launch (k_df_fused) instead of k_inv_zero, k_df_partial<true>,
// k_df_sum<true>, k_row_scan_parts and k_block_scan.  The slices of a range add
// their counts into a scratch row; the last of them to finish (a ticket per
// range) turns the range's columns into df and offsets.  Nothing a range needs
// comes from another range's counts: its first offset is the sum over the
// block's documents of the entries their rows hold before the range (rsplit).

// inv_blocks: n_blocks - first_block; sp: the commit's slice plan.  rows_knob /
// parts_knob / unfused_knob: TFIDF_DF_FROM_ROWS, TFIDF_TEST_SCAN_PARTS (a forced
// part count names k_row_scan_parts) and TFIDF_INV_UNFUSED (nullptr = unset; an
// A/B switch outside the CommitSig: the published index is the same either way).
inline bool fuse_plan(bool term_major, uint32_t inv_blocks, const SlicePlan &sp, const char *rows_knob,
                      const char *parts_knob, const char *unfused_knob) {
  auto on = [](const char *v) { return v && *v && !(v[0] == '0' && !v[1]); };
  if (term_major || inv_blocks != 1 || sp.slices < 2) return false;
  if (on(rows_knob) || on(unfused_knob)) return false;
  if (parts_knob && *parts_knob) return false;            // (as slice_plan reads it: any value forces)
  return true;
}

// The slices of the lone block that hold a document (docs >= 1 of them): each
// draws one ticket per range, so the one that draws this number - 1 is last.
inline uint32_t fuse_tickets(const SlicePlan &sp, uint64_t docs) {
  if (docs == 0 || sp.slice_docs == 0) return 0;
  return (uint32_t)std::min<uint64_t>(sp.slices, (docs + sp.slice_docs - 1) / sp.slice_docs);
}

// The scratch: [0, fuse_ctl_words(R)) control words (tickets [R], first offsets
// [R], the block total), then one count word per column.  The kernel finds it
// zero and leaves it zero, so it is zeroed only when it was just allocated or
// when the last fused commit is not known to have run to its end.
TFIDF_PLAN_HD uint32_t fuse_ctl_words(uint32_t R) { return (2 * R + 1 + 63) / 64 * 64; }
inline uint64_t fuse_scratch_words(uint32_t R, uint32_t NC) { return (uint64_t)fuse_ctl_words(R) + NC; }

struct FuseScratch {
  uint64_t words = 0;       // allocated (0: none yet)
  bool clean = false;       // every word is zero: set after a fused commit's last successful synchronisation
};
// need: this commit's fuse_scratch_words.  *grow: the buffer must be allocated
// anew (for at least `need` words).  Returns whether it must be zeroed before
// the launch.  The caller then marks the scratch dirty (fuse_scratch_launch)
// until the commit has synchronised without an error (fuse_scratch_done).
inline bool fuse_scratch_must_zero(const FuseScratch &s, uint64_t need, bool *grow) {
  *grow = need > s.words;
  return *grow || !s.clean;
}
inline void fuse_scratch_launch(FuseScratch *s, uint64_t words) { s->words = words; s->clean = false; }
inline void fuse_scratch_done(FuseScratch *s) { s->clean = true; }

// Host model of what a range's last slice computes (k_df_fused's finisher;
// tests/fuse_plan_check.cpp holds it against a scan of the whole row).
// rsplit[d R + r]: the entries of document d's row in ranges 0 .. r.
inline uint64_t fuse_range_start(const uint32_t *rsplit, uint64_t n_docs, uint32_t R, uint32_t r) {
  uint64_t s = 0;
  if (r)
    for (uint64_t d = 0; d < n_docs; d++) s += rsplit[d * R + r - 1];
  return s;
}
inline uint64_t fuse_block_total(const uint32_t *rsplit, uint64_t n_docs, uint32_t R) {
  uint64_t s = 0;
  for (uint64_t d = 0; d < n_docs; d++) s += rsplit[d * R + R - 1];
  return s;
}
// offsets[c0 .. c1) = start + the exclusive scan of counts[c0 .. c1); returns the offset behind the span
inline uint64_t fuse_range_offsets(const uint32_t *counts, uint32_t c0, uint32_t c1, uint64_t start, uint32_t *offsets) {
  for (uint32_t c = c0; c < c1; c++) {
    offsets[c] = (uint32_t)start;
    start += counts[c];
  }
  return start;
}

// ---------------------------------------------------------------------------
// Host mirrors of a block-major snapshot (h_dict: the dictionary's two key
// planes, h_df: df per slot, h_crank: the slot -> column words): how a commit
// brings each up to date.  A snapshot's mirrors match its device dictionary
// and per-slot df as of its last successful build (Snapshot::mir_ok); under a
// kept signature the dictionary only gains slots and df changes only for
// terms of the newly tokenized documents, so an incremental commit can move
// the changed slots alone.

enum MirrorForm : uint32_t { kMirrorNone = 0, kMirrorDelta = 1, kMirrorWhole = 2 };   // = TFIDF_MIRROR_* (tfidf.h)

// Dictionary: a delta entry is 24 bytes against 16 per slot of the whole
// copy, and the host writes each entry into two planes (apply_dict_delta:
// 5-9 ns per entry measured at 2^18 .. 2^21 slots, list in the kernel's
// nearly ascending order) where the whole copy moves a slot in ~0.3 ns (16
// bytes at the ~50 GB/s of a pinned copy).  The two meet near C / 20 new
// slots; the delta is taken up to C / 32.  A list of up to kDictDeltaMin
// entries (12 KB, < 4 us of host writes) costs less than the fixed latency of
// any copy, so it is taken whatever C is.  A commit that adds more (3 % of the
// slots, 12 % of a dictionary at its design load of 1/4) is a bulk load, and
// the whole copy is the right form.
constexpr uint32_t kDictDeltaDiv = 32;
constexpr uint32_t kDictDeltaMin = 512;
inline uint32_t dict_delta_max(uint32_t C) { return std::min(C, std::max(C / kDictDeltaDiv, kDictDeltaMin)); }
// df: an entry costs 8 bytes of copy and a near-sequential store (2-4 ns
// measured), and the list is copied after the commit's last synchronisation
// (its length is known only then): one more round trip, ~15 us, where the
// whole copy runs beside the scatter.  The whole copy of the smallest
// dictionary the benchmarks use (2^18 slots, 1 MB) takes ~20 us, so the list
// must stay short to win there: 4096 entries are 32 KB and ~10 us of host
// writes.  The cap also sizes the list buffer.
constexpr uint32_t kDfDeltaCap = 1u << 12;
// The changed-slot count is known only after the inversion, but it is at most
// the postings of the newly tokenized documents (new_nnz: each changes one
// slot's df, and postings of one term share a slot; Zipf text shares
// heavily).  The delta is tried up to 4 x cap postings; beyond that the list
// would likely overflow, and the whole copy is queued beside the inversion
// from the start, as in a full build.
constexpr uint32_t kDfDeltaTry = 4;

struct DictDelta {                 // one new dictionary slot and its key
  uint64_t slot, lo, hi;
};
struct DfDelta {                   // one slot whose df changed, and the new value
  uint32_t slot, df;
};

struct MirrorPlan {
  bool delta = false;              // the preconditions of a delta hold (else every mirror is copied whole)
  MirrorForm dict = kMirrorWhole, crank = kMirrorWhole, df = kMirrorWhole;
  uint32_t n_new = 0;              // new dictionary slots (dict == kMirrorDelta: the list's length)
};

// full / term_major / kept_inv: as for inversion_plan (kept_inv != 0: the
// target's last inversion succeeded, so crank_inv is the occupancy its
// mirrors were taken at).  mir_ok: the target's mirrors matched its device
// arrays when this commit began.  NC / NC_inv: occupied slots now and then.
// new_nnz: postings of the documents this commit tokenized.  df_cap: the df
// list's capacity (kDfDeltaCap unless a test lowers it).  full_knob:
// TFIDF_FULL_MIRROR (an A/B switch outside the CommitSig, as TFIDF_FULL_INVERSION).
inline MirrorPlan mirror_plan(bool full, bool term_major, uint64_t kept_inv, bool mir_ok, uint32_t C, uint32_t NC,
                              uint32_t NC_inv, uint64_t new_nnz, uint32_t df_cap, const char *full_knob) {
  MirrorPlan p;
  const bool forced = full_knob && *full_knob && !(full_knob[0] == '0' && !full_knob[1]);
  if (full || term_major || kept_inv == 0 || !mir_ok || forced || NC < NC_inv) return p;
  p.delta = true;
  p.n_new = NC - NC_inv;
  if (p.n_new == 0) p.dict = p.crank = kMirrorNone;
  else if (p.n_new <= dict_delta_max(C)) p.dict = kMirrorDelta;     // (crank: 8 bytes per 32 slots, whole)
  if (new_nnz == 0) p.df = kMirrorNone;                             // nothing tokenized: no df moved
  else if (new_nnz <= (uint64_t)df_cap * kDfDeltaTry) p.df = kMirrorDelta;
  return p;
}

// Per-slot df (k_df_slots) need not be rebuilt when the commit can prove it
// equal to the target's last build: that build succeeded and covered every
// document (kept_inv == N, so the rows inverted again hold the same counts),
// the columns are the same (no remap, no new slot), and the mirrors were valid
// and take nothing (mp.delta with df and dictionary kMirrorNone: nothing was
// tokenized).  Helps the commit that adds nothing only.  always_knob:
// TFIDF_DF_SLOTS_ALWAYS (A/B).
inline bool df_slots_kept(const MirrorPlan &mp, uint64_t kept_inv, uint64_t N, bool remap, uint32_t NC, uint32_t NC_inv,
                          const char *always_knob) {
  const bool forced = always_knob && *always_knob && !(always_knob[0] == '0' && !always_knob[1]);
  return !forced && mp.delta && mp.df == kMirrorNone && mp.dict == kMirrorNone && kept_inv != 0 && kept_inv == N &&
         !remap && NC == NC_inv;
}

// The lists applied to the mirrors (after the commit's error checks).  false:
// an entry names a slot >= C; nothing was written.
inline bool apply_dict_delta(uint64_t *h_dict, uint32_t C, const DictDelta *list, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (list[i].slot >= C) return false;
  for (uint64_t i = 0; i < n; i++) {
    h_dict[list[i].slot] = list[i].lo;
    h_dict[(size_t)C + list[i].slot] = list[i].hi;
  }
  return true;
}
inline bool apply_df_delta(uint32_t *h_df, uint32_t C, const DfDelta *list, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (list[i].slot >= C) return false;
  for (uint64_t i = 0; i < n; i++) h_df[list[i].slot] = list[i].df;
  return true;
}

}  // namespace tfidf
