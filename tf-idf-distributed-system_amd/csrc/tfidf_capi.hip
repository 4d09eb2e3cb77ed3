// tfidf_capi.hip — the C ABI (include/tfidf.h): index lifetime, corpus
// staging, commit orchestration, query analysis and result materialisation.
// All hot-path arithmetic runs in the kernels of kernels_*.hip; this file is
// the host runtime around them (memory, streams, events, error mapping).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/tfidf.h"
#include "analysis.h"
#include "commit_plan.h"
#include "compact_plan.h"
#include "compound_plan.h"
#include "compound_tree_plan.h"
#include "fuzzy_plan.h"
#include "fuzzy_search_plan.h"
#include "wildcard_plan.h"
#include "regex_plan.h"
#include "mlt_plan.h"
#include "phrase_plan.h"
#include "snippet_plan.h"
#include "tfidf_common.h"
#include "tfidf_internal.h"

namespace tfidf {
hipError_t add_u64(uint64_t *v, uint64_t n, uint64_t delta, hipStream_t s);
hipError_t sort_unique_keys128(const uint64_t *keys, uint64_t n, uint64_t *out, uint64_t *n_unique, hipStream_t s);
hipError_t slot_to_canon(const uint64_t *dict, uint32_t C, const uint64_t *canon, uint64_t n_canon,
                         uint32_t *canon_of_slot, hipStream_t s);
hipError_t scatter_df_canon(const uint32_t *df, const uint32_t *canon_of_slot, uint32_t C, uint32_t *out,
                            hipStream_t s);
hipError_t gather_df_canon(const uint32_t *dfc, const uint32_t *canon_of_slot, uint32_t C, uint32_t *gdf,
                           hipStream_t s);
hipError_t launch_compact_text(const uint8_t *src, uint8_t *dst, const CompactRun *runs, uint64_t n_runs,
                               uint64_t total, hipStream_t s);
}  // namespace tfidf

using namespace tfidf;

// ---------------------------------------------------------------------------
// errors

static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                                \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess) return fail(TFIDF_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                      __FILE__, __LINE__);                                           \
  } while (0)

// ---------------------------------------------------------------------------
// device buffers

struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  hipError_t reserve(size_t n) {
    if (n <= bytes && p) return hipSuccess;
    if (p) { hipFree(p); p = nullptr; bytes = 0; }
    if (n == 0) n = 16;
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  // scratch sized by the documents or postings of a shard that grows with every commit: an exact
  // reserve would free and allocate it again each time (hipFree waits for the device); 1/16 + 1 MiB
  // of slack makes that rare
  hipError_t reserve_slack(size_t n) {
    if (n <= bytes && p) return hipSuccess;
    if (reserve(n + n / 16 + (1u << 20)) == hipSuccess) return hipSuccess;
    hipGetLastError();                           // no room for the slack: the exact size
    return reserve(n);
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// pinned host array: the per-commit dictionary / df mirrors are copied at
// DMA rate instead of through pageable staging (4 MB at 2^18 slots, 128 MB at 2^23)
template <class T> struct PinnedVec {
  T *p = nullptr;
  size_t n = 0, cap = 0;
  PinnedVec() = default;
  PinnedVec(const PinnedVec &) = delete;
  PinnedVec &operator=(const PinnedVec &) = delete;
  ~PinnedVec() { if (p) hipHostFree(p); }
  hipError_t resize(size_t m) {
    if (m > cap) {
      if (p) hipHostFree(p);
      p = nullptr;
      cap = n = 0;
      hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), m * sizeof(T), hipHostMallocDefault);
      if (e != hipSuccess) { p = nullptr; return e; }
      cap = m;
    }
    n = m;
    return hipSuccess;
  }
  void clear() { n = 0; }
  hipError_t assign(size_t m, T v) {
    hipError_t e = resize(m);
    if (e == hipSuccess) for (size_t i = 0; i < m; i++) p[i] = v;
    return e;
  }
  T *data() { return p; }
  const T *data() const { return p; }
  size_t size() const { return n; }
  T &operator[](size_t i) { return p[i]; }
  const T &operator[](size_t i) const { return p[i]; }
};

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    hipGetDevice(&prev);
    if (prev != dev) hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    hipGetDevice(&cur);
    if (prev >= 0 && cur != prev) hipSetDevice(prev);
  }
};

// block-major rows are grouped into at most 64 dictionary ranges (the long
// path's per-range counters), i.e. C <= 64 x 32768
constexpr uint32_t kMaxBlockCapLog2 = 21;

enum { EV_START, EV_TOK, EV_L0, EV_LONG, EV_D0, EV_DF, EV_BSCAN, EV_CSCAN, EV_SCAT, EV_N };
enum { QEV_0, QEV_1, QEV_2, QEV_P0, QEV_P1, QEV_N };   // search timing events (per search context); P0 / P1: a whole phrase search

constexpr size_t kCoalesceMaxDefault = 8192;   // tfidf_search_coalesced: requests per batch

// device buffer with an owner's lifetime (freed on its device)
struct DevMem : DevBuf {
  int dev = 0;
  explicit DevMem(int d) : dev(d) {}
  DevMem(const DevMem &) = delete;
  DevMem &operator=(const DevMem &) = delete;
  ~DevMem() {
    if (p) { DeviceGuard g(dev); release(); }
  }
};

// Document keys (relative paths), append-only in chunks that never change
// once a published snapshot holds them: a snapshot keeps the chunk list it was
// committed with, the builder appends to its own last chunk (or starts a new
// one when a snapshot shares it).  Staged id -> chunk by binary search.
// A keyless document's key is its decimal ordinal: the number of documents
// staged before it since create, clear or load.  That is its staged id until
// tfidf_compact renumbers the staged ids; the ordinals stay (ord_first / ord).
struct KeyChunk {
  uint64_t first = 0;                // staged id of the chunk's first document
  uint64_t ord_first = 0;            // ordinal of document i = ord_first + i ...
  std::vector<uint64_t> ord;         // ... unless listed here (after a compaction left gaps)
  std::string arena;
  std::vector<uint64_t> off{0};
  std::vector<uint8_t> synth;        // 1 = key is the decimal ordinal
  uint64_t size() const { return synth.size(); }
  uint64_t ordinal(uint64_t i) const { return ord.empty() ? ord_first + i : ord[i]; }
};
struct KeyTable {
  std::vector<std::shared_ptr<KeyChunk>> ch;
  const KeyChunk &chunk_of(uint64_t st) const {
    size_t a = 0, z = ch.size();
    while (z - a > 1) {
      const size_t m = (a + z) / 2;
      if (ch[m]->first <= st) a = m; else z = m;
    }
    return *ch[a];
  }
  void key(uint64_t st, std::string *out) const {
    const KeyChunk &c = chunk_of(st);
    const uint64_t i = st - c.first;
    if (c.synth[i]) *out = std::to_string(c.ordinal(i));
    else out->assign(c.arena.data() + c.off[i], c.off[i + 1] - c.off[i]);
  }
  uint64_t key_len(uint64_t st) const {
    const KeyChunk &c = chunk_of(st);
    const uint64_t i = st - c.first;
    return c.synth[i] ? std::to_string(c.ordinal(i)).size() : c.off[i + 1] - c.off[i];
  }
  uint64_t ordinal(uint64_t st) const {
    const KeyChunk &c = chunk_of(st);
    return c.ordinal(st - c.first);
  }
  bool is_synth(uint64_t st) const {
    const KeyChunk &c = chunk_of(st);
    return c.synth[st - c.first] != 0;
  }
  // the builder's chunk to append the document of ordinal `ord` to (a new one
  // when a snapshot shares the last, or when its ordinals do not continue)
  KeyChunk &tail(uint64_t n_staged, uint64_t ord) {
    if (ch.empty() || ch.back().use_count() > 1 ||
        (ch.back()->ord.empty() && ch.back()->ord_first + ch.back()->size() != ord)) {
      ch.push_back(std::make_shared<KeyChunk>());
      ch.back()->first = n_staged;
      ch.back()->ord_first = ord;
    }
    if (!ch.back()->ord.empty()) ch.back()->ord.push_back(ord);
    return *ch.back();
  }
  // flat copies (persistence, compaction)
  void flatten(std::string *arena, std::vector<uint64_t> *off, std::vector<uint8_t> *synth,
               std::vector<uint64_t> *ord = nullptr) const {
    arena->clear();
    off->assign(1, 0);
    synth->clear();
    if (ord) ord->clear();
    for (const auto &c : ch) {
      for (uint64_t i = 0; i < c->size(); i++) {
        arena->append(c->arena, c->off[i], c->off[i + 1] - c->off[i]);
        off->push_back(arena->size());
        if (ord) ord->push_back(c->ordinal(i));
      }
      synth->insert(synth->end(), c->synth.begin(), c->synth.end());
    }
  }
  // a chunk's ordinals: a base when they are consecutive, else the list
  static void set_ordinals(KeyChunk *c, std::vector<uint64_t> &&ord) {
    if (ordinals_contiguous(ord)) {
      c->ord_first = ord.empty() ? 0 : ord[0];
      c->ord.clear();
    } else {
      c->ord = std::move(ord);
    }
  }
  // many small chunks (one per commit of a single upload): merge them into one
  void compact() {
    if (ch.size() <= 64) return;
    auto one = std::make_shared<KeyChunk>();
    std::vector<uint64_t> ord;
    flatten(&one->arena, &one->off, &one->synth, &ord);
    set_ordinals(one.get(), std::move(ord));
    ch.assign(1, one);
  }
};

// Statistics in force for BM25 (the shard's own, or GLOBAL from the node-level
// exchange).  Never edited once a search can see it: the GLOBAL setters
// publish a new view.
struct StatsView {
  int dev = 0;
  bool global = false;
  uint64_t doc_count = 0, sum_ttf = 0;   // docCount / sumTotalTermFreq in force
  PinnedVec<uint32_t> gdf;               // GLOBAL df per dictionary slot (host mirror)
  hipEvent_t gdf_ev = nullptr;           // gdf copied (set asynchronously by tfidf_set_global_df_device)
  bool gdf_pending = false;
  std::mutex gdf_mu;
  DevMem cache;                          // 256-entry BM25 norm cache (device)
  PinnedVec<float> h_cache;
  explicit StatsView(int d) : dev(d), cache(d) {
    DeviceGuard g(d);
    hipEventCreateWithFlags(&gdf_ev, hipEventDisableTiming);
  }
  ~StatsView() {
    DeviceGuard g(dev);
    if (gdf_ev) {
      hipEventSynchronize(gdf_ev);
      hipEventDestroy(gdf_ev);
    }
  }
  int wait_gdf();                        // the GLOBAL df mirror, before its first use
};

// One committed index: everything a search reads.  Published by tfidf_commit
// as a refcounted snapshot and never changed afterwards (only its `stats`
// pointer is replaced, under the index's snap_mu); a search holds a reference
// for its whole run, so a commit never waits for searches and a search never
// waits for a commit (the reference opens a DirectoryReader on the last commit
// per request, Worker.java:223, while uploads commit beside it, :136-139).
// A snapshot no search holds any more is rebuilt in place by a later commit.
struct Snapshot {
  int dev = 0;
  uint64_t generation = 0;
  uint32_t cap_log2 = 18, C = 0, range_shift = 15, R = 1, n_blocks = 0;
  uint64_t n_docs = 0, text_bytes = 0;
  bool term_major = false;
  std::vector<uint32_t> live_map;      // committed -> staged (empty = identity)
  KeyTable keys;                       // document keys of the staged ids
  std::shared_ptr<DevMem> text, offsets;   // the staged corpus it was built from
  DevMem dict, csr, csr_esc, post_esc, doc_len, doc_nuniq, doc_norm, rsplit, blk, bbase, post, row_off, toff, tdf;
  // block-major columns (kernels_index.hip col_rank): occupancy bits and
  // prefix counts per 32 slots, the per-slot df, and the host copy of crank
  DevMem crank, sdf;
  PinnedVec<uint2> h_crank;
  uint32_t NC = 0;                     // block-major columns (= num_terms)
  std::vector<uint32_t> malformed;     // ascending committed ids of documents that are not UTF-8
  std::vector<uint64_t> h_esc;         // CSR tf escapes, sorted (csr_put)
  std::vector<uint64_t> h_post_esc;    // block-major posting tf escapes, sorted (post_word)
  uint64_t hash_seed = 0;
  uint32_t hash_rebuilds = 0;
  // incremental commits (commit_plan.h): the staged documents dict, csr,
  // csr_esc, doc_len, doc_nuniq, doc_norm and rsplit cover, and what those
  // depend on.  0 while a build is in progress and after one that failed.
  uint64_t tok_docs = 0;
  CommitSig sig;
  // ... and the staged documents blk / bbase / post / post_esc were inverted
  // from (block-major; 0 as above), the column count blk's rows were laid out
  // for, the crank they were laid out by (crank and crank_inv trade places
  // before a commit's col_rank), a host copy of bbase, and the target a
  // remap writes the kept rows to (then swapped with blk)
  uint64_t inv_docs = 0;
  uint32_t NC_inv = 0;
  DevMem crank_inv, blk_alt;
  // ... and the df base (commit_plan.h df_base_plan): per column of blk's
  // layout, the counts of blocks [0, inv_docs / 8192), the blocks that were
  // full at the last inversion.  Valid exactly when the kept blk rows are
  // (inv_docs != 0 under the same signature); k_df_sum updates it in place,
  // which a failed commit's inv_docs = 0 makes harmless.  df_base_alt: the
  // target a remap writes it to (then swapped, as blk_alt).
  DevMem df_base, df_base_alt;
  PinnedVec<uint64_t> h_bbase;
  PinnedVec<uint64_t> h_dict;          // host mirrors for query analysis (pinned)
  PinnedVec<uint32_t> h_df;
  // h_dict, h_df and h_crank match dict, sdf and crank as of the last
  // successful build of this snapshot: cleared when a build begins, set at its
  // successful end.  Only then may the next build move deltas (mirror_plan).
  bool mir_ok = false;
  uint64_t doc_count = 0, sum_ttf = 0, nnz = 0, num_terms = 0, long_docs = 0;
  uint32_t pack_docs = 1;
  uint64_t pack_retried = 0, unicode_docs = 0, unicode_wave_docs = 0, long_chunked = 0;
  std::shared_ptr<StatsView> stats;    // replaced under tfidf_index::snap_mu
  std::unordered_map<uint32_t, std::string> term_cache;   // hashed slots' term strings (slot_term)
  std::mutex term_mu;
  // more-like-this: ClassicSimilarity idf of every df 0 .. n_docs (mlt_idf_table), built and uploaded on first use
  DevMem mlt_idf;
  std::vector<float> h_mlt_idf;
  bool mlt_ready = false;
  std::mutex mlt_mu;
  explicit Snapshot(int d)
      : dev(d), dict(d), csr(d), csr_esc(d), post_esc(d), doc_len(d), doc_nuniq(d), doc_norm(d), rsplit(d), blk(d),
        bbase(d), post(d), row_off(d), toff(d), tdf(d), crank(d), sdf(d), crank_inv(d), blk_alt(d), df_base(d),
        df_base_alt(d), mlt_idf(d) {}
  const uint32_t *df_dev() const { return term_major ? tdf.as<uint32_t>() : sdf.as<uint32_t>(); }   // per slot
  // what the scorers index a term's postings by: its column (block-major) or
  // its dictionary slot (term-major); the scorers' C is the matching count
  uint32_t col_of(uint32_t slot) const {
    if (term_major) return slot;
    const uint2 e = h_crank[slot >> 5];
    return e.y + (uint32_t)__builtin_popcount(e.x & ((1u << (slot & 31u)) - 1u));
  }
  uint32_t qcols() const { return term_major ? C : NC; }
  uint64_t staged_of(uint64_t doc) const { return live_map.empty() ? doc : live_map[doc]; }
};

// Per-search scratch: a stream (plus a side stream for the batch kernels'
// fork), timing events and buffers.  Searches take a context from the index's
// pool, so concurrent searches never share one.
struct SearchCtx {
  int dev = 0;
  hipStream_t own = nullptr, side = nullptr;
  hipEvent_t ev[QEV_N] = {};
  hipEvent_t q_ev[2] = {nullptr, nullptr};  // fork / join of the wave-unit kernel on `side`
  hipEvent_t q_in_ev = nullptr;             // the last upload out of q_host
  bool q_in_pending = false;
  bool q_rec_start = true;                  // run_scoring records QEV_0 (false: a later chunk of a batch)
  bool q_timing = true;
  DevMem q_in, q_out, cand, cand_n, out_doc, out_score, hits, hits_n, hits_c, hits_s, hits_P, ovf;
  DevMem hl_in, hl_cnt, hl_m, hl_s, hl_o;   // hit highlighting: plan, slice counts, matches, per-row ranges, packed output
  DevMem fz_in, fz_hs, fz_c, fz_tmp;        // fuzzy lookup: staged terms + counters, hashed slots, candidates, sort scratch
  DevMem fz_o;                              // fuzzy search: the selected expansions of a candidate chunk
  DevMem ph_in, ph_s, ph_o, ph_tmp;         // phrase search: phrases' keys / sequences / weights, per-row arrays, ordered hits, sort scratch
  DevMem ml_in, ml_c, ml_tmp;               // more-like-this: staged seeds + row extents + counters, candidates, sort scratch
  DevMem wc_bits, wc_cnt, wc_out, wc_len;   // wildcard union: pattern bitmaps, (pattern, block) counts, doc ids, matched rows' lengths
  DevMem rx_tab;                            // regex scan: the staged DFA tables of a scan chunk
  DevMem cq_in, cq_rows, cq_binned, cq_bins;   // compound queries: a chunk's offsets and occurs, its row entries, the binned entries, bin counts and cursors
  PinnedVec<uint32_t> q_host, q_res, q_cand_h;   // q_cand_h: fused single query's block candidates (host merge)
  std::vector<uint64_t> q_merge;
  std::vector<uint32_t> q_units;            // batch scoring units {q, b0, b1, 0} (run_scoring)
  uint32_t *res_doc = nullptr, *res_n = nullptr;
  float *res_score = nullptr;
  explicit SearchCtx(int d)
      : dev(d), q_in(d), q_out(d), cand(d), cand_n(d), out_doc(d), out_score(d), hits(d), hits_n(d), hits_c(d),
        hits_s(d), hits_P(d), ovf(d), hl_in(d), hl_cnt(d), hl_m(d), hl_s(d), hl_o(d), fz_in(d), fz_hs(d), fz_c(d),
        fz_tmp(d), fz_o(d), ph_in(d), ph_s(d), ph_o(d), ph_tmp(d), ml_in(d), ml_c(d), ml_tmp(d), wc_bits(d),
        wc_cnt(d), wc_out(d), wc_len(d), rx_tab(d), cq_in(d), cq_rows(d), cq_binned(d), cq_bins(d) {}
  int init() {
    DeviceGuard g(dev);
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&side, hipStreamNonBlocking) != hipSuccess)
      return fail(TFIDF_E_HIP, "hipStreamCreate failed");
    for (int i = 0; i < QEV_N; i++) hipEventCreate(&ev[i]);
    for (int i = 0; i < 2; i++) hipEventCreateWithFlags(&q_ev[i], hipEventDisableTiming);
    hipEventCreateWithFlags(&q_in_ev, hipEventDisableTiming);
    return TFIDF_OK;
  }
  ~SearchCtx() {
    DeviceGuard g(dev);
    if (own) hipStreamSynchronize(own);
    if (side) hipStreamSynchronize(side);
    for (int i = 0; i < QEV_N; i++) if (ev[i]) hipEventDestroy(ev[i]);
    for (int i = 0; i < 2; i++) if (q_ev[i]) hipEventDestroy(q_ev[i]);
    if (q_in_ev) hipEventDestroy(q_in_ev);
    if (side) hipStreamDestroy(side);
    if (own) hipStreamDestroy(own);
  }
};

struct tfidf_index {
  tfidf_config cfg;
  std::mutex mu;                     // writers: add_docs, commit, clear, load, the GLOBAL exchange
  hipStream_t stream = nullptr;      // the writers' stream (own_stream unless tfidf_set_stream)
  hipStream_t own_stream = nullptr;
  hipStream_t user_stream = nullptr; // tfidf_set_stream: searches run on it too (null also for the NULL stream)
  hipEvent_t ev[EV_N];
  // side stream for the dictionary's host mirror: its D2H copy overlaps the inversion
  hipStream_t copy_stream = nullptr;
  hipEvent_t mir_ev[3];            // [0] dictionary final (main stream), [1] mirror copied, [2] df final
  int num_cus = 256;

  // published snapshot (searches) and the one a commit may rebuild in place
  std::mutex snap_mu;
  std::shared_ptr<Snapshot> cur, spare;
  uint64_t generation = 0;           // successful commits so far

  // search contexts (one per concurrent search)
  std::mutex ctx_mu;
  std::vector<std::unique_ptr<SearchCtx>> ctx_free;
  std::atomic<bool> q_timing{true};  // record HIP events around each search (tfidf_set_query_timing)
  std::mutex ms_mu;
  float last_ms_scoring = 0, last_ms_total = 0;
  uint64_t last_hl_item_chunks = 0, last_hl_row_chunks = 0;   // of the last batched highlighting call (ms_mu)
  uint64_t last_fz_scan_chunks = 0, last_fz_cand_chunks = 0;  // of the last fuzzy term lookup (ms_mu)
  uint64_t last_ph_candidates = 0, last_ph_row_chunks = 0;    // of the last phrase search (ms_mu)
  uint64_t last_mlt_entries = 0, last_mlt_chunks = 0;         // of the last more-like-this call (ms_mu)
  uint64_t last_cq_entries = 0, last_cq_chunks = 0, last_cq_pairs = 0;   // of the last compound call (ms_mu)
  float last_cq_ms = 0;                                       // ... and its combine pass's device time
  uint64_t last_wc_scan_chunks = 0, last_wc_matches = 0, last_wc_union_chunks = 0;   // of the last wildcard call (ms_mu)
  uint64_t last_rx_scan_chunks = 0, last_rx_matches = 0, last_rx_union_chunks = 0, last_rx_table_bytes = 0;   // of the last regex call (ms_mu)

  // staged corpus (builder)
  std::shared_ptr<DevMem> text, offsets;   // offsets: u64[n_staged + 1]
  // corpus loader: two pinned host staging buffers, refilled while the other one's DMA runs
  void *stage[2] = {nullptr, nullptr};
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  uint64_t text_bytes = 0, n_staged = 0;
  std::vector<uint64_t> h_offsets{0};
  KeyTable keys;
  std::vector<uint8_t> staged_live;
  std::unordered_map<std::string, uint64_t> key_to_staged;
  uint64_t n_dead = 0;
  uint64_t dead_bytes = 0;             // staged text bytes of the dead documents
  // bumped whenever a staged document's id, text position or liveness may have
  // changed (clear, load, a compaction, live -> dead): rows a snapshot keeps
  // across commits are valid for one epoch only (CommitSig)
  uint64_t corpus_epoch = 0;
  uint64_t last_tok_docs = 0;          // documents the last commit's build tokenized (tfidf_commit_tokenized_docs)
  uint32_t last_tok_full = 1;          // ... and whether it was a full build
  // ... and the blocks its inversion kept / the published index holds, and whether the kept rows
  // were moved to another column layout (tfidf_commit_inverted_blocks)
  uint32_t last_inv_first = 0, last_inv_blocks = 0, last_inv_remap = 0;
  // ... and the launch shape it ran in (commit_plan.h slice_plan; tfidf_commit_inversion_shape)
  uint32_t last_inv_slices = 1, last_inv_scan_parts = 1;
  uint32_t last_inv_fused = 0;         // ... and whether a lone block took k_df_fused (fuse_plan; tfidf_commit_inversion_fused)
  // host side of the last commit (tfidf_commit_host_profile): points since prof_t0
  tfidf_host_profile prof{};
  std::chrono::steady_clock::time_point prof_t0;
  uint64_t next_ord = 0;               // documents staged since create / clear / load: the next keyless key
  uint32_t compact_pct = 0;            // tfidf_set_compact_threshold (0 = commit never compacts)
  uint64_t compactions = 0;            // tfidf_compact calls that reclaimed something (index lifetime)

  // build scratch (the commit in progress)
  uint32_t cap_log2 = 18;
  DevBuf d_live_map;
  DevBuf long_list, uni_list, counters, post_tmp;
  DevBuf retry_list;                   // packed wave path: documents deferred to the single-document pass
  DevBuf new_list;                     // incremental commit, one document per wave: [0] count, [1 ..] the new documents
  // delta mirrors (commit_plan.h): the device lists of new dictionary slots and of slots whose df changed, and
  // their pinned host copies (sized once for the largest list, so no commit reallocates pinned memory)
  DevBuf mir_dict_list, mir_df_list;
  DevBuf inv_aux;                      // sliced inversion (commit_plan.h slice_plan): the tiles' stream cursors, the rows' part totals
  DevBuf inv_fuse;                     // k_df_fused's tickets, first offsets and count row: zero between commits ...
  FuseScratch fuse_state;              // ... as far as the host knows (fuse_scratch_must_zero)
  PinnedVec<DictDelta> h_dict_delta;
  PinnedVec<DfDelta> h_df_delta;
  DevBuf bad_list;                     // documents that are not valid UTF-8 (indexed empty)
  uint64_t hash_seed = 0;              // KeyBuilder seed of the build (0 unless a collision was met)
  uint32_t hash_rebuilds = 0;          // builds redone for a hash collision in the last commit
  bool uni_first = false;              // the last commit's documents were mostly non-ASCII: UNI-first build
  uint32_t hash_floor = 0;             // first seed attempt of the next commit (tfidf_set_hash_attempt)
  uint32_t collision_doc = 0;          // a document of the last detected collision (diagnostics)
  // tfidf_search_coalesced: concurrent single top-k searches gathered into batches
  mutable std::mutex cq_mu;
  std::condition_variable cq_cv;
  std::vector<struct CoalesceReq *> cq;
  bool cq_leader = false;
  size_t cq_max = kCoalesceMaxDefault;  // requests per batch
  uint64_t cq_batches = 0, cq_queries = 0;
  std::atomic<uint64_t> unit_batches{0}, unit_count{0}, fused_queries{0};
  DevBuf verify_defer, lt_pos;
  DevBuf tvals, term_tmp, term_esc;     // term-major inversion: sort values, scratch, tf escapes
  DevBuf lt_keys, lt_cnt, lt_g;
  DevBuf pairs, pair_ub, chunk_list, chunk_docs, chunk_fail, uchunk;   // book-sized documents (chunk-parallel)
  PinnedVec<uint32_t> ldocs_h, pre_h;                            // their host staging
  PinnedVec<uint64_t> hctr_h;                                    // build counters read back after the tokenizers
  uint32_t lt_log2 = 0, lt_wgs = 64;   // lt_wgs: long-path workgroups always allowed
  tfidf_commit_timing timing{};

  // GLOBAL exchange (writers): canonical ids, record order -> slot, owner-side scratch
  DevBuf canon_of_slot;
  uint64_t n_canon = 0;
  DevBuf sent_slot, vcounts, vnu, vt_table, vt_sum, vt_rslot, gdf_dev;
  uint64_t n_sent = 0;
  // the statistics view a GLOBAL setter replaced, reused by the next one once
  // no search holds it (its pinned df mirror and device cache stay allocated)
  std::shared_ptr<StatsView> view_spare;
};

int StatsView::wait_gdf() {
  std::lock_guard<std::mutex> lk(gdf_mu);
  if (gdf_pending) {
    HIP_TRY(hipEventSynchronize(gdf_ev));
    gdf_pending = false;
  }
  return TFIDF_OK;
}

// the published snapshot and its statistics view (both null before the first commit)
static std::shared_ptr<Snapshot> current(tfidf_index *ix, std::shared_ptr<StatsView> *v = nullptr) {
  std::lock_guard<std::mutex> lk(ix->snap_mu);
  if (v) *v = ix->cur ? ix->cur->stats : nullptr;
  return ix->cur;
}
static std::shared_ptr<Snapshot> current(const tfidf_index *ix, std::shared_ptr<StatsView> *v = nullptr) {
  return current(const_cast<tfidf_index *>(ix), v);
}

// A search context from the pool (created on demand), returned on scope exit.
struct CtxLease {
  tfidf_index *ix;
  std::unique_ptr<SearchCtx> c;
  int rc = TFIDF_OK;
  explicit CtxLease(tfidf_index *x) : ix(x) {
    {
      std::lock_guard<std::mutex> lk(ix->ctx_mu);
      if (!ix->ctx_free.empty()) {
        c = std::move(ix->ctx_free.back());
        ix->ctx_free.pop_back();
      }
    }
    if (!c) {
      c.reset(new SearchCtx(ix->cfg.device));
      rc = c->init();
    }
    c->q_timing = ix->q_timing.load();
  }
  // A search returns its snapshot reference after its lease (declared later,
  // destroyed first): no kernel of a failed search may still read the
  // snapshot's buffers when a commit rebuilds that snapshot as its spare
  // (use_count() == 1).  Successful searches have synchronised already; an
  // error return (HIP_TRY, a failed preparation after earlier chunks were
  // queued) is drained here.
  ~CtxLease() {
    if (!c || rc) return;
    {
      DeviceGuard g(ix->cfg.device);
      const hipStream_t st = stream();
      if (hipStreamQuery(st) != hipSuccess) hipStreamSynchronize(st);
      if (c->side && hipStreamQuery(c->side) != hipSuccess) hipStreamSynchronize(c->side);
    }
    std::lock_guard<std::mutex> lk(ix->ctx_mu);
    ix->ctx_free.push_back(std::move(c));
  }
  hipStream_t stream() const { return ix->user_stream ? ix->user_stream : c->own; }
};

// ---------------------------------------------------------------------------

extern "C" const char *tfidf_version(void) { return "libtfidf 0.1.0 (gfx950)"; }
extern "C" const char *tfidf_last_error(void) { return g_err.c_str(); }

extern "C" int tfidf_config_init(tfidf_config *cfg) {
  if (!cfg) return fail(TFIDF_E_INVALID_ARG, "cfg is NULL");
  cfg->k1 = 1.2f;
  cfg->b = 0.75f;
  cfg->stats_mode = TFIDF_STATS_SHARD;
  cfg->device = 0;
  cfg->vocab_capacity_log2 = 18;
  cfg->max_token_len = 255;
  cfg->inversion = TFIDF_INVERSION_AUTO;
  return TFIDF_OK;
}

extern "C" int tfidf_create(const tfidf_config *cfg, tfidf_index **out) {
  if (!cfg || !out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (cfg->max_token_len != 255) return fail(TFIDF_E_INVALID_ARG, "only max_token_len = 255 is supported");
  uint32_t lg = cfg->vocab_capacity_log2 ? cfg->vocab_capacity_log2 : 18;
  if (lg < 10 || lg > 26) return fail(TFIDF_E_INVALID_ARG, "vocab_capacity_log2 must be in [10, 26]");
  if (lg > kMaxBlockCapLog2 && cfg->inversion == TFIDF_INVERSION_BLOCK)
    return fail(TFIDF_E_INVALID_ARG, "block-major inversion supports vocab_capacity_log2 <= %u", kMaxBlockCapLog2);
  // BM25Similarity(k1, b) throws on anything else: a negative or NaN k1 gives
  // negative or NaN scores, and every select and merge orders hits by the
  // unsigned bit pattern of the score (negated tests: NaN fails them too)
  if (!(std::isfinite(cfg->k1) && cfg->k1 >= 0.f))
    return fail(TFIDF_E_INVALID_ARG, "k1 must be finite and >= 0 (got %g)", (double)cfg->k1);
  if (!(cfg->b >= 0.f && cfg->b <= 1.f)) return fail(TFIDF_E_INVALID_ARG, "b must be in [0, 1] (got %g)", (double)cfg->b);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(TFIDF_E_NO_DEVICE, "no HIP device");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(TFIDF_E_NO_DEVICE, "device %d out of range", cfg->device);
  DeviceGuard g(cfg->device);
  tfidf_index *ix = new tfidf_index();
  ix->cfg = *cfg;
  ix->cfg.vocab_capacity_log2 = lg;
  ix->cap_log2 = lg;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) ix->num_cus = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&ix->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete ix;
    return fail(TFIDF_E_HIP, "hipStreamCreate failed");
  }
  ix->stream = ix->own_stream;
  if (const char *cm = knob("TFIDF_COALESCE_MAX")) ix->cq_max = std::max(1, atoi(cm));   // tests: small batches
  if (hipStreamCreateWithFlags(&ix->copy_stream, hipStreamNonBlocking) != hipSuccess) {
    hipStreamDestroy(ix->own_stream);
    delete ix;
    return fail(TFIDF_E_HIP, "hipStreamCreate failed");
  }
  for (int i = 0; i < EV_N; i++) hipEventCreate(&ix->ev[i]);
  for (int i = 0; i < 2; i++) hipEventCreateWithFlags(&ix->stage_ev[i], hipEventDisableTiming);
  for (int i = 0; i < 3; i++) hipEventCreateWithFlags(&ix->mir_ev[i], hipEventDisableTiming);
  ix->text = std::make_shared<DevMem>(cfg->device);
  ix->offsets = std::make_shared<DevMem>(cfg->device);
  hipError_t e = ix->offsets->reserve(64);
  if (e != hipSuccess) { delete ix; return fail(TFIDF_E_OOM, "hipMalloc offsets"); }
  uint64_t zero = 0;
  hipMemcpy(ix->offsets->p, &zero, 8, hipMemcpyHostToDevice);
  *out = ix;
  return TFIDF_OK;
}

extern "C" int tfidf_destroy(tfidf_index *ix) {
  if (!ix) return TFIDF_OK;
  DeviceGuard g(ix->cfg.device);
  hipStreamSynchronize(ix->stream);
  hipStreamSynchronize(ix->copy_stream);
  ix->cur.reset();
  ix->spare.reset();
  ix->ctx_free.clear();
  ix->text.reset();
  ix->offsets.reset();
  DevBuf *bufs[] = {&ix->d_live_map, &ix->long_list, &ix->uni_list, &ix->counters, &ix->retry_list, &ix->new_list, &ix->bad_list,
                    &ix->mir_dict_list, &ix->mir_df_list, &ix->inv_aux, &ix->inv_fuse,
                    &ix->post_tmp, &ix->lt_keys, &ix->lt_cnt, &ix->lt_g, &ix->lt_pos, &ix->verify_defer, &ix->pairs,
                    &ix->pair_ub, &ix->chunk_list, &ix->chunk_docs, &ix->chunk_fail, &ix->uchunk, &ix->canon_of_slot,
                    &ix->tvals, &ix->term_tmp, &ix->term_esc, &ix->sent_slot, &ix->vcounts, &ix->vnu, &ix->vt_table,
                    &ix->vt_sum, &ix->vt_rslot, &ix->gdf_dev};
  for (DevBuf *b : bufs) b->release();
  for (int i = 0; i < EV_N; i++) hipEventDestroy(ix->ev[i]);
  for (int i = 0; i < 2; i++) {
    if (ix->stage[i]) hipHostFree(ix->stage[i]);
    hipEventDestroy(ix->stage_ev[i]);
  }
  for (int i = 0; i < 3; i++) hipEventDestroy(ix->mir_ev[i]);
  hipStreamSynchronize(ix->own_stream);
  hipStreamDestroy(ix->copy_stream);
  hipStreamDestroy(ix->own_stream);
  delete ix;
  return TFIDF_OK;
}

// grow a device buffer shared with published snapshots: a new buffer with the
// first `keep` bytes copied (the snapshots keep the old one alive)
static int grow_shared(tfidf_index *ix, std::shared_ptr<DevMem> *buf, uint64_t need, uint64_t keep, bool zero) {
  if (need <= (*buf)->bytes) return TFIDF_OK;
  uint64_t cap = (*buf)->bytes ? (*buf)->bytes : (1ull << 20);
  while (cap < need) cap = cap + cap / 2 + (1ull << 20);
  auto nb = std::make_shared<DevMem>(ix->cfg.device);
  HIP_TRY(nb->reserve(cap));
  if (zero) HIP_TRY(hipMemsetAsync(nb->p, 0, cap, ix->stream));
  if ((*buf)->p && keep) HIP_TRY(hipMemcpyAsync(nb->p, (*buf)->p, keep, hipMemcpyDeviceToDevice, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  *buf = std::move(nb);
  return TFIDF_OK;
}

// grow the device corpus to hold `extra` more bytes (plus read slack)
static int grow_text(tfidf_index *ix, uint64_t extra) {
  return grow_shared(ix, &ix->text, ix->text_bytes + extra + 128, ix->text_bytes, true);
}

static int grow_offsets(tfidf_index *ix, uint64_t extra_docs) {
  return grow_shared(ix, &ix->offsets, (ix->n_staged + extra_docs + 1) * 8, (ix->n_staged + 1) * 8, false);
}

// Grow a buffer a snapshot owns alone (the commit's build target) with its
// first `keep` bytes kept: an incremental commit appends to the rows of the
// documents it does not tokenize again.  Geometric, so a shard that commits
// after every upload copies its rows rarely; keep == 0 is DevBuf::reserve.
static int grow_keep(tfidf_index *ix, DevMem *buf, uint64_t need, uint64_t keep) {
  if (!keep || !buf->p) {
    HIP_TRY(buf->reserve(need));
    return TFIDF_OK;
  }
  if (need <= buf->bytes) return TFIDF_OK;
  uint64_t cap = buf->bytes;
  while (cap < need) cap = cap + cap / 2 + (1ull << 20);
  DevMem nb(buf->dev);
  if (nb.reserve(cap) != hipSuccess) {          // no room for the slack: the exact size
    hipGetLastError();
    HIP_TRY(nb.reserve(need));
  }
  HIP_TRY(hipMemcpyAsync(nb.p, buf->p, std::min<uint64_t>(keep, buf->bytes), hipMemcpyDeviceToDevice, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  std::swap(buf->p, nb.p);
  std::swap(buf->bytes, nb.bytes);
  return TFIDF_OK;                              // (nb frees the old buffer)
}

// a staged document goes from live to dead (false: it was dead already)
static bool kill_staged(tfidf_index *ix, uint64_t st) {
  if (!ix->staged_live[st]) return false;
  ix->staged_live[st] = 0;
  ix->n_dead++;
  ix->corpus_epoch++;
  ix->dead_bytes += ix->h_offsets[st + 1] - ix->h_offsets[st];
  return true;
}

static void register_key(tfidf_index *ix, const uint8_t *k, uint64_t n, bool synth) {
  const uint64_t idx = ix->n_staged;
  KeyChunk &c = ix->keys.tail(idx, ix->next_ord++);
  if (!synth) {
    std::string key((const char *)k, n);
    auto it = ix->key_to_staged.find(key);
    if (it != ix->key_to_staged.end()) {       // updateDocument: delete-by-term, then add
      kill_staged(ix, it->second);
      it->second = idx;
    } else {
      ix->key_to_staged.emplace(std::move(key), idx);
    }
    c.arena.append((const char *)k, n);
  }
  c.off.push_back(c.arena.size());
  c.synth.push_back(synth ? 1 : 0);
  ix->staged_live.push_back(1);
}

// Corpus loader (replaces Worker.init's per-file
// Files.readString + IndexWriter feed, J/worker/Worker.java:77-86,198): host
// bytes are copied into one of two pinned staging buffers by a few host
// threads while the other buffer's DMA to HBM is in flight, so the PCIe link
// streams at DMA speed instead of through the runtime's pageable bounce path.
constexpr size_t kStageBytes = 32u << 20;

static void par_memcpy(uint8_t *dst, const uint8_t *src, size_t n) {
  const size_t kMinPer = 4u << 20;
  unsigned t = std::min<unsigned>(8, std::max(1u, std::thread::hardware_concurrency()));
  t = (unsigned)std::min<size_t>(t, std::max<size_t>(1, n / kMinPer));
  if (t <= 1) { memcpy(dst, src, n); return; }
  std::vector<std::thread> th;
  const size_t per = (n + t - 1) / t;
  for (unsigned i = 1; i < t; i++) {
    const size_t a = i * per, z = std::min(n, a + per);
    if (a < z) th.emplace_back([=] { memcpy(dst + a, src + a, z - a); });
  }
  memcpy(dst, src, std::min(n, per));
  for (auto &x : th) x.join();
}

static hipError_t h2d_staged(tfidf_index *ix, uint8_t *dst, const uint8_t *src, uint64_t n) {
  if (n < (1u << 20)) return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, ix->stream);
  for (int i = 0; i < 2; i++)
    if (!ix->stage[i]) {
      hipError_t e = hipHostMalloc(&ix->stage[i], kStageBytes, hipHostMallocDefault);
      if (e != hipSuccess) { ix->stage[i] = nullptr; return e; }
    }
  uint64_t off = 0;
  for (int c = 0; off < n; c++) {
    const int b = c & 1;
    const size_t sz = (size_t)std::min<uint64_t>(kStageBytes, n - off);
    hipError_t e = hipEventSynchronize(ix->stage_ev[b]);     // this buffer's previous DMA is done
    if (e != hipSuccess) return e;
    par_memcpy(static_cast<uint8_t *>(ix->stage[b]), src + off, sz);
    e = hipMemcpyAsync(dst + off, ix->stage[b], sz, hipMemcpyHostToDevice, ix->stream);
    if (e != hipSuccess) return e;
    e = hipEventRecord(ix->stage_ev[b], ix->stream);
    if (e != hipSuccess) return e;
    off += sz;
  }
  return hipSuccess;
}

extern "C" int tfidf_clear(tfidf_index *ix) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->cfg.device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  // The staged corpus restarts at offset 0: buffers a published snapshot (an
  // open reader, an in-flight search) still reads are replaced, not rewritten.
  if (ix->text.use_count() > 1) ix->text = std::make_shared<DevMem>(ix->cfg.device);
  if (ix->offsets.use_count() > 1) {
    auto no = std::make_shared<DevMem>(ix->cfg.device);
    HIP_TRY(no->reserve(64));
    HIP_TRY(hipMemsetAsync(no->p, 0, 8, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    ix->offsets = std::move(no);
  }
  ix->text_bytes = 0;
  ix->n_staged = 0;
  ix->corpus_epoch++;
  ix->h_offsets.assign(1, 0);
  ix->keys = KeyTable();
  ix->staged_live.clear();
  ix->key_to_staged.clear();
  ix->n_dead = 0;
  ix->dead_bytes = 0;
  ix->next_ord = 0;
  std::shared_ptr<Snapshot> old;
  {
    std::lock_guard<std::mutex> sl(ix->snap_mu);    // searches from now on: not committed
    old = std::move(ix->cur);
  }
  if (!ix->spare) ix->spare = std::move(old);       // buffers for the next commit
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// Persistence (the reference keeps a Lucene index in
// FSDirectory(lucene.index.path) and reopens it at start-up,
// J/worker/Worker.java:67-73).  What is stored is the staged corpus (text,
// offsets, document keys, liveness after replace-by-key) — the index
// structures are rebuilt by tfidf_commit on load: on MI355X the rebuild runs
// at tens of GB/s of corpus, faster than reading the derived structures
// (≈ 2x the corpus size) back from storage.
static const char kFileMagic[8] = {'T', 'F', 'I', 'D', 'F', 'I', 'X', '1'};

struct FileHeader {
  char magic[8];
  uint32_t version, reserved;
  float k1, b;
  int32_t stats_mode, inversion;
  uint32_t vocab_capacity_log2, pad;
  uint64_t n_staged, text_bytes, key_bytes, n_dead, meta_hash;
};

static uint64_t fnv1a(uint64_t h, const void *p, size_t n) {
  const uint8_t *c = static_cast<const uint8_t *>(p);
  for (size_t i = 0; i < n; i++) { h ^= c[i]; h *= 0x100000001B3ull; }
  return h;
}

static uint64_t meta_hash(const tfidf_index *ix, const std::string &arena, const std::vector<uint64_t> &koff,
                          const std::vector<uint8_t> &synth) {
  uint64_t h = 0xCBF29CE484222325ull;
  h = fnv1a(h, ix->h_offsets.data(), ix->h_offsets.size() * 8);
  h = fnv1a(h, koff.data(), koff.size() * 8);
  h = fnv1a(h, arena.data(), arena.size());
  h = fnv1a(h, synth.data(), synth.size());
  h = fnv1a(h, ix->staged_live.data(), ix->staged_live.size());
  return h;
}

extern "C" int tfidf_save(tfidf_index *ix, const char *path) {
  if (!ix || !path) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->cfg.device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  std::string key_arena;
  std::vector<uint64_t> key_off;
  std::vector<uint8_t> key_synth;
  std::vector<uint64_t> key_ord;
  ix->keys.flatten(&key_arena, &key_off, &key_synth, &key_ord);
  // Version 2 appends the keyless documents' ordinals (next_ord, ord[n_staged])
  // to the metadata.  Only an index whose keyless keys are no longer their
  // positions (tfidf_compact) needs it; every other index writes version 1.
  bool v2 = false;
  for (uint64_t i = 0; i < ix->n_staged; i++)
    if (key_synth[i] && (key_ord[i] != i || ix->next_ord != ix->n_staged)) { v2 = true; break; }
  FileHeader h{};
  memcpy(h.magic, kFileMagic, 8);
  h.version = v2 ? 2 : 1;
  h.k1 = ix->cfg.k1;
  h.b = ix->cfg.b;
  h.stats_mode = ix->cfg.stats_mode;
  h.inversion = ix->cfg.inversion;
  h.vocab_capacity_log2 = ix->cap_log2;
  h.n_staged = ix->n_staged;
  h.text_bytes = ix->text_bytes;
  h.key_bytes = key_arena.size();
  h.n_dead = ix->n_dead;
  h.meta_hash = meta_hash(ix, key_arena, key_off, key_synth);
  if (v2) {
    h.meta_hash = fnv1a(h.meta_hash, &ix->next_ord, 8);
    h.meta_hash = fnv1a(h.meta_hash, key_ord.data(), key_ord.size() * 8);
  }
  const std::string tmp = std::string(path) + ".tmp";
  FILE *f = fopen(tmp.c_str(), "wb");
  if (!f) return fail(TFIDF_E_INVALID_ARG, "cannot open %s for writing", tmp.c_str());
  bool ok = fwrite(&h, sizeof h, 1, f) == 1;
  ok = ok && fwrite(ix->h_offsets.data(), 8, ix->h_offsets.size(), f) == ix->h_offsets.size();
  ok = ok && fwrite(key_off.data(), 8, key_off.size(), f) == key_off.size();
  ok = ok && (key_arena.empty() || fwrite(key_arena.data(), 1, key_arena.size(), f) == key_arena.size());
  ok = ok && (ix->n_staged == 0 || fwrite(key_synth.data(), 1, ix->n_staged, f) == ix->n_staged);
  ok = ok && (ix->n_staged == 0 || fwrite(ix->staged_live.data(), 1, ix->n_staged, f) == ix->n_staged);
  if (v2) {
    ok = ok && fwrite(&ix->next_ord, 8, 1, f) == 1;
    ok = ok && fwrite(key_ord.data(), 8, key_ord.size(), f) == key_ord.size();
  }
  // corpus text: device -> pinned staging buffer -> file, chunk by chunk
  if (ok && ix->text_bytes) {
    if (!ix->stage[0]) {
      if (hipHostMalloc(&ix->stage[0], kStageBytes, hipHostMallocDefault) != hipSuccess) ix->stage[0] = nullptr;
    }
    if (!ix->stage[0]) { fclose(f); remove(tmp.c_str()); return fail(TFIDF_E_OOM, "pinned staging buffer"); }
    for (uint64_t off = 0; ok && off < ix->text_bytes; off += kStageBytes) {
      const size_t n = (size_t)std::min<uint64_t>(kStageBytes, ix->text_bytes - off);
      if (hipMemcpy(ix->stage[0], ix->text->as<uint8_t>() + off, n, hipMemcpyDeviceToHost) != hipSuccess) {
        fclose(f);
        remove(tmp.c_str());
        return fail(TFIDF_E_HIP, "copy of the corpus from the device failed");
      }
      ok = fwrite(ix->stage[0], 1, n, f) == n;
    }
  }
  ok = (fclose(f) == 0) && ok;
  if (!ok || rename(tmp.c_str(), path) != 0) {
    remove(tmp.c_str());
    return fail(TFIDF_E_INVALID_ARG, "write of %s failed", path);
  }
  return TFIDF_OK;
}

extern "C" int tfidf_add_docs(tfidf_index *ix, const uint8_t *utf8, const uint64_t *offsets, uint64_t n_docs,
                              const uint8_t *keys, const uint64_t *key_offsets);

extern "C" int tfidf_load(tfidf_index *ix, const char *path) {
  if (!ix || !path) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    if (ix->n_staged) return fail(TFIDF_E_STATE, "tfidf_load needs an empty index (tfidf_create / tfidf_clear)");
    ix->corpus_epoch++;
  }
  FILE *f = fopen(path, "rb");
  if (!f) return fail(TFIDF_E_INVALID_ARG, "cannot open %s", path);
  FileHeader h{};
  if (fread(&h, sizeof h, 1, f) != 1 || memcmp(h.magic, kFileMagic, 8) != 0 ||
      (h.version != 1 && h.version != 2)) {
    fclose(f);
    return fail(TFIDF_E_INVALID_ARG, "%s is not a tfidf index file (version 1 or 2)", path);
  }
  if (h.vocab_capacity_log2 != ix->cap_log2) {
    fclose(f);
    return fail(TFIDF_E_INVALID_ARG, "index file has vocab_capacity_log2 %u, this index %u", h.vocab_capacity_log2,
                ix->cap_log2);
  }
  // bit patterns: the saved index's scores are this index's only at the same floats
  if (memcmp(&h.k1, &ix->cfg.k1, sizeof(float)) != 0 || memcmp(&h.b, &ix->cfg.b, sizeof(float)) != 0) {
    fclose(f);
    return fail(TFIDF_E_INVALID_ARG, "index file has (k1, b) = (%.9g, %.9g), this index (%.9g, %.9g)", (double)h.k1,
                (double)h.b, (double)ix->cfg.k1, (double)ix->cfg.b);
  }
  const uint64_t n = h.n_staged;
  std::vector<uint64_t> offs(n + 1), koff(n + 1);
  std::string arena(h.key_bytes, '\0');
  std::vector<uint8_t> synth(n), live(n);
  bool ok = fread(offs.data(), 8, n + 1, f) == n + 1 && fread(koff.data(), 8, n + 1, f) == n + 1;
  ok = ok && (h.key_bytes == 0 || fread(&arena[0], 1, h.key_bytes, f) == h.key_bytes);
  ok = ok && (n == 0 || (fread(synth.data(), 1, n, f) == n && fread(live.data(), 1, n, f) == n));
  uint64_t next_ord = n;
  std::vector<uint64_t> ord;
  if (ok && h.version == 2) {          // ordinals: strictly increasing, below next_ord
    ord.resize(n);
    ok = fread(&next_ord, 8, 1, f) == 1 && (n == 0 || fread(ord.data(), 8, n, f) == n);
    for (uint64_t i = 0; ok && i < n; i++) ok = ord[i] < next_ord && (i == 0 || ord[i] > ord[i - 1]);
  }
  ok = ok && offs[0] == 0 && offs[n] == h.text_bytes && koff[0] == 0 && koff[n] == h.key_bytes;
  for (uint64_t i = 0; ok && i < n; i++) ok = offs[i + 1] >= offs[i] && koff[i + 1] >= koff[i];
  std::vector<uint8_t> text;
  if (ok) {
    text.resize(h.text_bytes);
    ok = h.text_bytes == 0 || fread(text.data(), 1, h.text_bytes, f) == h.text_bytes;
  }
  fclose(f);
  if (!ok) return fail(TFIDF_E_INVALID_ARG, "%s is truncated or corrupt", path);
  // stage every stored document (as if keyless), then restore keys and
  // liveness exactly as saved
  int rc = tfidf_add_docs(ix, n ? text.data() : nullptr, offs.data(), n, nullptr, nullptr);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(ix->mu);
  {
    auto one = std::make_shared<KeyChunk>();
    one->arena = arena;
    one->off.assign(koff.begin(), koff.end());
    one->synth = synth;
    if (h.version == 2) KeyTable::set_ordinals(one.get(), std::vector<uint64_t>(ord));
    ix->keys.ch.assign(1, one);
  }
  ix->next_ord = next_ord;
  ix->staged_live = live;
  ix->key_to_staged.clear();
  ix->n_dead = 0;
  ix->dead_bytes = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (!live[i]) { ix->n_dead++; ix->dead_bytes += offs[i + 1] - offs[i]; continue; }
    if (!synth[i]) ix->key_to_staged[std::string(arena, koff[i], koff[i + 1] - koff[i])] = i;
  }
  uint64_t mh = meta_hash(ix, arena, koff, synth);
  if (h.version == 2) {
    mh = fnv1a(mh, &next_ord, 8);
    mh = fnv1a(mh, ord.data(), ord.size() * 8);
  }
  if (ix->n_dead != h.n_dead || mh != h.meta_hash) {
    return fail(TFIDF_E_INVALID_ARG, "%s: metadata checksum mismatch", path);
  }
  return TFIDF_OK;
}

extern "C" int tfidf_add_docs(tfidf_index *ix, const uint8_t *utf8, const uint64_t *offsets, uint64_t n_docs,
                              const uint8_t *keys, const uint64_t *key_offsets) {
  if (!ix || (!utf8 && n_docs) || !offsets) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (keys && !key_offsets) return fail(TFIDF_E_INVALID_ARG, "keys without key_offsets");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->cfg.device);
  for (uint64_t i = 0; i < n_docs; i++)
    if (offsets[i + 1] < offsets[i]) return fail(TFIDF_E_INVALID_ARG, "offsets must be non-decreasing");
  const uint64_t nbytes = offsets[n_docs] - offsets[0];
  if (ix->n_staged + n_docs >= 0xFFFFFFF0ull) return fail(TFIDF_E_CAPACITY, "more than 2^32 documents per shard");
  int rc = grow_text(ix, nbytes);
  if (rc) return rc;
  rc = grow_offsets(ix, n_docs);
  if (rc) return rc;
  if (nbytes) HIP_TRY(h2d_staged(ix, ix->text->as<uint8_t>() + ix->text_bytes, utf8 + offsets[0], nbytes));
  std::vector<uint64_t> no(n_docs);
  for (uint64_t i = 0; i < n_docs; i++) no[i] = ix->text_bytes + (offsets[i + 1] - offsets[0]);
  if (n_docs)
    HIP_TRY(hipMemcpyAsync(ix->offsets->as<uint64_t>() + ix->n_staged + 1, no.data(), n_docs * 8,
                           hipMemcpyHostToDevice, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  for (uint64_t i = 0; i < n_docs; i++) {
    if (keys) register_key(ix, keys + key_offsets[i], key_offsets[i + 1] - key_offsets[i], false);
    else register_key(ix, nullptr, 0, true);
    ix->h_offsets.push_back(no[i]);
    ix->n_staged++;
  }
  ix->text_bytes += nbytes;                 // searches keep the last commit's snapshot
  return TFIDF_OK;
}

extern "C" int tfidf_add_docs_device(tfidf_index *ix, const void *d_utf8, const void *d_offsets, uint64_t n_docs,
                                     uint64_t total_bytes) {
  if (!ix || !d_offsets) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->cfg.device);
  if (ix->n_staged + n_docs >= 0xFFFFFFF0ull) return fail(TFIDF_E_CAPACITY, "more than 2^32 documents per shard");
  std::vector<uint64_t> ho(n_docs + 1);
  HIP_TRY(hipMemcpy(ho.data(), d_offsets, (n_docs + 1) * 8, hipMemcpyDeviceToHost));
  if (ho[n_docs] - ho[0] != total_bytes) return fail(TFIDF_E_INVALID_ARG, "total_bytes != offsets[n] - offsets[0]");
  int rc = grow_text(ix, total_bytes);
  if (rc) return rc;
  rc = grow_offsets(ix, n_docs);
  if (rc) return rc;
  if (total_bytes)
    HIP_TRY(hipMemcpyAsync(ix->text->as<uint8_t>() + ix->text_bytes, (const uint8_t *)d_utf8 + ho[0], total_bytes,
                           hipMemcpyDeviceToDevice, ix->stream));
  uint64_t *dst = ix->offsets->as<uint64_t>() + ix->n_staged + 1;
  HIP_TRY(hipMemcpyAsync(dst, (const uint64_t *)d_offsets + 1, n_docs * 8, hipMemcpyDeviceToDevice, ix->stream));
  HIP_TRY(add_u64(dst, n_docs, ix->text_bytes - ho[0], ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  for (uint64_t i = 0; i < n_docs; i++) {
    register_key(ix, nullptr, 0, true);
    ix->h_offsets.push_back(ix->text_bytes + (ho[i + 1] - ho[0]));
    ix->n_staged++;
  }
  ix->text_bytes += total_bytes;
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// Document lifecycle: delete by key, reclaim the dead documents, read a
// document back (IndexWriter.deleteDocuments; Lucene reclaims deletes when
// segments merge; the stored field of a hit).

// canonical decimal (no sign, no leading zero): a keyless document's key
static bool parse_ordinal(const std::string &k, uint64_t *out) {
  if (k.empty() || k.size() > 20 || (k[0] == '0' && k.size() > 1)) return false;
  uint64_t v = 0;
  for (char c : k) {
    if (c < '0' || c > '9') return false;
    const uint64_t d = (uint64_t)(c - '0');
    if (v > (~0ull - d) / 10) return false;
    v = v * 10 + d;
  }
  *out = v;
  return true;
}

// staged id of the document of ordinal `ord` (ordinals ascend with the staged ids)
static bool find_ordinal(const tfidf_index *ix, uint64_t ord, uint64_t *st) {
  uint64_t a = 0, z = ix->n_staged;
  while (a < z) {
    const uint64_t m = a + (z - a) / 2;
    if (ix->keys.ordinal(m) < ord) a = m + 1; else z = m;
  }
  if (a >= ix->n_staged || ix->keys.ordinal(a) != ord) return false;
  *st = a;
  return true;
}

extern "C" int tfidf_delete_docs(tfidf_index *ix, const uint8_t *keys, const uint64_t *key_offsets, uint64_t n_keys,
                                 uint64_t *n_deleted) {
  if (n_deleted) *n_deleted = 0;
  if (!ix || (n_keys && !key_offsets)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  for (uint64_t i = 0; i < n_keys; i++)
    if (key_offsets[i + 1] < key_offsets[i]) return fail(TFIDF_E_INVALID_ARG, "key_offsets must be non-decreasing");
  if (n_keys && !keys && key_offsets[n_keys] != key_offsets[0]) return fail(TFIDF_E_INVALID_ARG, "NULL keys");
  std::lock_guard<std::mutex> lk(ix->mu);
  uint64_t n = 0;
  for (uint64_t i = 0; i < n_keys; i++) {
    const uint64_t len = key_offsets[i + 1] - key_offsets[i];
    const std::string key(len ? (const char *)keys + key_offsets[i] : "", len);
    auto it = ix->key_to_staged.find(key);
    if (it != ix->key_to_staged.end()) {       // an explicit key: forgotten, a later add appends
      if (kill_staged(ix, it->second)) n++;
      ix->key_to_staged.erase(it);
      continue;
    }
    uint64_t ord = 0, st = 0;                  // a keyless document's decimal ordinal
    if (parse_ordinal(key, &ord) && find_ordinal(ix, ord, &st) && ix->keys.is_synth(st) && kill_staged(ix, st)) n++;
  }
  if (n_deleted) *n_deleted = n;
  return TFIDF_OK;
}

struct TimingEvents {
  hipEvent_t a = nullptr, b = nullptr;
  ~TimingEvents() {
    if (a) hipEventDestroy(a);
    if (b) hipEventDestroy(b);
  }
};

// tfidf_compact under ix->mu.  Everything that can fail happens before the
// first change to the index.
static int compact_locked(tfidf_index *ix, uint64_t *bytes_reclaimed, float *ms_device) {
  if (bytes_reclaimed) *bytes_reclaimed = 0;
  if (ms_device) *ms_device = 0.0f;
  if (!ix->n_dead) return TFIDF_OK;
  DeviceGuard g(ix->cfg.device);
  hipStream_t s = ix->stream;
  CompactPlan P;
  compact_plan(ix->staged_live.data(), ix->h_offsets.data(), ix->n_staged, &P);
  // New buffers: published snapshots, open readers and in-flight searches
  // share the old ones (with live_map and keys in the old staged ids).
  auto nt = std::make_shared<DevMem>(ix->cfg.device), no = std::make_shared<DevMem>(ix->cfg.device);
  DevMem runs(ix->cfg.device);
  const uint64_t tcap = (P.live_bytes + 128 + ((1ull << 20) - 1)) & ~((1ull << 20) - 1);
  const uint64_t ocap = std::max<uint64_t>(64, (P.n_live + 1) * 8);
  if (nt->reserve(tcap) != hipSuccess || no->reserve(ocap) != hipSuccess ||
      runs.reserve(P.runs.size() * sizeof(CompactRun)) != hipSuccess) {
    hipGetLastError();
    return fail(TFIDF_E_OOM, "tfidf_compact: no device memory for the compacted corpus (%llu bytes)",
                (unsigned long long)(tcap + ocap));
  }
  TimingEvents ev;
  HIP_TRY(hipEventCreate(&ev.a));
  HIP_TRY(hipEventCreate(&ev.b));
  // zero from the end of the live text to the capacity (the tokenizers read
  // into that slack); the kernel writes whole 16-byte chunks below z0
  const uint64_t z0 = (P.live_bytes + 15) & ~15ull;
  HIP_TRY(hipMemsetAsync(nt->as<uint8_t>() + z0, 0, tcap - z0, s));
  HIP_TRY(hipMemcpyAsync(no->p, P.new_offsets.data(), (P.n_live + 1) * 8, hipMemcpyHostToDevice, s));
  if (!P.runs.empty())
    HIP_TRY(hipMemcpyAsync(runs.p, P.runs.data(), P.runs.size() * sizeof(CompactRun), hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(ev.a, s));
  HIP_TRY(launch_compact_text(ix->text->as<uint8_t>(), nt->as<uint8_t>(), runs.as<CompactRun>(), P.runs.size(),
                              P.live_bytes, s));
  HIP_TRY(hipEventRecord(ev.b, s));
  HIP_TRY(hipStreamSynchronize(s));
  float ms = 0.0f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));

  // host tables: the live entries, in order; a fresh key table (snapshots share the old chunks)
  std::string arena;
  std::vector<uint64_t> koff, kord;
  std::vector<uint8_t> ksynth;
  ix->keys.flatten(&arena, &koff, &ksynth, &kord);
  auto one = std::make_shared<KeyChunk>();
  one->synth.reserve(P.n_live);
  for (uint64_t i = 0; i < ix->n_staged; i++) {
    if (!ix->staged_live[i]) continue;
    one->arena.append(arena, koff[i], koff[i + 1] - koff[i]);
    one->off.push_back(one->arena.size());
    one->synth.push_back(ksynth[i]);
  }
  KeyTable::set_ordinals(one.get(), compact_ordinals(ix->staged_live.data(), ix->n_staged, kord.data()));
  for (auto it = ix->key_to_staged.begin(); it != ix->key_to_staged.end();) {
    const uint64_t nw = P.old_to_new[it->second];
    if (nw == kCompactDead) it = ix->key_to_staged.erase(it);
    else { it->second = nw; ++it; }
  }
  ix->keys.ch.assign(1, one);
  ix->h_offsets = std::move(P.new_offsets);
  ix->staged_live.assign(P.n_live, 1);
  ix->n_staged = P.n_live;
  ix->text_bytes = P.live_bytes;
  ix->n_dead = 0;
  ix->dead_bytes = 0;
  ix->corpus_epoch++;                  // staged ids and text positions moved
  ix->text = std::move(nt);
  ix->offsets = std::move(no);
  ix->compactions++;
  if (bytes_reclaimed) *bytes_reclaimed = P.dead_bytes;
  if (ms_device) *ms_device = ms;
  return TFIDF_OK;
}

extern "C" int tfidf_compact(tfidf_index *ix, uint64_t *bytes_reclaimed, float *ms_device) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(ix->mu);
  return compact_locked(ix, bytes_reclaimed, ms_device);
}

extern "C" int tfidf_set_compact_threshold(tfidf_index *ix, uint32_t dead_pct) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  if (dead_pct > 100) return fail(TFIDF_E_INVALID_ARG, "dead_pct %u > 100", dead_pct);
  std::lock_guard<std::mutex> lk(ix->mu);
  ix->compact_pct = dead_pct;
  return TFIDF_OK;
}

// BM25 norm cache for the statistics in force (BM25Similarity.scorer, float ops)
static void norm_cache(float k1, float b, float avgdl, float *cache) {
  for (int i = 0; i < 256; i++) {
    volatile float len = (float)byte4_to_int((uint32_t)i);
    volatile float t1 = 1.0f - b;
    volatile float t2 = b * len;
    volatile float t3 = t2 / avgdl;
    volatile float t4 = t1 + t3;
    volatile float t5 = k1 * t4;
    cache[i] = 1.0f / t5;
  }
}

static float bm25_idf(uint64_t df, uint64_t doc_count) {
  const double x = ((double)((int64_t)doc_count - (int64_t)df) + 0.5) / ((double)df + 0.5);
  return (float)log(1.0 + x);
}

// BM25 norm cache of a statistics view (not yet visible to searches, or
// owned by the writer), uploaded on stream s.  sync = false: the caller
// guarantees no earlier upload out of v.h_cache is pending and orders the
// view's first use after this one (StatsView::gdf_ev).
static int upload_cache(const tfidf_config &cfg, StatsView &v, hipStream_t s, bool sync = true) {
  HIP_TRY(v.h_cache.resize(256));
  // the previous upload from the staging array must be done before it is rewritten
  if (sync) HIP_TRY(hipStreamSynchronize(s));
  float *c = v.h_cache.data();
  if (v.doc_count == 0) {
    for (int i = 0; i < 256; i++) c[i] = 0.0f;
  } else {
    const float avgdl = (float)((double)v.sum_ttf / (double)v.doc_count);
    norm_cache(cfg.k1, cfg.b, avgdl, c);
  }
  HIP_TRY(v.cache.reserve(256 * 4));
  HIP_TRY(hipMemcpyAsync(v.cache.p, c, 256 * 4, hipMemcpyHostToDevice, s));
  if (sync) HIP_TRY(hipStreamSynchronize(s));
  return TFIDF_OK;
}

static float ev_ms(tfidf_index *ix, int a, int b) {
  float ms = 0;
  hipEventElapsedTime(&ms, ix->ev[a], ix->ev[b]);
  return ms;
}

static float qev_ms(const SearchCtx &c, int a, int b) {
  float ms = 0;
  if (!c.q_timing) return -1.0f;                   // query timing off: not measured
  hipEventElapsedTime(&ms, c.ev[a], c.ev[b]);
  return ms;
}

static void set_last_ms(tfidf_index *ix, float scoring, float total) {
  std::lock_guard<std::mutex> lk(ix->ms_mu);
  ix->last_ms_scoring = scoring;
  ix->last_ms_total = total;
}

// The same for the routes that report a part they do not time, or a call without device work, as 0:
// with query timing off both values are -1, as after every other search (tfidf_set_query_timing).
static void set_route_ms_locked(tfidf_index *ix, float scoring, float total) {
  const bool timed = ix->q_timing.load();
  ix->last_ms_scoring = timed ? scoring : -1.0f;
  ix->last_ms_total = timed ? total : -1.0f;
}

static void set_route_ms(tfidf_index *ix, float scoring, float total) {
  std::lock_guard<std::mutex> lk(ix->ms_mu);
  set_route_ms_locked(ix, scoring, total);
}

// host time since tfidf_commit began (tfidf_commit_host_profile)
static double prof_ms(const tfidf_index *ix) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ix->prof_t0).count();
}
// a host wait of the commit for its stream, counted for tfidf_commit_host_profile
static hipError_t commit_sync(tfidf_index *ix, hipStream_t s) {
  ix->prof.stream_syncs++;
  return hipStreamSynchronize(s);
}

// One index build with ix->hash_seed; kRcCollision when two different terms
// met under one hashed key (tfidf_commit then rebuilds with another seed).
constexpr int kRcCollision = -1000;
constexpr int kRcNoPublish = -1001;             // TFIDF_DEBUG_STOP (profiling): the rows are incomplete
constexpr uint32_t kVerifyCap = 1u << 20;      // deferred hashed-key checks per build
// may_keep: the first attempt of a commit, which may keep the target's rows
// and dictionary and tokenize the documents behind them only (commit_plan.h);
// a seed retry is a full build.
static int commit_once(tfidf_index *ix, Snapshot &S, bool may_keep) {
  hipStream_t s = ix->stream;
  // what the target covers; it covers nothing until this build has succeeded
  const uint64_t kept_docs = S.tok_docs, kept_inv = S.inv_docs;
  const bool mir_was_ok = S.mir_ok;
  S.tok_docs = 0;
  S.inv_docs = 0;
  S.mir_ok = false;
  // live documents
  S.n_docs = ix->n_staged - ix->n_dead;
  S.live_map.clear();
  if (ix->n_dead) {
    S.live_map.reserve(S.n_docs);
    for (uint64_t i = 0; i < ix->n_staged; i++)
      if (ix->staged_live[i]) S.live_map.push_back((uint32_t)i);
    HIP_TRY(ix->d_live_map.reserve(S.n_docs * 4 + 4));
    HIP_TRY(hipMemcpyAsync(ix->d_live_map.p, S.live_map.data(), S.n_docs * 4, hipMemcpyHostToDevice, s));
  }
  const uint64_t N = S.n_docs;
  S.C = 1u << ix->cap_log2;
  const uint32_t C = S.C;
  S.n_blocks = (uint32_t)((N + kBlockDocs - 1) / kBlockDocs);
  const uint64_t row_cap = (ix->text_bytes + ix->n_staged) / 2 + 2;
  // Inversion layout: block-major needs a dense (blocks + 1) x C count table;
  // when that outgrows the CSR itself (huge vocabularies, SURVEY §8 cfg 5) the
  // postings are built term-major by a sort instead (kernels_term.hip).
  {
    const uint64_t blk_bytes = (uint64_t)(S.n_blocks + 1) * C * 4;
    if (ix->cfg.inversion == TFIDF_INVERSION_TERM) S.term_major = true;
    else if (ix->cfg.inversion == TFIDF_INVERSION_BLOCK) S.term_major = false;
    else {
      // Few (block, range) tiles of very long documents (a few hundred books,
      // SURVEY cfg 1): the block-major passes run one workgroup per tile and
      // starve; the sort-based term-major build is parallel in the postings.
      const uint64_t tiles = (uint64_t)S.n_blocks * (C < kRangeSlots ? 1u : C / kRangeSlots);
      const bool starved = tiles < ix->num_cus && ix->n_staged && ix->text_bytes / ix->n_staged >= (64u << 10);
      S.term_major = ix->cap_log2 > kMaxBlockCapLog2 || (blk_bytes > (1ull << 31) && blk_bytes > row_cap * 4) ||
                       starved;
    }
  }
  // CSR rows are grouped by dictionary range for the block-major passes only
  const uint32_t RS = S.term_major ? C : (C < kRangeSlots ? C : kRangeSlots);
  S.range_shift = 0;
  while ((1u << S.range_shift) < RS) S.range_shift++;
  S.R = C >> S.range_shift;

  // Full or incremental.  A document's row sits at csr_row_base of its own
  // staged id and offset, and its row, doc_len / doc_nuniq / doc_norm / rsplit
  // words and dictionary entries depend on its text and the signature only:
  // while the signature holds, the target keeps them and documents
  // [d_first, N) alone are tokenized.  The block-major inversion below then
  // keeps the blocks whose documents were all inverted before (inversion_plan).
  CommitSig sig;
  sig.epoch = ix->corpus_epoch;
  sig.hash_seed = ix->hash_seed;
  sig.n_dead = ix->n_dead;
  sig.cap_log2 = ix->cap_log2;
  sig.C = C;
  sig.range_shift = S.range_shift;
  sig.R = S.R;
  sig.term_major = S.term_major;
  for (int i = 0; i < kCommitKnobs; i++) sig.knobs[i] = knob_sig(knob(commit_knob_names()[i]));
  const CommitPlan plan = commit_plan(S.sig, may_keep ? kept_docs : 0, sig, ix->n_staged,
                                      knob(commit_knob_names()[kKnobFullCommit]));
  const uint64_t d_first = plan.full ? 0 : plan.d_first;
  const uint64_t kept_esc = plan.full ? 0 : S.h_esc.size();
  // an incremental block-major commit without new documents over a valid crank: the columns are those of
  // the target's last inversion
  const bool keep_rank = !plan.full && !S.term_major && kept_inv != 0 && N == d_first;
  ix->last_tok_docs = N - d_first;
  ix->last_tok_full = plan.full ? 1u : 0u;
  // the kept totals (the tokenizers' counters start at 0 and count the new documents)
  struct { uint64_t doc_count, sum_ttf, nnz, long_docs, long_chunked, unicode_docs, unicode_wave_docs, pack_retried; } kept{};
  if (!plan.full)
    kept = {S.doc_count, S.sum_ttf, S.nnz, S.long_docs, S.long_chunked, S.unicode_docs, S.unicode_wave_docs,
            S.pack_retried};
  else
    S.malformed.clear();

  HIP_TRY(S.dict.reserve((size_t)3 * C * 8));          // lo, hi, reference occurrence (dict_device.h); its size is in the signature
  HIP_TRY(ix->verify_defer.reserve((size_t)kVerifyCap * 16));
  // + 16: the inversion reads row segments in 16-byte pieces, and the piece
  // that holds the last row's last entry may end up to 12 bytes past it
  // (the kept prefixes: the rows, escapes and words of documents below d_first)
  const uint64_t kept_rows = d_first ? ((ix->h_offsets[d_first] + d_first) >> 1) : 0;   // csr_row_base(d_first)
  if (int rc = grow_keep(ix, &S.csr, row_cap * 4 + 16, kept_rows * 4)) return rc;
  // escapes: each needs tf >= the field's escape value, and a row holds at
  // most row_cap tokens in all, so this bounds their number
  const uint64_t esc_cap = row_cap / csr_esc_value(S.range_shift) + 64;
  if (int rc = grow_keep(ix, &S.csr_esc, esc_cap * 8, kept_esc * 8)) return rc;
  if (int rc = grow_keep(ix, &S.doc_len, N * 4 + 4, d_first * 4)) return rc;
  if (int rc = grow_keep(ix, &S.doc_nuniq, N * 4 + 4, d_first * 4)) return rc;
  if (int rc = grow_keep(ix, &S.doc_norm, N + 16, d_first)) return rc;
  if (int rc = grow_keep(ix, &S.rsplit, N * S.R * 4 + 4, d_first * S.R * 4)) return rc;
  HIP_TRY(ix->long_list.reserve_slack(N * 4 + 4));
  HIP_TRY(ix->uni_list.reserve_slack(N * 4 + 4));
  HIP_TRY(ix->counters.reserve(128));
  HIP_TRY(ix->bad_list.reserve_slack(N * 4 + 4));
  // Short-document corpora: the wave path indexes packs of consecutive
  // documents per window (about kPackBytes of text per pack; SURVEY cfg 5
  // shape: 6 documents of ~330 B).  TFIDF_PACK_DOCS overrides (tests).
  uint32_t pack = 1;
  {
    const uint64_t avg = ix->n_staged ? ix->text_bytes / ix->n_staged : 0;
    if (avg) pack = (uint32_t)std::min<uint64_t>(kPackMaxDocs, std::max<uint64_t>(1, kPackBytes / avg));
    if (const char *e = knob("TFIDF_PACK_DOCS")) pack = (uint32_t)std::max(1, std::min(atoi(e), (int)kPackMaxDocs));
    pack = std::min(pack, std::max(1u, kWaveGroups / S.R));   // (document, range) groups per unit
  }
  if (pack > 1) HIP_TRY(ix->retry_list.reserve_slack(N * 4 + 4));
  if (S.term_major) {
    HIP_TRY(S.row_off.reserve(N * 4 + 4));
    HIP_TRY(S.toff.reserve(((size_t)C + 1) * 8));
    HIP_TRY(S.tdf.reserve((size_t)C * 4));
  } else {
    // (the count table blk is sized by the columns, known after the tokenizers)
    // (bbase is sized with blk below, once the kept blocks are known)
    HIP_TRY(S.crank.reserve(((size_t)C / 32 + 1) * 8));
    HIP_TRY(S.crank_inv.reserve(((size_t)C / 32 + 1) * 8));
    // the crank the kept blk rows were laid out by stays in crank_inv; col_rank writes the other buffer
    // (nothing tokenized: no kernel touches the dictionary, crank and NC stand and col_rank does not run)
    if (!keep_rank) {
      std::swap(S.crank.p, S.crank_inv.p);
      std::swap(S.crank.bytes, S.crank_inv.bytes);
    }
    HIP_TRY(S.sdf.reserve((size_t)C * 4));
  }

  // counters: [0..2] stats u64, [3] err flags u32 + [3].hi first doc, [4] long_count, [5] retry_count,
  // [6] uni_count, [7] occupied dictionary slots, [8] bad_count, [9] CSR escape count, [10] posting
  // escapes, [11] deferred hashed-key checks, [12] term-major tf escapes, [13] flagged documents
  // the wave rules took (k_tokenize_wave<UNI>)
  uint64_t *ctr = ix->counters.as<uint64_t>();
  HIP_TRY(hipMemsetAsync(ix->counters.p, 0, 128, s));
  if (plan.full) HIP_TRY(hipMemsetAsync(S.dict.p, 0, (size_t)3 * C * 8, s));
  // incremental: the escape counter starts behind the kept sorted escapes, so new ones are appended
  else if (kept_esc) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(ctr + 9), (int)(uint32_t)kept_esc, 1, s));
  // per-document Unicode flags.  UNI-first (the last commit's documents were
  // mostly non-ASCII, one document per wave): every document starts flagged
  // and k_tokenize_wave<UNI> takes ASCII ones as well, so the ASCII pass —
  // which would only read each such document to flag it — does not run
  // (cfg-2 prose: 0.8 ms)
  const char *nouw = knob("TFIDF_NO_UNIWAVE");
  const bool uni_on = !(nouw && *nouw && *nouw != '0');
  const bool uni_first = ix->uni_first && uni_on && pack == 1 && !knob("TFIDF_NO_UNIFIRST");
  // (the flag scans read all N flags: those of the kept documents stay 0; without new documents none runs)
  if ((!uni_first || d_first) && N > d_first) HIP_TRY(hipMemsetAsync(ix->uni_list.p, 0, (size_t)N * 4, s));
  if (uni_first && N > d_first)
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(ix->uni_list.as<uint32_t>() + d_first), 1, N - d_first, s));

  BuildParams bp{};
  bp.text = ix->text->as<uint8_t>();
  bp.offsets = ix->offsets->as<uint64_t>();
  bp.live_map = ix->n_dead ? ix->d_live_map.as<uint32_t>() : nullptr;
  bp.n_docs = N;
  bp.dict = S.dict.as<uint64_t>();
  bp.cap_mask = C - 1;
  bp.range_shift = S.range_shift;
  bp.n_ranges = S.R;
  bp.hash_seed = ix->hash_seed;
  bp.verify_defer = ix->verify_defer.as<uint64_t>();
  bp.verify_count = reinterpret_cast<uint32_t *>(ctr + 11);
  bp.verify_cap = kVerifyCap;
  bp.csr = S.csr.as<uint32_t>();
  bp.csr_esc = S.csr_esc.as<uint64_t>();
  bp.esc_count = reinterpret_cast<uint32_t *>(ctr + 9);
  bp.esc_cap = esc_cap;
  bp.doc_len = S.doc_len.as<uint32_t>();
  bp.doc_nuniq = S.doc_nuniq.as<uint32_t>();
  bp.doc_norm = S.doc_norm.as<uint8_t>();
  bp.rsplit = S.rsplit.as<uint32_t>();
  bp.long_list = ix->long_list.as<uint32_t>();
  bp.long_count = reinterpret_cast<uint32_t *>(ctr + 4);
  bp.uni_list = ix->uni_list.as<uint32_t>();
  bp.uni_count = reinterpret_cast<uint32_t *>(ctr + 6);
  bp.uni_wave_count = reinterpret_cast<uint32_t *>(ctr + 13);
  bp.bad_list = ix->bad_list.as<uint32_t>();
  bp.bad_count = reinterpret_cast<uint32_t *>(ctr + 8);
  bp.stats = reinterpret_cast<unsigned long long *>(ctr);
  bp.err = reinterpret_cast<uint32_t *>(ctr + 3);
  if (const char *ds = knob("TFIDF_DEBUG_STOP")) bp.debug_stop = (uint32_t)atoi(ds);   // profiling only
  if (const char *uf = knob("TFIDF_UW_FULL")) bp.debug_uw_full = (uint32_t)atoi(uf);   // A/B only
  bp.pack = pack;
  bp.retry_list = pack > 1 ? ix->retry_list.as<uint32_t>() : nullptr;
  bp.retry_count = reinterpret_cast<uint32_t *>(ctr + 5);
  S.pack_docs = pack;
  S.pack_retried = kept.pack_retried;

  HIP_TRY(hipEventRecord(ix->ev[EV_START], s));
  if (N > d_first) {                        // (nothing new: no tokenizer kernel runs)
    const uint64_t n_new = N - d_first;
    const uint64_t units = (n_new + pack - 1) / pack;
    uint64_t wpc = kWaveWGsPerCU;
    if (const char *e = knob("TFIDF_WAVE_WGS_PER_CU")) wpc = (uint64_t)std::max(1, atoi(e));   // profiling only
    const uint64_t grid = std::min<uint64_t>(units, (uint64_t)ix->num_cus * wpc);
    // incremental: the packs start at d_first (first_doc); the one-document
    // pass takes the new documents as a doc_list, as the retry pass takes its
    bp.first_doc = d_first;
    if (d_first && pack == 1 && !uni_first) {
      HIP_TRY(ix->new_list.reserve(n_new * 4 + 8));
      uint32_t *nl = ix->new_list.as<uint32_t>();
      HIP_TRY(launch_doc_range(nl + 1, nl, (uint32_t)d_first, (uint32_t)n_new, s));
      BuildParams np = bp;
      np.doc_list = nl + 1;
      np.doc_list_count = nl;
      HIP_TRY(launch_tokenize_wave(np, (int)grid, s));
    } else if (!uni_first) HIP_TRY(launch_tokenize_wave(bp, (int)grid, s));
    if (pack > 1 && !bp.debug_stop) {       // documents the packs could not take: one per wave
      uint32_t n_retry = 0;
      HIP_TRY(hipMemcpyAsync(&n_retry, ctr + 5, 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(commit_sync(ix, s));
      S.pack_retried = kept.pack_retried + n_retry;
      if (n_retry) {
        BuildParams rp = bp;
        rp.pack = 1;
        rp.doc_list = bp.retry_list;
        rp.doc_list_count = bp.retry_count;
        const uint64_t rgrid = std::min<uint64_t>(n_retry, (uint64_t)ix->num_cus * kWaveWGsPerCU);
        HIP_TRY(launch_tokenize_wave(rp, (int)rgrid, s));
      }
    }
    // documents with non-ASCII text (flags read on the device; both exit at once
    // when none): the wave rules with non-ASCII letters where the document's
    // characters allow (k_tokenize_wave<UNI>), then the Unicode wave path for
    // the rest.  TFIDF_NO_UNIWAVE: the Unicode wave path for all (A/B).
    if (bp.debug_stop < 10 && uni_on)
      HIP_TRY(launch_tokenize_wave_uni(bp, (int)std::min<uint64_t>((N + 63) / 64, (uint64_t)ix->num_cus * kWaveWGsPerCU), s));
    if (!bp.debug_stop || bp.debug_stop >= 10)          // (stops 10..13: the Unicode wave path's phases)
      HIP_TRY(launch_tokenize_uwave(bp, (int)std::min<uint64_t>(N, (uint64_t)ix->num_cus * kUwaveWGsPerCU), s));
  }
  HIP_TRY(hipEventRecord(ix->ev[EV_TOK], s));
  if (bp.debug_stop) {                      // profiling only: rows are incomplete, stop here
    HIP_TRY(commit_sync(ix, s));
    ix->timing = tfidf_commit_timing{};
    ix->timing.ms_tokenize = ev_ms(ix, EV_START, EV_TOK);
    ix->timing.ms_total = ix->timing.ms_tokenize;
    ix->timing.text_bytes = ix->text_bytes;
    ix->timing.num_docs = N;
    return kRcNoPublish;
  }
  // block-major: columns of the dictionary as it stands (final unless the
  // long path runs below, which recomputes them); their count lands in ctr[7]
  auto col_rank = [&]() -> int {
    if (!S.term_major && !keep_rank) {
      HIP_TRY(launch_col_rank(S.dict.as<uint64_t>(), C, S.crank.as<uint2>(),
                              reinterpret_cast<unsigned long long *>(ctr + 7), s));
      ix->prof.col_rank_runs++;
    }
    return TFIDF_OK;
  };
  if (int rc = col_rank()) return rc;
  // one read of the counters: stats (0-2), error flags (3), long (4) and
  // non-ASCII (6) document counts, columns (7), CSR escapes (9) (32-bit
  // counters in the low halves); read again only when the long path ran
  // pinned: a pageable read is staged by the runtime (and makes the copy call wait for the stream).
  // [0, 14): the counters after the tokenizers; [14, 27): the commit's last read (tail)
  HIP_TRY(ix->hctr_h.resize(14 + 13));
  uint64_t *hctr = ix->hctr_h.data();
  HIP_TRY(hipMemcpyAsync(hctr, ctr, 14 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(commit_sync(ix, s));
  ix->prof.ms_counters = prof_ms(ix);
  const uint32_t n_long = (uint32_t)hctr[4], n_uni = (uint32_t)hctr[6];
  S.long_chunked = kept.long_chunked;
  S.long_docs = kept.long_docs + n_long;
  S.unicode_docs = kept.unicode_docs + n_uni + (uint32_t)hctr[13];
  S.unicode_wave_docs = kept.unicode_wave_docs + (uint32_t)hctr[13];
  ix->uni_first = pack == 1 && (uint64_t)S.unicode_docs * 2 > N;
  if (n_long) {
    HIP_TRY(hipEventRecord(ix->ev[EV_L0], s));
    // book-sized documents: chunk-parallel (k_tokenize_chunk + k_long_rows),
    // in groups whose unit pair lists fit kPairBudget; documents a chunk
    // could not take come back in long_list for k_tokenize_long
    // pinned host buffers: pageable copies are staged synchronously by the runtime
    PinnedVec<uint32_t> &ldocs = ix->ldocs_h;
    HIP_TRY(ldocs.resize(n_long));
    HIP_TRY(hipMemcpyAsync(ldocs.data(), ix->long_list.p, (size_t)n_long * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(commit_sync(ix, s));
    // pair buckets: at most 64, each a whole number of k_long_rows' LDS windows
    const uint32_t wlog = std::min<uint32_t>(ix->cap_log2, kLrWinBits);
    const uint32_t bsh = std::max<uint32_t>(wlog, ix->cap_log2 > 6 ? ix->cap_log2 - 6 : 0);
    const uint32_t nb = 1u << (ix->cap_log2 - bsh);
    uint64_t unit_max = std::max<uint64_t>(1, kPairBudget / ((uint64_t)kPairWords * 4));
    if (const char *e = knob("TFIDF_TEST_PAIR_UNITS")) unit_max = std::max(1, atoi(e));   // tests: many groups
    // per group: the first unit (document, core) of each document, prefix form
    std::vector<uint32_t> pre;
    std::vector<uint64_t> gpre, gdoc;               // each group's prefix array offset and first document
    uint64_t acc = 0, max_units = 0;
    for (uint64_t i = 0; i < n_long; i++) {
      const uint64_t st = S.live_map.empty() ? ldocs[i] : S.live_map[ldocs[i]];
      const uint64_t L = ix->h_offsets[st + 1] - ix->h_offsets[st];
      const uint64_t units = (L + kLongCoreBytes - 1) / kLongCoreBytes;
      if (i == 0 || acc + units > unit_max) {
        if (i) { pre.push_back((uint32_t)acc); max_units = std::max(max_units, acc); }
        gpre.push_back(pre.size());
        gdoc.push_back(i);
        acc = 0;
      }
      pre.push_back((uint32_t)acc);
      acc += units;
      if (acc >= 0xFFFFFFFFull) return fail(TFIDF_E_CAPACITY, "too many document chunks");
    }
    pre.push_back((uint32_t)acc);
    max_units = std::max(max_units, acc);
    gdoc.push_back(n_long);
    HIP_TRY(ix->pairs.reserve(max_units * kPairWords * 4));
    HIP_TRY(ix->pair_ub.reserve(max_units * (nb + 1) * 4));
    HIP_TRY(ix->chunk_list.reserve(pre.size() * 4 + 8));
    HIP_TRY(ix->chunk_docs.reserve((size_t)n_long * 4));
    HIP_TRY(ix->chunk_fail.reserve((size_t)n_long * 4));
    HIP_TRY(ix->uchunk.reserve(max_units * 4 + 16));     // [0] count, [4 ..] per unit: non-ASCII text
    HIP_TRY(ix->pre_h.resize(pre.size()));
    memcpy(ix->pre_h.data(), pre.data(), pre.size() * 4);
    HIP_TRY(hipMemcpyAsync(ix->chunk_list.p, ix->pre_h.data(), pre.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ix->chunk_docs.p, ix->long_list.p, (size_t)n_long * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(ix->chunk_fail.p, 0, (size_t)n_long * 4, s));
    HIP_TRY(hipMemsetAsync(bp.long_count, 0, 4, s));                   // the fallback list restarts
    for (size_t gi = 0; gi < gpre.size(); gi++) {
      const uint64_t g0 = gdoc[gi], n = gdoc[gi + 1] - g0;
      BuildParams cp = bp;
      cp.chunk_pre = ix->chunk_list.as<uint32_t>() + gpre[gi];
      cp.n_group_docs = (uint32_t)n;
      cp.n_chunks = pre[gpre[gi] + n];
      cp.chunk_docs = ix->chunk_docs.as<uint32_t>() + g0;
      cp.chunk_fail = ix->chunk_fail.as<uint32_t>() + g0;
      cp.pairs = ix->pairs.as<uint32_t>();
      cp.pair_ub = ix->pair_ub.as<uint32_t>();
      cp.pair_bshift = bsh;
      cp.pair_nb = nb;
      // units with non-ASCII text: the Unicode chunk kernel (TFIDF_NO_UCHUNK: their
      // documents go to k_tokenize_long whole, as before round 4; A/B only)
      const bool uch = !knob("TFIDF_NO_UCHUNK");
      cp.uchunk_count = uch ? ix->uchunk.as<uint32_t>() : nullptr;
      cp.uchunk_list = uch ? ix->uchunk.as<uint32_t>() + 4 : nullptr;
      if (uch) HIP_TRY(hipMemsetAsync(ix->uchunk.p, 0, (size_t)(cp.n_chunks + 4) * 4, s));
      const uint64_t grid = std::min<uint64_t>(cp.n_chunks, (uint64_t)ix->num_cus * kWaveWGsPerCU);
      HIP_TRY(launch_tokenize_chunks(cp, (int)grid, s));
      // flagged units by the wave rules where their text allows (TFIDF_NO_UNIWAVE: all
      // of them to the Unicode chunk kernel; A/B only), then the rest
      const char *nouw = knob("TFIDF_NO_UNIWAVE");
      if (uch && !(nouw && *nouw && *nouw != '0')) HIP_TRY(launch_tokenize_chunks_uni(cp, (int)grid, s));
      if (uch)      // the count is read on the device: exits at once when no unit was listed
        HIP_TRY(launch_tokenize_uchunk(cp, (int)std::min<uint64_t>(cp.n_chunks, (uint64_t)ix->num_cus * kUchunkWGsPerCU), s));
      HIP_TRY(launch_long_rows(cp, (uint32_t)n, s));
    }
    uint32_t n_fb = 0;
    HIP_TRY(hipMemcpyAsync(&n_fb, bp.long_count, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(commit_sync(ix, s));
    S.long_chunked = kept.long_chunked + n_long - n_fb;
    if (n_fb) {
      uint32_t lg = ix->cap_log2 + 1;
      // table size needed by the longest long document (2x its token bound)
      uint64_t maxlen = 0;
      for (uint64_t d = 0; d < ix->n_staged; d++) maxlen = std::max(maxlen, ix->h_offsets[d + 1] - ix->h_offsets[d]);
      uint32_t need = 10;
      while (need < 22 && (1ull << need) < maxlen + 2) need++;
      lg = std::min(lg, need);
      ix->lt_log2 = lg;
      // one workgroup per long document, up to 2 per CU, within a scratch budget
      // (24 B per table slot per workgroup: key lo/hi, count, dictionary slot)
      const uint64_t per_wg = 24ull << lg;
      const uint64_t by_budget = std::max<uint64_t>(ix->lt_wgs, kLongScratchBudget / per_wg);
      const uint32_t wgs = (uint32_t)std::min<uint64_t>({(uint64_t)n_fb, (uint64_t)ix->num_cus * 2, by_budget});
      HIP_TRY(ix->lt_keys.reserve((size_t)wgs * 2 * (1ull << lg) * 8));
      HIP_TRY(ix->lt_cnt.reserve((size_t)wgs * (1ull << lg) * 4));
      HIP_TRY(ix->lt_pos.reserve((size_t)wgs * (1ull << lg) * 8));
      HIP_TRY(ix->lt_g.reserve((size_t)wgs * (1ull << lg) * 4));
      bp.lt_keys = ix->lt_keys.as<uint64_t>();
      bp.lt_cnt = ix->lt_cnt.as<uint32_t>();
      bp.lt_pos = ix->lt_pos.as<uint64_t>();
      bp.lt_g = ix->lt_g.as<uint32_t>();
      bp.lt_slots_log2 = lg;
      HIP_TRY(launch_tokenize_long(bp, (int)wgs, s));
    }
    HIP_TRY(hipEventRecord(ix->ev[EV_LONG], s));
    if (int rc = col_rank()) return rc;
    HIP_TRY(hipMemcpyAsync(hctr, ctr, 10 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(commit_sync(ix, s));
  }
  const uint32_t err = (uint32_t)(hctr[3] & 0xFFFFFFFFu), err_doc = (uint32_t)(hctr[3] >> 32);
  if (err & kErrCollision) { ix->collision_doc = err_doc; return kRcCollision; }
  if (err) {
    if (err & kErrCapacity)
      return fail(TFIDF_E_CAPACITY, "vocabulary exceeds 2^%u dictionary slots (raise vocab_capacity_log2)",
                  ix->cap_log2);
    return fail(TFIDF_E_UNSUPPORTED_INPUT, "index build error flags 0x%x (doc %u)", err, err_doc);
  }
  S.doc_count = kept.doc_count + hctr[0];
  S.sum_ttf = kept.sum_ttf + hctr[1];
  S.nnz = kept.nnz + hctr[2];
  S.NC = S.term_major ? 0u : keep_rank ? S.NC_inv : (uint32_t)hctr[7];
  // Statistics in force: the shard's own (a GLOBAL exchange publishes another
  // view).  doc_count and sum_ttf are final here, so the BM25 norm cache is
  // uploaded ahead of the inversion and the commit's last synchronisation
  // covers it.  The stream was synchronised by the counter read just above, so
  // no earlier upload out of the view's staging array is pending (wait_gdf:
  // nor one behind a GLOBAL setter's event), and the view's first use follows
  // the publish.  A build that fails below leaves a target that covers
  // nothing; its private view is never seen by a search.
  if (!S.stats || S.stats.use_count() > 1) S.stats = std::make_shared<StatsView>(ix->cfg.device);
  {
    StatsView &V = *S.stats;
    if (int rc = V.wait_gdf()) return rc;
    V.global = false;
    V.gdf.clear();
    V.doc_count = S.doc_count;
    V.sum_ttf = S.sum_ttf;
    if (int rc = upload_cache(ix->cfg, V, s, false)) return rc;
  }
  // Block-major: the blocks kept from the target's last inversion.  Their blk
  // rows (offset form), bases and postings depend on their own documents' rows
  // and norms and on the slot -> column map only; when the dictionary gained
  // slots, the kept rows move to the new column layout (k_blk_remap).
  const InversionPlan inv = inversion_plan(plan.full, S.term_major, kept_inv, N, S.NC, S.NC_inv,
                                           knob("TFIDF_FULL_INVERSION"));
  const uint32_t first_block = inv.first_block;
  // ... their df comes from the snapshot's df base, which takes the rows that are full now (df_base_plan)
  const DfBasePlan dbp = df_base_plan(inv, S.term_major, N, knob("TFIDF_DF_FROM_ROWS"));
  // ... and how the host mirrors follow (commit_plan.h): whole, or the new slots and changed df alone
  uint32_t df_cap = kDfDeltaCap;
  if (const char *e = knob("TFIDF_TEST_DF_DELTA_CAP")) df_cap = (uint32_t)std::max(1, std::min(atoi(e), (int)kDfDeltaCap));
  const MirrorPlan mp = mirror_plan(plan.full, S.term_major, kept_inv, mir_was_ok, C, S.NC, S.NC_inv, hctr[2], df_cap,
                                    knob("TFIDF_FULL_MIRROR"));
  // sdf stands when nothing it is made from changed (the commit that adds nothing)
  const bool keep_sdf = !plan.full && !S.term_major &&
                        df_slots_kept(mp, kept_inv, N, inv.remap, S.NC, S.NC_inv, knob("TFIDF_DF_SLOTS_ALWAYS"));
  // the fused delta kernel builds either list; it replaces k_df_slots only when one is wanted
  const bool dict_delta = mp.dict == kMirrorDelta, df_delta = mp.df == kMirrorDelta;
  const bool dict_whole = mp.dict == kMirrorWhole, df_whole = mp.df == kMirrorWhole, crank_whole = mp.crank == kMirrorWhole;
  if (dict_delta) {
    HIP_TRY(ix->mir_dict_list.reserve((size_t)dict_delta_max(C) * sizeof(DictDelta)));
    HIP_TRY(ix->h_dict_delta.resize(dict_delta_max(C)));
  }
  if (df_delta) {
    HIP_TRY(ix->mir_df_list.reserve((size_t)kDfDeltaCap * sizeof(DfDelta)));
    HIP_TRY(ix->h_df_delta.resize(kDfDeltaCap));
  }
  const uint64_t kept_post = first_block ? S.h_bbase[first_block] : 0;      // postings of the kept blocks
  const uint64_t kept_pe = first_block ? post_esc_keep(S.h_post_esc, kept_post) : 0;
  ix->last_inv_first = first_block;
  ix->last_inv_blocks = S.n_blocks;
  ix->last_inv_remap = inv.remap ? 1u : 0u;
  // ... and the shape they are inverted in: few blocks leave most of the device idle with one workgroup
  // per (block, range) tile and per row, so their documents are sliced and their rows split (slice_plan)
  SlicePlan sp;
  if (!S.term_major) {
    const uint32_t inv_blocks = S.n_blocks - first_block;
    const uint64_t max_docs = inv_blocks == 0 ? 0 : inv_blocks > 1 ? kBlockDocs : N - (uint64_t)first_block * kBlockDocs;
    sp = slice_plan(inv_blocks, S.R, max_docs, S.NC, (uint32_t)ix->num_cus, knob("TFIDF_TEST_INV_SLICES"),
                    knob("TFIDF_TEST_SCAN_PARTS"));
    if (sp.slices > 1 || sp.scan_parts > 1)
      HIP_TRY(ix->inv_aux.reserve_slack(((uint64_t)inv_blocks * S.R * 64 * (sp.slices > 1) +
                                         (uint64_t)inv_blocks * ((S.NC + kScanPartAlign - 1) / kScanPartAlign) *
                                             (sp.scan_parts > 1)) * 4));   // (part_tot: a word per k_df_sum workgroup and row)
  }
  ix->last_inv_slices = sp.slices;
  ix->last_inv_scan_parts = sp.scan_parts;
  // a lone sliced block: count, df, row scan and block base in one launch (fuse_plan).  Its scratch is
  // left zero by the kernel; it is zeroed here when new, or when the last fused commit did not reach
  // its synchronisation (the flag stays down from here until then)
  const bool fused = fuse_plan(S.term_major, S.term_major ? 0u : S.n_blocks - first_block, sp, knob("TFIDF_DF_FROM_ROWS"),
                               knob("TFIDF_TEST_SCAN_PARTS"), knob("TFIDF_INV_UNFUSED"));
  ix->last_inv_fused = fused ? 1u : 0u;
  if (fused) {
    const uint64_t need = fuse_scratch_words(S.R, S.NC);
    bool grow = false;
    const bool zero = fuse_scratch_must_zero(ix->fuse_state, need, &grow);
    uint64_t words = ix->fuse_state.words;
    if (grow) {
      ix->fuse_state = FuseScratch{};
      HIP_TRY(ix->inv_fuse.reserve((size_t)((need + need / 8 + 4096 + 15) / 16 * 16) * 4));   // (NC grows with the vocabulary)
      words = ix->inv_fuse.bytes / 4;
    }
    if (zero) HIP_TRY(hipMemsetAsync(ix->inv_fuse.p, 0, (size_t)words * 4, s));
    fuse_scratch_launch(&ix->fuse_state, words);
  }
  const uint32_t *blk_old = nullptr, *df_old = nullptr;
  if (!S.term_major) {
    const uint64_t blk_need = (uint64_t)(S.n_blocks + 1) * S.NC * 4 + 16;
    const uint64_t base_need = (uint64_t)S.NC * 4 + 16;
    if (inv.remap) {
      HIP_TRY(S.blk_alt.reserve(blk_need + blk_need / 8));   // (slack: a shard that keeps gaining terms remaps every commit)
      std::swap(S.blk.p, S.blk_alt.p);
      std::swap(S.blk.bytes, S.blk_alt.bytes);
      blk_old = S.blk_alt.as<uint32_t>();
      HIP_TRY(S.df_base_alt.reserve(base_need + base_need / 8));
      std::swap(S.df_base.p, S.df_base_alt.p);
      std::swap(S.df_base.bytes, S.df_base_alt.bytes);
      df_old = S.df_base_alt.as<uint32_t>();
    } else {
      if (int rc = grow_keep(ix, &S.blk, blk_need, (uint64_t)first_block * S.NC * 4)) return rc;
      // (a trusted base has this commit's NC columns already: without a remap NC is NC_inv)
      if (int rc = grow_keep(ix, &S.df_base, base_need + base_need / 8, dbp.trusted ? (uint64_t)S.NC * 4 : 0)) return rc;
    }
    if (int rc = grow_keep(ix, &S.bbase, (uint64_t)(S.n_blocks + 2) * 8, first_block ? (uint64_t)(first_block + 1) * 8 : 0))
      return rc;
  }
  // CSR tf escapes (rare: block-major only for tf >= 65 535, the all-ones
  // value of the 16-bit field, csr_esc_value(kRangeBits)): sorted by entry
  // index for the binary searches of the inversion and tfidf_doc_terms
  {
    // (incremental: the new escapes were appended behind the kept sorted
    // ones, which S.h_esc still holds; without new ones the list stands)
    const EscAppend ea = esc_append_bounds(kept_esc, (uint32_t)hctr[9], esc_cap);
    if (ea.overflow) return fail(TFIDF_E_CAPACITY, "CSR escape list overflow");
    const uint64_t n_esc = ea.first + ea.count;
    S.h_esc.resize(n_esc);
    if (ea.count) {
      HIP_TRY(hipMemcpyAsync(S.h_esc.data() + ea.first, S.csr_esc.as<uint64_t>() + ea.first, ea.count * 8,
                             hipMemcpyDeviceToHost, s));
      HIP_TRY(commit_sync(ix, s));
      esc_merge(&S.h_esc, ea.first);
      HIP_TRY(hipMemcpyAsync(S.csr_esc.p, S.h_esc.data(), n_esc * 8, hipMemcpyHostToDevice, s));
      HIP_TRY(commit_sync(ix, s));
    }
  }
  if (S.nnz >= 0xFFFFFFFFull) return fail(TFIDF_E_CAPACITY, "more than 2^32 postings per shard");
  // postings: block-major u32 (post_word), term-major u64; pass-1 temp words u32
  // (term-major: the sort's u64 value buffer)
  if (int rc = grow_keep(ix, &S.post, S.nnz * (S.term_major ? 8 : 4) + 8, kept_post * 4)) return rc;
  HIP_TRY(ix->post_tmp.reserve_slack(S.nnz * (S.term_major ? 8 : 4) + 8));
  const uint64_t post_esc_cap = row_cap / kPostTfEsc + 64;       // each needs tf >= 2047 tokens of one doc
  // (the kept blocks' escapes are the first kept_pe of the sorted list; new ones are appended behind them)
  if (!S.term_major)
    if (int rc = grow_keep(ix, &S.post_esc, post_esc_cap * 8, kept_pe * 8)) return rc;
  if (kept_pe) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(ctr + 10), (int)(uint32_t)kept_pe, 1, s));

  // the dictionary is final here (wave, Unicode and long paths done): its host
  // mirror, the deferred identity checks and the occupied-slot count run on the
  // side stream while the inversion runs (cfg-5 shape, 2^23 slots: 30.2 -> 28.4
  // ms per build; cfg 2: the 4 MB mirror, the checks and the count left ~0.2 ms
  // of copies, kernels and launch gaps after the inversion).  TFIDF_MIRROR_MAIN=1
  // keeps a mirror below 32 MB on the main stream after the inversion (A/B).
  HIP_TRY(S.h_dict.resize((size_t)2 * C));
  HIP_TRY(S.h_df.resize(C));
  // On a caller's stream (tfidf_set_stream: torch's stream under torch.distributed)
  // the small mirror stays on the main stream: the cross-stream hand-off cost the
  // one-rank RCCL rehearsal ~1 ms per step (tools/ab_dist3.sh: 12.4-12.8 vs 11.4-11.6)
  static const bool mirror_main = knob("TFIDF_MIRROR_MAIN") != nullptr;
  const bool mirror_side = (!mirror_main && s == ix->own_stream) || (size_t)2 * C * 8 >= (32u << 20);
  // (the side-stream work is enqueued after the inversion's launches, so the
  // host's enqueue time does not delay the first inversion kernel)
  // (delta mirrors without new documents: nothing to copy, no deferred check was queued: no side-stream work)
  const bool side_work = mirror_side && !(mp.delta && N == d_first);
  if (side_work) HIP_TRY(hipEventRecord(ix->mir_ev[0], s));

  PostingParams pp{};
  pp.offsets = bp.offsets;
  pp.live_map = bp.live_map;
  pp.n_docs = N;
  pp.C = C;
  pp.NC = S.NC;
  pp.crank = S.crank.as<uint2>();
  pp.range_shift = S.range_shift;
  pp.n_ranges = S.R;
  pp.n_blocks = S.n_blocks;
  pp.csr = bp.csr;
  pp.csr_esc = bp.csr_esc;
  pp.n_esc = S.h_esc.size();
  pp.rsplit = bp.rsplit;
  pp.doc_norm = bp.doc_norm;
  pp.blk = S.blk.as<uint32_t>();
  pp.bbase = S.bbase.as<uint64_t>();
  pp.post = S.post.as<uint32_t>();
  pp.post_tmp = ix->post_tmp.as<uint32_t>();
  pp.post_esc = S.post_esc.as<uint64_t>();
  pp.post_esc_count = reinterpret_cast<uint32_t *>(ctr + 10);
  pp.post_esc_cap = post_esc_cap;
  pp.sort_spw = sp.sort_spw;                              // (4 unless few blocks are inverted)
  if (const char *e = knob("TFIDF_SORT_SPW")) pp.sort_spw = (uint32_t)std::max(1, std::min(8, atoi(e)));   // A/B only (<= kSortMaxSpw)
  pp.err = bp.err;
  pp.first_block = first_block;
  pp.slices = sp.slices;
  pp.slice_docs = sp.slice_docs;
  pp.scan_parts = sp.scan_parts;
  pp.scan_width = sp.scan_width;
  pp.slice_cur = ix->inv_aux.as<uint32_t>();
  pp.part_tot = pp.slice_cur + (sp.slices > 1 ? (size_t)(S.n_blocks - first_block) * S.R * 64 : 0);
  pp.df_base = S.df_base.as<uint32_t>();
  pp.df_fold_end = dbp.fold_end;
  pp.df_from_rows = dbp.from_rows ? 1u : 0u;
  pp.fuse = fused ? ix->inv_fuse.as<uint32_t>() : nullptr;
  pp.fuse_tickets = fused ? fuse_tickets(sp, N - (uint64_t)first_block * kBlockDocs) : 0u;
  HIP_TRY(hipEventRecord(ix->ev[EV_D0], s));
  if (S.term_major) {
    TermParams tp{};
    if (N > kTermMaxDocs)
      return fail(TFIDF_E_CAPACITY, "the term-major layout holds at most 2^26 documents per shard");
    tp.offsets = bp.offsets;
    tp.live_map = bp.live_map;
    tp.n_docs = N;
    tp.nnz = S.nnz;
    tp.C = C;
    tp.slot_bits = ix->cap_log2;
    tp.doc_bits = 1;
    while ((1ull << tp.doc_bits) < N) tp.doc_bits++;
    // >= 4 (slot, doc <= 26 bits); at most 24 (tf <= kMaxTf): a small shard
    // (40 books: 56 - 18 - 6 = 32) must not reach a 32-bit shift in tf_esc
    tp.tf_bits = std::min(56u - tp.slot_bits - tp.doc_bits, 24u);
    if (const char *e = knob("TFIDF_TEST_TERM_TF_BITS"))      // tests: exercise the tf escape list
      tp.tf_bits = std::max(1u, std::min(tp.tf_bits, (uint32_t)atoi(e)));
    tp.csr = bp.csr;
    tp.csr_esc = bp.csr_esc;
    tp.n_esc = S.h_esc.size();
    tp.doc_nuniq = bp.doc_nuniq;
    tp.doc_norm = bp.doc_norm;
    tp.row_off = S.row_off.as<uint32_t>();
    HIP_TRY(ix->tvals.reserve_slack(S.nnz * 8 + 16));
    tp.keys = ix->post_tmp.as<uint64_t>();
    tp.keys_alt = ix->tvals.as<uint64_t>();
    tp.post = S.post.as<uint64_t>();
    tp.toff = S.toff.as<uint64_t>();
    tp.df = S.tdf.as<uint32_t>();
    tp.err = bp.err;
    tp.tesc_cap = row_cap / ((1u << tp.tf_bits) - 1) + 64;   // each needs tf >= the escape value
    HIP_TRY(ix->term_esc.reserve(tp.tesc_cap * 16));
    tp.tesc = ix->term_esc.as<uint64_t>();
    tp.tesc_count = reinterpret_cast<uint32_t *>(ctr + 12);
    HIP_TRY(ix->term_tmp.reserve(term_invert_scratch_words(N, S.nnz, C) * 4));
    tp.scratch = ix->term_tmp.as<uint32_t>();
    // the whole inversion is reported under ms_scatter
    HIP_TRY(hipEventRecord(ix->ev[EV_DF], s));
    HIP_TRY(hipEventRecord(ix->ev[EV_BSCAN], s));
    HIP_TRY(hipEventRecord(ix->ev[EV_CSCAN], s));
    HIP_TRY(launch_term_pairs(tp, s));
    {   // tf >= 4095 (rare): the escape list sorted for the postings pass's binary search
      uint32_t ne = 0;
      HIP_TRY(hipMemcpyAsync(&ne, tp.tesc_count, 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(commit_sync(ix, s));
      if (ne > tp.tesc_cap) return fail(TFIDF_E_CAPACITY, "term-major escape list overflow");
      if (ne) {
        std::vector<std::pair<uint64_t, uint64_t>> h(ne);
        ix->prof.stream_syncs++;
        HIP_TRY(hipMemcpy(h.data(), tp.tesc, ne * 16, hipMemcpyDeviceToHost));
        std::sort(h.begin(), h.end());
        HIP_TRY(hipMemcpy(tp.tesc, h.data(), ne * 16, hipMemcpyHostToDevice));
      }
      tp.n_tesc = ne;
    }
    HIP_TRY(launch_term_sort(tp, s));
    HIP_TRY(hipEventRecord(ix->ev[EV_SCAT], s));
  } else {
    if (inv.remap) HIP_TRY(launch_blk_remap(pp, blk_old, df_old, S.crank_inv.as<uint2>(), S.NC_inv, s));
    if (fused) {
      HIP_TRY(launch_df_fused(pp, s));                    // the lone block: counts, df, offsets and its base
    } else if (S.n_blocks) {
      HIP_TRY(launch_inv_zero(pp, s));                    // (sliced / split shapes only)
      HIP_TRY(launch_df_partial(pp, s));                  // blocks [first_block, n_blocks)
    } else {
      HIP_TRY(hipMemsetAsync(S.blk.p, 0, (size_t)S.NC * 4, s));
    }
    HIP_TRY(hipEventRecord(ix->ev[EV_DF], s));
    if (!fused) HIP_TRY(launch_df_sum(pp, s));
    if (dict_delta || df_delta) {
      // sdf still holds the df of this snapshot's last build, crank_inv its occupancy: the slots that
      // differ are listed while sdf is rewritten (counts: ctr[14] df, ctr[15] dictionary)
      MirrorDeltaParams dp{};
      dp.crank = S.crank.as<uint2>();
      dp.crank_inv = S.crank_inv.as<uint2>();
      dp.df_col = S.blk.as<uint32_t>() + (size_t)S.n_blocks * S.NC;
      dp.C = C;
      dp.df_slot = S.sdf.as<uint32_t>();
      dp.dict = S.dict.as<uint64_t>();
      dp.dict_list = dict_delta ? ix->mir_dict_list.as<DictDelta>() : nullptr;
      dp.dict_cap = mp.n_new;
      dp.dict_count = reinterpret_cast<uint32_t *>(ctr + 15);
      dp.df_list = df_delta ? ix->mir_df_list.as<DfDelta>() : nullptr;
      dp.df_cap = df_cap;
      dp.df_count = reinterpret_cast<uint32_t *>(ctr + 14);
      HIP_TRY(launch_df_slots_delta(dp, s));
    } else if (!keep_sdf) {
      HIP_TRY(launch_df_slots(S.crank.as<uint2>(), S.blk.as<uint32_t>() + (size_t)S.n_blocks * S.NC, C,
                              S.sdf.as<uint32_t>(), s));
    }
    if (side_work) HIP_TRY(hipEventRecord(ix->mir_ev[2], s));   // df final: its host mirror copies beside the scatter
    if (S.n_blocks && !fused) HIP_TRY(launch_row_scan(pp, s));
    HIP_TRY(hipEventRecord(ix->ev[EV_BSCAN], s));
    if (!fused) HIP_TRY(launch_block_base(pp, s));
    HIP_TRY(hipEventRecord(ix->ev[EV_CSCAN], s));
    if (S.n_blocks) HIP_TRY(launch_scatter(pp, s));
    HIP_TRY(hipEventRecord(ix->ev[EV_SCAT], s));
  }
  if (side_work) {
    HIP_TRY(hipStreamWaitEvent(ix->copy_stream, ix->mir_ev[0], 0));
    if (dict_whole)
      HIP_TRY(hipMemcpyAsync(S.h_dict.data(), S.dict.p, (size_t)2 * C * 8, hipMemcpyDeviceToHost, ix->copy_stream));
    HIP_TRY(launch_verify_deferred(bp, ix->copy_stream));
    if (S.term_major)       // (block-major: col_rank counted the columns)
      HIP_TRY(launch_count_nonzero(S.dict.as<uint64_t>(), C, reinterpret_cast<unsigned long long *>(ctr + 7),
                                   ix->copy_stream));
    if (!S.term_major) {
      // block-major: df and the slot -> column map are final before the
      // scatter, so their host mirrors copy while it runs (on the main stream
      // after it they cost ~0.1 ms of the cfg-2 step)
      HIP_TRY(hipStreamWaitEvent(ix->copy_stream, ix->mir_ev[2], 0));
      if (df_whole)
        HIP_TRY(hipMemcpyAsync(S.h_df.data(), S.df_dev(), (size_t)C * 4, hipMemcpyDeviceToHost, ix->copy_stream));
      HIP_TRY(S.h_crank.resize((size_t)C / 32 + 1));
      if (crank_whole)
        HIP_TRY(hipMemcpyAsync(S.h_crank.data(), S.crank.p, ((size_t)C / 32 + 1) * 8, hipMemcpyDeviceToHost,
                               ix->copy_stream));
      // the new slots' keys: the list's length is known (n_new), so it is copied here and checked below
      if (dict_delta)
        HIP_TRY(hipMemcpyAsync(ix->h_dict_delta.data(), ix->mir_dict_list.p, (size_t)mp.n_new * sizeof(DictDelta),
                               hipMemcpyDeviceToHost, ix->copy_stream));
    }
    HIP_TRY(hipEventRecord(ix->mir_ev[1], ix->copy_stream));
  }
  {
    tfidf_host_profile &pf = ix->prof;
    pf.mirror_dict = mp.dict;
    pf.mirror_df = mp.df;
    pf.mirror_crank = S.term_major ? (uint32_t)TFIDF_MIRROR_NONE : (uint32_t)mp.crank;
    if (dict_whole) pf.bytes_dict += (uint64_t)2 * C * 8;
    if (dict_delta) pf.bytes_dict += (uint64_t)mp.n_new * sizeof(DictDelta);
    if (df_whole) pf.bytes_df += (uint64_t)C * 4;
    if (crank_whole && !S.term_major) pf.bytes_crank += ((uint64_t)C / 32 + 1) * 8;
    pf.dict_delta_entries = dict_delta ? mp.n_new : 0;
    pf.df_delta_entries = 0;
  }
  // host mirrors for query analysis: dictionary keys + df
  if (!mirror_side && dict_whole)
    HIP_TRY(hipMemcpyAsync(S.h_dict.data(), S.dict.p, (size_t)2 * C * 8, hipMemcpyDeviceToHost, s));
  if ((!mirror_side || S.term_major) && df_whole)
    HIP_TRY(hipMemcpyAsync(S.h_df.data(), S.df_dev(), (size_t)C * 4, hipMemcpyDeviceToHost, s));
  if (!S.term_major && !mirror_side) {                 // slot -> column for query preparation
    HIP_TRY(S.h_crank.resize((size_t)C / 32 + 1));
    if (crank_whole)
      HIP_TRY(hipMemcpyAsync(S.h_crank.data(), S.crank.p, ((size_t)C / 32 + 1) * 8, hipMemcpyDeviceToHost, s));
    if (dict_delta)
      HIP_TRY(hipMemcpyAsync(ix->h_dict_delta.data(), ix->mir_dict_list.p, (size_t)mp.n_new * sizeof(DictDelta),
                             hipMemcpyDeviceToHost, s));
  }
  if (side_work) {
    HIP_TRY(hipStreamWaitEvent(s, ix->mir_ev[1], 0));   // mirror, checks and count (side stream)
  } else if (!mirror_side) {
    // hashed-key identity checks the tokenizers had to defer
    HIP_TRY(launch_verify_deferred(bp, s));
    // occupied dictionary slots counted on the device (ctr[7]) instead of a host
    // pass over the mirror (8 M slots at 2^23 took milliseconds)
    if (S.term_major)
      HIP_TRY(launch_count_nonzero(S.dict.as<uint64_t>(), C, reinterpret_cast<unsigned long long *>(ctr + 7), s));
  }
  // ctr[3] error flags .. ctr[7] occupied slots, [8] malformed, [10] posting escapes, [14] / [15] delta list counts
  // (into pinned memory: a pageable destination makes the copy call itself wait for the stream)
  uint64_t *tail = hctr + 14;
  HIP_TRY(hipMemcpyAsync(tail, ctr + 3, 13 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  if (!S.term_major) {           // the block bases: the next commit's kept postings and escapes are found by them
    HIP_TRY(S.h_bbase.resize((size_t)S.n_blocks + 2));
    HIP_TRY(hipMemcpyAsync(S.h_bbase.data(), S.bbase.p, ((size_t)S.n_blocks + 1) * 8, hipMemcpyDeviceToHost, s));
  }
  ix->prof.ms_enqueued = prof_ms(ix);
  HIP_TRY(commit_sync(ix, s));
  ix->prof.ms_synced = prof_ms(ix);
  if (fused) fuse_scratch_done(&ix->fuse_state);      // k_df_fused ran to its end: its finishers left the scratch zero
  {
    // rare (tf >= 2047): sorted for the scorer's binary search.  The kept
    // blocks' entries stand; the new ones were appended behind them.
    const EscAppend pe = esc_append_bounds(kept_pe, S.term_major ? 0 : (uint32_t)tail[7], post_esc_cap);
    if (pe.overflow) return fail(TFIDF_E_CAPACITY, "posting escape list overflow");
    const uint64_t n_pe = pe.first + pe.count;
    S.h_post_esc.resize(n_pe);
    if (pe.count) {
      ix->prof.stream_syncs++;
      HIP_TRY(hipMemcpy(S.h_post_esc.data() + pe.first, S.post_esc.as<uint64_t>() + pe.first, pe.count * 8,
                        hipMemcpyDeviceToHost));
      esc_merge(&S.h_post_esc, pe.first);
      HIP_TRY(hipMemcpy(S.post_esc.p, S.h_post_esc.data(), n_pe * 8, hipMemcpyHostToDevice));
    }
  }
  if (const uint32_t n_bad = (uint32_t)tail[5]) {   // (incremental: S.malformed holds the kept documents' ids)
    std::vector<uint32_t> bad(n_bad);
    ix->prof.stream_syncs++;
    HIP_TRY(hipMemcpy(bad.data(), ix->bad_list.p, (size_t)n_bad * 4, hipMemcpyDeviceToHost));
    merge_malformed(&S.malformed, bad.data(), n_bad);
  }
  const uint32_t err2 = (uint32_t)tail[0];
  if (err2 & kErrCollision) { ix->collision_doc = (uint32_t)(tail[0] >> 32); return kRcCollision; }
  if (err2 & kErrTfTooLarge) return fail(TFIDF_E_UNSUPPORTED_INPUT, "a term frequency exceeds 2^24 - 1");
  // The mirrors' deltas, now that the build is known good (a failed one leaves
  // mir_ok false, and the next build copies whole).  The dictionary list's
  // length was known in advance; the device must have found exactly as many.
  if (dict_delta) {
    if ((uint32_t)tail[12] != mp.n_new)
      return fail(TFIDF_E_STATE, "dictionary mirror delta: %u new slots listed, %u expected", (uint32_t)tail[12],
                  mp.n_new);
    if (!apply_dict_delta(S.h_dict.data(), C, ix->h_dict_delta.data(), mp.n_new))
      return fail(TFIDF_E_STATE, "dictionary mirror delta names a slot past the dictionary");
  }
  if (df_delta) {
    const uint32_t n_df = (uint32_t)tail[11];
    if (n_df > df_cap) {               // the list overflowed (entries past the cap were counted, not stored)
      ix->prof.stream_syncs++;
      HIP_TRY(hipMemcpy(S.h_df.data(), S.df_dev(), (size_t)C * 4, hipMemcpyDeviceToHost));
      ix->prof.mirror_df = TFIDF_MIRROR_WHOLE;
      ix->prof.bytes_df += (uint64_t)C * 4;
    } else {
      if (n_df) {
        HIP_TRY(hipMemcpyAsync(ix->h_df_delta.data(), ix->mir_df_list.p, (size_t)n_df * sizeof(DfDelta),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(commit_sync(ix, s));
        if (!apply_df_delta(S.h_df.data(), C, ix->h_df_delta.data(), n_df))
          return fail(TFIDF_E_STATE, "df mirror delta names a slot past the dictionary");
      }
      ix->prof.bytes_df += (uint64_t)n_df * sizeof(DfDelta);
      ix->prof.df_delta_entries = n_df;
    }
  }
  S.num_terms = keep_rank ? S.NC : tail[4];     // (col_rank counts the occupied slots into ctr[7]; it did not run)

  tfidf_commit_timing &t = ix->timing;
  t.ms_tokenize = ev_ms(ix, EV_START, EV_TOK);
  t.ms_long = n_long ? ev_ms(ix, EV_L0, EV_LONG) : 0.0f;
  t.ms_df = ev_ms(ix, EV_D0, EV_DF);
  t.ms_blockscan = ev_ms(ix, EV_DF, EV_BSCAN);
  t.ms_colscan = ev_ms(ix, EV_BSCAN, EV_CSCAN);
  t.ms_scatter = ev_ms(ix, EV_CSCAN, EV_SCAT);
  t.ms_total = t.ms_tokenize + t.ms_long + ev_ms(ix, EV_D0, EV_SCAT);   // device time, host syncs excluded
  t.text_bytes = ix->text_bytes;
  t.num_docs = N;
  t.nnz = S.nnz;

  // what the snapshot was built from
  S.cap_log2 = ix->cap_log2;
  S.text_bytes = ix->text_bytes;
  S.text = ix->text;
  S.offsets = ix->offsets;
  ix->keys.compact();
  S.keys = ix->keys;                 // shares the chunks; the builder appends to a new one
  S.hash_seed = ix->hash_seed;
  S.sig = sig;
  {
    std::lock_guard<std::mutex> tl(S.term_mu);
    S.term_cache.clear();
  }
  {
    std::lock_guard<std::mutex> ml(S.mlt_mu);
    S.mlt_ready = false;
  }
  S.mir_ok = true;                     // the mirrors match dict, sdf / tdf and crank
  S.tok_docs = ix->n_staged;           // the rows and the dictionary cover every staged document
  if (!S.term_major) {                 // ... and so do blk (laid out by crank, NC columns), bbase and post
    S.inv_docs = ix->n_staged;
    S.NC_inv = S.NC;
  }
  return TFIDF_OK;
}

extern "C" int tfidf_commit(tfidf_index *ix) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->cfg.device);
  ix->prof = tfidf_host_profile{};
  ix->prof_t0 = std::chrono::steady_clock::now();
  struct Wall {                                // (every return below)
    tfidf_index *ix;
    ~Wall() { ix->prof.ms_wall = prof_ms(ix); }
  } wall{ix};
  // tfidf_set_compact_threshold: reclaim the dead documents first.  A
  // compaction that cannot get its memory leaves the index as it was, and the
  // commit builds through live_map as it always has.
  if (ix->compact_pct && ix->n_dead && ix->dead_bytes * 100 >= (uint64_t)ix->compact_pct * ix->text_bytes)
    compact_locked(ix, nullptr, nullptr);
  // The build target: the previous snapshot if no search holds it any more
  // (its buffers are reused as they are), else a new one.  The published
  // snapshot stays searchable until this build succeeds; a failed build
  // publishes nothing (the reference's readers keep the last commit).
  std::shared_ptr<Snapshot> S;
  if (ix->spare && ix->spare.use_count() == 1) S = std::move(ix->spare);
  ix->spare.reset();
  if (!S) S = std::make_shared<Snapshot>(ix->cfg.device);
  // Hash seeds: 0, then 1, 2, 3 after a detected collision (TFIDF_TEST_WEAK_HASH:
  // start from a seed under which equal-length hashed keys collide).  A floor
  // set by tfidf_set_hash_attempt (GLOBAL statistics: every shard must hash
  // with one seed) skips the earlier attempts.
  const char *weak = knob("TFIDF_TEST_WEAK_HASH");
  ix->hash_seed = ix->hash_floor ? ix->hash_floor : ((weak && atoi(weak)) ? kWeakHashSeed : 0);
  ix->hash_rebuilds = ix->hash_floor;
  for (uint32_t attempt = ix->hash_floor;; attempt++) {
    int rc = commit_once(ix, *S, attempt == ix->hash_floor);
    if (rc != TFIDF_OK) {
      hipStreamSynchronize(ix->stream);        // nothing of this build may still run on either stream
      hipStreamSynchronize(ix->copy_stream);
    }
    if (rc == kRcCollision) {
      if (attempt == 3) {
        ix->spare = std::move(S);
        return fail(TFIDF_E_UNSUPPORTED_INPUT, "hash collisions under 4 seeds (last in document %u)", ix->collision_doc);
      }
      ix->hash_seed = attempt + 1;
      ix->hash_rebuilds++;
      continue;
    }
    if (rc != TFIDF_OK) {
      ix->spare = std::move(S);
      return rc == kRcNoPublish ? TFIDF_OK : rc;
    }
    S->hash_rebuilds = ix->hash_rebuilds;
    S->generation = ++ix->generation;
    {
      std::lock_guard<std::mutex> sl(ix->snap_mu);
      std::swap(ix->cur, S);                   // published; S = the previous snapshot
    }
    ix->prof.ms_published = prof_ms(ix);
    ix->spare = std::move(S);                  // rebuilt in place next time if no search holds it
    return TFIDF_OK;
  }
}

extern "C" int tfidf_set_hash_attempt(tfidf_index *ix, uint32_t attempt) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  if (attempt > 3) return fail(TFIDF_E_INVALID_ARG, "hash seed attempt %u > 3", attempt);
  std::lock_guard<std::mutex> lk(ix->mu);
  ix->hash_floor = attempt;
  return TFIDF_OK;
}

extern "C" int tfidf_commit_tokenized_docs(const tfidf_index *ix, uint64_t *docs, uint32_t *was_full) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->mu);
  if (docs) *docs = ix->last_tok_docs;
  if (was_full) *was_full = ix->last_tok_full;
  return TFIDF_OK;
}

extern "C" int tfidf_commit_host_profile(const tfidf_index *ix, tfidf_host_profile *out) {
  if (!ix || !out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->mu);
  *out = ix->prof;
  return TFIDF_OK;
}

extern "C" int tfidf_commit_inverted_blocks(const tfidf_index *ix, uint32_t *first_block, uint32_t *n_blocks,
                                            uint32_t *remapped) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->mu);
  if (first_block) *first_block = ix->last_inv_first;
  if (n_blocks) *n_blocks = ix->last_inv_blocks;
  if (remapped) *remapped = ix->last_inv_remap;
  return TFIDF_OK;
}

extern "C" int tfidf_commit_inversion_shape(const tfidf_index *ix, uint32_t *slices, uint32_t *scan_parts) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->mu);
  if (slices) *slices = ix->last_inv_slices;
  if (scan_parts) *scan_parts = ix->last_inv_scan_parts;
  return TFIDF_OK;
}

extern "C" int tfidf_commit_inversion_fused(const tfidf_index *ix, uint32_t *fused) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->mu);
  if (fused) *fused = ix->last_inv_fused;
  return TFIDF_OK;
}

extern "C" int tfidf_get_commit_timing(const tfidf_index *ix, tfidf_commit_timing *out) {
  if (!ix || !out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  *out = ix->timing;
  return TFIDF_OK;
}

extern "C" int tfidf_stats(const tfidf_index *ix, tfidf_index_stats *out) {
  if (!ix || !out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const std::shared_ptr<Snapshot> S = current(ix);
  *out = tfidf_index_stats{};
  uint64_t staged_bytes = 0;
  {
    // builder-side fields: add_docs / clear / commit replace them under mu
    std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->mu);
    out->text_bytes = ix->text_bytes;
    out->hash_seed = ix->hash_seed;
    out->hash_rebuilds = ix->hash_rebuilds;
    staged_bytes = ix->text->bytes + ix->offsets->bytes;
    out->dead_docs = ix->n_dead;
    out->dead_bytes = ix->dead_bytes;
    out->compactions = ix->compactions;
  }
  if (S) {
    out->num_docs = S->n_docs;
    out->doc_count = S->doc_count;
    out->sum_ttf = S->sum_ttf;
    out->num_terms = S->num_terms;
    out->nnz = S->nnz;
    out->long_docs = S->long_docs;
    out->term_major = S->term_major;
    out->pack_docs = S->pack_docs;
    out->pack_retried = S->pack_retried;
    out->unicode_docs = S->unicode_docs;
    out->unicode_wave_docs = S->unicode_wave_docs;
    out->long_chunked = S->long_chunked;
    out->malformed_docs = S->malformed.size();
    out->hash_seed = S->hash_seed;
    out->hash_rebuilds = S->hash_rebuilds;
  }
  {
    std::lock_guard<std::mutex> cl(ix->cq_mu);
    out->coalesced_batches = ix->cq_batches;
    out->coalesced_queries = ix->cq_queries;
  }
  out->unit_batches = ix->unit_batches.load();
  out->fused_queries = ix->fused_queries.load();
  out->unit_count = ix->unit_count.load();
  uint64_t tot = staged_bytes;
  if (S) {
    const DevBuf *bufs[] = {&S->dict, &S->csr, &S->csr_esc, &S->doc_len, &S->doc_nuniq, &S->doc_norm,
                            &S->rsplit, &S->blk, &S->bbase, &S->post, &S->toff, &S->tdf, &S->crank, &S->sdf,
                            &S->crank_inv, &S->blk_alt, &S->df_base, &S->df_base_alt};
    for (const DevBuf *b : bufs) tot += b->bytes;
  }
  out->device_bytes = tot;
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// dictionary (host mirror)

static uint32_t host_lookup(const Snapshot &S, uint64_t lo, uint64_t hi) {
  if (S.C == 0) return kInvalidSlot;
  const uint32_t mask = S.C - 1;
  // same probe order as the device (kernels_index.hip dict_lookup_multi):
  // linear from the aligned 2-slot bucket of the hash; lo[C] then hi[C]
  uint32_t s = dict_home(dict_hash(lo, hi), mask) & ~1u;
  for (uint32_t it = 0; it <= mask; it++) {
    const uint64_t clo = S.h_dict[s], chi = S.h_dict[(size_t)S.C + s];
    if (clo == 0) return kInvalidSlot;
    if (clo == lo && chi == hi) return s;
    s = (s + 1) & mask;
  }
  return kInvalidSlot;
}

// Lower-cased term string of dictionary slot `slot`: decoded from an exact
// key, or (hashed key) read from its reference occurrence in the corpus.
struct StrSink {
  std::string s;
  void push(uint8_t c) { s.push_back((char)c); }
};
static int slot_term(Snapshot &S, uint32_t slot, std::string *out) {
  char b[32];
  const uint64_t lo = S.h_dict[slot], hi = S.h_dict[(size_t)S.C + slot];
  if (const uint32_t n = key_decode(lo, hi, b)) { out->assign(b, n); return TFIDF_OK; }
  std::lock_guard<std::mutex> tl(S.term_mu);             // batch preparation threads share the cache
  auto it = S.term_cache.find(slot);
  if (it != S.term_cache.end()) { *out = it->second; return TFIDF_OK; }
  uint64_t r = 0;
  HIP_TRY(hipMemcpy(&r, S.dict.as<uint64_t>() + 2 * (size_t)S.C + slot, 8, hipMemcpyDeviceToHost));
  if (r == 0) return fail(TFIDF_E_STATE, "dictionary slot %u has no reference occurrence", slot);
  std::vector<uint8_t> raw(dict_ref_len(r));
  if (!raw.empty())
    HIP_TRY(hipMemcpy(raw.data(), S.text->as<uint8_t>() + dict_ref_off(r), raw.size(), hipMemcpyDeviceToHost));
  StrSink sink;
  uc_token_bytes(raw.data(), raw.size(), 0, raw.size(), sink);
  S.term_cache.emplace(slot, sink.s);
  *out = sink.s;
  return TFIDF_OK;
}

// Dictionary slot of the (lower-cased) term t, kInvalidSlot if absent; a
// hashed key must also match the slot's term string.
static uint32_t lookup_term(Snapshot &S, const std::string &t) {
  uint64_t lo, hi;
  term_key(t, &lo, &hi, S.hash_seed);
  const uint32_t s = host_lookup(S, lo, hi);
  if (s == kInvalidSlot || !key_is_hashed(lo)) return s;
  std::string ts;
  if (slot_term(S, s, &ts) != TFIDF_OK || ts != t) return kInvalidSlot;
  return s;
}

struct PreparedQuery {
  std::vector<uint32_t> slot;    // per term: what the scorers index it by (Snapshot::col_of)
  std::vector<uint32_t> ldf;     // per term: the shard's own df
  std::vector<float> w;
  std::vector<uint32_t> role;    // role << 24 | MUST clause index
  uint32_t meta = 0;             // MUST clause count | has MUST_NOT << 31
};

// upper bound of a query's hits on this shard: the sum of its scoring terms' local df
static uint64_t hits_bound(const Snapshot &S, const PreparedQuery &pq) {
  uint64_t b = 0;
  for (size_t i = 0; i < pq.slot.size(); i++)
    if ((pq.role[i] >> 24) != kRoleNot) b += pq.ldf[i];
  return b;
}

// Query plan (analysis.h) -> dictionary slots + BM25 weights.  A term absent
// from this shard's dictionary has no scorer (TermWeight.scorer == null): a
// SHOULD or MUST_NOT term is dropped, a MUST clause without any present term
// leaves the query without hits (BooleanWeight: required scorer missing), and
// a query with neither MUST clauses nor a present SHOULD term has no hits.
static int prepare_query(Snapshot &S, StatsView &V, const uint8_t *q, uint64_t n, PreparedQuery *pq) {
  QueryPlan plan;
  const int rc = parse_query(q, n, &plan);
  if (rc == kQBadUtf8) return fail(TFIDF_E_UNSUPPORTED_QUERY, "query is not valid UTF-8");
  if (rc == kQSyntax)
    return fail(TFIDF_E_QUERY_SYNTAX, "query does not parse (QueryParser ParseException / TooManyClauses)");
  if (int e = V.wait_gdf()) return e;
  const uint64_t dc = V.doc_count;
  if (dc == 0) return TFIDF_OK;                        // no document holds a token
  std::vector<uint32_t> present(plan.n_groups, 0);
  uint32_t n_should = 0;
  bool has_not = false;
  for (const PlanTerm &t : plan.terms) {
    const uint32_t s = lookup_term(S, t.term);
    if (s == kInvalidSlot) continue;                   // absent term contributes nothing
    float wv = 0.0f;
    if (t.role != kRoleNot) {
      const uint64_t df = V.global ? V.gdf[s] : S.h_df[s];
      const float idf = bm25_idf(df, dc);
      volatile float w = t.boost * idf;                // BM25Scorer: weight = boost * idf
      wv = w;
    }
    if (t.role == kRoleMust) present[t.group]++;
    if (t.role == kRoleShould) n_should++;
    if (t.role == kRoleNot) has_not = true;
    pq->slot.push_back(S.col_of(s));
    pq->ldf.push_back(S.h_df[s]);
    pq->w.push_back(wv);
    pq->role.push_back(t.role << 24 | t.group);
  }
  bool empty = plan.n_groups == 0 && n_should == 0;
  for (uint32_t c : present) empty |= c == 0;
  if (empty) {
    pq->slot.clear();
    pq->ldf.clear();
    pq->w.clear();
    pq->role.clear();
    return TFIDF_OK;
  }
  pq->meta = plan.n_groups | (has_not ? 1u << 31 : 0u);
  return TFIDF_OK;
}

// Batch of prepared queries in device layout.
struct QueryBatch {
  std::vector<uint32_t> off{0}, slot, role, meta, ldf;
  std::vector<float> w;
  bool ops = false;                // some query has MUST / MUST_NOT clauses
  void add(const PreparedQuery &pq) {
    slot.insert(slot.end(), pq.slot.begin(), pq.slot.end());
    ldf.insert(ldf.end(), pq.ldf.begin(), pq.ldf.end());
    w.insert(w.end(), pq.w.begin(), pq.w.end());
    role.insert(role.end(), pq.role.begin(), pq.role.end());
    off.push_back((uint32_t)slot.size());
    meta.push_back(pq.slot.empty() ? 0u : pq.meta);
    ops |= !pq.slot.empty() && pq.meta != 0;
  }
};

// Prepare a batch's queries (parse, analysis, dictionary lookups, BM25
// weights) on host threads: large batches spend more time here than on the
// device (10 k queries: ~10 ms on one thread).  A query that does not parse
// (or is not UTF-8) has no hits, as the reference answers [] for it
// (Worker.java:182-185); the batch goes on.
// Persistent host workers for batch query preparation (spawning 16 threads per
// batch cost ~0.5 ms of a 10 k-query batch).  run(n, fn): fn(a, b) over `parts`
// slices of [0, n), the caller taking slice 0; one batch at a time.
struct PrepPool {
  std::vector<std::thread> th;
  std::mutex run_mu, mu;
  std::condition_variable cv, done_cv;
  std::function<void(uint32_t, uint32_t)> fn;
  uint32_t n = 0, parts = 0, next = 0, finished = 0;
  uint64_t gen = 0;
  explicit PrepPool(uint32_t workers) {
    for (uint32_t i = 0; i < workers; i++) th.emplace_back([this] { loop(); });
  }
  void slice(uint32_t i) { fn((uint32_t)((uint64_t)n * i / parts), (uint32_t)((uint64_t)n * (i + 1) / parts)); }
  void loop() {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return gen != seen; });
      seen = gen;
      while (next < parts) {
        const uint32_t i = next++;
        lk.unlock();
        slice(i);
        lk.lock();
        if (++finished == parts) done_cv.notify_all();
      }
    }
  }
  void run(uint32_t n_items, uint32_t n_parts, std::function<void(uint32_t, uint32_t)> f) {
    std::lock_guard<std::mutex> rl(run_mu);
    std::unique_lock<std::mutex> lk(mu);
    fn = std::move(f);
    n = n_items;
    parts = n_parts;
    next = 1;                                           // slice 0: the caller
    finished = 0;
    gen++;
    cv.notify_all();
    lk.unlock();
    slice(0);
    lk.lock();
    if (++finished < parts) done_cv.wait(lk, [&] { return finished == parts; });
  }
};
static PrepPool *prep_pool() {
  // never destroyed: its threads block forever on an idle pool
  static PrepPool *pool = new PrepPool(std::min<uint32_t>(std::max(1u, std::thread::hardware_concurrency()), 16u) - 1);
  return pool;
}

static int prepare_batch(tfidf_index *ix, Snapshot &S, StatsView &V, const uint8_t *q_utf8,
                         const uint64_t *q_offsets, uint32_t n_q, QueryBatch *qb) {
  if (int e = V.wait_gdf()) return e;                  // once, before the workers read the mirrors
  std::vector<PreparedQuery> pqs(n_q);
  auto work = [&](uint32_t a, uint32_t b) {
    DeviceGuard g(ix->cfg.device);                      // slot_term may read a reference occurrence
    for (uint32_t i = a; i < b; i++)
      if (prepare_query(S, V, q_utf8 + q_offsets[i], q_offsets[i + 1] - q_offsets[i], &pqs[i]) != TFIDF_OK)
        pqs[i] = PreparedQuery();
  };
  uint32_t nt = std::min<uint32_t>(std::max(1u, std::thread::hardware_concurrency()), 16u);
  nt = std::max(1u, std::min(nt, n_q / 128));
  if (nt <= 1) work(0, n_q);
  else prep_pool()->run(n_q, nt, work);
  size_t ns = 0;
  for (const PreparedQuery &pq : pqs) ns += pq.slot.size();
  qb->slot.reserve(ns);
  qb->ldf.reserve(ns);
  qb->w.reserve(ns);
  qb->role.reserve(ns);
  qb->off.reserve(n_q + 1);
  qb->meta.reserve(n_q);
  for (const PreparedQuery &pq : pqs) qb->add(pq);
  return TFIDF_OK;
}

// Test hook (TFIDF_TEST_FAIL_SCORING = n): every n-th scoring call fails after
// its kernels are queued, as a HIP error in a later launch would
// (tests/test_gpu_snapshot.py: the failed search must drain before its
// snapshot can be rebuilt by a commit).
static int scoring_done() {
  const char *e = knob("TFIDF_TEST_FAIL_SCORING");
  if (!e) return TFIDF_OK;
  static std::atomic<uint64_t> calls{0};
  const uint64_t n = (uint64_t)std::max(1, atoi(e));
  if (++calls % n) return TFIDF_OK;
  return fail(TFIDF_E_HIP, "injected scoring failure (TFIDF_TEST_FAIL_SCORING)");
}

// all_R2 (k == 0, a batch): runs per query of the batched all-hits layout
// (launch_hits_order_batch); 0: one query's runs, one per block.
static int run_scoring(tfidf_index *ix, Snapshot &S, StatsView &V, SearchCtx &X, hipStream_t s, const QueryBatch &qb,
                       uint32_t n_q, uint32_t k, uint32_t all_R2 = 0) {
  const std::vector<uint32_t> &qoff = qb.off, &slots = qb.slot;
  const size_t ns = slots.size(), nr = qb.ops ? ns + qb.meta.size() : 0;
  const size_t npairs = (size_t)n_q * S.n_blocks;
  const bool batch = k && npairs >= (size_t)ix->num_cus * 16 && npairs < (1ull << 32);
  // batches of plain disjunctions, k <= 64, block-major: workgroup per
  // (query, block range) unit (k_score_units); units of about unit_post
  // postings, queries above that split into equal block ranges, listed first
  // (heavy units start early, the light tail balances)
  std::vector<uint32_t> &units = X.q_units;
  units.clear();
  bool unit_path = batch && k <= kUnitMaxK && !qb.ops && !S.term_major && !knob("TFIDF_NO_UNITS");
  uint32_t n_wunits = 0;                 // the first n_wunits units are wave units
  if (unit_path) {
    std::vector<uint64_t> P(n_q, 0);
    uint64_t T = 0;
    for (uint32_t q = 0; q < n_q && unit_path; q++) {
      if (qoff[q + 1] - qoff[q] > kUnitMaxTerms) unit_path = false;
      for (uint32_t t = qoff[q]; t < qoff[q + 1]; t++)
        if (slots[t] != kInvalidSlot) P[q] += qb.ldf[t];
      T += P[q];
    }
    // light queries (at most light_post postings per block on average): wave
    // units (k_score_wunits, units of ~16 k postings); heavy ones: workgroup
    // units (k_score_units, dense block accumulator; ~T/4096 postings each)
    const uint32_t nb = S.n_blocks;
    uint64_t light_post = kWunitLightPost;
    if (const char *e = knob("TFIDF_WUNIT_LIGHT")) light_post = (uint64_t)atoll(e);   // A/B and test hook
    uint64_t unit_post = std::min<uint64_t>(std::max<uint64_t>(T / 4096, 8192), 1ull << 17);
    uint64_t wunit_post = 16384;
    if (const char *e = knob("TFIDF_UNIT_POST")) unit_post = wunit_post = std::max(1, atoi(e));   // test hook: force splits
    for (int pass = 0; pass < 3 && unit_path; pass++)        // light; heavy split; heavy whole
      for (uint32_t q = 0; q < n_q; q++) {
        const bool light = P[q] <= light_post * nb;
        if (light != (pass == 0)) continue;
        const uint64_t up = light ? wunit_post : unit_post;
        const uint64_t nch = std::min<uint64_t>(std::max<uint64_t>((P[q] + up - 1) / up, 1), nb);
        if (!light && (nch > 1) != (pass == 1)) continue;
        for (uint64_t c = 0; c < nch; c++) {
          units.push_back(q);
          units.push_back((uint32_t)(c * nb / nch));
          units.push_back((uint32_t)((c + 1) * nb / nch));
          units.push_back(0);
        }
        if (light) n_wunits += (uint32_t)nch;
      }
    if (!unit_path) units.clear();
  }
  const size_t words0 = (qoff.size() + 2 * ns + nr + 3) & ~(size_t)3;    // units 16-B aligned
  const size_t words = words0 + units.size();
  // one pinned staging buffer, one upload (the previous upload out of it must
  // have left: batch searches return before their copies run)
  if (X.q_in_pending) HIP_TRY(hipEventSynchronize(X.q_in_ev));
  HIP_TRY(X.q_host.resize(words));
  uint32_t *h = X.q_host.data();
  memcpy(h, qoff.data(), qoff.size() * 4);
  memcpy(h + qoff.size(), slots.data(), ns * 4);
  memcpy(h + qoff.size() + ns, qb.w.data(), ns * 4);
  if (qb.ops) {
    memcpy(h + qoff.size() + 2 * ns, qb.role.data(), ns * 4);
    memcpy(h + qoff.size() + 3 * ns, qb.meta.data(), qb.meta.size() * 4);
  }
  if (!units.empty()) memcpy(h + words0, units.data(), units.size() * 4);
  if (words * 4 + 16 > X.q_in.bytes) {
    // a pending chunk of a pipelined batch may still read q_in: finish it
    // before the buffer is replaced (1.5x headroom, so later chunks rarely grow it)
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(X.q_in.reserve(words * 6 + 16));
  }
  HIP_TRY(hipMemcpyAsync(X.q_in.p, h, words * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(X.q_in_ev, s));
  X.q_in_pending = true;
  uint32_t *din = X.q_in.as<uint32_t>();
  QueryParams qp{};
  qp.post = S.post.as<uint64_t>();
  qp.post32 = S.post.as<uint32_t>();
  qp.post_esc = S.post_esc.as<uint64_t>();
  qp.n_post_esc = S.h_post_esc.size();
  qp.bbase = S.bbase.as<uint64_t>();
  qp.blk = S.blk.as<uint32_t>();
  qp.toff = S.term_major ? S.toff.as<uint64_t>() : nullptr;
  qp.C = S.qcols();
  qp.n_blocks = S.n_blocks;
  qp.n_docs = S.n_docs;
  qp.cache = V.cache.as<float>();
  qp.q_off = din;
  qp.q_slot = din + qoff.size();
  qp.q_w = reinterpret_cast<const float *>(din + qoff.size() + ns);
  qp.q_role = qb.ops ? din + qoff.size() + 2 * ns : nullptr;
  qp.q_meta = qb.ops ? din + qoff.size() + 3 * ns : nullptr;
  qp.ops = qb.ops ? 1u : 0u;
  qp.n_q = n_q;
  qp.k = k;
  {   // enough (block, chunk) workgroups to fill the chip ~4 deep; never more chunks than queries
    const uint32_t want = (uint32_t)ix->num_cus * 4;
    uint32_t chunks = S.n_blocks ? (want + S.n_blocks - 1) / S.n_blocks : 1;
    chunks = std::max(1u, std::min(chunks, n_q));
    qp.q_chunk = (n_q + chunks - 1) / chunks;
  }
  if (k) {
    HIP_TRY(X.cand.reserve((size_t)n_q * S.n_blocks * k * 8 + 8));
    HIP_TRY(X.cand_n.reserve((size_t)n_q * S.n_blocks * 4 + 4));
    // results contiguous (doc | score | n): a single query reads them back in one copy
    HIP_TRY(X.q_out.reserve(((size_t)2 * n_q * k + n_q) * 4 + 16));
    X.res_doc = X.q_out.as<uint32_t>();
    X.res_score = reinterpret_cast<float *>(X.res_doc + (size_t)n_q * k);
    X.res_n = X.res_doc + (size_t)2 * n_q * k;
    qp.cand = X.cand.as<uint64_t>();
    qp.cand_n = X.cand_n.as<uint32_t>();
    qp.out_doc = X.res_doc;
    qp.out_score = X.res_score;
    qp.out_n = X.res_n;
  } else if (all_R2) {
    const size_t runs = (size_t)n_q * all_R2;
    HIP_TRY(X.hits.reserve(runs * kBlockDocs * 8 + 8));
    HIP_TRY(X.hits_n.reserve(runs * 4 + 4));
    qp.hits = X.hits.as<uint64_t>();
    qp.hits_n = X.hits_n.as<uint32_t>();
    qp.hits_R2 = all_R2;
    HIP_TRY(hipMemsetAsync(qp.hits_n, 0, runs * 4, s));   // the padding runs stay empty
  } else {
    HIP_TRY(X.hits.reserve((size_t)S.n_blocks * kBlockDocs * 8 + 8));
    HIP_TRY(X.hits_n.reserve((size_t)S.n_blocks * 4 + 4));
    qp.hits = X.hits.as<uint64_t>();
    qp.hits_n = X.hits_n.as<uint32_t>();
  }
  if (X.q_timing && X.q_rec_start) HIP_TRY(hipEventRecord(X.ev[QEV_0], s));
  if (unit_path) {
    HIP_TRY(X.ovf.reserve(64));
    uint32_t *ctr = X.ovf.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(ctr, 0, 8, s));
    const uint32_t n_units = (uint32_t)(units.size() / 4), n_gunits = n_units - n_wunits;
    ix->unit_batches++;
    ix->unit_count += n_units;
    const uint4 *ud = reinterpret_cast<const uint4 *>(din + words0);
    // both kinds at once: the wave units on the side stream (fork / join events),
    // so the two latency-bound kernels share the CUs instead of running in turn
    const bool both = n_wunits && n_gunits;
    hipStream_t ws = both ? X.side : s;
    if (both) {
      HIP_TRY(hipEventRecord(X.q_ev[0], s));
      HIP_TRY(hipStreamWaitEvent(ws, X.q_ev[0], 0));
    }
    if (n_wunits) {
      uint32_t wper_cu = kWunitWGsPerCU;
      if (const char *e = knob("TFIDF_WUNIT_WG_PER_CU")) wper_cu = (uint32_t)std::max(1, atoi(e));   // A/B
      const int grid = (int)std::min<uint64_t>((n_wunits + kWunitWavesPerWG - 1) / kWunitWavesPerWG,
                                               (uint64_t)ix->num_cus * wper_cu);
      HIP_TRY(launch_score_wunits(qp, ud, n_wunits, ctr, grid, ws));
    }
    if (n_gunits) {
      // (one per CU next to the wave units measured slower: 6.3 -> 7.8 ms at cfg 4)
      uint32_t per_cu = kUnitWGsPerCU;
      if (const char *e = knob("TFIDF_UNIT_WG_PER_CU")) per_cu = (uint32_t)std::max(1, atoi(e));   // A/B
      const int grid = (int)std::min<uint64_t>(n_gunits, (uint64_t)ix->num_cus * per_cu);
      HIP_TRY(launch_score_units(qp, ud + n_wunits, n_gunits, ctr + 1, grid, s));
    }
    if (both) {
      HIP_TRY(hipEventRecord(X.q_ev[1], ws));
      HIP_TRY(hipStreamWaitEvent(s, X.q_ev[1], 0));
    }
    if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_1], s));
    HIP_TRY(launch_merge_topk(qp, s));
    if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_2], s));
    return scoring_done();
  }
  if (batch) {
    // batches: wave per (block, query) pair; pairs with many postings are
    // listed for the dense per-block kernel (list mode, persistent grid).
    // Single queries keep the dense kernel: a few hundred pairs cannot fill
    // the chip one wave each.
    // plain heavy pairs -> ovf list (k_score_blocks<false>); pairs of operator
    // queries -> ovf2 list (k_score_blocks<true>)
    HIP_TRY(X.ovf.reserve(npairs * 8 + 64));
    qp.ovf_count = X.ovf.as<uint32_t>();
    qp.ovf2_count = qp.ovf_count + 1;
    qp.ovf_list = qp.ovf_count + 16;
    qp.ovf2_list = qp.ovf_list + npairs;
    qp.list_grid = (uint32_t)ix->num_cus * 2;
    HIP_TRY(hipMemsetAsync(qp.ovf_count, 0, 8, s));
    const uint64_t want = (npairs + kPairWavesPerWG - 1) / kPairWavesPerWG;
    const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ix->num_cus * 40));
    HIP_TRY(launch_score_pairs(qp, grid, s));
    qp.ops = 0;
    if (qb.ops) {
      QueryParams q2 = qp;
      q2.ovf_list = qp.ovf2_list;
      q2.ovf_count = qp.ovf2_count;
      q2.ops = 1;
      q2.list_grid = (uint32_t)ix->num_cus;          // one 134 KiB workgroup per CU
      HIP_TRY(launch_score_blocks(q2, s));
    }
  }
  HIP_TRY(launch_score_blocks(qp, s));
  if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_1], s));
  if (k) HIP_TRY(launch_merge_topk(qp, s));
  if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_2], s));
  return scoring_done();
}

// One search on a snapshot (tfidf_search: the published one; tfidf_reader_search:
// the reader's).
static int search_on(tfidf_index *ix, Snapshot &S, StatsView &V, const uint8_t *q, uint64_t q_len, uint32_t k,
                     uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *n_out) {
  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();
  if (k > 1024) return fail(TFIDF_E_INVALID_ARG, "k must be <= 1024 (0 = all hits)");
  DeviceGuard g(ix->cfg.device);
  PreparedQuery pq;
  int rc = prepare_query(S, V, q, q_len, &pq);
  if (rc) return rc;
  if (pq.slot.empty() || S.n_docs == 0) { set_route_ms(ix, 0, 0); return TFIDF_OK; }
  // fused path for k <= kFusedMaxK: each block workgroup writes its k
  // candidates to pinned host memory over PCIe and the host merges n_blocks x k
  // keys, a cost that grows with k (larger k: run_scoring + the device merge)
  if (k && k <= kFusedMaxK && pq.slot.size() <= kInlTerms && !knob("TFIDF_NO_FUSED")) {
    // one launch: query terms in the kernel arguments, block scoring with the
    // candidates written to pinned host memory, merged here
    HIP_TRY(X.q_res.resize((size_t)2 * k + 1));
    QueryParams qp{};
    qp.post = S.post.as<uint64_t>();
    qp.post32 = S.post.as<uint32_t>();
    qp.post_esc = S.post_esc.as<uint64_t>();
    qp.n_post_esc = S.h_post_esc.size();
    qp.bbase = S.bbase.as<uint64_t>();
    qp.blk = S.blk.as<uint32_t>();
    qp.toff = S.term_major ? S.toff.as<uint64_t>() : nullptr;
    qp.C = S.qcols();
    qp.n_blocks = S.n_blocks;
    qp.n_docs = S.n_docs;
    qp.cache = V.cache.as<float>();
    qp.inl_n = (uint32_t)pq.slot.size();
    qp.inl_meta = pq.meta;
    for (size_t i = 0; i < pq.slot.size(); i++) {
      qp.inl_slot[i] = pq.slot[i];
      qp.inl_w[i] = pq.w[i];
      qp.inl_role[i] = pq.role[i];
    }
    qp.ops = pq.meta != 0 ? 1u : 0u;
    qp.n_q = 1;
    qp.q_chunk = 1;
    qp.k = k;
    // the block workgroups write their candidates to pinned host memory; the
    // host merges them (a merge kernel + copies: p50 0.049 / 0.057 ms, this
    // path 0.034 ms; a last-workgroup merge in the scoring kernel 0.055 ms:
    // its device-scope fences cost more than the launch they save)
    HIP_TRY(X.q_cand_h.resize((size_t)S.n_blocks * k * 2 + S.n_blocks));
    qp.cand = reinterpret_cast<uint64_t *>(X.q_cand_h.data());
    qp.cand_n = X.q_cand_h.data() + (size_t)S.n_blocks * k * 2;
    if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_0], s));
    HIP_TRY(launch_score_blocks(qp, s));
    if (X.q_timing) {
      HIP_TRY(hipEventRecord(X.ev[QEV_1], s));
      HIP_TRY(hipEventRecord(X.ev[QEV_2], s));
    }
    ix->fused_queries++;
    HIP_TRY(hipStreamSynchronize(s));
    {
      // the blocks' candidate keys (score bits << 32 | ~doc: unique, key order =
      // score desc, doc asc) -> top k
      const uint64_t *ck = reinterpret_cast<const uint64_t *>(X.q_cand_h.data());
      const uint32_t *cn = X.q_cand_h.data() + (size_t)S.n_blocks * k * 2;
      std::vector<uint64_t> &all = X.q_merge;
      all.clear();
      for (uint32_t b = 0; b < S.n_blocks; b++)
        for (uint32_t i = 0; i < cn[b]; i++) all.push_back(ck[(size_t)b * k + i]);
      const size_t m = std::min<size_t>(k, all.size());
      std::partial_sort(all.begin(), all.begin() + m, all.end(), std::greater<uint64_t>());
      uint32_t *h = X.q_res.data();
      for (size_t i = 0; i < m; i++) {
        h[i] = ~(uint32_t)all[i];
        uint32_t sb = (uint32_t)(all[i] >> 32);
        memcpy(&h[k + i], &sb, 4);
      }
      h[2 * k] = (uint32_t)m;
    }
    const uint32_t n = X.q_res[2 * k];
    *n_out = n;
    if (n > cap) return fail(TFIDF_E_BUFFER, "need %u result slots", n);
    memcpy(doc_ids, X.q_res.data(), n * 4);
    memcpy(scores, X.q_res.data() + k, n * 4);
    set_last_ms(ix, qev_ms(X, QEV_0, QEV_1), qev_ms(X, QEV_0, QEV_2));
    return TFIDF_OK;
  }
  QueryBatch qb;
  qb.add(pq);
  rc = run_scoring(ix, S, V, X, s, qb, 1, k);
  if (rc) return rc;
  if (k) {
    // one copy of (doc[k] | score[k] | n) into pinned memory, one wait
    HIP_TRY(X.q_res.resize((size_t)2 * k + 1));
    HIP_TRY(hipMemcpyAsync(X.q_res.data(), X.res_doc, ((size_t)2 * k + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    X.q_in_pending = false;
    const uint32_t n = X.q_res[2 * k];
    *n_out = n;
    if (n > cap) return fail(TFIDF_E_BUFFER, "need %u result slots", n);
    memcpy(doc_ids, X.q_res.data(), n * 4);
    memcpy(scores, X.q_res.data() + k, n * 4);
    set_last_ms(ix, qev_ms(X, QEV_0, QEV_1), qev_ms(X, QEV_0, QEV_2));
    return TFIDF_OK;
  }
  // all hits: per-block sorted runs -> merge passes on the device -> (doc, score)
  const uint32_t R = S.n_blocks;
  HIP_TRY(X.hits_c.reserve((size_t)R * kBlockDocs * 8 + 8));
  HIP_TRY(X.hits_s.reserve((size_t)R * kBlockDocs * 8 + 8));
  HIP_TRY(X.hits_P.reserve(((size_t)R + 1) * 8));
  HIP_TRY(X.out_doc.reserve((size_t)R * kBlockDocs * 4 + 4));
  HIP_TRY(X.out_score.reserve((size_t)R * kBlockDocs * 4 + 4));
  HIP_TRY(launch_hits_order(X.hits.as<uint64_t>(), X.hits_n.as<uint32_t>(), R, X.hits_P.as<uint64_t>(),
                            X.hits_c.as<uint64_t>(), X.hits.as<uint64_t>(), X.hits_s.as<uint64_t>(),
                            X.out_doc.as<uint32_t>(),
                            X.out_score.as<float>(), nullptr, 0, hits_bound(S, pq), ix->num_cus * 4, s));
  if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_2], s));
  uint64_t H = 0;
  HIP_TRY(hipMemcpyAsync(&H, X.hits_P.as<uint64_t>() + R, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n_out = H;
  if (H > cap) return fail(TFIDF_E_BUFFER, "need %llu result slots", (unsigned long long)H);
  if (H) {
    HIP_TRY(hipMemcpyAsync(doc_ids, X.out_doc.p, H * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(scores, X.out_score.p, H * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  set_last_ms(ix, qev_ms(X, QEV_0, QEV_1), qev_ms(X, QEV_0, QEV_2));
  return TFIDF_OK;
}

extern "C" int tfidf_search(tfidf_index *ix, const uint8_t *q, uint64_t q_len, uint32_t k, uint32_t *doc_ids,
                            float *scores, uint64_t cap, uint64_t *n_out) {
  if (!ix || (!q && q_len) || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  *n_out = 0;
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "search before commit");
  return search_on(ix, *snap, *view, q, q_len, k, doc_ids, scores, cap, n_out);
}

static int doc_keys_of(const Snapshot *S, uint8_t *buf, uint64_t cap, uint64_t *offsets, uint64_t *n_bytes);

// ---- readers (Worker.java:223: DirectoryReader.open on the last commit per
// request; the hits' stored fields are read from that same reader, :234-238)
struct tfidf_reader {
  tfidf_index *ix;
  std::shared_ptr<Snapshot> S;
  std::shared_ptr<StatsView> V;
};

extern "C" int tfidf_reader_open(tfidf_index *ix, tfidf_reader **out) {
  if (!ix || !out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  *out = nullptr;
  std::shared_ptr<StatsView> v;
  std::shared_ptr<Snapshot> S = current(ix, &v);
  if (!S) return fail(TFIDF_E_STATE, "no commit to read");
  *out = new tfidf_reader{ix, std::move(S), std::move(v)};
  return TFIDF_OK;
}

extern "C" int tfidf_reader_close(tfidf_reader *rd) {
  delete rd;
  return TFIDF_OK;
}

extern "C" int tfidf_reader_info(const tfidf_reader *rd, uint64_t *generation, uint64_t *num_docs) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  if (generation) *generation = rd->S->generation;
  if (num_docs) *num_docs = rd->S->n_docs;
  return TFIDF_OK;
}

extern "C" int tfidf_reader_search(tfidf_reader *rd, const uint8_t *q, uint64_t q_len, uint32_t k, uint32_t *doc_ids,
                                   float *scores, uint64_t cap, uint64_t *n_out) {
  if (!rd || (!q && q_len) || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  *n_out = 0;
  return search_on(rd->ix, *rd->S, *rd->V, q, q_len, k, doc_ids, scores, cap, n_out);
}

extern "C" int tfidf_reader_doc_keys(const tfidf_reader *rd, uint8_t *buf, uint64_t cap, uint64_t *offsets,
                                     uint64_t *n_bytes) {
  if (!rd || !n_bytes || !offsets) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  return doc_keys_of(rd->S.get(), buf, cap, offsets, n_bytes);
}

extern "C" int tfidf_reader_doc_key(const tfidf_reader *rd, uint64_t doc, uint8_t *buf, uint64_t cap,
                                    uint64_t *n_out) {
  if (!rd || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (doc >= rd->S->n_docs) return fail(TFIDF_E_INVALID_ARG, "doc out of range");
  std::string k;
  rd->S->keys.key(rd->S->staged_of(doc), &k);
  *n_out = k.size();
  if (k.size() > cap) return fail(TFIDF_E_BUFFER, "key needs %zu bytes", k.size());
  if (buf && !k.empty()) memcpy(buf, k.data(), k.size());
  return TFIDF_OK;
}

static int doc_text_of(const Snapshot *S, uint64_t doc, uint8_t *buf, uint64_t cap, uint64_t *n_out);
extern "C" int tfidf_reader_doc_text(const tfidf_reader *rd, uint64_t doc, uint8_t *buf, uint64_t cap,
                                     uint64_t *n_out) {
  if (!rd || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  *n_out = 0;
  return doc_text_of(rd->S.get(), doc, buf, cap, n_out);
}

// ---------------------------------------------------------------------------
// hit highlighting: match offsets and snippets from the snapshot's own corpus
// (snippet_plan.h, kernels_highlight.hip)

struct HlOut {
  uint32_t W = 0;                       // snippet bytes; 0 = the matches of the whole documents
  uint8_t *text = nullptr;              // snippets only: packed bytes, their offsets, each snippet's
  uint64_t text_cap = 0;                // start in its document
  uint64_t *text_offsets = nullptr, *doc_starts = nullptr, *n_text = nullptr;
  uint64_t *starts = nullptr;           // matches (of the documents / inside the snippets)
  uint32_t *lens = nullptr, *ordinals = nullptr;
  uint64_t m_cap = 0;
  uint64_t *match_offsets = nullptr, *n_matches = nullptr;
  float *ms_device = nullptr;
};

// what tfidf_matches[_batch] fill
static HlOut hl_out_matches(uint64_t *starts, uint32_t *lens, uint32_t *ordinals, uint64_t cap,
                            uint64_t *match_offsets, uint64_t *n_out, float *ms_device) {
  HlOut o;
  o.starts = starts;
  o.lens = lens;
  o.ordinals = ordinals;
  o.m_cap = cap;
  o.match_offsets = match_offsets;
  o.n_matches = n_out;
  o.ms_device = ms_device;
  return o;
}

// what tfidf_snippets[_batch] fill
static HlOut hl_out_snippets(uint32_t max_bytes, uint8_t *text, uint64_t text_cap, uint64_t *text_offsets,
                             uint64_t *doc_starts, uint64_t *starts, uint32_t *lens, uint32_t *ordinals,
                             uint64_t m_cap, uint64_t *match_offsets, uint64_t *n_text, uint64_t *n_matches,
                             float *ms_device) {
  HlOut o = hl_out_matches(starts, lens, ordinals, m_cap, match_offsets, n_matches, ms_device);
  o.W = max_bytes;
  o.text = text;
  o.text_cap = text_cap;
  o.text_offsets = text_offsets;
  o.doc_starts = doc_starts;
  o.n_text = n_text;
  return o;
}

static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

static uint64_t hl_budget(const char *name, uint64_t dflt) {
  if (const char *e = knob(name)) return (uint64_t)std::max<long long>(1, atoll(e));   // tests: chunk edges anywhere
  return dflt;
}

constexpr uint64_t kHlChunkItems = 1ull << 16;     // (row, chunk) items per row chunk: 32 MiB of slice counts
constexpr uint64_t kHlChunkMatches = 1ull << 22;   // matches per row chunk: 128 MiB over hl_m + hl_o

// the rows of one call: at most 2^26, each a document of the snapshot
static int hl_check_rows(const Snapshot &S, const uint32_t *docs, uint64_t R) {
  if (R > (1ull << 26)) return fail(TFIDF_E_INVALID_ARG, "more than 2^26 rows in one call");
  for (uint64_t r = 0; r < R; r++)
    if (docs[r] >= S.n_docs) return fail(TFIDF_E_INVALID_ARG, "doc %u out of range", docs[r]);
  return TFIDF_OK;
}

// one query's key segment, appended to *keys: its positive terms that this
// snapshot holds, as dictionary keys (under its hash seed) with their ordinals,
// sorted on their own
static void hl_append_keys(Snapshot &S, const std::vector<std::string> &terms, std::vector<HlKey> *keys) {
  const size_t k0 = keys->size();
  for (size_t t = 0; t < terms.size(); t++) {
    const uint32_t slot = lookup_term(S, terms[t]);
    if (slot != kInvalidSlot) keys->push_back(HlKey{S.h_dict[slot], S.h_dict[(size_t)S.C + slot], (uint32_t)t, 0});
  }
  std::sort(keys->begin() + k0, keys->end(), [](const HlKey &x, const HlKey &y) { return hl_key_less(x, y); });
}

// The rows (query, document) of one call, single-query or batched: row r is
// docs[r] against the key segment [key_off[row_q[r]], key_off[row_q[r] + 1]) of
// its query (hl_check_rows has passed).  The chain of launches, copies and
// synchronisations is paid per call (per row chunk when the scratch budgets cut
// the rows), never per query.  report_chunks: the call is a batched one, whose
// chunks tfidf_last_highlight_chunks reports.
static int highlight_rows(tfidf_index *ix, Snapshot &S, const std::vector<HlKey> &keys,
                          const std::vector<uint32_t> &key_off, const std::vector<uint32_t> &row_q,
                          const uint32_t *docs, const HlOut &o, bool report_chunks) {
  const uint64_t R = row_q.size();
  const size_t n_q = key_off.size() - 1, n_keys = keys.size();
  for (uint64_t r = 0; r <= R; r++) {
    o.match_offsets[r] = 0;
    if (o.W) o.text_offsets[r] = 0;
  }
  *o.n_matches = 0;
  if (o.W) *o.n_text = 0;
  if (R == 0) return TFIDF_OK;

  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();
  DeviceGuard g(ix->cfg.device);
  const bool timed = o.ms_device != nullptr;
  auto finish = [&]() -> int {
    if (timed) HIP_TRY(hipEventRecord(X.ev[QEV_1], s));
    HIP_TRY(hipStreamSynchronize(s));
    if (timed) HIP_TRY(hipEventElapsedTime(o.ms_device, X.ev[QEV_0], X.ev[QEV_1]));
    return TFIDF_OK;
  };

  // the call's inputs, laid out on the host as on the device and sent in one copy: staged
  // ids, row -> query, key segments, keys; the extents follow them on the device
  const size_t in_rowq = up16(R * 4), in_koff = up16(in_rowq + R * 4), in_keys = up16(in_koff + (n_q + 1) * 4),
               in_ext = up16(in_keys + n_keys * sizeof(HlKey));
  std::vector<uint8_t> h_in(in_ext);
  uint32_t *h_staged = reinterpret_cast<uint32_t *>(h_in.data());
  for (uint64_t r = 0; r < R; r++) h_staged[r] = (uint32_t)S.staged_of(docs[r]);
  memcpy(h_in.data() + in_rowq, row_q.data(), R * 4);
  memcpy(h_in.data() + in_koff, key_off.data(), (n_q + 1) * 4);
  if (n_keys) memcpy(h_in.data() + in_keys, keys.data(), n_keys * sizeof(HlKey));
  std::vector<uint64_t> h_ext(2 * R);
  HIP_TRY(X.hl_in.reserve(in_ext + R * 16));
  uint8_t *ib = X.hl_in.as<uint8_t>();
  uint32_t *d_staged = reinterpret_cast<uint32_t *>(ib), *d_rowq = reinterpret_cast<uint32_t *>(ib + in_rowq),
           *d_koff = reinterpret_cast<uint32_t *>(ib + in_koff);
  uint64_t *d_ext = reinterpret_cast<uint64_t *>(ib + in_ext);
  HlKey *d_keys = reinterpret_cast<HlKey *>(ib + in_keys);
  const uint8_t *d_text = S.text->as<uint8_t>();
  if (timed) HIP_TRY(hipEventRecord(X.ev[QEV_0], s));
  HIP_TRY(hipMemcpyAsync(ib, h_in.data(), in_ext, hipMemcpyHostToDevice, s));
  HIP_TRY(launch_hl_extents(S.offsets->as<uint64_t>(), d_staged, R, d_ext, s));
  HIP_TRY(hipMemcpyAsync(h_ext.data(), d_ext, R * 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));

  // rows without work: an empty key segment, a malformed document (indexed empty)
  std::vector<uint8_t> skip(R);
  std::vector<uint64_t> row_items(R);
  for (uint64_t r = 0; r < R; r++) {
    skip[r] = key_off[row_q[r]] == key_off[row_q[r] + 1] ||
              (!S.malformed.empty() && std::binary_search(S.malformed.begin(), S.malformed.end(), docs[r]));
    row_items[r] = skip[r] ? 0 : hl_num_chunks(h_ext[2 * r + 1] - h_ext[2 * r]);
  }
  std::vector<uint64_t> cuts;
  hl_plan_chunks(row_items.data(), nullptr, 0, R, hl_budget("TFIDF_HL_CHUNK_ITEMS", kHlChunkItems), ~0ull, &cuts);
  const uint64_t budget_m = hl_budget("TFIDF_HL_CHUNK_MATCHES", kHlChunkMatches);

  uint64_t run_m = 0, run_t = 0;          // running totals: where the next chunk's payload goes
  uint64_t n_row_chunks = 0;
  bool fits = true;
  std::vector<HlItem> items;
  std::vector<uint64_t> first, h_row, row_m, sub, h_to, h_mo;
  for (size_t ci = 0; ci + 1 < cuts.size(); ci++) {
    const uint64_t r0 = cuts[ci], nr = cuts[ci + 1] - r0;
    hl_plan(h_ext.data() + 2 * r0, skip.data() + r0, nr, &items, &first);
    if (items.size() > (1ull << 24))
      return fail(TFIDF_E_INVALID_ARG, "a document of more than 2^24 chunks of %llu bytes",
                  (unsigned long long)kHlChunkBytes);
    const uint32_t n_items = (uint32_t)items.size();
    const uint64_t n_cnt = (uint64_t)n_items * kHlLanes;
    const size_t off_row = (nr + 1) * 8, off_items = 3 * off_row,
                 off_counts = up16(off_items + (size_t)n_items * sizeof(HlItem));
    HIP_TRY(X.hl_cnt.reserve(off_counts + (n_cnt + 1) * 8));
    uint8_t *cb = X.hl_cnt.as<uint8_t>();
    uint64_t *d_first = reinterpret_cast<uint64_t *>(cb), *d_row = reinterpret_cast<uint64_t *>(cb + off_row),
             *d_row_sub = reinterpret_cast<uint64_t *>(cb + 2 * off_row),
             *d_counts = reinterpret_cast<uint64_t *>(cb + off_counts);
    HlItem *d_items = reinterpret_cast<HlItem *>(cb + off_items);
    h_row.assign(nr + 1, 0);
    if (n_items) {
      // count per slice, scan, row offsets: the chunk's totals before any match is stored
      HIP_TRY(hipMemcpyAsync(d_first, first.data(), (nr + 1) * 8, hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemcpyAsync(d_items, items.data(), (size_t)n_items * sizeof(HlItem), hipMemcpyHostToDevice, s));
      HIP_TRY(launch_hl_scan(false, d_text, d_ext + 2 * r0, d_items, n_items, d_keys, d_koff, d_rowq + r0,
                                   S.hash_seed, d_counts, 0, nullptr, nullptr, nullptr, s));
      HIP_TRY(exclusive_scan_u64(d_counts, d_counts, n_cnt, s));
      HIP_TRY(launch_hl_row_offsets(d_counts, d_first, nr, 0, d_row, s));
      HIP_TRY(hipMemcpyAsync(h_row.data(), d_row, (nr + 1) * 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
    } else {
      HIP_TRY(hipMemsetAsync(d_row, 0, (nr + 1) * 8, s));
    }
    if (!o.W) {
      for (uint64_t i = 1; i <= nr; i++) o.match_offsets[r0 + i] = run_m + h_row[i];
      fits = fits && run_m + h_row[nr] <= o.m_cap && (!h_row[nr] || (o.starts && o.lens && o.ordinals));
      if (!fits) {                          // the sizes alone from here on
        run_m += h_row[nr];
        n_row_chunks++;
        continue;
      }
    }
    // the rows of the item chunk by the match budget
    row_m.resize(nr);
    for (uint64_t i = 0; i < nr; i++) row_m[i] = h_row[i + 1] - h_row[i];
    sub.clear();
    hl_plan_chunks(nullptr, row_m.data(), 0, nr, ~0ull, budget_m, &sub);
    for (size_t si = 0; si + 1 < sub.size(); si++) {
      const uint64_t s0 = sub[si], ns = sub[si + 1] - s0, m_base = h_row[s0], T = h_row[s0 + ns] - m_base;
      const uint64_t Tc = std::max<uint64_t>(T, 1);
      n_row_chunks++;
      const uint32_t i0 = (uint32_t)first[s0], ni = (uint32_t)first[s0 + ns] - i0;
      HIP_TRY(X.hl_m.reserve(Tc * 16));
      uint64_t *m_st = X.hl_m.as<uint64_t>();
      uint32_t *m_ln = reinterpret_cast<uint32_t *>(m_st + Tc), *m_od = m_ln + Tc;
      if (T)
        HIP_TRY(launch_hl_scan(true, d_text, d_ext + 2 * r0, d_items + i0, ni, d_keys, d_koff, d_rowq + r0,
                                     S.hash_seed, d_counts + (uint64_t)i0 * kHlLanes, m_base, m_st, m_ln, m_od, s));
      if (!o.W) {
        if (T) {
          HIP_TRY(hipMemcpyAsync(o.starts + run_m, m_st, T * 8, hipMemcpyDeviceToHost, s));
          HIP_TRY(hipMemcpyAsync(o.lens + run_m, m_ln, T * 4, hipMemcpyDeviceToHost, s));
          HIP_TRY(hipMemcpyAsync(o.ordinals + run_m, m_od, T * 4, hipMemcpyDeviceToHost, s));
        }
        run_m += T;
        continue;
      }
      // snippets: the chunk's matches stay on the device; its packed snippets,
      // offsets and in-snippet matches come back at the running totals
      const uint64_t *d_ext_s = d_ext + 2 * (r0 + s0);
      const uint64_t *d_row_s = d_row + s0;
      if (m_base) {
        HIP_TRY(launch_hl_row_offsets(d_counts, d_first + s0, ns, m_base, d_row_sub, s));
        d_row_s = d_row_sub;
      }
      uint64_t text_bound = 0;
      for (uint64_t i = 0; i < ns; i++) {
        const uint64_t r = r0 + s0 + i;
        text_bound += std::min<uint64_t>(h_ext[2 * r + 1] - h_ext[2 * r], o.W);
      }
      HIP_TRY(X.hl_s.reserve((4 * ns + 2) * 8));
      HIP_TRY(X.hl_o.reserve(Tc * 16 + text_bound + 16));
      uint64_t *sn_a = X.hl_s.as<uint64_t>(), *sn_len = sn_a + ns, *in_first = sn_len + ns + 1, *in_cnt = in_first + ns;
      uint64_t *o_st = X.hl_o.as<uint64_t>();
      uint32_t *o_ln = reinterpret_cast<uint32_t *>(o_st + Tc), *o_od = o_ln + Tc;
      uint8_t *o_text = reinterpret_cast<uint8_t *>(o_od + Tc);
      HIP_TRY(launch_hl_rank(d_text, d_ext_s, d_row_s, m_st, m_ln, m_od, o.W, ns, sn_a, sn_len, in_first, in_cnt, s));
      HIP_TRY(exclusive_scan_u64(sn_len, sn_len, ns, s));
      HIP_TRY(exclusive_scan_u64(in_cnt, in_cnt, ns, s));
      if (fits)
        HIP_TRY(launch_hl_pack(d_text, d_ext_s, sn_a, sn_len, o_text, m_st, m_ln, m_od, in_first, in_cnt, o_st, o_ln,
                               o_od, ns, s));
      h_to.resize(ns + 1);
      h_mo.resize(ns + 1);
      HIP_TRY(hipMemcpyAsync(h_to.data(), sn_len, (ns + 1) * 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(h_mo.data(), in_cnt, (ns + 1) * 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(o.doc_starts + r0 + s0, sn_a, ns * 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      for (uint64_t i = 1; i <= ns; i++) {
        o.text_offsets[r0 + s0 + i] = run_t + h_to[i];
        o.match_offsets[r0 + s0 + i] = run_m + h_mo[i];
      }
      const uint64_t nt = h_to[ns], nm = h_mo[ns];
      fits = fits && run_t + nt <= o.text_cap && run_m + nm <= o.m_cap && (!nt || o.text) &&
             (!nm || (o.starts && o.lens && o.ordinals));
      if (fits) {
        if (nt) HIP_TRY(hipMemcpyAsync(o.text + run_t, o_text, nt, hipMemcpyDeviceToHost, s));
        if (nm) {
          HIP_TRY(hipMemcpyAsync(o.starts + run_m, o_st, nm * 8, hipMemcpyDeviceToHost, s));
          HIP_TRY(hipMemcpyAsync(o.lens + run_m, o_ln, nm * 4, hipMemcpyDeviceToHost, s));
          HIP_TRY(hipMemcpyAsync(o.ordinals + run_m, o_od, nm * 4, hipMemcpyDeviceToHost, s));
        }
      }
      run_t += nt;
      run_m += nm;
    }
  }
  *o.n_matches = run_m;
  if (o.W) *o.n_text = run_t;
  if (int rc = finish()) return rc;
  if (report_chunks) {
    std::lock_guard<std::mutex> lk(ix->ms_mu);
    ix->last_hl_item_chunks = cuts.size() - 1;
    ix->last_hl_row_chunks = n_row_chunks;
  }
  if (!fits) {
    if (o.W)
      return fail(TFIDF_E_BUFFER, "need %llu text bytes and %llu match slots", (unsigned long long)run_t,
                  (unsigned long long)run_m);
    return fail(TFIDF_E_BUFFER, "need %llu match slots", (unsigned long long)run_m);
  }
  return TFIDF_OK;
}

// The single-query forms: the batch of one query over all n rows.  Unlike a
// batch, they report a query that does not parse, before any other check.
static int highlight_one_on(tfidf_index *ix, Snapshot &S, const uint8_t *q, uint64_t q_len, const uint32_t *docs,
                            uint64_t n, const HlOut &o) {
  if (o.ms_device) *o.ms_device = 0.0f;
  std::vector<std::string> terms;
  const int prc = positive_terms(q, q_len, &terms);
  if (prc == kQBadUtf8) return fail(TFIDF_E_UNSUPPORTED_QUERY, "query is not valid UTF-8");
  if (prc == kQSyntax)
    return fail(TFIDF_E_QUERY_SYNTAX, "query does not parse (QueryParser ParseException / TooManyClauses)");
  if (int rc = hl_check_rows(S, docs, n)) return rc;
  std::vector<HlKey> keys;
  hl_append_keys(S, terms, &keys);
  return highlight_rows(ix, S, keys, {0, (uint32_t)keys.size()}, std::vector<uint32_t>(n, 0), docs, o, false);
}

static int matches_on(tfidf_index *ix, Snapshot &S, const uint8_t *q, uint64_t q_len, const uint32_t *docs,
                      uint64_t n_docs, uint64_t *starts, uint32_t *lens, uint32_t *ordinals, uint64_t cap,
                      uint64_t *match_offsets, uint64_t *n_out, float *ms_device) {
  if ((!q && q_len) || (!docs && n_docs) || !match_offsets || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  return highlight_one_on(ix, S, q, q_len, docs, n_docs,
                          hl_out_matches(starts, lens, ordinals, cap, match_offsets, n_out, ms_device));
}

static int snippets_on(tfidf_index *ix, Snapshot &S, const uint8_t *q, uint64_t q_len, const uint32_t *docs,
                       uint64_t n_docs, uint32_t max_bytes, uint8_t *text, uint64_t text_cap, uint64_t *text_offsets,
                       uint64_t *doc_starts, uint64_t *starts, uint32_t *lens, uint32_t *ordinals, uint64_t m_cap,
                       uint64_t *match_offsets, uint64_t *n_text, uint64_t *n_matches, float *ms_device) {
  if ((!q && q_len) || (!docs && n_docs) || !text_offsets || (!doc_starts && n_docs) || !match_offsets || !n_text ||
      !n_matches)
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (max_bytes < kHlMinBytes || max_bytes > kHlMaxBytes)
    return fail(TFIDF_E_INVALID_ARG, "max_bytes %u outside %u..%u", max_bytes, kHlMinBytes, kHlMaxBytes);
  return highlight_one_on(ix, S, q, q_len, docs, n_docs,
                          hl_out_snippets(max_bytes, text, text_cap, text_offsets, doc_starts, starts, lens, ordinals,
                                          m_cap, match_offsets, n_text, n_matches, ms_device));
}

extern "C" int tfidf_reader_matches(tfidf_reader *rd, const uint8_t *q, uint64_t q_len, const uint32_t *docs,
                                    uint64_t n_docs, uint64_t *starts, uint32_t *lens, uint32_t *ordinals,
                                    uint64_t cap, uint64_t *match_offsets, uint64_t *n_out, float *ms_device) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  return matches_on(rd->ix, *rd->S, q, q_len, docs, n_docs, starts, lens, ordinals, cap, match_offsets, n_out,
                    ms_device);
}

extern "C" int tfidf_matches(tfidf_index *ix, const uint8_t *q, uint64_t q_len, const uint32_t *docs, uint64_t n_docs,
                             uint64_t *starts, uint32_t *lens, uint32_t *ordinals, uint64_t cap,
                             uint64_t *match_offsets, uint64_t *n_out, float *ms_device) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "matches before commit");
  return matches_on(ix, *snap, q, q_len, docs, n_docs, starts, lens, ordinals, cap, match_offsets, n_out, ms_device);
}

extern "C" int tfidf_reader_snippets(tfidf_reader *rd, const uint8_t *q, uint64_t q_len, const uint32_t *docs,
                                     uint64_t n_docs, uint32_t max_bytes, uint8_t *text, uint64_t text_cap,
                                     uint64_t *text_offsets, uint64_t *doc_starts, uint64_t *starts, uint32_t *lens,
                                     uint32_t *ordinals, uint64_t m_cap, uint64_t *match_offsets, uint64_t *n_text,
                                     uint64_t *n_matches, float *ms_device) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  return snippets_on(rd->ix, *rd->S, q, q_len, docs, n_docs, max_bytes, text, text_cap, text_offsets, doc_starts,
                     starts, lens, ordinals, m_cap, match_offsets, n_text, n_matches, ms_device);
}

extern "C" int tfidf_snippets(tfidf_index *ix, const uint8_t *q, uint64_t q_len, const uint32_t *docs, uint64_t n_docs,
                              uint32_t max_bytes, uint8_t *text, uint64_t text_cap, uint64_t *text_offsets,
                              uint64_t *doc_starts, uint64_t *starts, uint32_t *lens, uint32_t *ordinals,
                              uint64_t m_cap, uint64_t *match_offsets, uint64_t *n_text, uint64_t *n_matches,
                              float *ms_device) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "snippets before commit");
  return snippets_on(ix, *snap, q, q_len, docs, n_docs, max_bytes, text, text_cap, text_offsets, doc_starts, starts,
                     lens, ordinals, m_cap, match_offsets, n_text, n_matches, ms_device);
}

// ---------------------------------------------------------------------------
// batched hit highlighting: the rows (query, document) of many queries in one
// call.  Row r's result is the single-query call's for (its query, docs[r]):
// both are highlight_rows.

static int highlight_batch_on(tfidf_index *ix, Snapshot &S, const uint8_t *q_utf8, const uint64_t *q_offsets,
                              uint32_t n_q, const uint32_t *docs, const uint64_t *doc_offsets, const HlOut &o) {
  if (o.ms_device) *o.ms_device = 0.0f;
  if (doc_offsets[0] != 0) return fail(TFIDF_E_INVALID_ARG, "doc_offsets[0] is not 0");
  for (uint32_t i = 0; i < n_q; i++) {
    if (doc_offsets[i + 1] < doc_offsets[i]) return fail(TFIDF_E_INVALID_ARG, "doc_offsets decrease at query %u", i);
    if (q_offsets[i + 1] < q_offsets[i]) return fail(TFIDF_E_INVALID_ARG, "q_offsets decrease at query %u", i);
  }
  const uint64_t R = doc_offsets[n_q];
  if (int rc = hl_check_rows(S, docs, R)) return rc;

  // every query's key segment; a query that does not parse has an empty one (no matches)
  std::vector<HlKey> keys;
  std::vector<uint32_t> key_off((size_t)n_q + 1, 0), row_q(R);
  std::vector<std::string> terms;
  for (uint32_t i = 0; i < n_q; i++) {
    key_off[i] = (uint32_t)keys.size();
    for (uint64_t r = doc_offsets[i]; r < doc_offsets[i + 1]; r++) row_q[r] = i;
    if (doc_offsets[i + 1] == doc_offsets[i]) continue;
    terms.clear();
    if (positive_terms(q_utf8 + q_offsets[i], q_offsets[i + 1] - q_offsets[i], &terms) != 0) continue;
    hl_append_keys(S, terms, &keys);
    if (keys.size() > (1ull << 31)) return fail(TFIDF_E_INVALID_ARG, "more than 2^31 query terms in one call");
  }
  key_off[n_q] = (uint32_t)keys.size();
  return highlight_rows(ix, S, keys, key_off, row_q, docs, o, true);
}

static int matches_batch_on(tfidf_index *ix, Snapshot &S, const uint8_t *q_utf8, const uint64_t *q_offsets,
                            uint32_t n_q, const uint32_t *docs, const uint64_t *doc_offsets, uint64_t *starts,
                            uint32_t *lens, uint32_t *ordinals, uint64_t cap, uint64_t *match_offsets, uint64_t *n_out,
                            float *ms_device) {
  if ((n_q && (!q_offsets || (!q_utf8 && q_offsets[n_q]))) || !doc_offsets || (!docs && doc_offsets[n_q]) ||
      !match_offsets || !n_out)
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  return highlight_batch_on(ix, S, q_utf8, q_offsets, n_q, docs, doc_offsets,
                            hl_out_matches(starts, lens, ordinals, cap, match_offsets, n_out, ms_device));
}

static int snippets_batch_on(tfidf_index *ix, Snapshot &S, const uint8_t *q_utf8, const uint64_t *q_offsets,
                             uint32_t n_q, const uint32_t *docs, const uint64_t *doc_offsets, uint32_t max_bytes,
                             uint8_t *text, uint64_t text_cap, uint64_t *text_offsets, uint64_t *doc_starts,
                             uint64_t *starts, uint32_t *lens, uint32_t *ordinals, uint64_t m_cap,
                             uint64_t *match_offsets, uint64_t *n_text, uint64_t *n_matches, float *ms_device) {
  if ((n_q && (!q_offsets || (!q_utf8 && q_offsets[n_q]))) || !doc_offsets || (!docs && doc_offsets[n_q]) ||
      !text_offsets || (!doc_starts && doc_offsets[n_q]) || !match_offsets || !n_text || !n_matches)
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (max_bytes < kHlMinBytes || max_bytes > kHlMaxBytes)
    return fail(TFIDF_E_INVALID_ARG, "max_bytes %u outside %u..%u", max_bytes, kHlMinBytes, kHlMaxBytes);
  return highlight_batch_on(ix, S, q_utf8, q_offsets, n_q, docs, doc_offsets,
                            hl_out_snippets(max_bytes, text, text_cap, text_offsets, doc_starts, starts, lens,
                                            ordinals, m_cap, match_offsets, n_text, n_matches, ms_device));
}

extern "C" int tfidf_reader_matches_batch(tfidf_reader *rd, const uint8_t *q_utf8, const uint64_t *q_offsets,
                                          uint32_t n_q, const uint32_t *docs, const uint64_t *doc_offsets,
                                          uint64_t *starts, uint32_t *lens, uint32_t *ordinals, uint64_t cap,
                                          uint64_t *match_offsets, uint64_t *n_out, float *ms_device) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  return matches_batch_on(rd->ix, *rd->S, q_utf8, q_offsets, n_q, docs, doc_offsets, starts, lens, ordinals, cap,
                          match_offsets, n_out, ms_device);
}

extern "C" int tfidf_matches_batch(tfidf_index *ix, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                   const uint32_t *docs, const uint64_t *doc_offsets, uint64_t *starts, uint32_t *lens,
                                   uint32_t *ordinals, uint64_t cap, uint64_t *match_offsets, uint64_t *n_out,
                                   float *ms_device) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "matches before commit");
  return matches_batch_on(ix, *snap, q_utf8, q_offsets, n_q, docs, doc_offsets, starts, lens, ordinals, cap,
                          match_offsets, n_out, ms_device);
}

extern "C" int tfidf_reader_snippets_batch(tfidf_reader *rd, const uint8_t *q_utf8, const uint64_t *q_offsets,
                                           uint32_t n_q, const uint32_t *docs, const uint64_t *doc_offsets,
                                           uint32_t max_bytes, uint8_t *text, uint64_t text_cap,
                                           uint64_t *text_offsets, uint64_t *doc_starts, uint64_t *starts,
                                           uint32_t *lens, uint32_t *ordinals, uint64_t m_cap,
                                           uint64_t *match_offsets, uint64_t *n_text, uint64_t *n_matches,
                                           float *ms_device) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  return snippets_batch_on(rd->ix, *rd->S, q_utf8, q_offsets, n_q, docs, doc_offsets, max_bytes, text, text_cap,
                           text_offsets, doc_starts, starts, lens, ordinals, m_cap, match_offsets, n_text, n_matches,
                           ms_device);
}

extern "C" int tfidf_snippets_batch(tfidf_index *ix, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                    const uint32_t *docs, const uint64_t *doc_offsets, uint32_t max_bytes,
                                    uint8_t *text, uint64_t text_cap, uint64_t *text_offsets, uint64_t *doc_starts,
                                    uint64_t *starts, uint32_t *lens, uint32_t *ordinals, uint64_t m_cap,
                                    uint64_t *match_offsets, uint64_t *n_text, uint64_t *n_matches,
                                    float *ms_device) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "snippets before commit");
  return snippets_batch_on(ix, *snap, q_utf8, q_offsets, n_q, docs, doc_offsets, max_bytes, text, text_cap,
                           text_offsets, doc_starts, starts, lens, ordinals, m_cap, match_offsets, n_text, n_matches,
                           ms_device);
}

extern "C" int tfidf_last_highlight_chunks(const tfidf_index *ix, uint64_t *item_chunks, uint64_t *row_chunks) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->ms_mu);
  if (item_chunks) *item_chunks = ix->last_hl_item_chunks;
  if (row_chunks) *row_chunks = ix->last_hl_row_chunks;
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// fuzzy term lookup: the vocabulary terms within max_edits of each input term
// (fuzzy_plan.h, kernels_fuzzy.hip).  Per scan chunk of input terms: one
// counting pass over the dictionary (n_within and the scratch sizes), then per
// candidate chunk a filling pass, the (term, dist, df) sort and the selection
// of what the host orders: the first max_out candidates of a term and the tie
// group of the max_out-th.  Only those candidates' strings are materialised
// (exact keys from the host mirror, hashed ones from their reference
// occurrence), where the byte order breaks the ties.

constexpr uint64_t kFzCandBudget = 1ull << 22;   // candidates per fill: 96 MiB of keys and slots, both sort buffers
constexpr uint32_t kFzHashedInit = 1u << 16;     // hashed slots listed before the list is grown and the scan redone

// One entry of a fuzzy search's expansion, and the expansions of a call's input
// terms in selection order (fuzzy_search_plan.h).
struct FzsEntry {
  uint32_t slot, dist, boost_bits;
};
typedef std::vector<std::vector<FzsEntry>> FuzzyExpansions;

// ex != nullptr: the fuzzy search's expansion instead of the lookup's lists:
// candidates by fzs_keep, sorted by fzs_sort_key, the first max_out <=
// kFzsMaxExpansions of each term selected and ordered on the device
// (k_fzs_select); out then carries n_within and the device time only.
static int fuzzy_on(tfidf_index *ix, Snapshot &S, const uint8_t *t_utf8, const uint64_t *t_offsets, uint32_t n_terms,
                    uint32_t max_edits, uint32_t prefix_len, uint32_t max_out, FuzzyLists *out,
                    FuzzyExpansions *ex = nullptr) {
  out->ms_device = 0.0f;
  out->cands.assign(n_terms, {});
  if (ex) ex->assign(n_terms, {});
  out->n_within.assign(n_terms, 0);
  // input terms -> lower-cased code points (none: a term without candidates)
  std::vector<std::vector<uint32_t>> cps(n_terms);
  std::vector<uint32_t> n_cps(n_terms, 0);
  uint32_t buf[kMaxTokenLen];
  bool any = false;
  for (uint32_t i = 0; i < n_terms; i++) {
    const uint64_t len = t_offsets[i + 1] - t_offsets[i];
    if (len == 0 || len > 4ull * kMaxTokenLen) continue;
    n_cps[i] = fz_decode_term(t_utf8 + t_offsets[i], len, buf);
    cps[i].assign(buf, buf + n_cps[i]);
    any = any || n_cps[i];
  }
  uint64_t n_scan = 0, n_fill = 0;
  auto publish = [&]() {
    std::lock_guard<std::mutex> lk(ix->ms_mu);
    ix->last_fz_scan_chunks = n_scan;
    ix->last_fz_cand_chunks = n_fill;
  };
  if (!any) { publish(); return TFIDF_OK; }
  std::vector<uint64_t> cuts;
  fz_plan_scan_chunks(n_cps.data(), n_terms, kFzChunkTerms, kFzChunkCps, &cuts);
  const uint64_t budget = std::min<uint64_t>(hl_budget("TFIDF_FUZZY_CAND_BUDGET", kFzCandBudget), 1ull << 30);

  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();
  DeviceGuard g(ix->cfg.device);
  const int max_grid = ix->num_cus * 8;
  HIP_TRY(hipEventRecord(X.ev[QEV_0], s));

  // staged terms and counters: off[kFzChunkTerms + 1], cps[kFzChunkCps], counts[kFzChunkTerms], seg and
  // out_off [kFzChunkTerms + 1] each, take[kFzChunkTerms], the fill cursor and the hashed-slot count
  const size_t in_cps = (kFzChunkTerms + 1) * 4, in_cnt = in_cps + kFzChunkCps * 4, in_seg = in_cnt + kFzChunkTerms * 4,
               in_oo = in_seg + (kFzChunkTerms + 1) * 4, in_take = in_oo + (kFzChunkTerms + 1) * 4,
               in_cur = in_take + kFzChunkTerms * 4, in_end = in_cur + 8;
  HIP_TRY(X.fz_in.reserve(in_end));
  uint8_t *ib = X.fz_in.as<uint8_t>();
  uint32_t *d_off = reinterpret_cast<uint32_t *>(ib), *d_cps = reinterpret_cast<uint32_t *>(ib + in_cps),
           *d_cnt = reinterpret_cast<uint32_t *>(ib + in_cnt), *d_seg = reinterpret_cast<uint32_t *>(ib + in_seg),
           *d_oo = reinterpret_cast<uint32_t *>(ib + in_oo), *d_take = reinterpret_cast<uint32_t *>(ib + in_take),
           *d_cur = reinterpret_cast<uint32_t *>(ib + in_cur), *d_hsn = d_cur + 1;

  FzScan a{};
  a.dict = S.dict.as<uint64_t>();
  a.df = S.df_dev();
  a.C = S.C;
  a.t_off = d_off;
  a.t_cps = d_cps;
  a.max_edits = max_edits;
  a.prefix_len = prefix_len;
  a.search = ex ? 1u : 0u;
  a.counts = d_cnt;
  a.cursor = d_cur;
  const uint8_t *d_text = S.text->as<uint8_t>();
  bool listed = false;                     // the hashed slots are listed by the first counting scan
  uint32_t hs_n = 0;

  FzStage st;
  std::vector<uint32_t> counts, seg, take, oo, h_slots;
  std::vector<uint64_t> sub, h_keys;
  std::vector<uint8_t> h_sel;
  std::string ts;
  for (size_t ci = 0; ci + 1 < cuts.size(); ci++) {
    const uint64_t t0 = cuts[ci], nt = cuts[ci + 1] - t0;
    fz_stage_terms(cps, t0, t0 + nt, &st);
    if (st.cps.empty()) continue;                                   // only terms without candidates
    if (nt > kFzChunkTerms || st.cps.size() > kFzChunkCps) return fail(TFIDF_E_STATE, "fuzzy scan chunk over its limits");
    n_scan++;
    HIP_TRY(hipMemcpyAsync(d_off, st.off.data(), (nt + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_cps, st.cps.data(), st.cps.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, nt * 4, s));
    a.n_terms = (uint32_t)nt;
    a.t_off = d_off;
    a.keys = nullptr;
    a.slots = nullptr;
    a.cap = 0;
    a.hs_list = nullptr;
    a.hs_cap = 0;
    if (!listed) {
      HIP_TRY(X.fz_hs.reserve((size_t)kFzHashedInit * 4));
      HIP_TRY(hipMemsetAsync(d_hsn, 0, 4, s));
      a.hs_list = X.fz_hs.as<uint32_t>();
      a.hs_count = d_hsn;
      a.hs_cap = (uint32_t)(X.fz_hs.bytes / 4);
    }
    HIP_TRY(launch_fz_scan(false, a, max_grid, s));
    if (!listed) {
      HIP_TRY(hipMemcpyAsync(&hs_n, d_hsn, 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      if (hs_n > a.hs_cap) {                                        // more hashed slots than the list held: list them again
        HIP_TRY(X.fz_hs.reserve((size_t)hs_n * 4));
        HIP_TRY(hipMemsetAsync(d_hsn, 0, 4, s));
        FzScan l = a;
        l.n_terms = 0;
        l.hs_list = X.fz_hs.as<uint32_t>();
        l.hs_cap = hs_n;
        HIP_TRY(launch_fz_scan(false, l, max_grid, s));
      }
      listed = true;
    }
    a.hs_list = X.fz_hs.as<uint32_t>();
    a.hs_count = nullptr;
    a.hs_n = hs_n;
    HIP_TRY(launch_fz_hashed(false, a, d_text, S.text_bytes, max_grid, s));
    counts.resize(nt);
    HIP_TRY(hipMemcpyAsync(counts.data(), d_cnt, nt * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint64_t t = 0; t < nt; t++) out->n_within[t0 + t] = counts[t];

    sub.clear();
    fz_plan_cand_chunks(counts.data(), 0, nt, budget, &sub);
    for (size_t si = 0; si + 1 < sub.size(); si++) {
      const uint64_t a0 = sub[si], na = sub[si + 1] - a0;
      seg.assign(na + 1, 0);
      uint64_t T = 0;
      for (uint64_t t = 0; t < na; t++) {
        T += counts[a0 + t];
        if (T >= (1ull << 31)) return fail(TFIDF_E_INVALID_ARG, "more than 2^31 candidates for one term range");
        seg[t + 1] = (uint32_t)T;
      }
      if (T == 0) continue;
      n_fill++;
      // candidates: keys [T] x 2 (sort in / out), slots [T] x 2
      const size_t Tp = (T + 1) & ~(size_t)1;
      HIP_TRY(X.fz_c.reserve(Tp * 24));
      uint64_t *k_in = X.fz_c.as<uint64_t>(), *k_out = k_in + Tp;
      uint32_t *s_in = reinterpret_cast<uint32_t *>(k_out + Tp), *s_out = s_in + Tp;
      HIP_TRY(hipMemsetAsync(d_cur, 0, 4, s));
      FzScan f = a;
      f.t_off = d_off + a0;                 // the range's terms: offsets into the chunk's code points
      f.n_terms = (uint32_t)na;
      f.keys = k_in;
      f.slots = s_in;
      f.cap = (uint32_t)T;
      HIP_TRY(launch_fz_scan(true, f, max_grid, s));
      HIP_TRY(launch_fz_hashed(true, f, d_text, S.text_bytes, max_grid, s));
      size_t tmp_bytes = 0;
      HIP_TRY(fz_sort(nullptr, &tmp_bytes, k_in, k_out, s_in, s_out, (uint32_t)T, s));
      HIP_TRY(X.fz_tmp.reserve(tmp_bytes));
      tmp_bytes = X.fz_tmp.bytes;
      HIP_TRY(fz_sort(X.fz_tmp.p, &tmp_bytes, k_in, k_out, s_in, s_out, (uint32_t)T, s));
      if (ex) {
        // the expansions, selected and ordered on the device: counts [na], keys and slots [na][kFzsMaxExpansions]
        const size_t o_keys = up16(na * 4), o_slots = o_keys + na * kFzsMaxExpansions * 8,
                     o_end = o_slots + na * kFzsMaxExpansions * 4;
        HIP_TRY(X.fz_o.reserve(o_end));
        uint8_t *ob = X.fz_o.as<uint8_t>();
        HIP_TRY(hipMemcpyAsync(d_seg, seg.data(), (na + 1) * 4, hipMemcpyHostToDevice, s));
        FzsSelect q{};
        q.keys = k_out;
        q.slots = s_out;
        q.seg = d_seg;
        q.n_terms = (uint32_t)na;
        q.E = max_out;
        q.dict = a.dict;
        q.C = S.C;
        q.text = d_text;
        q.text_bytes = S.text_bytes;
        q.out_n = reinterpret_cast<uint32_t *>(ob);
        q.out_keys = reinterpret_cast<uint64_t *>(ob + o_keys);
        q.out_slots = reinterpret_cast<uint32_t *>(ob + o_slots);
        HIP_TRY(launch_fzs_select(q, s));
        h_sel.resize(o_end);
        HIP_TRY(hipMemcpyAsync(h_sel.data(), ob, o_end, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const uint32_t *h_n = reinterpret_cast<const uint32_t *>(h_sel.data());
        const uint64_t *h_k = reinterpret_cast<const uint64_t *>(h_sel.data() + o_keys);
        const uint32_t *h_s = reinterpret_cast<const uint32_t *>(h_sel.data() + o_slots);
        for (uint64_t t = 0; t < na; t++) {
          if (h_n[t] != std::min<uint32_t>(seg[t + 1] - seg[t], max_out))
            return fail(TFIDF_E_STATE, "fuzzy expansion of term %llu has %u entries", (unsigned long long)t, h_n[t]);
          std::vector<FzsEntry> &L = (*ex)[t0 + a0 + t];
          L.reserve(h_n[t]);
          for (uint32_t i = 0; i < h_n[t]; i++) {
            const uint64_t k = h_k[t * kFzsMaxExpansions + i];
            const uint32_t slot = h_s[t * kFzsMaxExpansions + i];
            if (fzs_key_term(k) != t || slot >= S.C || fzs_key_dist(k) > max_edits)
              return fail(TFIDF_E_STATE, "fuzzy expansion entry %u of term %llu is out of place", i,
                          (unsigned long long)t);
            L.push_back(FzsEntry{slot, fzs_key_dist(k), fzs_key_boost_bits(k)});
          }
        }
        continue;
      }
      // what the host orders: everything (max_out == 0), or the selection packed into the sort's input buffers
      uint64_t n_take = T;
      oo = seg;
      const uint64_t *src_k = k_out;
      const uint32_t *src_s = s_out;
      if (max_out) {
        take.resize(na);
        HIP_TRY(hipMemcpyAsync(d_seg, seg.data(), (na + 1) * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_fz_select(k_out, d_seg, (uint32_t)na, max_out, d_take, s));
        HIP_TRY(hipMemcpyAsync(take.data(), d_take, na * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        n_take = 0;
        for (uint64_t t = 0; t < na; t++) {
          if (take[t] > seg[t + 1] - seg[t]) return fail(TFIDF_E_STATE, "fuzzy selection past its segment");
          oo[t] = (uint32_t)n_take;
          n_take += take[t];
        }
        oo[na] = (uint32_t)n_take;
        HIP_TRY(hipMemcpyAsync(d_oo, oo.data(), (na + 1) * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_fz_gather(k_out, s_out, d_seg, d_oo, (uint32_t)na, k_in, s_in, s));
        src_k = k_in;
        src_s = s_in;
      }
      h_keys.resize(n_take);
      h_slots.resize(n_take);
      HIP_TRY(hipMemcpyAsync(h_keys.data(), src_k, n_take * 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(h_slots.data(), src_s, n_take * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      for (uint64_t t = 0; t < na; t++) {
        std::vector<FuzzyCand> &L = out->cands[t0 + a0 + t];
        L.reserve(oo[t + 1] - oo[t]);
        for (uint32_t i = oo[t]; i < oo[t + 1]; i++) {
          if (fz_key_term(h_keys[i]) != t || h_slots[i] >= S.C)
            return fail(TFIDF_E_STATE, "fuzzy candidate %u of term %llu is out of place", i, (unsigned long long)t);
          if (int rc = slot_term(S, h_slots[i], &ts)) return rc;
          L.push_back(FuzzyCand{ts, fz_key_df(h_keys[i]), fz_key_dist(h_keys[i])});
        }
        std::sort(L.begin(), L.end(), [](const FuzzyCand &x, const FuzzyCand &y) {
          if (x.dist != y.dist) return x.dist < y.dist;
          if (x.df != y.df) return x.df > y.df;
          return x.term < y.term;
        });
        if (max_out && L.size() > max_out) L.resize(max_out);
      }
    }
  }
  HIP_TRY(hipEventRecord(X.ev[QEV_1], s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipEventElapsedTime(&out->ms_device, X.ev[QEV_0], X.ev[QEV_1]));
  publish();
  return TFIDF_OK;
}

static int fuzzy_check_args(const uint8_t *t_utf8, const uint64_t *t_offsets, uint32_t n_terms, uint32_t max_edits,
                            uint32_t max_out, bool all) {
  if (n_terms > kFzMaxTerms) return fail(TFIDF_E_INVALID_ARG, "more than %u terms in one call", kFzMaxTerms);
  if (max_edits > kFzMaxEdits) return fail(TFIDF_E_INVALID_ARG, "max_edits %u above %u", max_edits, kFzMaxEdits);
  if (!all && (max_out < 1 || max_out > kFzMaxOut))
    return fail(TFIDF_E_INVALID_ARG, "max_out %u outside 1..%u", max_out, kFzMaxOut);
  if (n_terms && (!t_offsets || (!t_utf8 && t_offsets[n_terms] != t_offsets[0])))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  for (uint32_t i = 0; i < n_terms; i++)
    if (t_offsets[i + 1] < t_offsets[i]) return fail(TFIDF_E_INVALID_ARG, "t_offsets decrease at term %u", i);
  return TFIDF_OK;
}

int tfidf::index_fuzzy_terms(tfidf_index *ix, const uint8_t *t_utf8, const uint64_t *t_offsets, uint32_t n_terms,
                             uint32_t max_edits, uint32_t prefix_len, uint32_t max_out, FuzzyLists *out) {
  if (!ix || !out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (int rc = fuzzy_check_args(t_utf8, t_offsets, n_terms, max_edits, max_out, max_out == 0)) return rc;
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "fuzzy lookup before commit");
  return fuzzy_on(ix, *snap, t_utf8, t_offsets, n_terms, max_edits, prefix_len, max_out, out);
}

// the CSR output of the fuzzy calls: offsets, n_within and the totals always, the payload when it fits
static int fuzzy_batch_on(tfidf_index *ix, Snapshot &S, const uint8_t *t_utf8, const uint64_t *t_offsets,
                          uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len, uint32_t max_out,
                          uint64_t *cand_offsets, uint64_t *n_within, uint64_t *term_offsets, uint8_t *terms,
                          uint64_t terms_cap, uint32_t *df, uint8_t *dist, uint64_t cand_cap, uint64_t *n_cands,
                          uint64_t *n_term_bytes, float *ms_device) {
  if (int rc = fuzzy_check_args(t_utf8, t_offsets, n_terms, max_edits, max_out, false)) return rc;
  if (!cand_offsets || (n_terms && !n_within) || !n_cands || !n_term_bytes)
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (ms_device) *ms_device = 0.0f;
  FuzzyLists fl;
  if (int rc = fuzzy_on(ix, S, t_utf8, t_offsets, n_terms, max_edits, prefix_len, max_out, &fl)) return rc;
  if (ms_device) *ms_device = fl.ms_device;
  uint64_t nc = 0, nb = 0;
  cand_offsets[0] = 0;
  for (uint32_t i = 0; i < n_terms; i++) {
    n_within[i] = fl.n_within[i];
    nc += fl.cands[i].size();
    for (const FuzzyCand &c : fl.cands[i]) nb += c.term.size();
    cand_offsets[i + 1] = nc;
  }
  *n_cands = nc;
  *n_term_bytes = nb;
  if (nc > cand_cap || nb > terms_cap || (nc && (!term_offsets || !df || !dist)) || (nb && !terms))
    return fail(TFIDF_E_BUFFER, "need %llu candidate slots and %llu term bytes", (unsigned long long)nc,
                (unsigned long long)nb);
  uint64_t at = 0, b = 0;
  if (term_offsets) term_offsets[0] = 0;
  for (uint32_t i = 0; i < n_terms; i++)
    for (const FuzzyCand &c : fl.cands[i]) {
      memcpy(terms + b, c.term.data(), c.term.size());
      b += c.term.size();
      df[at] = (uint32_t)c.df;
      dist[at] = (uint8_t)c.dist;
      term_offsets[++at] = b;
    }
  return TFIDF_OK;
}

extern "C" int tfidf_reader_fuzzy_terms_batch(tfidf_reader *rd, const uint8_t *t_utf8, const uint64_t *t_offsets,
                                              uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len,
                                              uint32_t max_out, uint64_t *cand_offsets, uint64_t *n_within,
                                              uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *df,
                                              uint8_t *dist, uint64_t cand_cap, uint64_t *n_cands,
                                              uint64_t *n_term_bytes, float *ms_device) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  return fuzzy_batch_on(rd->ix, *rd->S, t_utf8, t_offsets, n_terms, max_edits, prefix_len, max_out, cand_offsets,
                        n_within, term_offsets, terms, terms_cap, df, dist, cand_cap, n_cands, n_term_bytes, ms_device);
}

extern "C" int tfidf_fuzzy_terms_batch(tfidf_index *ix, const uint8_t *t_utf8, const uint64_t *t_offsets,
                                       uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len, uint32_t max_out,
                                       uint64_t *cand_offsets, uint64_t *n_within, uint64_t *term_offsets,
                                       uint8_t *terms, uint64_t terms_cap, uint32_t *df, uint8_t *dist,
                                       uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes,
                                       float *ms_device) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  if (int rc = fuzzy_check_args(t_utf8, t_offsets, n_terms, max_edits, max_out, false)) return rc;
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "fuzzy lookup before commit");
  return fuzzy_batch_on(ix, *snap, t_utf8, t_offsets, n_terms, max_edits, prefix_len, max_out, cand_offsets, n_within,
                        term_offsets, terms, terms_cap, df, dist, cand_cap, n_cands, n_term_bytes, ms_device);
}

// the batch of one, without the offsets arrays of the input and of the terms' candidates
extern "C" int tfidf_reader_fuzzy_terms(tfidf_reader *rd, const uint8_t *term, uint64_t len, uint32_t max_edits,
                                        uint32_t prefix_len, uint32_t max_out, uint64_t *n_within,
                                        uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *df,
                                        uint8_t *dist, uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes,
                                        float *ms_device) {
  if (!n_within || (!term && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t t_off[2] = {0, len};
  uint64_t c_off[2];
  return tfidf_reader_fuzzy_terms_batch(rd, term, t_off, 1, max_edits, prefix_len, max_out, c_off, n_within,
                                        term_offsets, terms, terms_cap, df, dist, cand_cap, n_cands, n_term_bytes,
                                        ms_device);
}

extern "C" int tfidf_fuzzy_terms(tfidf_index *ix, const uint8_t *term, uint64_t len, uint32_t max_edits,
                                 uint32_t prefix_len, uint32_t max_out, uint64_t *n_within, uint64_t *term_offsets,
                                 uint8_t *terms, uint64_t terms_cap, uint32_t *df, uint8_t *dist, uint64_t cand_cap,
                                 uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device) {
  if (!n_within || (!term && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t t_off[2] = {0, len};
  uint64_t c_off[2];
  return tfidf_fuzzy_terms_batch(ix, term, t_off, 1, max_edits, prefix_len, max_out, c_off, n_within, term_offsets,
                                 terms, terms_cap, df, dist, cand_cap, n_cands, n_term_bytes, ms_device);
}

extern "C" int tfidf_last_fuzzy_chunks(const tfidf_index *ix, uint64_t *scan_chunks, uint64_t *cand_chunks) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->ms_mu);
  if (scan_chunks) *scan_chunks = ix->last_fz_scan_chunks;
  if (cand_chunks) *cand_chunks = ix->last_fz_cand_chunks;
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// wildcard and prefix search (wildcard_plan.h, kernels_wildcard.hip).  Per scan
// chunk of patterns: one counting pass over the dictionary (n_matched and the
// scratch sizes), then per match chunk a filling pass and the (pattern, df)
// sort, which also groups the matched slots by pattern.  The terms route then
// selects what the host orders, exactly as the fuzzy lookup does; the document
// route unions the matched terms' postings per union chunk of patterns:
// bitmaps, counts per (pattern, block), one prefix sum, ascending doc ids.
// Every hit of the document route scores 1.0 (Lucene's constant-score rewrite
// of a multi-term query, boost 1), so no score is returned, and no clause
// limit applies: the matched terms never become scorer clauses.
// Regular-expression search (regex_plan.h, kernels_regex.hip) runs the same
// driver: only the scan step differs (DFA tables staged in a buffer of their
// own, chunked by their bytes, walked by k_rx_scan / k_rx_hashed).

constexpr uint64_t kWcMatchBudget = 1ull << 22;  // (pattern, term) matches per fill, as kFzCandBudget
constexpr uint64_t kWcHitBudget = 1ull << 27;    // bitmap bits per union chunk: 16 MiB of bitmaps, <= 512 MiB of doc ids
static_assert(kWcChunkPatterns <= kFzChunkTerms && kWcChunkElems <= kFzChunkCps, "the staging area of the fuzzy scan holds a pattern chunk");

// What a matcher brings to the shared driver: its name in messages, the knobs
// of its budgets, how its staged words are counted and chunked, where they are
// staged on the device, its two scan kernels and where its stats go.
struct MultiTermRoute {
  const char *what, *match_knob, *hit_knob;
  uint32_t unit_bytes;                      // n_el counts a pattern's staged words in this unit
  size_t stage_words;                       // words a scan chunk stages at most
  void (*plan)(const uint32_t *n_el, uint64_t n, std::vector<uint64_t> *cuts);
  DevMem SearchCtx::*stage;                 // a staging buffer of the route's own (nullptr: the fuzzy scan's element area)
  hipError_t (*scan)(bool fill, const FzScan &a, int max_grid, hipStream_t s);
  hipError_t (*scan_hashed)(bool fill, const FzScan &a, const uint8_t *text, uint64_t text_bytes, int max_grid,
                            hipStream_t s);
  void (*publish)(tfidf_index *ix, uint64_t scans, uint64_t matches, uint64_t unions, uint64_t staged_bytes);
};
static const MultiTermRoute kWildcardRoute = {
    "wildcard", "TFIDF_WILDCARD_MATCH_BUDGET", "TFIDF_WILDCARD_HIT_BUDGET", 4, kWcChunkElems,
    [](const uint32_t *n_el, uint64_t n, std::vector<uint64_t> *cuts) { wc_plan_scan_chunks(n_el, n, cuts); },
    nullptr, launch_wc_scan, launch_wc_hashed,
    [](tfidf_index *ix, uint64_t scans, uint64_t matches, uint64_t unions, uint64_t) {
      ix->last_wc_scan_chunks = scans;
      ix->last_wc_matches = matches;
      ix->last_wc_union_chunks = unions;
    }};
static const MultiTermRoute kRegexRoute = {
    "regex", "TFIDF_REGEX_MATCH_BUDGET", "TFIDF_REGEX_HIT_BUDGET", 1, kRxStageWords,
    [](const uint32_t *n_el, uint64_t n, std::vector<uint64_t> *cuts) {
      rx_plan_scan_chunks(n_el, n, hl_budget("TFIDF_REGEX_TABLE_BUDGET", kRxStageBytes), cuts);
    },
    &SearchCtx::rx_tab, launch_rx_scan, launch_rx_hashed,      // the fuzzy scan's element area is too small for tables
    [](tfidf_index *ix, uint64_t scans, uint64_t matches, uint64_t unions, uint64_t staged_bytes) {
      ix->last_rx_scan_chunks = scans;
      ix->last_rx_matches = matches;
      ix->last_rx_union_chunks = unions;
      ix->last_rx_table_bytes = staged_bytes;
    }};

// els[i]: what pattern i stages for its scan (empty: a pattern that matches
// nothing): wildcard elements or the words of a DFA table.
static int multiterm_on(tfidf_index *ix, Snapshot &S, const std::vector<std::vector<uint32_t>> &els, uint32_t n_p,
                        const MultiTermRoute &R, bool want_docs, uint32_t max_out, WildcardLists *out) {
  const char *const what = R.what;
  out->ms_device = 0.0f;
  out->terms.assign(want_docs ? 0 : n_p, {});
  out->n_matched.assign(n_p, 0);
  out->docs.clear();
  out->hit_off.assign((size_t)n_p + 1, 0);
  std::vector<uint32_t> n_el(n_p, 0);          // elements of a wildcard pattern, bytes of a regex table
  bool any = false;
  for (uint32_t i = 0; i < n_p; i++) {
    n_el[i] = (uint32_t)(els[i].size() * 4 / R.unit_bytes);
    any = any || n_el[i];
  }
  uint64_t n_scan = 0, n_match = 0, n_union = 0, n_tab_bytes = 0;
  auto publish = [&](float ms) {
    std::lock_guard<std::mutex> lk(ix->ms_mu);
    R.publish(ix, n_scan, n_match, n_union, n_tab_bytes);
    set_route_ms_locked(ix, 0.0f, ms);
  };
  if (!any || S.n_docs == 0 || S.C == 0) { publish(0.0f); return TFIDF_OK; }
  std::vector<uint64_t> cuts;
  R.plan(n_el.data(), n_p, &cuts);
  const uint64_t budget = std::min<uint64_t>(hl_budget(R.match_knob, kWcMatchBudget), 1ull << 30);
  const uint64_t hit_budget = hl_budget(R.hit_knob, kWcHitBudget);
  const size_t stage_words = R.stage_words;
  const uint32_t nb = (uint32_t)((S.n_docs + kBlockDocs - 1) / kBlockDocs);
  if (!S.term_major && nb != S.n_blocks) return fail(TFIDF_E_STATE, "block count of the snapshot is off");

  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();
  DeviceGuard g(ix->cfg.device);
  const int max_grid = ix->num_cus * 8;
  HIP_TRY(hipEventRecord(X.ev[QEV_0], s));

  // the staging area of the fuzzy scan (fuzzy_on): offsets, elements, counts, seg, out_off, take, cursor, hashed count
  const size_t in_cps = (kFzChunkTerms + 1) * 4, in_cnt = in_cps + kFzChunkCps * 4, in_seg = in_cnt + kFzChunkTerms * 4,
               in_oo = in_seg + (kFzChunkTerms + 1) * 4, in_take = in_oo + (kFzChunkTerms + 1) * 4,
               in_cur = in_take + kFzChunkTerms * 4, in_end = in_cur + 8;
  HIP_TRY(X.fz_in.reserve(in_end));
  uint8_t *ib = X.fz_in.as<uint8_t>();
  uint32_t *d_off = reinterpret_cast<uint32_t *>(ib), *d_cps = reinterpret_cast<uint32_t *>(ib + in_cps),
           *d_cnt = reinterpret_cast<uint32_t *>(ib + in_cnt), *d_seg = reinterpret_cast<uint32_t *>(ib + in_seg),
           *d_oo = reinterpret_cast<uint32_t *>(ib + in_oo), *d_take = reinterpret_cast<uint32_t *>(ib + in_take),
           *d_cur = reinterpret_cast<uint32_t *>(ib + in_cur), *d_hsn = d_cur + 1;
  if (R.stage) {
    HIP_TRY((X.*R.stage).reserve(R.stage_words * 4));
    d_cps = (X.*R.stage).as<uint32_t>();
  }

  FzScan a{};
  a.dict = S.dict.as<uint64_t>();
  a.df = S.df_dev();
  a.C = S.C;
  a.t_off = d_off;
  a.t_cps = d_cps;
  a.counts = d_cnt;
  a.cursor = d_cur;
  const uint8_t *d_text = S.text->as<uint8_t>();
  // the scan step of the two matchers
  auto scan = [&](bool fill, const FzScan &f) {
    return R.scan(fill, f, max_grid, s);
  };
  auto scan_hashed = [&](bool fill, const FzScan &f) {
    return R.scan_hashed(fill, f, d_text, S.text_bytes, max_grid, s);
  };
  bool listed = false;                     // the hashed slots are listed by the first counting scan
  uint32_t hs_n = 0;

  WcUnion u{};
  u.C = S.C;
  u.n_blocks = nb;
  u.NC = S.NC;
  u.n_docs = S.n_docs;
  u.post_words = S.nnz;
  if (S.term_major) {
    u.toff = S.toff.as<uint64_t>();
    u.post = S.post.as<uint64_t>();
  } else {
    u.crank = S.crank.as<uint2>();
    u.blk = S.blk.as<uint32_t>();
    u.bbase = S.bbase.as<uint64_t>();
    u.post32 = S.post.as<uint32_t>();
  }

  FzStage st;
  std::vector<uint32_t> counts, seg, take, oo, h_slots;
  std::vector<uint64_t> sub, usub, h_keys, h_cnt;
  std::string ts;
  for (size_t ci = 0; ci + 1 < cuts.size(); ci++) {
    const uint64_t t0 = cuts[ci], nt = cuts[ci + 1] - t0;
    fz_stage_terms(els, t0, t0 + nt, &st);
    if (st.cps.empty()) continue;                                   // only patterns that match nothing
    if (nt > kWcChunkPatterns || st.cps.size() > stage_words)
      return fail(TFIDF_E_STATE, "%s scan chunk over its limits", what);
    n_scan++;
    n_tab_bytes += st.cps.size() * 4;
    HIP_TRY(hipMemcpyAsync(d_off, st.off.data(), (nt + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_cps, st.cps.data(), st.cps.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, nt * 4, s));
    a.n_terms = (uint32_t)nt;
    a.t_off = d_off;
    a.keys = nullptr;
    a.slots = nullptr;
    a.cap = 0;
    a.hs_list = nullptr;
    a.hs_cap = 0;
    if (!listed) {
      HIP_TRY(X.fz_hs.reserve((size_t)kFzHashedInit * 4));
      HIP_TRY(hipMemsetAsync(d_hsn, 0, 4, s));
      a.hs_list = X.fz_hs.as<uint32_t>();
      a.hs_count = d_hsn;
      a.hs_cap = (uint32_t)(X.fz_hs.bytes / 4);
    }
    HIP_TRY(scan(false, a));
    if (!listed) {
      HIP_TRY(hipMemcpyAsync(&hs_n, d_hsn, 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      if (hs_n > a.hs_cap) {                                        // more hashed slots than the list held: list them again
        HIP_TRY(X.fz_hs.reserve((size_t)hs_n * 4));
        HIP_TRY(hipMemsetAsync(d_hsn, 0, 4, s));
        FzScan l = a;
        l.n_terms = 0;
        l.hs_list = X.fz_hs.as<uint32_t>();
        l.hs_cap = hs_n;
        HIP_TRY(scan(false, l));
      }
      listed = true;
    }
    a.hs_list = X.fz_hs.as<uint32_t>();
    a.hs_count = nullptr;
    a.hs_n = hs_n;
    HIP_TRY(scan_hashed(false, a));
    counts.resize(nt);
    HIP_TRY(hipMemcpyAsync(counts.data(), d_cnt, nt * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint64_t t = 0; t < nt; t++) {
      out->n_matched[t0 + t] = counts[t];
      n_match += counts[t];
    }

    sub.clear();
    wc_plan_match_chunks(counts.data(), 0, nt, budget, &sub);
    for (size_t si = 0; si + 1 < sub.size(); si++) {
      const uint64_t a0 = sub[si], na = sub[si + 1] - a0;
      seg.assign(na + 1, 0);
      uint64_t T = 0;
      for (uint64_t t = 0; t < na; t++) {
        T += counts[a0 + t];
        if (T >= (1ull << 31)) return fail(TFIDF_E_INVALID_ARG, "more than 2^31 matches for one pattern range");
        seg[t + 1] = (uint32_t)T;
      }
      if (T == 0) continue;
      // matches: keys [T] x 2 (sort in / out), slots [T] x 2
      const size_t Tp = (T + 1) & ~(size_t)1;
      HIP_TRY(X.fz_c.reserve(Tp * 24));
      uint64_t *k_in = X.fz_c.as<uint64_t>(), *k_out = k_in + Tp;
      uint32_t *s_in = reinterpret_cast<uint32_t *>(k_out + Tp), *s_out = s_in + Tp;
      HIP_TRY(hipMemsetAsync(d_cur, 0, 4, s));
      HIP_TRY(hipMemsetAsync(s_in, 0xFF, T * 4, s));                 // a slot the fill does not write is out of range
      FzScan f = a;
      f.t_off = d_off + a0;                 // the range's patterns: offsets into the chunk's elements
      f.n_terms = (uint32_t)na;
      f.keys = k_in;
      f.slots = s_in;
      f.cap = (uint32_t)T;
      HIP_TRY(scan(true, f));
      HIP_TRY(scan_hashed(true, f));
      size_t tmp_bytes = 0;
      HIP_TRY(fz_sort(nullptr, &tmp_bytes, k_in, k_out, s_in, s_out, (uint32_t)T, s));
      HIP_TRY(X.fz_tmp.reserve(tmp_bytes));
      tmp_bytes = X.fz_tmp.bytes;
      HIP_TRY(fz_sort(X.fz_tmp.p, &tmp_bytes, k_in, k_out, s_in, s_out, (uint32_t)T, s));
      HIP_TRY(hipMemcpyAsync(d_seg, seg.data(), (na + 1) * 4, hipMemcpyHostToDevice, s));

      if (want_docs) {
        usub.clear();
        wc_plan_union_chunks(0, na, (uint64_t)nb * kBlockDocs, hit_budget, &usub);
        for (size_t ui = 0; ui + 1 < usub.size(); ui++) {
          const uint64_t u0 = usub[ui], np = usub[ui + 1] - u0;
          const uint32_t M = seg[u0 + np] - seg[u0];
          if (M == 0) continue;                                     // no pattern of the chunk has a term
          n_union++;
          const uint64_t n_pb = np * nb;
          HIP_TRY(X.wc_bits.reserve(n_pb * (kBlockDocs / 8)));
          HIP_TRY(X.wc_cnt.reserve((n_pb + 1) * 8));
          u.slots = s_out;
          u.seg = d_seg + u0;
          u.n_pat = (uint32_t)np;
          u.bits = X.wc_bits.as<uint32_t>();
          u.cnt = X.wc_cnt.as<uint64_t>();
          u.out = nullptr;
          u.out_cap = 0;
          if (S.term_major) {
            HIP_TRY(hipMemsetAsync(u.bits, 0, n_pb * (kBlockDocs / 8), s));
            HIP_TRY(X.wc_len.reserve(((size_t)M + 1) * 8));
            u.row_off = X.wc_len.as<uint64_t>();
            HIP_TRY(launch_wc_rows(u, M, s));
            HIP_TRY(exclusive_scan_u64(u.row_off, u.row_off, M, s));
            HIP_TRY(launch_wc_union_term(u, M, S.nnz, max_grid, s));
          } else {
            HIP_TRY(launch_wc_union_block(u, s));
          }
          HIP_TRY(launch_wc_count(u, s));
          HIP_TRY(exclusive_scan_u64(u.cnt, u.cnt, n_pb, s));
          h_cnt.resize(n_pb + 1);
          HIP_TRY(hipMemcpyAsync(h_cnt.data(), u.cnt, (n_pb + 1) * 8, hipMemcpyDeviceToHost, s));
          HIP_TRY(hipStreamSynchronize(s));
          const uint64_t H = h_cnt[n_pb];
          if (H > np * S.n_docs) return fail(TFIDF_E_STATE, "%s union counted more hits than documents", what);
          for (uint64_t t = 0; t < np; t++)
            out->hit_off[t0 + a0 + u0 + t + 1] = h_cnt[(t + 1) * nb] - h_cnt[t * nb];
          if (H == 0) continue;
          HIP_TRY(X.wc_out.reserve(H * 4));
          u.out = X.wc_out.as<uint32_t>();
          u.out_cap = H;
          HIP_TRY(launch_wc_expand(u, s));
          const size_t at = out->docs.size();
          out->docs.resize(at + H);
          HIP_TRY(hipMemcpyAsync(out->docs.data() + at, u.out, H * 4, hipMemcpyDeviceToHost, s));
          HIP_TRY(hipStreamSynchronize(s));
        }
        continue;
      }

      // what the host orders: everything (max_out == 0), or the selection packed into the sort's input buffers
      uint64_t n_take = T;
      oo = seg;
      const uint64_t *src_k = k_out;
      const uint32_t *src_s = s_out;
      if (max_out) {
        take.resize(na);
        HIP_TRY(launch_fz_select(k_out, d_seg, (uint32_t)na, max_out, d_take, s));
        HIP_TRY(hipMemcpyAsync(take.data(), d_take, na * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        n_take = 0;
        for (uint64_t t = 0; t < na; t++) {
          if (take[t] > seg[t + 1] - seg[t]) return fail(TFIDF_E_STATE, "%s selection past its segment", what);
          oo[t] = (uint32_t)n_take;
          n_take += take[t];
        }
        oo[na] = (uint32_t)n_take;
        HIP_TRY(hipMemcpyAsync(d_oo, oo.data(), (na + 1) * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_fz_gather(k_out, s_out, d_seg, d_oo, (uint32_t)na, k_in, s_in, s));
        src_k = k_in;
        src_s = s_in;
      }
      h_keys.resize(n_take);
      h_slots.resize(n_take);
      HIP_TRY(hipMemcpyAsync(h_keys.data(), src_k, n_take * 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(h_slots.data(), src_s, n_take * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      for (uint64_t t = 0; t < na; t++) {
        std::vector<FuzzyCand> &L = out->terms[t0 + a0 + t];
        L.reserve(oo[t + 1] - oo[t]);
        for (uint32_t i = oo[t]; i < oo[t + 1]; i++) {
          if (fz_key_term(h_keys[i]) != t || h_slots[i] >= S.C)
            return fail(TFIDF_E_STATE, "%s match %u of pattern %llu is out of place", what, i, (unsigned long long)t);
          if (int rc = slot_term(S, h_slots[i], &ts)) return rc;
          L.push_back(FuzzyCand{ts, fz_key_df(h_keys[i]), 0});
        }
        std::sort(L.begin(), L.end(), [](const FuzzyCand &x, const FuzzyCand &y) {
          if (x.df != y.df) return x.df > y.df;
          return x.term < y.term;
        });
        if (max_out && L.size() > max_out) L.resize(max_out);
      }
    }
  }
  for (uint32_t i = 0; i < n_p; i++) out->hit_off[i + 1] += out->hit_off[i];
  if (want_docs && out->hit_off[n_p] != out->docs.size()) return fail(TFIDF_E_STATE, "%s hit lists are out of step", what);
  HIP_TRY(hipEventRecord(X.ev[QEV_1], s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipEventElapsedTime(&out->ms_device, X.ev[QEV_0], X.ev[QEV_1]));
  publish(out->ms_device);
  return TFIDF_OK;
}

// the wildcard route's parse step
static int wildcard_on(tfidf_index *ix, Snapshot &S, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                       bool want_docs, uint32_t max_out, WildcardLists *out) {
  std::vector<std::vector<uint32_t>> els(n_p);
  uint32_t buf[kWcMaxElems];
  for (uint32_t i = 0; i < n_p; i++) {
    const uint64_t len = p_offsets[i + 1] - p_offsets[i];
    if (len == 0) continue;
    const uint32_t n = wc_parse(p_utf8 + p_offsets[i], len, buf);
    els[i].assign(buf, buf + n);
  }
  return multiterm_on(ix, S, els, n_p, kWildcardRoute, want_docs, max_out, out);
}

static int multiterm_check_args(const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p) {
  if (n_p > kWcMaxPatterns) return fail(TFIDF_E_INVALID_ARG, "more than %u patterns in one call", kWcMaxPatterns);
  if (n_p && (!p_offsets || (!p_utf8 && p_offsets[n_p] != p_offsets[0])))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  for (uint32_t i = 0; i < n_p; i++)
    if (p_offsets[i + 1] < p_offsets[i]) return fail(TFIDF_E_INVALID_ARG, "p_offsets decrease at pattern %u", i);
  return TFIDF_OK;
}

int tfidf::index_wildcard(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p, bool docs,
                          uint32_t max_out, WildcardLists *out) {
  if (!ix || !out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (int rc = multiterm_check_args(p_utf8, p_offsets, n_p)) return rc;
  if (max_out > kWcMaxOut) return fail(TFIDF_E_INVALID_ARG, "max_out %u above %u", max_out, kWcMaxOut);
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "wildcard search before commit");
  return wildcard_on(ix, *snap, p_utf8, p_offsets, n_p, docs, max_out, out);
}

// the regex route's parse step: every pattern to its DFA table (empty: a pattern
// that matches nothing).  The first pattern in error fails the call.
int tfidf::regex_compile_all(const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                             std::vector<std::vector<uint32_t>> *tabs) {
  tabs->assign(n_p, {});
  for (uint32_t i = 0; i < n_p; i++) {
    uint64_t err_at = 0;
    const uint64_t len = p_offsets[i + 1] - p_offsets[i];
    const int rc = rx_compile(len ? p_utf8 + p_offsets[i] : nullptr, len, &(*tabs)[i], &err_at);
    if (rc == kRxSyntax)
      return fail(TFIDF_E_QUERY_SYNTAX, "regex pattern %u: syntax error at byte %llu", i, (unsigned long long)err_at);
    if (rc == kRxUnsupported)
      return fail(TFIDF_E_UNSUPPORTED_QUERY,
                  "regex pattern %u: unsupported at byte %llu ('<', or an automaton over the limits of regex_plan.h)", i,
                  (unsigned long long)err_at);
    if (rx_table_matches_nothing((*tabs)[i])) (*tabs)[i].clear();
  }
  return TFIDF_OK;
}

int tfidf::index_regex(tfidf_index *ix, const std::vector<std::vector<uint32_t>> &tabs, bool docs, uint32_t max_out,
                       WildcardLists *out) {
  if (!ix || !out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (tabs.size() > kWcMaxPatterns) return fail(TFIDF_E_INVALID_ARG, "more than %u patterns in one call", kWcMaxPatterns);
  if (max_out > kWcMaxOut) return fail(TFIDF_E_INVALID_ARG, "max_out %u above %u", max_out, kWcMaxOut);
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "regex search before commit");
  return multiterm_on(ix, *snap, tabs, (uint32_t)tabs.size(), kRegexRoute, docs, max_out, out);
}

// the CSR output of the term calls: offsets, n_matched and the totals always, the payload when it fits
// (regex: a pattern in error fails the call before anything is written)
static int multiterm_terms_on(tfidf_index *ix, Snapshot &S, bool regex, const uint8_t *p_utf8, const uint64_t *p_offsets,
                             uint32_t n_p, uint32_t max_out, uint64_t *cand_offsets, uint64_t *n_matched,
                             uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *df,
                             uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device) {
  if (int rc = multiterm_check_args(p_utf8, p_offsets, n_p)) return rc;
  if (max_out < 1 || max_out > kWcMaxOut) return fail(TFIDF_E_INVALID_ARG, "max_out %u outside 1..%u", max_out, kWcMaxOut);
  if (!cand_offsets || (n_p && !n_matched) || !n_cands || !n_term_bytes) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::vector<std::vector<uint32_t>> tabs;
  if (regex)
    if (int rc = regex_compile_all(p_utf8, p_offsets, n_p, &tabs)) return rc;
  if (ms_device) *ms_device = 0.0f;
  WildcardLists wl;
  if (int rc = regex ? multiterm_on(ix, S, tabs, n_p, kRegexRoute, false, max_out, &wl)
                     : wildcard_on(ix, S, p_utf8, p_offsets, n_p, false, max_out, &wl))
    return rc;
  if (ms_device) *ms_device = wl.ms_device;
  uint64_t nc = 0, nbytes = 0;
  cand_offsets[0] = 0;
  for (uint32_t i = 0; i < n_p; i++) {
    n_matched[i] = wl.n_matched[i];
    nc += wl.terms[i].size();
    for (const FuzzyCand &c : wl.terms[i]) nbytes += c.term.size();
    cand_offsets[i + 1] = nc;
  }
  *n_cands = nc;
  *n_term_bytes = nbytes;
  if (nc > cand_cap || nbytes > terms_cap || (nc && (!term_offsets || !df)) || (nbytes && !terms))
    return fail(TFIDF_E_BUFFER, "need %llu term slots and %llu term bytes", (unsigned long long)nc,
                (unsigned long long)nbytes);
  uint64_t at = 0, b = 0;
  if (term_offsets) term_offsets[0] = 0;
  for (uint32_t i = 0; i < n_p; i++)
    for (const FuzzyCand &c : wl.terms[i]) {
      memcpy(terms + b, c.term.data(), c.term.size());
      b += c.term.size();
      df[at] = (uint32_t)c.df;
      term_offsets[++at] = b;
    }
  return TFIDF_OK;
}

// the output of the document calls: hit_offsets, n_matched and *n_out always, the doc ids when they fit
static int multiterm_docs_on(tfidf_index *ix, Snapshot &S, bool regex, const uint8_t *p_utf8, const uint64_t *p_offsets,
                            uint32_t n_p, uint32_t *doc_ids, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_matched,
                            uint64_t *n_out, float *ms_device) {
  if (int rc = multiterm_check_args(p_utf8, p_offsets, n_p)) return rc;
  if (!hit_offsets || (n_p && !n_matched) || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::vector<std::vector<uint32_t>> tabs;
  if (regex)
    if (int rc = regex_compile_all(p_utf8, p_offsets, n_p, &tabs)) return rc;
  if (ms_device) *ms_device = 0.0f;
  WildcardLists wl;
  if (int rc = regex ? multiterm_on(ix, S, tabs, n_p, kRegexRoute, true, 0, &wl)
                     : wildcard_on(ix, S, p_utf8, p_offsets, n_p, true, 0, &wl))
    return rc;
  if (ms_device) *ms_device = wl.ms_device;
  for (uint32_t i = 0; i < n_p; i++) n_matched[i] = wl.n_matched[i];
  memcpy(hit_offsets, wl.hit_off.data(), ((size_t)n_p + 1) * 8);
  *n_out = wl.docs.size();
  if (wl.docs.size() > cap || (!wl.docs.empty() && !doc_ids))
    return fail(TFIDF_E_BUFFER, "need %llu hit slots", (unsigned long long)wl.docs.size());
  if (!wl.docs.empty()) memcpy(doc_ids, wl.docs.data(), wl.docs.size() * 4);
  return TFIDF_OK;
}

extern "C" int tfidf_reader_wildcard_terms_batch(tfidf_reader *rd, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                                 uint32_t n_p, uint32_t max_out, uint64_t *cand_offsets,
                                                 uint64_t *n_matched, uint64_t *term_offsets, uint8_t *terms,
                                                 uint64_t terms_cap, uint32_t *df, uint64_t cand_cap,
                                                 uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  return multiterm_terms_on(rd->ix, *rd->S, false, p_utf8, p_offsets, n_p, max_out, cand_offsets, n_matched, term_offsets,
                           terms, terms_cap, df, cand_cap, n_cands, n_term_bytes, ms_device);
}

extern "C" int tfidf_wildcard_terms_batch(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                          uint32_t n_p, uint32_t max_out, uint64_t *cand_offsets, uint64_t *n_matched,
                                          uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *df,
                                          uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes,
                                          float *ms_device) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  if (int rc = multiterm_check_args(p_utf8, p_offsets, n_p)) return rc;
  if (max_out < 1 || max_out > kWcMaxOut) return fail(TFIDF_E_INVALID_ARG, "max_out %u outside 1..%u", max_out, kWcMaxOut);
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "wildcard lookup before commit");
  return multiterm_terms_on(ix, *snap, false, p_utf8, p_offsets, n_p, max_out, cand_offsets, n_matched, term_offsets, terms,
                           terms_cap, df, cand_cap, n_cands, n_term_bytes, ms_device);
}

extern "C" int tfidf_reader_search_wildcard_batch(tfidf_reader *rd, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                                  uint32_t n_p, uint32_t *doc_ids, uint64_t cap, uint64_t *hit_offsets,
                                                  uint64_t *n_matched, uint64_t *n_out, float *ms_device) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  return multiterm_docs_on(rd->ix, *rd->S, false, p_utf8, p_offsets, n_p, doc_ids, cap, hit_offsets, n_matched, n_out,
                          ms_device);
}

extern "C" int tfidf_search_wildcard_batch(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                           uint32_t n_p, uint32_t *doc_ids, uint64_t cap, uint64_t *hit_offsets,
                                           uint64_t *n_matched, uint64_t *n_out, float *ms_device) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  if (int rc = multiterm_check_args(p_utf8, p_offsets, n_p)) return rc;
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "wildcard search before commit");
  return multiterm_docs_on(ix, *snap, false, p_utf8, p_offsets, n_p, doc_ids, cap, hit_offsets, n_matched, n_out, ms_device);
}

// the batch of one, without the offsets arrays of the input and of the patterns' lists
extern "C" int tfidf_reader_wildcard_terms(tfidf_reader *rd, const uint8_t *pattern, uint64_t len, uint32_t max_out,
                                           uint64_t *n_matched, uint64_t *term_offsets, uint8_t *terms,
                                           uint64_t terms_cap, uint32_t *df, uint64_t cand_cap, uint64_t *n_cands,
                                           uint64_t *n_term_bytes, float *ms_device) {
  if (!n_matched || (!pattern && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t p_off[2] = {0, len};
  uint64_t c_off[2];
  return tfidf_reader_wildcard_terms_batch(rd, pattern, p_off, 1, max_out, c_off, n_matched, term_offsets, terms,
                                           terms_cap, df, cand_cap, n_cands, n_term_bytes, ms_device);
}

extern "C" int tfidf_wildcard_terms(tfidf_index *ix, const uint8_t *pattern, uint64_t len, uint32_t max_out,
                                    uint64_t *n_matched, uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap,
                                    uint32_t *df, uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes,
                                    float *ms_device) {
  if (!n_matched || (!pattern && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t p_off[2] = {0, len};
  uint64_t c_off[2];
  return tfidf_wildcard_terms_batch(ix, pattern, p_off, 1, max_out, c_off, n_matched, term_offsets, terms, terms_cap,
                                    df, cand_cap, n_cands, n_term_bytes, ms_device);
}

extern "C" int tfidf_reader_search_wildcard(tfidf_reader *rd, const uint8_t *pattern, uint64_t len, uint32_t *doc_ids,
                                            uint64_t cap, uint64_t *n_matched, uint64_t *n_out, float *ms_device) {
  if (!n_matched || (!pattern && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t p_off[2] = {0, len};
  uint64_t h_off[2];
  return tfidf_reader_search_wildcard_batch(rd, pattern, p_off, 1, doc_ids, cap, h_off, n_matched, n_out, ms_device);
}

extern "C" int tfidf_search_wildcard(tfidf_index *ix, const uint8_t *pattern, uint64_t len, uint32_t *doc_ids,
                                     uint64_t cap, uint64_t *n_matched, uint64_t *n_out, float *ms_device) {
  if (!n_matched || (!pattern && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t p_off[2] = {0, len};
  uint64_t h_off[2];
  return tfidf_search_wildcard_batch(ix, pattern, p_off, 1, doc_ids, cap, h_off, n_matched, n_out, ms_device);
}

extern "C" int tfidf_last_wildcard_stats(const tfidf_index *ix, uint64_t *scan_chunks, uint64_t *matches,
                                         uint64_t *union_chunks) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->ms_mu);
  if (scan_chunks) *scan_chunks = ix->last_wc_scan_chunks;
  if (matches) *matches = ix->last_wc_matches;
  if (union_chunks) *union_chunks = ix->last_wc_union_chunks;
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// regular-expression search: the wildcard calls' twins on the regex route

extern "C" int tfidf_reader_regex_terms_batch(tfidf_reader *rd, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                                 uint32_t n_p, uint32_t max_out, uint64_t *cand_offsets,
                                                 uint64_t *n_matched, uint64_t *term_offsets, uint8_t *terms,
                                                 uint64_t terms_cap, uint32_t *df, uint64_t cand_cap,
                                                 uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  return multiterm_terms_on(rd->ix, *rd->S, true, p_utf8, p_offsets, n_p, max_out, cand_offsets, n_matched, term_offsets,
                           terms, terms_cap, df, cand_cap, n_cands, n_term_bytes, ms_device);
}

extern "C" int tfidf_regex_terms_batch(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                          uint32_t n_p, uint32_t max_out, uint64_t *cand_offsets, uint64_t *n_matched,
                                          uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *df,
                                          uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes,
                                          float *ms_device) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  if (int rc = multiterm_check_args(p_utf8, p_offsets, n_p)) return rc;
  if (max_out < 1 || max_out > kWcMaxOut) return fail(TFIDF_E_INVALID_ARG, "max_out %u outside 1..%u", max_out, kWcMaxOut);
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "regex lookup before commit");
  return multiterm_terms_on(ix, *snap, true, p_utf8, p_offsets, n_p, max_out, cand_offsets, n_matched, term_offsets, terms,
                           terms_cap, df, cand_cap, n_cands, n_term_bytes, ms_device);
}

extern "C" int tfidf_reader_search_regex_batch(tfidf_reader *rd, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                                  uint32_t n_p, uint32_t *doc_ids, uint64_t cap, uint64_t *hit_offsets,
                                                  uint64_t *n_matched, uint64_t *n_out, float *ms_device) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  return multiterm_docs_on(rd->ix, *rd->S, true, p_utf8, p_offsets, n_p, doc_ids, cap, hit_offsets, n_matched, n_out,
                          ms_device);
}

extern "C" int tfidf_search_regex_batch(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                           uint32_t n_p, uint32_t *doc_ids, uint64_t cap, uint64_t *hit_offsets,
                                           uint64_t *n_matched, uint64_t *n_out, float *ms_device) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  if (int rc = multiterm_check_args(p_utf8, p_offsets, n_p)) return rc;
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "regex search before commit");
  return multiterm_docs_on(ix, *snap, true, p_utf8, p_offsets, n_p, doc_ids, cap, hit_offsets, n_matched, n_out, ms_device);
}

// the batch of one, without the offsets arrays of the input and of the patterns' lists
extern "C" int tfidf_reader_regex_terms(tfidf_reader *rd, const uint8_t *pattern, uint64_t len, uint32_t max_out,
                                           uint64_t *n_matched, uint64_t *term_offsets, uint8_t *terms,
                                           uint64_t terms_cap, uint32_t *df, uint64_t cand_cap, uint64_t *n_cands,
                                           uint64_t *n_term_bytes, float *ms_device) {
  if (!n_matched || (!pattern && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t p_off[2] = {0, len};
  uint64_t c_off[2];
  return tfidf_reader_regex_terms_batch(rd, pattern, p_off, 1, max_out, c_off, n_matched, term_offsets, terms,
                                           terms_cap, df, cand_cap, n_cands, n_term_bytes, ms_device);
}

extern "C" int tfidf_regex_terms(tfidf_index *ix, const uint8_t *pattern, uint64_t len, uint32_t max_out,
                                    uint64_t *n_matched, uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap,
                                    uint32_t *df, uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes,
                                    float *ms_device) {
  if (!n_matched || (!pattern && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t p_off[2] = {0, len};
  uint64_t c_off[2];
  return tfidf_regex_terms_batch(ix, pattern, p_off, 1, max_out, c_off, n_matched, term_offsets, terms, terms_cap,
                                    df, cand_cap, n_cands, n_term_bytes, ms_device);
}

extern "C" int tfidf_reader_search_regex(tfidf_reader *rd, const uint8_t *pattern, uint64_t len, uint32_t *doc_ids,
                                            uint64_t cap, uint64_t *n_matched, uint64_t *n_out, float *ms_device) {
  if (!n_matched || (!pattern && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t p_off[2] = {0, len};
  uint64_t h_off[2];
  return tfidf_reader_search_regex_batch(rd, pattern, p_off, 1, doc_ids, cap, h_off, n_matched, n_out, ms_device);
}

extern "C" int tfidf_search_regex(tfidf_index *ix, const uint8_t *pattern, uint64_t len, uint32_t *doc_ids,
                                     uint64_t cap, uint64_t *n_matched, uint64_t *n_out, float *ms_device) {
  if (!n_matched || (!pattern && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t p_off[2] = {0, len};
  uint64_t h_off[2];
  return tfidf_search_regex_batch(ix, pattern, p_off, 1, doc_ids, cap, h_off, n_matched, n_out, ms_device);
}

extern "C" int tfidf_last_regex_stats(const tfidf_index *ix, uint64_t *scan_chunks, uint64_t *matches,
                                      uint64_t *union_chunks, uint64_t *table_bytes) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->ms_mu);
  if (scan_chunks) *scan_chunks = ix->last_rx_scan_chunks;
  if (matches) *matches = ix->last_rx_matches;
  if (union_chunks) *union_chunks = ix->last_rx_union_chunks;
  if (table_bytes) *table_bytes = ix->last_rx_table_bytes;
  return TFIDF_OK;
}

extern "C" int tfidf_query_positive_terms(const uint8_t *q, uint64_t q_len, char *out, uint64_t cap, uint64_t *n_terms,
                                          uint64_t *n_bytes) {
  if ((!q && q_len) || !n_terms || !n_bytes || (!out && cap)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::vector<std::string> terms;
  const int prc = positive_terms(q, q_len, &terms);
  if (prc == kQBadUtf8) return fail(TFIDF_E_UNSUPPORTED_QUERY, "query is not valid UTF-8");
  if (prc == kQSyntax)
    return fail(TFIDF_E_QUERY_SYNTAX, "query does not parse (QueryParser ParseException / TooManyClauses)");
  uint64_t need = 0;
  for (auto &t : terms) need += t.size() + 1;
  *n_terms = terms.size();
  *n_bytes = need;
  if (need > cap) return fail(TFIDF_E_BUFFER, "buffer too small");
  uint64_t p = 0;
  for (auto &t : terms) {
    memcpy(out + p, t.data(), t.size());
    out[p + t.size()] = 0;
    p += t.size() + 1;
  }
  return TFIDF_OK;
}

extern "C" int tfidf_search_batch(tfidf_index *ix, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                  uint32_t k, uint32_t *doc_ids, float *scores, uint32_t *counts) {
  if (!ix || !q_offsets || !doc_ids || !scores || !counts) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (k == 0 || k > 1024) return fail(TFIDF_E_INVALID_ARG, "batch search needs 1 <= k <= 1024");
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "search before commit");
  Snapshot &S = *snap;
  StatsView &V = *view;
  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();
  DeviceGuard g(ix->cfg.device);
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  if (n_q == 0) return TFIDF_OK;
  if (S.n_docs == 0) {
    memset(counts, 0, (size_t)n_q * 4);
    return TFIDF_OK;
  }
  // Pipelined in chunks: chunk c + 1 is prepared on the host (parse, analysis,
  // dictionary lookups, weights) while chunk c scores on the device; each
  // chunk's results are copied (stream-ordered) into its region of one pinned
  // buffer.  Chunks are ceil-sized, so the first one is the largest and the
  // buffers sized by the query count (cand, cand_n, q_out) are reserved by it;
  // q_in (sized by each chunk's terms) grows with an explicit stream sync in
  // run_scoring.  TFIDF_BATCH_CHUNKS overrides.
  // 10 k queries at cfg 2 (tools/gpu_batch_ab.sh): 1 chunk 7.6 ms end to end
  // (prepare 1.5 on the pool, device 5.65), 2 chunks 7.0 (device 6.05), 4
  // chunks 7.45 (device 6.9: every chunk pays the unit kernels' tail)
  // Chunks interleave the queries (chunk c: queries c, c + n_chunks, ...), so
  // each holds the batch's mix of heavy (k_score_units) and light
  // (k_score_wunits) queries and its two concurrent kernels end together
  // (round 6; a contiguous split gave cfg 2's two chunks 3.0 / 1.4 ms and
  // 1.2 / 2.6 ms of heavy / light work: 5.6 ms device)
  uint32_t n_chunks = n_q >= 4096 ? 2 : 1;
  if (const char *e = knob("TFIDF_BATCH_CHUNKS")) n_chunks = (uint32_t)std::max(1, std::min(atoi(e), 64));
  n_chunks = std::max(1u, std::min(n_chunks, n_q));
  const size_t words = (size_t)2 * n_q * k + n_q;
  HIP_TRY(X.q_res.resize(words));
  double t_prep = 0, t_sub = 0;
  bool any = false;
  uint32_t c0 = 0;                                       // results of chunk c start at row c0
  std::vector<uint8_t> cq;                               // chunk c's queries, contiguous
  std::vector<uint64_t> co;
  for (uint32_t c = 0; c < n_chunks; c++) {
    const uint32_t nc = (n_q - c + n_chunks - 1) / n_chunks;   // the first chunk is the largest
    const auto ta = clk::now();
    const uint8_t *cu = q_utf8;
    const uint64_t *coffs = q_offsets;
    if (n_chunks > 1) {
      cq.clear();
      co.assign(1, 0);
      for (uint32_t i = 0; i < nc; i++) {
        const uint32_t q = c + i * n_chunks;
        cq.insert(cq.end(), q_utf8 + q_offsets[q], q_utf8 + q_offsets[q + 1]);
        co.push_back(cq.size());
      }
      cu = cq.data();
      coffs = co.data();
    }
    QueryBatch qb;
    if (int e = prepare_batch(ix, S, V, cu, coffs, nc, &qb)) { X.q_rec_start = true; return e; }
    const auto tb = clk::now();
    uint32_t *hres = X.q_res.data() + (size_t)2 * c0 * k + c0;
    if (qb.slot.empty()) {
      memset(hres + (size_t)2 * nc * k, 0, (size_t)nc * 4);   // no term of the chunk is present
    } else {
      X.q_rec_start = !any;
      const int rc = run_scoring(ix, S, V, X, s, qb, nc, k);
      X.q_rec_start = true;
      if (rc) return rc;
      HIP_TRY(hipMemcpyAsync(hres, X.res_doc, ((size_t)2 * nc * k + nc) * 4, hipMemcpyDeviceToHost, s));
      any = true;
    }
    t_prep += std::chrono::duration<double, std::milli>(tb - ta).count();
    t_sub += std::chrono::duration<double, std::milli>(clk::now() - tb).count();
    c0 += nc;
  }
  const auto t2 = clk::now();
  HIP_TRY(hipStreamSynchronize(s));
  X.q_in_pending = false;
  const auto t3 = clk::now();
  c0 = 0;
  for (uint32_t c = 0; c < n_chunks; c++) {
    const uint32_t nc = (n_q - c + n_chunks - 1) / n_chunks;
    const uint32_t *hres = X.q_res.data() + (size_t)2 * c0 * k + c0;
    for (uint32_t i = 0; i < nc; i++) {
      const uint32_t q = c + i * n_chunks;
      memcpy(doc_ids + (size_t)q * k, hres + (size_t)i * k, (size_t)k * 4);
      memcpy(scores + (size_t)q * k, hres + (size_t)nc * k + (size_t)i * k, (size_t)k * 4);
      counts[q] = hres[(size_t)2 * nc * k + i];
    }
    c0 += nc;
  }
  const float ms_total = any ? qev_ms(X, QEV_0, QEV_2) : 0.0f;
  set_route_ms(ix, any ? qev_ms(X, QEV_0, QEV_1) : 0.0f, ms_total);
  if (knob("TFIDF_HOST_TIMING")) {          // profiling only
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "batch %u (%u chunks): prepare %.3f  submit %.3f  wait %.3f  copy-out %.3f  total %.3f ms (device %.3f)\n",
            n_q, n_chunks, t_prep, t_sub, ms(t2, t3), ms(t3, clk::now()), ms(t0, clk::now()), ms_total);
  }
  return TFIDF_OK;
}

// Every hit of each query of a batch (tfidf_search_batch_all): the queries are
// prepared together, then scored and merged in chunks (launch_hits_order_batch)
// whose scratch stays under kAllHitsBudget however many queries the batch
// holds.  Per chunk: the gapped runs take R2 x 64 KiB per query (8 MiB at 1 M
// documents), the two compact merge buffers and the (doc, score) output 8 B
// each per possible hit (a query's hits are bounded by the sum of its scoring
// terms' df).  1 GiB: about 120 mid-frequency queries per chunk at 1 M
// documents, so the chunk's one upload, ~6 launches and two syncs are spread
// over two orders of magnitude more queries than the single search's, while
// sixteen concurrent callers' contexts together stay near 5 % of the 288 GB.
// A chunk always holds at least one query.  TFIDF_ALLHITS_CHUNK=<queries>
// fixes the chunk size (tests).
constexpr uint64_t kAllHitsBudget = 1ull << 30;

// chunk [a, *z) of a prepared batch's queries [a, end): queries while the
// chunk's scratch stays in the budget (fixed: TFIDF_ALLHITS_CHUNK); *bound =
// the chunk's hit bound
static void all_hits_chunk(const QueryBatch &qb, const Snapshot &S, uint32_t a, uint32_t end, uint32_t fixed,
                           uint32_t *z_out, uint64_t *bound_out) {
  const uint32_t R2 = hits_runs_per_query(S.n_blocks);
  const uint64_t gap_bytes = (uint64_t)R2 * kBlockDocs * 8;
  const uint32_t max_q = std::max(1u, (1u << 30) / R2);     // run indices stay in 32 bits
  uint32_t z = a;
  uint64_t bound = 0, bytes = 0;
  while (z < end && z - a < max_q) {
    uint64_t hb = 0;
    for (uint32_t t = qb.off[z]; t < qb.off[z + 1]; t++)
      if ((qb.role[t] >> 24) != kRoleNot) hb += qb.ldf[t];
    hb = std::min<uint64_t>(hb, S.n_docs);
    if (z > a && (fixed ? z - a >= fixed : bytes + gap_bytes + hb * 24 > kAllHitsBudget)) break;
    bound += hb;
    bytes += gap_bytes + hb * 24;
    z++;
  }
  *z_out = z;
  *bound_out = bound;
}

static uint32_t all_hits_fixed_chunk() {
  if (const char *e = knob("TFIDF_ALLHITS_CHUNK")) return (uint32_t)std::max(1, atoi(e));
  return 0;
}

// Scores chunk [a, z) of a prepared batch and orders its hits, query-major and
// contiguous: into X.out_doc / X.out_score, or as merge keys with doc_base into
// keys_out (room for `bound` keys).  qoff_h: the queries' offsets in the chunk
// (nc + 1, read back: the stream is idle on return); left empty when no term of
// the chunk is present.
static int all_hits_score_chunk(tfidf_index *ix, Snapshot &S, StatsView &V, SearchCtx &X, hipStream_t s,
                                const QueryBatch &qb, uint32_t a, uint32_t z, uint64_t bound, bool *any,
                                uint64_t *keys_out, uint64_t doc_base, std::vector<uint64_t> *qoff_h) {
  qoff_h->clear();
  const uint32_t nc = z - a, R = S.n_blocks, R2 = hits_runs_per_query(R);
  const uint32_t t0 = qb.off[a], t1 = qb.off[z];
  if (t1 == t0) return TFIDF_OK;
  QueryBatch sub;
  sub.off.resize(nc + 1);
  for (uint32_t i = 0; i <= nc; i++) sub.off[i] = qb.off[a + i] - t0;
  sub.slot.assign(qb.slot.begin() + t0, qb.slot.begin() + t1);
  sub.w.assign(qb.w.begin() + t0, qb.w.begin() + t1);
  sub.role.assign(qb.role.begin() + t0, qb.role.begin() + t1);
  sub.ldf.assign(qb.ldf.begin() + t0, qb.ldf.begin() + t1);
  sub.meta.assign(qb.meta.begin() + a, qb.meta.begin() + z);
  for (uint32_t m : sub.meta) sub.ops |= m != 0;
  X.q_rec_start = !*any;
  const int rc = run_scoring(ix, S, V, X, s, sub, nc, 0, R2);
  X.q_rec_start = true;
  if (rc) return rc;
  *any = true;
  const size_t runs = (size_t)nc * R2;
  HIP_TRY(X.hits_c.reserve(bound * 8 + 8));
  HIP_TRY(X.hits_s.reserve(bound * 8 + 8));
  HIP_TRY(X.hits_P.reserve((runs + 1 + nc + 1) * 8));
  if (!keys_out) {
    HIP_TRY(X.out_doc.reserve(bound * 4 + 4));
    HIP_TRY(X.out_score.reserve(bound * 4 + 4));
  }
  uint64_t *d_qoff = X.hits_P.as<uint64_t>() + runs + 1;
  HIP_TRY(launch_hits_order_batch(X.hits.as<uint64_t>(), X.hits_n.as<uint32_t>(), nc, R, X.hits_P.as<uint64_t>(),
                                  X.hits_c.as<uint64_t>(), X.hits_s.as<uint64_t>(),
                                  keys_out ? nullptr : X.out_doc.as<uint32_t>(),
                                  keys_out ? nullptr : X.out_score.as<float>(), d_qoff, keys_out, doc_base, bound,
                                  ix->num_cus * 4, s));
  if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_2], s));
  qoff_h->resize(nc + 1);
  HIP_TRY(hipMemcpyAsync(qoff_h->data(), d_qoff, ((size_t)nc + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  X.q_in_pending = false;
  return TFIDF_OK;
}

// Every hit of each of a prepared batch's n_q queries, chunk by chunk, into the
// caller's arrays (hit_offsets zeroed by the caller).  ms_before: device time the
// call spent ahead of the scoring, added to the total of tfidf_last_search_ms
// (*ms_total, when non-null, receives that total).
static int batch_all_prepared(tfidf_index *ix, Snapshot &S, StatsView &V, SearchCtx &X, hipStream_t s,
                              const QueryBatch &qb, uint32_t n_q, uint32_t *doc_ids, float *scores, uint64_t cap,
                              uint64_t *hit_offsets, uint64_t *n_out, float ms_before = 0.0f,
                              float *ms_total = nullptr) {
  const uint32_t fixed = all_hits_fixed_chunk();
  std::vector<uint64_t> qoff_h;
  uint64_t total = 0;
  bool any = false, fits = true;
  for (uint32_t a = 0; a < n_q;) {
    uint32_t z = a;
    uint64_t bound = 0;
    all_hits_chunk(qb, S, a, n_q, fixed, &z, &bound);
    const uint32_t nc = z - a;
    if (int rc = all_hits_score_chunk(ix, S, V, X, s, qb, a, z, bound, &any, nullptr, 0, &qoff_h)) return rc;
    if (!qoff_h.empty()) {
      const uint64_t H = qoff_h[nc];
      for (uint32_t i = 1; i <= nc; i++) hit_offsets[a + i] = total + qoff_h[i];
      fits = fits && total + H <= cap;
      if (fits && H) {
        // the chunk's hits, contiguous, at the batch's running offset
        HIP_TRY(hipMemcpyAsync(doc_ids + total, X.out_doc.p, H * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(scores + total, X.out_score.p, H * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
      }
      total += H;
    } else {
      for (uint32_t i = 1; i <= nc; i++) hit_offsets[a + i] = total;     // no term of the chunk is present
    }
    a = z;
  }
  *n_out = total;
  const float ms_all = ms_before + (any ? qev_ms(X, QEV_0, QEV_2) : 0.0f);
  set_route_ms(ix, any ? qev_ms(X, QEV_0, QEV_1) : 0.0f, ms_all);
  if (ms_total) *ms_total = ms_all;
  if (!fits) return fail(TFIDF_E_BUFFER, "need %llu result slots", (unsigned long long)total);
  return TFIDF_OK;
}

static int batch_all_on(tfidf_index *ix, Snapshot &S, StatsView &V, const uint8_t *q_utf8, const uint64_t *q_offsets,
                        uint32_t n_q, uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                        uint64_t *n_out) {
  for (uint32_t i = 0; i <= n_q; i++) hit_offsets[i] = 0;
  *n_out = 0;
  if (n_q == 0 || S.n_docs == 0) return TFIDF_OK;
  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();
  DeviceGuard g(ix->cfg.device);
  QueryBatch qb;
  if (int e = prepare_batch(ix, S, V, q_utf8, q_offsets, n_q, &qb)) return e;
  return batch_all_prepared(ix, S, V, X, s, qb, n_q, doc_ids, scores, cap, hit_offsets, n_out);
}

extern "C" int tfidf_search_batch_all(tfidf_index *ix, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                      uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                      uint64_t *n_out) {
  if (!ix || !hit_offsets || !n_out || (n_q && !q_offsets) || (cap && (!doc_ids || !scores)))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "search before commit");
  return batch_all_on(ix, *snap, *view, q_utf8, q_offsets, n_q, doc_ids, scores, cap, hit_offsets, n_out);
}

extern "C" int tfidf_reader_search_batch_all(tfidf_reader *rd, const uint8_t *q_utf8, const uint64_t *q_offsets,
                                             uint32_t n_q, uint32_t *doc_ids, float *scores, uint64_t cap,
                                             uint64_t *hit_offsets, uint64_t *n_out) {
  if (!rd || !hit_offsets || !n_out || (n_q && !q_offsets) || (cap && (!doc_ids || !scores)))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  return batch_all_on(rd->ix, *rd->S, *rd->V, q_utf8, q_offsets, n_q, doc_ids, scores, cap, hit_offsets, n_out);
}

// ---------------------------------------------------------------------------
// fuzzy search (fuzzy_search_plan.h, kernels_fuzzy_search.hip): FuzzyQuery's
// top-terms blended-frequency rewrite.  The expansion of every input term comes
// from the term lookup's scans with the search's key and candidate rule and the
// device selection (fuzzy_on with ex); nothing but the expansions' slots, boosts
// and distances reaches the host.  The search then weights every term of an
// expansion with boost * idf(largest df of the expansion) and hands one
// all-SHOULD prepared query per input term to the batched all-hits path; the
// expand call resolves the strings (exact keys from the host mirror).

static int fuzzy_search_check_args(const uint8_t *t_utf8, const uint64_t *t_offsets, uint32_t n_terms,
                                   uint32_t max_edits, uint32_t max_exp) {
  if (max_exp < 1 || max_exp > kFzsMaxExpansions)
    return fail(TFIDF_E_INVALID_ARG, "max_expansions %u outside 1..%u", max_exp, kFzsMaxExpansions);
  return fuzzy_check_args(t_utf8, t_offsets, n_terms, max_edits, 0, true);
}

static int fuzzy_expand_on(tfidf_index *ix, Snapshot &S, const uint8_t *t_utf8, const uint64_t *t_offsets,
                           uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len, uint32_t max_exp,
                           uint64_t *cand_offsets, uint64_t *n_within, uint64_t *term_offsets, uint8_t *terms,
                           uint64_t terms_cap, uint32_t *df, uint8_t *dist, float *boosts, uint64_t cand_cap,
                           uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device) {
  if (int rc = fuzzy_search_check_args(t_utf8, t_offsets, n_terms, max_edits, max_exp)) return rc;
  if (!cand_offsets || (n_terms && !n_within) || !n_cands || !n_term_bytes)
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (ms_device) *ms_device = 0.0f;
  FuzzyLists fl;
  FuzzyExpansions ex;
  if (int rc = fuzzy_on(ix, S, t_utf8, t_offsets, n_terms, max_edits, prefix_len, max_exp, &fl, &ex)) return rc;
  if (ms_device) *ms_device = fl.ms_device;
  set_route_ms(ix, 0.0f, fl.ms_device);
  DeviceGuard g(ix->cfg.device);                       // slot_term may read a reference occurrence
  std::vector<std::string> strs;
  std::string ts;
  uint64_t nc = 0, nb = 0;
  cand_offsets[0] = 0;
  for (uint32_t i = 0; i < n_terms; i++) {
    n_within[i] = fl.n_within[i];
    for (const FzsEntry &e : ex[i]) {
      if (int rc = slot_term(S, e.slot, &ts)) return rc;
      nb += ts.size();
      strs.push_back(ts);
    }
    nc += ex[i].size();
    cand_offsets[i + 1] = nc;
  }
  *n_cands = nc;
  *n_term_bytes = nb;
  if (nc > cand_cap || nb > terms_cap || (nc && (!term_offsets || !df || !dist || !boosts)) || (nb && !terms))
    return fail(TFIDF_E_BUFFER, "need %llu candidate slots and %llu term bytes", (unsigned long long)nc,
                (unsigned long long)nb);
  uint64_t at = 0, b = 0;
  if (term_offsets) term_offsets[0] = 0;
  for (uint32_t i = 0; i < n_terms; i++)
    for (const FzsEntry &e : ex[i]) {
      const std::string &t = strs[at];
      memcpy(terms + b, t.data(), t.size());
      b += t.size();
      df[at] = S.h_df[e.slot];
      dist[at] = (uint8_t)e.dist;
      boosts[at] = fzs_bits_float(e.boost_bits);
      term_offsets[++at] = b;
    }
  return TFIDF_OK;
}

static int fuzzy_search_on(tfidf_index *ix, Snapshot &S, StatsView &V, const uint8_t *t_utf8,
                           const uint64_t *t_offsets, uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len,
                           uint32_t max_exp, uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                           uint32_t *n_expanded, uint64_t *n_out, float *ms_device) {
  if (int rc = fuzzy_search_check_args(t_utf8, t_offsets, n_terms, max_edits, max_exp)) return rc;
  if (!hit_offsets || !n_out || (n_terms && !n_expanded) || (cap && (!doc_ids || !scores)))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (ms_device) *ms_device = 0.0f;
  for (uint32_t i = 0; i <= n_terms; i++) hit_offsets[i] = 0;
  *n_out = 0;
  FuzzyLists fl;
  FuzzyExpansions ex;
  if (int rc = fuzzy_on(ix, S, t_utf8, t_offsets, n_terms, max_edits, prefix_len, max_exp, &fl, &ex)) return rc;
  if (ms_device) *ms_device = fl.ms_device;
  set_route_ms(ix, 0.0f, fl.ms_device);
  for (uint32_t i = 0; i < n_terms; i++) n_expanded[i] = (uint32_t)ex[i].size();
  if (n_terms == 0 || S.n_docs == 0) return TFIDF_OK;
  if (int e = V.wait_gdf()) return e;
  // one flat disjunction per input term: SHOULD clauses in selection order, all weighted with the expansion's largest df
  QueryBatch qb;
  for (uint32_t i = 0; i < n_terms; i++) {
    PreparedQuery pq;
    if (V.doc_count) {
      uint64_t max_df = 0;
      for (const FzsEntry &e : ex[i]) max_df = std::max<uint64_t>(max_df, V.global ? V.gdf[e.slot] : S.h_df[e.slot]);
      const float idf = bm25_idf(max_df, V.doc_count);
      for (const FzsEntry &e : ex[i]) {
        volatile float w = fzs_bits_float(e.boost_bits) * idf;         // BM25Scorer: weight = boost * idf
        const float wv = w;
        pq.slot.push_back(S.col_of(e.slot));
        pq.ldf.push_back(S.h_df[e.slot]);
        pq.w.push_back(wv);
        pq.role.push_back(kRoleShould << 24);
      }
    }
    qb.add(pq);
  }
  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  DeviceGuard g(ix->cfg.device);
  return batch_all_prepared(ix, S, V, *lease.c, lease.stream(), qb, n_terms, doc_ids, scores, cap, hit_offsets, n_out,
                            fl.ms_device, ms_device);
}

extern "C" int tfidf_fuzzy_expand_batch(tfidf_index *ix, const uint8_t *t_utf8, const uint64_t *t_offsets,
                                        uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len,
                                        uint32_t max_expansions, uint64_t *cand_offsets, uint64_t *n_within,
                                        uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *df,
                                        uint8_t *dist, float *boosts, uint64_t cand_cap, uint64_t *n_cands,
                                        uint64_t *n_term_bytes, float *ms_device) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  if (int rc = fuzzy_search_check_args(t_utf8, t_offsets, n_terms, max_edits, max_expansions)) return rc;
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "fuzzy expansion before commit");
  return fuzzy_expand_on(ix, *snap, t_utf8, t_offsets, n_terms, max_edits, prefix_len, max_expansions, cand_offsets,
                         n_within, term_offsets, terms, terms_cap, df, dist, boosts, cand_cap, n_cands, n_term_bytes,
                         ms_device);
}

extern "C" int tfidf_reader_fuzzy_expand_batch(tfidf_reader *rd, const uint8_t *t_utf8, const uint64_t *t_offsets,
                                               uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len,
                                               uint32_t max_expansions, uint64_t *cand_offsets, uint64_t *n_within,
                                               uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap,
                                               uint32_t *df, uint8_t *dist, float *boosts, uint64_t cand_cap,
                                               uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  return fuzzy_expand_on(rd->ix, *rd->S, t_utf8, t_offsets, n_terms, max_edits, prefix_len, max_expansions,
                         cand_offsets, n_within, term_offsets, terms, terms_cap, df, dist, boosts, cand_cap, n_cands,
                         n_term_bytes, ms_device);
}

// the batch of one, without the offsets arrays of the input and of the terms' candidates
extern "C" int tfidf_fuzzy_expand(tfidf_index *ix, const uint8_t *term, uint64_t len, uint32_t max_edits,
                                  uint32_t prefix_len, uint32_t max_expansions, uint64_t *n_within,
                                  uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *df,
                                  uint8_t *dist, float *boosts, uint64_t cand_cap, uint64_t *n_cands,
                                  uint64_t *n_term_bytes, float *ms_device) {
  if (!n_within || (!term && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t t_off[2] = {0, len};
  uint64_t c_off[2];
  return tfidf_fuzzy_expand_batch(ix, term, t_off, 1, max_edits, prefix_len, max_expansions, c_off, n_within,
                                  term_offsets, terms, terms_cap, df, dist, boosts, cand_cap, n_cands, n_term_bytes,
                                  ms_device);
}

extern "C" int tfidf_reader_fuzzy_expand(tfidf_reader *rd, const uint8_t *term, uint64_t len, uint32_t max_edits,
                                         uint32_t prefix_len, uint32_t max_expansions, uint64_t *n_within,
                                         uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *df,
                                         uint8_t *dist, float *boosts, uint64_t cand_cap, uint64_t *n_cands,
                                         uint64_t *n_term_bytes, float *ms_device) {
  if (!n_within || (!term && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t t_off[2] = {0, len};
  uint64_t c_off[2];
  return tfidf_reader_fuzzy_expand_batch(rd, term, t_off, 1, max_edits, prefix_len, max_expansions, c_off, n_within,
                                         term_offsets, terms, terms_cap, df, dist, boosts, cand_cap, n_cands,
                                         n_term_bytes, ms_device);
}

extern "C" int tfidf_search_fuzzy_batch(tfidf_index *ix, const uint8_t *t_utf8, const uint64_t *t_offsets,
                                        uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len,
                                        uint32_t max_expansions, uint32_t *doc_ids, float *scores, uint64_t cap,
                                        uint64_t *hit_offsets, uint32_t *n_expanded, uint64_t *n_out,
                                        float *ms_device) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  if (int rc = fuzzy_search_check_args(t_utf8, t_offsets, n_terms, max_edits, max_expansions)) return rc;
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "fuzzy search before commit");
  return fuzzy_search_on(ix, *snap, *view, t_utf8, t_offsets, n_terms, max_edits, prefix_len, max_expansions, doc_ids,
                         scores, cap, hit_offsets, n_expanded, n_out, ms_device);
}

extern "C" int tfidf_reader_search_fuzzy_batch(tfidf_reader *rd, const uint8_t *t_utf8, const uint64_t *t_offsets,
                                               uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len,
                                               uint32_t max_expansions, uint32_t *doc_ids, float *scores, uint64_t cap,
                                               uint64_t *hit_offsets, uint32_t *n_expanded, uint64_t *n_out,
                                               float *ms_device) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  return fuzzy_search_on(rd->ix, *rd->S, *rd->V, t_utf8, t_offsets, n_terms, max_edits, prefix_len, max_expansions,
                         doc_ids, scores, cap, hit_offsets, n_expanded, n_out, ms_device);
}

extern "C" int tfidf_search_fuzzy(tfidf_index *ix, const uint8_t *term, uint64_t len, uint32_t max_edits,
                                  uint32_t prefix_len, uint32_t max_expansions, uint32_t *doc_ids, float *scores,
                                  uint64_t cap, uint32_t *n_expanded, uint64_t *n_out, float *ms_device) {
  if (!n_expanded || (!term && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t t_off[2] = {0, len};
  uint64_t h_off[2];
  return tfidf_search_fuzzy_batch(ix, term, t_off, 1, max_edits, prefix_len, max_expansions, doc_ids, scores, cap,
                                  h_off, n_expanded, n_out, ms_device);
}

extern "C" int tfidf_reader_search_fuzzy(tfidf_reader *rd, const uint8_t *term, uint64_t len, uint32_t max_edits,
                                         uint32_t prefix_len, uint32_t max_expansions, uint32_t *doc_ids,
                                         float *scores, uint64_t cap, uint32_t *n_expanded, uint64_t *n_out,
                                         float *ms_device) {
  if (!n_expanded || (!term && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t t_off[2] = {0, len};
  uint64_t h_off[2];
  return tfidf_reader_search_fuzzy_batch(rd, term, t_off, 1, max_edits, prefix_len, max_expansions, doc_ids, scores,
                                         cap, h_off, n_expanded, n_out, ms_device);
}

// ---------------------------------------------------------------------------
// exact phrase search (phrase_plan.h, kernels_phrase.hip): the documents that
// hold the phrase's terms next to each other in order, scored by BM25 over the
// phrase frequency (Lucene's PhraseQuery with slop 0).  The sloppy calls
// (tfidf_search_phrase_slop*) take the same path with a slop per phrase: they
// differ in the frequency kernel (k_ph_sloppy_freq, a float frequency) and the
// score kernel, nothing else.
//
// Per call: the phrases are analysed and looked up on the host, one upload
// carries their key segments, ordinal sequences and weights.  Per all-hits chunk
// of phrases (all_hits_chunk): the conjunction of each phrase's distinct terms
// gives the candidate rows (phrase, document), phrase-major on the device; their
// ids come to the host, their staged ids go back, the extents come to the host
// (three copies, two synchronisations).  Per item chunk of rows (hl_plan_chunks
// by the (row, chunk) items): plan upload, count pass, two scans, row offsets,
// one copy back and a synchronisation.  Per row chunk (by the listed tokens):
// fill, frequency, score, flag scan, compaction, one copy of the scanned flags
// and a synchronisation (the hit count sizes the sort), two stable radix passes,
// emit, and three copies of the chunk's ordered hits to the caller's arrays.
// Rows are whole documents, so a row chunk's frequencies are final.  A phrase
// whose rows span several row chunks has one ordered run per chunk, contiguous
// in the output; the host merges them after the last chunk.

struct PhrasePrep {
  std::vector<uint32_t> seq;         // ordinal of the term at each phrase position
  std::vector<uint32_t> slot;        // dictionary slot per distinct term, in order of first appearance
  std::vector<std::string> terms;    // the distinct terms
  float w = 0.0f;                    // 1.0f * (float) sum of the positions' idf
  bool work = false;
};

// analysed, deduplicated and looked up; a phrase without work (no term, not
// UTF-8, a term this snapshot lacks) keeps work == false
// slop > 0: a phrase of several terms must have at most kPhMaxSloppyTerms, all different
static int phrase_prepare(Snapshot &S, StatsView &V, const uint8_t *p, uint64_t n, uint32_t index, uint32_t slop,
                          PhrasePrep *pp) {
  std::vector<std::string> toks;
  if (!analyze(p, n, &toks)) return TFIDF_OK;
  if (toks.size() > kPhMaxTerms)
    return fail(TFIDF_E_INVALID_ARG, "phrase %u has %zu terms (more than %u)", index, toks.size(), kPhMaxTerms);
  if (slop > 0 && toks.size() > 1) {
    if (toks.size() > kPhMaxSloppyTerms)
      return fail(TFIDF_E_UNSUPPORTED_QUERY, "phrase %u has %zu terms (more than %u) and slop %u", index, toks.size(),
                  kPhMaxSloppyTerms, slop);
    if (std::unordered_set<std::string>(toks.begin(), toks.end()).size() != toks.size())
      return fail(TFIDF_E_UNSUPPORTED_QUERY, "phrase %u repeats a term and has slop %u", index, slop);
  }
  if (toks.empty() || V.doc_count == 0) return TFIDF_OK;
  std::unordered_map<std::string, uint32_t> ordinal;
  for (const std::string &t : toks) {
    auto it = ordinal.find(t);
    if (it == ordinal.end()) {
      it = ordinal.emplace(t, (uint32_t)pp->terms.size()).first;
      pp->terms.push_back(t);
    }
    pp->seq.push_back(it->second);
  }
  for (const std::string &t : pp->terms) {
    const uint32_t s = lookup_term(S, t);
    if (s == kInvalidSlot || S.h_df[s] == 0) return TFIDF_OK;
    pp->slot.push_back(s);
  }
  // PhraseWeight.getStats / BM25Similarity.idfExplain(CollectionStatistics, TermStatistics[])
  double idf = 0.0;
  for (uint32_t o : pp->seq) {
    const uint32_t s = pp->slot[o];
    idf += (double)bm25_idf(V.global ? V.gdf[s] : S.h_df[s], V.doc_count);
  }
  volatile float w = 1.0f * (float)idf;
  pp->w = w;
  pp->work = true;
  return TFIDF_OK;
}

// slops == nullptr: the exact calls, freqs holds counts; else one slop per
// phrase and freqs holds float frequencies (4 bytes per hit either way)
static int phrase_batch_on(tfidf_index *ix, Snapshot &S, StatsView &V, const uint8_t *p_utf8,
                           const uint64_t *p_offsets, const uint32_t *slops, uint32_t n_p, uint32_t *doc_ids,
                           float *scores, uint32_t *freqs, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out) {
  if (n_p && p_offsets[0] != 0) return fail(TFIDF_E_INVALID_ARG, "p_offsets[0] is not 0");
  for (uint32_t i = 0; i < n_p; i++)
    if (p_offsets[i + 1] < p_offsets[i]) return fail(TFIDF_E_INVALID_ARG, "p_offsets decrease at phrase %u", i);
  if (int e = V.wait_gdf()) return e;
  DeviceGuard g(ix->cfg.device);                       // slot_term may read a reference occurrence
  std::vector<PhrasePrep> pp(n_p);
  for (uint32_t i = 0; i < n_p; i++)
    if (int rc = phrase_prepare(S, V, p_utf8 + p_offsets[i], p_offsets[i + 1] - p_offsets[i], i, slops ? slops[i] : 0,
                                &pp[i]))
      return rc;
  for (uint32_t i = 0; i <= n_p; i++) hit_offsets[i] = 0;
  *n_out = 0;
  uint64_t n_cand = 0, n_row_chunks = 0;
  auto report = [&]() {
    std::lock_guard<std::mutex> lk(ix->ms_mu);
    ix->last_ph_candidates = n_cand;
    ix->last_ph_row_chunks = n_row_chunks;
  };
  bool any_work = false;
  for (const PhrasePrep &p : pp) any_work |= p.work;
  if (!any_work || S.n_docs == 0) {
    report();
    return TFIDF_OK;
  }

  // the conjunctions: every distinct term a MUST clause of its own
  QueryBatch qb;
  std::vector<HlKey> keys;
  std::vector<uint32_t> key_off((size_t)n_p + 1, 0), seq_off((size_t)n_p + 1, 0), seq;
  std::vector<float> w(n_p, 0.0f);
  for (uint32_t i = 0; i < n_p; i++) {
    key_off[i] = (uint32_t)keys.size();
    seq_off[i] = (uint32_t)seq.size();
    PreparedQuery pq;
    if (pp[i].work) {
      for (size_t o = 0; o < pp[i].slot.size(); o++) {
        const uint32_t s = pp[i].slot[o];
        pq.slot.push_back(S.col_of(s));
        pq.ldf.push_back(S.h_df[s]);
        pq.w.push_back(bm25_idf(V.global ? V.gdf[s] : S.h_df[s], V.doc_count));
        pq.role.push_back(kRoleMust << 24 | (uint32_t)o);
      }
      pq.meta = (uint32_t)pp[i].slot.size();
      hl_append_keys(S, pp[i].terms, &keys);
      seq.insert(seq.end(), pp[i].seq.begin(), pp[i].seq.end());
      w[i] = pp[i].w;
      if (keys.size() > (1ull << 30) || seq.size() > (1ull << 30))
        return fail(TFIDF_E_INVALID_ARG, "more than 2^30 phrase terms in one call");
    }
    qb.add(pq);
  }
  key_off[n_p] = (uint32_t)keys.size();
  seq_off[n_p] = (uint32_t)seq.size();

  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();

  // one upload: key segments, ordinal sequences, weights, slops
  const size_t in_soff = up16(((size_t)n_p + 1) * 4), in_w = up16(in_soff + ((size_t)n_p + 1) * 4),
               in_seq = up16(in_w + (size_t)n_p * 4), in_keys = up16(in_seq + seq.size() * 4),
               in_slop = up16(in_keys + keys.size() * sizeof(HlKey)),
               in_end = up16(in_slop + (slops ? (size_t)n_p * 4 : 0));
  std::vector<uint8_t> h_in(in_end);
  memcpy(h_in.data(), key_off.data(), ((size_t)n_p + 1) * 4);
  memcpy(h_in.data() + in_soff, seq_off.data(), ((size_t)n_p + 1) * 4);
  memcpy(h_in.data() + in_w, w.data(), (size_t)n_p * 4);
  memcpy(h_in.data() + in_seq, seq.data(), seq.size() * 4);
  memcpy(h_in.data() + in_keys, keys.data(), keys.size() * sizeof(HlKey));
  if (slops) memcpy(h_in.data() + in_slop, slops, (size_t)n_p * 4);
  HIP_TRY(X.ph_in.reserve(in_end));
  uint8_t *pb = X.ph_in.as<uint8_t>();
  if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_P0], s));
  HIP_TRY(hipMemcpyAsync(pb, h_in.data(), in_end, hipMemcpyHostToDevice, s));
  const uint32_t *d_koff = reinterpret_cast<uint32_t *>(pb), *d_soff = reinterpret_cast<uint32_t *>(pb + in_soff),
                 *d_seq = reinterpret_cast<uint32_t *>(pb + in_seq),
                 *d_slop = reinterpret_cast<uint32_t *>(pb + in_slop);
  const float *d_w = reinterpret_cast<float *>(pb + in_w);
  const HlKey *d_keys = reinterpret_cast<HlKey *>(pb + in_keys);
  const uint8_t *d_text = S.text->as<uint8_t>();

  const uint64_t budget_i = hl_budget("TFIDF_HL_CHUNK_ITEMS", kHlChunkItems),
                 budget_m = hl_budget("TFIDF_HL_CHUNK_MATCHES", kHlChunkMatches);
  const uint32_t fixed = all_hits_fixed_chunk();
  std::vector<uint64_t> cnt(n_p, 0), qoff_h, h_ext, row_items, cuts, first, h_row, row_m, sub, h_at;
  std::vector<uint32_t> runs(n_p, 0), h_docs, h_in2;
  std::vector<uint8_t> skip;
  std::vector<HlItem> items;
  uint64_t run = 0;
  bool any = false, fits = true;
  for (uint32_t a = 0; a < n_p;) {
    uint32_t z = a;
    uint64_t bound = 0;
    all_hits_chunk(qb, S, a, n_p, fixed, &z, &bound);
    const uint32_t nc = z - a;
    if (int rc = all_hits_score_chunk(ix, S, V, X, s, qb, a, z, bound, &any, nullptr, 0, &qoff_h)) return rc;
    const uint32_t q_lo = a;
    a = z;
    if (qoff_h.empty() || qoff_h[nc] == 0) continue;
    const uint64_t R = qoff_h[nc];
    if (R > 0xFFFFFFFFull) return fail(TFIDF_E_INVALID_ARG, "more than 2^32 candidate rows in one chunk of phrases");
    n_cand += R;
    const uint32_t *d_docs = X.out_doc.as<uint32_t>();
    h_docs.resize(R);
    HIP_TRY(hipMemcpyAsync(h_docs.data(), d_docs, R * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // staged ids and row -> phrase up, extents back
    const size_t in_rowq = up16(R * 4), in_ext = up16(in_rowq + R * 4);
    h_in2.resize(in_ext / 4);
    for (uint64_t r = 0; r < R; r++) h_in2[r] = (uint32_t)S.staged_of(h_docs[r]);
    for (uint32_t i = 0; i < nc; i++)
      for (uint64_t r = qoff_h[i]; r < qoff_h[i + 1]; r++) h_in2[in_rowq / 4 + r] = q_lo + i;
    HIP_TRY(X.hl_in.reserve(in_ext + R * 16));
    uint8_t *ib = X.hl_in.as<uint8_t>();
    const uint32_t *d_staged = reinterpret_cast<uint32_t *>(ib), *d_rowq = reinterpret_cast<uint32_t *>(ib + in_rowq);
    uint64_t *d_ext = reinterpret_cast<uint64_t *>(ib + in_ext);
    h_ext.resize(2 * R);
    HIP_TRY(hipMemcpyAsync(ib, h_in2.data(), in_ext, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_hl_extents(S.offsets->as<uint64_t>(), d_staged, R, d_ext, s));
    HIP_TRY(hipMemcpyAsync(h_ext.data(), d_ext, R * 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    skip.assign(R, 0);
    row_items.assign(R, 0);
    for (uint64_t r = 0; r < R; r++) {
      const uint64_t L = h_ext[2 * r + 1] - h_ext[2 * r];
      if (L > 0xFFFFFFFFull) return fail(TFIDF_E_INVALID_ARG, "a candidate document of more than 2^32 bytes");
      skip[r] = !S.malformed.empty() && std::binary_search(S.malformed.begin(), S.malformed.end(), h_docs[r]);
      row_items[r] = skip[r] ? 0 : hl_num_chunks(L);
    }
    cuts.clear();
    hl_plan_chunks(row_items.data(), nullptr, 0, R, budget_i, ~0ull, &cuts);
    for (size_t ci = 0; ci + 1 < cuts.size(); ci++) {
      const uint64_t r0 = cuts[ci], nr = cuts[ci + 1] - r0;
      hl_plan(h_ext.data() + 2 * r0, skip.data() + r0, nr, &items, &first);
      if (items.size() > (1ull << 24))
        return fail(TFIDF_E_INVALID_ARG, "a document of more than 2^24 chunks of %llu bytes",
                    (unsigned long long)kHlChunkBytes);
      const uint32_t n_items = (uint32_t)items.size();
      const uint64_t n_cnt = (uint64_t)n_items * kHlLanes;
      const size_t off_row = (nr + 1) * 8, off_items = 2 * off_row,
                   off_all = up16(off_items + (size_t)n_items * sizeof(HlItem)), off_listed = off_all + (n_cnt + 1) * 8;
      HIP_TRY(X.hl_cnt.reserve(off_listed + (n_cnt + 1) * 8));
      uint8_t *cb = X.hl_cnt.as<uint8_t>();
      uint64_t *d_first = reinterpret_cast<uint64_t *>(cb), *d_row = reinterpret_cast<uint64_t *>(cb + off_row),
               *d_all = reinterpret_cast<uint64_t *>(cb + off_all),
               *d_listed = reinterpret_cast<uint64_t *>(cb + off_listed);
      HlItem *d_items = reinterpret_cast<HlItem *>(cb + off_items);
      h_row.assign(nr + 1, 0);
      if (n_items) {
        // tokens and listed tokens per slice, their scans, the rows' offsets
        HIP_TRY(hipMemcpyAsync(d_first, first.data(), (nr + 1) * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_items, items.data(), (size_t)n_items * sizeof(HlItem), hipMemcpyHostToDevice, s));
        HIP_TRY(launch_ph_scan(false, d_text, d_ext + 2 * r0, d_items, 0, n_items, d_keys, d_koff, d_rowq + r0,
                               S.hash_seed, d_first, d_all, d_listed, 0, nullptr, nullptr, s));
        HIP_TRY(exclusive_scan_u64(d_all, d_all, n_cnt, s));
        HIP_TRY(exclusive_scan_u64(d_listed, d_listed, n_cnt, s));
        HIP_TRY(launch_hl_row_offsets(d_listed, d_first, nr, 0, d_row, s));
        HIP_TRY(hipMemcpyAsync(h_row.data(), d_row, (nr + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
      } else {
        HIP_TRY(hipMemsetAsync(d_row, 0, (nr + 1) * 8, s));
      }
      row_m.resize(nr);
      for (uint64_t i = 0; i < nr; i++) row_m[i] = h_row[i + 1] - h_row[i];
      sub.clear();
      hl_plan_chunks(nullptr, row_m.data(), 0, nr, ~0ull, budget_m, &sub);
      for (size_t si = 0; si + 1 < sub.size(); si++) {
        const uint64_t s0 = sub[si], ns = sub[si + 1] - s0, m_base = h_row[s0], T = h_row[s0 + ns] - m_base;
        const uint64_t Tc = std::max<uint64_t>(T, 1), g0 = r0 + s0;
        n_row_chunks++;
        const uint32_t i0 = (uint32_t)first[s0], ni = (uint32_t)first[s0 + ns] - i0;
        HIP_TRY(X.hl_m.reserve(Tc * 8));
        uint32_t *m_pos = X.hl_m.as<uint32_t>(), *m_ord = m_pos + Tc;
        if (T)
          HIP_TRY(launch_ph_scan(true, d_text, d_ext + 2 * r0, d_items, i0, ni, d_keys, d_koff, d_rowq + r0,
                                 S.hash_seed, d_first, d_all, d_listed, m_base, m_pos, m_ord, s));
        // per row: freq, key, flag (scanned in place), then the packed hits
        const size_t s_flag = up16(ns * 8), s_ckey = up16(s_flag + (ns + 1) * 8), s_freq = up16(s_ckey + ns * 8),
                     s_crow = up16(s_freq + ns * 4), s_end = up16(s_crow + ns * 4);
        HIP_TRY(X.ph_s.reserve(s_end));
        uint8_t *sb = X.ph_s.as<uint8_t>();
        uint64_t *r_key = reinterpret_cast<uint64_t *>(sb), *r_flag = reinterpret_cast<uint64_t *>(sb + s_flag),
                 *c_key = reinterpret_cast<uint64_t *>(sb + s_ckey);
        uint32_t *r_freq = reinterpret_cast<uint32_t *>(sb + s_freq), *c_row = reinterpret_cast<uint32_t *>(sb + s_crow);
        if (slops) {
          float *r_freq_f = reinterpret_cast<float *>(r_freq);
          HIP_TRY(launch_ph_sloppy_freq(d_row + s0, m_base, m_pos, m_ord, d_rowq + g0, d_seq, d_soff, d_slop, ns,
                                        r_freq_f, s));
          HIP_TRY(launch_ph_score_f(r_freq_f, d_docs + g0, d_rowq + g0, d_w, V.cache.as<float>(),
                                    S.doc_norm.as<uint8_t>(), ns, r_key, r_flag, s));
        } else {
          HIP_TRY(launch_ph_freq(d_row + s0, m_base, m_pos, m_ord, d_rowq + g0, d_seq, d_soff, ns, r_freq, s));
          HIP_TRY(launch_ph_score(r_freq, d_docs + g0, d_rowq + g0, d_w, V.cache.as<float>(),
                                  S.doc_norm.as<uint8_t>(), ns, r_key, r_flag, s));
        }
        HIP_TRY(exclusive_scan_u64(r_flag, r_flag, ns, s));
        HIP_TRY(launch_ph_compact(r_key, r_freq, r_flag, ns, c_key, c_row, s));
        h_at.resize(ns + 1);
        HIP_TRY(hipMemcpyAsync(h_at.data(), r_flag, (ns + 1) * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const uint64_t Hn = h_at[ns];
        if (Hn == 0) continue;
        // the chunk's phrases and their hits
        const uint32_t qa = h_in2[in_rowq / 4 + g0], qz = h_in2[in_rowq / 4 + g0 + ns - 1];
        for (uint32_t q = qa; q <= qz; q++) {
          const uint64_t lo = std::max<uint64_t>(qoff_h[q - q_lo], g0), hi = std::min<uint64_t>(qoff_h[q - q_lo + 1], g0 + ns);
          if (hi <= lo) continue;
          const uint64_t c = h_at[hi - g0] - h_at[lo - g0];
          cnt[q] += c;
          if (c) runs[q]++;
        }
        fits = fits && run + Hn <= cap && doc_ids && scores && freqs;
        if (fits) {
          size_t tb = 0;
          HIP_TRY(ph_sort_bytes(&tb, (uint32_t)Hn));
          HIP_TRY(X.ph_tmp.reserve(tb));
          const size_t o_rowa = up16(Hn * 8), o_qa = up16(o_rowa + Hn * 4), o_qb = up16(o_qa + Hn * 4),
                       o_doc = up16(o_qb + Hn * 4), o_sc = up16(o_doc + Hn * 4), o_fr = up16(o_sc + Hn * 4),
                       o_end = up16(o_fr + Hn * 4);
          HIP_TRY(X.ph_o.reserve(o_end));
          uint8_t *ob = X.ph_o.as<uint8_t>();
          uint64_t *key_a = reinterpret_cast<uint64_t *>(ob);
          uint32_t *row_a = reinterpret_cast<uint32_t *>(ob + o_rowa), *q_a = reinterpret_cast<uint32_t *>(ob + o_qa),
                   *q_b = reinterpret_cast<uint32_t *>(ob + o_qb), *e_doc = reinterpret_cast<uint32_t *>(ob + o_doc),
                   *e_fr = reinterpret_cast<uint32_t *>(ob + o_fr);
          float *e_sc = reinterpret_cast<float *>(ob + o_sc);
          const uint32_t *rows = nullptr;
          HIP_TRY(ph_sort(X.ph_tmp.p, tb, c_key, key_a, c_row, row_a, q_a, q_b, d_rowq + g0, qa, qz - qa + 1,
                          (uint32_t)Hn, &rows, s));
          HIP_TRY(launch_ph_emit(rows, r_key, r_freq, Hn, e_doc, e_sc, e_fr, s));
          HIP_TRY(hipMemcpyAsync(doc_ids + run, e_doc, Hn * 4, hipMemcpyDeviceToHost, s));
          HIP_TRY(hipMemcpyAsync(scores + run, e_sc, Hn * 4, hipMemcpyDeviceToHost, s));
          HIP_TRY(hipMemcpyAsync(freqs + run, e_fr, Hn * 4, hipMemcpyDeviceToHost, s));
          HIP_TRY(hipStreamSynchronize(s));
        }
        run += Hn;
      }
    }
  }
  if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_P1], s));
  HIP_TRY(hipStreamSynchronize(s));
  // tfidf_last_search_ms: the conjunctions' scoring of the last chunk of phrases, the whole call on the device
  set_route_ms(ix, any ? qev_ms(X, QEV_0, QEV_1) : 0.0f, qev_ms(X, QEV_P0, QEV_P1));
  for (uint32_t i = 0; i < n_p; i++) hit_offsets[i + 1] = hit_offsets[i] + cnt[i];
  *n_out = run;
  report();
  if (!fits) return fail(TFIDF_E_BUFFER, "need %llu result slots", (unsigned long long)run);
  // a phrase whose rows spanned several row chunks: merge its ordered runs
  std::vector<uint64_t> order;
  std::vector<uint32_t> t_doc, t_fr;
  std::vector<float> t_sc;
  for (uint32_t q = 0; q < n_p; q++) {
    if (runs[q] <= 1) continue;
    const uint64_t b = hit_offsets[q], n = cnt[q];
    order.resize(n);
    for (uint64_t i = 0; i < n; i++) {
      uint32_t bits;
      memcpy(&bits, scores + b + i, 4);
      order[i] = ph_sort_key(bits, doc_ids[b + i]);
    }
    std::vector<uint64_t> idx(n);
    for (uint64_t i = 0; i < n; i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](uint64_t x, uint64_t y) { return order[x] < order[y]; });
    t_doc.assign(doc_ids + b, doc_ids + b + n);
    t_sc.assign(scores + b, scores + b + n);
    t_fr.assign(freqs + b, freqs + b + n);
    for (uint64_t i = 0; i < n; i++) {
      doc_ids[b + i] = t_doc[idx[i]];
      scores[b + i] = t_sc[idx[i]];
      freqs[b + i] = t_fr[idx[i]];
    }
  }
  return TFIDF_OK;
}

static bool phrase_null_args(const void *h, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                             const uint32_t *doc_ids, const float *scores, const uint32_t *freqs, uint64_t cap,
                             const uint64_t *hit_offsets, const uint64_t *n_out) {
  return !h || !hit_offsets || !n_out || (n_p && (!p_offsets || (!p_utf8 && p_offsets[n_p]))) ||
         (cap && (!doc_ids || !scores || !freqs));
}

extern "C" int tfidf_search_phrase_batch(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                         uint32_t n_p, uint32_t *doc_ids, float *scores, uint32_t *freqs, uint64_t cap,
                                         uint64_t *hit_offsets, uint64_t *n_out) {
  if (phrase_null_args(ix, p_utf8, p_offsets, n_p, doc_ids, scores, freqs, cap, hit_offsets, n_out))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "phrase search before commit");
  return phrase_batch_on(ix, *snap, *view, p_utf8, p_offsets, nullptr, n_p, doc_ids, scores, freqs, cap, hit_offsets,
                         n_out);
}

extern "C" int tfidf_reader_search_phrase_batch(tfidf_reader *rd, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                                uint32_t n_p, uint32_t *doc_ids, float *scores, uint32_t *freqs,
                                                uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out) {
  if (phrase_null_args(rd, p_utf8, p_offsets, n_p, doc_ids, scores, freqs, cap, hit_offsets, n_out))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  return phrase_batch_on(rd->ix, *rd->S, *rd->V, p_utf8, p_offsets, nullptr, n_p, doc_ids, scores, freqs, cap,
                         hit_offsets, n_out);
}

// the single forms: the batch of one phrase
extern "C" int tfidf_search_phrase(tfidf_index *ix, const uint8_t *p, uint64_t p_len, uint32_t *doc_ids, float *scores,
                                   uint32_t *freqs, uint64_t cap, uint64_t *n_out) {
  if (!n_out || (!p && p_len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t offs[2] = {0, p_len};
  uint64_t ho[2];
  return tfidf_search_phrase_batch(ix, p, offs, 1, doc_ids, scores, freqs, cap, ho, n_out);
}

extern "C" int tfidf_reader_search_phrase(tfidf_reader *rd, const uint8_t *p, uint64_t p_len, uint32_t *doc_ids,
                                          float *scores, uint32_t *freqs, uint64_t cap, uint64_t *n_out) {
  if (!n_out || (!p && p_len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t offs[2] = {0, p_len};
  uint64_t ho[2];
  return tfidf_reader_search_phrase_batch(rd, p, offs, 1, doc_ids, scores, freqs, cap, ho, n_out);
}

// the sloppy calls: the exact path with a slop per phrase and float frequencies
extern "C" int tfidf_search_phrase_slop_batch(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                              const uint32_t *slops, uint32_t n_p, uint32_t *doc_ids, float *scores,
                                              float *freqs, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out) {
  if (phrase_null_args(ix, p_utf8, p_offsets, n_p, doc_ids, scores, reinterpret_cast<uint32_t *>(freqs), cap,
                       hit_offsets, n_out) ||
      (n_p && !slops))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "phrase search before commit");
  const uint32_t none = 0;                             // n_p == 0: slops may be NULL
  return phrase_batch_on(ix, *snap, *view, p_utf8, p_offsets, slops ? slops : &none, n_p, doc_ids, scores,
                         reinterpret_cast<uint32_t *>(freqs), cap, hit_offsets, n_out);
}

extern "C" int tfidf_reader_search_phrase_slop_batch(tfidf_reader *rd, const uint8_t *p_utf8,
                                                     const uint64_t *p_offsets, const uint32_t *slops, uint32_t n_p,
                                                     uint32_t *doc_ids, float *scores, float *freqs, uint64_t cap,
                                                     uint64_t *hit_offsets, uint64_t *n_out) {
  if (phrase_null_args(rd, p_utf8, p_offsets, n_p, doc_ids, scores, reinterpret_cast<uint32_t *>(freqs), cap,
                       hit_offsets, n_out) ||
      (n_p && !slops))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint32_t none = 0;
  return phrase_batch_on(rd->ix, *rd->S, *rd->V, p_utf8, p_offsets, slops ? slops : &none, n_p, doc_ids, scores,
                         reinterpret_cast<uint32_t *>(freqs), cap, hit_offsets, n_out);
}

extern "C" int tfidf_search_phrase_slop(tfidf_index *ix, const uint8_t *p, uint64_t p_len, uint32_t slop,
                                        uint32_t *doc_ids, float *scores, float *freqs, uint64_t cap,
                                        uint64_t *n_out) {
  if (!n_out || (!p && p_len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t offs[2] = {0, p_len};
  uint64_t ho[2];
  return tfidf_search_phrase_slop_batch(ix, p, offs, &slop, 1, doc_ids, scores, freqs, cap, ho, n_out);
}

extern "C" int tfidf_reader_search_phrase_slop(tfidf_reader *rd, const uint8_t *p, uint64_t p_len, uint32_t slop,
                                               uint32_t *doc_ids, float *scores, float *freqs, uint64_t cap,
                                               uint64_t *n_out) {
  if (!n_out || (!p && p_len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t offs[2] = {0, p_len};
  uint64_t ho[2];
  return tfidf_reader_search_phrase_slop_batch(rd, p, offs, &slop, 1, doc_ids, scores, freqs, cap, ho, n_out);
}

extern "C" int tfidf_last_phrase_stats(const tfidf_index *ix, uint64_t *candidates, uint64_t *row_chunks) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->ms_mu);
  if (candidates) *candidates = ix->last_ph_candidates;
  if (row_chunks) *row_chunks = ix->last_ph_row_chunks;
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// compound queries ("Compound queries"; rules in
// compound_plan.h, device pass in kernels_compound.hip).  The call's clauses
// are grouped by kind (fuzzy clauses also by their parameters) and each group
// runs once as a batch through its route on the call's snapshot and view; the
// rows come back as the routes' host arrays.  Chunks of whole queries are then
// uploaded clause by clause, combined on the device and ordered by the batched
// all-hits merge; each chunk's hits go to the caller at the running offset.

namespace {
struct CqGroup {
  uint32_t kind = 0, max_edits = 0, prefix_len = 0, max_exp = 0;
  std::vector<uint32_t> clause;            // the call's clauses of this group, ascending
  std::vector<uint32_t> docs;              // their rows, one after the other
  std::vector<float> scores;               // empty: a set row, every score 1.0f
  std::vector<uint64_t> off{0};            // clause.size() + 1
};
struct CqRow {
  const uint32_t *docs = nullptr;
  const float *scores = nullptr;
  uint64_t n = 0;
};
}  // namespace

static float route_total_ms(tfidf_index *ix) {
  std::lock_guard<std::mutex> lk(ix->ms_mu);
  return ix->last_ms_total > 0.0f ? ix->last_ms_total : 0.0f;
}

// clauses [a, z) of a group through the group's route, appended to the group's rows; *ms: the route's device time
static int cq_run_slice(tfidf_index *ix, Snapshot &S, StatsView &V, const uint8_t *c_utf8, const uint64_t *c_offsets,
                        const tfidf_clause *clauses, CqGroup &g, size_t a, size_t z, float *ms) {
  const uint32_t n = (uint32_t)(z - a);
  std::string blob;
  std::vector<uint64_t> off((size_t)n + 1, 0);
  std::vector<uint32_t> slops(n ? n : 1, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t c = g.clause[a + i];
    if (c_offsets[c + 1] > c_offsets[c])
      blob.append(reinterpret_cast<const char *>(c_utf8 + c_offsets[c]), c_offsets[c + 1] - c_offsets[c]);
    off[i + 1] = blob.size();
    slops[i] = clauses[c].slop;
  }
  const uint8_t *text = reinterpret_cast<const uint8_t *>(blob.data());
  const uint64_t base = g.docs.size();
  if (g.kind == TFIDF_CLAUSE_WILDCARD || g.kind == TFIDF_CLAUSE_REGEX) {
    std::vector<std::vector<uint32_t>> tabs;
    if (g.kind == TFIDF_CLAUSE_REGEX)
      if (int rc = regex_compile_all(text, off.data(), n, &tabs)) return rc;
    WildcardLists wl;
    if (int rc = g.kind == TFIDF_CLAUSE_REGEX ? multiterm_on(ix, S, tabs, n, kRegexRoute, true, 0, &wl)
                                              : wildcard_on(ix, S, text, off.data(), n, true, 0, &wl))
      return rc;
    *ms += wl.ms_device > 0.0f ? wl.ms_device : 0.0f;
    g.docs.insert(g.docs.end(), wl.docs.begin(), wl.docs.end());
    for (uint32_t i = 0; i < n; i++) g.off.push_back(base + wl.hit_off[i + 1]);
    return TFIDF_OK;
  }
  // the scored routes: once with a guessed payload size, once more with the size the route reports
  std::vector<uint64_t> hoff((size_t)n + 1, 0);
  std::vector<uint32_t> n_exp(n ? n : 1, 0), freqs;
  uint64_t total = 0, guess = std::min<uint64_t>(256ull * n + 4096, 1ull << 24);
  int rc = TFIDF_OK;
  for (int attempt = 0; attempt < 2; attempt++) {
    g.docs.resize(base + guess);
    g.scores.resize(base + guess);
    uint32_t *d = g.docs.data() + base;
    float *sc = g.scores.data() + base;
    if (g.kind == TFIDF_CLAUSE_TEXT) {
      rc = batch_all_on(ix, S, V, text, off.data(), n, d, sc, guess, hoff.data(), &total);
    } else if (g.kind == TFIDF_CLAUSE_PHRASE) {
      freqs.resize(guess ? guess : 1);
      rc = phrase_batch_on(ix, S, V, text, off.data(), slops.data(), n, d, sc, freqs.data(), guess, hoff.data(), &total);
    } else {
      rc = fuzzy_search_on(ix, S, V, text, off.data(), n, g.max_edits, g.prefix_len, g.max_exp, d, sc, guess,
                           hoff.data(), n_exp.data(), &total, nullptr);
    }
    *ms += route_total_ms(ix);
    if (rc != TFIDF_E_BUFFER) break;
    guess = total;
  }
  if (rc) {
    g.docs.resize(base);
    g.scores.resize(base);
    return rc;
  }
  g.docs.resize(base + total);
  g.scores.resize(base + total);
  for (uint32_t i = 0; i < n; i++) g.off.push_back(base + hoff[i + 1]);
  return TFIDF_OK;
}

// The rows of the call's clauses: the clauses grouped by kind, each group
// through its route in slices, a failed slice run again clause by clause to name
// the culprit as "query Q <unit> N:".  A nested call passes its nodes as
// clauses; a group node (TFIDF_CLAUSE_GROUP) has no route and an empty row.
// groups owns what rows points into.
static int cq_run_routes(tfidf_index *ix, Snapshot &S, StatsView &V, const uint8_t *c_utf8, const uint64_t *c_offsets,
                         const tfidf_clause *clauses, const uint64_t *q_coff, uint32_t n_q, const char *unit,
                         std::vector<std::unique_ptr<CqGroup>> &groups, std::vector<CqRow> *rows_out,
                         float *ms_routes_out) {
  const uint64_t n_c = n_q ? q_coff[n_q] : 0;
  // the groups: one per kind, the fuzzy clauses one per (max_edits, prefix_len, max_expansions)
  for (uint64_t c = 0; c < n_c; c++) {
    const tfidf_clause &cl = clauses[c];
    if (cl.kind == TFIDF_CLAUSE_GROUP) continue;
    const bool fz = cl.kind == TFIDF_CLAUSE_FUZZY;
    CqGroup *g = nullptr;
    for (auto &x : groups)
      if (x->kind == cl.kind &&
          (!fz || (x->max_edits == cl.max_edits && x->prefix_len == cl.prefix_len && x->max_exp == cl.max_expansions)))
        g = x.get();
    if (!g) {
      groups.emplace_back(new CqGroup());
      g = groups.back().get();
      g->kind = cl.kind;
      if (fz) { g->max_edits = cl.max_edits; g->prefix_len = cl.prefix_len; g->max_exp = cl.max_expansions; }
    }
    g->clause.push_back((uint32_t)c);
  }
  auto query_of = [&](uint32_t c) {
    return (uint32_t)(std::upper_bound(q_coff, q_coff + n_q + 1, (uint64_t)c) - q_coff - 1);
  };
  float ms_routes = 0.0f;
  const size_t kSlice = std::min<size_t>(kWcMaxPatterns, kFzMaxTerms);
  for (auto &gp : groups) {
    CqGroup &g = *gp;
    for (size_t a = 0; a < g.clause.size(); a += kSlice) {
      const size_t z = std::min(g.clause.size(), a + kSlice);
      const int rc = cq_run_slice(ix, S, V, c_utf8, c_offsets, clauses, g, a, z, &ms_routes);
      if (rc == TFIDF_OK) continue;
      // the route failed the whole slice: find the first clause it fails alone, and name it
      const std::string why = g_err;
      for (size_t i = a; i < z; i++) {
        CqGroup one;
        one.kind = g.kind;
        one.max_edits = g.max_edits;
        one.prefix_len = g.prefix_len;
        one.max_exp = g.max_exp;
        one.clause.push_back(g.clause[i]);
        float ms1 = 0.0f;
        if (cq_run_slice(ix, S, V, c_utf8, c_offsets, clauses, one, 0, 1, &ms1) == rc) {
          const uint32_t q = query_of(g.clause[i]);
          const std::string w1 = g_err;
          return fail(rc, "query %u %s %u: %s", q, unit, (uint32_t)(g.clause[i] - q_coff[q]), w1.c_str());
        }
      }
      return fail(rc, "a %s of kind %u: %s", unit, g.kind, why.c_str());
    }
  }
  std::vector<CqRow> &rows = *rows_out;
  rows.assign(n_c, CqRow());
  for (auto &gp : groups)
    for (size_t i = 0; i < gp->clause.size(); i++) {
      CqRow &r = rows[gp->clause[i]];
      r.n = gp->off[i + 1] - gp->off[i];
      r.docs = gp->docs.data() + gp->off[i];
      r.scores = gp->scores.empty() ? nullptr : gp->scores.data() + gp->off[i];
    }
  *ms_routes_out = ms_routes;
  return TFIDF_OK;
}

// nodes: NULL for the flat call; else the nested call's trees, clauses holding every node's occur, kind and
// parameters (q_coff then counts nodes)
static int compound_on(tfidf_index *ix, Snapshot &S, StatsView &V, const uint8_t *c_utf8, const uint64_t *c_offsets,
                       const tfidf_clause *clauses, const tfidf_qnode *nodes, const uint64_t *q_coff, uint32_t n_q,
                       uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out,
                       float *ms_device) {
  const uint64_t n_c = n_q ? q_coff[n_q] : 0;
  std::vector<std::unique_ptr<CqGroup>> groups;
  std::vector<CqRow> rows;
  float ms_routes = 0.0f;
  if (int rc = cq_run_routes(ix, S, V, c_utf8, c_offsets, clauses, q_coff, n_q, nodes ? "node" : "clause", groups,
                             &rows, &ms_routes))
    return rc;

  for (uint32_t i = 0; i <= n_q; i++) hit_offsets[i] = 0;
  *n_out = 0;
  if (ms_device) *ms_device = 0.0f;
  uint64_t st_entries = 0, st_chunks = 0, st_pairs = 0;
  float ms_combine = 0.0f;
  auto report = [&]() {
    std::lock_guard<std::mutex> lk(ix->ms_mu);
    ix->last_cq_entries = st_entries;
    ix->last_cq_chunks = st_chunks;
    ix->last_cq_pairs = st_pairs;
    ix->last_cq_ms = ms_combine;
    set_route_ms_locked(ix, ms_combine, ms_routes + ms_combine);
  };
  if (n_q == 0 || S.n_docs == 0) {
    report();
    return TFIDF_OK;
  }

  const uint32_t R = S.n_blocks, R2 = hits_runs_per_query(R);
  std::vector<uint64_t> q_entries(n_q, 0), row_n(n_c, 0);
  for (uint64_t c = 0; c < n_c; c++) row_n[c] = rows[c].n;
  for (uint32_t q = 0; q < n_q; q++)
    for (uint64_t c = q_coff[q]; c < q_coff[q + 1]; c++) q_entries[q] += rows[c].n;
  uint64_t budget = kCqEntryBudget;
  if (const char *e = knob("TFIDF_COMPOUND_CHUNK")) budget = (uint64_t)std::max<long long>(1, atoll(e));
  // the gapped runs of a chunk stay in the all-hits budget, its run and pair indices in 31 bits, its bins in 2^22
  const uint64_t max_q = std::max<uint64_t>(
      1, std::min<uint64_t>(kAllHitsBudget / ((uint64_t)R2 * kBlockDocs * 8), (1u << 30) / R2));
  const uint64_t max_c = std::max<uint64_t>(kCqMaxClausesPerQuery, (1ull << 22) / R);
  std::vector<uint64_t> cuts;
  cq_plan_chunks(q_entries.data(), q_coff, n_q, budget, max_q, max_c, &cuts);

  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();
  DeviceGuard dg(ix->cfg.device);
  std::vector<uint2> h_rows;
  std::vector<uint64_t> h_coff, qoff_h;
  std::vector<uint32_t> h_occ, h_qc, h_tree;         // h_tree, nested only: the nodes' parents, then their min_should_match
  uint64_t total = 0;
  bool fits = true;
  for (size_t k = 0; k + 1 < cuts.size(); k++) {
    const uint32_t a = (uint32_t)cuts[k], z = (uint32_t)cuts[k + 1], nq = z - a;
    const uint64_t c_lo = q_coff[a], c_hi = q_coff[z];
    const uint32_t nc = (uint32_t)(c_hi - c_lo);
    uint64_t n_e = 0, bound = 0;
    uint32_t levels = 1;                               // nested: the most groups a query of the chunk has open at once
    for (uint32_t q = a; q < z; q++) {
      n_e += q_entries[q];
      const uint64_t c0 = q_coff[q], n = q_coff[q + 1] - c0;
      bound += nodes ? cqn_hit_bound(nodes + c0, row_n.data() + c0, (uint32_t)n, S.n_docs)
                     : cq_hit_bound(clauses + c0, row_n.data() + c0, n, S.n_docs);
      if (nodes) levels = std::max(levels, cqn_levels(nodes + c0, (uint32_t)n));
    }
    st_chunks++;
    st_entries += n_e;
    st_pairs += (uint64_t)nq * R;
    if (n_e == 0 || bound == 0) {                      // no hit in the chunk
      for (uint32_t i = 1; i <= nq; i++) hit_offsets[a + i] = total;
      continue;
    }
    h_rows.resize(n_e);
    h_coff.assign((size_t)nc + 1, 0);
    h_occ.resize(nc);
    h_qc.resize((size_t)nq + 1);
    if (nodes) h_tree.resize((size_t)nc * 2);
    uint64_t at = 0;
    for (uint32_t c = 0; c < nc; c++) {
      const CqRow &r = rows[c_lo + c];
      for (uint64_t i = 0; i < r.n; i++)
        h_rows[at++] = make_uint2(r.docs[i], r.scores ? cq_float_bits(r.scores[i]) : 0x3F800000u);
      h_coff[c + 1] = at;
      h_occ[c] = clauses[c_lo + c].occur | (clauses[c_lo + c].kind == TFIDF_CLAUSE_GROUP ? 0x100u : 0u);
      if (nodes) {
        h_tree[c] = nodes[c_lo + c].parent;
        h_tree[(size_t)nc + c] = nodes[c_lo + c].min_should_match;
      }
    }
    for (uint32_t i = 0; i <= nq; i++) h_qc[i] = (uint32_t)(q_coff[a + i] - c_lo);
    const uint64_t n_bins = (uint64_t)nc * R;
    const size_t runs = (size_t)nq * R2;
    const size_t in_coff = 0, in_occ = ((size_t)nc + 1) * 8, in_qc = in_occ + (((size_t)nc * 4 + 7) & ~(size_t)7),
                 in_tree = (in_qc + ((size_t)nq + 1) * 4 + 7) & ~(size_t)7,
                 in_bytes = in_tree + (nodes ? (size_t)nc * 8 : 0);
    HIP_TRY(X.cq_in.reserve(in_bytes));
    HIP_TRY(X.cq_rows.reserve(n_e * 8));
    HIP_TRY(X.cq_binned.reserve(n_e * 8));
    HIP_TRY(X.cq_bins.reserve(2 * (n_bins + 1) * 8));
    HIP_TRY(X.hits.reserve(runs * kBlockDocs * 8));
    HIP_TRY(X.hits_n.reserve(runs * 4));
    HIP_TRY(X.hits_c.reserve(bound * 8 + 8));
    HIP_TRY(X.hits_s.reserve(bound * 8 + 8));
    HIP_TRY(X.hits_P.reserve((runs + 1 + nq + 1) * 8));
    HIP_TRY(X.out_doc.reserve(bound * 4 + 4));
    HIP_TRY(X.out_score.reserve(bound * 4 + 4));
    uint8_t *d_in = X.cq_in.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(d_in + in_coff, h_coff.data(), ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_in + in_occ, h_occ.data(), (size_t)nc * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_in + in_qc, h_qc.data(), ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, s));
    if (nodes) HIP_TRY(hipMemcpyAsync(d_in + in_tree, h_tree.data(), (size_t)nc * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(X.cq_rows.p, h_rows.data(), n_e * 8, hipMemcpyHostToDevice, s));
    CqPass p{};
    if (nodes) {
      p.c_parent = reinterpret_cast<const uint32_t *>(d_in + in_tree);
      p.c_msm = p.c_parent + nc;
      p.levels = levels;
    }
    p.rows = X.cq_rows.as<uint2>();
    p.c_off = reinterpret_cast<const uint64_t *>(d_in + in_coff);
    p.c_occur = reinterpret_cast<const uint32_t *>(d_in + in_occ);
    p.q_coff = reinterpret_cast<const uint32_t *>(d_in + in_qc);
    p.bin_cnt = X.cq_bins.as<uint64_t>();
    p.bin_off = p.bin_cnt + n_bins + 1;
    p.binned = X.cq_binned.as<uint2>();
    p.hits = X.hits.as<uint64_t>();
    p.hits_n = X.hits_n.as<uint32_t>();
    p.n_e = n_e;
    p.n_c = nc;
    p.n_q = nq;
    p.n_blocks = R;
    p.R2 = R2;
    p.n_docs = (uint32_t)S.n_docs;
    HIP_TRY(hipEventRecord(X.ev[QEV_P0], s));
    HIP_TRY(launch_compound_pass(p, ix->num_cus * 8, s));
    uint64_t *d_qoff = X.hits_P.as<uint64_t>() + runs + 1;
    HIP_TRY(launch_hits_order_batch(X.hits.as<uint64_t>(), X.hits_n.as<uint32_t>(), nq, R, X.hits_P.as<uint64_t>(),
                                    X.hits_c.as<uint64_t>(), X.hits_s.as<uint64_t>(), X.out_doc.as<uint32_t>(),
                                    X.out_score.as<float>(), d_qoff, nullptr, 0, bound, ix->num_cus * 4, s));
    HIP_TRY(hipEventRecord(X.ev[QEV_P1], s));
    qoff_h.resize((size_t)nq + 1);
    HIP_TRY(hipMemcpyAsync(qoff_h.data(), d_qoff, ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, X.ev[QEV_P0], X.ev[QEV_P1]));
    ms_combine += ms;
    const uint64_t H = qoff_h[nq];
    for (uint32_t i = 1; i <= nq; i++) hit_offsets[a + i] = total + qoff_h[i];
    fits = fits && total + H <= cap;
    if (fits && H) {
      HIP_TRY(hipMemcpyAsync(doc_ids + total, X.out_doc.p, H * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipMemcpyAsync(scores + total, X.out_score.p, H * 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
    }
    total += H;
  }
  *n_out = total;
  if (ms_device) *ms_device = ms_routes + ms_combine;
  report();
  if (!fits) return fail(TFIDF_E_BUFFER, "need %llu result slots", (unsigned long long)total);
  return TFIDF_OK;
}

static int compound_check(const void *h, const uint8_t *c_utf8, const uint64_t *c_offsets, const tfidf_clause *clauses,
                          const uint64_t *q_coff, uint32_t n_q, const uint32_t *doc_ids, const float *scores,
                          uint64_t cap, const uint64_t *hit_offsets, const uint64_t *n_out) {
  if (!h || !hit_offsets || !n_out || (n_q && !q_coff) || (cap && (!doc_ids || !scores)))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (n_q && n_q <= kCqMaxQueries && q_coff[n_q] && (!clauses || !c_offsets))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  uint64_t at = 0;
  switch (cq_check_args(c_offsets, clauses, q_coff, n_q, &at)) {
    case kCqOk:
      if (n_q && q_coff[n_q] && !c_utf8 && c_offsets[q_coff[n_q]]) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
      return TFIDF_OK;
    case kCqTooManyQueries: return fail(TFIDF_E_INVALID_ARG, "more than %u queries in one call", kCqMaxQueries);
    case kCqBadQueryOffsets: return fail(TFIDF_E_INVALID_ARG, "q_clause_offsets do not start at 0 or decrease at query %llu", (unsigned long long)at);
    case kCqTooManyInQuery: return fail(TFIDF_E_INVALID_ARG, "query %llu has more than %u clauses", (unsigned long long)at, kCqMaxClausesPerQuery);
    case kCqTooManyClauses: return fail(TFIDF_E_INVALID_ARG, "more than 2^20 clauses in one call");
    case kCqBadPayloadOffsets: return fail(TFIDF_E_INVALID_ARG, "c_offsets do not start at 0 or decrease at clause %llu", (unsigned long long)at);
    case kCqBadOccur: return fail(TFIDF_E_INVALID_ARG, "clause %llu: unknown occur", (unsigned long long)at);
    default: return fail(TFIDF_E_INVALID_ARG, "clause %llu: unknown kind", (unsigned long long)at);
  }
}

extern "C" int tfidf_search_compound_batch(tfidf_index *ix, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                           const tfidf_clause *clauses, const uint64_t *q_clause_offsets, uint32_t n_q,
                                           uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                           uint64_t *n_out, float *ms_device) {
  if (int rc = compound_check(ix, c_utf8, c_offsets, clauses, q_clause_offsets, n_q, doc_ids, scores, cap, hit_offsets,
                              n_out))
    return rc;
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "compound search before commit");
  return compound_on(ix, *snap, *view, c_utf8, c_offsets, clauses, nullptr, q_clause_offsets, n_q, doc_ids, scores,
                     cap, hit_offsets, n_out, ms_device);
}

extern "C" int tfidf_reader_search_compound_batch(tfidf_reader *rd, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                                  const tfidf_clause *clauses, const uint64_t *q_clause_offsets,
                                                  uint32_t n_q, uint32_t *doc_ids, float *scores, uint64_t cap,
                                                  uint64_t *hit_offsets, uint64_t *n_out, float *ms_device) {
  if (int rc = compound_check(rd, c_utf8, c_offsets, clauses, q_clause_offsets, n_q, doc_ids, scores, cap, hit_offsets,
                              n_out))
    return rc;
  return compound_on(rd->ix, *rd->S, *rd->V, c_utf8, c_offsets, clauses, nullptr, q_clause_offsets, n_q, doc_ids,
                     scores, cap, hit_offsets, n_out, ms_device);
}

// the single forms: the batch of one query
extern "C" int tfidf_search_compound(tfidf_index *ix, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                     const tfidf_clause *clauses, uint32_t n_clauses, uint32_t *doc_ids, float *scores,
                                     uint64_t cap, uint64_t *n_out, float *ms_device) {
  if (!n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t qo[2] = {0, n_clauses};
  uint64_t ho[2];
  return tfidf_search_compound_batch(ix, c_utf8, c_offsets, clauses, qo, 1, doc_ids, scores, cap, ho, n_out, ms_device);
}

extern "C" int tfidf_reader_search_compound(tfidf_reader *rd, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                            const tfidf_clause *clauses, uint32_t n_clauses, uint32_t *doc_ids,
                                            float *scores, uint64_t cap, uint64_t *n_out, float *ms_device) {
  if (!n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t qo[2] = {0, n_clauses};
  uint64_t ho[2];
  return tfidf_reader_search_compound_batch(rd, c_utf8, c_offsets, clauses, qo, 1, doc_ids, scores, cap, ho, n_out,
                                            ms_device);
}

// nested compound queries ("Nested compound queries"; rules in compound_tree_plan.h): the
// flat call's path with the nodes as its clauses, a group node's row empty, and k_cqn_combine as the combine
static int nested_check(const void *h, const uint8_t *c_utf8, const uint64_t *c_offsets, const tfidf_qnode *nodes,
                        const uint64_t *q_noff, uint32_t n_q, const uint32_t *doc_ids, const float *scores,
                        uint64_t cap, const uint64_t *hit_offsets, const uint64_t *n_out) {
  if (!h || !hit_offsets || !n_out || (n_q && !q_noff) || (cap && (!doc_ids || !scores)))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (n_q && n_q <= kCqMaxQueries && q_noff[n_q] && (!nodes || !c_offsets))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  uint64_t q = 0, i = 0;
  const char *why = nullptr;
  switch (cqn_check_args(c_offsets, nodes, q_noff, n_q, &q, &i)) {
    case kCqnOk:
      if (n_q && q_noff[n_q] && !c_utf8 && c_offsets[q_noff[n_q]]) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
      return TFIDF_OK;
    case kCqnTooManyQueries: return fail(TFIDF_E_INVALID_ARG, "more than %u queries in one call", kCqMaxQueries);
    case kCqnBadQueryOffsets: return fail(TFIDF_E_INVALID_ARG, "q_node_offsets do not start at 0 or decrease at query %llu", (unsigned long long)q);
    case kCqnTooManyInQuery: return fail(TFIDF_E_INVALID_ARG, "query %llu has more than %u nodes", (unsigned long long)q, kCqnMaxNodes);
    case kCqnTooManyNodes: return fail(TFIDF_E_INVALID_ARG, "more than 2^20 nodes in one call");
    case kCqnBadPayloadOffsets: why = "c_offsets do not start at 0 or decrease"; break;
    case kCqnBadOccur: why = "unknown occur"; break;
    case kCqnBadKind: why = "unknown kind"; break;
    case kCqnBadRoot: why = "node 0 is not a group, or has a parent"; break;
    case kCqnBadParent: why = "the parent is not an earlier group that is the node before or one of its ancestors"; break;
    case kCqnGroupPayload: why = "a group with a payload"; break;
    default: why = "a group deeper than 3 or a leaf deeper than 4"; break;
  }
  return fail(TFIDF_E_INVALID_ARG, "query %llu node %llu: %s", (unsigned long long)q, (unsigned long long)i, why);
}

static int nested_on(tfidf_index *ix, Snapshot &S, StatsView &V, const uint8_t *c_utf8, const uint64_t *c_offsets,
                     const tfidf_qnode *nodes, const uint64_t *q_noff, uint32_t n_q, uint32_t *doc_ids, float *scores,
                     uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out, float *ms_device) {
  const uint64_t n_n = n_q ? q_noff[n_q] : 0;
  std::vector<tfidf_clause> cl(n_n ? n_n : 1);
  for (uint64_t i = 0; i < n_n; i++)
    cl[i] = tfidf_clause{nodes[i].occur, nodes[i].kind, nodes[i].max_edits, nodes[i].max_expansions,
                         nodes[i].prefix_len, nodes[i].slop};
  return compound_on(ix, S, V, c_utf8, c_offsets, cl.data(), nodes, q_noff, n_q, doc_ids, scores, cap, hit_offsets,
                     n_out, ms_device);
}

extern "C" int tfidf_search_nested_batch(tfidf_index *ix, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                         const tfidf_qnode *nodes, const uint64_t *q_node_offsets, uint32_t n_q,
                                         uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                         uint64_t *n_out, float *ms_device) {
  if (int rc = nested_check(ix, c_utf8, c_offsets, nodes, q_node_offsets, n_q, doc_ids, scores, cap, hit_offsets, n_out))
    return rc;
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "nested search before commit");
  return nested_on(ix, *snap, *view, c_utf8, c_offsets, nodes, q_node_offsets, n_q, doc_ids, scores, cap, hit_offsets,
                   n_out, ms_device);
}

extern "C" int tfidf_reader_search_nested_batch(tfidf_reader *rd, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                                const tfidf_qnode *nodes, const uint64_t *q_node_offsets, uint32_t n_q,
                                                uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                                uint64_t *n_out, float *ms_device) {
  if (int rc = nested_check(rd, c_utf8, c_offsets, nodes, q_node_offsets, n_q, doc_ids, scores, cap, hit_offsets, n_out))
    return rc;
  return nested_on(rd->ix, *rd->S, *rd->V, c_utf8, c_offsets, nodes, q_node_offsets, n_q, doc_ids, scores, cap,
                   hit_offsets, n_out, ms_device);
}

// the single forms: the batch of one query
extern "C" int tfidf_search_nested(tfidf_index *ix, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                   const tfidf_qnode *nodes, uint32_t n_nodes, uint32_t *doc_ids, float *scores,
                                   uint64_t cap, uint64_t *n_out, float *ms_device) {
  if (!n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t qo[2] = {0, n_nodes};
  uint64_t ho[2];
  return tfidf_search_nested_batch(ix, c_utf8, c_offsets, nodes, qo, 1, doc_ids, scores, cap, ho, n_out, ms_device);
}

extern "C" int tfidf_reader_search_nested(tfidf_reader *rd, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                          const tfidf_qnode *nodes, uint32_t n_nodes, uint32_t *doc_ids, float *scores,
                                          uint64_t cap, uint64_t *n_out, float *ms_device) {
  if (!n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const uint64_t qo[2] = {0, n_nodes};
  uint64_t ho[2];
  return tfidf_reader_search_nested_batch(rd, c_utf8, c_offsets, nodes, qo, 1, doc_ids, scores, cap, ho, n_out,
                                          ms_device);
}

extern "C" int tfidf_last_compound_stats(const tfidf_index *ix, uint64_t *row_entries, uint64_t *chunks,
                                         uint64_t *pairs) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->ms_mu);
  if (row_entries) *row_entries = ix->last_cq_entries;
  if (chunks) *chunks = ix->last_cq_chunks;
  if (pairs) *pairs = ix->last_cq_pairs;
  return TFIDF_OK;
}

extern "C" int tfidf_last_compound_ms(const tfidf_index *ix, float *ms_combine) {
  if (!ix || !ms_combine) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->ms_mu);
  *ms_combine = ix->last_cq_ms;
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// more-like-this ("More like this"; rules in mlt_plan.h).
// The seeds' forward rows are scanned on the device (kernels_mlt.hip): count
// the candidates per seed, fill (key, value) pairs by candidate chunks, sort,
// select each seed's first max_terms and their score ties.  Only those (slot,
// tf) pairs come to the host, where the strings are materialised (exact keys
// from the mirror, hashed ones from their reference occurrence) and the bytes
// break the ties.  The seeds' queries are built from the slots and go through
// the batched top-k scorer like any search batch.

// the snapshot's idf table on the device, built and uploaded by the first call that needs it
static int mlt_table(Snapshot &S, hipStream_t s, const float **d_idf) {
  std::lock_guard<std::mutex> lk(S.mlt_mu);
  if (!S.mlt_ready) {
    mlt_idf_table(S.n_docs, &S.h_mlt_idf);
    HIP_TRY(S.mlt_idf.reserve(S.h_mlt_idf.size() * 4));
    HIP_TRY(hipMemcpyAsync(S.mlt_idf.p, S.h_mlt_idf.data(), S.h_mlt_idf.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    S.mlt_ready = true;
  }
  *d_idf = S.mlt_idf.as<float>();
  return TFIDF_OK;
}

static int mlt_rules(const tfidf_mlt_params *p, MltRules *r) {
  tfidf_mlt_params d;
  tfidf_mlt_params_init(&d);
  if (p) d = *p;
  if (d.max_terms < 1 || d.max_terms > kMltMaxTerms)
    return fail(TFIDF_E_INVALID_ARG, "max_terms %u outside 1..%u", d.max_terms, kMltMaxTerms);
  *r = MltRules{d.min_tf ? d.min_tf : 1u, d.min_df, d.max_df, d.max_terms};
  return TFIDF_OK;
}

static int mlt_check_seeds(const Snapshot &S, const uint32_t *seeds, uint32_t n) {
  if (n > kMltMaxSeeds) return fail(TFIDF_E_INVALID_ARG, "more than %u seeds in one call", kMltMaxSeeds);
  if (n && !seeds) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  for (uint32_t i = 0; i < n; i++)
    if (seeds[i] >= S.n_docs)
      return fail(TFIDF_E_INVALID_ARG, "seed %u (doc %u) out of range: %llu documents", i, seeds[i],
                  (unsigned long long)S.n_docs);
  return TFIDF_OK;
}

// interesting terms of checked seeds, on the caller's search context
static int mlt_terms_on(tfidf_index *ix, Snapshot &S, SearchCtx &X, hipStream_t s, const uint32_t *seeds, uint32_t n,
                        const MltRules &R, MltLists *out) {
  out->terms.assign(n, {});
  out->n_cand.assign(n, 0);
  uint64_t n_entries = 0, n_fill = 0;
  auto publish = [&]() {
    std::lock_guard<std::mutex> lk(ix->ms_mu);
    ix->last_mlt_entries = n_entries;
    ix->last_mlt_chunks = n_fill;
  };
  if (n == 0 || S.n_docs == 0) { publish(); return TFIDF_OK; }
  const float *d_idf = nullptr;
  if (int rc = mlt_table(S, s, &d_idf)) return rc;
  const uint64_t budget = std::min<uint64_t>(hl_budget("TFIDF_MLT_CAND_BUDGET", kMltCandBudget), 1ull << 30);
  const int max_grid = ix->num_cus * 8;

  // staged seeds and counters: row_base u64[n], row_off u64[n + 1], then u32: doc[n], staged[n], counts[n],
  // seg and out_off [n + 1] each, take[n], the fill cursor
  const size_t in_off = (size_t)n * 8, in_doc = in_off + ((size_t)n + 1) * 8, in_st = in_doc + (size_t)n * 4,
               in_cnt = in_st + (size_t)n * 4, in_seg = in_cnt + (size_t)n * 4, in_oo = in_seg + ((size_t)n + 1) * 4,
               in_take = in_oo + ((size_t)n + 1) * 4, in_cur = in_take + (size_t)n * 4, in_end = in_cur + 8;
  HIP_TRY(X.ml_in.reserve(in_end));
  uint8_t *ib = X.ml_in.as<uint8_t>();
  uint64_t *d_base = reinterpret_cast<uint64_t *>(ib), *d_off = reinterpret_cast<uint64_t *>(ib + in_off);
  uint32_t *d_doc = reinterpret_cast<uint32_t *>(ib + in_doc), *d_st = reinterpret_cast<uint32_t *>(ib + in_st),
           *d_cnt = reinterpret_cast<uint32_t *>(ib + in_cnt), *d_seg = reinterpret_cast<uint32_t *>(ib + in_seg),
           *d_oo = reinterpret_cast<uint32_t *>(ib + in_oo), *d_take = reinterpret_cast<uint32_t *>(ib + in_take),
           *d_cur = reinterpret_cast<uint32_t *>(ib + in_cur);
  std::vector<uint32_t> h_in((size_t)2 * n);
  for (uint32_t i = 0; i < n; i++) {
    h_in[i] = seeds[i];
    h_in[(size_t)n + i] = (uint32_t)S.staged_of(seeds[i]);
  }
  HIP_TRY(hipMemcpyAsync(d_doc, h_in.data(), (size_t)2 * n * 4, hipMemcpyHostToDevice, s));   // doc[n] | staged[n]
  HIP_TRY(hipMemsetAsync(d_cnt, 0, (size_t)n * 4, s));
  HIP_TRY(launch_mlt_extents(S.offsets->as<uint64_t>(), S.doc_nuniq.as<uint32_t>(), d_doc, d_st, n, d_base, d_off, s));
  HIP_TRY(exclusive_scan_u64(d_off, d_off, n, s));

  MltScan a{};
  a.csr = S.csr.as<uint32_t>();
  a.csr_words = S.csr.bytes / 4;
  a.rsplit = S.rsplit.as<uint32_t>();
  a.R = S.R;
  a.range_shift = S.range_shift;
  a.C = S.C;
  a.csr_esc = S.csr_esc.as<uint64_t>();
  a.n_esc = S.h_esc.size();
  a.df = S.df_dev();
  a.idf = d_idf;
  a.n_docs = S.n_docs;
  a.seed_doc = d_doc;
  a.row_base = d_base;
  a.row_off = d_off;
  a.s0 = 0;
  a.s1 = n;
  a.min_tf = R.min_tf;
  a.min_df = R.min_df;
  a.max_df = R.max_df;
  a.counts = d_cnt;
  a.cursor = d_cur;
  // the rows' lengths are not known here yet: a grid for ~1024 entries per seed, the kernel strides over the rest
  HIP_TRY(launch_mlt_scan(false, a, std::max<uint64_t>((uint64_t)n * 1024, 16384), max_grid, s));
  std::vector<uint32_t> counts(n), seg, take, oo;
  std::vector<uint64_t> h_off((size_t)n + 1), cuts, h_keys, h_vals;
  HIP_TRY(hipMemcpyAsync(counts.data(), d_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(h_off.data(), d_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  n_entries = h_off[n];
  for (uint32_t i = 0; i < n; i++) out->n_cand[i] = counts[i];

  mlt_plan_chunks(counts.data(), 0, n, budget, &cuts);
  std::string ts;
  for (size_t ci = 0; ci + 1 < cuts.size(); ci++) {
    const uint64_t a0 = cuts[ci], na = cuts[ci + 1] - a0;
    seg.assign(na + 1, 0);
    uint64_t T = 0;
    for (uint64_t t = 0; t < na; t++) {
      T += counts[a0 + t];
      if (T >= (1ull << 31)) return fail(TFIDF_E_INVALID_ARG, "more than 2^31 candidates for one seed range");
      seg[t + 1] = (uint32_t)T;
    }
    if (T == 0) continue;
    n_fill++;
    // candidates: keys [T] x 2 (sort in / out), values [T] x 2
    HIP_TRY(X.ml_c.reserve((size_t)T * 32));
    uint64_t *k_in = X.ml_c.as<uint64_t>(), *k_out = k_in + T, *v_in = k_out + T, *v_out = v_in + T;
    HIP_TRY(hipMemsetAsync(d_cur, 0, 4, s));
    MltScan f = a;
    f.s0 = (uint32_t)a0;
    f.s1 = (uint32_t)(a0 + na);
    f.keys = k_in;
    f.vals = v_in;
    f.cap = (uint32_t)T;
    HIP_TRY(launch_mlt_scan(true, f, h_off[a0 + na] - h_off[a0], max_grid, s));
    const int end_bit = mlt_key_bits((uint32_t)na);
    size_t tmp_bytes = 0;
    HIP_TRY(mlt_sort(nullptr, &tmp_bytes, k_in, k_out, v_in, v_out, (uint32_t)T, end_bit, s));
    HIP_TRY(X.ml_tmp.reserve(tmp_bytes));
    tmp_bytes = X.ml_tmp.bytes;
    HIP_TRY(mlt_sort(X.ml_tmp.p, &tmp_bytes, k_in, k_out, v_in, v_out, (uint32_t)T, end_bit, s));
    // what the host orders: the selection, packed into the sort's input buffers
    take.resize(na);
    HIP_TRY(hipMemcpyAsync(d_seg, seg.data(), (na + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_mlt_select(k_out, d_seg, (uint32_t)na, R.max_terms, d_take, s));
    HIP_TRY(hipMemcpyAsync(take.data(), d_take, na * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    oo.assign(na + 1, 0);
    uint64_t n_take = 0;
    for (uint64_t t = 0; t < na; t++) {
      if (take[t] > seg[t + 1] - seg[t]) return fail(TFIDF_E_STATE, "more-like-this selection past its segment");
      oo[t] = (uint32_t)n_take;
      n_take += take[t];
    }
    oo[na] = (uint32_t)n_take;
    HIP_TRY(hipMemcpyAsync(d_oo, oo.data(), (na + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_mlt_gather(k_out, v_out, d_seg, d_oo, (uint32_t)na, k_in, v_in, s));
    h_keys.resize(n_take);
    h_vals.resize(n_take);
    HIP_TRY(hipMemcpyAsync(h_keys.data(), k_in, n_take * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_vals.data(), v_in, n_take * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint64_t t = 0; t < na; t++) {
      std::vector<MltTerm> &L = out->terms[a0 + t];
      L.reserve(oo[t + 1] - oo[t]);
      for (uint32_t i = oo[t]; i < oo[t + 1]; i++) {
        const uint32_t slot = mlt_val_slot(h_vals[i]), tf = mlt_val_tf(h_vals[i]);
        if (mlt_key_seed(h_keys[i]) != t || slot >= S.C)
          return fail(TFIDF_E_STATE, "more-like-this candidate %u of seed %llu is out of place", i,
                      (unsigned long long)(a0 + t));
        const uint32_t df = S.h_df[slot];
        const float score = mlt_score(tf, S.h_mlt_idf[std::min<uint64_t>(df, S.n_docs)]);
        if (mlt_float_bits(score) != mlt_key_score_bits(h_keys[i]))
          return fail(TFIDF_E_STATE, "more-like-this score of slot %u differs between device and host", slot);
        if (int rc = slot_term(S, slot, &ts)) return rc;
        L.push_back(MltTerm{ts, slot, tf, df, score});
      }
      std::sort(L.begin(), L.end(), [](const MltTerm &x, const MltTerm &y) {
        const uint32_t bx = mlt_float_bits(x.score), by = mlt_float_bits(y.score);
        if (bx != by) return bx > by;
        return x.term < y.term;
      });
      if (L.size() > R.max_terms) L.resize(R.max_terms);
    }
  }
  publish();
  return TFIDF_OK;
}

// Top kk of each prepared query on the caller's search context, in chunks
// whose candidate buffers stay near 1 GiB: docs / scores [n * kk], counts [n].
static int score_prepared(tfidf_index *ix, Snapshot &S, StatsView &V, SearchCtx &X, hipStream_t s,
                          const std::vector<PreparedQuery> &pqs, uint32_t kk, uint32_t *docs, float *scores,
                          uint32_t *counts, bool *any_out) {
  const uint32_t n = (uint32_t)pqs.size();
  *any_out = false;
  memset(counts, 0, (size_t)n * 4);
  if (n == 0 || S.n_docs == 0) return TFIDF_OK;
  const uint64_t per_q = (uint64_t)std::max(1u, S.n_blocks) * kk * 8;
  const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, (1ull << 30) / per_q));
  HIP_TRY(X.q_res.resize((size_t)2 * n * kk + n));
  std::vector<uint8_t> ran((n + chunk - 1) / chunk, 0);
  for (uint32_t c0 = 0, ci = 0; c0 < n; c0 += chunk, ci++) {
    const uint32_t nc = std::min(chunk, n - c0);
    QueryBatch qb;
    for (uint32_t i = 0; i < nc; i++) qb.add(pqs[c0 + i]);
    if (qb.slot.empty()) continue;
    X.q_rec_start = true;
    if (int rc = run_scoring(ix, S, V, X, s, qb, nc, kk)) return rc;
    uint32_t *hres = X.q_res.data() + (size_t)2 * c0 * kk + c0;
    HIP_TRY(hipMemcpyAsync(hres, X.res_doc, ((size_t)2 * nc * kk + nc) * 4, hipMemcpyDeviceToHost, s));
    ran[ci] = 1;
    *any_out = true;
  }
  HIP_TRY(hipStreamSynchronize(s));
  X.q_in_pending = false;
  for (uint32_t c0 = 0, ci = 0; c0 < n; c0 += chunk, ci++) {
    if (!ran[ci]) continue;
    const uint32_t nc = std::min(chunk, n - c0);
    const uint32_t *hres = X.q_res.data() + (size_t)2 * c0 * kk + c0;
    memcpy(docs + (size_t)c0 * kk, hres, (size_t)nc * kk * 4);
    memcpy(scores + (size_t)c0 * kk, hres + (size_t)nc * kk, (size_t)nc * kk * 4);
    memcpy(counts + c0, hres + (size_t)2 * nc * kk, (size_t)nc * 4);
  }
  return TFIDF_OK;
}

// one SHOULD clause of boost 1 for dictionary slot `slot` (prepare_query's weights)
static void add_should(const Snapshot &S, const StatsView &V, uint32_t slot, PreparedQuery *pq) {
  const uint64_t df = V.global ? V.gdf[slot] : S.h_df[slot];
  volatile float w = 1.0f * bm25_idf(df, V.doc_count);
  pq->slot.push_back(S.col_of(slot));
  pq->ldf.push_back(S.h_df[slot]);
  const float wv = w;
  pq->w.push_back(wv);
  pq->role.push_back(kRoleShould << 24);
}

static int mlt_terms_call(tfidf_index *ix, Snapshot &S, const uint32_t *seeds, uint32_t n, const MltRules &R,
                          MltLists *out) {
  if (int rc = mlt_check_seeds(S, seeds, n)) return rc;
  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();
  DeviceGuard g(ix->cfg.device);
  if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_P0], s));
  if (int rc = mlt_terms_on(ix, S, X, s, seeds, n, R, out)) return rc;
  if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_P1], s));
  HIP_TRY(hipStreamSynchronize(s));
  set_route_ms(ix, 0.0f, qev_ms(X, QEV_P0, QEV_P1));
  return TFIDF_OK;
}

int tfidf::index_mlt_terms(tfidf_index *ix, const uint32_t *seeds, uint32_t n, const MltRules &rules, MltLists *out) {
  if (!ix || !out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "more-like-this before commit");
  return mlt_terms_call(ix, *snap, seeds, n, rules, out);
}

int tfidf::index_search_term_lists(tfidf_index *ix, const std::vector<std::vector<std::string>> &lists, uint32_t k,
                                   uint32_t *doc_ids, float *scores, uint32_t *counts) {
  if (!ix || (lists.size() && (!doc_ids || !scores || !counts))) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (k == 0 || k > 1024) return fail(TFIDF_E_INVALID_ARG, "term-list search needs 1 <= k <= 1024");
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "search before commit");
  Snapshot &S = *snap;
  StatsView &V = *view;
  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  DeviceGuard g(ix->cfg.device);
  if (int e = V.wait_gdf()) return e;
  std::vector<PreparedQuery> pqs(lists.size());
  if (V.doc_count)
    for (size_t i = 0; i < lists.size(); i++)
      for (const std::string &t : lists[i]) {
        const uint32_t slot = lookup_term(S, t);
        if (slot != kInvalidSlot) add_should(S, V, slot, &pqs[i]);   // absent: no scorer
      }
  bool any = false;
  if (int rc = score_prepared(ix, S, V, *lease.c, lease.stream(), pqs, k, doc_ids, scores, counts, &any)) return rc;
  set_route_ms(ix, any ? qev_ms(*lease.c, QEV_0, QEV_1) : 0.0f, any ? qev_ms(*lease.c, QEV_0, QEV_2) : 0.0f);
  return TFIDF_OK;
}

static int mlt_terms_batch_on(tfidf_index *ix, Snapshot &S, const uint32_t *seeds, uint32_t n, const MltRules &R,
                              uint64_t *term_offsets, uint64_t *n_candidates,
                              uint64_t *blob_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *tf, uint32_t *df,
                              float *score, uint64_t term_cap, uint64_t *n_terms, uint64_t *n_term_bytes) {
  if (!term_offsets || (n && !n_candidates) || !n_terms || !n_term_bytes)
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  MltLists ml;
  if (int rc = mlt_terms_call(ix, S, seeds, n, R, &ml)) return rc;
  uint64_t nt = 0, nb = 0;
  term_offsets[0] = 0;
  for (uint32_t i = 0; i < n; i++) {
    n_candidates[i] = ml.n_cand[i];
    nt += ml.terms[i].size();
    for (const MltTerm &t : ml.terms[i]) nb += t.term.size();
    term_offsets[i + 1] = nt;
  }
  *n_terms = nt;
  *n_term_bytes = nb;
  if (nt > term_cap || nb > terms_cap || (nt && (!blob_offsets || !tf || !df || !score)) || (nb && !terms))
    return fail(TFIDF_E_BUFFER, "need %llu term slots and %llu term bytes", (unsigned long long)nt,
                (unsigned long long)nb);
  uint64_t at = 0, b = 0;
  if (blob_offsets) blob_offsets[0] = 0;
  for (uint32_t i = 0; i < n; i++)
    for (const MltTerm &t : ml.terms[i]) {
      memcpy(terms + b, t.term.data(), t.term.size());
      b += t.term.size();
      tf[at] = t.tf;
      df[at] = t.df;
      score[at] = t.score;
      blob_offsets[++at] = b;
    }
  return TFIDF_OK;
}

static int mlt_search_on(tfidf_index *ix, Snapshot &S, StatsView &V, const uint32_t *seeds, uint32_t n,
                         const MltRules &R, uint32_t k, uint32_t flags, uint32_t *doc_ids, float *scores,
                         uint32_t *counts) {
  const bool excl = (flags & TFIDF_MLT_EXCLUDE_SEED) != 0;
  if (flags & ~TFIDF_MLT_EXCLUDE_SEED) return fail(TFIDF_E_INVALID_ARG, "unknown flags 0x%x", flags);
  if (k == 0 || k > (excl ? 1023u : 1024u))
    return fail(TFIDF_E_INVALID_ARG, "more-like-this needs 1 <= k <= %u", excl ? 1023u : 1024u);
  if (n && (!doc_ids || !scores || !counts)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (int rc = mlt_check_seeds(S, seeds, n)) return rc;
  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();
  DeviceGuard g(ix->cfg.device);
  if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_P0], s));
  MltLists ml;
  if (int rc = mlt_terms_on(ix, S, X, s, seeds, n, R, &ml)) return rc;
  if (int e = V.wait_gdf()) return e;
  std::vector<PreparedQuery> pqs(n);
  if (V.doc_count)
    for (uint32_t i = 0; i < n; i++)
      for (const MltTerm &t : ml.terms[i]) add_should(S, V, t.slot, &pqs[i]);
  const uint32_t kk = excl ? k + 1 : k;
  std::vector<uint32_t> t_docs, t_cnt;
  std::vector<float> t_scores;
  uint32_t *pd = doc_ids, *pc = counts;
  float *ps = scores;
  if (excl) {
    t_docs.resize((size_t)n * kk);
    t_scores.resize((size_t)n * kk);
    t_cnt.resize(n);
    pd = t_docs.data();
    ps = t_scores.data();
    pc = t_cnt.data();
  }
  bool any = false;
  if (int rc = score_prepared(ix, S, V, X, s, pqs, kk, pd, ps, pc, &any)) return rc;
  if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_P1], s));
  HIP_TRY(hipStreamSynchronize(s));
  set_route_ms(ix, any ? qev_ms(X, QEV_0, QEV_2) : 0.0f, qev_ms(X, QEV_P0, QEV_P1));
  if (excl)
    for (uint32_t i = 0; i < n; i++) {   // the top k of the others: the seed dropped from the top k + 1
      uint32_t m = 0;
      for (uint32_t j = 0; j < pc[i] && m < k; j++) {
        if (pd[(size_t)i * kk + j] == seeds[i]) continue;
        doc_ids[(size_t)i * k + m] = pd[(size_t)i * kk + j];
        scores[(size_t)i * k + m] = ps[(size_t)i * kk + j];
        m++;
      }
      counts[i] = m;
    }
  return TFIDF_OK;
}

extern "C" int tfidf_mlt_params_init(tfidf_mlt_params *params) {
  if (!params) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  *params = tfidf_mlt_params{2, 5, 0, 25};   // MoreLikeThis.DEFAULT_MIN_TERM_FREQ / _MIN_DOC_FREQ / _MAX_DOC_FREQ / _MAX_QUERY_TERMS
  return TFIDF_OK;
}

extern "C" int tfidf_mlt_terms_batch(tfidf_index *ix, const uint32_t *seeds, uint32_t n, const tfidf_mlt_params *params,
                                     uint64_t *term_offsets, uint64_t *n_candidates, uint64_t *blob_offsets,
                                     uint8_t *terms, uint64_t terms_cap, uint32_t *tf, uint32_t *df, float *score,
                                     uint64_t term_cap, uint64_t *n_terms, uint64_t *n_term_bytes) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  MltRules R;
  if (int rc = mlt_rules(params, &R)) return rc;
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "more-like-this before commit");
  return mlt_terms_batch_on(ix, *snap, seeds, n, R, term_offsets, n_candidates, blob_offsets, terms, terms_cap, tf,
                            df, score, term_cap, n_terms, n_term_bytes);
}

extern "C" int tfidf_reader_mlt_terms_batch(tfidf_reader *rd, const uint32_t *seeds, uint32_t n,
                                            const tfidf_mlt_params *params, uint64_t *term_offsets,
                                            uint64_t *n_candidates, uint64_t *blob_offsets, uint8_t *terms,
                                            uint64_t terms_cap, uint32_t *tf, uint32_t *df, float *score,
                                            uint64_t term_cap, uint64_t *n_terms, uint64_t *n_term_bytes) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  MltRules R;
  if (int rc = mlt_rules(params, &R)) return rc;
  return mlt_terms_batch_on(rd->ix, *rd->S, seeds, n, R, term_offsets, n_candidates, blob_offsets, terms, terms_cap,
                            tf, df, score, term_cap, n_terms, n_term_bytes);
}

extern "C" int tfidf_more_like_this_batch(tfidf_index *ix, const uint32_t *seeds, uint32_t n,
                                          const tfidf_mlt_params *params, uint32_t k, uint32_t flags, uint32_t *doc_ids,
                                          float *scores, uint32_t *counts) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  MltRules R;
  if (int rc = mlt_rules(params, &R)) return rc;
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "more-like-this before commit");
  return mlt_search_on(ix, *snap, *view, seeds, n, R, k, flags, doc_ids, scores, counts);
}

extern "C" int tfidf_reader_more_like_this_batch(tfidf_reader *rd, const uint32_t *seeds, uint32_t n,
                                                 const tfidf_mlt_params *params, uint32_t k, uint32_t flags,
                                                 uint32_t *doc_ids, float *scores, uint32_t *counts) {
  if (!rd) return fail(TFIDF_E_INVALID_ARG, "NULL reader");
  MltRules R;
  if (int rc = mlt_rules(params, &R)) return rc;
  return mlt_search_on(rd->ix, *rd->S, *rd->V, seeds, n, R, k, flags, doc_ids, scores, counts);
}

// the single forms: the batch of one seed
extern "C" int tfidf_more_like_this(tfidf_index *ix, uint32_t seed, const tfidf_mlt_params *params, uint32_t k,
                                    uint32_t flags, uint32_t *doc_ids, float *scores, uint32_t *count) {
  if (!count) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  return tfidf_more_like_this_batch(ix, &seed, 1, params, k, flags, doc_ids, scores, count);
}

extern "C" int tfidf_reader_more_like_this(tfidf_reader *rd, uint32_t seed, const tfidf_mlt_params *params, uint32_t k,
                                           uint32_t flags, uint32_t *doc_ids, float *scores, uint32_t *count) {
  if (!count) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  return tfidf_reader_more_like_this_batch(rd, &seed, 1, params, k, flags, doc_ids, scores, count);
}

extern "C" int tfidf_last_mlt_stats(const tfidf_index *ix, uint64_t *row_entries_scanned, uint64_t *cand_chunks) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->ms_mu);
  if (row_entries_scanned) *row_entries_scanned = ix->last_mlt_entries;
  if (cand_chunks) *cand_chunks = ix->last_mlt_chunks;
  return TFIDF_OK;
}

// Concurrent single searches (the reference's Worker.processDocuments runs on
// concurrent request threads, Worker.java:175-186).  Requests queue up; the
// first caller to find no batch forming leads one: it waits wait_us for
// companions, takes every queued request (up to cq_max), runs them
// through the batched scorers (top-k requests: tfidf_search_batch, one launch
// for all; all-hits requests, k == 0, the shape every reference request has,
// Worker.java:230: tfidf_search_batch_all) and hands each caller its own
// hits; callers arriving meanwhile form the next batch.  Results are those of
// tfidf_search(k) for each query, including its errors (a query that does not
// parse gets TFIDF_E_QUERY_SYNTAX, not []; a k == 0 caller whose cap is below
// its hit count gets TFIDF_E_BUFFER with *n_out set, the others unaffected).
struct CoalesceReq {
  const uint8_t *q;
  uint64_t len;
  uint32_t k;
  uint32_t *docs;
  float *scores;
  uint64_t cap;
  uint64_t *n_out;
  int rc;
  std::string err;
  bool done;
  bool taken;        // in a batch a leader took (waits for that batch, never leads)
};

// One coalesced batch: queries that do not parse answer as tfidf_search
// would; the top-k requests go through one tfidf_search_batch launch, the
// all-hits requests (k == 0) through one tfidf_search_batch_all.
static void coalesced_run(tfidf_index *ix, const std::vector<CoalesceReq *> &batch) {
  std::vector<CoalesceReq *> run, run_all;
  std::vector<uint8_t> text, text_all;
  std::vector<uint64_t> offs{0}, offs_all{0};
  uint32_t kmax = 0;
  for (CoalesceReq *c : batch) {
    QueryPlan plan;
    const int prc = parse_query(c->q, c->len, &plan);
    if (prc == kQBadUtf8 || prc == kQSyntax) {
      c->rc = prc == kQBadUtf8 ? TFIDF_E_UNSUPPORTED_QUERY : TFIDF_E_QUERY_SYNTAX;
      c->err = prc == kQBadUtf8 ? "query is not valid UTF-8"
                                : "query does not parse (QueryParser ParseException / TooManyClauses)";
      *c->n_out = 0;
      continue;
    }
    std::vector<uint8_t> &tx = c->k ? text : text_all;
    tx.insert(tx.end(), c->q, c->q + c->len);
    (c->k ? offs : offs_all).push_back(tx.size());
    (c->k ? run : run_all).push_back(c);
    kmax = std::max(kmax, c->k);
  }
  if (!run.empty()) {
    std::vector<uint32_t> docs((size_t)run.size() * kmax), counts(run.size());
    std::vector<float> sc((size_t)run.size() * kmax);
    const int rc = tfidf_search_batch(ix, text.data(), offs.data(), (uint32_t)run.size(), kmax, docs.data(), sc.data(),
                                      counts.data());
    const std::string err = rc != TFIDF_OK ? std::string(tfidf_last_error()) : std::string();
    for (size_t i = 0; i < run.size(); i++) {
      CoalesceReq *c = run[i];
      if (rc != TFIDF_OK) { c->rc = rc; c->err = err; *c->n_out = 0; continue; }
      const uint64_t n = std::min<uint64_t>(counts[i], c->k);     // a prefix of the kmax list = the top-k
      *c->n_out = n;
      if (n > c->cap) { c->rc = TFIDF_E_BUFFER; c->err = "result buffer too small"; continue; }
      memcpy(c->docs, docs.data() + i * kmax, n * 4);
      memcpy(c->scores, sc.data() + i * kmax, n * 4);
    }
  }
  if (!run_all.empty()) {
    // the batch's own buffer: sized by the callers' capacities first, by the
    // reported size when some caller's hits exceed its capacity
    const uint32_t n = (uint32_t)run_all.size();
    uint64_t cap = 0, total = 0;
    const std::shared_ptr<Snapshot> snap = current(ix);
    const uint64_t n_docs = snap ? snap->n_docs : 0;
    for (CoalesceReq *c : run_all) cap += std::min(c->cap, n_docs);
    std::vector<uint32_t> docs(cap);
    std::vector<float> sc(cap);
    std::vector<uint64_t> ho(n + 1);
    int rc = tfidf_search_batch_all(ix, text_all.data(), offs_all.data(), n, docs.data(), sc.data(), cap, ho.data(),
                                    &total);
    if (rc == TFIDF_E_BUFFER) {
      docs.resize(total);
      sc.resize(total);
      rc = tfidf_search_batch_all(ix, text_all.data(), offs_all.data(), n, docs.data(), sc.data(), total, ho.data(),
                                  &total);
    }
    const std::string err = rc != TFIDF_OK ? std::string(tfidf_last_error()) : std::string();
    for (uint32_t i = 0; i < n; i++) {
      CoalesceReq *c = run_all[i];
      if (rc != TFIDF_OK) { c->rc = rc; c->err = err; *c->n_out = 0; continue; }
      const uint64_t h = ho[i + 1] - ho[i];
      *c->n_out = h;
      if (h > c->cap) {
        c->rc = TFIDF_E_BUFFER;
        c->err = "need " + std::to_string(h) + " result slots";
        continue;
      }
      memcpy(c->docs, docs.data() + ho[i], h * 4);
      memcpy(c->scores, sc.data() + ho[i], h * 4);
    }
  }
}


extern "C" int tfidf_search_coalesced(tfidf_index *ix, const uint8_t *q, uint64_t q_len, uint32_t k, uint32_t *doc_ids,
                                      float *scores, uint64_t cap, uint64_t *n_out, uint32_t wait_us) {
  if (!ix || (!q && q_len) || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (k > 1024) return fail(TFIDF_E_INVALID_ARG, "coalesced search needs k <= 1024 (0 = all hits)");
  CoalesceReq r{q, q_len, k, doc_ids, scores, cap, n_out, TFIDF_OK, std::string(), false, false};
  std::unique_lock<std::mutex> lk(ix->cq_mu);
  ix->cq.push_back(&r);
  bool slept = false;
  for (;;) {
    // served by a leader, or not yet taken and no batch is forming: lead one.
    // A request a running leader took waits for that leader (taking part in
    // the next batch would run an empty one).  A leader whose own request did
    // not fit its (capped) batch comes back here; requests left over after a
    // capped batch are woken and one of their callers leads next.
    ix->cq_cv.wait(lk, [&] { return r.done || (!r.taken && !ix->cq_leader); });
    if (r.done) break;
    ix->cq_leader = true;
    if (wait_us && !slept) {
      slept = true;
      lk.unlock();
      std::this_thread::sleep_for(std::chrono::microseconds(wait_us));
      lk.lock();
    }
    const size_t take = std::min(ix->cq.size(), ix->cq_max);   // >= 1: r itself is queued
    std::vector<CoalesceReq *> batch(ix->cq.begin(), ix->cq.begin() + take);
    ix->cq.erase(ix->cq.begin(), ix->cq.begin() + take);
    for (CoalesceReq *c : batch) c->taken = true;
    ix->cq_leader = false;                                // later arrivals lead the next batch
    if (!ix->cq.empty()) ix->cq_cv.notify_all();
    lk.unlock();
    coalesced_run(ix, batch);
    lk.lock();
    ix->cq_batches++;
    ix->cq_queries += batch.size();
    for (CoalesceReq *c : batch) c->done = true;
    ix->cq_cv.notify_all();
  }
  lk.unlock();
  if (r.rc != TFIDF_OK) return fail(r.rc, "%s", r.err.c_str());
  return TFIDF_OK;
}

extern "C" int tfidf_set_query_timing(tfidf_index *ix, int on) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  ix->q_timing = on != 0;
  return TFIDF_OK;
}

extern "C" int tfidf_last_search_ms(const tfidf_index *ix, float *ms_scoring, float *ms_total) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(const_cast<tfidf_index *>(ix)->ms_mu);
  if (ms_scoring) *ms_scoring = ix->last_ms_scoring;
  if (ms_total) *ms_total = ix->last_ms_total;
  return TFIDF_OK;
}

extern "C" int tfidf_set_stream(tfidf_index *ix, void *stream) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->cfg.device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  ix->stream = stream == TFIDF_OWN_STREAM ? ix->own_stream : static_cast<hipStream_t>(stream);
  ix->user_stream = stream == TFIDF_OWN_STREAM ? nullptr : static_cast<hipStream_t>(stream);
  return TFIDF_OK;
}

static int batch_keys_on(tfidf_index *ix, Snapshot &S, StatsView &V, const uint8_t *q_utf8,
                         const uint64_t *q_offsets, uint32_t n_q, uint32_t k, uint64_t doc_base, void *d_keys) {
  if (!ix || !q_offsets || (n_q && !d_keys)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (k == 0 || k > 1024) return fail(TFIDF_E_INVALID_ARG, "1 <= k <= 1024");
  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();
  DeviceGuard g(ix->cfg.device);
  if (n_q == 0) return TFIDF_OK;
  QueryBatch qb;
  if (int e = prepare_batch(ix, S, V, q_utf8, q_offsets, n_q, &qb)) return e;
  if (S.n_docs == 0 || qb.slot.empty()) {
    HIP_TRY(hipMemsetAsync(d_keys, 0, (size_t)n_q * k * 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    return TFIDF_OK;
  }
  int rc = run_scoring(ix, S, V, X, s, qb, n_q, k);
  if (rc) return rc;
  HIP_TRY(launch_pack_keys(X.res_doc, X.res_score, X.res_n, n_q, k,
                           doc_base, static_cast<uint64_t *>(d_keys), s));
  HIP_TRY(hipStreamSynchronize(s));
  set_last_ms(ix, qev_ms(X, QEV_0, QEV_1), qev_ms(X, QEV_0, QEV_2));
  return TFIDF_OK;
}

extern "C" int tfidf_search_batch_keys_device(tfidf_index *ix, const uint8_t *q_utf8, const uint64_t *q_offsets,
                                              uint32_t n_q, uint32_t k, uint64_t doc_base, void *d_keys) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "search before commit");
  return batch_keys_on(ix, *snap, *view, q_utf8, q_offsets, n_q, k, doc_base, d_keys);
}

static int all_keys_on(tfidf_index *ix, Snapshot &S, StatsView &V, const uint8_t *q, uint64_t q_len,
                       uint64_t doc_base, void *d_keys, uint64_t cap, uint64_t *n_out) {
  if (!ix || (!q && q_len) || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  *n_out = 0;
  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();
  if (cap < S.n_docs || (S.n_docs && !d_keys))
    return fail(TFIDF_E_BUFFER, "the key buffer needs num_docs = %llu entries", (unsigned long long)S.n_docs);
  DeviceGuard g(ix->cfg.device);
  PreparedQuery pq;
  int rc = prepare_query(S, V, q, q_len, &pq);
  if (rc) return rc;
  if (pq.slot.empty() || S.n_docs == 0) return TFIDF_OK;
  QueryBatch qb;
  qb.add(pq);
  rc = run_scoring(ix, S, V, X, s, qb, 1, 0);
  if (rc) return rc;
  const uint32_t R = S.n_blocks;
  HIP_TRY(X.hits_c.reserve((size_t)R * kBlockDocs * 8 + 8));
  HIP_TRY(X.hits_s.reserve((size_t)R * kBlockDocs * 8 + 8));
  HIP_TRY(X.hits_P.reserve(((size_t)R + 1) * 8));
  HIP_TRY(launch_hits_order(X.hits.as<uint64_t>(), X.hits_n.as<uint32_t>(), R, X.hits_P.as<uint64_t>(),
                            X.hits_c.as<uint64_t>(), X.hits.as<uint64_t>(), X.hits_s.as<uint64_t>(), nullptr, nullptr,
                            static_cast<uint64_t *>(d_keys), doc_base, hits_bound(S, pq), ix->num_cus * 4, s));
  if (X.q_timing) HIP_TRY(hipEventRecord(X.ev[QEV_2], s));
  HIP_TRY(hipMemcpyAsync(n_out, X.hits_P.as<uint64_t>() + R, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  set_last_ms(ix, qev_ms(X, QEV_0, QEV_1), qev_ms(X, QEV_0, QEV_2));
  return TFIDF_OK;
}

extern "C" int tfidf_search_all_keys_device(tfidf_index *ix, const uint8_t *q, uint64_t q_len, uint64_t doc_base,
                                            void *d_keys, uint64_t cap, uint64_t *n_out) {
  if (!ix || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  *n_out = 0;
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "search before commit");
  return all_keys_on(ix, *snap, *view, q, q_len, doc_base, d_keys, cap, n_out);
}

// the same on a reader's pinned snapshot (the node-level searches: status
// check, local search and document count from one snapshot)
int tfidf::reader_batch_keys_device(tfidf_reader *rd, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                    uint32_t k, uint64_t doc_base, void *d_keys) {
  return batch_keys_on(rd->ix, *rd->S, *rd->V, q_utf8, q_offsets, n_q, k, doc_base, d_keys);
}
int tfidf::reader_all_keys_device(tfidf_reader *rd, const uint8_t *q, uint64_t q_len, uint64_t doc_base, void *d_keys,
                                  uint64_t cap, uint64_t *n_out) {
  return all_keys_on(rd->ix, *rd->S, *rd->V, q, q_len, doc_base, d_keys, cap, n_out);
}

// A batch prepared once on a reader's snapshot (parse, analysis, dictionary
// lookups, weights), for the node-level all-hits batches: they score it in
// node chunks, each through reader_batch_all_keys_device.
struct tfidf::PreparedAllHits {
  QueryBatch qb;
};

int tfidf::reader_prepare_all_hits(tfidf_reader *rd, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                   PreparedAllHits **out, uint64_t *bounds) {
  if (!rd || !out || (n_q && (!q_offsets || !bounds))) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  *out = nullptr;
  std::unique_ptr<PreparedAllHits> pb(new PreparedAllHits());
  Snapshot &S = *rd->S;
  if (n_q && S.n_docs) {
    if (int e = prepare_batch(rd->ix, S, *rd->V, q_utf8, q_offsets, n_q, &pb->qb)) return e;
  } else {
    pb->qb.off.assign((size_t)n_q + 1, 0);
    pb->qb.meta.assign(n_q, 0);
  }
  const QueryBatch &qb = pb->qb;
  for (uint32_t i = 0; i < n_q; i++) {
    uint64_t hb = 0;
    for (uint32_t t = qb.off[i]; t < qb.off[i + 1]; t++)
      if ((qb.role[t] >> 24) != kRoleNot) hb += qb.ldf[t];
    bounds[i] = std::min<uint64_t>(hb, S.n_docs);
  }
  *out = pb.release();
  return TFIDF_OK;
}

void tfidf::free_prepared_all_hits(PreparedAllHits *pb) { delete pb; }

int tfidf::reader_batch_all_keys_device(tfidf_reader *rd, const PreparedAllHits *pb, uint32_t a, uint32_t z,
                                        uint64_t doc_base, void *d_keys, uint64_t cap, uint64_t *counts,
                                        uint64_t *n_out) {
  if (!rd || !pb || !n_out || a > z || (size_t)z + 1 > pb->qb.off.size() || (z > a && !counts))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument or query range out of the batch");
  *n_out = 0;
  for (uint32_t i = 0; i < z - a; i++) counts[i] = 0;
  tfidf_index *ix = rd->ix;
  Snapshot &S = *rd->S;
  if (z == a || S.n_docs == 0) return TFIDF_OK;
  CtxLease lease(ix);
  if (lease.rc) return lease.rc;
  SearchCtx &X = *lease.c;
  const hipStream_t s = lease.stream();
  DeviceGuard g(ix->cfg.device);
  const uint32_t fixed = all_hits_fixed_chunk();
  std::vector<uint64_t> qoff_h;
  uint64_t total = 0;
  bool any = false;
  for (uint32_t la = a; la < z;) {
    uint32_t lz = la;
    uint64_t bound = 0;
    all_hits_chunk(pb->qb, S, la, z, fixed, &lz, &bound);
    if (total + bound > cap || (bound && !d_keys))
      return fail(TFIDF_E_BUFFER, "the key buffer needs the range's hit bounds (%llu entries)",
                  (unsigned long long)(total + bound));
    if (int rc = all_hits_score_chunk(ix, S, *rd->V, X, s, pb->qb, la, lz, bound, &any,
                                      static_cast<uint64_t *>(d_keys) + total, doc_base, &qoff_h))
      return rc;
    if (!qoff_h.empty()) {
      for (uint32_t i = 0; i < lz - la; i++) counts[la - a + i] = qoff_h[i + 1] - qoff_h[i];
      total += qoff_h[lz - la];                    // the local chunks append
    }
    la = lz;
  }
  *n_out = total;
  set_route_ms(ix, any ? qev_ms(X, QEV_0, QEV_1) : 0.0f, any ? qev_ms(X, QEV_0, QEV_2) : 0.0f);
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// inspection

extern "C" int tfidf_doc_key(const tfidf_index *ix, uint64_t doc, uint8_t *buf, uint64_t cap, uint64_t *n_out) {
  if (!ix || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const std::shared_ptr<Snapshot> S = current(ix);
  if (!S || doc >= S->n_docs) return fail(TFIDF_E_INVALID_ARG, "doc out of range");
  std::string k;
  S->keys.key(S->staged_of(doc), &k);
  *n_out = k.size();
  if (k.size() > cap) return fail(TFIDF_E_BUFFER, "key needs %zu bytes", k.size());
  if (buf && !k.empty()) memcpy(buf, k.data(), k.size());
  return TFIDF_OK;
}

// the document's bytes out of the snapshot's own corpus buffer
static int doc_text_of(const Snapshot *S, uint64_t doc, uint8_t *buf, uint64_t cap, uint64_t *n_out) {
  if (doc >= S->n_docs) return fail(TFIDF_E_INVALID_ARG, "doc out of range");
  DeviceGuard g(S->dev);
  const uint64_t st = S->staged_of(doc);
  uint64_t o[2] = {0, 0};
  HIP_TRY(hipMemcpy(o, S->offsets->as<uint64_t>() + st, 16, hipMemcpyDeviceToHost));
  const uint64_t n = o[1] - o[0];
  *n_out = n;
  if (n > cap || (n && !buf)) return fail(TFIDF_E_BUFFER, "text needs %llu bytes", (unsigned long long)n);
  if (n) HIP_TRY(hipMemcpy(buf, S->text->as<uint8_t>() + o[0], n, hipMemcpyDeviceToHost));
  return TFIDF_OK;
}

extern "C" int tfidf_doc_text(tfidf_index *ix, uint64_t doc, uint8_t *buf, uint64_t cap, uint64_t *n_out) {
  if (!ix || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  *n_out = 0;
  const std::shared_ptr<Snapshot> S = current(ix);
  if (!S) return fail(TFIDF_E_INVALID_ARG, "doc out of range");
  return doc_text_of(S.get(), doc, buf, cap, n_out);
}

static int doc_keys_of(const Snapshot *S, uint8_t *buf, uint64_t cap, uint64_t *offsets, uint64_t *n_bytes) {
  uint64_t need = 0;
  for (uint64_t d = 0; d < S->n_docs; d++) need += S->keys.key_len(S->staged_of(d));
  *n_bytes = need;
  if (need > cap || (need && !buf)) return fail(TFIDF_E_BUFFER, "keys need %llu bytes", (unsigned long long)need);
  uint64_t p = 0;
  offsets[0] = 0;
  std::string k;
  for (uint64_t d = 0; d < S->n_docs; d++) {
    S->keys.key(S->staged_of(d), &k);
    memcpy(buf + p, k.data(), k.size());
    p += k.size();
    offsets[d + 1] = p;
  }
  return TFIDF_OK;
}

extern "C" int tfidf_doc_keys(const tfidf_index *ix, uint8_t *buf, uint64_t cap, uint64_t *offsets,
                              uint64_t *n_bytes) {
  if (!ix || !n_bytes || !offsets) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const std::shared_ptr<Snapshot> S = current(ix);
  if (!S) return fail(TFIDF_E_STATE, "not committed");
  return doc_keys_of(S.get(), buf, cap, offsets, n_bytes);
}

extern "C" int tfidf_malformed_docs(const tfidf_index *ix, uint64_t *docs, uint64_t cap, uint64_t *n_out) {
  if (!ix || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const std::shared_ptr<Snapshot> S = current(ix);
  if (!S) return fail(TFIDF_E_STATE, "not committed");
  *n_out = S->malformed.size();
  if (S->malformed.size() > cap || (cap && !docs && !S->malformed.empty()))
    return fail(TFIDF_E_BUFFER, "need %zu entries", S->malformed.size());
  for (size_t i = 0; i < S->malformed.size(); i++) docs[i] = S->malformed[i];
  return TFIDF_OK;
}

extern "C" int tfidf_doc_len(tfidf_index *ix, uint64_t doc, uint32_t *len, uint8_t *norm) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  const std::shared_ptr<Snapshot> S = current(ix);
  if (!S || doc >= S->n_docs) return fail(TFIDF_E_INVALID_ARG, "doc out of range");
  DeviceGuard g(ix->cfg.device);
  uint32_t l = 0;
  uint8_t n = 0;
  HIP_TRY(hipMemcpy(&l, S->doc_len.as<uint32_t>() + doc, 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&n, S->doc_norm.as<uint8_t>() + doc, 1, hipMemcpyDeviceToHost));
  if (len) *len = l;
  if (norm) *norm = n;
  return TFIDF_OK;
}

extern "C" int tfidf_doc_terms(tfidf_index *ix, uint64_t doc, char *terms, uint64_t terms_cap, uint32_t *tfs,
                               uint64_t cap, uint64_t *n_out) {
  if (!ix || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap || doc >= snap->n_docs) return fail(TFIDF_E_INVALID_ARG, "doc out of range");
  Snapshot &S = *snap;
  DeviceGuard g(ix->cfg.device);
  uint32_t nu = 0;
  HIP_TRY(hipMemcpy(&nu, S.doc_nuniq.as<uint32_t>() + doc, 4, hipMemcpyDeviceToHost));
  const uint64_t st = S.staged_of(doc);
  uint64_t off_st = 0;                               // the document's corpus offset (its CSR row base)
  HIP_TRY(hipMemcpy(&off_st, S.offsets->as<uint64_t>() + st, 8, hipMemcpyDeviceToHost));
  const uint64_t base = (off_st + st) >> 1;          // csr_row_base
  // packed entries: the row's range segments (rsplit) give each slot's range
  std::vector<uint32_t> ent(nu), col(nu), tf(nu), split(S.R);
  if (nu) {
    HIP_TRY(hipMemcpy(ent.data(), S.csr.as<uint32_t>() + base, nu * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(split.data(), S.rsplit.as<uint32_t>() + doc * S.R, S.R * 4, hipMemcpyDeviceToHost));
  }
  const uint32_t rs = S.range_shift, esc = csr_esc_value(rs);
  for (uint32_t i = 0, r = 0; i < nu; i++) {
    while (r + 1 < S.R && i >= split[r]) r++;
    col[i] = (r << rs) | csr_local(ent[i], rs);
    const uint32_t f = csr_tf_field(ent[i], rs);
    tf[i] = f == esc ? csr_esc_tf(S.h_esc.data(), S.h_esc.size(), base + i) : f;
  }
  std::vector<std::pair<std::string, uint32_t>> rows;
  for (uint32_t i = 0; i < nu; i++) {
    std::string t;
    if (int rc = slot_term(S, col[i], &t)) return rc;
    rows.emplace_back(std::move(t), tf[i]);
  }
  std::sort(rows.begin(), rows.end());
  uint64_t need = 0;
  for (auto &r : rows) need += r.first.size() + 1;
  *n_out = rows.size();
  if (need > terms_cap || rows.size() > cap) return fail(TFIDF_E_BUFFER, "buffers too small");
  uint64_t p = 0;
  for (size_t i = 0; i < rows.size(); i++) {
    memcpy(terms + p, rows[i].first.c_str(), rows[i].first.size() + 1);
    p += rows[i].first.size() + 1;
    tfs[i] = rows[i].second;
  }
  return TFIDF_OK;
}

extern "C" int tfidf_term_df(tfidf_index *ix, const uint8_t *term, uint64_t len, uint64_t *df_local,
                             uint64_t *df_effective) {
  if (!ix || (!term && len)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::shared_ptr<StatsView> V;
  const std::shared_ptr<Snapshot> S = current(ix, &V);
  if (!S) return fail(TFIDF_E_STATE, "not committed");
  if (int e = V->wait_gdf()) return e;
  DeviceGuard g(ix->cfg.device);
  std::string t((const char *)term, len);
  const uint32_t s = lookup_term(*S, t);
  const uint64_t l = s == kInvalidSlot ? 0 : S->h_df[s];
  if (df_local) *df_local = l;
  if (df_effective) *df_effective = (s != kInvalidSlot && V->global) ? V->gdf[s] : l;
  return TFIDF_OK;
}

extern "C" int tfidf_term_key(const uint8_t *term, uint64_t len, uint64_t *lo, uint64_t *hi) {
  if ((!term && len) || !lo || !hi) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::string t((const char *)term, len);
  term_key(t, lo, hi);
  return TFIDF_OK;
}

extern "C" int tfidf_analyze(const uint8_t *text, uint64_t len, char *out, uint64_t cap, uint64_t *n_tokens,
                             uint64_t *n_bytes) {
  if ((!text && len) || !n_tokens || !n_bytes || (!out && cap)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::vector<std::string> toks;
  if (!analyze(text, len, &toks)) return fail(TFIDF_E_UNSUPPORTED_INPUT, "text is not valid UTF-8");
  uint64_t need = 0;
  for (auto &t : toks) need += t.size() + 1;
  *n_tokens = toks.size();
  *n_bytes = need;
  if (need > cap) return fail(TFIDF_E_BUFFER, "buffer too small");
  uint64_t p = 0;
  for (auto &t : toks) {
    memcpy(out + p, t.data(), t.size());
    out[p + t.size()] = 0;
    p += t.size() + 1;
  }
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// GLOBAL statistics

extern "C" int tfidf_vocab_size(const tfidf_index *ix, uint64_t *n) {
  if (!ix || !n) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const std::shared_ptr<Snapshot> S = current(ix);
  *n = S ? S->num_terms : 0;
  return TFIDF_OK;
}

extern "C" int tfidf_vocab_export_device(tfidf_index *ix, void *d_keys, void *d_df, uint64_t cap, uint64_t *n_out) {
  if (!ix || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "not committed");
  const Snapshot &S = *snap;
  DeviceGuard g(ix->cfg.device);
  *n_out = S.num_terms;
  if (S.num_terms > cap) return fail(TFIDF_E_BUFFER, "need %llu keys", (unsigned long long)S.num_terms);
  // sorted (hi, lo) key list of this shard + df, assembled from the host mirror
  std::vector<std::pair<std::pair<uint64_t, uint64_t>, uint32_t>> v;
  v.reserve(S.num_terms);
  for (uint32_t s = 0; s < S.C; s++)
    if (S.h_dict[s])
      v.push_back({{S.h_dict[(size_t)S.C + s], S.h_dict[s]}, S.h_df[s]});
  std::sort(v.begin(), v.end());
  std::vector<uint64_t> keys(2 * v.size());
  std::vector<uint32_t> df(v.size());
  for (size_t i = 0; i < v.size(); i++) {
    keys[2 * i] = v[i].first.second;
    keys[2 * i + 1] = v[i].first.first;
    df[i] = v[i].second;
  }
  if (!v.empty()) {
    if (d_keys) HIP_TRY(hipMemcpy(d_keys, keys.data(), keys.size() * 8, hipMemcpyHostToDevice));
    if (d_df) HIP_TRY(hipMemcpy(d_df, df.data(), df.size() * 4, hipMemcpyHostToDevice));
  }
  return TFIDF_OK;
}

extern "C" int tfidf_vocab_export(tfidf_index *ix, uint64_t *keys, uint32_t *df_local, uint32_t *df_effective,
                                  uint64_t cap, uint64_t *n_out) {
  if (!ix || !n_out) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::shared_ptr<StatsView> view;
  const std::shared_ptr<Snapshot> snap = current(ix, &view);
  if (!snap) return fail(TFIDF_E_STATE, "not committed");
  const Snapshot &S = *snap;
  StatsView &V = *view;
  if (int e = V.wait_gdf()) return e;
  *n_out = S.num_terms;
  if (S.num_terms > cap) return fail(TFIDF_E_BUFFER, "need %llu terms", (unsigned long long)S.num_terms);
  std::vector<std::pair<std::pair<uint64_t, uint64_t>, uint32_t>> v;   // ((hi, lo), slot)
  v.reserve(S.num_terms);
  for (uint32_t s = 0; s < S.C; s++)
    if (S.h_dict[s]) v.push_back({{S.h_dict[(size_t)S.C + s], S.h_dict[s]}, s});
  std::sort(v.begin(), v.end());
  for (size_t i = 0; i < v.size(); i++) {
    const uint32_t s = v[i].second;
    if (keys) { keys[2 * i] = v[i].first.second; keys[2 * i + 1] = v[i].first.first; }
    if (df_local) df_local[i] = S.h_df[s];
    if (df_effective) df_effective[i] = V.global ? V.gdf[s] : S.h_df[s];
  }
  return TFIDF_OK;
}

extern "C" int tfidf_vocab_canonicalize_device(tfidf_index *ix, const void *d_all_keys, uint64_t n_all,
                                               void *d_df_canonical, uint64_t cap, uint64_t *n_canonical) {
  if (!ix || !n_canonical) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "not committed");
  const Snapshot &S = *snap;
  DeviceGuard g(ix->cfg.device);
  hipStream_t s = ix->stream;
  DevBuf canon;
  HIP_TRY(canon.reserve(n_all * 16 + 16));
  uint64_t nu = 0;
  HIP_TRY(sort_unique_keys128((const uint64_t *)d_all_keys, n_all, canon.as<uint64_t>(), &nu, s));
  *n_canonical = nu;
  if (nu > cap) { canon.release(); return fail(TFIDF_E_BUFFER, "need %llu canonical slots", (unsigned long long)nu); }
  HIP_TRY(ix->canon_of_slot.reserve((size_t)S.C * 4));
  HIP_TRY(slot_to_canon(S.dict.as<uint64_t>(), S.C, canon.as<uint64_t>(), nu, ix->canon_of_slot.as<uint32_t>(), s));
  if (d_df_canonical) {
    HIP_TRY(hipMemsetAsync(d_df_canonical, 0, nu * 4, s));
    HIP_TRY(scatter_df_canon(S.df_dev(), ix->canon_of_slot.as<uint32_t>(), S.C, (uint32_t *)d_df_canonical, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  canon.release();
  ix->n_canon = nu;
  return TFIDF_OK;
}

// The device-buffer exchange calls run on ix->stream.  On a caller's stream
// (tfidf_set_stream) they stay asynchronous: the caller's allocator orders
// its buffers on that stream.  On the index's own stream nothing orders the
// caller's buffers against the work, so the call returns only once the work
// that reads or writes them is done.
static int exchange_done(tfidf_index *ix) {
  if (ix->stream == ix->own_stream && hipStreamSynchronize(ix->stream) != hipSuccess)
    return fail(TFIDF_E_HIP, "hipStreamSynchronize failed");
  return TFIDF_OK;
}

static int vocab_partition(tfidf_index *ix, uint32_t n_ranks, void *d_records, uint64_t cap, void *d_counts,
                           uint64_t *n_out, bool sync) {
  if (!ix || !n_out || !d_counts || n_ranks == 0 || n_ranks > 1024)
    return fail(TFIDF_E_INVALID_ARG, "NULL argument or n_ranks not in [1, 1024]");
  std::lock_guard<std::mutex> lk(ix->mu);
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "not committed");
  const Snapshot &S = *snap;
  DeviceGuard g(ix->cfg.device);
  *n_out = S.num_terms;
  if (S.num_terms > cap) return fail(TFIDF_E_BUFFER, "need %llu records", (unsigned long long)S.num_terms);
  if (S.num_terms && !d_records) return fail(TFIDF_E_INVALID_ARG, "NULL records");
  hipStream_t s = ix->stream;
  HIP_TRY(ix->vcounts.reserve((size_t)n_ranks * 8 + 64));
  HIP_TRY(ix->sent_slot.reserve(S.num_terms * 4 + 4));
  uint32_t *cnt = ix->vcounts.as<uint32_t>(), *cur = cnt + n_ranks;
  HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)n_ranks * 4, s));
  HIP_TRY(vocab_count(S.dict.as<uint64_t>(), S.C, n_ranks, cnt, s));
  HIP_TRY(vocab_starts(cnt, n_ranks, cur, static_cast<uint64_t *>(d_counts), s));
  HIP_TRY(vocab_scatter(S.dict.as<uint64_t>(), S.df_dev(), S.C, n_ranks, cur, (uint64_t *)d_records,
                        ix->sent_slot.as<uint32_t>(), s));
  ix->n_sent = S.num_terms;
  return sync ? exchange_done(ix) : TFIDF_OK;          // asynchronous on a caller's stream
}
extern "C" int tfidf_vocab_partition_device(tfidf_index *ix, uint32_t n_ranks, void *d_records, uint64_t cap,
                                            void *d_counts, uint64_t *n_out) {
  return vocab_partition(ix, n_ranks, d_records, cap, d_counts, n_out, true);
}
int tfidf::vocab_partition_async(tfidf_index *ix, uint32_t n_ranks, void *d_records, uint64_t cap, void *d_counts,
                                 uint64_t *n_out) {
  return vocab_partition(ix, n_ranks, d_records, cap, d_counts, n_out, false);
}

static int vocab_reduce_dev(tfidf_index *ix, const void *d_records, uint64_t n, void *d_df_out, void *d_n_unique,
                            bool sync) {
  if (!ix || (n && (!d_records || !d_df_out))) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->cfg.device);
  hipStream_t s = ix->stream;
  if (n >= (1ull << 30)) return fail(TFIDF_E_CAPACITY, "too many vocabulary records");
  if (n == 0) {
    if (d_n_unique) HIP_TRY(hipMemsetAsync(d_n_unique, 0, 8, s));
    return TFIDF_OK;
  }
  uint64_t T = 1024;
  while (T < 2 * n) T <<= 1;
  HIP_TRY(ix->vt_table.reserve(T * 16));
  HIP_TRY(ix->vt_sum.reserve(T * 4));
  HIP_TRY(ix->vt_rslot.reserve(n * 4));
  HIP_TRY(hipMemsetAsync(ix->vt_table.p, 0, T * 16, s));
  HIP_TRY(hipMemsetAsync(ix->vt_sum.p, 0, T * 4, s));
  HIP_TRY(ix->vnu.reserve(64));
  unsigned long long *nu = reinterpret_cast<unsigned long long *>(d_n_unique ? d_n_unique : ix->vnu.p);   // counted in place
  HIP_TRY(hipMemsetAsync(nu, 0, 8, s));
  HIP_TRY(vocab_reduce((const uint64_t *)d_records, n, ix->vt_table.as<uint64_t>(), (uint32_t)(T - 1),
                       ix->vt_sum.as<uint32_t>(), ix->vt_rslot.as<uint32_t>(), (uint32_t *)d_df_out, nu, s));
  return sync ? exchange_done(ix) : TFIDF_OK;          // asynchronous on a caller's stream
}
extern "C" int tfidf_vocab_reduce_device(tfidf_index *ix, const void *d_records, uint64_t n, void *d_df_out,
                                         void *d_n_unique) {
  return vocab_reduce_dev(ix, d_records, n, d_df_out, d_n_unique, true);
}
int tfidf::vocab_reduce_async(tfidf_index *ix, const void *d_records, uint64_t n, void *d_df_out, void *d_n_unique) {
  return vocab_reduce_dev(ix, d_records, n, d_df_out, d_n_unique, false);
}

// A new statistics view for the current snapshot (the GLOBAL setters): built
// aside, complete on the device (norm cache uploaded) before searches see it.
// The view it replaces is kept as the next setter's spare.  async: the cache
// upload (and whatever the caller queued for the view before) completes
// behind the view's event, which every search waits for before its first use
// (StatsView::wait_gdf) — the setter itself never waits for the device.
static int publish_view(tfidf_index *ix, Snapshot &S, const std::shared_ptr<StatsView> &v, bool async = false) {
  if (int e = upload_cache(ix->cfg, *v, ix->stream, !async)) return e;
  if (async) {
    std::lock_guard<std::mutex> gl(v->gdf_mu);
    HIP_TRY(hipEventRecord(v->gdf_ev, ix->stream));
    v->gdf_pending = true;
  }
  std::shared_ptr<StatsView> old;
  {
    std::lock_guard<std::mutex> sl(ix->snap_mu);
    old = std::move(S.stats);
    S.stats = v;
  }
  if (old && old != v) ix->view_spare = std::move(old);
  return TFIDF_OK;
}

// A statistics view to fill: the spare one once no search holds it (ADVICE
// r05: a fresh view per GLOBAL exchange pinned C x 4 bytes of host memory and
// freed the previous view's, which synchronises the device), else a new one.
static std::shared_ptr<StatsView> take_view(tfidf_index *ix) {
  std::shared_ptr<StatsView> v;
  if (ix->view_spare && ix->view_spare.use_count() == 1) {
    v = std::move(ix->view_spare);
    if (v->wait_gdf() != TFIDF_OK) v.reset();          // its last uploads have left h_cache / gdf
  }
  ix->view_spare.reset();
  if (!v) v = std::make_shared<StatsView>(ix->cfg.device);
  v->global = false;
  v->gdf.clear();
  return v;
}

// tfidf_set_global_df_device (sync: the public call, which returns when the
// caller's df buffer has been read on the index's own stream) and its
// asynchronous form for tfidf_dist_global_commit (every buffer is the
// communicator's, ordered on the index's stream).  *generation: the commit
// generation of the snapshot the GLOBAL view was published on.
static int set_global_df(tfidf_index *ix, const void *d_df, uint64_t n, uint64_t doc_count, uint64_t sum_ttf,
                         bool sync, uint64_t *generation) {
  if (!ix || (n && !d_df)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "not committed");
  Snapshot &S = *snap;
  if (n != ix->n_sent) return fail(TFIDF_E_STATE, "expected %llu records (tfidf_vocab_partition_device)",
                                   (unsigned long long)ix->n_sent);
  DeviceGuard g(ix->cfg.device);
  hipStream_t s = ix->stream;
  std::shared_ptr<StatsView> v = take_view(ix);
  HIP_TRY(ix->gdf_dev.reserve((size_t)S.C * 4));
  HIP_TRY(hipMemsetAsync(ix->gdf_dev.p, 0, (size_t)S.C * 4, s));
  HIP_TRY(vocab_import(ix->sent_slot.as<uint32_t>(), (const uint32_t *)d_df, n, ix->gdf_dev.as<uint32_t>(), s));
  // host mirror for query analysis: copied asynchronously, waited for by the
  // first query (prepare_query) — the exchange itself needs no host sync
  HIP_TRY(v->gdf.resize(S.C));
  HIP_TRY(hipMemcpyAsync(v->gdf.data(), ix->gdf_dev.p, (size_t)S.C * 4, hipMemcpyDeviceToHost, s));
  {
    std::lock_guard<std::mutex> gl(v->gdf_mu);
    HIP_TRY(hipEventRecord(v->gdf_ev, s));
    v->gdf_pending = true;
  }
  v->global = true;
  v->doc_count = doc_count;
  v->sum_ttf = sum_ttf;
  if (generation) *generation = S.generation;
  if (sync) {
    if (int e = exchange_done(ix)) return e;
    return publish_view(ix, S, v);
  }
  return publish_view(ix, S, v, true);
}

extern "C" int tfidf_set_global_df_device(tfidf_index *ix, const void *d_df, uint64_t n, uint64_t doc_count,
                                          uint64_t sum_ttf) {
  return set_global_df(ix, d_df, n, doc_count, sum_ttf, true, nullptr);
}

int tfidf::set_global_df_async(tfidf_index *ix, const void *d_df, uint64_t n, uint64_t doc_count, uint64_t sum_ttf,
                               uint64_t *generation) {
  return set_global_df(ix, d_df, n, doc_count, sum_ttf, false, generation);
}

extern "C" int tfidf_set_global_stats_device(tfidf_index *ix, const void *d_df_canonical, uint64_t n_canonical,
                                             uint64_t doc_count, uint64_t sum_ttf) {
  if (!ix || !d_df_canonical) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "not committed");
  Snapshot &S = *snap;
  if (n_canonical != ix->n_canon) return fail(TFIDF_E_STATE, "canonical vocabulary size mismatch");
  DeviceGuard g(ix->cfg.device);
  hipStream_t s = ix->stream;
  std::shared_ptr<StatsView> v = take_view(ix);
  DevBuf gd;
  HIP_TRY(gd.reserve((size_t)S.C * 4));
  HIP_TRY(gather_df_canon((const uint32_t *)d_df_canonical, ix->canon_of_slot.as<uint32_t>(), S.C,
                          gd.as<uint32_t>(), s));
  HIP_TRY(v->gdf.resize(S.C));
  HIP_TRY(hipMemcpyAsync(v->gdf.data(), gd.p, (size_t)S.C * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  gd.release();
  v->global = true;
  v->doc_count = doc_count;
  v->sum_ttf = sum_ttf;
  return publish_view(ix, S, v);
}

extern "C" int tfidf_set_global_stats(tfidf_index *ix, const uint64_t *keys_lohi, const uint64_t *df, uint64_t n,
                                      uint64_t doc_count, uint64_t sum_ttf) {
  if (!ix || (n && (!keys_lohi || !df))) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return fail(TFIDF_E_STATE, "not committed");
  Snapshot &S = *snap;
  DeviceGuard g(ix->cfg.device);
  std::shared_ptr<StatsView> v = take_view(ix);
  HIP_TRY(v->gdf.assign(S.C, 0));
  for (uint32_t s = 0; s < S.C; s++) v->gdf[s] = S.h_df[s];  // keys not listed keep local df
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t s = host_lookup(S, keys_lohi[2 * i], keys_lohi[2 * i + 1]);
    if (s != kInvalidSlot) v->gdf[s] = (uint32_t)df[i];
  }
  v->global = true;
  v->doc_count = doc_count;
  v->sum_ttf = sum_ttf;
  return publish_view(ix, S, v);
}

extern "C" int tfidf_clear_global_stats(tfidf_index *ix) {
  if (!ix) return fail(TFIDF_E_INVALID_ARG, "NULL index");
  std::lock_guard<std::mutex> lk(ix->mu);
  const std::shared_ptr<Snapshot> snap = current(ix);
  if (!snap) return TFIDF_OK;
  Snapshot &S = *snap;
  DeviceGuard g(ix->cfg.device);
  std::shared_ptr<StatsView> v = take_view(ix);
  v->doc_count = S.doc_count;
  v->sum_ttf = S.sum_ttf;
  return publish_view(ix, S, v);
}

// ---------------------------------------------------------------------------
// Leader.start merge (host: it merges per-worker result lists by name)

// String.compareTo order of two UTF-8 names: Java compares UTF-16 code units,
// so a supplementary code point (a surrogate pair, lead 0xD800..0xDBFF)
// sorts below U+E000..U+FFFF although its code point is larger.  Both names
// are walked as UTF-16 code units (a supplementary code point yields its lead,
// then its trail surrogate); a malformed UTF-8 sequence compares by its bytes.
static bool utf8_next(const uint8_t *s, uint64_t n, uint64_t *i, uint32_t *cp) {
  const uint8_t c = s[*i];
  uint32_t len = c < 0x80 ? 1 : (c >> 5) == 6 ? 2 : (c >> 4) == 14 ? 3 : (c >> 3) == 30 ? 4 : 0;
  if (!len || *i + len > n) return false;
  uint32_t v = len == 1 ? c : c & (0x7Fu >> len);
  for (uint32_t k = 1; k < len; k++) {
    if ((s[*i + k] & 0xC0) != 0x80) return false;
    v = (v << 6) | (s[*i + k] & 0x3F);
  }
  *i += len;
  *cp = v;
  return true;
}

struct Utf16Units {                // UTF-8 bytes -> UTF-16 code units
  const uint8_t *s;
  uint64_t n, i = 0;
  uint32_t trail = 0;              // pending trail surrogate of a supplementary code point
  bool more() const { return trail || i < n; }
  // next code unit; false (at byte i) if the UTF-8 there is malformed
  bool next(uint32_t *u) {
    if (trail) { *u = trail; trail = 0; return true; }
    uint32_t cp;
    if (!utf8_next(s, n, &i, &cp)) return false;
    if (cp >= 0x10000) {
      *u = 0xD800 + ((cp - 0x10000) >> 10);
      trail = 0xDC00 + ((cp - 0x10000) & 0x3FF);
    } else {
      *u = cp;
    }
    return true;
  }
};

int tfidf::utf16_compare(const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb) {
  Utf16Units x{a, na}, y{b, nb};
  while (x.more() && y.more()) {
    const uint64_t i0 = x.i, j0 = y.i;
    uint32_t u, v;
    if (!x.next(&u) || !y.next(&v)) {                     // malformed: bytes from here on
      const uint64_t ra = na - i0, rb = nb - j0;
      const int c = memcmp(a + i0, b + j0, std::min(ra, rb));
      return c ? c : (ra < rb ? -1 : ra > rb);
    }
    if (u != v) return u < v ? -1 : 1;
  }
  return x.more() ? 1 : (y.more() ? -1 : 0);
}

extern "C" int tfidf_sort_names(const uint8_t *names, const uint64_t *offsets, uint64_t n, uint64_t *perm) {
  if (n && (!names || !offsets || !perm)) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  for (uint64_t i = 0; i < n; i++) perm[i] = i;
  std::stable_sort(perm, perm + n, [&](uint64_t x, uint64_t y) {
    return utf16_compare(names + offsets[x], offsets[x + 1] - offsets[x], names + offsets[y],
                         offsets[y + 1] - offsets[y]) < 0;
  });
  return TFIDF_OK;
}

extern "C" int tfidf_leader_merge(const uint8_t *names, const uint64_t *offsets, uint64_t n, const double *scores,
                                  uint64_t *out_first, double *out_sum, uint64_t *n_out) {
  if (!n_out || (n && (!names || !offsets || !scores || !out_first || !out_sum)))
    return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  std::unordered_map<std::string, size_t> pos;
  std::vector<uint64_t> first;
  std::vector<double> sum;
  for (uint64_t i = 0; i < n; i++) {
    std::string k((const char *)names + offsets[i], offsets[i + 1] - offsets[i]);
    auto it = pos.find(k);
    if (it == pos.end()) {                   // HashMap.merge: first value stored as-is
      pos.emplace(std::move(k), sum.size());
      first.push_back(i);
      sum.push_back(scores[i]);
    } else {
      sum[it->second] += scores[i];          // Double::sum in response order
    }
  }
  std::vector<size_t> idx(first.size());
  for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {   // TreeMap<String, Double>: String.compareTo
    const uint64_t x = first[a], y = first[b];
    return utf16_compare(names + offsets[x], offsets[x + 1] - offsets[x], names + offsets[y],
                         offsets[y + 1] - offsets[y]) < 0;
  });
  for (size_t r = 0; r < idx.size(); r++) {
    out_first[r] = first[idx[r]];
    out_sum[r] = sum[idx[r]];
  }
  *n_out = idx.size();
  return TFIDF_OK;
}

// ---------------------------------------------------------------------------
// synthetic corpus

extern "C" int tfidf_synth_corpus(int device, uint64_t seed, uint64_t n_docs, uint64_t doc_base, const double *cdf,
                                  uint32_t V, uint32_t len_min, uint32_t len_max, void **d_text, void **d_offsets,
                                  uint64_t *total_bytes) {
  if (!cdf || !d_text || !d_offsets || !total_bytes || V == 0 || len_max < len_min)
    return fail(TFIDF_E_INVALID_ARG, "bad argument");
  if (len_max >= (1u << 20) - 1) return fail(TFIDF_E_INVALID_ARG, "len_max must be < 2^20 - 1");
  DeviceGuard g(device);
  hipStream_t s;
  HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  const uint32_t G = 1u << 16;
  std::vector<uint32_t> guide(G + 1);
  for (uint32_t i = 0; i <= G; i++) {
    const double u = (double)i / (double)G;
    guide[i] = (uint32_t)(std::upper_bound(cdf, cdf + V, u) - cdf);
    if (guide[i] > V - 1) guide[i] = V - 1;
  }
  DevBuf dcdf, dguide, bytes;
  HIP_TRY(dcdf.reserve((size_t)V * 8));
  HIP_TRY(dguide.reserve((size_t)(G + 1) * 4));
  HIP_TRY(bytes.reserve(n_docs * 8 + 8));
  void *off = nullptr;
  HIP_TRY(hipMalloc(&off, (n_docs + 1) * 8));
  HIP_TRY(hipMemcpyAsync(dcdf.p, cdf, (size_t)V * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(dguide.p, guide.data(), (size_t)(G + 1) * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(synth_doc_lengths(seed, n_docs, doc_base, dcdf.as<double>(), dguide.as<uint32_t>(), V, len_min, len_max,
                            bytes.as<uint64_t>(), s));
  HIP_TRY(exclusive_scan_u64(bytes.as<uint64_t>(), (uint64_t *)off, n_docs, s));
  uint64_t tot = 0;
  HIP_TRY(hipMemcpyAsync(&tot, (uint64_t *)off + n_docs, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  void *txt = nullptr;
  HIP_TRY(hipMalloc(&txt, tot + 128));
  HIP_TRY(hipMemsetAsync(txt, 0, tot + 128, s));
  HIP_TRY(synth_doc_text(seed, n_docs, doc_base, dcdf.as<double>(), dguide.as<uint32_t>(), V, len_min, len_max,
                         (const uint64_t *)off, (uint8_t *)txt, s));
  HIP_TRY(hipStreamSynchronize(s));
  dcdf.release();
  dguide.release();
  bytes.release();
  hipStreamDestroy(s);
  *d_text = txt;
  *d_offsets = off;
  *total_bytes = tot;
  return TFIDF_OK;
}

extern "C" int tfidf_device_free(int device, void *d_ptr) {
  DeviceGuard g(device);
  if (d_ptr) HIP_TRY(hipFree(d_ptr));
  return TFIDF_OK;
}

extern "C" int tfidf_device_copy(int device, void *dst, const void *src, uint64_t bytes, int kind) {
  if ((!dst || !src) && bytes) return fail(TFIDF_E_INVALID_ARG, "NULL argument");
  if (kind != 1 && kind != 2) return fail(TFIDF_E_INVALID_ARG, "kind must be 1 (H2D) or 2 (D2H)");
  DeviceGuard g(device);
  if (bytes) HIP_TRY(hipMemcpy(dst, src, bytes, kind == 1 ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
  return TFIDF_OK;
}

extern "C" int tfidf_device_copy_ms(int device, const void *d_src, uint64_t bytes, uint32_t reps, float *ms) {
  if (!d_src || !bytes || !reps || !ms) return fail(TFIDF_E_INVALID_ARG, "NULL or empty argument");
  DeviceGuard g(device);
  DevMem dst(device);
  if (dst.reserve(bytes) != hipSuccess) {
    hipGetLastError();
    return fail(TFIDF_E_OOM, "tfidf_device_copy_ms: %llu bytes", (unsigned long long)bytes);
  }
  hipStream_t s = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  TimingEvents ev;
  int rc = TFIDF_OK;
  auto run = [&]() -> int {
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    for (uint32_t r = 0; r <= reps; r++) {             // round 0 warms up (first touch of dst)
      HIP_TRY(hipEventRecord(ev.a, s));
      HIP_TRY(hipMemcpyAsync(dst.p, d_src, bytes, hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipEventRecord(ev.b, s));
      HIP_TRY(hipStreamSynchronize(s));
      if (r) HIP_TRY(hipEventElapsedTime(&ms[r - 1], ev.a, ev.b));
    }
    return TFIDF_OK;
  };
  rc = run();
  hipStreamSynchronize(s);
  hipStreamDestroy(s);
  return rc;
}

// ---------------------------------------------------------------------------
// internal accessors for the node-level orchestration (tfidf_dist.hip)

hipStream_t tfidf::index_stream(tfidf_index *ix) { return ix->stream; }
int tfidf::index_device(const tfidf_index *ix) { return ix->cfg.device; }
bool tfidf::index_committed(const tfidf_index *ix) { return current(ix) != nullptr; }
uint64_t tfidf::index_num_docs(const tfidf_index *ix) {
  const std::shared_ptr<Snapshot> S = current(ix);
  return S ? S->n_docs : 0;
}
uint64_t tfidf::index_generation(const tfidf_index *ix) {
  const std::shared_ptr<Snapshot> S = current(ix);
  return S ? S->generation : 0;
}
int tfidf::set_error(int code, const char *msg) { return fail(code, "%s", msg); }
