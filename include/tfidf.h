/*
 * tfidf.h — C ABI of libtfidf, the MI355X-native TF-IDF/BM25 engine.
 *
 * Drop-in boundary for the reference's hot path (kheder-hassoun/
 * Tf-IDF-Distributed-System, Java + Lucene 9.8.0).  The reference has no
 * plugin API: the path sits behind direct Lucene calls in two Java methods
 * and one merge loop.  Each entry point below names the reference interface
 * it replaces (paths relative to TF-IDF-System-Core/src/main/java/):
 *
 *   tfidf_create / tfidf_destroy
 *       me/zookeeper/leader_election/worker/Worker.java:67-73
 *       (FSDirectory.open + new IndexWriter(dir, IndexWriterConfig(new StandardAnalyzer())))
 *   tfidf_add_docs / tfidf_add_docs_device
 *       Worker.java:190-220 addDocToIndex -> indexWriter.updateDocument(Term("path", rel), doc)
 *       (called from the Files.walk loop Worker.java:77-86 and upload Worker.java:136-139)
 *   tfidf_commit
 *       Worker.java:88 and :138 indexWriter.commit() (+ DirectoryReader.open at :223 sees it)
 *   tfidf_search / tfidf_search_batch / tfidf_search_batch_all
 *       Worker.java:222-241 searchIndex: QueryParser("contents", StandardAnalyzer)
 *       .parse(QueryParser.escape(q)); searcher.search(query, Integer.MAX_VALUE)
 *   tfidf_doc_key
 *       Worker.java:235-236 searcher.doc(sd.doc).get("path")
 *   tfidf_delete_docs / tfidf_compact / tfidf_set_compact_threshold
 *       IndexWriter.deleteDocuments(Term("path", key)) and the reclaiming of
 *       deletes by Lucene's segment merges; the upload path overwrites files by
 *       name (Worker.java:133-138 Files.copy REPLACE_EXISTING + updateDocument)
 *   tfidf_stats
 *       Worker.java:147-172 /worker/index-size (device bytes) + Lucene CollectionStatistics
 *   tfidf_vocab_* / tfidf_set_global_*
 *       no reference counterpart: GLOBAL statistics across GPU shards (the
 *       reference's 1-worker semantics, Leader.java:39-92 with one worker)
 *   tfidf_leader_merge
 *       me/zookeeper/leader_election/leader/Leader.java:73-88 (sum per name, TreeMap order)
 *   tfidf_node_* / tfidf_dist_* / tfidf_comm_*
 *       Leader.java:39-92 start (fan-out :51-70 over Worker.java:222-241, merge :73-88)
 *       with the workers as GPU shards and RCCL collectives in place of HTTP
 *   tfidf_node_search_batch_all / tfidf_dist_search_batch_all (GLOBAL),
 *   tfidf_node_search_names_batch / tfidf_dist_shard_search_batch (SHARD)
 *       the same for a batch of requests (Worker.java:230: every request asks
 *       for all hits), every hit of every query in one pass over the shards
 *
 * Conventions: every call returns an int status (TFIDF_OK == 0); the message
 * of the last failure on the calling thread is tfidf_last_error().  Buffers
 * are caller-owned and only borrowed for the duration of a call.
 * Threading (Worker.java:223 opens a DirectoryReader on the last commit per
 * request while uploads commit beside it, :136-139): every commit publishes an
 * immutable, refcounted snapshot.  Searches and the other read calls run on
 * the snapshot published when they start, concurrently with each other (each
 * on its own stream and scratch) and with tfidf_add_docs / tfidf_commit on
 * another thread, and never wait for a commit; a snapshot is freed, or rebuilt
 * by a later commit, when its last reader leaves.  Documents added after a
 * commit are invisible to searches until the next commit.  Writers (add_docs,
 * commit, clear, load, the GLOBAL statistics setters) serialise among
 * themselves (Worker.java:136 synchronized(indexWriter)).
 * Scores are IEEE float32 bit-identical to Lucene 9.8.0 BM25Similarity
 * (k1 = 1.2, b = 0.75); hits are ordered by (score desc, doc asc).
 */
#ifndef TFIDF_H
#define TFIDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFIDF_OK 0
#define TFIDF_E_INVALID_ARG 1
#define TFIDF_E_HIP 2
#define TFIDF_E_OOM 3
#define TFIDF_E_UNSUPPORTED_INPUT 4 /* tf >= 2^24 (a malformed UTF-8 document is indexed empty, see
                                       tfidf_malformed_docs) */
#define TFIDF_E_UNSUPPORTED_QUERY 5 /* malformed UTF-8 query */
#define TFIDF_E_CAPACITY 6          /* vocabulary capacity exceeded */
#define TFIDF_E_STATE 7             /* e.g. search before commit */
#define TFIDF_E_BUFFER 8            /* caller buffer too small; *n_out holds the size needed */
#define TFIDF_E_NO_DEVICE 9
#define TFIDF_E_QUERY_SYNTAX 10     /* QueryParser ParseException / TooManyClauses (Worker.java:182-185 -> []):
                                       empty query, leading AND/OR, trailing or doubled operator word */

#define TFIDF_STATS_SHARD 0  /* per-shard statistics: the reference's N-worker semantics */
#define TFIDF_STATS_GLOBAL 1 /* statistics imported from all shards: 1-worker semantics */

/* Inverted-index layout built by tfidf_commit (results are identical). */
#define TFIDF_INVERSION_AUTO 0  /* block-major unless its (docs/8192 + 1) x 2^vocab_capacity_log2 count table
                                   outgrows the CSR, or vocab_capacity_log2 > 21 (huge vocabularies), or the
                                   corpus is a few very long documents (fewer (block, range) tiles than CUs,
                                   >= 64 KB per document: books) */
#define TFIDF_INVERSION_BLOCK 1 /* block-major: postings grouped by 8192-doc block, then term */
#define TFIDF_INVERSION_TERM 2  /* term-major: postings grouped by term, docs ascending (sort-based) */

typedef struct tfidf_index tfidf_index;

typedef struct tfidf_config {
  float k1;                     /* BM25 k1, default 1.2f (BM25Similarity()); finite and >= 0 */
  float b;                      /* BM25 b,  default 0.75f; in [0, 1].  tfidf_create returns
                                   TFIDF_E_INVALID_ARG for any other k1 / b (NaN included), as
                                   BM25Similarity(k1, b) throws: scores must stay >= 0 and ordered.
                                   Legal values can give scores of exactly 0.0f (tf * norm_inverse
                                   <= 2^-24 at a large k1); such hits are returned like any other */
  int32_t stats_mode;           /* TFIDF_STATS_SHARD (default) or TFIDF_STATS_GLOBAL */
  int32_t device;               /* HIP device ordinal */
  uint32_t vocab_capacity_log2; /* dictionary slots = 2^x, x in [10, 26]; default 18.  A shard holds at most
                                   2^x distinct terms, exactly: a commit of 2^x terms succeeds on every
                                   tokenizer path, one of 2^x + 1 returns TFIDF_E_CAPACITY (see
                                   tfidf_commit).  The default is meant for <= ~200k terms (probes get
                                   longer as the table fills); x > 21 implies the term-major inversion */
  uint32_t max_token_len;       /* StandardAnalyzer.DEFAULT_MAX_TOKEN_LENGTH = 255 (only value supported) */
  int32_t inversion;            /* TFIDF_INVERSION_AUTO (default), _BLOCK or _TERM */
} tfidf_config;

typedef struct tfidf_index_stats {
  uint64_t num_docs;      /* live documents (maxDoc after compaction) */
  uint64_t doc_count;     /* documents with >= 1 token (CollectionStatistics.docCount) */
  uint64_t sum_ttf;       /* sumTotalTermFreq */
  uint64_t num_terms;     /* distinct terms in this shard */
  uint64_t nnz;           /* (doc, term) postings = sumDocFreq */
  uint64_t device_bytes;  /* HBM held by the index (feeds /worker/index-size) */
  uint64_t long_docs;     /* documents indexed by the long-document path */
  uint64_t text_bytes;    /* corpus bytes resident on the device */
  uint64_t term_major;    /* 1 if the last commit built the term-major layout (TFIDF_INVERSION_TERM) */
  uint64_t pack_docs;     /* documents per tokenizer window in the last commit (1 = one per window) */
  uint64_t pack_retried;  /* documents the packed windows handed to the one-per-window pass */
  uint64_t unicode_docs;  /* documents (window <= 4 KB) the ASCII wave path found non-ASCII text in */
  uint64_t long_chunked;  /* long documents indexed chunk-parallel (the rest of long_docs: k_tokenize_long) */
  uint64_t malformed_docs;/* documents that are not valid UTF-8, indexed empty (tfidf_malformed_docs) */
  uint64_t hash_seed;     /* seed of the hashed term keys (> 16-byte terms, > 14-byte non-ASCII ones); 0 unless a
                             hash collision was detected and the build redone (term identity stays
                             exact: every merge under a hashed key compares the strings) */
  uint64_t hash_rebuilds; /* seed attempt in force (0 = first seed): builds redone in the last commit because of
                             a hash collision, plus the floor set by tfidf_set_hash_attempt */
  uint64_t coalesced_batches;  /* tfidf_search_coalesced: batches run / queries served (index lifetime) */
  uint64_t coalesced_queries;
  uint64_t unit_batches;   /* batched top-k searches scored by query units (k_score_units) / units run */
  uint64_t unit_count;
  uint64_t fused_queries;  /* tfidf_search top-k calls served by the one-launch fused path (index lifetime) */
  uint64_t unicode_wave_docs;  /* of unicode_docs: those the wave rules took (non-ASCII letters that are
                                  ALetter and lower case only); the rest went to the Unicode wave path */
  uint64_t dead_docs;      /* staged documents replaced or deleted and not yet reclaimed (tfidf_compact) */
  uint64_t dead_bytes;     /* their staged text bytes (part of text_bytes) */
  uint64_t compactions;    /* tfidf_compact calls and commit-time compactions that reclaimed something (index
                              lifetime) */
} tfidf_index_stats;

/* Per-phase device times of the last commit, measured with HIP events on the
 * index's stream around each kernel. */
typedef struct tfidf_commit_timing {
  float ms_total;
  float ms_tokenize;   /* tfidf_tokenize_count: text -> per-doc TF rows (CSR) */
  float ms_long;       /* long-document path */
  /* (a lone inverted block taken in one launch, tfidf_commit_inversion_fused: ms_df also carries the DF
   * sum, the offset scan and the block base; ms_blockscan is the per-slot df kernel alone, ms_colscan ~0) */
  float ms_df;         /* per (doc block, term range) DF histograms */
  float ms_blockscan;  /* DF = sum over doc blocks + per-block posting offsets (scan over slots) */
  float ms_colscan;    /* exclusive scan of block totals -> block bases */
  float ms_scatter;    /* CSR -> block-segmented inverted postings */
  uint64_t text_bytes;
  uint64_t num_docs;
  uint64_t nnz;
} tfidf_commit_timing;

/* Host side of the last tfidf_commit (std::chrono::steady_clock; no GPU work
 * is added to take it).  The ms_* points are host times since the call began;
 * with seed retries they are those of the last attempt, while the counts and
 * bytes sum over all attempts.  A mirror form is how the snapshot's host copy
 * of the dictionary, the per-slot df or the slot -> column words was brought
 * up to date: not copied (nothing changed), a list of the changed slots, or
 * the whole array (see tfidf_commit). */
enum { TFIDF_MIRROR_NONE = 0, TFIDF_MIRROR_DELTA = 1, TFIDF_MIRROR_WHOLE = 2 };
typedef struct tfidf_host_profile {
  double ms_wall;          /* the whole call */
  double ms_counters;      /* the first read of the build counters returned */
  double ms_enqueued;      /* every kernel and copy of the inversion is enqueued */
  double ms_synced;        /* the final stream synchronisation returned */
  double ms_published;     /* the snapshot is published (0: the commit failed) */
  uint32_t stream_syncs;   /* host waits for the stream (blocking copies included) */
  uint32_t col_rank_runs;  /* times the slot -> column words were recomputed */
  uint32_t mirror_dict, mirror_df, mirror_crank;        /* TFIDF_MIRROR_* */
  uint32_t dict_delta_entries, df_delta_entries;        /* list lengths of the delta forms */
  uint64_t bytes_dict, bytes_df, bytes_crank;           /* copied device -> host */
} tfidf_host_profile;

const char *tfidf_version(void);
const char *tfidf_last_error(void);
int tfidf_config_init(tfidf_config *cfg);

int tfidf_create(const tfidf_config *cfg, tfidf_index **out);
int tfidf_destroy(tfidf_index *ix);

/* Host corpus: n_docs documents, document i = utf8[offsets[i] .. offsets[i+1]).
 * keys (may be NULL) = relative paths, key i = keys[key_offsets[i] .. key_offsets[i+1]);
 * a key already present replaces that document (updateDocument by Term("path", key)).
 * With keys == NULL the key of a document is its decimal ordinal in this index.
 * Bytes reach HBM through two pinned staging buffers (host copy of one overlapped
 * with the DMA of the other); the call returns once they are resident. */
int tfidf_add_docs(tfidf_index *ix, const uint8_t *utf8, const uint64_t *offsets, uint64_t n_docs,
                   const uint8_t *keys, const uint64_t *key_offsets);
/* Drop every staged and committed document (the index is empty, as after
 * tfidf_create); device and pinned staging buffers are kept for reuse. */
int tfidf_clear(tfidf_index *ix);
/* Device-resident corpus (e.g. produced by tfidf_synth_corpus): copied device-to-device. */
int tfidf_add_docs_device(tfidf_index *ix, const void *d_utf8, const void *d_offsets, uint64_t n_docs,
                          uint64_t total_bytes);

/* Build the index of the staged documents and publish it (IndexWriter.commit).
 * A commit that fails publishes nothing:
 *   - it returns the error (TFIDF_E_CAPACITY: more than 2^vocab_capacity_log2
 *     distinct terms, tfidf_last_error names the slot count;
 *     TFIDF_E_UNSUPPORTED_INPUT: a term more than 2^24 - 1 times in one
 *     document, which tf 2^24 - 1 itself is not);
 *   - searches, readers (those open and those opened afterwards), tfidf_stats'
 *     index fields, tfidf_term_df, tfidf_doc_* and tfidf_malformed_docs keep
 *     serving the last successful commit, bit for bit, and no commit
 *     generation is used up; before the first successful commit the index
 *     answers as a new one does (searches and tfidf_reader_open:
 *     TFIDF_E_STATE; tfidf_stats: num_docs 0);
 *   - every staged document stays staged (tfidf_stats.text_bytes and
 *     device_bytes count the staged corpus, not the published one), so
 *     calling tfidf_commit again fails the same way;
 *   - to recover, delete the offending documents (tfidf_delete_docs with their
 *     keys; a failed commit keeps every staged document, so delete followed by
 *     commit is the recovery path), replace them by key (tfidf_add_docs with
 *     their keys), or tfidf_clear and add a corpus that fits, then commit: the
 *     result is that of a new index given the same documents.  The index may
 *     also be destroyed and created again with a larger vocab_capacity_log2.
 * With a compaction threshold set (tfidf_set_compact_threshold) the commit
 * first reclaims the dead documents when they hold enough of the staged text.
 * Incremental commits (IndexWriter never analyses a document twice): a
 *   snapshot remembers which staged documents its term rows and dictionary
 *   cover.  When the snapshot a commit rebuilds was built from a prefix of the
 *   same staged corpus — no clear, load, delete, replace-by-key or compaction
 *   since, no dead document, the same layout, hash seed and debug knobs — the
 *   commit tokenizes the documents added since only.  A block-major snapshot
 *   also keeps the count rows, bases and postings of every 8192-document
 *   block whose documents were all present at its last inversion, and builds
 *   those of the later blocks only (a partial last block is always built
 *   again, also when nothing was added); df is summed over all blocks.  A
 *   term-major snapshot rebuilds its postings from the rows of all documents.
 *   Any other commit (the first build of a snapshot, a seed retry, the commit
 *   after a failed one) is a full build.  The published index is the same
 *   either way: equal through every call (the order of the postings inside a
 *   block's segment of one term is not fixed).  Commits alternate between two
 *   snapshots, so a new document is tokenized once for each (by two
 *   successive commits).
 * tfidf_commit_tokenized_docs: what the last tfidf_commit tokenized: *docs
 *   (may be NULL) = documents, *was_full (may be NULL) = 1 for a full build.
 *   TFIDF_DEBUG=1 TFIDF_FULL_COMMIT=1 forces full builds (A/B runs).
 * tfidf_commit_inverted_blocks: what the last tfidf_commit's inversion built:
 *   blocks [*first_block, *n_blocks) (the blocks before were kept; 0 for
 *   term-major and full builds), *remapped = 1 when the kept count rows moved
 *   to a wider column layout because the vocabulary grew.  Each pointer may be
 *   NULL.  TFIDF_DEBUG=1 TFIDF_FULL_INVERSION=1 inverts every block (A/B runs).
 *   The df of the kept blocks comes from a per-column base the snapshot keeps;
 *   TFIDF_DEBUG=1 TFIDF_DF_FROM_ROWS=1 sums their count rows instead (A/B runs).
 * tfidf_commit_inversion_shape: the launch shape of the last tfidf_commit's
 *   block-major inversion: *slices = document slices per (block, range) tile,
 *   *scan_parts = workgroups per block row in the row scan (1 / 1: one
 *   workgroup each, as for every grid that fills the device; also for
 *   term-major).  Few inverted blocks (an incremental commit's tail) are cut
 *   up so that they use the whole device; the published index is the same
 *   under every shape.  Each pointer may be NULL.
 * tfidf_commit_inversion_fused: *fused = 1 when the last tfidf_commit inverted
 *   exactly one block in two or more slices and took its counts, df, column
 *   offsets and block base in one launch (the usual case of an incremental
 *   commit's tail block), 0 when it ran the separate kernels.  The published
 *   index is the same either way.  TFIDF_DEBUG=1 TFIDF_INV_UNFUSED=1 keeps the
 *   separate kernels (A/B runs); a forced TFIDF_TEST_SCAN_PARTS and
 *   TFIDF_DF_FROM_ROWS do as well.
 * Host mirrors: df lookups, the vocabulary export, query analysis and the
 *   GLOBAL setters read pinned host copies of a snapshot's dictionary keys,
 *   per-slot df and slot -> column words.  An incremental block-major commit
 *   whose target's last build succeeded brings them up to date with the new
 *   slots' keys and the changed df alone, or copies nothing when nothing
 *   changed; every other commit copies them whole.  The published index is
 *   the same either way.  TFIDF_DEBUG=1 TFIDF_FULL_MIRROR=1 copies them whole
 *   always (A/B runs).
 * tfidf_commit_host_profile: the host side of the last tfidf_commit (see
 *   tfidf_host_profile above): where the host's time went, how often it
 *   waited for the stream (2 for an incremental commit without new documents,
 *   3 for one that adds documents, plus the waits of the tokenizer's packed
 *   and long-document paths where they run), and per mirror the form it took
 *   and the bytes copied device -> host.  It costs nothing on the device. */
int tfidf_commit(tfidf_index *ix);
int tfidf_commit_tokenized_docs(const tfidf_index *ix, uint64_t *docs, uint32_t *was_full);
int tfidf_commit_inverted_blocks(const tfidf_index *ix, uint32_t *first_block, uint32_t *n_blocks,
                                 uint32_t *remapped);
int tfidf_commit_inversion_shape(const tfidf_index *ix, uint32_t *slices, uint32_t *scan_parts);
int tfidf_commit_inversion_fused(const tfidf_index *ix, uint32_t *fused);
int tfidf_commit_host_profile(const tfidf_index *ix, tfidf_host_profile *out);

/* ---- document lifecycle: delete, reclaim, read back ----
 * tfidf_delete_docs: IndexWriter.deleteDocuments(new Term("path", key)) for
 *   n_keys keys, key i = keys[key_offsets[i] .. key_offsets[i+1]).  A writer
 *   call, staged like tfidf_add_docs: searches and readers keep the last
 *   commit until the next tfidf_commit.  A key that names no live document is
 *   not an error and is not counted (Lucene's delete-by-term); a key given
 *   twice counts once; *n_deleted (may be NULL) = documents that went from
 *   live to dead.  The key is forgotten: adding it later appends a new
 *   document, as for a key never seen.  A keyless document (keys == NULL at add
 *   time) is addressed by its key, its decimal ordinal; explicit keys are
 *   looked up first.
 * Keys never change: a keyless document keeps the ordinal it received when it
 *   was added (the number of documents staged before it since create, clear
 *   or load), whatever tfidf_compact does to the staged corpus, and later
 *   keyless documents keep counting from there, never reusing a number.
 * tfidf_compact: reclaim the dead documents (replaced or deleted) of the
 *   staged corpus, as Lucene does when segments merge.  A writer call.  The
 *   live documents are copied, in their order, into a NEW corpus buffer and
 *   offsets buffer by one device copy kernel; the old buffers are never
 *   written, because the published snapshot, open readers and in-flight
 *   searches still read them, and they are freed when the last of those goes
 *   (for the published snapshot: at the commit after the next).  Until then
 *   both corpora are resident: the peak is old + new text, at most 2x the
 *   staged text.  *bytes_reclaimed (may be NULL) = text bytes reclaimed;
 *   *ms_device (may be NULL) = the copy kernel's time (HIP events on the
 *   index's stream).  Nothing dead: no allocation, no kernel, 0 reclaimed.  On
 *   TFIDF_E_OOM / TFIDF_E_HIP the index is exactly as before the call.  The
 *   commit after a compaction produces the same index (doc ids, keys, scores)
 *   as the commit without it; tfidf_save afterwards writes live documents only.
 * tfidf_set_compact_threshold: with dead_pct in 1..100, tfidf_commit compacts
 *   first when dead text bytes x 100 >= dead_pct x staged text bytes; 0
 *   (default) = never.
 * tfidf_doc_text / tfidf_reader_doc_text: the committed document's bytes as
 *   they were added (its "stored field"), copied from the snapshot's own corpus
 *   buffer; TFIDF_E_BUFFER with *n_out = size needed when cap is too small. */
int tfidf_delete_docs(tfidf_index *ix, const uint8_t *keys, const uint64_t *key_offsets, uint64_t n_keys,
                      uint64_t *n_deleted);
int tfidf_compact(tfidf_index *ix, uint64_t *bytes_reclaimed, float *ms_device);
int tfidf_set_compact_threshold(tfidf_index *ix, uint32_t dead_pct);
int tfidf_doc_text(tfidf_index *ix, uint64_t doc, uint8_t *buf, uint64_t cap, uint64_t *n_out);
/* GLOBAL statistics match terms across shards by their keys, so every shard
 * must hash its long / non-ASCII terms with one seed.  A commit tries seed
 * attempts 0, 1, 2, 3 in turn (the next one after a detected collision);
 * this sets the attempt the following commits start from (0..3; 0 = the
 * default).  Multi-GPU: the ranks agree on the highest attempt any shard
 * needed and re-commit under it (tfidf_amd/distributed.py global_commit).
 * No reference counterpart: each Lucene worker is independent (Leader.java:67-69). */
int tfidf_set_hash_attempt(tfidf_index *ix, uint32_t attempt);

/* Persistence (the reference's FSDirectory index, Worker.java:67-73).  tfidf_save
 * writes the staged corpus (text, offsets, document keys, replace-by-key
 * liveness) to `path` (atomically: path.tmp, then rename).  tfidf_load stages a
 * saved file into an EMPTY index (same vocab_capacity_log2); call tfidf_commit
 * afterwards (more documents may be added first, replacing by key as usual).
 * The inverted index itself is rebuilt by the commit rather than stored.
 * File version 1; an index whose keyless documents' keys are no longer their
 * positions (after tfidf_compact) writes version 2, which adds their ordinals.
 * Both load.  The file records k1 and b: tfidf_load returns
 * TFIDF_E_INVALID_ARG, and stages nothing, when their bit patterns differ from
 * this index's configuration (the saved index's ranking is not this one's). */
int tfidf_save(tfidf_index *ix, const char *path);
int tfidf_load(tfidf_index *ix, const char *path);
int tfidf_get_commit_timing(const tfidf_index *ix, tfidf_commit_timing *out);
int tfidf_stats(const tfidf_index *ix, tfidf_index_stats *out);

/* Single query. k == 0 returns all hits (searcher.search(q, Integer.MAX_VALUE)).
 * doc_ids are local document ordinals; scores are float32. */
int tfidf_search(tfidf_index *ix, const uint8_t *q, uint64_t q_len, uint32_t k, uint32_t *doc_ids,
                 float *scores, uint64_t cap, uint64_t *n_out);
/* n_q queries; query i = q_utf8[q_offsets[i] .. q_offsets[i+1]).  1 <= k <= 1024.
 * Outputs are n_q x k (row i holds counts[i] valid hits). */
/* Concurrent single searches (Worker.processDocuments on concurrent request
 * threads, Worker.java:175-186): same arguments and results as tfidf_search
 * with k <= 1024, but callers arriving together are served by ONE batched
 * scoring launch per kind (the first waits wait_us for companions): the top-k
 * requests by tfidf_search_batch, the all-hits requests (k == 0, what every
 * reference request asks for, Worker.java:230) by tfidf_search_batch_all.  A
 * k == 0 caller whose cap is below its hit count gets TFIDF_E_BUFFER with
 * *n_out set, like tfidf_search; the batch's other callers are unaffected.
 * Thread-safe; a caller blocks until its own results are written. */
int tfidf_search_coalesced(tfidf_index *ix, const uint8_t *q, uint64_t q_len, uint32_t k, uint32_t *doc_ids,
                           float *scores, uint64_t cap, uint64_t *n_out, uint32_t wait_us);
int tfidf_search_batch(tfidf_index *ix, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                       uint32_t k, uint32_t *doc_ids, float *scores, uint32_t *counts);
/* Every hit of each of n_q queries (tfidf_search with k == 0, per query):
 * query i's hits are doc_ids/scores[hit_offsets[i] .. hit_offsets[i+1]), ordered
 * (score desc, doc asc); hit_offsets has n_q + 1 entries and is always written
 * in full.  *n_out = hit_offsets[n_q].  TFIDF_E_BUFFER when that exceeds cap
 * (nothing is promised about doc_ids/scores then; call again with the size).
 * A query that does not parse has no hits, as in tfidf_search_batch.
 * Worker.java:230 for a batch of requests (cfg 4).  The device scratch is
 * bounded: the queries are scored and merged in chunks. */
int tfidf_search_batch_all(tfidf_index *ix, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                           uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out);
/* Readers (Worker.java:223 DirectoryReader.open per request; the hits' stored
 * "path" fields are read from the same reader, :234-238): a reader pins the
 * snapshot published when it is opened, so doc ids it returns map to keys
 * with tfidf_reader_doc_key even while later commits publish other snapshots.
 * tfidf_reader_search: as tfidf_search, on the reader's snapshot.
 * tfidf_reader_info: the snapshot's commit generation (1, 2, ... per
 * successful commit) and document count.  A reader may be used from several
 * threads; close it once (its snapshot is released with the last user). */
typedef struct tfidf_reader tfidf_reader;
int tfidf_reader_open(tfidf_index *ix, tfidf_reader **out);
int tfidf_reader_close(tfidf_reader *rd);
int tfidf_reader_info(const tfidf_reader *rd, uint64_t *generation, uint64_t *num_docs);
int tfidf_reader_search(tfidf_reader *rd, const uint8_t *q, uint64_t q_len, uint32_t k, uint32_t *doc_ids,
                        float *scores, uint64_t cap, uint64_t *n_out);
/* tfidf_search_batch_all on the reader's snapshot. */
int tfidf_reader_search_batch_all(tfidf_reader *rd, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                  uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                  uint64_t *n_out);
int tfidf_reader_doc_key(const tfidf_reader *rd, uint64_t doc, uint8_t *buf, uint64_t cap, uint64_t *n_out);
/* tfidf_doc_text on the reader's snapshot (unchanged by later deletes, compactions and commits). */
int tfidf_reader_doc_text(const tfidf_reader *rd, uint64_t doc, uint8_t *buf, uint64_t cap, uint64_t *n_out);
/* tfidf_doc_keys of the reader's snapshot (offsets[num_docs + 1] of tfidf_reader_info). */
int tfidf_reader_doc_keys(const tfidf_reader *rd, uint8_t *buf, uint64_t cap, uint64_t *offsets, uint64_t *n_bytes);
/* ---- hit highlighting: match offsets and snippets from the device corpus ----
 * No reference counterpart (Worker.java:216 stores "contents" with Store.NO);
 * the step past tfidf_doc_text: the device re-scans only the listed documents
 * of the snapshot's own corpus and returns which words matched and one short
 * passage per document, instead of the caller downloading whole documents.
 * Positive terms of a query: parsed as tfidf_search parses it, the analysed
 *   terms of every clause that is not MUST_NOT, distinct, in order of first
 *   appearance; a term's position in that list is its ordinal (a function of the
 *   query alone: a term the index does not hold keeps its ordinal and matches
 *   nothing).  tfidf_query_positive_terms returns them NUL-terminated, in
 *   ordinal order (host only; buffer protocol of tfidf_analyze).
 * Matches of (query, document): the tokens of the document, as the index
 *   tokenised it, whose term is a positive term: (start, len, ordinal), start and
 *   len in bytes of the original text relative to the document's first byte (len
 *   is the raw span: "İstanbul" is 9 bytes for the term "istanbul"), ascending by
 *   start.  A document that is not valid UTF-8 (indexed empty) has none; a
 *   document that is not a hit of the query is legal and yields what it holds.
 * Snippet of (query, document, W = max_bytes, 16 <= W <= 65536): every match
 *   of at most W bytes is a candidate whose window holds the matches from it on
 *   that end within W bytes of its start; the best window has the most distinct
 *   terms (ordinals >= 63 count as one), then the most matches, then the
 *   earliest start.  The range starts half the unused bytes before the window
 *   (not before the document), is W bytes long (not past the document's end),
 *   and both ends move inwards to UTF-8 character boundaries; without a
 *   candidate it is the head of the document.  The snippet is that byte range;
 *   its matches are the document's matches wholly inside it, starts relative
 *   to the snippet.  DESIGN.md section 2 states the rule exactly.
 * docs may repeat and come in any order; output row i belongs to docs[i]: its
 *   matches are [match_offsets[i], match_offsets[i + 1]) of starts / lens /
 *   ordinals, its snippet [text_offsets[i], text_offsets[i + 1]) of text, which
 *   begins at byte doc_starts[i] of the document.  A doc >= num_docs:
 *   TFIDF_E_INVALID_ARG, nothing written.  n_docs == 0: OK, offsets {0}.
 * Query errors as in tfidf_search.  The offsets arrays (n_docs + 1 entries),
 *   doc_starts and the totals are always written in full; TFIDF_E_BUFFER when a
 *   total exceeds its cap (nothing is promised about the payload then; cap 0
 *   with NULL payload pointers asks for the sizes).  Snippet text never exceeds
 *   n_docs x max_bytes.  *ms_device (may be NULL): HIP events on the call's
 *   stream, first copy to last.
 * A call is served as the batch of one query (below): its rows run in
 *   consecutive chunks under the batch's scratch budgets, so a call that plans
 *   more than 2^16 (row, 16 KiB) items or finds more than 2^22 matches takes
 *   several chunks with bounded scratch instead of one pass with scratch for
 *   all of it.  The planned items of one call are not limited (2^24 once);
 *   n_docs > 2^26 is TFIDF_E_INVALID_ARG.  tfidf_last_highlight_chunks does
 *   not report these calls.
 * The calls run on a search context (own stream and scratch) beside other
 *   readers, tfidf_add_docs and tfidf_commit, and never wait for a commit;
 *   tfidf_matches / tfidf_snippets use the snapshot published at the call. */
int tfidf_reader_matches(tfidf_reader *rd, const uint8_t *q, uint64_t q_len, const uint32_t *docs, uint64_t n_docs,
                         uint64_t *starts, uint32_t *lens, uint32_t *ordinals, uint64_t cap,
                         uint64_t *match_offsets, uint64_t *n_out, float *ms_device);
int tfidf_reader_snippets(tfidf_reader *rd, const uint8_t *q, uint64_t q_len, const uint32_t *docs, uint64_t n_docs,
                          uint32_t max_bytes, uint8_t *text, uint64_t text_cap, uint64_t *text_offsets,
                          uint64_t *doc_starts, uint64_t *starts, uint32_t *lens, uint32_t *ordinals, uint64_t m_cap,
                          uint64_t *match_offsets, uint64_t *n_text, uint64_t *n_matches, float *ms_device);
int tfidf_matches(tfidf_index *ix, const uint8_t *q, uint64_t q_len, const uint32_t *docs, uint64_t n_docs,
                  uint64_t *starts, uint32_t *lens, uint32_t *ordinals, uint64_t cap, uint64_t *match_offsets,
                  uint64_t *n_out, float *ms_device);
int tfidf_snippets(tfidf_index *ix, const uint8_t *q, uint64_t q_len, const uint32_t *docs, uint64_t n_docs,
                   uint32_t max_bytes, uint8_t *text, uint64_t text_cap, uint64_t *text_offsets, uint64_t *doc_starts,
                   uint64_t *starts, uint32_t *lens, uint32_t *ordinals, uint64_t m_cap, uint64_t *match_offsets,
                   uint64_t *n_text, uint64_t *n_matches, float *ms_device);
int tfidf_query_positive_terms(const uint8_t *q, uint64_t q_len, char *out, uint64_t cap, uint64_t *n_terms,
                               uint64_t *n_bytes);
/* ---- batched hit highlighting: the rows of many queries in one call ----
 * A row is one (query, document) pair.  The n_q queries come as in
 * tfidf_search_batch_all (q_utf8, q_offsets[n_q + 1]); their documents in CSR
 * form: query i owns rows [doc_offsets[i], doc_offsets[i + 1]) of docs, R =
 * doc_offsets[n_q].  This is the layout tfidf_search_batch_all writes
 * (hit_offsets, doc_ids), so its output, or any per-query prefix of it, can be
 * passed on.  Rows may repeat documents within and across queries; a query may
 * own no row; n_q == 0 or R == 0: OK, offsets {0}.
 * Row r's matches and snippet are exactly what tfidf_matches / tfidf_snippets
 *   return for (its query, docs[r]) on the same snapshot: the positive terms
 *   and ordinals of that query, the match triples, the passage rule, the UTF-8
 *   snapping and the in-snippet matches.  All output offset arrays have R + 1
 *   entries; doc_starts has R.
 * A query that does not parse, or is not valid UTF-8, does not fail the batch
 *   (the convention of tfidf_search_batch[_all]: it has no hits): its rows have
 *   no matches and get head-of-document snippets, as a query with no positive
 *   term present does.
 * TFIDF_E_INVALID_ARG, nothing written: doc_offsets not non-decreasing from 0,
 *   a doc >= num_docs, R > 2^26, max_bytes outside 16..65536.
 * Buffer protocol of the single form: offsets, doc_starts and totals are
 *   always written in full, also when a payload cap is too small
 *   (TFIDF_E_BUFFER); cap 0 with NULL payload pointers asks for the sizes.
 * One call costs one chain of launches and synchronisations, not one per
 *   query.  Scratch is bounded: the rows are processed in consecutive chunks
 *   under a budget of 2^16 planned (row, 16 KiB) items and 2^22 matches (one
 *   row at least), each chunk appending its payload at the running totals.
 * The calls run on a search context beside readers, tfidf_add_docs and
 *   tfidf_commit; tfidf_matches_batch / tfidf_snippets_batch use the snapshot
 *   published at the call.  *ms_device as in the single form. */
int tfidf_reader_matches_batch(tfidf_reader *rd, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                               const uint32_t *docs, const uint64_t *doc_offsets, uint64_t *starts, uint32_t *lens,
                               uint32_t *ordinals, uint64_t cap, uint64_t *match_offsets, uint64_t *n_out,
                               float *ms_device);
int tfidf_reader_snippets_batch(tfidf_reader *rd, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                const uint32_t *docs, const uint64_t *doc_offsets, uint32_t max_bytes, uint8_t *text,
                                uint64_t text_cap, uint64_t *text_offsets, uint64_t *doc_starts, uint64_t *starts,
                                uint32_t *lens, uint32_t *ordinals, uint64_t m_cap, uint64_t *match_offsets,
                                uint64_t *n_text, uint64_t *n_matches, float *ms_device);
int tfidf_matches_batch(tfidf_index *ix, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                        const uint32_t *docs, const uint64_t *doc_offsets, uint64_t *starts, uint32_t *lens,
                        uint32_t *ordinals, uint64_t cap, uint64_t *match_offsets, uint64_t *n_out, float *ms_device);
int tfidf_snippets_batch(tfidf_index *ix, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                         const uint32_t *docs, const uint64_t *doc_offsets, uint32_t max_bytes, uint8_t *text,
                         uint64_t text_cap, uint64_t *text_offsets, uint64_t *doc_starts, uint64_t *starts,
                         uint32_t *lens, uint32_t *ordinals, uint64_t m_cap, uint64_t *match_offsets,
                         uint64_t *n_text, uint64_t *n_matches, float *ms_device);
/* Row chunks of the last batched highlighting call that ran on this index
 * (any form): the chunks the item budget cut, and the final chunks after the
 * match budget cut those further (1, 1 when everything fitted). */
int tfidf_last_highlight_chunks(const tfidf_index *ix, uint64_t *item_chunks, uint64_t *row_chunks);
/* ---- fuzzy term lookup: the vocabulary terms within max_edits of a term ----
 * (Lucene's FuzzyQuery term enumeration / DirectSpellChecker; the reference
 * has no counterpart: QueryParser.escape neutralises '~'.)
 * Vocabulary of a snapshot: every term of its dictionary with local df >= 1,
 *   as lower-cased UTF-8 bytes.
 * Input: n_terms byte strings (t_utf8, t_offsets[n_terms + 1], the layout of
 *   q_utf8 / q_offsets).  A term is not tokenised; it is lower-cased per code
 *   point as LowerCaseFilter does.  An empty term, one that is not strict
 *   UTF-8, or one longer than 255 UTF-16 units has no candidates and n_within
 *   0, without failing the call.
 * Distance: optimal string alignment over Unicode code points: insert,
 *   delete, substitute and transpose two adjacent code points cost 1 each, no
 *   substring is edited twice (ca -> abc is 3).  max_edits is 0, 1 or 2.
 * Prefix: with p = min(prefix_len, code points of the term), a candidate has
 *   at least p code points and its first p equal the term's; the distance is
 *   still taken over the whole strings.
 * Candidates of a term: the vocabulary terms passing the prefix rule with
 *   distance <= max_edits (the term itself at distance 0 when present), in
 *   (distance ascending, df descending, term bytes ascending) order; the first
 *   max_out (1..1024) are returned, n_within[i] counts them before truncation.
 *   df is the shard's own document frequency in that snapshot, whatever
 *   tfidf_set_global_* installed.
 * Output, CSR: term i's candidates are [cand_offsets[i], cand_offsets[i + 1]);
 *   candidate j's bytes are terms[term_offsets[j] .. term_offsets[j + 1]),
 *   with df[j] and dist[j].  cand_offsets[n_terms + 1], n_within[n_terms],
 *   *n_cands and *n_term_bytes are always written; term_offsets (cand_cap + 1
 *   entries), terms, df and dist when n_cands <= cand_cap and n_term_bytes <=
 *   terms_cap, else TFIDF_E_BUFFER.  Caps 0 with NULL payload pointers ask for
 *   the sizes.  n_terms == 0 is legal.
 * TFIDF_E_INVALID_ARG, nothing written: max_edits > 2, max_out outside
 *   1..1024, n_terms > 65536, decreasing t_offsets.  TFIDF_E_STATE before the
 *   first commit.
 * Runs on a search context beside readers, tfidf_add_docs and tfidf_commit;
 *   the reader forms see their own snapshot's vocabulary.  Scratch is bounded:
 *   the input terms are scanned in chunks that fit the kernels' staging, and a
 *   chunk whose counted candidates exceed 2^22 is filled by ranges of its
 *   terms (one term at least).  *ms_device (may be NULL): HIP-event time of
 *   the call's device work.
 * tfidf_fuzzy_terms / tfidf_reader_fuzzy_terms: the batch of one, without the
 *   two offsets arrays that one term does not need. */
int tfidf_fuzzy_terms_batch(tfidf_index *ix, const uint8_t *t_utf8, const uint64_t *t_offsets, uint32_t n_terms,
                            uint32_t max_edits, uint32_t prefix_len, uint32_t max_out, uint64_t *cand_offsets,
                            uint64_t *n_within, uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap,
                            uint32_t *df, uint8_t *dist, uint64_t cand_cap, uint64_t *n_cands,
                            uint64_t *n_term_bytes, float *ms_device);
int tfidf_reader_fuzzy_terms_batch(tfidf_reader *rd, const uint8_t *t_utf8, const uint64_t *t_offsets,
                                   uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len, uint32_t max_out,
                                   uint64_t *cand_offsets, uint64_t *n_within, uint64_t *term_offsets, uint8_t *terms,
                                   uint64_t terms_cap, uint32_t *df, uint8_t *dist, uint64_t cand_cap,
                                   uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device);
int tfidf_fuzzy_terms(tfidf_index *ix, const uint8_t *term, uint64_t len, uint32_t max_edits, uint32_t prefix_len,
                      uint32_t max_out, uint64_t *n_within, uint64_t *term_offsets, uint8_t *terms,
                      uint64_t terms_cap, uint32_t *df, uint8_t *dist, uint64_t cand_cap, uint64_t *n_cands,
                      uint64_t *n_term_bytes, float *ms_device);
int tfidf_reader_fuzzy_terms(tfidf_reader *rd, const uint8_t *term, uint64_t len, uint32_t max_edits,
                             uint32_t prefix_len, uint32_t max_out, uint64_t *n_within, uint64_t *term_offsets,
                             uint8_t *terms, uint64_t terms_cap, uint32_t *df, uint8_t *dist, uint64_t cand_cap,
                             uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device);
/* Chunks of the last fuzzy lookup that ran on this index (any form): the scans
 * of the dictionary (one per staged chunk of input terms) and the candidate
 * chunks filled and sorted (1, 1 when everything fitted; 0, 0 when no input
 * term could have candidates). */
int tfidf_last_fuzzy_chunks(const tfidf_index *ix, uint64_t *scan_chunks, uint64_t *cand_chunks);
/* ---- fuzzy search: the documents holding any near spelling of a term ----
 * (Lucene 9.8 FuzzyQuery(term, maxEdits, prefixLength, maxExpansions,
 * transpositions = true) under its default rewrite,
 * TopTermsBlendedFreqScoringRewrite, restated: DESIGN.md section 2, "Fuzzy
 * search"; parity with Lucene is not pinned by a fixture.)
 * Input, distance, prefix rule and vocabulary: those of tfidf_fuzzy_terms_batch.
 * Candidates of a term: the lookup's candidates with one more condition.  With
 *   ed the distance and m = min(code points of the candidate, code points of
 *   the term), a candidate needs m > ed (Lucene's boost would be 0 or negative
 *   otherwise; this restatement drops such terms).  n_within[i] counts them.
 * Boost: 1 when ed == 0, else 1 - (float) ed / (float) m in float arithmetic.
 * Expansion of a term: its first max_expansions (1..64; Lucene's default is
 *   50) candidates in (boost descending, lower-cased UTF-8 bytes ascending as
 *   unsigned bytes) order, selected and ordered on the device.
 * tfidf_fuzzy_expand_batch: the expansions in that order, in the CSR layout and
 *   with the size-query / TFIDF_E_BUFFER protocol of tfidf_fuzzy_terms_batch;
 *   boosts[j] is candidate j's boost, df[j] the shard's own df.
 * tfidf_search_fuzzy_batch: every hit of every term's expansion, as
 *   tfidf_search_batch_all writes hits (hit_offsets[n_terms + 1] and *n_out
 *   always, doc_ids / scores when *n_out <= cap, else TFIDF_E_BUFFER);
 *   n_expanded[i] is the size of term i's expansion.  The expansion is a flat
 *   disjunction of SHOULD term clauses, each weighted boost * idf(max df,
 *   docCount) where max df is the largest df among the expansion's terms
 *   (blended frequency) under the statistics tfidf_search would use on that
 *   snapshot; clause scores are BM25 as in tfidf_search, a document's score is
 *   their sum, the order is (score descending, doc ascending).  An expansion of
 *   the input term alone gives exactly tfidf_search(term, k = 0).
 * TFIDF_E_INVALID_ARG, nothing written: max_edits > 2, max_expansions outside
 *   1..64, n_terms > 65536, decreasing t_offsets.  TFIDF_E_STATE before the
 *   first commit.  tfidf_last_fuzzy_chunks reports for these calls too;
 *   tfidf_last_search_ms holds the last all-hits chunk's scoring and, as the
 *   total, the whole call's device time (*ms_device, may be NULL).
 * The single forms are the batch of one. */
int tfidf_fuzzy_expand_batch(tfidf_index *ix, const uint8_t *t_utf8, const uint64_t *t_offsets, uint32_t n_terms,
                             uint32_t max_edits, uint32_t prefix_len, uint32_t max_expansions, uint64_t *cand_offsets,
                             uint64_t *n_within, uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap,
                             uint32_t *df, uint8_t *dist, float *boosts, uint64_t cand_cap, uint64_t *n_cands,
                             uint64_t *n_term_bytes, float *ms_device);
int tfidf_reader_fuzzy_expand_batch(tfidf_reader *rd, const uint8_t *t_utf8, const uint64_t *t_offsets,
                                    uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len, uint32_t max_expansions,
                                    uint64_t *cand_offsets, uint64_t *n_within, uint64_t *term_offsets, uint8_t *terms,
                                    uint64_t terms_cap, uint32_t *df, uint8_t *dist, float *boosts, uint64_t cand_cap,
                                    uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device);
int tfidf_fuzzy_expand(tfidf_index *ix, const uint8_t *term, uint64_t len, uint32_t max_edits, uint32_t prefix_len,
                       uint32_t max_expansions, uint64_t *n_within, uint64_t *term_offsets, uint8_t *terms,
                       uint64_t terms_cap, uint32_t *df, uint8_t *dist, float *boosts, uint64_t cand_cap,
                       uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device);
int tfidf_reader_fuzzy_expand(tfidf_reader *rd, const uint8_t *term, uint64_t len, uint32_t max_edits,
                              uint32_t prefix_len, uint32_t max_expansions, uint64_t *n_within, uint64_t *term_offsets,
                              uint8_t *terms, uint64_t terms_cap, uint32_t *df, uint8_t *dist, float *boosts,
                              uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device);
int tfidf_search_fuzzy_batch(tfidf_index *ix, const uint8_t *t_utf8, const uint64_t *t_offsets, uint32_t n_terms,
                             uint32_t max_edits, uint32_t prefix_len, uint32_t max_expansions, uint32_t *doc_ids,
                             float *scores, uint64_t cap, uint64_t *hit_offsets, uint32_t *n_expanded, uint64_t *n_out,
                             float *ms_device);
int tfidf_reader_search_fuzzy_batch(tfidf_reader *rd, const uint8_t *t_utf8, const uint64_t *t_offsets,
                                    uint32_t n_terms, uint32_t max_edits, uint32_t prefix_len, uint32_t max_expansions,
                                    uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                    uint32_t *n_expanded, uint64_t *n_out, float *ms_device);
int tfidf_search_fuzzy(tfidf_index *ix, const uint8_t *term, uint64_t len, uint32_t max_edits, uint32_t prefix_len,
                       uint32_t max_expansions, uint32_t *doc_ids, float *scores, uint64_t cap, uint32_t *n_expanded,
                       uint64_t *n_out, float *ms_device);
int tfidf_reader_search_fuzzy(tfidf_reader *rd, const uint8_t *term, uint64_t len, uint32_t max_edits,
                              uint32_t prefix_len, uint32_t max_expansions, uint32_t *doc_ids, float *scores,
                              uint64_t cap, uint32_t *n_expanded, uint64_t *n_out, float *ms_device);
/* ---- wildcard and prefix search (Lucene's WildcardQuery / PrefixQuery; the
 * reference has no counterpart: QueryParser.escape neutralises '*' and '?';
 * DESIGN.md section 2, "Wildcard search") ----
 * Pattern: a byte string, not tokenised and not parsed as a query, decoded as
 *   strict UTF-8 into elements.  '*' matches any run of code points, the empty
 *   one included; '?' matches exactly one code point (not a byte, not a UTF-16
 *   unit); '\x' is the literal x and a trailing lone '\' a literal backslash;
 *   everything else is a literal, lower-cased per code point as the fuzzy
 *   lookup lower-cases its input.  Runs of '*' collapse to one.  An empty
 *   pattern, one that is not strict UTF-8 and one of more than 255 elements
 *   after collapsing match nothing, without failing the call.
 * Match: the whole vocabulary term (the vocabulary of the fuzzy lookup: local
 *   df >= 1, lower-cased UTF-8) matches the pattern, anchored at both ends.
 *   "abc*" is the prefix query, a pattern without '*' or '?' the exact term,
 *   "*" every term.  Leading wildcards are legal.
 * tfidf_wildcard_terms_batch (type-ahead): pattern i's matching terms in (df
 *   descending, term bytes ascending, unsigned) order, the first max_out
 *   (1..1024); n_matched[i] counts them before truncation.  df is the shard's
 *   own.  The CSR layout, the TFIDF_E_BUFFER / size-query protocol, the n_p
 *   limits (0 legal, > 65536 invalid) and TFIDF_E_STATE before the first commit
 *   are those of tfidf_fuzzy_terms_batch, without the dist array.
 * tfidf_search_wildcard_batch (the query): pattern i's hits are the live
 *   documents holding at least one matching term, doc id ascending, at
 *   doc_ids[hit_offsets[i] .. hit_offsets[i + 1]).  Every hit scores 1.0f
 *   (Lucene's constant-score rewrite of a multi-term query, boost 1), so no
 *   score array is returned.  There is no clause limit: a pattern matching the
 *   whole vocabulary returns every document that has a token.  hit_offsets[n_p
 *   + 1], n_matched[n_p] (matching terms) and *n_out are always written;
 *   doc_ids when *n_out <= cap, else TFIDF_E_BUFFER; cap 0 with NULL doc_ids
 *   asks for the sizes.  Doc ids are positions among the live documents.
 * Both run on a search context beside readers, tfidf_add_docs and
 *   tfidf_commit; the reader forms see their own snapshot.  Scratch is bounded:
 *   patterns are scanned in chunks that fit the kernels' staging, a chunk whose
 *   matches exceed 2^22 is filled by ranges of its patterns, and the union runs
 *   over ranges of patterns whose document bitmaps stay within 2^27 bits (one
 *   pattern at least); the output does not depend on the chunking.
 *   *ms_device (may be NULL): HIP-event time of the call's device work, also
 *   the total of tfidf_last_search_ms.
 * tfidf_wildcard_terms / tfidf_search_wildcard and their reader forms: the
 *   batch of one, without the offsets arrays one pattern does not need. */
int tfidf_wildcard_terms_batch(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                               uint32_t max_out, uint64_t *cand_offsets, uint64_t *n_matched, uint64_t *term_offsets,
                               uint8_t *terms, uint64_t terms_cap, uint32_t *df, uint64_t cand_cap, uint64_t *n_cands,
                               uint64_t *n_term_bytes, float *ms_device);
int tfidf_reader_wildcard_terms_batch(tfidf_reader *rd, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                                      uint32_t max_out, uint64_t *cand_offsets, uint64_t *n_matched,
                                      uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *df,
                                      uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device);
int tfidf_wildcard_terms(tfidf_index *ix, const uint8_t *pattern, uint64_t len, uint32_t max_out, uint64_t *n_matched,
                         uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *df, uint64_t cand_cap,
                         uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device);
int tfidf_reader_wildcard_terms(tfidf_reader *rd, const uint8_t *pattern, uint64_t len, uint32_t max_out,
                                uint64_t *n_matched, uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap,
                                uint32_t *df, uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes,
                                float *ms_device);
int tfidf_search_wildcard_batch(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                                uint32_t *doc_ids, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_matched,
                                uint64_t *n_out, float *ms_device);
int tfidf_reader_search_wildcard_batch(tfidf_reader *rd, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                                       uint32_t *doc_ids, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_matched,
                                       uint64_t *n_out, float *ms_device);
int tfidf_search_wildcard(tfidf_index *ix, const uint8_t *pattern, uint64_t len, uint32_t *doc_ids, uint64_t cap,
                          uint64_t *n_matched, uint64_t *n_out, float *ms_device);
int tfidf_reader_search_wildcard(tfidf_reader *rd, const uint8_t *pattern, uint64_t len, uint32_t *doc_ids,
                                 uint64_t cap, uint64_t *n_matched, uint64_t *n_out, float *ms_device);
/* Of the last wildcard call that ran on this index (any form): the scans of
 * the dictionary (one per staged chunk of patterns), the (pattern, term)
 * matches found and the union chunks (0 for the term calls). */
int tfidf_last_wildcard_stats(const tfidf_index *ix, uint64_t *scan_chunks, uint64_t *matches,
                              uint64_t *union_chunks);
/* ---- regular-expression search (Lucene's RegexpQuery; DESIGN.md section 2,
 * "Regular-expression search"; the rules and limits are csrc/regex_plan.h) ----
 * Pattern: a byte string, not tokenised and not parsed as a query, decoded as
 *   strict UTF-8 into code points and read by the grammar of Lucene 9.8 RegExp:
 *   union `|`, intersection `&`, concatenation, the repeats `? * + {n} {n,}
 *   {n,m}`, complement `~`, classes `[...]` and `[^...]` with ranges, `.` (one
 *   code point), `#` (the empty language), `@` (any string), `"..."` (literal),
 *   `()` (the empty string), groups, `\d \D \s \S \w \W` (outside brackets)
 *   and `\x` (the literal x).  `^` and `$` are literals: there are no anchors
 *   and no lazy quantifiers.  Unlike the wildcard calls the pattern is NOT
 *   lower-cased (Lucene does not lower-case it either): the vocabulary is
 *   lower-case, so "Foo.*" matches nothing.  A pattern that is not strict UTF-8
 *   matches nothing without failing the call; the empty pattern is the
 *   empty-string language and matches no term.
 * Match: the whole vocabulary term (the vocabulary of the fuzzy and wildcard
 *   calls: local df >= 1) belongs to the pattern's language, over code points.
 * Errors, with nothing written: a syntax error in any pattern (an unbalanced
 *   `(`, `[` or `"`, `{` without an integer, a dangling `\`, a repeat with
 *   nothing before it, an empty alternative, an empty class, a range that runs
 *   down) answers TFIDF_E_QUERY_SYNTAX; `<` (named automata, numeric
 *   intervals) and a pattern whose minimal DFA table exceeds 32 KiB
 *   (kRxMaxTableBytes: at least every DFA of <= 257 states and <= 32 classes)
 *   or whose compilation exceeds the work limits (Lucene's
 *   TooComplexToDeterminizeException) answer TFIDF_E_UNSUPPORTED_QUERY.
 *   tfidf_last_error carries the pattern's index and the byte offset.
 * The outputs, the CSR layouts, the TFIDF_E_BUFFER / size-query protocol, the
 *   n_p limits, TFIDF_E_STATE before the first commit, *ms_device and running
 *   beside readers, tfidf_add_docs and tfidf_commit are those of the wildcard
 *   twins: tfidf_regex_terms* return the matching terms in (df descending,
 *   bytes ascending) order, the first max_out (1..1024), n_matched before
 *   truncation; tfidf_search_regex* the live documents holding any matching
 *   term, doc id ascending, every hit the constant score 1.0f, no clause
 *   limit.  Scratch is bounded as for the wildcard calls; the patterns' tables
 *   are scanned in chunks that fit the kernels' 32 KiB staging area. */
int tfidf_regex_terms_batch(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                            uint32_t max_out, uint64_t *cand_offsets, uint64_t *n_matched, uint64_t *term_offsets,
                            uint8_t *terms, uint64_t terms_cap, uint32_t *df, uint64_t cand_cap, uint64_t *n_cands,
                            uint64_t *n_term_bytes, float *ms_device);
int tfidf_reader_regex_terms_batch(tfidf_reader *rd, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                                   uint32_t max_out, uint64_t *cand_offsets, uint64_t *n_matched,
                                   uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *df,
                                   uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device);
int tfidf_regex_terms(tfidf_index *ix, const uint8_t *pattern, uint64_t len, uint32_t max_out, uint64_t *n_matched,
                      uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint32_t *df, uint64_t cand_cap,
                      uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device);
int tfidf_reader_regex_terms(tfidf_reader *rd, const uint8_t *pattern, uint64_t len, uint32_t max_out,
                             uint64_t *n_matched, uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap,
                             uint32_t *df, uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes,
                             float *ms_device);
int tfidf_search_regex_batch(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                             uint32_t *doc_ids, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_matched,
                             uint64_t *n_out, float *ms_device);
int tfidf_reader_search_regex_batch(tfidf_reader *rd, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                                    uint32_t *doc_ids, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_matched,
                                    uint64_t *n_out, float *ms_device);
int tfidf_search_regex(tfidf_index *ix, const uint8_t *pattern, uint64_t len, uint32_t *doc_ids, uint64_t cap,
                       uint64_t *n_matched, uint64_t *n_out, float *ms_device);
int tfidf_reader_search_regex(tfidf_reader *rd, const uint8_t *pattern, uint64_t len, uint32_t *doc_ids,
                              uint64_t cap, uint64_t *n_matched, uint64_t *n_out, float *ms_device);
/* Of the last regex call that ran on this index (any form): the scans of the
 * dictionary (one per staged chunk of tables), the (pattern, term) matches
 * found, the union chunks (0 for the term calls) and the bytes of the DFA
 * tables the call staged. */
int tfidf_last_regex_stats(const tfidf_index *ix, uint64_t *scan_chunks, uint64_t *matches, uint64_t *union_chunks,
                           uint64_t *table_bytes);
/* ---- exact phrase search (no reference counterpart: Worker.java:225-227
 * escapes the quotes away; DESIGN.md section 2, "Phrase search") ----
 * The phrase bytes are analysed as a whole the way a document is (they are not
 * parsed as a query): terms t_0 .. t_{m-1}, every position increment 1.  The
 * hits are the live documents whose tokens hold the terms next to each other in
 * this order at least once; freq counts every start position (overlaps count),
 * and score = BM25 over freq with idf = the float of the sum of the positions'
 * idf (PhraseWeight / BM25Similarity.idfExplain of Lucene 9.8), on the
 * statistics tfidf_search uses.  For m = 1 the hits, order and score bits are
 * those of tfidf_search(term, k = 0).  Order: score descending, doc ascending.
 * Phrase i is p_utf8[p_offsets[i], p_offsets[i + 1]); p_offsets start at 0 and
 * never decrease.  A phrase without terms, with a term this shard lacks or that
 * is not UTF-8 has no hits; one of more than 1024 terms is TFIDF_E_INVALID_ARG
 * with nothing written.  Output in CSR like tfidf_search_batch_all:
 * hit_offsets[n_p + 1] and *n_out are always written in full, the payload
 * (doc_ids, scores, freqs) when *n_out <= cap, else TFIDF_E_BUFFER (cap = 0
 * with NULL payload pointers asks for the sizes).  The candidates (documents
 * holding every term) are found by the batched all-hits scorer and re-scanned
 * on the device; no document text crosses to the host. */
int tfidf_search_phrase_batch(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                              uint32_t *doc_ids, float *scores, uint32_t *freqs, uint64_t cap, uint64_t *hit_offsets,
                              uint64_t *n_out);
int tfidf_reader_search_phrase_batch(tfidf_reader *rd, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                                     uint32_t *doc_ids, float *scores, uint32_t *freqs, uint64_t cap,
                                     uint64_t *hit_offsets, uint64_t *n_out);
/* The batch of one phrase. */
int tfidf_search_phrase(tfidf_index *ix, const uint8_t *p, uint64_t p_len, uint32_t *doc_ids, float *scores,
                        uint32_t *freqs, uint64_t cap, uint64_t *n_out);
int tfidf_reader_search_phrase(tfidf_reader *rd, const uint8_t *p, uint64_t p_len, uint32_t *doc_ids, float *scores,
                               uint32_t *freqs, uint64_t cap, uint64_t *n_out);
/* ---- sloppy phrase search: PhraseQuery with slop > 0 (DESIGN.md section 2,
 * "Sloppy phrases") ----
 * tfidf_search_phrase_batch with a slop per phrase (slops[n_p]; values above
 * INT32_MAX behave as INT32_MAX) and a float frequency.  Analysis, candidates,
 * statistics, weight, order, limits and the output protocol are those of the
 * exact calls.  slop = 0: the exact rule, repeated terms allowed; hits, order
 * and score bits are tfidf_search_phrase_batch's, freq is the count as a float.
 * One term, any slop: the hits and score bits of tfidf_search(term, k = 0),
 * freq = tf.  slop > 0 and m >= 2: Lucene 9.8's SloppyPhraseMatcher for a
 * phrase without a repeated term: freq is the float sum, in match order, of
 * 1 / (1 + matchLength) over the matches of matchLength <= slop, the hits are
 * the candidates with freq > 0, score = weight - weight / (1 + freq *
 * cache[norm(d)]) in float.  Limits of this library: with slop > 0, a phrase
 * that repeats a term (Lucene's repeat groups are not restated) or has more
 * than 64 terms is TFIDF_E_UNSUPPORTED_QUERY with nothing written; at slop 0
 * both are served.  A NULL slops with n_p > 0 is TFIDF_E_INVALID_ARG.
 * tfidf_last_phrase_stats and tfidf_last_search_ms are set as by the exact
 * calls. */
int tfidf_search_phrase_slop_batch(tfidf_index *ix, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                   const uint32_t *slops, uint32_t n_p, uint32_t *doc_ids, float *scores, float *freqs,
                                   uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out);
int tfidf_reader_search_phrase_slop_batch(tfidf_reader *rd, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                          const uint32_t *slops, uint32_t n_p, uint32_t *doc_ids, float *scores,
                                          float *freqs, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out);
/* The batch of one phrase. */
int tfidf_search_phrase_slop(tfidf_index *ix, const uint8_t *p, uint64_t p_len, uint32_t slop, uint32_t *doc_ids,
                             float *scores, float *freqs, uint64_t cap, uint64_t *n_out);
int tfidf_reader_search_phrase_slop(tfidf_reader *rd, const uint8_t *p, uint64_t p_len, uint32_t slop,
                                    uint32_t *doc_ids, float *scores, float *freqs, uint64_t cap, uint64_t *n_out);
/* Of the last phrase search that ran on this index (any form): the (phrase,
 * document) rows that were scanned and the row chunks they ran in (test and
 * bench instruments). */
int tfidf_last_phrase_stats(const tfidf_index *ix, uint64_t *candidates, uint64_t *row_chunks);
/* ---- compound queries: MUST / SHOULD / MUST_NOT / FILTER over every query kind
 * (Lucene 9.8 BooleanQuery, flat, restated; DESIGN.md section 2, "Compound
 * queries") ----
 * A compound query is an ordered list of 0..64 clauses.  A clause has an occur
 * (TFIDF_OCCUR_*), a kind (TFIDF_CLAUSE_*), a payload byte string and the kind's
 * parameters: slop for PHRASE; max_edits, prefix_len and max_expansions for
 * FUZZY (the other fields are ignored).  A clause's row is exactly what its
 * kind's all-hits batch call returns for the payload on the same snapshot and
 * statistics: TEXT tfidf_search_batch_all (the whole grammar; a payload that does
 * not parse has an empty row), PHRASE tfidf_search_phrase_slop_batch, WILDCARD
 * and REGEX the document set with every score 1.0f, FUZZY
 * tfidf_search_fuzzy_batch.  Whatever fails that route's whole call fails this
 * one with the same code and nothing written (a regex syntax error, an
 * unsupported automaton, a sloppy phrase that repeats a term, a phrase of more
 * than 1024 terms, max_edits > 2, max_expansions outside 1..64);
 * tfidf_last_error names the query and the clause.
 * With R the MUST and FILTER clauses, N the MUST_NOT clauses and S the SHOULD
 * clauses, a document matches when it is in every row of R, in no row of N and,
 * when R is empty, in at least one row of S; a query with neither R nor S has no
 * hits.  Equal clauses are not de-duplicated.  Score: must = (float) of the
 * double sum of the MUST clauses' scores, should = (float) of the double sum of
 * the scores of the SHOULD clauses that hold the document, both in clause order;
 * must + should in one float addition when both exist, else the one that does,
 * else 0.0f (FILTER only).  FILTER and MUST_NOT scores never count.  Hits are
 * ordered by score bits descending, then doc ascending.
 * Input: the payloads in c_utf8 by c_offsets[n_clauses + 1], clauses[n_clauses],
 * and q_clause_offsets[n_q + 1] giving each query's clauses (n_clauses =
 * q_clause_offsets[n_q]).  Output protocol of tfidf_search_batch_all:
 * hit_offsets[n_q + 1] and *n_out always, the payload when *n_out <= cap, else
 * TFIDF_E_BUFFER (cap 0 with NULL payload pointers asks for the sizes).
 * ms_device (may be NULL): the call's device time, also tfidf_last_search_ms's
 * total.  TFIDF_E_INVALID_ARG with nothing written: an unknown occur or kind,
 * more than 64 clauses in a query, more than 65 536 queries or 2^20 clauses,
 * offsets that do not start at 0 or decrease, NULL arguments.  TFIDF_E_STATE
 * before the first commit.
 * The clause rows are combined on the device in chunks of whole queries whose
 * rows total at most 2^22 entries (one query at least); the result does not
 * depend on the chunking.  Out of scope: nesting, boosts, minimumShouldMatch,
 * top-k (the call returns all hits). */
#define TFIDF_OCCUR_SHOULD 0
#define TFIDF_OCCUR_MUST 1
#define TFIDF_OCCUR_MUST_NOT 2
#define TFIDF_OCCUR_FILTER 3
#define TFIDF_CLAUSE_TEXT 0
#define TFIDF_CLAUSE_PHRASE 1
#define TFIDF_CLAUSE_WILDCARD 2
#define TFIDF_CLAUSE_REGEX 3
#define TFIDF_CLAUSE_FUZZY 4
typedef struct tfidf_clause {
  uint8_t occur, kind, max_edits, max_expansions;
  uint32_t prefix_len, slop;
} tfidf_clause;
int tfidf_search_compound_batch(tfidf_index *ix, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                const tfidf_clause *clauses, const uint64_t *q_clause_offsets, uint32_t n_q,
                                uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out,
                                float *ms_device);
int tfidf_reader_search_compound_batch(tfidf_reader *rd, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                       const tfidf_clause *clauses, const uint64_t *q_clause_offsets, uint32_t n_q,
                                       uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                       uint64_t *n_out, float *ms_device);
/* The batch of one query of n_clauses clauses. */
int tfidf_search_compound(tfidf_index *ix, const uint8_t *c_utf8, const uint64_t *c_offsets,
                          const tfidf_clause *clauses, uint32_t n_clauses, uint32_t *doc_ids, float *scores,
                          uint64_t cap, uint64_t *n_out, float *ms_device);
int tfidf_reader_search_compound(tfidf_reader *rd, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                 const tfidf_clause *clauses, uint32_t n_clauses, uint32_t *doc_ids, float *scores,
                                 uint64_t cap, uint64_t *n_out, float *ms_device);
/* Of the last compound call that ran on this index (any form): the clause-row
 * entries it combined, the chunks it ran in and the (query, block) pairs of
 * those chunks (test and bench instruments). */
int tfidf_last_compound_stats(const tfidf_index *ix, uint64_t *row_entries, uint64_t *chunks, uint64_t *pairs);
/* The combine pass's own device time within the last compound call, in ms (the
 * rest of the call's device time is its clause routes'). */
int tfidf_last_compound_ms(const tfidf_index *ix, float *ms_combine);
/* ---- nested compound queries: clause groups and minimumShouldMatch (Lucene 9.8
 * BooleanQuery as a clause of a BooleanQuery, restated and evaluated as written;
 * DESIGN.md section 2, "Nested compound queries") ----
 * A query is a tree of at most 64 nodes given in pre-order.  A leaf is a clause
 * of the flat call (kind TEXT .. FUZZY, its payload and parameters) and its row
 * is that clause's row.  A group has kind TFIDF_CLAUSE_GROUP, an empty payload,
 * the nodes that name it as their parent as its children, in order, and
 * min_should_match m.  Node 0 is the root, a group whose parent is
 * TFIDF_QNODE_ROOT; every other node's parent is an earlier group node of the
 * query and its occur is the one towards that parent.  Groups sit at depths
 * 0..3 (the root is depth 0), leaves at depths 1..4.  A query of 0 nodes has no
 * hits.
 * With R a group's MUST and FILTER children, N its MUST_NOT children and S its
 * SHOULD children, a document matches the group when every R child holds it, no
 * N child holds it and at least max(m, R empty ? 1 : 0) S children hold it, a
 * leaf holding its row's documents and a group child the documents it matches;
 * the comparison is made in 32 bits, so any m > |S| matches nothing.  A group
 * without children, or with MUST_NOT children only, matches nothing.  The score
 * is the flat rule per group, a group child scoring what the rule gave it: must
 * = (float) of the double sum of the MUST children's scores, should = (float) of
 * the double sum of the scores of the SHOULD children that hold the document,
 * both in child order; must + should in one float addition, or the one that
 * exists, or 0.0f.  No rewrite is applied (no inlining of nested disjunctions,
 * no SHOULD -> MUST when m = |S|, no de-duplication).  Order: score bits
 * descending, then doc ascending.  A root with m = 0 and leaf children only
 * gives exactly the flat call's result for the same clause list.
 * Input and output follow tfidf_search_compound_batch, with nodes[n_nodes] and
 * q_node_offsets[n_q + 1] in place of the clauses (n_nodes =
 * q_node_offsets[n_q]; c_offsets has n_nodes + 1 entries, a group's payload is
 * empty).  A failing leaf route fails the call with the route's code and
 * tfidf_last_error starts with "query Q node N:".  TFIDF_E_INVALID_ARG with
 * nothing written, the error naming the query and the node: more than 65 536
 * queries, 64 nodes in a query or 2^20 nodes in a call; offsets that do not
 * start at 0 or decrease; an unknown occur or a kind above 5; a node 0 that is
 * no group or has a parent; a later node whose parent is not an earlier group
 * that is node i - 1 or one of its ancestors; a group with a payload; a group
 * deeper than 3 or a leaf deeper than 4; NULL arguments.  TFIDF_E_STATE before
 * the first commit.  tfidf_last_compound_stats and tfidf_last_compound_ms report
 * these calls as they report the flat ones.  Out of scope: boosts, top-k. */
#define TFIDF_CLAUSE_GROUP 5              /* nested calls only */
#define TFIDF_QNODE_ROOT 0xFFFFFFFFu
typedef struct tfidf_qnode {
  uint8_t occur, kind, max_edits, max_expansions;
  uint32_t prefix_len, slop;
  uint32_t parent;             /* index within the query; TFIDF_QNODE_ROOT for node 0 */
  uint32_t min_should_match;   /* groups only */
} tfidf_qnode;                 /* 20 bytes */
int tfidf_search_nested_batch(tfidf_index *ix, const uint8_t *c_utf8, const uint64_t *c_offsets,
                              const tfidf_qnode *nodes, const uint64_t *q_node_offsets, uint32_t n_q,
                              uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out,
                              float *ms_device);
int tfidf_reader_search_nested_batch(tfidf_reader *rd, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                     const tfidf_qnode *nodes, const uint64_t *q_node_offsets, uint32_t n_q,
                                     uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                     uint64_t *n_out, float *ms_device);
/* The batch of one query of n_nodes nodes. */
int tfidf_search_nested(tfidf_index *ix, const uint8_t *c_utf8, const uint64_t *c_offsets, const tfidf_qnode *nodes,
                        uint32_t n_nodes, uint32_t *doc_ids, float *scores, uint64_t cap, uint64_t *n_out,
                        float *ms_device);
int tfidf_reader_search_nested(tfidf_reader *rd, const uint8_t *c_utf8, const uint64_t *c_offsets,
                               const tfidf_qnode *nodes, uint32_t n_nodes, uint32_t *doc_ids, float *scores,
                               uint64_t cap, uint64_t *n_out, float *ms_device);
/* ---- more-like-this: documents similar to a seed document (Lucene 9.8
 * MoreLikeThis restated on the index's own forward rows; the reference stores
 * no term vectors and cannot offer it; DESIGN.md section 2, "More like this") ----
 * A seed is a committed doc id of the snapshot.  Its candidate terms are the
 * terms t of its indexed row with tf >= min_tf, df(t) >= min_df and, when
 * max_df != 0, df(t) <= max_df, where df is the shard's own df of that snapshot
 * (tfidf_set_global_* does not change the selection).  A candidate's score is
 * (float)tf * idf with idf = (float)(log((num_docs + 1) / (double)(df + 1)) +
 * 1.0) (ClassicSimilarity.idf; num_docs = the snapshot's live documents).  The
 * interesting terms are the first max_terms candidates by score bits
 * descending, then lower-cased term bytes ascending (unsigned).
 * tfidf_mlt_params_init sets Lucene's defaults: min_tf 2, min_df 5, max_df 0 (no
 * upper bound), max_terms 25; params == NULL means those.  min_tf 0 is read as
 * 1; max_terms outside 1..1024 is TFIDF_E_INVALID_ARG.
 * Seeds may repeat and come in any order; n == 0 is legal; n > 65536 or a seed
 * >= num_docs is TFIDF_E_INVALID_ARG with nothing written; TFIDF_E_STATE before
 * the first commit.  A seed that is empty, or was indexed empty (malformed
 * UTF-8), has no terms and no hits.
 *
 * tfidf_mlt_terms_batch (MoreLikeThis.retrieveInterestingTerms): CSR output.
 * term_offsets[n + 1], n_candidates[n] (the candidates before truncation),
 * *n_terms and *n_term_bytes are always written; then, in selection order,
 * blob_offsets[*n_terms + 1] into the term blob `terms`, tf, df and score per
 * term when *n_terms <= term_cap and *n_term_bytes <= terms_cap, else
 * TFIDF_E_BUFFER (caps 0 with NULL payload pointers ask for the sizes).
 *
 * tfidf_more_like_this_batch: per seed the top k (1..1024) of the disjunction
 * of its interesting terms, one SHOULD TermQuery each in selection order,
 * scored exactly as tfidf_search scores that disjunction on the snapshot (BM25
 * with the statistics in force, GLOBAL ones when set); score descending, doc
 * ascending; layout of tfidf_search_batch: doc_ids[n * k], scores[n * k],
 * counts[n].  flags & TFIDF_MLT_EXCLUDE_SEED removes the seed from its own
 * list: the list is then the top k of the other documents (k <= 1023).
 * The device reads only the seeds' rows and hands the host each seed's first
 * max_terms candidates and their score ties; no row's full term list and no
 * part of the vocabulary crosses to the host. */
typedef struct tfidf_mlt_params {
  uint32_t min_tf, min_df, max_df, max_terms;
} tfidf_mlt_params;
#define TFIDF_MLT_EXCLUDE_SEED 1u
int tfidf_mlt_params_init(tfidf_mlt_params *params);
int tfidf_mlt_terms_batch(tfidf_index *ix, const uint32_t *seeds, uint32_t n, const tfidf_mlt_params *params,
                          uint64_t *term_offsets, uint64_t *n_candidates, uint64_t *blob_offsets, uint8_t *terms,
                          uint64_t terms_cap, uint32_t *tf, uint32_t *df, float *score, uint64_t term_cap,
                          uint64_t *n_terms, uint64_t *n_term_bytes);
int tfidf_reader_mlt_terms_batch(tfidf_reader *rd, const uint32_t *seeds, uint32_t n, const tfidf_mlt_params *params,
                                 uint64_t *term_offsets, uint64_t *n_candidates, uint64_t *blob_offsets,
                                 uint8_t *terms, uint64_t terms_cap, uint32_t *tf, uint32_t *df, float *score,
                                 uint64_t term_cap, uint64_t *n_terms, uint64_t *n_term_bytes);
int tfidf_more_like_this_batch(tfidf_index *ix, const uint32_t *seeds, uint32_t n, const tfidf_mlt_params *params,
                               uint32_t k, uint32_t flags, uint32_t *doc_ids, float *scores, uint32_t *counts);
int tfidf_reader_more_like_this_batch(tfidf_reader *rd, const uint32_t *seeds, uint32_t n,
                                      const tfidf_mlt_params *params, uint32_t k, uint32_t flags, uint32_t *doc_ids,
                                      float *scores, uint32_t *counts);
/* The batch of one seed: doc_ids[k], scores[k], *count. */
int tfidf_more_like_this(tfidf_index *ix, uint32_t seed, const tfidf_mlt_params *params, uint32_t k, uint32_t flags,
                         uint32_t *doc_ids, float *scores, uint32_t *count);
int tfidf_reader_more_like_this(tfidf_reader *rd, uint32_t seed, const tfidf_mlt_params *params, uint32_t k,
                                uint32_t flags, uint32_t *doc_ids, float *scores, uint32_t *count);
/* Of the last more-like-this call that ran on this index (any form): the
 * forward-row entries the device scanned (the seeds' distinct terms, a repeated
 * seed counted again) and the candidate chunks filled and sorted (test and
 * bench instruments).  tfidf_last_search_ms then holds the last scoring chunk
 * and, as the total, the whole call's device time. */
int tfidf_last_mlt_stats(const tfidf_index *ix, uint64_t *row_entries_scanned, uint64_t *cand_chunks);
/* Per-query device time of the last search call on this index (HIP events on the search's stream);
 * after a phrase search: the last conjunction chunk's scoring, and the whole call as the total. */
int tfidf_last_search_ms(const tfidf_index *ix, float *ms_scoring, float *ms_total);
/* Device-time measurement of searches (HIP events around scoring; on by
 * default).  Off for serving: the three event records cost ~17 us per single
 * query (cfg 2: 72 -> 55 us p50); tfidf_last_search_ms then reports -1. */
int tfidf_set_query_timing(tfidf_index *ix, int on);

/* ---- device-resident results (multi-GPU orchestration; no reference
 * counterpart: they feed the RCCL all-gather that replaces Leader.java:51-70) ----
 * Merge keys: (float32 score bits << 32) | ~(doc_base + doc) as u64 — BM25
 * scores are > 0, so descending key order is (score desc, doc asc); 0 = empty.
 * tfidf_search_batch_keys_device: n_q x k keys into caller device memory
 *   (a query that does not parse has none).
 * tfidf_search_all_keys_device: every hit of one query, ordered, into caller
 *   device memory of cap >= num_docs keys; *n_out = hits.
 * Both return after the keys are written (the index's stream is synchronised). */
int tfidf_search_batch_keys_device(tfidf_index *ix, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                   uint32_t k, uint64_t doc_base, void *d_keys);
int tfidf_search_all_keys_device(tfidf_index *ix, const uint8_t *q, uint64_t q_len, uint64_t doc_base, void *d_keys,
                                 uint64_t cap, uint64_t *n_out);
/* Issue the index's device work on the caller's stream (a hipStream_t, e.g.
 * torch.cuda.current_stream().cuda_stream), or back on the index's own stream
 * with TFIDF_OWN_STREAM.  With a caller's stream the writers (commit,
 * compaction, the GLOBAL exchange) and every search and reader run on it.
 * NULL is the legacy default stream for the writers only: searches and
 * readers keep their contexts' own streams, as under TFIDF_OWN_STREAM.
 * Pending work on the previous stream is finished first. */
#define TFIDF_OWN_STREAM ((void *)-1)
int tfidf_set_stream(tfidf_index *ix, void *stream);

int tfidf_doc_key(const tfidf_index *ix, uint64_t doc, uint8_t *buf, uint64_t cap, uint64_t *n_out);
/* Every committed document's key (Worker.java:214 StringField "path"), in doc
 * order: bytes concatenated into buf, offsets[num_docs + 1]; TFIDF_E_BUFFER with
 * *n_bytes = size needed when cap is too small.  num_docs is that of the
 * snapshot published at the call: beside concurrent commits, size offsets from
 * a reader (tfidf_reader_doc_keys). */
int tfidf_doc_keys(const tfidf_index *ix, uint8_t *buf, uint64_t cap, uint64_t *offsets, uint64_t *n_bytes);
int tfidf_doc_len(tfidf_index *ix, uint64_t doc, uint32_t *len, uint8_t *norm);
/* Documents of the last commit whose bytes are not valid UTF-8 (where the
 * reference's Files.readString throws MalformedInputException and Tika
 * extracts the text instead, Worker.java:199-211): they are indexed as empty
 * documents (no tokens, norm 0) rather than failing the commit.  Committed doc
 * ids, ascending; *n_out = count (TFIDF_E_BUFFER if cap is too small).  A
 * caller with a text extractor re-adds the extracted text under the same key
 * (replace-by-key) and commits again. */
int tfidf_malformed_docs(const tfidf_index *ix, uint64_t *docs, uint64_t cap, uint64_t *n_out);
/* Distinct terms of one document: NUL-separated strings (sorted by bytes) + tf. */
int tfidf_doc_terms(tfidf_index *ix, uint64_t doc, char *terms, uint64_t terms_cap, uint32_t *tfs,
                    uint64_t cap, uint64_t *n_out);
int tfidf_term_df(tfidf_index *ix, const uint8_t *term, uint64_t len, uint64_t *df_local,
                  uint64_t *df_effective);

/* ---- GLOBAL statistics across shards (no reference counterpart) ----
 * Term-ownership exchange (used by the multi-GPU orchestration; O(vocabulary)
 * per rank, no sort).  With a caller's stream (tfidf_set_stream: the
 * collective stream) the three device calls are ASYNCHRONOUS on it: the
 * caller's device buffers must stay allocated until that stream reaches the
 * work (true when they come from an allocator that orders them on that
 * stream, as torch's caching allocator does), and the exchange needs one host
 * read — the split sizes.  On the index's own stream each call returns after
 * its device work is done, so the buffers may be freed as soon as it returns.
 * 1. tfidf_vocab_partition_device: this shard's vocabulary as records
 *    (lo, hi, df: 3 x u64 each) grouped by owner rank (a hash of the term key
 *    mod n_ranks) into d_records; d_counts (device, n_ranks x u64) = records
 *    per owner; *n_out = records (the shard's vocabulary size, host-known).
 * 2. caller all-to-alls the records to their owners (RCCL), then the owner
 *    calls tfidf_vocab_reduce_device on everything it received: d_df_out
 *    (u32 per record, same order) = df summed over identical terms;
 *    d_n_unique (device u64, may be NULL) = distinct terms this rank owns.
 * 3. caller all-to-alls the answers back (reverse split sizes), sums
 *    {doc_count, sum_ttf} over ranks, and tfidf_set_global_df_device imports
 *    the answers (in the record order step 1 produced); its host mirror is
 *    copied in the background and waited for by the next search.
 * Canonical-vocabulary form (sorted union; kept for tools and tests):
 * 1. tfidf_vocab_export_device: this shard's term keys (16 B each, sorted
 *    ascending as (hi, lo)) and local df into caller device buffers.
 * 2. caller all-gathers the key lists (RCCL), then
 *    tfidf_vocab_canonicalize_device: sorted union of all shards' keys ->
 *    canonical term ids; fills d_df_canonical (u32[n_canonical]) with this
 *    shard's df in canonical order (zero elsewhere).
 * 3. caller all-reduces d_df_canonical and {doc_count, sum_ttf} (RCCL SUM), then
 *    tfidf_set_global_stats_device imports them. */
int tfidf_vocab_partition_device(tfidf_index *ix, uint32_t n_ranks, void *d_records, uint64_t cap, void *d_counts,
                                 uint64_t *n_out);
int tfidf_vocab_reduce_device(tfidf_index *ix, const void *d_records, uint64_t n, void *d_df_out, void *d_n_unique);
int tfidf_set_global_df_device(tfidf_index *ix, const void *d_df, uint64_t n, uint64_t doc_count,
                               uint64_t sum_ttf);
int tfidf_vocab_size(const tfidf_index *ix, uint64_t *n);
/* Host copy of this shard's vocabulary with the statistics in force: term
 * keys (lo, hi: 2 x u64 each, sorted ascending as (hi, lo)), the shard's own
 * docFreq and the effective one (the GLOBAL df after an exchange, else the
 * shard's own).  Any output may be NULL; *n_out = the vocabulary size
 * (TFIDF_E_BUFFER if it exceeds cap). */
int tfidf_vocab_export(tfidf_index *ix, uint64_t *keys, uint32_t *df_local, uint32_t *df_effective, uint64_t cap,
                       uint64_t *n_out);
int tfidf_vocab_export_device(tfidf_index *ix, void *d_keys, void *d_df, uint64_t cap, uint64_t *n_out);
int tfidf_vocab_canonicalize_device(tfidf_index *ix, const void *d_all_keys, uint64_t n_all,
                                    void *d_df_canonical, uint64_t cap, uint64_t *n_canonical);
int tfidf_set_global_stats_device(tfidf_index *ix, const void *d_df_canonical, uint64_t n_canonical,
                                  uint64_t doc_count, uint64_t sum_ttf);
/* Host-buffer form of the same import: df for arbitrary keys (2 x u64 per key: lo, hi). */
int tfidf_set_global_stats(tfidf_index *ix, const uint64_t *keys_lohi, const uint64_t *df, uint64_t n,
                           uint64_t doc_count, uint64_t sum_ttf);
int tfidf_clear_global_stats(tfidf_index *ix);

/* Term key of an analysed (lower-cased) token, as the device computes it. */
int tfidf_term_key(const uint8_t *term, uint64_t len, uint64_t *lo, uint64_t *hi);

/* StandardAnalyzer (Worker.java:71,225: StandardTokenizer + LowerCaseFilter,
 * full Unicode, maxTokenLength 255) on the host, the same scanner the index
 * build runs on the device: NUL-terminated lower-cased UTF-8 tokens in order.
 * TFIDF_E_BUFFER with *n_bytes = size needed when cap is too small;
 * TFIDF_E_UNSUPPORTED_INPUT for malformed UTF-8. */
int tfidf_analyze(const uint8_t *text, uint64_t len, char *out, uint64_t cap, uint64_t *n_tokens,
                  uint64_t *n_bytes);

/* Leader.start merge (Leader.java:73-88): names (concatenated, offsets[n+1])
 * with double scores in worker-response order -> distinct names sorted by
 * String.compareTo (UTF-16 code units) with Double::sum totals.  out_first[i]
 * = index of the first occurrence of the i-th distinct name.  n_out = #distinct. */
int tfidf_leader_merge(const uint8_t *names, const uint64_t *offsets, uint64_t n, const double *scores,
                       uint64_t *out_first, double *out_sum, uint64_t *n_out);
/* Stable permutation of n UTF-8 names in String.compareTo (UTF-16) order (the
 * TreeMap order of Leader.java:80-88; the multi-GPU name table). */
int tfidf_sort_names(const uint8_t *names, const uint64_t *offsets, uint64_t n, uint64_t *perm);

/* ==========================================================================
 * Node level: documents sharded over GPUs, one shard (tfidf_index) per GPU.
 *
 * Replaces the reference's fan-out + merge, Leader.java:39-92 (POST
 * {worker}/worker/process to every registered worker, :51-70; merge by name,
 * :73-88) over each worker's Worker.java:222-241 searchIndex, with
 * collectives between the shards (RCCL over xGMI on one MI355X node):
 *   GLOBAL statistics (cfg.stats_mode TFIDF_STATS_GLOBAL: the reference's
 *     1-worker results on a sharded corpus): per commit, each term's (key, df)
 *     records go to an owner rank (all-to-all), the owner sums df and answers
 *     (all-to-all back); docCount / sumTotalTermFreq summed; per query, every
 *     shard's top-k as merge keys, all-gathered and merged on the device.
 *     Global doc id = shard base + local id (contiguous shards): (score desc,
 *     doc asc) is the single-index order.  At most 2^32 documents per node.
 *   SHARD statistics (TFIDF_STATS_SHARD: the reference's N-worker results):
 *     every shard scores with its own statistics and returns ALL its hits;
 *     the hits are summed per document name in double in rank (= worker
 *     response) order (HashMap.merge Double::sum, Leader.java:73-77) and
 *     ordered by String.compareTo (TreeMap, :80-88).
 *
 * Two process models, one orchestration (the code below the ABI is the same):
 *   (1) tfidf_node: ONE process owns every GPU of a device list (SURVEY §8b:
 *       "one JVM owns all 8 GPUs"); one host thread per shard; collectives
 *       over an RCCL communicator of the devices (ncclCommInitAll), or an
 *       in-process host transport when a device repeats (tests) or
 *       TFIDF_NODE_INPROC is asked for.
 *   (2) SPMD, one process per GPU: each rank creates its own tfidf_index and a
 *       tfidf_comm (built-in RCCL from a unique id the caller broadcasts, or
 *       the caller's own collectives through tfidf_collectives), and calls the
 *       tfidf_dist_* functions collectively (every rank, same order).
 * ========================================================================== */
typedef struct tfidf_comm tfidf_comm;
typedef struct tfidf_node tfidf_node;

#define TFIDF_COLL_HOST 0    /* collective buffers are host memory (gloo / MPI / sockets ...) */
#define TFIDF_COLL_DEVICE 1  /* device memory of the rank's GPU, ordered on `stream` (a hipStream_t) */

/* Caller-supplied collectives (the transport of process model (2) when the
 * built-in RCCL communicator is not used).  Each returns 0 on success.
 *   all_gather   : recv[r * bytes .. (r + 1) * bytes) = rank r's send, bytes each
 *   all_to_all_v : send_bytes[r] bytes at send + send_offs[r] go to rank r;
 *                  recv_bytes[r] bytes from rank r land at recv + recv_offs[r]
 * Buffers may be NULL when their byte counts are 0.  With TFIDF_COLL_DEVICE the
 * call may be asynchronous on `stream`; with TFIDF_COLL_HOST it must be complete
 * on return. */
typedef struct tfidf_collectives {
  void *ctx;
  int32_t memory;              /* TFIDF_COLL_HOST or TFIDF_COLL_DEVICE */
  int (*all_gather)(void *ctx, const void *send, void *recv, uint64_t bytes, void *stream);
  int (*all_to_all_v)(void *ctx, const void *send, const uint64_t *send_bytes, const uint64_t *send_offs,
                      void *recv, const uint64_t *recv_bytes, const uint64_t *recv_offs, void *stream);
} tfidf_collectives;

/* A communicator over the caller's collectives (the table is copied). */
int tfidf_comm_create(int32_t rank, int32_t world, const tfidf_collectives *coll, tfidf_comm **out);
/* Built-in RCCL communicator (librccl of the HIP runtime the library runs on,
 * loaded at first use): rank 0 calls tfidf_rccl_unique_id, the caller sends the
 * 128 bytes to every rank (its own channel), then every rank calls
 * tfidf_comm_init_rccl with its rank and GPU (collective). */
int tfidf_rccl_unique_id(uint8_t id[128]);
int tfidf_comm_init_rccl(const uint8_t id[128], int32_t rank, int32_t world, int32_t device, tfidf_comm **out);
/* `world` communicators of one process sharing an in-process host transport
 * (comms[0 .. world-1], rank i = comms[i]); each rank's calls run on its own
 * thread.  The transport tfidf_node uses when shards share a device. */
int tfidf_comm_create_inproc(int32_t world, tfidf_comm **comms);
int tfidf_comm_destroy(tfidf_comm *c);
int tfidf_comm_info(const tfidf_comm *c, int32_t *rank, int32_t *world, int32_t *transport);
#define TFIDF_TRANSPORT_CALLBACK 0
#define TFIDF_TRANSPORT_RCCL 1
#define TFIDF_TRANSPORT_INPROC 2
/* Transport check (no index needed): an all-gather of each rank's id and an
 * all-to-all-v of rank-tagged bytes through the communicator, verified on
 * every rank.  Collective. */
int tfidf_comm_selftest(tfidf_comm *c);

/* ---- process model (2): per-rank calls, collective over the communicator ----
 * Every rank calls each of them, in the same order, after its own
 * tfidf_commit; a rank that cannot serve still takes part.  Its status rides in
 * the first collective of the call (a header ahead of its top-k keys, or the
 * count row of a variable-length gather), so no rank is left waiting:
 *   commits and GLOBAL searches: every rank returns the failing rank's error
 *     together (TFIDF_E_STATE for an index not committed, or re-committed since
 *     the last tfidf_dist_global_commit; TFIDF_E_INVALID_ARG when two ranks'
 *     [doc_base, doc_base + num_docs) ranges overlap: merge keys would collide);
 *   SHARD searches: the other ranks' hits are merged without the failing rank
 *     (Leader.start skips a failed worker, Leader.java:67-69): TFIDF_OK, the
 *     skipped ranks in tfidf_dist_last_failed and a tfidf_last_error() message
 *     naming them; only when no rank can serve is the error returned.  A rank
 *     whose index was re-committed after tfidf_dist_shard_commit is skipped.
 * A query that does not parse
 * (TFIDF_E_QUERY_SYNTAX / _UNSUPPORTED_QUERY) fails on every rank alike before
 * any collective (the reference's Worker answers [] and its Leader merges
 * nothing, Worker.java:182-185).
 *
 * tfidf_dist_global_commit: GLOBAL statistics (term ownership); the shards
 *   whose commits hashed long / non-ASCII terms with different seeds first agree
 *   on the highest attempt (the others re-commit under it).  Outputs may be
 *   NULL (n_vocab = distinct terms over all shards: one more collective).
 * tfidf_dist_search: k >= 1 top-k, or k == 0 every hit, with global doc ids
 *   (doc_base = this shard's first global id); *n_out = hits; TFIDF_E_BUFFER if
 *   they exceed cap (the first cap are written; the whole list stays readable
 *   through tfidf_dist_last_hits, no collective).
 * tfidf_dist_search_batch: n_q queries, 1 <= k <= 1024, outputs n_q x k.
 * tfidf_dist_shard_commit: SHARD mode name table (every rank's document keys,
 *   sorted by String.compareTo, de-duplicated); *n_names may be NULL.
 * tfidf_dist_shard_search: Leader.start over the ranks: *n_out distinct names,
 *   *n_bytes of name text; read them with tfidf_dist_last_names. */
int tfidf_dist_global_commit(tfidf_index *ix, tfidf_comm *c, uint64_t *n_vocab, uint64_t *doc_count,
                             uint64_t *sum_ttf);
int tfidf_dist_search(tfidf_index *ix, tfidf_comm *c, uint64_t doc_base, const uint8_t *q, uint64_t q_len,
                      uint32_t k, uint64_t *doc_ids, float *scores, uint64_t cap, uint64_t *n_out);
int tfidf_dist_search_batch(tfidf_index *ix, tfidf_comm *c, uint64_t doc_base, const uint8_t *q_utf8,
                            const uint64_t *q_offsets, uint32_t n_q, uint32_t k, uint64_t *doc_ids, float *scores,
                            uint32_t *counts);
int tfidf_dist_shard_commit(tfidf_index *ix, tfidf_comm *c, uint64_t *n_names);
int tfidf_dist_shard_search(tfidf_index *ix, tfidf_comm *c, const uint8_t *q, uint64_t q_len, uint64_t *n_out,
                            uint64_t *n_bytes);
/* All-hits batches (Worker.java:230 for a batch of requests, over the ranks).
 * tfidf_dist_search_batch_all (GLOBAL): tfidf_search_batch_all's contract with
 *   global doc ids: query i's hits are doc_ids/scores[hit_offsets[i] ..
 *   hit_offsets[i+1]) in (score desc, doc asc) order over all ranks;
 *   hit_offsets (n_q + 1 entries) and *n_out are always written in full;
 *   TFIDF_E_BUFFER when the total exceeds cap (nothing is promised about
 *   doc_ids / scores then).  A query that does not parse has no hits and does
 *   not fail the batch.  Collective: every rank takes part in every collective
 *   whatever its own cap; a rank called with cap == 0 gets the offsets only
 *   (no result merge, no copy-out).  The first collective carries every rank's
 *   status and per-query hit bounds: a stale GLOBAL generation fails on every
 *   rank with TFIDF_E_STATE, overlapping doc ranges with TFIDF_E_INVALID_ARG,
 *   as tfidf_dist_search.  The batch is served in node chunks of queries whose
 *   boundaries every rank derives from the gathered bounds alone; each chunk's
 *   count row carries the rank's status, so a rank that fails inside a chunk
 *   (TFIDF_E_HIP, TFIDF_E_OOM) fails the call on every rank at that chunk.
 * tfidf_dist_shard_search_batch (SHARD): tfidf_dist_shard_search's result for
 *   each query (distinct names in String.compareTo order, each the double sum
 *   of its hits' float scores in rank order), searched once; *n_out names in
 *   all, *n_bytes of name text.  tfidf_dist_last_names_batch reads what the
 *   communicator kept (no collective, no second search): the names of all
 *   queries concatenated, query i's entries [name_offsets[i], name_offsets[i+1]).
 *   A rank that cannot serve at the first collective is skipped for the whole
 *   batch (tfidf_dist_last_failed); one that fails inside a chunk fails the
 *   call on every rank together.  A query that does not parse has no names. */
int tfidf_dist_search_batch_all(tfidf_index *ix, tfidf_comm *c, uint64_t doc_base, const uint8_t *q_utf8,
                                const uint64_t *q_offsets, uint32_t n_q, uint64_t *doc_ids, float *scores,
                                uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out);
int tfidf_dist_shard_search_batch(tfidf_index *ix, tfidf_comm *c, const uint8_t *q_utf8, const uint64_t *q_offsets,
                                  uint32_t n_q, uint64_t *n_out, uint64_t *n_bytes);
int tfidf_dist_last_names_batch(const tfidf_comm *c, uint8_t *buf, uint64_t cap, uint64_t *offsets, double *scores,
                                uint64_t n_cap, uint64_t *name_offsets /* n_q + 1 */, uint64_t *n_out,
                                uint64_t *n_bytes);
/* Results of the communicator's last search (local copies, no collective). */
int tfidf_dist_last_hits(const tfidf_comm *c, uint64_t *doc_ids, float *scores, uint64_t cap, uint64_t *n_out);
/* Ranks skipped by the last SHARD search (bit r = rank r; 0 = every rank answered). */
int tfidf_dist_last_failed(const tfidf_comm *c, uint64_t *rank_mask);
/* names concatenated into buf (cap bytes), offsets[n + 1], scores[n] (double sums) */
int tfidf_dist_last_names(const tfidf_comm *c, uint8_t *buf, uint64_t cap, uint64_t *offsets, double *scores,
                          uint64_t n_cap, uint64_t *n_out, uint64_t *n_bytes);

/* ---- process model (1): one process, one shard per GPU of a device list ----
 * cfg applies to every shard (cfg->device is ignored; cfg->stats_mode selects
 * GLOBAL or SHARD results).  tfidf_node_create: the devices of device_mask (bit
 * i = HIP device i).  tfidf_node_create_devices: an explicit list (a repeated
 * device forces the in-process transport). */
#define TFIDF_NODE_INPROC 1u   /* flags: in-process host transport instead of RCCL */
int tfidf_node_create(const tfidf_config *cfg, uint64_t device_mask, tfidf_node **out);
int tfidf_node_create_devices(const tfidf_config *cfg, const int32_t *devices, uint32_t n_devices, uint32_t flags,
                              tfidf_node **out);
int tfidf_node_destroy(tfidf_node *n);
/* shard i's index (owned by the node): per-shard calls such as tfidf_add_docs_device.
 * A shard changed or committed through this handle needs tfidf_node_commit
 * again: until then GLOBAL searches fail (TFIDF_E_STATE) and SHARD searches
 * skip that shard. */
int tfidf_node_shard(tfidf_node *n, uint32_t i, tfidf_index **ix, uint32_t *n_shards);
/* Documents go to one shard (shard >= 0: the caller routes, as Leader.upload
 * picks a worker, Leader.java:153-207) or are split contiguously over the shards
 * (shard == -1).  Replace-by-key applies within a shard. */
int tfidf_node_add_docs(tfidf_node *n, int32_t shard, const uint8_t *utf8, const uint64_t *offsets, uint64_t n_docs,
                        const uint8_t *keys, const uint64_t *key_offsets);
/* Commits every shard (in parallel), then GLOBAL statistics or the SHARD name table. */
int tfidf_node_commit(tfidf_node *n);
/* tfidf_delete_docs on one shard (shard >= 0) or on every shard (shard == -1:
 * a name can live on several shards, as with Leader-routed uploads); *n_deleted
 * (may be NULL) is summed over the shards.  tfidf_node_compact: tfidf_compact on
 * every shard, in parallel; *bytes_reclaimed (may be NULL) summed.  Both only
 * stage changes: the node serves its last tfidf_node_commit until the next one. */
int tfidf_node_delete_docs(tfidf_node *n, int32_t shard, const uint8_t *keys, const uint64_t *key_offsets,
                           uint64_t n_keys, uint64_t *n_deleted);
int tfidf_node_compact(tfidf_node *n, uint64_t *bytes_reclaimed);
/* GLOBAL mode; same results as tfidf_dist_search / _batch (global doc ids). */
int tfidf_node_search(tfidf_node *n, const uint8_t *q, uint64_t q_len, uint32_t k, uint64_t *doc_ids, float *scores,
                      uint64_t cap, uint64_t *n_out);
int tfidf_node_search_batch(tfidf_node *n, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q, uint32_t k,
                            uint64_t *doc_ids, float *scores, uint32_t *counts);
/* SHARD mode (Leader.start): name-ordered {name: double} of the merged hits.
 * A shard that cannot serve is skipped (Leader.java:67-69): TFIDF_OK with the
 * other shards' merged hits, tfidf_node_last_failed names the skipped shards
 * and tfidf_last_error() their reasons. */
int tfidf_node_search_names(tfidf_node *n, const uint8_t *q, uint64_t q_len, uint8_t *buf, uint64_t cap,
                            uint64_t *offsets, double *scores, uint64_t n_cap, uint64_t *n_out, uint64_t *n_bytes);
/* All-hits batches over the node's shards: tfidf_dist_search_batch_all (GLOBAL
 * mode) and tfidf_dist_shard_search_batch (SHARD mode) run on every shard at
 * once; shard 0 delivers.  tfidf_node_search_names_batch searches once and
 * reports the sizes; tfidf_node_last_names_batch then reads the kept result
 * (TFIDF_E_BUFFER with the sizes when a buffer is too small). */
int tfidf_node_search_batch_all(tfidf_node *n, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                uint64_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                uint64_t *n_out);
int tfidf_node_search_names_batch(tfidf_node *n, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                                  uint64_t *n_out, uint64_t *n_bytes);
int tfidf_node_last_names_batch(const tfidf_node *n, uint8_t *buf, uint64_t cap, uint64_t *offsets, double *scores,
                                uint64_t n_cap, uint64_t *name_offsets /* n_q + 1 */, uint64_t *n_out,
                                uint64_t *n_bytes);
/* Shards skipped by the last tfidf_node_search_names / _names_batch (bit g = shard g). */
int tfidf_node_last_failed(const tfidf_node *n, uint64_t *shard_mask);
/* Global doc id -> its document key (Worker.java:235-236, across shards). */
int tfidf_node_doc_key(tfidf_node *n, uint64_t doc, uint8_t *buf, uint64_t cap, uint64_t *n_out);
/* tfidf_matches_batch / tfidf_snippets_batch over the node: docs are global
 * doc ids (what the node's searches return).  After tfidf_node_commit, in
 * either statistics mode.  Each row is routed to its shard as
 * tfidf_node_doc_key routes it; every shard runs one batch of its own rows
 * (query grouping and order kept) at once, and the results come back in the
 * caller's row order with the offsets recomputed.  A global id >= the node's
 * num_docs: TFIDF_E_INVALID_ARG, nothing written.  A shard's failure fails the
 * call with that shard's code (no partial answer).  Everything else (results,
 * queries that do not parse, buffer protocol) as in the single-index batch
 * form; *ms_device is the largest of the shards' device times. */
int tfidf_node_matches_batch(tfidf_node *n, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                             const uint64_t *docs, const uint64_t *doc_offsets, uint64_t *starts, uint32_t *lens,
                             uint32_t *ordinals, uint64_t cap, uint64_t *match_offsets, uint64_t *n_out,
                             float *ms_device);
int tfidf_node_snippets_batch(tfidf_node *n, const uint8_t *q_utf8, const uint64_t *q_offsets, uint32_t n_q,
                              const uint64_t *docs, const uint64_t *doc_offsets, uint32_t max_bytes, uint8_t *text,
                              uint64_t text_cap, uint64_t *text_offsets, uint64_t *doc_starts, uint64_t *starts,
                              uint32_t *lens, uint32_t *ordinals, uint64_t m_cap, uint64_t *match_offsets,
                              uint64_t *n_text, uint64_t *n_matches, float *ms_device);
/* tfidf_fuzzy_terms_batch over the node, after tfidf_node_commit: every shard
 * runs the batch at once on its own device, untruncated, and the host merges
 * the shards' candidates by term bytes: df is the sum over the shards (u64
 * here), n_within counts the distinct terms, the order and max_out apply to
 * the merged lists.  A shard's failure fails the call with that shard's code.
 * *ms_device is the largest of the shards' device times. */
int tfidf_node_fuzzy_terms_batch(tfidf_node *n, const uint8_t *t_utf8, const uint64_t *t_offsets, uint32_t n_terms,
                                 uint32_t max_edits, uint32_t prefix_len, uint32_t max_out, uint64_t *cand_offsets,
                                 uint64_t *n_within, uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap,
                                 uint64_t *df, uint8_t *dist, uint64_t cand_cap, uint64_t *n_cands,
                                 uint64_t *n_term_bytes, float *ms_device);
/* tfidf_search_fuzzy_batch over the node, after tfidf_node_commit, in both
 * statistics modes: every shard with documents expands each term over its own
 * vocabulary (as a searcher per shard would), blends with the df of the
 * statistics in force and returns its hits; ids become global by the shard's
 * doc_base (u64 here) and the host merges each term's lists by (score
 * descending, global id ascending).  n_expanded[i] is the sum of the shards'
 * expansion sizes.  A shard's failure fails the call with that shard's code.
 * *ms_device is the largest of the shards' device times. */
int tfidf_node_search_fuzzy_batch(tfidf_node *n, const uint8_t *t_utf8, const uint64_t *t_offsets, uint32_t n_terms,
                                  uint32_t max_edits, uint32_t prefix_len, uint32_t max_expansions, uint64_t *doc_ids,
                                  float *scores, uint64_t cap, uint64_t *hit_offsets, uint32_t *n_expanded,
                                  uint64_t *n_out, float *ms_device);
/* The wildcard calls over the node, after tfidf_node_commit, in both
 * statistics modes: every shard with documents runs the batch at once on its
 * own device.  Terms are merged as tfidf_node_fuzzy_terms_batch merges them
 * (df summed over the shards, u64 here; n_matched counts the distinct terms;
 * the order and max_out apply to the merged lists).  Hit ids become global by
 * the shard's doc_base; shards are contiguous, so a pattern's list is the
 * shards' lists in shard order (u64 ids), and n_matched counts the distinct
 * matching terms.  A shard's failure fails the call with that shard's code.
 * *ms_device is the largest of the shards' device times. */
int tfidf_node_wildcard_terms_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                                    uint32_t max_out, uint64_t *cand_offsets, uint64_t *n_matched,
                                    uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint64_t *df,
                                    uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device);
int tfidf_node_search_wildcard_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                                     uint64_t *doc_ids, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_matched,
                                     uint64_t *n_out, float *ms_device);
/* The regex calls over the node: the shard merge of the wildcard node calls
 * (df summed over the shards, distinct n_matched, global doc ids).  A pattern
 * in error fails the call before any shard runs. */
int tfidf_node_regex_terms_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                                 uint32_t max_out, uint64_t *cand_offsets, uint64_t *n_matched,
                                 uint64_t *term_offsets, uint8_t *terms, uint64_t terms_cap, uint64_t *df,
                                 uint64_t cand_cap, uint64_t *n_cands, uint64_t *n_term_bytes, float *ms_device);
int tfidf_node_search_regex_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                                  uint64_t *doc_ids, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_matched,
                                  uint64_t *n_out, float *ms_device);
/* tfidf_search_phrase_batch over the node, after tfidf_node_commit, in both
 * statistics modes: every shard with documents runs the batch at once on its
 * own device, doc_ids become global by the shard's doc_base, and the host
 * merges each phrase's ordered lists by (score descending, global id
 * ascending); the shards' scores are comparable in GLOBAL mode by
 * construction.  A shard's failure fails the call with that shard's code. */
int tfidf_node_search_phrase_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets, uint32_t n_p,
                                   uint64_t *doc_ids, float *scores, uint32_t *freqs, uint64_t cap,
                                   uint64_t *hit_offsets, uint64_t *n_out);
/* tfidf_search_phrase_slop_batch over the node, as tfidf_node_search_phrase_batch. */
int tfidf_node_search_phrase_slop_batch(tfidf_node *n, const uint8_t *p_utf8, const uint64_t *p_offsets,
                                        const uint32_t *slops, uint32_t n_p, uint64_t *doc_ids, float *scores,
                                        float *freqs, uint64_t cap, uint64_t *hit_offsets, uint64_t *n_out);
/* tfidf_more_like_this_batch over the node, after tfidf_node_commit, in both
 * statistics modes.  Seeds are global ids, routed by doc_base as
 * tfidf_node_doc_key routes them; one >= the node's num_docs is
 * TFIDF_E_INVALID_ARG with nothing written.  The shard that owns a seed selects
 * its interesting terms by its own df and num_docs; the term strings go to every
 * shard with documents, which looks them up in its own dictionary (a term it
 * lacks has no scorer), scores the disjunction with its statistics in force
 * and returns its top k (k + 1 when excluding); the host merges per seed by
 * (score descending, global id ascending), drops the seed when asked and
 * truncates to k.  doc_ids[n * k], scores[n * k], counts[n].  A shard's failure
 * fails the call with that shard's code. */
int tfidf_node_more_like_this_batch(tfidf_node *n, const uint64_t *seeds, uint32_t n_seeds,
                                    const tfidf_mlt_params *params, uint32_t k, uint32_t flags, uint64_t *doc_ids,
                                    float *scores, uint32_t *counts);
/* tfidf_search_compound_batch over the node, after tfidf_node_commit, in both
 * statistics modes: every shard with documents runs the batch at once on its own
 * device (wildcard, regex and fuzzy clauses expand on the shard's own
 * vocabulary, as their node routes do), doc_ids become global by the shard's
 * doc_base, and the host merges each query's ordered lists by (score
 * descending, global id ascending).  A shard's failure fails the call with that
 * shard's code. */
int tfidf_node_search_compound_batch(tfidf_node *n, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                     const tfidf_clause *clauses, const uint64_t *q_clause_offsets, uint32_t n_q,
                                     uint64_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                     uint64_t *n_out, float *ms_device);
/* tfidf_search_nested_batch over the node, built exactly as
 * tfidf_node_search_compound_batch: every shard runs the batch, the host merges
 * by (score bits descending, global id ascending), a shard's failure fails the
 * call with that shard's code. */
int tfidf_node_search_nested_batch(tfidf_node *n, const uint8_t *c_utf8, const uint64_t *c_offsets,
                                   const tfidf_qnode *nodes, const uint64_t *q_node_offsets, uint32_t n_q,
                                   uint64_t *doc_ids, float *scores, uint64_t cap, uint64_t *hit_offsets,
                                   uint64_t *n_out, float *ms_device);
typedef struct tfidf_node_stats {
  uint64_t n_shards;
  uint64_t num_docs;      /* all shards */
  uint64_t doc_count;     /* node statistics in force (GLOBAL: exchanged; SHARD: sum of the shards') */
  uint64_t sum_ttf;
  uint64_t num_terms;     /* distinct terms over all shards (GLOBAL mode), else 0 */
  uint64_t transport;     /* TFIDF_TRANSPORT_RCCL or _INPROC */
} tfidf_node_stats;
int tfidf_node_stats_get(const tfidf_node *n, tfidf_node_stats *out);

/* ---- synthetic corpus (bench/test input generator, device side) ----
 * Zipf(s) over V ranks, rank r -> bijective base-26 word of
 * (r + 18278), doc lengths uniform in [len_min, len_max], ' ' separators and
 * '\n' after every 16th token and after the last.  cdf = double[V] (host). */
int tfidf_synth_corpus(int device, uint64_t seed, uint64_t n_docs, uint64_t doc_base, const double *cdf,
                       uint32_t V, uint32_t len_min, uint32_t len_max, void **d_text, void **d_offsets,
                       uint64_t *total_bytes);
int tfidf_device_free(int device, void *d_ptr);
/* Synchronous copy through the library's own HIP runtime (test/bench helper:
 * a process may hold a second HIP runtime, e.g. PyTorch's bundled one, whose
 * handles do not see the library's allocations).  kind 1 = host -> device,
 * 2 = device -> host. */
int tfidf_device_copy(int device, void *dst, const void *src, uint64_t bytes, int kind);
/* Bench helper: `reps` contiguous device-to-device hipMemcpyAsync copies of
 * `bytes` from d_src into a scratch buffer, each timed with HIP events on a
 * stream of its own (ms[reps]; one untimed copy first).  The yardstick of
 * tfidf_compact's copy kernel: a plain copy moves exactly the traffic a
 * compaction must move. */
int tfidf_device_copy_ms(int device, const void *d_src, uint64_t bytes, uint32_t reps, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* TFIDF_H */
