// compound_plan.h — compound queries (tfidf_search_compound*): the rules shared
// by the device pass over the clause rows (kernels_compound.hip), the host
// around it (tfidf_capi.hip) and a stand-alone host checker
// (tests/compound_check.cpp).
//
// A compound query is a flat list of clauses (Lucene 9.8 BooleanQuery without
// nesting, boosts or minimumShouldMatch; DESIGN.md section 2, "Compound
// queries").  Each clause has a row: the documents, each with a float score,
// that the clause's own all-hits route returns.  With R the MUST and FILTER
// clauses, N the MUST_NOT clauses and S the SHOULD clauses, a document matches
// when it is in every row of R, in no row of N and, when R is empty, in a row of
// S.  Its score is (float)(double sum of the MUST scores) + (float)(double sum
// of the matching SHOULD scores), one float addition (ReqOptSumScorer), both
// sums in clause order; a part that is absent is left out, none gives 0.0f.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "tfidf.h"
#include "tfidf_common.h"

namespace tfidf {

constexpr uint32_t kCqMaxClausesPerQuery = 64;
constexpr uint32_t kCqMaxQueries = 65536;            // queries per call
constexpr uint64_t kCqMaxClauses = 1ull << 20;       // clauses per call
// Row entries per chunk of the device pass.  The figure of kMltCandBudget and of
// the wildcard match budget (32 MiB of entries, as much again binned); it is not
// a measured optimum.  TFIDF_COMPOUND_CHUNK overrides it (a debug knob).
constexpr uint64_t kCqEntryBudget = 1ull << 22;
constexpr uint32_t kCqBlockDocs = 8192;              // = kBlockDocs: the doc block of a bin and of a run
constexpr uint32_t kCqTileDocs = 2048;               // documents whose state a workgroup holds at once
static_assert(kCqBlockDocs % kCqTileDocs == 0, "a block is whole tiles");

// per-document flag bits of the combine pass
constexpr uint32_t kCqVeto = 1u;                     // a MUST_NOT row holds the document
constexpr uint32_t kCqShould = 2u;                   // a SHOULD row holds the document

// argument validation: 0, or the first rule broken
enum {
  kCqOk = 0,
  kCqTooManyQueries,       // n_q > kCqMaxQueries
  kCqBadQueryOffsets,      // q_clause_offsets[0] != 0 or decreasing (*at: the query)
  kCqTooManyInQuery,       // a query of more than kCqMaxClausesPerQuery clauses (*at: the query)
  kCqTooManyClauses,       // more than kCqMaxClauses clauses in the call
  kCqBadPayloadOffsets,    // c_offsets[0] != 0 or decreasing (*at: the clause)
  kCqBadOccur,             // (*at: the clause)
  kCqBadKind,              // (*at: the clause)
};

inline int cq_check_args(const uint64_t *c_offsets, const tfidf_clause *clauses, const uint64_t *q_clause_offsets,
                         uint64_t n_q, uint64_t *at) {
  *at = 0;
  if (n_q > kCqMaxQueries) return kCqTooManyQueries;
  if (n_q == 0) return kCqOk;
  if (q_clause_offsets[0] != 0) return kCqBadQueryOffsets;
  for (uint64_t q = 0; q < n_q; q++) {
    *at = q;
    if (q_clause_offsets[q + 1] < q_clause_offsets[q]) return kCqBadQueryOffsets;
    if (q_clause_offsets[q + 1] - q_clause_offsets[q] > kCqMaxClausesPerQuery) return kCqTooManyInQuery;
  }
  const uint64_t n_c = q_clause_offsets[n_q];
  *at = 0;
  if (n_c > kCqMaxClauses) return kCqTooManyClauses;
  if (n_c == 0) return kCqOk;
  if (c_offsets[0] != 0) return kCqBadPayloadOffsets;
  for (uint64_t c = 0; c < n_c; c++) {
    *at = c;
    if (c_offsets[c + 1] < c_offsets[c]) return kCqBadPayloadOffsets;
    if (clauses[c].occur > TFIDF_OCCUR_FILTER) return kCqBadOccur;
    if (clauses[c].kind > TFIDF_CLAUSE_FUZZY) return kCqBadKind;
  }
  return kCqOk;
}

// what a query's clause list asks of a document
struct CqNeeds {
  uint32_t n_req;      // MUST + FILTER clauses
  uint32_t n_must;     // MUST clauses
};

TFIDF_HD void cq_needs_add(CqNeeds *n, uint32_t occur) {
  if (occur == TFIDF_OCCUR_MUST) { n->n_req++; n->n_must++; }
  else if (occur == TFIDF_OCCUR_FILTER) n->n_req++;
}

// One clause's row holds the document with this score: the update of the
// document's state.  Called in clause order, so the sums are in clause order.
TFIDF_HD void cq_apply(uint32_t occur, float score, uint8_t *req, uint8_t *flags, double *must, double *should) {
  if (occur == TFIDF_OCCUR_MUST) {
    *req = (uint8_t)(*req + 1);
    *must += (double)score;
  } else if (occur == TFIDF_OCCUR_FILTER) {
    *req = (uint8_t)(*req + 1);
  } else if (occur == TFIDF_OCCUR_MUST_NOT) {
    *flags = (uint8_t)(*flags | kCqVeto);
  } else {
    *flags = (uint8_t)(*flags | kCqShould);
    *should += (double)score;
  }
}

TFIDF_HD bool cq_match(const CqNeeds &n, uint32_t req, uint32_t flags) {
  if (flags & kCqVeto) return false;
  if (req != n.n_req) return false;
  return n.n_req > 0 || (flags & kCqShould) != 0;
}

// the score of a matching document
TFIDF_HD float cq_score(const CqNeeds &n, uint32_t flags, double must, double should) {
  const bool has_m = n.n_must > 0, has_s = (flags & kCqShould) != 0;
  const float m = (float)must, s = (float)should;
  if (has_m && has_s) return m + s;                 // ReqOptSumScorer: one float addition
  if (has_m) return m;
  if (has_s) return s;
  return 0.0f;
}

TFIDF_HD uint32_t cq_float_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
#endif
}

// the all-hits merge key of a hit (descending key order = score bits descending, doc ascending)
TFIDF_HD uint64_t cq_hit_key(float score, uint32_t doc) { return (uint64_t)cq_float_bits(score) << 32 | (uint32_t)~doc; }

// bin of a row entry: (clause of the chunk, doc block)
TFIDF_HD uint64_t cq_bin(uint32_t clause, uint32_t doc, uint32_t n_blocks) {
  return (uint64_t)clause * n_blocks + doc / kCqBlockDocs;
}

// Clause holding flattened entry e: off[c] <= e < off[c + 1] (off[0 .. n])
TFIDF_HD uint32_t cq_clause_of(const uint64_t *off, uint32_t n, uint64_t e) {
  uint32_t lo = 0, hi = n;                                           // last c with off[c] <= e
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// A query's bound on its hits from its clauses' row sizes: the smallest R row,
// or without R the sum of the SHOULD rows; never more than n_docs.
inline uint64_t cq_hit_bound(const tfidf_clause *clauses, const uint64_t *rows, uint64_t n_c, uint64_t n_docs) {
  uint64_t min_req = UINT64_MAX, sum_should = 0;
  for (uint64_t c = 0; c < n_c; c++) {
    if (clauses[c].occur == TFIDF_OCCUR_MUST || clauses[c].occur == TFIDF_OCCUR_FILTER) {
      if (rows[c] < min_req) min_req = rows[c];
    } else if (clauses[c].occur == TFIDF_OCCUR_SHOULD) {
      sum_should += rows[c];
    }
  }
  const uint64_t b = min_req != UINT64_MAX ? min_req : sum_should;
  return b < n_docs ? b : n_docs;
}

// Chunks of whole, consecutive queries: while the queries' row entries stay in
// the budget, and their count and their clauses in the two scratch limits; a
// chunk holds at least one query.  cuts: 0 = c_0 < c_1 < ... = n_q.
inline void cq_plan_chunks(const uint64_t *q_entries, const uint64_t *q_clause_offsets, uint64_t n_q, uint64_t budget,
                           uint64_t max_queries, uint64_t max_clauses, std::vector<uint64_t> *cuts) {
  cuts->clear();
  cuts->push_back(0);
  uint64_t sum = 0;
  for (uint64_t q = 0; q < n_q; q++) {
    const uint64_t a = cuts->back();
    if (q > a && (sum + q_entries[q] > budget || q - a >= max_queries ||
                  q_clause_offsets[q + 1] - q_clause_offsets[a] > max_clauses)) {
      cuts->push_back(q);
      sum = 0;
    }
    sum += q_entries[q];
  }
  if (n_q) cuts->push_back(n_q);
}

}  // namespace tfidf
