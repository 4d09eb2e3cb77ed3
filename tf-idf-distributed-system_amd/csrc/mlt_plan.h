// mlt_plan.h — more-like-this (tfidf_mlt_terms*, tfidf_more_like_this*): the
// rules shared by the device pass over the seeds' forward rows
// (kernels_mlt.hip), the host around it (tfidf_capi.hip) and a stand-alone
// host checker (tests/mlt_check.cpp).
//
// A seed's candidate terms are the entries of its CSR row that pass the
// tf / df filters; a candidate's score is (float)tf * idf(df) with Lucene's
// ClassicSimilarity idf, read from a table the host computes once per snapshot
// (the device never evaluates log).  Candidates are ordered by score bits
// descending, then term bytes ascending; the device orders by score only and
// hands the host the first max_terms of a seed plus the rest of the score tie
// group the max_terms-th belongs to, where the bytes break the ties.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "tfidf_common.h"

namespace tfidf {

constexpr uint32_t kMltMaxTerms = 1024;        // max_terms (BooleanQuery's kMaxClauseCount)
constexpr uint32_t kMltMaxSeeds = 65536;       // seeds per call
constexpr uint64_t kMltCandBudget = 1ull << 22;   // candidates per fill: 64 MiB of keys and values, both sort buffers

struct MltRules {
  uint32_t min_tf, min_df, max_df, max_terms;   // min_tf >= 1 (0 is read as 1); max_df 0 = no upper bound
};

TFIDF_HD bool mlt_keep(const MltRules &r, uint32_t tf, uint32_t df) {
  return tf >= r.min_tf && df >= r.min_df && (r.max_df == 0 || df <= r.max_df);
}

// ClassicSimilarity.idf: (float)(log((docCount + 1) / (double)(docFreq + 1)) + 1.0).  Host only.
inline float mlt_idf(uint64_t df, uint64_t num_docs) {
  return (float)(log((double)(num_docs + 1) / (double)(df + 1)) + 1.0);
}
inline void mlt_idf_table(uint64_t num_docs, std::vector<float> *out) {
  out->resize(num_docs + 1);
  for (uint64_t df = 0; df <= num_docs; df++) (*out)[df] = mlt_idf(df, num_docs);
}

// one float multiply (the library is built with -ffp-contract=off; there is nothing to fuse with anyway)
TFIDF_HD float mlt_score(uint32_t tf, float idf) { return (float)tf * idf; }

TFIDF_HD uint32_t mlt_float_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
#endif
}

// Sort key of a candidate: the seed's index in its candidate chunk above the
// complemented score bits (scores are positive floats: bit order = value
// order), so an ascending sort groups the seeds and puts the best score first.
// The value carries what the host needs: dictionary slot and tf.
TFIDF_HD uint64_t mlt_key(uint32_t seed, float score) { return (uint64_t)seed << 32 | (uint32_t)~mlt_float_bits(score); }
TFIDF_HD uint32_t mlt_key_seed(uint64_t k) { return (uint32_t)(k >> 32); }
TFIDF_HD uint32_t mlt_key_score_bits(uint64_t k) { return ~(uint32_t)k; }
TFIDF_HD uint64_t mlt_val(uint32_t slot, uint32_t tf) { return (uint64_t)slot << 32 | tf; }
TFIDF_HD uint32_t mlt_val_slot(uint64_t v) { return (uint32_t)(v >> 32); }
TFIDF_HD uint32_t mlt_val_tf(uint64_t v) { return (uint32_t)v; }
// bits of the key a sort must order when a chunk holds n_seeds seeds
TFIDF_HD int mlt_key_bits(uint32_t n_seeds) {
  int b = 32;
  while (b < 64 && ((uint64_t)1 << (b - 32)) < n_seeds) b++;
  return b < 33 ? 33 : b;
}

// Sorted keys of one seed: keys[0 .. c).  What the host orders: everything when
// there are at most max_terms, else the first max_terms and the rest of the
// tie group (equal key = equal score bits) of the max_terms-th.
TFIDF_HD uint32_t mlt_select(const uint64_t *keys, uint32_t c, uint32_t max_terms) {
  if (c <= max_terms) return c;
  const uint64_t k = keys[max_terms - 1];
  uint32_t lo = max_terms, hi = c;                                   // first key > k
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] <= k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Range segment of entry i of a row: split[r] = the first entry past range r's
// segment (non-decreasing; the last range takes the rest).  R = 1: range 0.
template <class T> TFIDF_HD uint32_t mlt_range_of(const T *split, uint32_t R, uint32_t i) {
  uint32_t lo = 0, hi = R - 1;                                       // first r with i < split[r], else R - 1
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (i < split[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Seed holding flattened entry e: off[i] <= e < off[i + 1] (off[0 .. n], exclusive scan of the row lengths)
TFIDF_HD uint32_t mlt_seed_of(const uint64_t *off, uint32_t n, uint64_t e) {
  uint32_t lo = 0, hi = n;                                           // last i with off[i] <= e
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// Candidate chunks: consecutive seeds while their counted survivors fit the
// budget; a chunk holds at least one seed.  cuts: t0 = c_0 < c_1 < ... = t1.
inline void mlt_plan_chunks(const uint32_t *counts, uint64_t t0, uint64_t t1, uint64_t budget,
                            std::vector<uint64_t> *cuts) {
  cuts->push_back(t0);
  uint64_t sum = 0;
  for (uint64_t t = t0; t < t1; t++) {
    if (t > cuts->back() && sum + counts[t] > budget) {
      cuts->push_back(t);
      sum = 0;
    }
    sum += counts[t];
  }
  if (t1 > t0) cuts->push_back(t1);
}

}  // namespace tfidf
