// fuzzy_search_plan.h — fuzzy search (tfidf_fuzzy_expand*, tfidf_search_fuzzy*):
// Lucene's FuzzyQuery under its top-terms blended-frequency rewrite, restated.
// The rules shared by the device (kernels_fuzzy.hip, kernels_fuzzy_search.hip),
// the host around it (tfidf_capi.hip) and a stand-alone host checker
// (tests/fuzzy_search_check.cpp).  The candidates, the distance and the cursors
// are those of the term lookup (fuzzy_plan.h); what differs is the order: an
// expansion is the first max_expansions candidates by (boost descending, term
// bytes ascending), and the bytes are compared on the device.
#pragma once

#include <stdint.h>
#include <string.h>

#include "fuzzy_plan.h"

namespace tfidf {

constexpr uint32_t kFzsMaxExpansions = 64;      // one expansion entry per lane of a wave

// m = min(code points of the candidate, code points of the input term).  A
// candidate at distance ed needs m > ed: Lucene's boost 1 - ed / m would be 0
// (scores nothing) or negative (BoostQuery rejects it) otherwise.
TFIDF_HD uint32_t fzs_min_len(uint32_t n_term, uint32_t n_cand) { return n_term < n_cand ? n_term : n_cand; }
TFIDF_HD bool fzs_keep(uint32_t ed, uint32_t m) { return m > ed; }

// one IEEE float division, one float subtraction (-ffp-contract=off: never fused)
TFIDF_HD float fzs_boost(uint32_t ed, uint32_t m) {
  if (ed == 0) return 1.0f;
  const float q = (float)ed / (float)m;
  return 1.0f - q;
}
TFIDF_HD uint32_t fzs_float_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
TFIDF_HD float fzs_bits_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// --- the candidate sort key ---
// (term index within its scan chunk, ~boost bits, dist): ascending u64 order is
// by term, then boost descending.  A boost is a float in (0, 1], so the order
// of its bits is the order of its value, and distinct ed / m (ed <= 2, m <=
// 255) differ by far more than an ulp near 1, so it is the order of the
// rationals too.  Candidates of equal boost form a tie group (fzs_key_group
// equal); the distance in the low byte only rides along.
TFIDF_HD uint64_t fzs_sort_key(uint32_t term, uint32_t ed, uint32_t m) {
  return ((uint64_t)term << 40) | ((uint64_t)(~fzs_float_bits(fzs_boost(ed, m))) << 8) | (uint64_t)ed;
}
TFIDF_HD uint64_t fzs_key_group(uint64_t k) { return k >> 8; }                    // (term, boost)
TFIDF_HD uint32_t fzs_key_term(uint64_t k) { return (uint32_t)(k >> 40); }
TFIDF_HD uint32_t fzs_key_boost_bits(uint64_t k) { return ~(uint32_t)(k >> 8); }
TFIDF_HD uint32_t fzs_key_dist(uint64_t k) { return (uint32_t)k & 0xFFu; }

// --- the byte order of two candidates ---
// A candidate of either kind behind one cursor: an exact key's two words, or a
// hashed key's reference occurrence (lower-cased on the way); n code points.
struct FzsCand {
  FzWordCursor w;
  FzTextCursor t;
  uint32_t n;
  bool text;
  TFIDF_HD uint32_t next() { return text ? t.next() : w.next(); }
};
TFIDF_HD FzsCand fzs_cand_words(const FzWordCursor &w, uint32_t n) { return FzsCand{w, FzTextCursor{nullptr, 0, 0}, n, false}; }
TFIDF_HD FzsCand fzs_cand_text(const uint8_t *s, uint32_t len) {
  return FzsCand{FzWordCursor{0, 0, 0}, FzTextCursor{s, len, 0}, fz_text_cps(s, len), true};
}

// BytesRef.compareTo of the lower-cased UTF-8 of two candidates: < 0, 0, > 0.
// UTF-8 byte order is code-point order, so the cursors' code points decide
// (both taken by value).
TFIDF_HD int fzs_compare(FzsCand a, FzsCand b) {
  const uint32_t n = a.n < b.n ? a.n : b.n;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t x = a.next(), y = b.next();
    if (x != y) return x < y ? -1 : 1;
  }
  return a.n == b.n ? 0 : (a.n < b.n ? -1 : 1);
}

// --- the selection of one term's expansion from its sorted candidates ---
// keys[0, c) ascending.  The first E form the expansion; where the tie group
// of the E-th goes on past position E, the group's smallest by bytes fill the
// places left.  Returns the plan: [0, *g0) are taken as they stand, then
// *r of the group [*g0, *g1) (all of it when the group ends at or before E).
TFIDF_HD void fzs_straddle(const uint64_t *keys, uint32_t c, uint32_t E, uint32_t *g0, uint32_t *g1, uint32_t *r) {
  if (c <= E) {
    *g0 = *g1 = c;
    *r = 0;
    return;
  }
  const uint64_t g = fzs_key_group(keys[E - 1]);
  uint32_t lo = 0, hi = E - 1;                                       // first key of the group
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (fzs_key_group(keys[mid]) < g) lo = mid + 1; else hi = mid;
  }
  *g0 = lo;
  lo = E;
  hi = c;                                                             // first key past the group
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (fzs_key_group(keys[mid]) <= g) lo = mid + 1; else hi = mid;
  }
  *g1 = lo;
  *r = E - *g0;
  if (*g1 == E) {                                                     // the group ends exactly at E: nothing to choose
    *g0 = *g1 = E;
    *r = 0;
  }
}

}  // namespace tfidf
