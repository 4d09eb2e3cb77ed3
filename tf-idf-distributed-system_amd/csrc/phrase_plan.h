// phrase_plan.h — the logic of exact phrase search (tfidf_search_phrase*) and
// of sloppy phrase search (tfidf_search_phrase_slop*; the last section) that
// the host and the device share: the scan of one slice that numbers every
// token and lists those of the phrase, the frequency rule over a row's listed
// tokens, the score and the ordering key.  Plain C++ (TFIDF_HD; no HIP), so all
// of it is tested on its own (tests/phrase_check.cpp); kernels_phrase.hip runs
// the same functions.  The work split (chunks, slices, items, row chunks) is
// snippet_plan.h's, unchanged.
//
// Positions.  A document's tokens w_0 .. w_{n-1} are the index's (StandardTokenizer
// spans cut at 255 UTF-16 units, the scan restarted at the cut), every position
// increment 1.  Slice and chunk cuts fall only after an ASCII class-OTHER byte,
// so no token straddles one: a token's position is the number of tokens of the
// row's earlier slices plus its index in its own slice.
//
// Listed tokens.  The phrase's distinct terms, in order of first appearance,
// have ordinals 0 .. n-1 (HlKey::ordinal); seq[0, m) holds the ordinal at each
// phrase position.  A row's listed tokens are its tokens whose key is in the
// phrase's segment, as (position, ordinal), ascending by position.  Every term
// of the phrase is listed, so an occurrence at position p is a run of m
// consecutive list entries with positions p .. p + m - 1 and ordinals seq.
#pragma once

#include <stdint.h>

#include "snippet_plan.h"

namespace tfidf {

constexpr uint32_t kPhMaxTerms = 1024;   // analysed terms of one phrase (kMaxClauseCount)
constexpr uint32_t kPhMaxSloppyTerms = 64;   // of a phrase searched with slop > 0: one lane of a wave each

// hl_scan_slice that also numbers the tokens: emit(i, k, ordinal) for the i-th
// listed token, the k-th token of the slice.  Returns the listed tokens, *n_all
// = the tokens that start in [pos, stop).  The scan, its bounded lookahead and
// its retry rule are hl_scan_slice's, step for step.
template <class Emit>
TFIDF_HD uint32_t ph_scan_slice(const uint8_t *doc, uint64_t L, uint64_t pos, uint64_t stop, const HlKey *keys,
                                uint32_t n_keys, uint64_t seed, uint32_t *n_all, Emit emit) {
  uint32_t n = 0, k = 0;
  bool whole = false;                   // this step sees the whole document
  while (pos < stop) {
    const uint64_t win = whole || L - pos <= kHlWindow ? L : pos + kHlWindow;
    const uint64_t lim = stop < win ? stop : win;
    uint64_t p = pos, ts = 0, te = 0, lo = 0, hi = 0, cut = 0, mark = 0;
    bool bad = false;
    const bool found = uc_next_span(HlSrc{doc, win, &mark}, win, &p, lim, &ts, &te, &bad);
    if (found) cut = uc_token_key(doc, win, ts, te, &lo, &hi, seed);
    if (win < L && !(found && cut < te) && mark >= win) {
      whole = true;
      continue;
    }
    whole = false;
    if (bad) break;
    pos = p;
    if (!found) continue;
    if (cut < te) pos = cut;            // the rest of a cut token is the next token
    const uint32_t o = hl_find(keys, n_keys, lo, hi);
    if (o != kHlNone) {
      emit(n, k, o);
      n++;
    }
    k++;
  }
  *n_all = k;
  return n;
}

// listed token i of a row (n of them: pos ascending, ord) starts an occurrence of seq[0, m)
TFIDF_HD bool ph_match_at(const uint32_t *pos, const uint32_t *ord, uint64_t n, uint64_t i, const uint32_t *seq,
                          uint32_t m) {
  if (m == 0 || i + m > n || ord[i] != seq[0]) return false;
  const uint32_t p = pos[i];
  for (uint32_t j = 1; j < m; j++)
    if (pos[i + j] != p + j || ord[i + j] != seq[j]) return false;
  return true;
}

// BM25Scorer.score for tf = freq in Java float order (built without FMA contraction)
TFIDF_HD float ph_score(float w, uint32_t freq, float norm_inverse) {
  const float t = (float)freq * norm_inverse;
  const float u = 1.0f + t;
  const float v = w / u;
  return w - v;
}

// --- sloppy phrases (tfidf_search_phrase_slop*; Lucene's SloppyPhraseMatcher) ---
// Only phrases without a repeated term are matched with slop > 0, so the
// ordinal of a listed token is its phrase position j, and the cursor of j walks
// the row's list entries of ordinal j with position = token position - j.

// a term stands at two positions of seq[0, m) (ordinals are dense: 0 .. n-1)
TFIDF_HD bool ph_has_repeat(const uint32_t *seq, uint32_t m) {
  for (uint32_t j = 0; j < m; j++)
    if (seq[j] != j) return true;
  return false;
}

TFIDF_HD int32_t ph_slop(uint32_t slop) { return slop > 0x7FFFFFFFu ? 0x7FFFFFFF : (int32_t)slop; }

// the queue order of PhraseQueue.lessThan as one ascending key: (position, j);
// position >= -63 for j < 64
TFIDF_HD uint64_t ph_cursor_key(int64_t position, uint32_t j) { return (uint64_t)(position + 64) << 8 | j; }
TFIDF_HD int64_t ph_key_position(uint64_t key) { return (int64_t)(key >> 8) - 64; }

// PhraseScorer's freq += sloppyWeight() for one match, in float
TFIDF_HD float ph_sloppy_add(float freq, int64_t match_length) {
  const float d = 1.0f + (float)match_length;
  const float v = 1.0f / d;
  return freq + v;
}

// SloppyPhraseMatcher over one row's listed tokens (n of them: pos ascending,
// ord) for a phrase of 2 <= m <= 64 distinct terms: the float frequency, the sum
// of 1 / (1 + matchLength) over the matches of matchLength <= slop in match
// order.  0 when a term has no listed token.  One thread; k_ph_sloppy_freq
// walks the same steps with one lane per cursor.
TFIDF_HD float ph_sloppy_freq(const uint32_t *pos, const uint32_t *ord, uint64_t n, uint32_t m, uint32_t slop) {
  if (m < 2 || m > kPhMaxSloppyTerms) return 0.0f;
  const int64_t max_len = ph_slop(slop);
  uint64_t at[kPhMaxSloppyTerms], key[kPhMaxSloppyTerms];          // per cursor: list index, queue key
  auto next_of = [&](uint32_t j, uint64_t from) {
    while (from < n && ord[from] != j) from++;
    return from;
  };
  int64_t end = 0;
  for (uint32_t j = 0; j < m; j++) {
    at[j] = next_of(j, 0);
    if (at[j] == n) return 0.0f;
    const int64_t p = (int64_t)pos[at[j]] - j;
    key[j] = ph_cursor_key(p, j);
    if (j == 0 || p > end) end = p;
  }
  // least key of the cursors other than skip (m = none)
  auto least = [&](uint32_t skip) {
    uint64_t best = ~0ull;
    for (uint32_t j = 0; j < m; j++)
      if (j != skip && key[j] < best) best = key[j];
    return best;
  };
  float freq = 0.0f;
  uint64_t top = least(m);
  uint32_t pp = (uint32_t)(top & 0xFFu);
  int64_t match_length = end - ph_key_position(top), next = ph_key_position(least(pp));
  for (;;) {
    at[pp] = next_of(pp, at[pp] + 1);
    if (at[pp] == n) break;
    const int64_t p = (int64_t)pos[at[pp]] - pp;
    key[pp] = ph_cursor_key(p, pp);
    if (p > end) end = p;
    if (p > next) {
      if (match_length <= max_len) freq = ph_sloppy_add(freq, match_length);
      top = least(m);
      pp = (uint32_t)(top & 0xFFu);
      next = ph_key_position(least(pp));
      match_length = end - ph_key_position(top);
    } else {
      const int64_t l = end - p;
      if (l < match_length) match_length = l;
    }
  }
  if (match_length <= max_len) freq = ph_sloppy_add(freq, match_length);
  return freq;
}

// ph_score for a float frequency (built without FMA contraction)
TFIDF_HD float ph_score_f(float w, float freq, float norm_inverse) {
  const float t = freq * norm_inverse;
  const float u = 1.0f + t;
  const float v = w / u;
  return w - v;
}

// ascending keys = (score descending, doc ascending); scores are positive floats
TFIDF_HD uint64_t ph_sort_key(uint32_t score_bits, uint32_t doc) { return (uint64_t)(~score_bits) << 32 | doc; }
TFIDF_HD uint32_t ph_key_score_bits(uint64_t key) { return ~(uint32_t)(key >> 32); }
TFIDF_HD uint32_t ph_key_doc(uint64_t key) { return (uint32_t)key; }

}  // namespace tfidf
