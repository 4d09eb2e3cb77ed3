// fuzzy_plan.h — fuzzy term lookup (tfidf_fuzzy_terms*): the rules shared by
// the device scan of the dictionary (kernels_fuzzy.hip), the host around it
// (tfidf_capi.hip) and a stand-alone host checker (tests/fuzzy_check.cpp).
//
// A term is a string of lower-cased Unicode code points.  The distance is
// optimal string alignment (OSA): insert, delete, substitute and transpose two
// adjacent code points cost 1 each, and no substring is edited twice (ca ->
// abc is 3).  Only distances <= max_edits <= 2 matter, so the DP keeps the 5
// diagonals around the main one (any cell further out is > 2) in named
// registers; a candidate is read once, front to back, through a cursor
// (next() -> code point), so an exact dictionary key is walked in the two
// registers it decodes to and a hashed key's reference occurrence straight
// from the corpus.  Before the DP: a character-set signature test, the length
// test and the prefix rule, each of which only rejects pairs the DP would.
#pragma once

#include <stdint.h>

#include <vector>

#include "tfidf_common.h"
#include "unicode_scan.h"

// the band loops run over compile-time indices only when unrolled (hipcc); a host compiler may keep them
#if defined(__clang__)
#define FZ_UNROLL _Pragma("unroll")
#else
#define FZ_UNROLL
#endif

namespace tfidf {

constexpr uint32_t kFzMaxEdits = 2;
constexpr uint32_t kFzMaxOut = 1024;
constexpr uint32_t kFzMaxTerms = 65536;        // input terms per call
constexpr uint32_t kFzFar = 64;                // "more than max_edits" inside the DP (never wraps: + 1 per step)
// LDS staging of one scan: at most kFzChunkTerms input terms of at most kFzChunkCps code points together
constexpr uint32_t kFzChunkTerms = 256;
constexpr uint32_t kFzChunkCps = 4096;
static_assert(kFzChunkCps >= kMaxTokenLen, "a single input term fits a chunk");

TFIDF_HD uint32_t fz_lower(uint32_t cp) { return cp < 0x80u ? (uint32_t)ascii_lower((uint8_t)cp) : uc_lower(cp); }

// Input term -> lower-cased code points (out: kMaxTokenLen entries).  Returns
// their count, or 0 for a term without candidates: empty, not strict UTF-8, or
// longer than 255 UTF-16 units.
TFIDF_HD uint32_t fz_decode_term(const uint8_t *s, uint64_t n, uint32_t *out) {
  uint32_t u16 = 0, k = 0;
  uint64_t p = 0;
  while (p < n) {
    uint32_t l;
    const uint32_t cp = utf8_decode(s, n, p, &l);
    if (cp == kUcBad) return 0;
    u16 += cp >= 0x10000u ? 2u : 1u;
    if (u16 > kMaxTokenLen) return 0;
    out[k++] = fz_lower(cp);
    p += l;
  }
  return k;
}

// --- candidate cursors: next() yields the candidate's code points in order ---

// valid UTF-8 held in two words (bytes 0..7 in w0, 8..15 in w1): an exact dictionary key
struct FzWordCursor {
  uint64_t w0, w1;
  uint32_t at;
  TFIDF_HD uint32_t byte() {
    const uint64_t w = at < 8 ? w0 : w1;
    const uint32_t b = (uint32_t)(w >> (8 * (at & 7u))) & 0xFFu;
    at++;
    return b;
  }
  TFIDF_HD uint32_t next() {
    const uint32_t b0 = byte();
    if (b0 < 0x80u) return b0;
    if (b0 < 0xE0u) return ((b0 & 0x1Fu) << 6) | (byte() & 0x3Fu);
    if (b0 < 0xF0u) {
      const uint32_t b1 = byte() & 0x3Fu;
      return ((b0 & 0x0Fu) << 12) | (b1 << 6) | (byte() & 0x3Fu);
    }
    const uint32_t b1 = byte() & 0x3Fu, b2 = byte() & 0x3Fu;
    return ((b0 & 0x07u) << 18) | (b1 << 12) | (b2 << 6) | (byte() & 0x3Fu);
  }
};

// Exact key -> its bytes in two words and its length in code points; false for a hashed key.
TFIDF_HD bool fz_key_words(uint64_t lo, uint64_t hi, FzWordCursor *c, uint32_t *n_cps) {
  if (key_is_hashed(lo)) return false;
  uint64_t w0, w1;
  if ((lo & kLoLong) && (lo & kLoUniExact)) {                       // exact non-ASCII form (KeyBuilder::finish)
    const uint64_t r = (lo & ((1ull << 47) - 1)) | (((lo >> 48) & 0x3Full) << 47);
    w0 = (hi & ~kKeyValid) | ((r & 1ull) << 63);
    w1 = (r >> 1) & 0xFFFFFFFFFFFFull;
  } else {
    w0 = lo & ~kLoLong;
    w1 = (lo & kLoLong) ? (hi & ~kKeyValid) : 0ull;
  }
  // a token holds no 0 byte, so the zero padding gives the length; code points = bytes that are not 10xxxxxx
  const uint64_t k7 = 0x7F7F7F7F7F7F7F7Full, k8 = 0x8080808080808080ull;
  const uint64_t nz0 = (((w0 & k7) + k7) | w0) & k8, nz1 = (((w1 & k7) + k7) | w1) & k8;
  const uint64_t ct0 = w0 & ~(w0 << 1) & k8, ct1 = w1 & ~(w1 << 1) & k8;
  *n_cps = (uint32_t)(__builtin_popcountll(nz0) + __builtin_popcountll(nz1) - __builtin_popcountll(ct0) -
                      __builtin_popcountll(ct1));
  c->w0 = w0;
  c->w1 = w1;
  c->at = 0;
  return true;
}

// raw token bytes (a reference occurrence in the corpus, or a vocabulary string
// of the checker): lower-cased on the way, cut at 255 UTF-16 units as uc_token_bytes cuts
struct FzTextCursor {
  const uint8_t *s;
  uint32_t n, at;
  TFIDF_HD uint32_t next() {
    uint32_t l = 1;
    const uint32_t cp = utf8_decode(s, n, at, &l);
    at += l;
    return fz_lower(cp);
  }
};
TFIDF_HD uint32_t fz_text_cps(const uint8_t *s, uint32_t n) {
  uint32_t u16 = 0, k = 0, p = 0;
  while (p < n) {
    uint32_t l = 1;
    const uint32_t cp = utf8_decode(s, n, p, &l);
    if (cp == kUcBad) break;
    const uint32_t w = cp >= 0x10000u ? 2u : 1u;
    if (u16 + w > kMaxTokenLen) break;
    u16 += w;
    k++;
    p += l;
  }
  return k;
}

// --- the filter and the distance ---

// length filter: the distance is at least the difference of the lengths
TFIDF_HD bool fz_len_ok(uint32_t n_term, uint32_t n_cand, uint32_t max_edits) {
  return n_term <= n_cand + max_edits && n_cand <= n_term + max_edits;
}

// prefix rule: p = min(prefix_len, n_term); the candidate has at least p code
// points and its first p equal the term's (the cursor is taken by value)
template <class Cursor>
TFIDF_HD bool fz_prefix_ok(const uint32_t *term, uint32_t n_term, Cursor c, uint32_t n_cand, uint32_t prefix_len) {
  const uint32_t p = prefix_len < n_term ? prefix_len : n_term;
  if (n_cand < p) return false;
  for (uint32_t i = 0; i < p; i++)
    if (c.next() != term[i]) return false;
  return true;
}

// OSA distance of term[0, n) and the candidate's m code points when it is <=
// max_edits (<= kFzMaxEdits), else some value > max_edits.  Requires
// fz_len_ok.  Row r of the DP is the candidate's prefix of r code points; band
// entry k of a row is the term's prefix of i = r + k - 2 code points.
template <class Cursor>
TFIDF_HD uint32_t fz_osa_banded(const uint32_t *term, uint32_t n, Cursor c, uint32_t m, uint32_t max_edits) {
  uint32_t p2[5], p1[5], cur[5];
  FZ_UNROLL
  for (int k = 0; k < 5; k++) {
    p2[k] = kFzFar;
    p1[k] = (k >= 2 && (uint32_t)(k - 2) <= n) ? (uint32_t)(k - 2) : kFzFar;   // row 0: D[0][i] = i
  }
  uint32_t b_prev = 0;
  for (uint32_t r = 1; r <= m; r++) {
    const uint32_t b = c.next();
    uint32_t row_min = kFzFar;
    FZ_UNROLL
    for (int k = 0; k < 5; k++) {
      const int32_t i = (int32_t)r + k - 2;
      uint32_t v = kFzFar;
      if (i == 0) {
        v = r;
      } else if (i > 0 && (uint32_t)i <= n) {
        const uint32_t a = term[i - 1];
        v = p1[k] + (a != b ? 1u : 0u);                             // D[r-1][i-1]
        if (k < 4 && p1[k < 4 ? k + 1 : 4] + 1 < v) v = p1[k < 4 ? k + 1 : 4] + 1;   // D[r-1][i]
        if (k > 0 && cur[k > 0 ? k - 1 : 0] + 1 < v) v = cur[k > 0 ? k - 1 : 0] + 1; // D[r][i-1]
        if (r >= 2 && i >= 2 && a == b_prev && term[i - 2] == b && p2[k] + 1 < v) v = p2[k] + 1;   // D[r-2][i-2]
      }
      cur[k] = v;
      if (v < row_min) row_min = v;
    }
    if (row_min > max_edits) return max_edits + 1;                  // every later cell is at least the row's minimum
    FZ_UNROLL
    for (int k = 0; k < 5; k++) {
      p2[k] = p1[k];
      p1[k] = cur[k];
    }
    b_prev = b;
  }
  const uint32_t kk = n + 2 - m;                                    // D[m][n]: 0..4 by fz_len_ok
  uint32_t d = p1[0];
  FZ_UNROLL
  for (int k = 1; k < 5; k++)
    if (kk == (uint32_t)k) d = p1[k];
  return d;
}

// Character-set signature: one bit per distinct code point (hashed to 64
// bits).  An edit removes at most one distinct code point from a string and
// adds at most one (a transposition neither), so strings within max_edits have
// at most max_edits signature bits on either side that the other lacks: a
// cheap test that never rejects a pair within the distance.
TFIDF_HD uint64_t fz_sig_bit(uint32_t cp) { return 1ull << ((cp * 0x9E3779B1u) >> 26); }
template <class Cursor>
TFIDF_HD uint64_t fz_sig(Cursor c, uint32_t m) {
  uint64_t s = 0;
  for (uint32_t i = 0; i < m; i++) s |= fz_sig_bit(c.next());
  return s;
}
TFIDF_HD uint64_t fz_sig_term(const uint32_t *term, uint32_t n) {
  uint64_t s = 0;
  for (uint32_t i = 0; i < n; i++) s |= fz_sig_bit(term[i]);
  return s;
}
TFIDF_HD bool fz_sig_ok(uint64_t sig_term, uint64_t sig_cand, uint32_t max_edits) {
  return (uint32_t)__builtin_popcountll(sig_term & ~sig_cand) <= max_edits &&
         (uint32_t)__builtin_popcountll(sig_cand & ~sig_term) <= max_edits;
}

// the whole test of one (term, candidate) pair: distance, or kFzFar when the candidate does not qualify
template <class Cursor>
TFIDF_HD uint32_t fz_match(const uint32_t *term, uint32_t n_term, const Cursor &c, uint32_t n_cand, uint32_t max_edits,
                           uint32_t prefix_len) {
  if (!fz_len_ok(n_term, n_cand, max_edits)) return kFzFar;
  if (!fz_prefix_ok(term, n_term, c, n_cand, prefix_len)) return kFzFar;
  const uint32_t d = fz_osa_banded(term, n_term, c, n_cand, max_edits);
  return d <= max_edits ? d : kFzFar;
}

// --- the candidate sort key ---
// (term index within its scan chunk, dist, ~df): ascending u64 order is by
// term, then distance ascending, then df descending.  The byte order of the
// term strings breaks the remaining ties on the host.
TFIDF_HD uint64_t fz_sort_key(uint32_t term, uint32_t dist, uint32_t df) {
  return ((uint64_t)term << 40) | ((uint64_t)dist << 32) | (uint64_t)(~df);
}
TFIDF_HD uint32_t fz_key_term(uint64_t k) { return (uint32_t)(k >> 40); }
TFIDF_HD uint32_t fz_key_dist(uint64_t k) { return (uint32_t)(k >> 32) & 0xFFu; }
TFIDF_HD uint32_t fz_key_df(uint64_t k) { return ~(uint32_t)k; }

// --- the host plan ---
// Scan chunks: consecutive input terms staged together in LDS for one pass
// over the dictionary: at most kFzChunkTerms terms and kFzChunkCps code points
// (n_cps[i]: term i's code points; 0 = a term without candidates, staged
// nowhere but still a member of its chunk).  Appends the cut points 0, ..., n.
inline void fz_plan_scan_chunks(const uint32_t *n_cps, uint64_t n, uint32_t max_terms, uint32_t max_cps,
                                std::vector<uint64_t> *cuts) {
  cuts->push_back(0);
  uint64_t nt = 0, nc = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (i > cuts->back() && (nt + 1 > max_terms || nc + n_cps[i] > max_cps)) {
      cuts->push_back(i);
      nt = nc = 0;
    }
    nt++;
    nc += n_cps[i];
  }
  if (n) cuts->push_back(n);
}

// Candidate chunks of a scan chunk [t0, t1): the counted candidates per term
// (the count pass) cut greedily into consecutive term ranges of at most
// `budget` candidates; a range always takes one term, so a single term above
// the budget is a range of its own.  Appends the cut points t0, ..., t1.
inline void fz_plan_cand_chunks(const uint32_t *counts, uint64_t t0, uint64_t t1, uint64_t budget,
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

// LDS image of a range of staged terms: off[i] .. off[i + 1] index cps (i relative to the range)
struct FzStage {
  std::vector<uint32_t> off, cps;
};
inline void fz_stage_terms(const std::vector<std::vector<uint32_t>> &terms, uint64_t t0, uint64_t t1, FzStage *st) {
  st->off.assign(1, 0);
  st->cps.clear();
  for (uint64_t t = t0; t < t1; t++) {
    st->cps.insert(st->cps.end(), terms[t].begin(), terms[t].end());
    st->off.push_back((uint32_t)st->cps.size());
  }
}

}  // namespace tfidf
