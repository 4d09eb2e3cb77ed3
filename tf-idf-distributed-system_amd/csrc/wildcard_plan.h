// wildcard_plan.h — wildcard and prefix search (tfidf_wildcard_terms*,
// tfidf_search_wildcard*): the rules shared by the device scan of the
// dictionary and the posting union (kernels_wildcard.hip), the host around
// them (tfidf_capi.hip) and a stand-alone host checker
// (tests/wildcard_check.cpp).
//
// A pattern is a byte string, decoded as strict UTF-8 into elements: `*` (any
// run of code points, none included), `?` (exactly one code point), `\x` (the
// literal x; a trailing lone `\` is a literal backslash) and literals, which
// are lower-cased per code point with fz_lower.  Runs of `*` collapse to one.
// A vocabulary term matches when the whole term does (anchored at both ends).
// This restates Lucene 9.8 WildcardQuery.toAutomaton and PrefixQuery (`abc*`);
// the lower-casing of the literals is ours.
//
// The matcher reads a candidate once, front to back, through the cursors of
// fuzzy_plan.h.  Before it: the minimum code-point count (the exact count for
// a pattern without `*`) and the literal prefix before the first wildcard; a
// pure prefix pattern and an exact term end there.  Past the prefix the set of
// reached pattern positions (0 .. n, n <= 255) lives in four 64-bit words and
// every code point moves the set bits: a `*` position stays and also reaches
// its successor, a `?` or an equal literal advances.
#pragma once

#include <stdint.h>

#include <vector>

#include "fuzzy_plan.h"

namespace tfidf {

constexpr uint32_t kWcMaxElems = 255;           // elements of a pattern after collapsing
constexpr uint32_t kWcMaxOut = 1024;
constexpr uint32_t kWcMaxPatterns = 65536;      // patterns per call
constexpr uint32_t kWcStar = 0x80000000u;       // element codes above every code point
constexpr uint32_t kWcAny = 0x80000001u;
// LDS staging of one scan: at most kWcChunkPatterns patterns of at most kWcChunkElems elements together
constexpr uint32_t kWcChunkPatterns = 128;
constexpr uint32_t kWcChunkElems = 2048;
static_assert(kWcChunkElems >= kWcMaxElems, "a single pattern fits a chunk");

// Pattern -> elements (out: kWcMaxElems entries).  Returns their count, or 0
// for a pattern that matches nothing: empty, not strict UTF-8, or more than
// kWcMaxElems elements after collapsing.
TFIDF_HD uint32_t wc_parse(const uint8_t *s, uint64_t n, uint32_t *out) {
  uint32_t k = 0;
  uint64_t p = 0;
  while (p < n) {
    uint32_t l;
    uint32_t cp = utf8_decode(s, n, p, &l);
    if (cp == kUcBad) return 0;
    p += l;
    uint32_t e;
    if (cp == '*') {
      if (k && out[k - 1] == kWcStar) continue;
      e = kWcStar;
    } else if (cp == '?') {
      e = kWcAny;
    } else {
      if (cp == '\\' && p < n) {
        cp = utf8_decode(s, n, p, &l);
        if (cp == kUcBad) return 0;
        p += l;
      }
      e = fz_lower(cp);
    }
    if (k == kWcMaxElems) return 0;
    out[k++] = e;
  }
  return k;
}

// what the cheap tests read: the literal elements before the first wildcard,
// the code points every match has at least, and whether a `*` occurs
struct WcMeta {
  uint32_t prefix, min_cps, star;
};
TFIDF_HD WcMeta wc_meta(const uint32_t *el, uint32_t n) {
  WcMeta m{n, 0, 0};
  for (uint32_t i = 0; i < n; i++) {
    if (el[i] == kWcStar) m.star = 1; else m.min_cps++;
    if (el[i] >= kWcStar && m.prefix == n) m.prefix = i;
  }
  return m;
}

// the reached pattern positions 0 .. n (bit i: the first i elements are matched)
struct WcState {
  uint64_t w[4];
};
TFIDF_HD void wc_set(WcState &s, uint32_t i) {
  FZ_UNROLL
  for (uint32_t k = 0; k < 4; k++) s.w[k] |= (i >> 6) == k ? 1ull << (i & 63u) : 0ull;
}
TFIDF_HD bool wc_has(const WcState &s, uint32_t i) {
  uint64_t v = 0;
  FZ_UNROLL
  for (uint32_t k = 0; k < 4; k++) v |= (i >> 6) == k ? s.w[k] : 0ull;
  return (v >> (i & 63u)) & 1ull;
}
// position i and, when element i is `*`, the position after it (runs are collapsed: no chain)
TFIDF_HD void wc_reach(WcState &s, const uint32_t *el, uint32_t n, uint32_t i) {
  wc_set(s, i);
  if (i < n && el[i] == kWcStar) wc_set(s, i + 1);
}

// Does the candidate (n_cand code points behind the cursor, taken by value) match the pattern?
template <class Cursor>
TFIDF_HD bool wc_match(const uint32_t *el, uint32_t n, const WcMeta &m, Cursor c, uint32_t n_cand) {
  if (n == 0 || n_cand < m.min_cps || (!m.star && n_cand != m.min_cps)) return false;
  for (uint32_t i = 0; i < m.prefix; i++)
    if (c.next() != el[i]) return false;
  if (m.prefix == n) return true;                                    // an exact term (the counts are equal)
  if (m.prefix + 1 == n && el[m.prefix] == kWcStar) return true;     // a pure prefix pattern
  WcState cur{{0, 0, 0, 0}};
  wc_reach(cur, el, n, m.prefix);
  for (uint32_t r = m.prefix; r < n_cand; r++) {
    const uint32_t ch = c.next();
    WcState nx{{0, 0, 0, 0}};
    FZ_UNROLL
    for (uint32_t k = 0; k < 4; k++) {
      uint64_t bits = cur.w[k];
      while (bits) {
        const uint32_t i = k * 64u + (uint32_t)__builtin_ctzll(bits);
        bits &= bits - 1;
        if (i >= n) continue;                                        // the accepting position has no way on
        const uint32_t e = el[i];
        if (e == kWcStar) wc_reach(nx, el, n, i);
        else if (e == kWcAny || e == ch) wc_reach(nx, el, n, i + 1);
      }
    }
    if ((nx.w[0] | nx.w[1] | nx.w[2] | nx.w[3]) == 0) return false;
    cur = nx;
  }
  return wc_has(cur, n);
}

// --- the match sort key ---
// (pattern index within its scan chunk, ~df): fz_sort_key with distance 0, so
// the fuzzy route's sort, selection and gather order a pattern's terms by df descending
TFIDF_HD uint64_t wc_sort_key(uint32_t pattern, uint32_t df) { return fz_sort_key(pattern, 0, df); }

// --- the host plan ---
// Scan chunks: consecutive patterns staged together in LDS for one pass over
// the dictionary (n_el[i] = 0: a pattern that matches nothing, staged nowhere
// but still a member of its chunk).  Appends the cut points 0, ..., n.
inline void wc_plan_scan_chunks(const uint32_t *n_el, uint64_t n, std::vector<uint64_t> *cuts) {
  fz_plan_scan_chunks(n_el, n, kWcChunkPatterns, kWcChunkElems, cuts);
}
// Match chunks of a scan chunk: consecutive patterns of at most `budget`
// (pattern, term) matches together (one pattern above the budget is a chunk of its own).
inline void wc_plan_match_chunks(const uint32_t *counts, uint64_t t0, uint64_t t1, uint64_t budget,
                                 std::vector<uint64_t> *cuts) {
  fz_plan_cand_chunks(counts, t0, t1, budget, cuts);
}
// Union chunks of a match chunk [t0, t1): consecutive patterns whose document
// bitmaps (bits_per_pattern each: the hits a pattern can have) stay within
// `budget` bits together; always at least one pattern.  Appends t0, ..., t1.
inline void wc_plan_union_chunks(uint64_t t0, uint64_t t1, uint64_t bits_per_pattern, uint64_t budget,
                                 std::vector<uint64_t> *cuts) {
  uint64_t per = bits_per_pattern ? budget / bits_per_pattern : t1 - t0;
  if (per < 1) per = 1;
  for (uint64_t t = t0; t < t1; t += per) cuts->push_back(t);
  cuts->push_back(t1);
}

}  // namespace tfidf
