// snippet_plan.h — the logic of hit highlighting (tfidf_matches,
// tfidf_snippets) that the host and the device share: how a document is cut
// into chunks and per-lane slices, the scan of one slice against the query's
// term keys, the passage rule (candidate windows, their ranking, the byte
// range and its snap to character boundaries) and the host's work plan.
// Plain C++ (TFIDF_HD; no HIP), so all of it is tested on its own
// (tests/highlight_check.cpp); kernels_highlight.hip runs the same functions.
//
// Matches.  A match is a token of the document as the index tokenised it
// (unicode_scan.h: StandardTokenizer spans cut at 255 UTF-16 units) whose
// 128-bit key equals the key of a positive query term.  A committed snapshot
// never holds two terms under one key (tfidf_common.h), and every token of a
// committed document is in its dictionary, so key equality is term equality.
//
// Work split.  A document is cut at multiples of kHlChunkBytes, each cut moved
// forward to just after the next ASCII class-OTHER byte (uc_split_byte: the
// scanner is in its start state there, and no token spans such a byte); a
// chunk is cut the same way into kHlLanes slices.  A cut with no such byte
// ahead moves to the end of its chunk / document, so a long run of letters or
// of Han characters is one slice.  A slice owns the tokens that start in it;
// slices in (chunk, lane) order give the matches in ascending start order.
#pragma once

#include <stdint.h>

#include <vector>

#include "tfidf_common.h"
#include "unicode_scan.h"

namespace tfidf {

constexpr uint64_t kHlChunkBytes = 16384;   // document bytes per work item (one wave)
constexpr uint32_t kHlLanes = 64;           // slices per chunk (one lane each)
constexpr uint32_t kHlMinBytes = 16, kHlMaxBytes = 65536;   // legal max_bytes of a snippet
constexpr uint32_t kHlNone = 0xFFFFFFFFu;

// a positive query term present in the dictionary: its key and its ordinal
// (position among the query's distinct positive terms); lists are sorted by (lo, hi)
struct HlKey {
  uint64_t lo, hi;
  uint32_t ordinal, pad;
};

TFIDF_HD bool hl_key_less(const HlKey &x, const HlKey &y) { return x.lo != y.lo ? x.lo < y.lo : x.hi < y.hi; }

// ordinal of the key (lo, hi) in the sorted list, kHlNone if absent
TFIDF_HD uint32_t hl_find(const HlKey *keys, uint32_t n, uint64_t lo, uint64_t hi) {
  uint32_t a = 0, z = n;
  while (a < z) {
    const uint32_t m = (a + z) >> 1;
    const uint64_t ml = keys[m].lo;
    if (ml < lo || (ml == lo && keys[m].hi < hi)) a = m + 1; else z = m;
  }
  return a < n && keys[a].lo == lo && keys[a].hi == hi ? keys[a].ordinal : kHlNone;
}

// the first cut point >= q in [lo, hi]: lo, hi, or just after a split byte
TFIDF_HD uint64_t hl_boundary(const uint8_t *doc, uint64_t lo, uint64_t hi, uint64_t q) {
  if (q <= lo) return lo;
  if (q >= hi) return hi;
  while (q < hi && !uc_split_byte(doc[q - 1])) q++;
  return q;
}

TFIDF_HD uint64_t hl_num_chunks(uint64_t L) { return (L + kHlChunkBytes - 1) / kHlChunkBytes; }

// chunk c of a document of L bytes: [*cs, *ce) (empty when an earlier chunk ran on past it)
TFIDF_HD void hl_chunk(const uint8_t *doc, uint64_t L, uint64_t c, uint64_t *cs, uint64_t *ce) {
  *cs = hl_boundary(doc, 0, L, c * kHlChunkBytes);
  *ce = hl_boundary(doc, 0, L, (c + 1) * kHlChunkBytes);
}

// slice `lane` of the chunk [cs, ce): [*pos, *stop)
TFIDF_HD void hl_slice(const uint8_t *doc, uint64_t cs, uint64_t ce, uint32_t lane, uint64_t *pos, uint64_t *stop) {
  const uint64_t seg = (ce - cs + kHlLanes - 1) / kHlLanes;
  *pos = hl_boundary(doc, cs, ce, cs + lane * seg);
  *stop = lane + 1 == kHlLanes ? ce : hl_boundary(doc, cs, ce, cs + (lane + 1) * seg);
}

// UcDecodeSrc that also records how far the scanner has looked: *mark = the
// largest end of a character it read (n for a sequence that does not decode
// within [0, n)).
struct HlSrc {
  const uint8_t *s;
  uint64_t n;
  uint64_t *mark;
  TFIDF_HD uint32_t at(uint64_t i, uint32_t *len) const {
    const uint32_t b = s[i];
    uint32_t c;
    if (b < 0x80u) {
      *len = 1;
      c = uc_ascii_class(b);
    } else {
      const uint32_t cp = utf8_decode(s, n, i, len);
      if (cp == kUcBad) { *mark = n; return kUcBad; }
      c = uc_class(cp);
    }
    if (i + *len > *mark) *mark = i + *len;
    return c;
  }
};

constexpr uint64_t kHlWindow = 2048;   // bytes of lookahead of the first try (255 UTF-16 units are <= 1020 bytes)

// The tokens starting in [pos, stop) of the document doc[0, L) whose key is in
// the list: emit(i, start, len, ordinal) for the i-th of them (start and len
// in document bytes, the raw span).  Returns their number.  A malformed
// sequence ends the scan (the host plans no work for malformed documents).
//
// The same tokens as uc_next_token over the whole document, found with bounded
// lookahead: the scanner's longest match walks to the end of a run of letters
// before the token is cut at 255 units and restarts at the cut, which is
// quadratic in the run.  So the scanner first sees only kHlWindow bytes past
// pos.  What it finds there stands when it never read up to the window's end
// (nothing hidden could have changed a step), or when the token was cut (the
// hidden text can only lengthen the span, and the first 255 units are the
// token either way); otherwise the step is taken again with the whole document
// in view.
template <class Emit>
TFIDF_HD uint32_t hl_scan_slice(const uint8_t *doc, uint64_t L, uint64_t pos, uint64_t stop, const HlKey *keys,
                                uint32_t n_keys, uint64_t seed, Emit emit) {
  uint32_t n = 0;
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
    if (cut < te) { te = cut; pos = cut; }
    const uint32_t o = hl_find(keys, n_keys, lo, hi);
    if (o == kHlNone) continue;
    emit(n, ts, (uint32_t)(te - ts), o);
    n++;
  }
  return n;
}

// --- the passage rule ---
// Candidate i (a match with len <= W) and its window: the matches j >= i that
// end at or before start_i + W.  Matches are sorted and do not overlap, so the
// window is the run i .. i + cnt - 1.
struct HlCand {
  uint32_t valid, pop, cnt, pad;   // pop: distinct terms (ordinals >= 63 share bit 63)
  uint64_t start, end;             // of the window: start_i, end of its last match
};

TFIDF_HD HlCand hl_window(const uint64_t *starts, const uint32_t *lens, const uint32_t *ords, uint64_t n, uint64_t i,
                          uint32_t W) {
  HlCand c{0, 0, 0, 0, 0, 0};
  if (lens[i] > W) return c;
  const uint64_t lim = starts[i] + W;
  uint64_t bits = 0;
  for (uint64_t j = i; j < n && starts[j] + lens[j] <= lim; j++) {
    bits |= 1ull << (ords[j] < 63u ? ords[j] : 63u);
    c.cnt++;
    c.end = starts[j] + lens[j];
  }
  c.valid = 1;
  c.pop = (uint32_t)__builtin_popcountll(bits);
  c.start = starts[i];
  return c;
}

// x ranks before y: more distinct terms, then more matches, then the earlier start
TFIDF_HD bool hl_better(const HlCand &x, const HlCand &y) {
  if (x.valid != y.valid) return x.valid > y.valid;
  if (x.pop != y.pop) return x.pop > y.pop;
  if (x.cnt != y.cnt) return x.cnt > y.cnt;
  return x.start < y.start;
}

// byte range [*a, *b) of the snippet around the best window (none: the head
// of the document), snapped inwards to UTF-8 character boundaries
TFIDF_HD void hl_range(const uint8_t *doc, uint64_t L, uint32_t W, const HlCand &best, uint64_t *a, uint64_t *b) {
  uint64_t a0 = 0;
  if (best.valid) {
    const uint64_t slack = W - (best.end - best.start);
    const uint64_t back = slack / 2;
    a0 = best.start - (best.start < back ? best.start : back);
  }
  uint64_t b0 = a0 + W < L ? a0 + W : L;
  while (a0 < b0 && (doc[a0] & 0xC0u) == 0x80u) a0++;
  while (b0 < L && a0 < b0 && (doc[b0] & 0xC0u) == 0x80u) b0--;
  *a = a0;
  *b = b0;
}

// --- the host's work plan ---
struct HlItem {
  uint32_t row, chunk;   // output row (position in the caller's docs list), chunk of its document
};

// ext[2 * i], ext[2 * i + 1]: corpus byte range of row i's document; skip[i]
// != 0: no work (a malformed document).  items: (row, chunk) ascending;
// first[i] = row i's first item (n + 1 entries).  Returns the bytes planned.
inline uint64_t hl_plan(const uint64_t *ext, const uint8_t *skip, uint64_t n, std::vector<HlItem> *items,
                        std::vector<uint64_t> *first) {
  items->clear();
  first->assign(n + 1, 0);
  uint64_t bytes = 0;
  for (uint64_t i = 0; i < n; i++) {
    (*first)[i] = items->size();
    if (skip && skip[i]) continue;
    const uint64_t L = ext[2 * i + 1] - ext[2 * i];
    const uint64_t nc = hl_num_chunks(L);
    for (uint64_t c = 0; c < nc; c++) items->push_back(HlItem{(uint32_t)i, (uint32_t)c});
    bytes += L;
  }
  (*first)[n] = items->size();
  return bytes;
}

// --- batches: many queries, each with its own rows ---
// The present positive terms of all queries are one HlKey array: query q's
// keys are the segment [key_off[q], key_off[q + 1]), sorted by hl_key_less on
// its own (two queries may give one term different ordinals), and row r is
// scanned against the segment of its query row_q[r].
TFIDF_HD void hl_segment(const HlKey *keys, const uint32_t *key_off, uint32_t q, const HlKey **seg, uint32_t *n) {
  *seg = keys + key_off[q];
  *n = key_off[q + 1] - key_off[q];
}

// Row chunks of a batch.  Scratch is bounded by two budgets: the (row, chunk)
// items of a chunk (known from the extents: they size the slice counts) and
// its matches (known after the count pass: they size the match arrays).
// Rows [r0, r1) are cut greedily into consecutive ranges: a range takes the
// next row while both sums stay within their budgets, and always takes one
// row, so a single row above a budget is a range of its own.  items / matches
// are per row, indexed from 0 (either may be null: not counted).  Appends the
// cut points to *cuts: r0, ..., r1 (only r0 when r0 == r1), ascending; range k
// is [cuts[k], cuts[k + 1]).
inline void hl_plan_chunks(const uint64_t *items, const uint64_t *matches, uint64_t r0, uint64_t r1,
                           uint64_t budget_items, uint64_t budget_matches, std::vector<uint64_t> *cuts) {
  cuts->push_back(r0);
  uint64_t si = 0, sm = 0;
  for (uint64_t r = r0; r < r1; r++) {
    const uint64_t ni = items ? items[r] : 0, nm = matches ? matches[r] : 0;
    if (r > cuts->back() && (si + ni > budget_items || sm + nm > budget_matches)) {
      cuts->push_back(r);
      si = sm = 0;
    }
    si += ni;     // a first row above a budget leaves its sum above it: the next row starts a range
    sm += nm;
  }
  if (r1 > r0) cuts->push_back(r1);
}

}  // namespace tfidf
