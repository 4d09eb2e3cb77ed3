// highlight_batch_check.cpp — stand-alone run of the batch side of
// csrc/snippet_plan.h on the host (built with -fsanitize=address,undefined and
// run as a child process by test_highlight_batch_cpu.py).
//
//   highlight_batch_check scan CASES
// scans the rows (query, document) of a batch the way the device does: the
// queries' keys are one array of per-query sorted segments (hl_segment), the
// rows are cut into chunks by hl_plan_chunks under the given budgets (items
// first, then matches inside each item chunk), every chunk is planned with
// hl_plan and its items scanned slice by slice against the segment of the
// row's query, and the passage rule is applied per row.
// Input, little endian:
//   u32 W, u64 budget_items, u64 budget_matches
//   u32 n_q, then per query: u32 n_terms, n_terms x (u32 ordinal, u32 len, bytes)
//   u32 n_docs, then per document: u32 malformed, u64 len, bytes
//   u32 R, then per row: u32 query, u32 document
// Output per row: "row <r> <n_matches> <a> <b>" and n_matches lines
// "<start> <len> <ordinal>", then "chunks <item chunks> <match chunks>" and "ok <R>".
//
//   highlight_batch_check plan CASES
// Input: u32 R, u64 budget_items, u64 budget_matches, R x u64 items, R x u64 matches.
// Output: the cut points of hl_plan_chunks on one line, then "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "snippet_plan.h"
#include "unicode_scan.h"

using namespace tfidf;

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "%s:%d: %s failed (row %lld)\n", __FILE__, __LINE__, #c, g_row); \
      exit(1);                                                              \
    }                                                                       \
  } while (0)
static long long g_row = -1;

struct Match {
  uint64_t start;
  uint32_t len, ord;
};

static FILE *g_f;
static void rd(void *p, size_t n) { CHECK(n == 0 || fread(p, 1, n, g_f) == n); }
template <class T> static T get() {
  T v;
  rd(&v, sizeof(T));
  return v;
}

static int plan_mode() {
  const uint32_t R = get<uint32_t>();
  const uint64_t bi = get<uint64_t>(), bm = get<uint64_t>();
  std::vector<uint64_t> items(R), matches(R), cuts;
  rd(items.data(), R * 8);
  rd(matches.data(), R * 8);
  hl_plan_chunks(items.data(), matches.data(), 0, R, bi, bm, &cuts);
  for (size_t i = 0; i < cuts.size(); i++) printf(i ? " %llu" : "%llu", (unsigned long long)cuts[i]);
  printf("\nok\n");
  return 0;
}

static int scan_mode() {
  const uint32_t W = get<uint32_t>();
  const uint64_t budget_items = get<uint64_t>(), budget_matches = get<uint64_t>();
  // the queries: concatenated key segments, each sorted on its own
  const uint32_t n_q = get<uint32_t>();
  std::vector<HlKey> keys;
  std::vector<uint32_t> key_off(n_q + 1, 0);
  for (uint32_t q = 0; q < n_q; q++) {
    key_off[q] = (uint32_t)keys.size();
    const uint32_t n_terms = get<uint32_t>();
    for (uint32_t t = 0; t < n_terms; t++) {
      const uint32_t ord = get<uint32_t>(), len = get<uint32_t>();
      std::vector<uint8_t> term(len);
      rd(term.data(), len);
      KeyBuilder kb;
      for (uint8_t c : term) kb.push(c);
      HlKey k{0, 0, ord, 0};
      kb.finish(&k.lo, &k.hi, 0);
      keys.push_back(k);
    }
    std::sort(keys.begin() + key_off[q], keys.end(), [](const HlKey &x, const HlKey &y) { return hl_key_less(x, y); });
  }
  key_off[n_q] = (uint32_t)keys.size();
  // an exact-size heap block (a read past the array is an ASan error)
  HlKey *kp = (HlKey *)malloc(keys.size() ? keys.size() * sizeof(HlKey) : 1);
  if (!keys.empty()) memcpy(kp, keys.data(), keys.size() * sizeof(HlKey));
  // the documents: an exact-size heap block each (a read past a document is an ASan error)
  const uint32_t n_docs = get<uint32_t>();
  std::vector<uint8_t *> doc_ptr(n_docs);
  std::vector<uint64_t> doc_len(n_docs);
  std::vector<uint8_t> bad(n_docs);
  for (uint32_t d = 0; d < n_docs; d++) {
    bad[d] = (uint8_t)get<uint32_t>();
    doc_len[d] = get<uint64_t>();
    doc_ptr[d] = (uint8_t *)malloc(doc_len[d] ? doc_len[d] : 1);
    CHECK(doc_ptr[d]);
    rd(doc_ptr[d], doc_len[d]);
  }
  // the rows
  const uint32_t R = get<uint32_t>();
  std::vector<uint32_t> row_q(R), row_d(R);
  std::vector<uint64_t> ext(2 * (size_t)R), row_items(R);
  std::vector<uint8_t> skip(R);
  for (uint32_t r = 0; r < R; r++) {
    row_q[r] = get<uint32_t>();
    row_d[r] = get<uint32_t>();
    CHECK(row_q[r] < n_q && row_d[r] < n_docs);
    ext[2 * r] = 0;                              // extents relative to the row's own block
    ext[2 * r + 1] = doc_len[row_d[r]];
    skip[r] = key_off[row_q[r]] == key_off[row_q[r] + 1] || bad[row_d[r]];
    row_items[r] = skip[r] ? 0 : hl_num_chunks(ext[2 * r + 1] - ext[2 * r]);
  }

  std::vector<std::vector<Match>> got(R);
  std::vector<uint64_t> cuts, sub, first, row_m;
  std::vector<HlItem> items;
  hl_plan_chunks(row_items.data(), nullptr, 0, R, budget_items, ~0ull, &cuts);
  CHECK(cuts.front() == 0 && cuts.back() == R);
  uint64_t n_sub = 0, filled = 0;
  for (size_t ci = 0; ci + 1 < cuts.size(); ci++) {
    const uint64_t r0 = cuts[ci], nr = cuts[ci + 1] - r0;
    CHECK(nr >= 1);
    hl_plan(ext.data() + 2 * r0, skip.data() + r0, nr, &items, &first);
    CHECK(items.size() <= budget_items || nr == 1);
    // count pass: per slice, as the device's counts array
    std::vector<uint64_t> counts(items.size() * kHlLanes + 1, 0);
    auto scan_item = [&](size_t it, bool fill, uint64_t m_base, std::vector<Match> *out) {
      const HlItem x = items[it];
      const uint64_t row = r0 + x.row;
      g_row = (long long)row;
      const uint64_t L = ext[2 * row + 1] - ext[2 * row];
      const uint8_t *doc = doc_ptr[row_d[row]];
      const HlKey *seg;
      uint32_t n_keys;
      hl_segment(kp, key_off.data(), row_q[row], &seg, &n_keys);
      uint64_t cs, ce;
      hl_chunk(doc, L, x.chunk, &cs, &ce);
      for (uint32_t lane = 0; lane < kHlLanes; lane++) {
        uint64_t pos, stop;
        hl_slice(doc, cs, ce, lane, &pos, &stop);
        const uint64_t at = it * kHlLanes + lane;
        if (!fill) {
          counts[at] = hl_scan_slice(doc, L, pos, stop, seg, n_keys, 0, [](uint32_t, uint64_t, uint32_t, uint32_t) {});
        } else {
          const uint64_t base = counts[at] - m_base, n = counts[at + 1] - counts[at];
          const uint32_t c = hl_scan_slice(doc, L, pos, stop, seg, n_keys, 0,
                                           [&](uint32_t i, uint64_t s, uint32_t len, uint32_t o) {
                                             CHECK(base + i < out->size());
                                             (*out)[base + i] = Match{s, len, o};
                                           });
          CHECK(c == n);
        }
      }
    };
    for (size_t it = 0; it < items.size(); it++) scan_item(it, false, 0, nullptr);
    uint64_t run = 0;                            // exclusive scan in place, total at the end
    for (size_t i = 0; i < counts.size(); i++) {
      const uint64_t c = counts[i];
      counts[i] = run;
      run += c;
    }
    row_m.assign(nr, 0);
    for (uint64_t i = 0; i < nr; i++) row_m[i] = counts[first[i + 1] * kHlLanes] - counts[first[i] * kHlLanes];
    // match chunks inside the item chunk: fill only their items, at offsets relative to their first match
    sub.clear();
    hl_plan_chunks(nullptr, row_m.data(), 0, nr, ~0ull, budget_matches, &sub);
    CHECK(sub.front() == 0 && sub.back() == nr);
    for (size_t si = 0; si + 1 < sub.size(); si++) {
      const uint64_t s0 = sub[si], s1 = sub[si + 1];
      const uint64_t m_base = counts[first[s0] * kHlLanes], T = counts[first[s1] * kHlLanes] - m_base;
      CHECK(T <= budget_matches || s1 - s0 == 1);
      std::vector<Match> buf(T, Match{~0ull, 0, 0});
      for (size_t it = first[s0]; it < first[s1]; it++) scan_item(it, true, m_base, &buf);
      for (uint64_t i = s0; i < s1; i++) {
        const uint64_t a = counts[first[i] * kHlLanes] - m_base, z = counts[first[i + 1] * kHlLanes] - m_base;
        CHECK(got[r0 + i].empty());
        got[r0 + i].assign(buf.begin() + a, buf.begin() + z);
        filled++;
      }
      n_sub++;
    }
  }
  CHECK(filled == R);

  for (uint32_t r = 0; r < R; r++) {
    g_row = r;
    const std::vector<Match> &M = got[r];
    const uint64_t L = ext[2 * r + 1] - ext[2 * r];
    for (size_t k = 0; k < M.size(); k++) {
      CHECK(M[k].start != ~0ull && M[k].start + M[k].len <= L);
      if (k) CHECK(M[k - 1].start + M[k - 1].len <= M[k].start);
    }
    std::vector<uint64_t> st;
    std::vector<uint32_t> ln, od;
    for (const Match &m : M) { st.push_back(m.start); ln.push_back(m.len); od.push_back(m.ord); }
    HlCand best{0, 0, 0, 0, 0, 0};
    for (uint64_t i = 0; i < M.size(); i++) {
      const HlCand c = hl_window(st.data(), ln.data(), od.data(), M.size(), i, W);
      if (hl_better(c, best)) best = c;
    }
    uint64_t a, b;
    hl_range(doc_ptr[row_d[r]], L, W, best, &a, &b);
    CHECK(a <= b && b <= L && b - a <= W);
    printf("row %u %zu %llu %llu\n", r, M.size(), (unsigned long long)a, (unsigned long long)b);
    for (const Match &m : M) printf("%llu %u %u\n", (unsigned long long)m.start, m.len, m.ord);
  }
  printf("chunks %zu %llu\n", cuts.size() - 1, (unsigned long long)n_sub);
  printf("ok %u\n", R);
  for (uint8_t *p : doc_ptr) free(p);
  free(kp);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: highlight_batch_check scan|plan CASES\n"); return 2; }
  g_f = fopen(argv[2], "rb");
  if (!g_f) { perror(argv[2]); return 2; }
  const int rc = !strcmp(argv[1], "plan") ? plan_mode() : scan_mode();
  fclose(g_f);
  return rc;
}
