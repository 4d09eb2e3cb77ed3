// phrase_check.cpp — stand-alone run of csrc/phrase_plan.h on the host (built
// with -fsanitize=address,undefined and run as a child process by
// test_phrase_cpu.py).
//
//   phrase_check CASES
// scans the rows (phrase, document) the way the device does: the phrases' keys
// are one array of per-phrase sorted segments, the rows are cut into chunks by
// hl_plan_chunks under the given budgets (items first, then listed tokens inside
// each item chunk), every chunk is planned with hl_plan, its items are scanned
// slice by slice (count pass: tokens and listed tokens per slice; scans; fill:
// (position, ordinal) per listed token), the frequency rule runs over every
// row's listed tokens, and the hits of each phrase are ordered by ph_sort_key.
// Input, little endian:
//   u64 budget_items, u64 budget_matches
//   u32 n_p, then per phrase: f32 weight, u32 n_distinct, n_distinct x (u32 len,
//       bytes) in ordinal order, u32 m, m x u32 ordinal
//   u32 n_docs, then per document: u32 malformed, f32 cache[norm], u64 len, bytes
//   u32 R, then per row: u32 phrase, u32 document
// Output per row: "row <r> <freq> <tokens> <listed>"; per phrase "phrase <q> <n>"
// and n lines "<doc> <score bits> <freq>"; then "chunks <item chunks> <row
// chunks>" and "ok <R>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "phrase_plan.h"
#include "unicode_scan.h"

using namespace tfidf;

static long long g_row = -1;
#define CHECK(c)                                                                        \
  do {                                                                                  \
    if (!(c)) {                                                                         \
      fprintf(stderr, "%s:%d: %s failed (row %lld)\n", __FILE__, __LINE__, #c, g_row); \
      exit(1);                                                                          \
    }                                                                                   \
  } while (0)

static FILE *g_f;
static void rd(void *p, size_t n) { CHECK(n == 0 || fread(p, 1, n, g_f) == n); }
template <class T> static T get() {
  T v;
  rd(&v, sizeof(T));
  return v;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: phrase_check CASES\n"); return 2; }
  g_f = fopen(argv[1], "rb");
  if (!g_f) { perror(argv[1]); return 2; }
  const uint64_t budget_items = get<uint64_t>(), budget_matches = get<uint64_t>();
  const uint32_t n_p = get<uint32_t>();
  std::vector<HlKey> keys;
  std::vector<uint32_t> key_off(n_p + 1, 0), seq_off(n_p + 1, 0), seq;
  std::vector<float> weight(n_p);
  for (uint32_t q = 0; q < n_p; q++) {
    key_off[q] = (uint32_t)keys.size();
    seq_off[q] = (uint32_t)seq.size();
    weight[q] = get<float>();
    const uint32_t nd = get<uint32_t>();
    for (uint32_t t = 0; t < nd; t++) {
      const uint32_t len = get<uint32_t>();
      std::vector<uint8_t> term(len);
      rd(term.data(), len);
      KeyBuilder kb;
      for (uint8_t c : term) kb.push(c);
      HlKey k{0, 0, t, 0};
      kb.finish(&k.lo, &k.hi, 0);
      keys.push_back(k);
    }
    std::sort(keys.begin() + key_off[q], keys.end(), [](const HlKey &x, const HlKey &y) { return hl_key_less(x, y); });
    const uint32_t m = get<uint32_t>();
    CHECK(m <= kPhMaxTerms);
    for (uint32_t j = 0; j < m; j++) {
      seq.push_back(get<uint32_t>());
      CHECK(seq.back() < nd);
    }
  }
  key_off[n_p] = (uint32_t)keys.size();
  seq_off[n_p] = (uint32_t)seq.size();
  // exact-size heap blocks (a read past an array is an ASan error)
  HlKey *kp = (HlKey *)malloc(keys.size() ? keys.size() * sizeof(HlKey) : 1);
  if (!keys.empty()) memcpy(kp, keys.data(), keys.size() * sizeof(HlKey));
  uint32_t *sp = (uint32_t *)malloc(seq.size() ? seq.size() * 4 : 1);
  if (!seq.empty()) memcpy(sp, seq.data(), seq.size() * 4);
  const uint32_t n_docs = get<uint32_t>();
  std::vector<uint8_t *> doc_ptr(n_docs);
  std::vector<uint64_t> doc_len(n_docs);
  std::vector<uint8_t> bad(n_docs);
  std::vector<float> cn(n_docs);
  for (uint32_t d = 0; d < n_docs; d++) {
    bad[d] = (uint8_t)get<uint32_t>();
    cn[d] = get<float>();
    doc_len[d] = get<uint64_t>();
    doc_ptr[d] = (uint8_t *)malloc(doc_len[d] ? doc_len[d] : 1);
    CHECK(doc_ptr[d]);
    rd(doc_ptr[d], doc_len[d]);
  }
  const uint32_t R = get<uint32_t>();
  std::vector<uint32_t> row_q(R), row_d(R);
  std::vector<uint64_t> ext(2 * (size_t)R), row_items(R);
  std::vector<uint8_t> skip(R);
  for (uint32_t r = 0; r < R; r++) {
    row_q[r] = get<uint32_t>();
    row_d[r] = get<uint32_t>();
    CHECK(row_q[r] < n_p && row_d[r] < n_docs);
    CHECK(r == 0 || row_q[r] >= row_q[r - 1]);           // phrase-major, as the candidates are
    ext[2 * r] = 0;
    ext[2 * r + 1] = doc_len[row_d[r]];
    skip[r] = bad[row_d[r]];
    row_items[r] = skip[r] ? 0 : hl_num_chunks(doc_len[row_d[r]]);
  }

  std::vector<uint32_t> freq(R, 0), n_tok(R, 0), n_listed(R, 0);
  std::vector<uint8_t> done(R, 0);
  std::vector<uint64_t> cuts, sub, first, row_m;
  std::vector<HlItem> items;
  hl_plan_chunks(row_items.data(), nullptr, 0, R, budget_items, ~0ull, &cuts);
  CHECK(cuts.front() == 0 && cuts.back() == R);
  uint64_t n_sub = 0;
  for (size_t ci = 0; ci + 1 < cuts.size(); ci++) {
    const uint64_t r0 = cuts[ci], nr = cuts[ci + 1] - r0;
    hl_plan(ext.data() + 2 * r0, skip.data() + r0, nr, &items, &first);
    CHECK(items.size() <= budget_items || nr == 1);
    std::vector<uint64_t> all(items.size() * kHlLanes + 1, 0), listed(items.size() * kHlLanes + 1, 0);
    auto scan_item = [&](size_t it, bool fill, uint64_t m_base, uint64_t T, uint32_t *o_pos, uint32_t *o_ord) {
      const HlItem x = items[it];
      const uint64_t row = r0 + x.row;
      g_row = (long long)row;
      const uint64_t L = ext[2 * row + 1];
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
        uint32_t n_all = 0;
        if (!fill) {
          listed[at] = ph_scan_slice(doc, L, pos, stop, seg, n_keys, 0, &n_all, [](uint32_t, uint32_t, uint32_t) {});
          all[at] = n_all;
        } else {
          const uint64_t base = listed[at] - m_base, cn_ = listed[at + 1] - listed[at];
          const uint64_t tok0 = all[at] - all[first[x.row] * kHlLanes];
          const uint32_t c = ph_scan_slice(doc, L, pos, stop, seg, n_keys, 0, &n_all,
                                           [&](uint32_t i, uint32_t k, uint32_t o) {
                                             CHECK(i < cn_ && base + i < T);      // never past the count pass
                                             o_pos[base + i] = (uint32_t)(tok0 + k);
                                             o_ord[base + i] = o;
                                           });
          CHECK(c == cn_ && n_all == all[at + 1] - all[at]);
        }
      }
    };
    for (size_t it = 0; it < items.size(); it++) scan_item(it, false, 0, 0, nullptr, nullptr);
    uint64_t ra = 0, rl = 0;                       // exclusive scans in place, totals at the end
    for (size_t i = 0; i < all.size(); i++) {
      const uint64_t a = all[i], l = listed[i];
      all[i] = ra;
      listed[i] = rl;
      ra += a;
      rl += l;
    }
    row_m.assign(nr, 0);
    for (uint64_t i = 0; i < nr; i++) row_m[i] = listed[first[i + 1] * kHlLanes] - listed[first[i] * kHlLanes];
    sub.clear();
    hl_plan_chunks(nullptr, row_m.data(), 0, nr, ~0ull, budget_matches, &sub);
    CHECK(sub.front() == 0 && sub.back() == nr);
    for (size_t si = 0; si + 1 < sub.size(); si++) {
      const uint64_t s0 = sub[si], s1 = sub[si + 1];
      const uint64_t m_base = listed[first[s0] * kHlLanes], T = listed[first[s1] * kHlLanes] - m_base;
      CHECK(T <= budget_matches || s1 - s0 == 1);
      uint32_t *o_pos = (uint32_t *)malloc(T ? T * 4 : 1), *o_ord = (uint32_t *)malloc(T ? T * 4 : 1);
      memset(o_pos, 0xFF, T * 4);
      memset(o_ord, 0xFF, T * 4);
      for (size_t it = first[s0]; it < first[s1]; it++) scan_item(it, true, m_base, T, o_pos, o_ord);
      for (uint64_t i = s0; i < s1; i++) {
        const uint64_t row = r0 + i;
        g_row = (long long)row;
        const uint64_t a = listed[first[i] * kHlLanes] - m_base, n = row_m[i];
        const uint32_t q = row_q[row], m = seq_off[q + 1] - seq_off[q];
        for (uint64_t k = 0; k < n; k++) {
          CHECK(o_ord[a + k] != 0xFFFFFFFFu);
          if (k) CHECK(o_pos[a + k] > o_pos[a + k - 1]);
        }
        uint32_t f = 0;
        for (uint64_t k = 0; k < n; k++) f += ph_match_at(o_pos + a, o_ord + a, n, k, sp + seq_off[q], m) ? 1u : 0u;
        CHECK(!done[row]);
        done[row] = 1;
        freq[row] = f;
        n_listed[row] = (uint32_t)n;
        n_tok[row] = (uint32_t)(all[first[i + 1] * kHlLanes] - all[first[i] * kHlLanes]);
        if (n) CHECK(o_pos[a + n - 1] < n_tok[row]);
      }
      free(o_pos);
      free(o_ord);
      n_sub++;
    }
  }
  for (uint32_t r = 0; r < R; r++) {
    CHECK(done[r]);
    printf("row %u %u %u %u\n", r, freq[r], n_tok[r], n_listed[r]);
  }
  // score, drop, order: per phrase by ph_sort_key
  for (uint32_t q = 0, r = 0; q < n_p; q++) {
    std::vector<std::pair<uint64_t, uint32_t>> hits;
    for (; r < R && row_q[r] == q; r++) {
      if (!freq[r]) continue;
      const float sc = ph_score(weight[q], freq[r], cn[row_d[r]]);
      uint32_t bits;
      memcpy(&bits, &sc, 4);
      hits.push_back({ph_sort_key(bits, row_d[r]), freq[r]});
    }
    std::sort(hits.begin(), hits.end());
    printf("phrase %u %zu\n", q, hits.size());
    for (auto &h : hits) printf("%u %u %u\n", ph_key_doc(h.first), ph_key_score_bits(h.first), h.second);
  }
  printf("chunks %zu %llu\n", cuts.size() - 1, (unsigned long long)n_sub);
  printf("ok %u\n", R);
  for (uint8_t *p : doc_ptr) free(p);
  free(kp);
  free(sp);
  fclose(g_f);
  return 0;
}
