// highlight_check.cpp — stand-alone run of csrc/snippet_plan.h on the host
// (built with -fsanitize=address,undefined and run as a child process by
// test_highlight_cpu.py).  Reads cases (query terms with ordinals, W, text)
// from the file named on the command line, scans every document the way the
// device does — the host's plan of (row, chunk) items, 64 slices per chunk,
// each slice on its own — applies the passage rule, and prints the matches and
// the snippet range of each case for the test to compare with the oracle.
//
// Input, little endian:  u32 n_cases, then per case
//   u32 W, u32 malformed, u32 n_terms, n_terms x (u32 ordinal, u32 len, bytes), u64 text_len, bytes
// Output per case:  "case <i> <n_matches> <a> <b>" and n_matches lines "<start> <len> <ordinal>".
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
      fprintf(stderr, "%s:%d: %s failed (case %d)\n", __FILE__, __LINE__, #c, g_case); \
      exit(1);                                                              \
    }                                                                       \
  } while (0)
static int g_case = -1;

struct Match {
  uint64_t start;
  uint32_t len, ord;
  bool operator==(const Match &o) const { return start == o.start && len == o.len && ord == o.ord; }
};

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: highlight_check CASES\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t n_cases = 0;
  CHECK(read_exact(f, &n_cases, 4));
  for (uint32_t ci = 0; ci < n_cases; ci++) {
    g_case = (int)ci;
    uint32_t W, malformed, n_terms;
    CHECK(read_exact(f, &W, 4) && read_exact(f, &malformed, 4) && read_exact(f, &n_terms, 4));
    std::vector<HlKey> keys;
    for (uint32_t t = 0; t < n_terms; t++) {
      uint32_t ord, len;
      CHECK(read_exact(f, &ord, 4) && read_exact(f, &len, 4));
      std::vector<uint8_t> term(len);
      CHECK(read_exact(f, term.data(), len));
      KeyBuilder kb;
      for (uint8_t c : term) kb.push(c);
      HlKey k{0, 0, ord, 0};
      kb.finish(&k.lo, &k.hi, 0);
      keys.push_back(k);
    }
    std::sort(keys.begin(), keys.end(), [](const HlKey &x, const HlKey &y) { return hl_key_less(x, y); });
    uint64_t L = 0;
    CHECK(read_exact(f, &L, 8));
    // an exact-size heap block: a read past the document is an ASan error
    uint8_t *doc = (uint8_t *)malloc(L ? L : 1);
    CHECK(doc && read_exact(f, doc, L));

    // the plan of a one-row call, then every item's 64 slices, each on its own
    const uint64_t ext[2] = {0, L};
    const uint8_t skip[1] = {(uint8_t)(malformed || keys.empty())};
    std::vector<HlItem> items;
    std::vector<uint64_t> first;
    const uint64_t planned = hl_plan(ext, skip, 1, &items, &first);
    CHECK(first.size() == 2 && first[0] == 0 && first[1] == items.size());
    CHECK(items.size() == (skip[0] ? 0 : hl_num_chunks(L)));
    CHECK(planned == (skip[0] ? 0 : L));
    std::vector<Match> got;
    uint64_t cursor = 0;                       // the slices tile [0, L) in (chunk, lane) order
    for (size_t it = 0; it < items.size(); it++) {
      CHECK(items[it].row == 0 && items[it].chunk == it);
      uint64_t cs, ce;
      hl_chunk(doc, L, items[it].chunk, &cs, &ce);
      CHECK(cs == cursor && ce >= cs && ce <= L);
      for (uint32_t lane = 0; lane < kHlLanes; lane++) {
        uint64_t pos, stop;
        hl_slice(doc, cs, ce, lane, &pos, &stop);
        CHECK(pos == cursor && stop >= pos && stop <= ce);
        if (pos > 0 && pos < L) CHECK(uc_split_byte(doc[pos - 1]));
        // count, then fill: the two passes of the device agree
        const uint32_t cnt = hl_scan_slice(doc, L, pos, stop, keys.data(), (uint32_t)keys.size(), 0,
                                           [](uint32_t, uint64_t, uint32_t, uint32_t) {});
        const size_t before = got.size();
        const uint32_t cnt2 = hl_scan_slice(doc, L, pos, stop, keys.data(), (uint32_t)keys.size(), 0,
                                            [&](uint32_t i, uint64_t s, uint32_t len, uint32_t o) {
                                              CHECK(i == got.size() - before);
                                              got.push_back(Match{s, len, o});
                                            });
        CHECK(cnt == cnt2 && got.size() - before == cnt);
        for (size_t k = before; k < got.size(); k++) CHECK(got[k].start >= pos && got[k].start + got[k].len <= stop);
        cursor = stop;
      }
      CHECK(cursor == ce);
    }
    if (!items.empty()) CHECK(cursor == L);
    // one scan of the whole document finds the same matches
    if (!skip[0]) {
      std::vector<Match> whole;
      hl_scan_slice(doc, L, 0, L, keys.data(), (uint32_t)keys.size(), 0,
                    [&](uint32_t, uint64_t s, uint32_t len, uint32_t o) { whole.push_back(Match{s, len, o}); });
      CHECK(whole == got);
    }
    for (size_t k = 1; k < got.size(); k++) CHECK(got[k - 1].start + got[k - 1].len <= got[k].start);

    // the passage rule, as k_hl_rank applies it: lane-strided candidates, then the best of the lanes
    std::vector<uint64_t> st;
    std::vector<uint32_t> ln, od;
    for (const Match &m : got) { st.push_back(m.start); ln.push_back(m.len); od.push_back(m.ord); }
    HlCand lanes[kHlLanes];
    for (uint32_t lane = 0; lane < kHlLanes; lane++) {
      HlCand best{0, 0, 0, 0, 0, 0};
      for (uint64_t i = lane; i < got.size(); i += kHlLanes) {
        const HlCand c = hl_window(st.data(), ln.data(), od.data(), got.size(), i, W);
        if (hl_better(c, best)) best = c;
      }
      lanes[lane] = best;
    }
    HlCand best = lanes[0];
    for (uint32_t lane = 1; lane < kHlLanes; lane++)
      if (hl_better(lanes[lane], best)) best = lanes[lane];
    uint64_t a, b;
    hl_range(doc, L, W, best, &a, &b);
    CHECK(a <= b && b <= L && b - a <= W);
    printf("case %u %zu %llu %llu\n", ci, got.size(), (unsigned long long)a, (unsigned long long)b);
    for (const Match &m : got) printf("%llu %u %u\n", (unsigned long long)m.start, m.len, m.ord);
    free(doc);
  }
  fclose(f);
  printf("ok %u\n", n_cases);
  return 0;
}
