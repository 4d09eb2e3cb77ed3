// regex_check.cpp — stand-alone host checker of csrc/regex_plan.h (built by
// test_regex_cpu.py with the host compiler under ASan + UBSan).
//
//   regex_check pairs FILE     u32 n, then (pattern, u32 m, m subjects) each:
//     prints "status states classes bits" (status 0 ok, 1 syntax error, 2
//     unsupported; bits: one 0/1 per subject, "-" for none).
//   regex_check table FILE     u32 n, then n patterns: prints "status
//     err_at hex" (hex: the serialised table's words, "-" for none).
//   regex_check lookup FILE    vocabulary + cases -> the terms of each case
//     FILE: u32 match budget, u32 table budget, u32 n_vocab, then (u32 len,
//     bytes, u32 df) each; u32 n_cases, then (u32 max_out, u32 len, bytes)
//     each.  The cases go through the scan and match chunk plans; prints
//     "case i n_matched n_out" and per term "df hex".
//   regex_check plan FILE      u32 n, u32 budget, n x u32 table bytes: the cut points.
// (strings: u32 length, bytes.)  Every candidate of <= 16 bytes (ASCII) or <=
// 14 bytes (non-ASCII) is also walked as the exact dictionary key the device
// decodes (KeyBuilder -> fz_key_words -> FzWordCursor); a disagreement with
// the byte cursor aborts.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "regex_plan.h"

using namespace tfidf;

static std::vector<uint8_t> data;
static size_t at = 0;

static uint32_t rd32() {
  if (at + 4 > data.size()) { fprintf(stderr, "truncated input\n"); exit(2); }
  uint32_t v;
  memcpy(&v, data.data() + at, 4);
  at += 4;
  return v;
}
static std::string rdstr() {
  const uint32_t n = rd32();
  if (at + n > data.size()) { fprintf(stderr, "truncated input\n"); exit(2); }
  std::string s((const char *)data.data() + at, n);
  at += n;
  return s;
}

// a table against candidate bytes, by both cursors where an exact key exists
static bool match(const std::vector<uint32_t> &table, const std::string &cand) {
  if (table.empty()) return false;
  // the table lives in an exactly sized heap block, so a read past it is an ASan error
  const uint8_t *cb = (const uint8_t *)cand.data();
  const uint32_t m = fz_text_cps(cb, (uint32_t)cand.size());
  const FzTextCursor tc{cb, (uint32_t)cand.size(), 0};
  const bool r = rx_match(table.data(), tc, m);
  KeyBuilder kb;
  for (char c : cand) kb.push((uint8_t)c);
  uint64_t lo, hi;
  kb.finish(&lo, &hi);
  FzWordCursor wc;
  uint32_t wm = 0;
  if (!cand.empty() && fz_key_words(lo, hi, &wc, &wm)) {
    if (wm != m) { fprintf(stderr, "key of '%s': %u code points, text %u\n", cand.c_str(), wm, m); exit(3); }
    if (rx_match(table.data(), wc, wm) != r) { fprintf(stderr, "key cursor != text cursor on '%s'\n", cand.c_str()); exit(3); }
  }
  return r;
}

struct Term {
  std::string term;
  uint32_t df;
};

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: regex_check pairs|table|lookup|plan FILE\n"); return 2; }
  FILE *f = fopen(argv[2], "rb");
  if (!f) { perror(argv[2]); return 2; }
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
  fclose(f);
  const std::string mode = argv[1];
  if (mode == "pairs") {
    const uint32_t np = rd32();
    std::vector<uint32_t> table;
    for (uint32_t i = 0; i < np; i++) {
      const std::string p = rdstr();
      const int st = rx_compile((const uint8_t *)p.data(), p.size(), &table, nullptr);
      const uint32_t m = rd32();
      printf("%d %u %u ", st, table.empty() ? 0u : table[1] & 0xFFFFu, table.empty() ? 0u : table[1] >> 16);
      if (table.size() * 4 > kRxMaxTableBytes || (!table.empty() && table[0] != table.size())) { fprintf(stderr, "table size is off\n"); return 3; }
      for (uint32_t k = 0; k < m; k++) {
        const std::string c = rdstr();
        putchar(st == kRxOk && match(table, c) ? '1' : '0');
      }
      printf(m ? "\n" : "-\n");
    }
    printf("ok %u\n", np);
  } else if (mode == "table") {
    const uint32_t np = rd32();
    std::vector<uint32_t> table;
    for (uint32_t i = 0; i < np; i++) {
      const std::string p = rdstr();
      uint64_t err_at = 0;
      const int st = rx_compile((const uint8_t *)p.data(), p.size(), &table, &err_at);
      printf("%d %llu ", st, (unsigned long long)err_at);
      for (uint32_t w : table) printf("%08x", w);
      printf(table.empty() ? "-\n" : "\n");
    }
    printf("ok %u\n", np);
  } else if (mode == "lookup") {
    const uint32_t budget = rd32(), table_budget = rd32();
    const uint32_t nv = rd32();
    std::vector<std::pair<std::string, uint32_t>> vocab(nv);
    for (auto &v : vocab) { v.first = rdstr(); v.second = rd32(); }
    const uint32_t nc = rd32();
    std::vector<uint32_t> max_out(nc), n_bytes(nc);
    std::vector<std::vector<uint32_t>> tabs(nc);
    for (uint32_t i = 0; i < nc; i++) {
      max_out[i] = rd32();
      const std::string p = rdstr();
      if (rx_compile((const uint8_t *)p.data(), p.size(), &tabs[i], nullptr) != kRxOk) { fprintf(stderr, "case %u does not compile\n", i); return 3; }
      if (rx_table_matches_nothing(tabs[i])) tabs[i].clear();
      n_bytes[i] = (uint32_t)tabs[i].size() * 4;
    }
    // as the host does: scan chunks, a count per pattern, match chunks, then the lists
    std::vector<std::vector<Term>> out(nc);
    std::vector<uint64_t> cuts, sub;
    rx_plan_scan_chunks(n_bytes.data(), nc, table_budget, &cuts);
    FzStage st;
    uint32_t seen = 0;
    for (size_t ci = 0; ci + 1 < cuts.size(); ci++) {
      const uint64_t t0 = cuts[ci], nt = cuts[ci + 1] - t0;
      fz_stage_terms(tabs, t0, t0 + nt, &st);
      if (nt > kWcChunkPatterns || st.cps.size() > kRxStageWords) { fprintf(stderr, "scan chunk over its limits\n"); return 3; }
      std::vector<uint32_t> counts(nt, 0);
      // the staged image in an exactly sized block, walked at the staged offsets
      auto tab_of = [&](uint64_t t) { return std::vector<uint32_t>(st.cps.begin() + st.off[t], st.cps.begin() + st.off[t + 1]); };
      for (uint64_t t = 0; t < nt; t++) {
        const std::vector<uint32_t> tb = tab_of(t);
        for (auto &v : vocab)
          if (v.second >= 1 && match(tb, v.first)) counts[t]++;
      }
      sub.clear();
      wc_plan_match_chunks(counts.data(), 0, nt, budget, &sub);
      for (size_t si = 0; si + 1 < sub.size(); si++)
        for (uint64_t t = sub[si]; t < sub[si + 1]; t++) {
          const std::vector<uint32_t> tb = tab_of(t);
          for (auto &v : vocab)
            if (v.second >= 1 && match(tb, v.first)) out[t0 + t].push_back(Term{v.first, v.second});
          if (out[t0 + t].size() != counts[t]) { fprintf(stderr, "fill != count\n"); return 3; }
          seen++;
        }
    }
    if (seen != nc) { fprintf(stderr, "the plans covered %u of %u patterns\n", seen, nc); return 3; }
    for (uint32_t i = 0; i < nc; i++) {
      // the device orders by the packed key, the host breaks ties by bytes
      std::sort(out[i].begin(), out[i].end(), [](const Term &x, const Term &y) {
        const uint64_t kx = wc_sort_key(0, x.df), ky = wc_sort_key(0, y.df);
        if (kx != ky) return kx < ky;
        return x.term < y.term;
      });
      const size_t n_out = std::min<size_t>(out[i].size(), max_out[i]);
      printf("case %u %zu %zu\n", i, out[i].size(), n_out);
      for (size_t j = 0; j < n_out; j++) {
        printf("%u ", out[i][j].df);
        for (char c : out[i][j].term) printf("%02x", (unsigned)(uint8_t)c);
        printf("\n");
      }
    }
    printf("ok %u\n", nc);
  } else if (mode == "plan") {
    const uint32_t cnt = rd32(), budget = rd32();
    std::vector<uint32_t> v(cnt);
    for (auto &x : v) x = rd32();
    std::vector<uint64_t> cuts;
    rx_plan_scan_chunks(v.data(), cnt, budget, &cuts);
    for (uint64_t c : cuts) printf("%llu\n", (unsigned long long)c);
    printf("ok %zu\n", cuts.size());
  } else {
    return 2;
  }
  return 0;
}
