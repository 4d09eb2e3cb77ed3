// wildcard_check.cpp — stand-alone host checker of csrc/wildcard_plan.h (built
// by test_wildcard_cpu.py with the host compiler under ASan + UBSan).
//
//   wildcard_check pairs FILE    u32 n, then (u32 lp, pattern, u32 lc,
//     candidate) each: prints "elements match" (elements 0 = a pattern that
//     matches nothing).
//   wildcard_check lookup FILE   vocabulary + cases -> the terms of each case
//     FILE: u32 n_vocab, then (u32 len, bytes, u32 df) each; u32 n_cases, then
//     (u32 max_out, u32 len, bytes) each.  The cases go through the scan and
//     match chunk plans (limits given first: u32 match budget); prints "case i
//     n_matched n_out" and per term "df hex".
//   wildcard_check plan FILE     u32 mode (0 scan chunks, 1 match chunks, 2
//     union chunks), u32 n, u32 limit_a, u32 limit_b, n x u32: the cut points.
// Every candidate of <= 16 bytes (ASCII) or <= 14 bytes (non-ASCII) is also
// walked as the exact dictionary key the device decodes (KeyBuilder ->
// fz_key_words -> FzWordCursor); a disagreement with the byte cursor aborts.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "wildcard_plan.h"

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

// pattern elements against candidate bytes, by both cursors where an exact key exists
static bool match(const uint32_t *el, uint32_t n, const std::string &cand) {
  const uint8_t *cb = (const uint8_t *)cand.data();
  const uint32_t m = fz_text_cps(cb, (uint32_t)cand.size());
  const FzTextCursor tc{cb, (uint32_t)cand.size(), 0};
  const WcMeta meta = wc_meta(el, n);
  const bool r = wc_match(el, n, meta, tc, m);
  KeyBuilder kb;
  for (char c : cand) kb.push((uint8_t)c);
  uint64_t lo, hi;
  kb.finish(&lo, &hi);
  FzWordCursor wc;
  uint32_t wm = 0;
  if (!cand.empty() && fz_key_words(lo, hi, &wc, &wm)) {
    if (wm != m) { fprintf(stderr, "key of '%s': %u code points, text %u\n", cand.c_str(), wm, m); exit(3); }
    if (wc_match(el, n, meta, wc, wm) != r) { fprintf(stderr, "key cursor != text cursor on '%s'\n", cand.c_str()); exit(3); }
  }
  return r;
}

struct Term {
  std::string term;
  uint32_t df;
};

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: wildcard_check lookup|pairs|plan FILE\n"); return 2; }
  FILE *f = fopen(argv[2], "rb");
  if (!f) { perror(argv[2]); return 2; }
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
  fclose(f);
  const std::string mode = argv[1];
  if (mode == "pairs") {
    const uint32_t np = rd32();
    // the elements live in an exactly sized heap block, so a write past kWcMaxElems is an ASan error
    std::vector<uint32_t> el(kWcMaxElems);
    for (uint32_t i = 0; i < np; i++) {
      const std::string p = rdstr(), c = rdstr();
      const uint32_t ne = wc_parse((const uint8_t *)p.data(), p.size(), el.data());
      printf("%u %d\n", ne, ne && match(el.data(), ne, c) ? 1 : 0);
    }
    printf("ok %u\n", np);
  } else if (mode == "lookup") {
    const uint32_t budget = rd32();
    const uint32_t nv = rd32();
    std::vector<std::pair<std::string, uint32_t>> vocab(nv);
    for (auto &v : vocab) { v.first = rdstr(); v.second = rd32(); }
    const uint32_t nc = rd32();
    std::vector<uint32_t> max_out(nc), n_el(nc);
    std::vector<std::vector<uint32_t>> els(nc);
    std::vector<uint32_t> el(kWcMaxElems);
    for (uint32_t i = 0; i < nc; i++) {
      max_out[i] = rd32();
      const std::string p = rdstr();
      n_el[i] = wc_parse((const uint8_t *)p.data(), p.size(), el.data());
      els[i].assign(el.begin(), el.begin() + n_el[i]);
    }
    // as the host does: scan chunks, a count per pattern, match chunks, then the lists
    std::vector<std::vector<Term>> out(nc);
    std::vector<uint64_t> cuts, sub;
    wc_plan_scan_chunks(n_el.data(), nc, &cuts);
    FzStage st;
    uint32_t seen = 0;
    for (size_t ci = 0; ci + 1 < cuts.size(); ci++) {
      const uint64_t t0 = cuts[ci], nt = cuts[ci + 1] - t0;
      fz_stage_terms(els, t0, t0 + nt, &st);
      if (nt > kWcChunkPatterns || st.cps.size() > kWcChunkElems) { fprintf(stderr, "scan chunk over its limits\n"); return 3; }
      std::vector<uint32_t> counts(nt, 0);
      for (uint64_t t = 0; t < nt; t++) {
        const uint32_t *e = st.cps.data() + st.off[t], ne = st.off[t + 1] - st.off[t];
        for (auto &v : vocab)
          if (v.second >= 1 && ne && match(e, ne, v.first)) counts[t]++;
      }
      sub.clear();
      wc_plan_match_chunks(counts.data(), 0, nt, budget, &sub);
      for (size_t si = 0; si + 1 < sub.size(); si++)
        for (uint64_t t = sub[si]; t < sub[si + 1]; t++) {
          const uint32_t *e = st.cps.data() + st.off[t], ne = st.off[t + 1] - st.off[t];
          for (auto &v : vocab)
            if (v.second >= 1 && ne && match(e, ne, v.first)) out[t0 + t].push_back(Term{v.first, v.second});
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
    const uint32_t which = rd32(), cnt = rd32(), la = rd32(), lb = rd32();
    std::vector<uint32_t> v(cnt);
    for (auto &x : v) x = rd32();
    std::vector<uint64_t> cuts;
    if (which == 0) wc_plan_scan_chunks(v.data(), cnt, &cuts);
    else if (which == 1) wc_plan_match_chunks(v.data(), 0, cnt, la, &cuts);
    else wc_plan_union_chunks(0, cnt, la, lb, &cuts);
    for (uint64_t c : cuts) printf("%llu\n", (unsigned long long)c);
    printf("ok %zu\n", cuts.size());
  } else {
    return 2;
  }
  return 0;
}
