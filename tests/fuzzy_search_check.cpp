// fuzzy_search_check.cpp — stand-alone host checker of csrc/fuzzy_search_plan.h
// (built by test_fuzzy_search_cpu.py with the host compiler under ASan + UBSan).
//
//   fuzzy_search_check boost       for ed 0..2, m 1..255: "ed m keep boost_bits key"
//     (boost bits and the sort key of term 0 in hex)
//   fuzzy_search_check compare FILE   u32 n, then (u32 as_text, u32 len, bytes)
//     each: a candidate behind the cursor the device would use (as_text 0: the
//     exact dictionary key, which must exist; 1: the raw bytes as a reference
//     occurrence, lower-cased on the way).  Prints n lines of n signs (- 0 +):
//     fzs_compare(candidate i, candidate j).
//   fuzzy_search_check select FILE    u32 n_vocab, then (u32 len, bytes, u32 df)
//     each; u32 n_cases, then (u32 max_edits, u32 prefix_len, u32 E, u32 len,
//     bytes) each.  The selection as the device makes it: candidates by
//     fz_match and fzs_keep, sorted by fzs_sort_key alone (ties left in reverse
//     byte order), fzs_straddle, the group's smallest by fzs_compare, the final
//     order by (boost group, fzs_compare).  Prints "case i n_within n_out" and
//     per entry "dist boost_bits hex".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fuzzy_search_plan.h"

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

// the candidate as the device sees a vocabulary term: its exact key where one exists, else its bytes
static FzsCand cand_of(const std::string &s, bool force_text) {
  if (!force_text) {
    KeyBuilder kb;
    for (char c : s) kb.push((uint8_t)c);
    uint64_t lo, hi;
    kb.finish(&lo, &hi);
    FzWordCursor w;
    uint32_t n = 0;
    if (!s.empty() && fz_key_words(lo, hi, &w, &n)) return fzs_cand_words(w, n);
  }
  return fzs_cand_text((const uint8_t *)s.data(), (uint32_t)s.size());
}

struct Cand {
  std::string term;
  uint64_t key;
};

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: fuzzy_search_check boost | compare FILE | select FILE\n"); return 2; }
  const std::string mode = argv[1];
  if (mode == "boost") {
    for (uint32_t ed = 0; ed <= kFzMaxEdits; ed++)
      for (uint32_t m = 1; m <= kMaxTokenLen; m++) {
        const uint64_t k = fzs_sort_key(0, ed, m);
        if (fzs_key_dist(k) != ed || fzs_key_boost_bits(k) != fzs_float_bits(fzs_boost(ed, m)) || fzs_key_term(k) != 0 ||
            fzs_key_term(fzs_sort_key(255, ed, m)) != 255) {
          fprintf(stderr, "key of (%u, %u) does not decode\n", ed, m);
          return 3;
        }
        printf("%u %u %d %08x %012llx\n", ed, m, fzs_keep(ed, m) ? 1 : 0, fzs_float_bits(fzs_boost(ed, m)),
               (unsigned long long)k);
      }
    printf("ok\n");
    return 0;
  }
  if (argc != 3) return 2;
  FILE *f = fopen(argv[2], "rb");
  if (!f) { perror(argv[2]); return 2; }
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
  fclose(f);
  if (mode == "compare") {
    const uint32_t nv = rd32();
    std::vector<std::string> raw(nv);
    std::vector<uint32_t> as_text(nv);
    for (uint32_t i = 0; i < nv; i++) { as_text[i] = rd32(); raw[i] = rdstr(); }
    for (uint32_t i = 0; i < nv; i++) {
      const FzsCand a = cand_of(raw[i], as_text[i] != 0);
      if (!as_text[i] && a.text) { fprintf(stderr, "'%s' has no exact key\n", raw[i].c_str()); return 3; }
      std::string line(nv, '0');
      for (uint32_t j = 0; j < nv; j++) {
        const int c = fzs_compare(a, cand_of(raw[j], as_text[j] != 0));
        line[j] = c < 0 ? '-' : (c > 0 ? '+' : '0');
      }
      printf("%s\n", line.c_str());
    }
    printf("ok %u\n", nv);
  } else if (mode == "select") {
    const uint32_t nv = rd32();
    std::vector<std::pair<std::string, uint32_t>> vocab(nv);
    for (auto &v : vocab) { v.first = rdstr(); v.second = rd32(); }
    const uint32_t nc = rd32();
    std::vector<uint32_t> cps(kMaxTokenLen);
    for (uint32_t i = 0; i < nc; i++) {
      const uint32_t max_edits = rd32(), prefix_len = rd32(), E = rd32();
      const std::string t = rdstr();
      if (E < 1 || E > kFzsMaxExpansions) return 2;
      const uint32_t nt = t.size() > 4 * kMaxTokenLen ? 0 : fz_decode_term((const uint8_t *)t.data(), t.size(), cps.data());
      std::vector<Cand> all;
      if (nt)
        for (auto &v : vocab) {
          if (v.second < 1) continue;
          const FzsCand c = cand_of(v.first, false);
          const uint32_t d = c.text ? fz_match(cps.data(), nt, c.t, c.n, max_edits, prefix_len)
                                    : fz_match(cps.data(), nt, c.w, c.n, max_edits, prefix_len);
          if (d == kFzFar || !fzs_keep(d, fzs_min_len(nt, c.n))) continue;
          all.push_back(Cand{v.first, fzs_sort_key(0, d, fzs_min_len(nt, c.n))});
        }
      // the radix sort orders by the key alone; leave the ties in the worst order for the selection
      std::sort(all.begin(), all.end(), [](const Cand &x, const Cand &y) {
        if (x.key != y.key) return x.key < y.key;
        return x.term > y.term;
      });
      std::vector<uint64_t> keys;
      for (const Cand &c : all) keys.push_back(c.key);
      const uint32_t c = (uint32_t)all.size();
      uint32_t g0, g1, r;
      fzs_straddle(keys.data(), c, E, &g0, &g1, &r);
      if (g0 > g1 || g1 > c || g0 + r > std::min(c, E) || (r && (g0 + r != E || g1 - g0 <= r))) {
        fprintf(stderr, "straddle plan (%u, %u, %u) of %u candidates, E = %u\n", g0, g1, r, c, E);
        return 3;
      }
      std::vector<Cand> out(all.begin(), all.begin() + g0);
      if (r) {
        // the r smallest of the group, kept ascending: insertion as the wave inserts
        std::vector<Cand> kept;
        for (uint32_t j = g0; j < g1; j++) {
          const FzsCand cj = cand_of(all[j].term, false);
          if (kept.size() == r && fzs_compare(cj, cand_of(kept.back().term, false)) >= 0) continue;
          size_t pos = 0;
          while (pos < kept.size() && fzs_compare(cand_of(kept[pos].term, false), cj) < 0) pos++;
          kept.insert(kept.begin() + pos, all[j]);
          if (kept.size() > r) kept.pop_back();
        }
        out.insert(out.end(), kept.begin(), kept.end());
      }
      std::stable_sort(out.begin(), out.end(), [](const Cand &x, const Cand &y) {
        if (fzs_key_group(x.key) != fzs_key_group(y.key)) return fzs_key_group(x.key) < fzs_key_group(y.key);
        return fzs_compare(cand_of(x.term, false), cand_of(y.term, false)) < 0;
      });
      printf("case %u %u %zu\n", i, c, out.size());
      for (const Cand &o : out) {
        printf("%u %08x ", fzs_key_dist(o.key), fzs_key_boost_bits(o.key));
        for (char ch : o.term) printf("%02x", (unsigned)(uint8_t)ch);
        printf("\n");
      }
    }
    printf("ok %u\n", nc);
  } else {
    return 2;
  }
  return 0;
}
