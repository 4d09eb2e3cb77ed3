// fuzzy_check.cpp — stand-alone host checker of csrc/fuzzy_plan.h (built by
// test_fuzzy_cpu.py with the host compiler under ASan + UBSan).
//
//   fuzzy_check lookup FILE   vocabulary + cases -> the candidates of each case
//     FILE: u32 n_vocab, then (u32 len, bytes, u32 df) each; u32 n_cases, then
//     (u32 max_edits, u32 prefix_len, u32 max_out, u32 len, bytes) each.
//     Prints "case i n_within n_out" and per candidate "dist df hex".
//   fuzzy_check pairs FILE    u32 n, then (u32 max_edits, u32 prefix_len, u32
//     la, a, u32 lb, b) each: prints fz_match(term a, candidate b) or -1.
//   fuzzy_check plan FILE     u32 mode (0 scan chunks, 1 candidate chunks), u32
//     n, u32 limit_a, u32 limit_b, n x u32: prints the cut points.
// Every candidate of <= 16 bytes (ASCII) or <= 14 bytes (non-ASCII) is also
// walked as the exact dictionary key the device decodes (KeyBuilder ->
// fz_key_words -> FzWordCursor); a disagreement with the byte cursor aborts,
// and so does a pair within the distance that the signature filter rejects.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fuzzy_plan.h"

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

// distance of term (lower-cased code points) and candidate bytes, by both cursors where an exact key exists
static uint32_t match(const uint32_t *term, uint32_t n, const std::string &cand, uint32_t max_edits, uint32_t prefix_len) {
  const uint8_t *cb = (const uint8_t *)cand.data();
  const uint32_t m = fz_text_cps(cb, (uint32_t)cand.size());
  const FzTextCursor tc{cb, (uint32_t)cand.size(), 0};
  const uint32_t d = fz_match(term, n, tc, m, max_edits, prefix_len);
  if (d != kFzFar && !fz_sig_ok(fz_sig_term(term, n), fz_sig(tc, m), max_edits)) {
    fprintf(stderr, "the signature filter rejects '%s' at distance %u\n", cand.c_str(), d);
    exit(3);
  }
  KeyBuilder kb;
  for (char c : cand) kb.push((uint8_t)c);
  uint64_t lo, hi;
  kb.finish(&lo, &hi);
  FzWordCursor wc;
  uint32_t wm = 0;
  if (!cand.empty() && fz_key_words(lo, hi, &wc, &wm)) {
    if (wm != m) { fprintf(stderr, "key of '%s': %u code points, text %u\n", cand.c_str(), wm, m); exit(3); }
    const uint32_t d2 = fz_match(term, n, wc, wm, max_edits, prefix_len);
    if (fz_sig(wc, wm) != fz_sig(tc, m)) { fprintf(stderr, "signatures differ on '%s'\n", cand.c_str()); exit(3); }
    if (d2 != d) { fprintf(stderr, "key cursor %u != text cursor %u on '%s'\n", d2, d, cand.c_str()); exit(3); }
  }
  return d;
}

struct Cand {
  std::string term;
  uint32_t df, dist;
};

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: fuzzy_check lookup|pairs|plan FILE\n"); return 2; }
  FILE *f = fopen(argv[2], "rb");
  if (!f) { perror(argv[2]); return 2; }
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
  fclose(f);
  const std::string mode = argv[1];
  std::vector<uint32_t> cps(kMaxTokenLen);
  if (mode == "lookup") {
    const uint32_t nv = rd32();
    std::vector<std::pair<std::string, uint32_t>> vocab(nv);
    for (auto &v : vocab) { v.first = rdstr(); v.second = rd32(); }
    const uint32_t nc = rd32();
    for (uint32_t i = 0; i < nc; i++) {
      const uint32_t max_edits = rd32(), prefix_len = rd32(), max_out = rd32();
      const std::string t = rdstr();
      const uint32_t nt = t.size() > 4 * kMaxTokenLen ? 0 : fz_decode_term((const uint8_t *)t.data(), t.size(), cps.data());
      std::vector<Cand> out;
      if (nt)
        for (auto &v : vocab) {
          if (v.second < 1) continue;
          const uint32_t d = match(cps.data(), nt, v.first, max_edits, prefix_len);
          if (d != kFzFar) out.push_back(Cand{v.first, v.second, d});
        }
      // the device orders by the packed key, the host breaks ties by bytes
      std::sort(out.begin(), out.end(), [](const Cand &x, const Cand &y) {
        const uint64_t kx = fz_sort_key(0, x.dist, x.df), ky = fz_sort_key(0, y.dist, y.df);
        if (kx != ky) return kx < ky;
        return x.term < y.term;
      });
      const size_t n_out = std::min<size_t>(out.size(), max_out);
      printf("case %u %zu %zu\n", i, out.size(), n_out);
      for (size_t j = 0; j < n_out; j++) {
        printf("%u %u ", out[j].dist, out[j].df);
        for (char c : out[j].term) printf("%02x", (unsigned)(uint8_t)c);
        printf("\n");
      }
    }
    printf("ok %u\n", nc);
  } else if (mode == "pairs") {
    const uint32_t np = rd32();
    for (uint32_t i = 0; i < np; i++) {
      const uint32_t max_edits = rd32(), prefix_len = rd32();
      const std::string a = rdstr(), b = rdstr();
      const uint32_t nt = a.size() > 4 * kMaxTokenLen ? 0 : fz_decode_term((const uint8_t *)a.data(), a.size(), cps.data());
      const uint32_t d = nt ? match(cps.data(), nt, b, max_edits, prefix_len) : kFzFar;
      printf("%d\n", d == kFzFar ? -1 : (int)d);
    }
    printf("ok %u\n", np);
  } else if (mode == "plan") {
    const uint32_t which = rd32(), cnt = rd32(), la = rd32(), lb = rd32();
    std::vector<uint32_t> v(cnt);
    for (auto &x : v) x = rd32();
    std::vector<uint64_t> cuts;
    if (which == 0) fz_plan_scan_chunks(v.data(), cnt, la, lb, &cuts);
    else fz_plan_cand_chunks(v.data(), 0, cnt, la, &cuts);
    for (uint64_t c : cuts) printf("%llu\n", (unsigned long long)c);
    printf("ok %zu\n", cuts.size());
  } else {
    return 2;
  }
  return 0;
}
