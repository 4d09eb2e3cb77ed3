// fuzzy_host_scan.cpp — the host route tools/bench_fuzzy.py measures the device
// against: one thread running the rules of csrc/fuzzy_plan.h over the exported
// vocabulary strings, as a caller without tfidf_fuzzy_terms would have to.
//   fuzzy_host_scan FILE
//     FILE: u32 max_edits, u32 prefix_len, u32 n_vocab, then (u32 len, bytes)
//     each; u32 n_terms, then (u32 len, bytes) each.
// Prints "ms candidates": the time of the scan alone (the file is in memory,
// the vocabulary decoded to code points before the clock starts) and the
// candidates found over all terms.  No ordering and no output: the device
// call's time includes both.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
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

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint8_t> buf(1 << 20);
  size_t n;
  while ((n = fread(buf.data(), 1, buf.size(), f)) > 0) data.insert(data.end(), buf.begin(), buf.begin() + n);
  fclose(f);
  const uint32_t max_edits = rd32(), prefix_len = rd32(), nv = rd32();
  std::vector<uint32_t> starts(nv), v_len(nv), v_cnt(nv);
  for (uint32_t i = 0; i < nv; i++) {
    const uint32_t len = rd32();
    if (at + len > data.size()) { fprintf(stderr, "truncated input\n"); return 2; }
    starts[i] = (uint32_t)at;
    v_len[i] = len;
    v_cnt[i] = fz_text_cps(data.data() + at, len);
    at += len;
  }
  const uint32_t nt = rd32();
  std::vector<std::vector<uint32_t>> terms(nt);
  std::vector<uint64_t> t_sig(nt);
  uint32_t cps[kMaxTokenLen];
  for (uint32_t i = 0; i < nt; i++) {
    const uint32_t len = rd32();
    if (at + len > data.size()) { fprintf(stderr, "truncated input\n"); return 2; }
    const uint32_t k = len > 4 * kMaxTokenLen ? 0 : fz_decode_term(data.data() + at, len, cps);
    terms[i].assign(cps, cps + k);
    t_sig[i] = fz_sig_term(cps, k);
    at += len;
  }
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t found = 0;
  for (uint32_t v = 0; v < nv; v++) {
    const FzTextCursor c{data.data() + starts[v], v_len[v], 0};
    const uint32_t m = v_cnt[v];
    const uint64_t sig = fz_sig(c, m);
    for (uint32_t t = 0; t < nt; t++) {
      if (terms[t].empty() || !fz_sig_ok(t_sig[t], sig, max_edits)) continue;
      found += fz_match(terms[t].data(), (uint32_t)terms[t].size(), c, m, max_edits, prefix_len) != kFzFar;
    }
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("%.3f %llu\n", ms, (unsigned long long)found);
  return 0;
}
