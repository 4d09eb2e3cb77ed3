// compound_check.cpp — stand-alone host checker of csrc/compound_plan.h
// (tests/test_compound_cpu.py builds it with the host compiler under
// AddressSanitizer and UBSan).  It reads one binary case file and prints, for
// test_compound_cpu.py to compare with compound_ref.py:
//
//   queries   every query's hits, computed the way the device pass computes
//             them with the header's functions: the clause rows flattened,
//             binned by cq_bin through cq_clause_of, then per (query, block) and
//             per tile the clauses applied in clause order with cq_apply, the
//             survivors chosen by cq_match, scored by cq_score, packed by
//             cq_hit_key and ordered by descending key
//   plans     cq_plan_chunks under each budget
//   checks    cq_check_args on each argument case
//
// File (little endian): u32 n_blocks, u32 n_docs, u32 n_q; per query u32 n_c,
// per clause u8 occur, u32 n, n x (u32 doc, u32 score bits); u64 max_queries,
// u64 max_clauses, u32 n_budgets, u64 budgets; u32 n_cases, per case u32 n_q,
// (n_q + 1) u64 query offsets, u32 n_c, (n_c + 1) u64 payload offsets, n_c x
// (u8 occur, u8 kind).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "compound_plan.h"

using namespace tfidf;

static FILE *g_f;

template <class T> static T rd() {
  T v;
  if (fread(&v, sizeof v, 1, g_f) != 1) {
    fprintf(stderr, "short file\n");
    exit(2);
  }
  return v;
}

struct Entry {
  uint32_t doc, bits;
};

int main(int argc, char **argv) {
  if (argc != 2 || !(g_f = fopen(argv[1], "rb"))) {
    fprintf(stderr, "usage: compound_check case.bin\n");
    return 2;
  }
  const uint32_t n_blocks = rd<uint32_t>(), n_docs = rd<uint32_t>(), n_q = rd<uint32_t>();
  std::vector<uint64_t> q_coff(1, 0), c_off(1, 0), q_entries;
  std::vector<uint32_t> occur;
  std::vector<Entry> rows;
  for (uint32_t q = 0; q < n_q; q++) {
    const uint32_t nc = rd<uint32_t>();
    uint64_t e = 0;
    for (uint32_t c = 0; c < nc; c++) {
      occur.push_back(rd<uint8_t>());
      const uint32_t n = rd<uint32_t>();
      for (uint32_t i = 0; i < n; i++) {
        Entry x;
        x.doc = rd<uint32_t>();
        x.bits = rd<uint32_t>();
        rows.push_back(x);
      }
      e += n;
      c_off.push_back(rows.size());
    }
    q_entries.push_back(e);
    q_coff.push_back(occur.size());
  }
  const uint32_t n_c = (uint32_t)occur.size();
  const uint64_t n_e = rows.size(), n_bins = (uint64_t)n_c * n_blocks;

  // count, scan, scatter: as k_cq_bin and the scan between its two passes
  std::vector<uint64_t> cnt(n_bins + 1, 0), start(n_bins + 1, 0);
  for (uint64_t e = 0; e < n_e; e++) {
    if (rows[e].doc >= n_docs) continue;
    const uint64_t bin = cq_bin(cq_clause_of(c_off.data(), n_c, e), rows[e].doc, n_blocks);
    if (bin >= n_bins) return 3;
    cnt[bin]++;
  }
  for (uint64_t b = 0; b < n_bins; b++) start[b + 1] = start[b] + cnt[b];
  std::vector<uint64_t> cur(start.begin(), start.end());
  std::vector<Entry> binned(n_e ? n_e : 1);
  for (uint64_t e = 0; e < n_e; e++) {
    if (rows[e].doc >= n_docs) continue;
    const uint64_t bin = cq_bin(cq_clause_of(c_off.data(), n_c, e), rows[e].doc, n_blocks);
    const uint64_t at = cur[bin]++;
    if (at >= n_e) return 3;
    binned[at] = rows[e];
  }

  // combine: as k_cq_combine, tile by tile
  std::vector<double> must(kCqTileDocs), shd(kCqTileDocs);
  std::vector<uint8_t> req(kCqTileDocs), flags(kCqTileDocs);
  for (uint32_t q = 0; q < n_q; q++) {
    const uint32_t c0 = (uint32_t)q_coff[q], nc = (uint32_t)(q_coff[q + 1] - q_coff[q]);
    CqNeeds needs{0, 0};
    for (uint32_t c = 0; c < nc; c++) cq_needs_add(&needs, occur[c0 + c]);
    std::vector<uint64_t> keys;
    for (uint32_t b = 0; b < n_blocks; b++)
      for (uint32_t t = 0; t < kCqBlockDocs / kCqTileDocs; t++) {
        const uint32_t d0 = b * kCqBlockDocs + t * kCqTileDocs;
        if (d0 >= n_docs) break;
        std::fill(must.begin(), must.end(), 0.0);
        std::fill(shd.begin(), shd.end(), 0.0);
        std::fill(req.begin(), req.end(), 0);
        std::fill(flags.begin(), flags.end(), 0);
        for (uint32_t c = 0; c < nc; c++) {
          const uint64_t bin = cq_bin(c0 + c, b * kCqBlockDocs, n_blocks);
          for (uint64_t i = start[bin]; i < cur[bin]; i++) {
            const uint32_t ld = binned[i].doc - d0;
            if (ld >= kCqTileDocs) continue;
            float s;
            memcpy(&s, &binned[i].bits, 4);
            cq_apply(occur[c0 + c], s, &req[ld], &flags[ld], &must[ld], &shd[ld]);
          }
        }
        for (uint32_t ld = 0; ld < kCqTileDocs && d0 + ld < n_docs; ld++)
          if (cq_match(needs, req[ld], flags[ld]))
            keys.push_back(cq_hit_key(cq_score(needs, flags[ld], must[ld], shd[ld]), d0 + ld));
      }
    std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
    printf("q %u %zu\n", q, keys.size());
    for (uint64_t k : keys) printf("%u %u\n", (uint32_t)~(uint32_t)k, (uint32_t)(k >> 32));
  }

  const uint64_t max_q = rd<uint64_t>(), max_c = rd<uint64_t>();
  const uint32_t n_budgets = rd<uint32_t>();
  for (uint32_t i = 0; i < n_budgets; i++) {
    const uint64_t budget = rd<uint64_t>();
    std::vector<uint64_t> cuts;
    cq_plan_chunks(q_entries.data(), q_coff.data(), n_q, budget, max_q, max_c, &cuts);
    printf("plan %llu:", (unsigned long long)budget);
    for (uint64_t c : cuts) printf(" %llu", (unsigned long long)c);
    printf("\n");
  }

  const uint32_t n_cases = rd<uint32_t>();
  for (uint32_t i = 0; i < n_cases; i++) {
    const uint32_t nq = rd<uint32_t>();
    std::vector<uint64_t> qo((size_t)nq + 1);
    for (uint64_t &v : qo) v = rd<uint64_t>();
    const uint32_t nc = rd<uint32_t>();
    std::vector<uint64_t> co((size_t)nc + 1);
    for (uint64_t &v : co) v = rd<uint64_t>();
    std::vector<tfidf_clause> cl(nc ? nc : 1);
    for (uint32_t c = 0; c < nc; c++) {
      memset(&cl[c], 0, sizeof cl[c]);
      cl[c].occur = rd<uint8_t>();
      cl[c].kind = rd<uint8_t>();
    }
    uint64_t at = 0;
    const int rc = cq_check_args(co.data(), cl.data(), qo.data(), nq, &at);
    printf("check %d %llu\n", rc, (unsigned long long)at);
  }
  printf("ok\n");
  fclose(g_f);
  return 0;
}
