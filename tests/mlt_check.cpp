// mlt_check.cpp — csrc/mlt_plan.h on the host, without a device: the rules the
// more-like-this kernels and the host around them share, run over the cases of
// a binary file (tests/test_mlt_cpu.py writes it and compares the output with
// mlt_ref.py).  Built with the host compiler under ASan + UBSan.
//
// File: u64 num_docs | u32 max_terms | u32 n_seeds, per seed: u32 c, c x (u32 tf, u32 df) |
//       u32 n_counts, n_counts x u32 | u32 n_budgets, n_budgets x u64
// Output: "idf <df> <bits>" for df 0..num_docs; "keys ok"; per seed "take <seed> <n>" and the
// taken "<score bits> <tf> <df>" lines in device order; per budget "cuts <budget> c0 c1 ..."; "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "mlt_plan.h"

using namespace tfidf;

static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "mlt_check: %s failed (line %d)\n", #c, __LINE__); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static int check_keys() {
  const float scores[] = {1.0f, 1.0000001f, 2.5f, 220076.69f, 3.4e38f, 1.17549435e-38f};
  const uint32_t seeds[] = {0u, 1u, 255u, 65535u};
  for (float a : scores)
    for (uint32_t s : seeds) {
      const uint64_t k = mlt_key(s, a);
      CHECK(mlt_key_seed(k) == s && mlt_key_score_bits(k) == mlt_float_bits(a));
      for (float b : scores)
        for (uint32_t t : seeds) {
          const uint64_t k2 = mlt_key(t, b);
          // ascending key order = seed ascending, then score descending
          CHECK((k < k2) == (s != t ? s < t : a > b));
        }
    }
  const uint32_t slots[] = {0u, 1u, 262143u, 0xFFFFFFFEu}, tfs[] = {1u, 2u, 65535u, kMaxTf};
  for (uint32_t s : slots)
    for (uint32_t t : tfs) CHECK(mlt_val_slot(mlt_val(s, t)) == s && mlt_val_tf(mlt_val(s, t)) == t);
  CHECK(mlt_key_bits(1) == 33 && mlt_key_bits(2) == 33 && mlt_key_bits(3) == 34 && mlt_key_bits(256) == 40 &&
        mlt_key_bits(257) == 41 && mlt_key_bits(65536) == 48);
  // every seed index of a chunk fits the sorted bits
  for (uint32_t n : {1u, 2u, 3u, 100u, 65536u}) CHECK(((uint64_t)(n - 1) << 32) >> mlt_key_bits(n) == 0);
  const MltRules r{2, 5, 0, 25}, r2{1, 1, 7, 25};
  CHECK(mlt_keep(r, 2, 5) && !mlt_keep(r, 1, 5) && !mlt_keep(r, 2, 4) && mlt_keep(r, 9, 1u << 30));
  CHECK(mlt_keep(r2, 1, 7) && !mlt_keep(r2, 1, 8) && mlt_keep(r2, 1, 1));
  // row segments: split[r] = first entry past range r
  const uint32_t split[4] = {3, 3, 10, 0};                           // the last range takes the rest
  const uint32_t want[12] = {0, 0, 0, 2, 2, 2, 2, 2, 2, 2, 3, 3};
  for (uint32_t i = 0; i < 12; i++) CHECK(mlt_range_of(split, 4u, i) == want[i]);
  const uint32_t one[1] = {0};
  CHECK(mlt_range_of(one, 1u, 5) == 0);
  // flattened entries -> seed, empty rows between
  const uint64_t off[7] = {0, 0, 4, 4, 4, 9, 9};                     // rows of 0, 4, 0, 0, 5, 0 entries
  const uint32_t seed_of[9] = {1, 1, 1, 1, 4, 4, 4, 4, 4};
  for (uint64_t e = 0; e < 9; e++) CHECK(mlt_seed_of(off, 6, e) == seed_of[e]);
  CHECK(mlt_seed_of(off + 1, 3, 0) == 0 && mlt_seed_of(off + 4, 1, 6) == 0);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t num_docs = 0;
  uint32_t max_terms = 0, n_seeds = 0;
  if (!rd(f, &num_docs, 8) || !rd(f, &max_terms, 4) || !rd(f, &n_seeds, 4)) return 2;
  std::vector<float> idf;
  mlt_idf_table(num_docs, &idf);
  for (uint64_t df = 0; df <= num_docs; df++) printf("idf %llu %u\n", (unsigned long long)df, mlt_float_bits(idf[df]));
  if (check_keys()) return 1;
  printf("keys ok\n");

  // the device's part of the selection: keys of all seeds in one array, sorted, mlt_select per segment
  struct Cand {
    uint64_t key, val;
    uint32_t df;
  };
  std::vector<Cand> all;
  std::vector<uint32_t> seg(1, 0);
  for (uint32_t s = 0; s < n_seeds; s++) {
    uint32_t c = 0;
    if (!rd(f, &c, 4)) return 2;
    for (uint32_t i = 0; i < c; i++) {
      uint32_t tf = 0, df = 0;
      if (!rd(f, &tf, 4) || !rd(f, &df, 4) || df > num_docs) return 2;
      all.push_back(Cand{mlt_key(s, mlt_score(tf, idf[df])), mlt_val(i, tf), df});
    }
    seg.push_back((uint32_t)all.size());
  }
  std::stable_sort(all.begin(), all.end(), [](const Cand &a, const Cand &b) { return a.key < b.key; });
  std::vector<uint64_t> keys(all.size());
  for (size_t i = 0; i < all.size(); i++) keys[i] = all[i].key;
  for (uint32_t s = 0; s < n_seeds; s++) {
    const uint32_t take = mlt_select(keys.data() + seg[s], seg[s + 1] - seg[s], max_terms);
    if (take > seg[s + 1] - seg[s]) return 1;
    printf("take %u %u\n", s, take);
    for (uint32_t i = 0; i < take; i++) {
      const Cand &c = all[seg[s] + i];
      if (mlt_key_seed(c.key) != s) return 1;
      printf("%u %u %u\n", mlt_key_score_bits(c.key), mlt_val_tf(c.val), c.df);
    }
  }

  uint32_t n_counts = 0, n_budgets = 0;
  if (!rd(f, &n_counts, 4)) return 2;
  std::vector<uint32_t> counts(n_counts);
  if (n_counts && !rd(f, counts.data(), (size_t)n_counts * 4)) return 2;
  if (!rd(f, &n_budgets, 4)) return 2;
  for (uint32_t b = 0; b < n_budgets; b++) {
    uint64_t budget = 0;
    if (!rd(f, &budget, 8)) return 2;
    std::vector<uint64_t> cuts;
    mlt_plan_chunks(counts.data(), 0, n_counts, budget, &cuts);
    printf("cuts %llu", (unsigned long long)budget);
    for (uint64_t c : cuts) printf(" %llu", (unsigned long long)c);
    printf("\n");
  }
  fclose(f);
  printf("ok\n");
  return 0;
}
