// A lone inverted block in one launch (csrc/commit_plan.h fuse_plan,
// fuse_tickets, fuse_scratch_must_zero and the host model of k_df_fused's
// finisher):
//   - fuse_plan over 0 / 1 / 2 inverted blocks, both layouts, slices of 1 and
//     more, and every knob (TFIDF_DF_FROM_ROWS, TFIDF_TEST_SCAN_PARTS,
//     TFIDF_INV_UNFUSED), values "0" and "" included;
//   - the ticket count against the slices slice_range leaves with documents,
//     for random (documents, slices) under the plan's own shape and forced
//     slice counts (empty slices included);
//   - the scratch-clean rule over random histories of commits that succeed,
//     fail before their synchronisation, run unfused, or need a larger buffer:
//     a model of the scratch's words must be all zero at every fused launch;
//   - the finisher's arithmetic for random rsplit tables with R = 1, 2, 8 and
//     empty ranges: per range start = sum of `lo`, offsets = start + exclusive
//     scan of the range's counts, total = sum of `hi`, held against a naive
//     exclusive scan of the whole row.
// Stand-alone; built with -fsanitize=address,undefined by test_fuse_plan_cpu.py.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "commit_plan.h"

using namespace tfidf;

static int checks = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    checks++;                                                       \
    if (!(c)) {                                                     \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);           \
      return 1;                                                     \
    }                                                               \
  } while (0)

static bool knob_on(const char *v) { return v && *v && !(v[0] == '0' && !v[1]); }

static int check_fuse_plan() {
  const char *vals[] = {nullptr, "", "0", "1", "4", "yes"};
  const uint32_t slices_of[] = {1, 2, 3, 35, 256};
  for (int term_major = 0; term_major < 2; term_major++)
    for (uint32_t blocks = 0; blocks <= 3; blocks++)
      for (uint32_t slices : slices_of)
        for (const char *rows : vals)
          for (const char *parts : vals)
            for (const char *unf : vals) {
              SlicePlan sp;
              sp.slices = slices;
              sp.slice_docs = slices > 1 ? 240 : (uint32_t)kPlanBlockDocs;
              const bool want = !term_major && blocks == 1 && slices >= 2 && !knob_on(rows) && !(parts && *parts) &&
                                !knob_on(unf);
              CHECK(fuse_plan(term_major != 0, blocks, sp, rows, parts, unf) == want);
            }
  // pinned: bench.py's step (a 576-document tail, 3 slices) is fused; a 383-document tail at R = 1 is one slice
  CHECK(fuse_plan(false, 1, slice_plan(1, 8, 576, 100000, 256, nullptr, nullptr), nullptr, nullptr, nullptr));
  CHECK(!fuse_plan(false, 1, slice_plan(1, 1, 383, 1000, 256, nullptr, nullptr), nullptr, nullptr, nullptr));
  CHECK(!fuse_plan(false, 2, slice_plan(2, 8, 8192, 100000, 256, nullptr, nullptr), nullptr, nullptr, nullptr));
  CHECK(!fuse_plan(false, 1, slice_plan(1, 8, 576, 100000, 256, nullptr, "4"), nullptr, "4", nullptr));
  return 0;
}

static int check_tickets(std::mt19937_64 &rng) {
  const char *slice_knobs[] = {nullptr, "2", "3", "7", "32", "256", "400"};
  const uint32_t ranges[] = {1, 2, 8};
  for (int it = 0; it < 20000; it++) {
    const uint64_t docs = it < 8192 ? (uint64_t)it + 1 : 1 + rng() % kPlanBlockDocs;
    const uint32_t R = ranges[rng() % 3];
    const char *sk = slice_knobs[rng() % 7];
    const SlicePlan sp = slice_plan(1, R, docs, 1000 + (uint32_t)(rng() % 100000), 256, sk, nullptr);
    const uint64_t d0 = (rng() % 200) * kPlanBlockDocs, d1 = d0 + docs;
    uint32_t nonempty = 0;
    bool gap = false;                      // the slices with documents are the first ones
    for (uint32_t i = 0; i < sp.slices; i++) {
      uint64_t lo, hi;
      slice_range(sp, i, d0, d1, &lo, &hi);
      if (lo < hi) {
        CHECK(!gap);
        nonempty++;
      } else {
        gap = true;
      }
    }
    CHECK(nonempty >= 1);
    CHECK(fuse_tickets(sp, docs) == nonempty);
  }
  SlicePlan sp;
  CHECK(fuse_tickets(sp, 0) == 0);
  return 0;
}

// The scratch as the device sees it: `dirty` when a fused kernel was launched
// and did not run to its end; `garbage` in words a new allocation brings.
static int check_scratch_rule(std::mt19937_64 &rng) {
  for (int trial = 0; trial < 400; trial++) {
    FuseScratch st;
    uint64_t alloc = 0;                    // words the device buffer holds
    bool zero_on_device = false;           // every allocated word is zero
    for (int step = 0; step < 60; step++) {
      const int kind = (int)(rng() % 10);
      if (kind == 0) continue;             // an unfused commit: the scratch is not touched
      const uint64_t need = 1 + rng() % (kind < 3 ? 200000 : 2000);
      bool grow = false;
      const bool zero = fuse_scratch_must_zero(st, need, &grow);
      CHECK(grow == (need > st.words));
      uint64_t words = st.words;
      if (grow) {
        st = FuseScratch{};
        if (rng() % 16 == 0) {             // the allocation fails: nothing is kept, the commit returns
          alloc = 0;
          zero_on_device = false;
          continue;
        }
        alloc = words = need + need / 8 + 4096;
        zero_on_device = false;            // fresh memory
      }
      CHECK(words == alloc && words >= need);
      if (zero) zero_on_device = true;     // hipMemsetAsync over the whole buffer
      CHECK(zero_on_device);               // what the kernel relies on
      fuse_scratch_launch(&st, words);
      CHECK(!st.clean && st.words == alloc);
      const int end = (int)(rng() % 8);
      if (end == 0) {                      // an error before the launch or before the synchronisation returned
        zero_on_device = rng() % 2 == 0;   // (the kernel may or may not have run)
        continue;
      }
      // the kernel ran to its end: the finishers left every word zero
      fuse_scratch_done(&st);
      CHECK(st.clean);
      // (a commit that fails after this point, a collision found at the end, leaves a clean scratch)
    }
  }
  return 0;
}

static int check_finisher_model(std::mt19937_64 &rng) {
  const uint32_t ranges[] = {1, 2, 8};
  for (int it = 0; it < 600; it++) {
    const uint32_t R = ranges[it % 3];
    const uint64_t n_docs = 1 + rng() % (it % 7 == 0 ? 3000 : 300);
    const uint32_t cols_per_range_max = 1 + (uint32_t)(rng() % 40);
    // columns of each range (some ranges have none)
    std::vector<uint32_t> c_first(R + 1, 0);
    std::vector<bool> empty_range(R, false);
    for (uint32_t r = 0; r < R; r++) {
      empty_range[r] = rng() % 4 == 0;
      c_first[r + 1] = c_first[r] + (empty_range[r] ? 0u : 1u + (uint32_t)(rng() % cols_per_range_max));
    }
    const uint32_t NC = c_first[R];
    // each document holds a few distinct columns; rsplit = its entries up to the end of each range
    std::vector<uint32_t> rsplit(n_docs * R, 0), counts(NC, 0);
    for (uint64_t d = 0; d < n_docs; d++) {
      uint32_t run = 0;
      for (uint32_t r = 0; r < R; r++) {
        const uint32_t nc = c_first[r + 1] - c_first[r];
        const uint32_t take = nc && rng() % 3 ? (uint32_t)(rng() % (std::min(nc, 6u) + 1)) : 0u;
        // `take` distinct columns of the range: a random start, consecutive
        const uint32_t from = nc ? (uint32_t)(rng() % nc) : 0u;
        for (uint32_t j = 0; j < take; j++) counts[c_first[r] + (from + j) % nc]++;
        run += take;
        rsplit[d * R + r] = run;
      }
    }
    // the naive scan of the whole row
    std::vector<uint32_t> want(NC, 0);
    uint64_t total = 0;
    for (uint32_t c = 0; c < NC; c++) {
      want[c] = (uint32_t)total;
      total += counts[c];
    }
    // the model: every range on its own, in any order
    std::vector<uint32_t> got(NC, 0xFFFFFFFFu);
    std::vector<uint32_t> order(R);
    for (uint32_t r = 0; r < R; r++) order[r] = r;
    std::shuffle(order.begin(), order.end(), rng);
    for (uint32_t r : order) {
      const uint64_t start = fuse_range_start(rsplit.data(), n_docs, R, r);
      const uint64_t end = fuse_range_offsets(counts.data(), c_first[r], c_first[r + 1], start, got.data());
      // the offset behind the range is the next range's start, and the total behind the last
      if (r + 1 < R) CHECK(end == fuse_range_start(rsplit.data(), n_docs, R, r + 1));
      else CHECK(end == fuse_block_total(rsplit.data(), n_docs, R));
      if (empty_range[r]) CHECK(end == start);
    }
    CHECK(fuse_block_total(rsplit.data(), n_docs, R) == total);
    CHECK(fuse_range_start(rsplit.data(), n_docs, R, 0) == 0);
    for (uint32_t c = 0; c < NC; c++) CHECK(got[c] == want[c]);
    // the sums as the slices add them: any split of the documents gives the same words
    for (uint32_t r = 0; r < R; r++) {
      uint64_t sum = 0;
      const uint64_t cut = rng() % (n_docs + 1);
      sum += fuse_range_start(rsplit.data(), cut, R, r);
      sum += fuse_range_start(rsplit.data() + cut * R, n_docs - cut, R, r);
      CHECK(sum == fuse_range_start(rsplit.data(), n_docs, R, r));
    }
  }
  // the control words are a whole number of 64-word lines and hold 2 R + 1 words
  for (uint32_t R = 1; R <= 64; R++) {
    CHECK(fuse_ctl_words(R) % 64 == 0 && fuse_ctl_words(R) >= 2 * R + 1);
    CHECK(fuse_scratch_words(R, 1000) == fuse_ctl_words(R) + 1000);
  }
  return 0;
}

int main() {
  std::mt19937_64 rng(20261021);
  if (check_fuse_plan() || check_tickets(rng) || check_scratch_rule(rng) || check_finisher_model(rng)) return 1;
  printf("ok %d checks\n", checks);
  return 0;
}
