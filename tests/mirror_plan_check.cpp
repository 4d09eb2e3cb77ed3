// How a commit brings a snapshot's host mirrors up to date (csrc/commit_plan.h):
// the none / delta / whole decision with every precondition broken one at a
// time and the sizes at their thresholds, and the two delta lists applied to a
// mirror against a naive rebuild.  Stand-alone; built with
// -fsanitize=address,undefined by test_mirror_plan_cpu.py.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
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

static uint64_t rnd(uint64_t *st) {
  *st = *st * 6364136223846793005ull + 1442695040888963407ull;
  return *st >> 33;
}

static bool all_whole(const MirrorPlan &p) {
  return !p.delta && p.dict == kMirrorWhole && p.crank == kMirrorWhole && p.df == kMirrorWhole;
}

int main() {
  const uint32_t C = 1u << 18, NC = 1000, cap = kDfDeltaCap;
  const uint32_t frac = C / kDictDeltaDiv;                  // (above the floor kDictDeltaMin at this C)
  // the delta case: incremental, block-major, a valid last inversion, valid mirrors, no knob
  {
    MirrorPlan p = mirror_plan(false, false, 900, true, C, NC + 5, NC, 70, cap, nullptr);
    CHECK(p.delta && p.dict == kMirrorDelta && p.crank == kMirrorWhole && p.df == kMirrorDelta && p.n_new == 5);
    p = mirror_plan(false, false, 900, true, C, NC + 5, NC, 70, cap, "0");       // TFIDF_FULL_MIRROR=0 is off
    CHECK(p.delta && p.dict == kMirrorDelta);
    p = mirror_plan(false, false, 900, true, C, NC + 5, NC, 70, cap, "");
    CHECK(p.delta);
  }
  // every precondition broken, one at a time: everything is copied whole
  {
    CHECK(all_whole(mirror_plan(true, false, 900, true, C, NC + 5, NC, 70, cap, nullptr)));    // a full build
    CHECK(all_whole(mirror_plan(false, true, 900, true, C, NC + 5, NC, 70, cap, nullptr)));    // term-major
    CHECK(all_whole(mirror_plan(false, false, 0, true, C, NC + 5, NC, 70, cap, nullptr)));     // kept_inv == 0
    CHECK(all_whole(mirror_plan(false, false, 900, false, C, NC + 5, NC, 70, cap, nullptr)));  // mir_ok false
    CHECK(all_whole(mirror_plan(false, false, 900, true, C, NC + 5, NC, 70, cap, "1")));       // the knob
    CHECK(all_whole(mirror_plan(false, false, 900, true, C, NC + 5, NC, 70, cap, "yes")));
    CHECK(all_whole(mirror_plan(false, false, 900, true, C, NC - 1, NC, 70, cap, nullptr)));   // slots lost: never a delta
    // ... also with nothing new
    CHECK(all_whole(mirror_plan(true, false, 900, true, C, NC, NC, 0, cap, nullptr)));
    CHECK(all_whole(mirror_plan(false, false, 900, false, C, NC, NC, 0, cap, nullptr)));
  }
  // n_new at 0, at 1, at the fraction and one above it
  {
    MirrorPlan p = mirror_plan(false, false, 900, true, C, NC, NC, 70, cap, nullptr);
    CHECK(p.delta && p.n_new == 0 && p.dict == kMirrorNone && p.crank == kMirrorNone && p.df == kMirrorDelta);
    p = mirror_plan(false, false, 900, true, C, NC + 1, NC, 70, cap, nullptr);
    CHECK(p.n_new == 1 && p.dict == kMirrorDelta && p.crank == kMirrorWhole);
    p = mirror_plan(false, false, 900, true, C, NC + frac, NC, 70, cap, nullptr);
    CHECK(p.n_new == frac && p.dict == kMirrorDelta && p.crank == kMirrorWhole);
    p = mirror_plan(false, false, 900, true, C, NC + frac + 1, NC, 70, cap, nullptr);
    CHECK(p.delta && p.n_new == frac + 1 && p.dict == kMirrorWhole && p.crank == kMirrorWhole);
    for (uint32_t lg = 6; lg <= 21; lg++) {           // every dictionary size: the fraction or the floor, never past C
      const uint32_t c = 1u << lg, top = dict_delta_max(c);
      CHECK(top <= c && top >= std::min(c, kDictDeltaMin) && top >= c / kDictDeltaDiv);
      p = mirror_plan(false, false, 1, true, c, top, 0, 1, cap, nullptr);
      CHECK(p.dict == kMirrorDelta && p.n_new == top);
      if (top < c) {
        p = mirror_plan(false, false, 1, true, c, top + 1, 0, 1, cap, nullptr);
        CHECK(p.dict == kMirrorWhole);
      }
    }
    CHECK(dict_delta_max(1u << 10) == kDictDeltaMin && dict_delta_max(1u << 18) == frac && frac > kDictDeltaMin);
  }
  // df: nothing tokenized, postings up to the try bound, and beyond; a lowered cap
  {
    MirrorPlan p = mirror_plan(false, false, 900, true, C, NC, NC, 0, cap, nullptr);
    CHECK(p.delta && p.df == kMirrorNone && p.dict == kMirrorNone && p.crank == kMirrorNone);
    p = mirror_plan(false, false, 900, true, C, NC, NC, 1, cap, nullptr);
    CHECK(p.df == kMirrorDelta);
    p = mirror_plan(false, false, 900, true, C, NC, NC, (uint64_t)cap * kDfDeltaTry, cap, nullptr);
    CHECK(p.df == kMirrorDelta);
    p = mirror_plan(false, false, 900, true, C, NC, NC, (uint64_t)cap * kDfDeltaTry + 1, cap, nullptr);
    CHECK(p.delta && p.df == kMirrorWhole && p.dict == kMirrorNone);
    p = mirror_plan(false, false, 900, true, C, NC, NC, 1ull << 40, cap, nullptr);              // no 32-bit wrap
    CHECK(p.df == kMirrorWhole);
    p = mirror_plan(false, false, 900, true, C, NC, NC, 40, 10, nullptr);
    CHECK(p.df == kMirrorDelta);
    p = mirror_plan(false, false, 900, true, C, NC, NC, 41, 10, nullptr);
    CHECK(p.df == kMirrorWhole);
  }
  // the lists applied to a mirror against a naive rebuild
  uint64_t st = 20251021;
  for (int round = 0; round < 60; round++) {
    const uint32_t c = round < 3 ? 64u : (uint32_t)(64 + rnd(&st) % 4000);
    std::vector<uint64_t> dict((size_t)2 * c), want_dict;
    std::vector<uint32_t> df(c), want_df;
    for (uint32_t s = 0; s < c; s++) {
      const bool occ = rnd(&st) % 3 == 0;
      dict[s] = occ ? rnd(&st) | 1 : 0;
      dict[(size_t)c + s] = occ ? rnd(&st) : 0;
      df[s] = occ ? (uint32_t)(1 + rnd(&st) % 100) : 0;
    }
    want_dict = dict;
    want_df = df;
    // duplicate-free lists in any order: a shuffled slot set; rounds 0-2: empty, slot 0 and C - 1, every slot
    std::vector<uint32_t> slots(c);
    for (uint32_t s = 0; s < c; s++) slots[s] = s;
    for (uint32_t i = c - 1; i > 0; i--) std::swap(slots[i], slots[rnd(&st) % (i + 1)]);
    size_t n = round == 0 ? 0 : round == 2 ? c : rnd(&st) % c;
    if (round == 1) {
      slots[0] = c - 1;
      slots[1] = 0;
      n = 2;
    }
    std::vector<DictDelta> dl;
    std::vector<DfDelta> fl;
    for (size_t i = 0; i < n; i++) {
      const uint32_t s = slots[i];
      if (want_dict[s] == 0) {                        // a new slot: its key and its first df
        const DictDelta e{s, rnd(&st) | 1, rnd(&st)};
        dl.push_back(e);
        want_dict[s] = e.lo;
        want_dict[(size_t)c + s] = e.hi;
      }
      const DfDelta f{s, want_df[s] + 1 + (uint32_t)(rnd(&st) % 9)};
      fl.push_back(f);
      want_df[s] = f.df;
    }
    CHECK(apply_dict_delta(dict.data(), c, dl.data(), dl.size()));
    CHECK(apply_df_delta(df.data(), c, fl.data(), fl.size()));
    CHECK(dict == want_dict);
    CHECK(df == want_df);
    // empty lists through null pointers
    CHECK(apply_dict_delta(dict.data(), c, nullptr, 0) && dict == want_dict);
    CHECK(apply_df_delta(df.data(), c, nullptr, 0) && df == want_df);
    // a slot >= C anywhere in the list: an error, and nothing is written
    for (uint64_t bad : {(uint64_t)c, (uint64_t)c + 1, (uint64_t)0xFFFFFFFFull, (uint64_t)1 << 32}) {
      std::vector<DictDelta> dl2;
      std::vector<DfDelta> fl2;
      for (uint32_t i = 0; i < 5; i++) {
        dl2.push_back(DictDelta{slots[i], 11, 12});
        fl2.push_back(DfDelta{slots[i], 13});
      }
      const size_t at = rnd(&st) % 5;
      dl2[at].slot = bad;
      CHECK(!apply_dict_delta(dict.data(), c, dl2.data(), dl2.size()));
      CHECK(dict == want_dict);
      if (bad <= 0xFFFFFFFFull) {
        fl2[at].slot = (uint32_t)bad;
        CHECK(!apply_df_delta(df.data(), c, fl2.data(), fl2.size()));
        CHECK(df == want_df);
      }
    }
  }
  printf("ok %d checks\n", checks);
  return 0;
}
