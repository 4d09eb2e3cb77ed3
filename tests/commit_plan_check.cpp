// The host side of an incremental tfidf_commit (csrc/commit_plan.h): the full /
// incremental decision for every signature field changed one at a time, and
// the list merges against a naive sort.  Stand-alone; built with
// -fsanitize=address,undefined by test_commit_plan_cpu.py.
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

static CommitSig base_sig() {
  CommitSig s;
  s.epoch = 7;
  s.hash_seed = 0;
  s.n_dead = 0;
  s.cap_log2 = 18;
  s.C = 1u << 18;
  s.range_shift = 16;
  s.R = 4;
  s.term_major = false;
  return s;
}

static uint64_t rnd(uint64_t *st) {
  *st = *st * 6364136223846793005ull + 1442695040888963407ull;
  return *st >> 33;
}

int main() {
  const CommitSig b = base_sig();
  // the incremental case: same signature, tok_docs <= n_staged
  {
    CommitPlan p = commit_plan(b, 600, b, 900, nullptr);
    CHECK(!p.full && p.d_first == 600);
    p = commit_plan(b, 900, b, 900, nullptr);          // nothing new: still incremental, from the end
    CHECK(!p.full && p.d_first == 900);
    p = commit_plan(b, 1, b, 1, "0");                  // TFIDF_FULL_COMMIT=0 is off
    CHECK(!p.full && p.d_first == 1);
    p = commit_plan(b, 1, b, 1, "");
    CHECK(!p.full);
  }
  // every fallback, one field at a time
  {
    CHECK(commit_plan(b, 0, b, 900, nullptr).full);                 // a new snapshot / one a failed commit left
    CHECK(commit_plan(b, 901, b, 900, nullptr).full);               // tok_docs > n_staged
    CHECK(commit_plan(b, 600, b, 900, "1").full);                   // forced
    CHECK(commit_plan(b, 600, b, 900, "yes").full);
    CHECK(commit_plan(b, 600, b, 900, "1").d_first == 0);
    CommitSig n = b;
    n.epoch = 8;
    CHECK(commit_plan(b, 600, n, 900, nullptr).full);
    n = b; n.hash_seed = 1;
    CHECK(commit_plan(b, 600, n, 900, nullptr).full);
    CHECK(commit_plan(n, 600, b, 900, nullptr).full);               // built under seed 1 after a collision, restarts at 0
    CHECK(!commit_plan(n, 600, n, 900, nullptr).full);              // a floor of 1 on both sides
    n = b; n.n_dead = 1;
    CHECK(commit_plan(b, 600, n, 900, nullptr).full);
    CHECK(commit_plan(n, 600, n, 900, nullptr).full);               // dead documents on both sides: still full
    CHECK(commit_plan(n, 600, b, 900, nullptr).full);
    n = b; n.cap_log2 = 19;
    CHECK(commit_plan(b, 600, n, 900, nullptr).full);
    n = b; n.C = 1u << 19;
    CHECK(commit_plan(b, 600, n, 900, nullptr).full);
    n = b; n.range_shift = 15;
    CHECK(commit_plan(b, 600, n, 900, nullptr).full);
    n = b; n.R = 8;
    CHECK(commit_plan(b, 600, n, 900, nullptr).full);
    n = b; n.term_major = true;
    CHECK(commit_plan(b, 600, n, 900, nullptr).full);
    for (int k = 0; k < kCommitKnobs; k++) {
      n = b;
      n.knobs[k] = knob_sig("1");
      CHECK(commit_plan(b, 600, n, 900, nullptr).full);             // set now, unset then
      CHECK(commit_plan(n, 600, b, 900, nullptr).full);             // and the reverse
      CommitSig m = b;
      m.knobs[k] = knob_sig("2");
      CHECK(commit_plan(m, 600, n, 900, nullptr).full);             // another value
      if (k != kKnobFullCommit) CHECK(!commit_plan(n, 600, n, 900, nullptr).full);
    }
  }
  // the knob word: unset, empty and "0" are three different values; names are all there
  {
    CHECK(knob_sig(nullptr) == 0);
    CHECK(knob_sig("") != 0 && knob_sig("0") != 0 && knob_sig("") != knob_sig("0") && knob_sig("0") != knob_sig("1"));
    CHECK(knob_sig("4") == knob_sig("4"));
    for (int k = 0; k < kCommitKnobs; k++) CHECK(commit_knob_names()[k] && commit_knob_names()[k][0] == 'T');
  }
  // malformed ids: kept ascending + new in any order == the naive sort
  {
    uint64_t st = 12345;
    for (int round = 0; round < 200; round++) {
      const uint64_t nk = round % 5 == 0 ? 0 : rnd(&st) % 40, nf = round % 7 == 0 ? 0 : rnd(&st) % 40;
      std::vector<uint32_t> kept(nk), fresh(nf);
      for (auto &x : kept) x = (uint32_t)(rnd(&st) % 1000);
      std::sort(kept.begin(), kept.end());
      // new ids usually lie above the kept ones; the merge must not rely on it
      for (auto &x : fresh) x = (uint32_t)((round & 1 ? 1000 : 0) + rnd(&st) % 1000);
      std::vector<uint32_t> want = kept;
      want.insert(want.end(), fresh.begin(), fresh.end());
      std::sort(want.begin(), want.end());
      merge_malformed(&kept, fresh.data(), fresh.size());
      CHECK(kept == want);
    }
    std::vector<uint32_t> e;
    merge_malformed(&e, nullptr, 0);
    CHECK(e.empty());
  }
  // escape append bounds and the merge
  {
    EscAppend a = esc_append_bounds(0, 0, 64);
    CHECK(!a.overflow && a.first == 0 && a.count == 0);
    a = esc_append_bounds(3, 3, 64);
    CHECK(!a.overflow && a.first == 3 && a.count == 0);
    a = esc_append_bounds(3, 10, 64);
    CHECK(!a.overflow && a.first == 3 && a.count == 7);
    a = esc_append_bounds(3, 64, 64);
    CHECK(!a.overflow && a.count == 61);
    a = esc_append_bounds(3, 65, 64);
    CHECK(a.overflow && a.count == 0);
    a = esc_append_bounds(5, 4, 64);                  // a counter below the kept count: never read as a huge count
    CHECK(a.overflow && a.count == 0);
    uint64_t st = 99;
    for (int round = 0; round < 200; round++) {
      const uint64_t nk = round % 5 == 0 ? 0 : rnd(&st) % 30, nf = round % 3 == 0 ? 0 : rnd(&st) % 30;
      std::vector<uint64_t> list(nk);
      for (auto &x : list) x = (rnd(&st) % 5000) << 24 | (rnd(&st) & 0xFFFFFF);
      std::sort(list.begin(), list.end());
      for (uint64_t i = 0; i < nf; i++) list.push_back(((round & 1 ? 5000 : 0) + rnd(&st) % 5000) << 24 | (rnd(&st) & 0xFFFFFF));
      std::vector<uint64_t> want = list;
      std::sort(want.begin(), want.end());
      esc_merge(&list, nk);
      CHECK(list == want);
    }
    std::vector<uint64_t> e;
    esc_merge(&e, 0);
    CHECK(e.empty());
  }
  printf("ok %d\n", checks);
  return 0;
}
