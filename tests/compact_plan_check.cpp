// compact_plan_check.cpp — stand-alone check of csrc/compact_plan.h against a
// naive per-document loop (built with -fsanitize=address,undefined and run as a
// child process by test_compact_plan_cpu.py).  Prints "ok <cases>" and exits 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "compact_plan.h"

using namespace tfidf;

static int g_cases = 0;

#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, g_name); \
      exit(1);                                                            \
    }                                                                     \
  } while (0)
static const char *g_name = "";

// Every live byte's destination, document by document, against the plan's
// runs: walks the runs beside the documents without touching any text.
static void check(const char *name, const std::vector<uint8_t> &live, const std::vector<uint64_t> &len,
                  uint64_t first_off = 0) {
  g_name = name;
  g_cases++;
  const uint64_t n = live.size();
  std::vector<uint64_t> off(n + 1, 0);
  // first_off shifts every document but the first boundary (offsets[0] == 0):
  // a large first document puts the rest above 2^32
  for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + len[i] + (i == 0 ? first_off : 0);
  CompactPlan p;
  compact_plan(live.data(), off.data(), n, &p);
  uint64_t n_live = 0, dst = 0, dead = 0, n_dead = 0;
  size_t r = 0;        // current run
  uint64_t in_run = 0; // bytes of runs[r] consumed
  bool prev_live = false;
  CHECK(p.new_offsets.size() >= 1 && p.new_offsets[0] == 0);
  CHECK(p.old_to_new.size() == n);
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t L = off[i + 1] - off[i];
    if (!live[i]) {
      CHECK(p.old_to_new[i] == kCompactDead);
      dead += L;
      n_dead++;
      // a dead document ends the stretch: the run in progress must be used up
      if (r < p.runs.size() && in_run) { CHECK(in_run == p.runs[r].len); r++; in_run = 0; }
      prev_live = false;
      continue;
    }
    CHECK(p.old_to_new[i] == n_live);
    CHECK(n_live + 1 < p.new_offsets.size());
    CHECK(p.new_offsets[n_live] == dst && p.new_offsets[n_live + 1] == dst + L);
    if (L) {
      CHECK(r < p.runs.size());
      const CompactRun &run = p.runs[r];
      CHECK(run.len > 0);
      // the document's bytes sit at the run's cursor, in source and destination
      CHECK(run.src + in_run == off[i]);
      CHECK(run.dst + in_run == dst);
      CHECK(in_run + L <= run.len);
      if (in_run) CHECK(prev_live);
      in_run += L;
    }
    prev_live = true;
    dst += L;
    n_live++;
  }
  if (r < p.runs.size() && in_run) { CHECK(in_run == p.runs[r].len); r++; }
  CHECK(r == p.runs.size());                      // no run left over, so none is empty or unreferenced
  CHECK(p.runs.size() <= n_dead + 1);
  for (size_t k = 0; k < p.runs.size(); k++) {
    CHECK(p.runs[k].len > 0);
    if (k == 0) CHECK(p.runs[k].dst == 0);
    else CHECK(p.runs[k].dst == p.runs[k - 1].dst + p.runs[k - 1].len && p.runs[k].src > p.runs[k - 1].src);
  }
  CHECK(p.n_live == n_live && p.live_bytes == dst && p.dead_bytes == dead);
  CHECK(p.new_offsets.size() == n_live + 1);
  CHECK(dst + dead == off[n]);
}

// Keyless documents across two compactions: keys are ordinals, never reused.
static void check_ordinals() {
  g_name = "ordinals";
  g_cases++;
  uint64_t next = 0;
  std::vector<uint64_t> ord;                 // ordinal of each staged document
  std::vector<uint8_t> live;
  auto add = [&](int k) { for (int i = 0; i < k; i++) { ord.push_back(next++); live.push_back(1); } };
  add(8);
  CHECK(ordinals_contiguous(ord));
  // never compacted: the ordinals are the positions (nullptr form)
  {
    std::vector<uint8_t> lv = {1, 0, 1, 1, 0, 0, 1, 0};
    std::vector<uint64_t> a = compact_ordinals(lv.data(), 8, nullptr), b = compact_ordinals(lv.data(), 8, ord.data());
    CHECK(a == b && a == (std::vector<uint64_t>{0, 2, 3, 6}));
    CHECK(!ordinals_contiguous(a));
    live = lv;
  }
  ord = compact_ordinals(live.data(), live.size(), ord.data());
  live.assign(ord.size(), 1);
  add(3);                                    // 8, 9, 10: the reclaimed 7 is not reused
  CHECK(ord == (std::vector<uint64_t>{0, 2, 3, 6, 8, 9, 10}));
  live[0] = 0;
  live[4] = 0;
  live[6] = 0;
  ord = compact_ordinals(live.data(), live.size(), ord.data());
  live.assign(ord.size(), 1);
  CHECK(ord == (std::vector<uint64_t>{2, 3, 6, 9}));
  add(1);
  CHECK(ord.back() == 11 && next == 12);
  // a stretch that stays consecutive needs only a base
  std::vector<uint8_t> lv2 = {1, 1, 0, 0, 0};
  CHECK(ordinals_contiguous(compact_ordinals(lv2.data(), 5, ord.data())));
  std::vector<uint8_t> none = {0, 0, 0, 0, 0};
  CHECK(compact_ordinals(none.data(), 5, ord.data()).empty());
  CHECK(ordinals_contiguous(std::vector<uint64_t>{}));
}

int main() {
  const std::vector<uint64_t> L8 = {5, 0, 17, 3, 0, 0, 40, 1};
  check("nothing dead", {1, 1, 1, 1, 1, 1, 1, 1}, L8);
  check("everything dead", {0, 0, 0, 0, 0, 0, 0, 0}, L8);
  check("first dead", {0, 1, 1, 1, 1, 1, 1, 1}, L8);
  check("last dead", {1, 1, 1, 1, 1, 1, 1, 0}, L8);
  check("first and last dead", {0, 1, 1, 1, 1, 1, 1, 0}, L8);
  check("alternating a", {1, 0, 1, 0, 1, 0, 1, 0}, L8);
  check("alternating b", {0, 1, 0, 1, 0, 1, 0, 1}, L8);
  // empty live documents beside dead ones: no zero-length run
  check("empty live beside dead", {0, 1, 0, 1, 1, 1, 0, 1}, {4, 0, 4, 0, 0, 0, 9, 0});
  check("only empty live", {0, 1, 0, 1, 0}, {4, 0, 4, 0, 2});
  check("empty dead inside live", {1, 0, 1, 1, 0, 1}, {3, 0, 2, 0, 0, 7});
  check("all empty", {1, 0, 1}, {0, 0, 0});
  check("no documents", {}, {});
  // offsets above 2^32 (the plan needs no text)
  check("above 4 GiB", {1, 0, 1, 1, 0, 1, 1, 0}, L8, (1ull << 32) + 12345);
  check("first dead above 4 GiB", {0, 1, 0, 1, 1, 0, 1, 1}, L8, 3 * (1ull << 32) + 7);
  {
    std::vector<uint8_t> lv;
    std::vector<uint64_t> ln;
    uint64_t x = 88172645463325252ull;       // xorshift: a long random case
    for (int i = 0; i < 5000; i++) {
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      lv.push_back((x >> 20) % 3 != 0);
      ln.push_back((x >> 8) % 7 == 0 ? 0 : (x >> 32) % 3000000);
    }
    check("random", lv, ln);                  // ~ 6 GB of offsets
  }
  check_ordinals();
  printf("ok %d\n", g_cases);
  return 0;
}
