// The host side of an incremental inversion (csrc/commit_plan.h): which blocks
// a commit keeps (inversion_plan, every condition flipped one at a time), the
// kept count rows in a wider column layout (remap_old_col / remap_row_value,
// the formula k_blk_remap runs) against a naive rebuild, and the posting
// escapes of the kept blocks (post_esc_keep) against a linear filter.
// Stand-alone; built with -fsanitize=address,undefined by test_inv_plan_cpu.py.
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

// crank of an occupancy bitmap: per 32 slots {bits, occupied slots before}, + the sentinel word
struct Crank {
  std::vector<uint32_t> bits, base;
  uint32_t NC = 0;
};
static Crank crank_of(const std::vector<uint8_t> &occ) {
  Crank c;
  const size_t W = occ.size() / 32;
  c.bits.assign(W + 1, 0);
  c.base.assign(W + 1, 0);
  uint32_t run = 0;
  for (size_t w = 0; w < W; w++) {
    c.base[w] = run;
    for (int b = 0; b < 32; b++)
      if (occ[32 * w + b]) { c.bits[w] |= 1u << b; run++; }
  }
  c.base[W] = run;
  c.NC = run;
  return c;
}

// One kept block: per-slot posting counts (nonzero only in old slots) -> the
// offset row of the layout `occ`, and the block total.
static std::vector<uint32_t> offsets_row(const std::vector<uint8_t> &occ, const std::vector<uint32_t> &count,
                                         uint32_t *total) {
  std::vector<uint32_t> row;
  uint32_t run = 0;
  for (size_t s = 0; s < occ.size(); s++)
    if (occ[s]) { row.push_back(run); run += count[s]; }
  *total = run;
  return row;
}

// the kernel's walk: every occupied new slot, in slot order, through the shared formula
static std::vector<uint32_t> remap_row(const Crank &nw, const Crank &old, const std::vector<uint32_t> &old_row,
                                       uint32_t total) {
  std::vector<uint32_t> row(nw.NC, 0xDEADBEEFu);
  for (size_t w = 0; w + 1 < nw.bits.size(); w++) {
    uint32_t bits = nw.bits[w], col = nw.base[w];
    while (bits) {
      const uint32_t bit = (uint32_t)__builtin_ctz(bits);
      bits &= bits - 1;
      row[col++] = remap_row_value(old_row.data(), old.NC, total, remap_old_col(old.bits[w], old.base[w], bit));
    }
  }
  return row;
}

static int remap_case(const std::vector<uint8_t> &old_occ, const std::vector<uint8_t> &new_occ,
                      const std::vector<uint32_t> &count) {
  const Crank oc = crank_of(old_occ), nc = crank_of(new_occ);
  uint32_t total = 0, total2 = 0;
  const std::vector<uint32_t> old_row = offsets_row(old_occ, count, &total);
  const std::vector<uint32_t> want = offsets_row(new_occ, count, &total2);    // the naive rebuild
  CHECK(total == total2 && old_row.size() == oc.NC && want.size() == nc.NC);
  const std::vector<uint32_t> got = remap_row(nc, oc, old_row, total);
  CHECK(got == want);
  // the segments the scorers read: [row[c], row[c + 1]) (the last: up to the total) hold each slot's count
  uint32_t c = 0;
  for (size_t s = 0; s < new_occ.size(); s++)
    if (new_occ[s]) {
      const uint32_t hi = c + 1 < nc.NC ? got[c + 1] : total;
      CHECK(hi - got[c] == count[s]);
      c++;
    }
  return 0;
}

int main() {
  // ---- inversion_plan: the kept case, then each condition flipped alone
  {
    const uint64_t N = 3 * 8192 + 100;
    InversionPlan p = inversion_plan(false, false, 2 * 8192 + 5, N, 500, 500, nullptr);
    CHECK(p.first_block == 2 && !p.remap);
    CHECK(inversion_plan(true, false, 2 * 8192 + 5, N, 500, 500, nullptr).first_block == 0);      // full commit plan
    CHECK(!inversion_plan(true, false, 2 * 8192 + 5, N, 500, 501, nullptr).remap);
    CHECK(inversion_plan(false, true, 2 * 8192 + 5, N, 500, 500, nullptr).first_block == 0);      // term-major
    CHECK(!inversion_plan(false, true, 2 * 8192 + 5, N, 500, 501, nullptr).remap);
    // inv_docs: floor to fully covered blocks
    CHECK(inversion_plan(false, false, 0, N, 500, 500, nullptr).first_block == 0);
    CHECK(!inversion_plan(false, false, 0, N, 501, 500, nullptr).remap);                          // nothing kept: no remap
    CHECK(inversion_plan(false, false, 8191, N, 500, 500, nullptr).first_block == 0);
    CHECK(!inversion_plan(false, false, 8191, N, 501, 500, nullptr).remap);
    CHECK(inversion_plan(false, false, 8192, N, 500, 500, nullptr).first_block == 1);
    CHECK(inversion_plan(false, false, 8193, N, 500, 500, nullptr).first_block == 1);
    CHECK(inversion_plan(false, false, N, N, 500, 500, nullptr).first_block == 3);                // nothing added: the tail block again
    CHECK(inversion_plan(false, false, N + 1, N, 500, 500, nullptr).first_block == 0);            // inv_docs > N
    CHECK(!inversion_plan(false, false, N + 1, N, 501, 500, nullptr).remap);
    CHECK(inversion_plan(false, false, 4 * 8192, 4 * 8192, 500, 500, nullptr).first_block == 4);  // N a multiple: every block kept
    CHECK(inversion_plan(false, false, 1ull << 40, 1ull << 41, 1, 1, nullptr).first_block == (1u << 27));
    // the A/B switch
    CHECK(inversion_plan(false, false, 2 * 8192, N, 500, 500, "1").first_block == 0);
    CHECK(!inversion_plan(false, false, 2 * 8192, N, 501, 500, "1").remap);
    CHECK(inversion_plan(false, false, 2 * 8192, N, 500, 500, "yes").first_block == 0);
    CHECK(inversion_plan(false, false, 2 * 8192, N, 500, 500, "0").first_block == 2);
    CHECK(inversion_plan(false, false, 2 * 8192, N, 500, 500, "").first_block == 2);
    // NC equal and larger
    p = inversion_plan(false, false, 2 * 8192, N, 501, 500, nullptr);
    CHECK(p.first_block == 2 && p.remap);
    p = inversion_plan(false, false, 2 * 8192, N, 500, 0, nullptr);                               // kept blocks of empty documents
    CHECK(p.first_block == 2 && p.remap);
    p = inversion_plan(false, false, 2 * 8192, N, 0, 0, nullptr);
    CHECK(p.first_block == 2 && !p.remap);
    CHECK(kPlanBlockDocs == 8192);
  }
  // ---- the remap formula against a naive rebuild
  {
    uint64_t st = 2024;
    for (int round = 0; round < 300; round++) {
      const size_t C = 32u << (round % 4);                       // 32 .. 256 slots
      std::vector<uint8_t> old_occ(C, 0), new_occ(C, 0);
      std::vector<uint32_t> count(C, 0);
      const uint32_t p_old = (uint32_t)(rnd(&st) % 90), p_new = (uint32_t)(rnd(&st) % 60);
      // round % 6: 0 = a window of old slots with new slots below, between and above; 1 = no old slot
      // (NC_inv = 0); 2 = a kept block with total 0; 3 = no new slot; else free
      const size_t lo = round % 6 == 0 ? C / 4 : 0, hi = round % 6 == 0 ? C - C / 4 : C;
      for (size_t s = 0; s < C; s++) {
        const bool in_old = round % 6 != 1 && s >= lo && s < hi && rnd(&st) % 100 < p_old;
        old_occ[s] = in_old;
        new_occ[s] = in_old || (round % 6 != 3 && rnd(&st) % 100 < p_new);
        // a block holds postings of some of the old slots only (others have count 0 there)
        if (in_old && round % 6 != 2 && rnd(&st) % 3) count[s] = 1 + (uint32_t)(rnd(&st) % 8192);
      }
      if (round % 6 == 0) {                                      // the three positions named above, for certain
        old_occ[lo] = new_occ[lo] = 1;
        old_occ[hi - 1] = new_occ[hi - 1] = 1;
        old_occ[lo + 1] = 0; new_occ[lo + 1] = 1;                // between (lo + 1 < hi - 1: C >= 32)
        new_occ[0] = 1;                                          // below the first old slot
        new_occ[C - 1] = 1;                                      // above the last
        count[lo] = 3; count[hi - 1] = 5; count[lo + 1] = 0; count[0] = 0; count[C - 1] = 0;
      }
      if (remap_case(old_occ, new_occ, count)) return 1;
    }
    // slot 31 / slot 32: the word edge (bit 31's mask, the next word's base)
    std::vector<uint8_t> o(64, 0), n(64, 0);
    std::vector<uint32_t> cnt(64, 0);
    o[31] = n[31] = 1; cnt[31] = 7;
    n[30] = n[32] = n[63] = 1;
    if (remap_case(o, n, cnt)) return 1;
    o[32] = 1; cnt[32] = 9;
    if (remap_case(o, n, cnt)) return 1;
  }
  // ---- the posting escapes of the kept blocks
  {
    uint64_t st = 77;
    for (int round = 0; round < 200; round++) {
      const uint64_t n = round % 5 == 0 ? 0 : rnd(&st) % 40;
      std::vector<uint64_t> list(n);
      for (auto &x : list) x = (rnd(&st) % 3000) << 24 | (2047 + rnd(&st) % 100000);
      std::sort(list.begin(), list.end());
      uint64_t base = rnd(&st) % 3200;
      if (n && round % 3 == 0) base = list[rnd(&st) % n] >> 24;          // an escape exactly at the base: not kept
      uint64_t want = 0;
      for (uint64_t x : list) want += (x >> 24) < base;
      const uint64_t got = post_esc_keep(list, base);
      CHECK(got == want);
      for (uint64_t i = 0; i < list.size(); i++) CHECK(((list[i] >> 24) < base) == (i < got));
    }
    std::vector<uint64_t> e;
    CHECK(post_esc_keep(e, 0) == 0 && post_esc_keep(e, 100) == 0);
    std::vector<uint64_t> one{(5ull << 24) | 4000};
    CHECK(post_esc_keep(one, 5) == 0 && post_esc_keep(one, 6) == 1 && post_esc_keep(one, 0) == 0);
    // ... and the new entries behind the kept ones merge as the CSR escapes do
    std::vector<uint64_t> list{(1ull << 24) | 2047, (9ull << 24) | 3000, (20ull << 24) | 2100};
    const uint64_t kept = post_esc_keep(list, 10);
    CHECK(kept == 2);
    list.resize(kept);
    list.push_back((30ull << 24) | 5000);
    list.push_back((12ull << 24) | 2500);
    const EscAppend a = esc_append_bounds(kept, 4, 64);
    CHECK(!a.overflow && a.first == 2 && a.count == 2);
    esc_merge(&list, a.first);
    CHECK(std::is_sorted(list.begin(), list.end()) && list.size() == 4 && (list[2] >> 24) == 12);
  }
  printf("ok %d\n", checks);
  return 0;
}
