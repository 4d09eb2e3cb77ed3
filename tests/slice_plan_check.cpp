// The launch shape of a few-block inversion (csrc/commit_plan.h slice_plan):
// document slices per (block, range) tile and workgroups per block row, over
// full grids, 1 / 2 / 8 blocks, R of 1 / 2 / 8, blocks of 1 .. 8192
// documents, NC of 0 .. 100 000 and both test knobs.  For every case the
// slices' document ranges (slice_range) must cover each block once, in order
// and on group boundaries, the grid must stay under its cap, and the row parts
// (scan_part_range) must cover the columns once on k_df_sum's workgroup
// boundaries.  Stand-alone; built with -fsanitize=address,undefined by
// test_slice_plan_cpu.py.
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

constexpr uint32_t kCus = 256;

// every property one plan must have; docs = the documents of the largest inverted block
static int check_plan(const SlicePlan &p, uint32_t blocks, uint32_t R, uint64_t docs, uint32_t NC, uint32_t cus,
                      int forced_slices, int forced_parts) {
  CHECK(p.slices >= 1 && p.scan_parts >= 1);
  CHECK(p.slice_docs >= 1 && p.slice_docs <= kPlanBlockDocs);
  if (p.slices > 1) CHECK(p.slice_docs % kSliceGroupDocs == 0);
  if (p.slices == 1) CHECK(p.slice_docs == kPlanBlockDocs);
  if (forced_slices > 0) CHECK(p.slices == (uint32_t)std::min(forced_slices, (int)kSliceKnobMax));
  if (forced_parts > 0) CHECK(p.scan_parts == (uint32_t)std::min(forced_parts, (int)kScanKnobMax));
  // the slices of the largest block and of a shorter tail block behind it (or the one block itself)
  const uint64_t sizes[3] = {docs, 1, docs > 1 ? docs - 1 : 1};
  for (uint64_t n : sizes) {
    if (n > docs) continue;
    const uint64_t d0 = 5 * kPlanBlockDocs, d1 = d0 + n;
    uint64_t at = d0;
    for (uint32_t i = 0; i < p.slices; i++) {
      uint64_t lo, hi;
      slice_range(p, i, d0, d1, &lo, &hi);
      CHECK(lo <= hi && hi <= d1);
      CHECK(lo == at);                                               // in order, no gap, no overlap
      if (lo < hi) CHECK((lo - d0) % kSliceGroupDocs == 0);
      if (lo < hi && hi < d1) CHECK((hi - lo) % kSliceGroupDocs == 0);
      if (forced_slices <= 0 && n == docs) CHECK(lo < hi);           // no empty slice unless forced
      if (forced_slices <= 0 && n == docs && p.slices > 1 && i + 1 < p.slices) CHECK(hi - lo >= kSliceMinDocs);
      at = hi;
    }
    CHECK(at == d1);                                                 // covered
  }
  // the tile grid: never above the device's capacity unless it was unsliced already or forced
  const uint64_t tiles = (uint64_t)blocks * R;
  if (forced_slices <= 0) {
    CHECK(tiles * p.slices <= std::max<uint64_t>(tiles, (uint64_t)cus * kSliceWgsPerCu));
    if (tiles >= cus) CHECK(p.slices == 1);                          // a full grid stays as it is
  } else {
    CHECK(tiles * p.slices <= tiles * kSliceKnobMax);
  }
  // the sort's streams per workgroup: 4 for a grid that fills the device, halved while it does not
  CHECK(p.sort_spw == 1 || p.sort_spw == 2 || p.sort_spw == 4);
  if (p.sort_spw < kSortSpw) CHECK(tiles * (kSortStreams / (2 * p.sort_spw)) < (uint64_t)cus * kSortWgsPerCu);
  if (p.sort_spw > 1) CHECK(tiles * (kSortStreams / p.sort_spw) >= (uint64_t)cus * kSortWgsPerCu);
  // row parts
  const uint32_t max_parts = std::max<uint32_t>(1, (NC + kScanPartCols - 1) / kScanPartCols);
  if (forced_parts <= 0) {
    CHECK(p.scan_parts <= max_parts);
    CHECK((uint64_t)blocks * p.scan_parts <= std::max<uint64_t>(blocks, cus));
    if (blocks * 2 > cus) CHECK(p.scan_parts == 1);                  // many rows
  }
  if (p.scan_parts > 1) {
    CHECK(p.scan_width >= kScanPartAlign && p.scan_width % kScanPartAlign == 0);
    CHECK((uint64_t)p.scan_width * p.scan_parts >= NC);
    if (forced_parts <= 0) CHECK((uint64_t)p.scan_width * (p.scan_parts - 1) < NC);   // no part without columns
  }
  uint64_t at = 0;
  for (uint32_t j = 0; j < p.scan_parts; j++) {
    uint64_t lo, hi;
    scan_part_range(p, j, NC, &lo, &hi);
    CHECK(lo == at && lo <= hi && hi <= NC);
    at = hi;
  }
  CHECK(at == NC);
  return 0;
}

int main() {
  // full grids: the cfg-2 full build (123 blocks x 8 ranges, 123 rows) and anything larger stay unsliced
  {
    const SlicePlan p = slice_plan(123, 8, 8192, 100000, kCus, nullptr, nullptr);
    CHECK(p.slices == 1 && p.scan_parts == 1 && p.slice_docs == kPlanBlockDocs && p.sort_spw == 4);
    const SlicePlan q = slice_plan(1000, 1, 8192, 100000, kCus, nullptr, nullptr);
    CHECK(q.slices == 1 && q.scan_parts == 1);
    const SlicePlan r = slice_plan(32, 8, 8192, 100000, kCus, nullptr, nullptr);    // 256 tiles on 256 CUs
    CHECK(r.slices == 1);
    if (check_plan(p, 123, 8, 8192, 100000, kCus, 0, 0) || check_plan(q, 1000, 1, 8192, 100000, kCus, 0, 0)) return 1;
  }
  // nothing to invert
  {
    const SlicePlan p = slice_plan(0, 8, 0, 100000, kCus, "7", "4");
    CHECK(p.slices == 1 && p.scan_parts == 1 && p.sort_spw == 4);
  }
  // pinned values: bench.py's step (a 576-document tail at R = 8, 100 k columns) and a full lone block
  {
    const SlicePlan p = slice_plan(1, 8, 576, 100000, kCus, nullptr, nullptr);
    CHECK(p.slices == 3 && p.slice_docs == 192 && p.scan_parts == 7 && p.scan_width == 14336 && p.sort_spw == 1);
    const SlicePlan q = slice_plan(1, 8, 8192, 100000, kCus, nullptr, nullptr);
    CHECK(q.slices == 35 && q.slice_docs == 240);                                  // 42 slices of 196 -> groups of 48
    const SlicePlan r = slice_plan(1, 1, 383, 1000, kCus, nullptr, nullptr);
    CHECK(r.slices == 1 && r.scan_parts == 1);
    const SlicePlan t = slice_plan(1, 1, 384, 16385, kCus, nullptr, nullptr);
    CHECK(t.slices == 2 && t.scan_parts == 2);
  }
  const uint32_t blocks_of[] = {1, 2, 8, 31, 123, 130};
  const uint32_t ranges[] = {1, 2, 8};
  const uint64_t docs_of[] = {1, 4, 47, 48, 49, 191, 192, 193, 383, 384, 576, 1000, 8191, 8192};
  const uint32_t ncs[] = {0, 1, 255, 256, 257, 16383, 16384, 16385, 33001, 100000};
  const uint32_t cus_of[] = {256, 304, 64, 1};
  const char *slice_knobs[] = {nullptr, "1", "2", "3", "7", "32", "400", "100000", "0", "-3", "", "x"};
  const char *part_knobs[] = {nullptr, "1", "2", "4", "64", "1000", "0", ""};
  for (uint32_t blocks : blocks_of)
    for (uint32_t R : ranges)
      for (uint64_t docs : docs_of) {
        if (blocks > 1 && docs != 8192) continue;                    // a block before the tail is full
        for (uint32_t NC : ncs)
          for (uint32_t cus : cus_of)
            for (const char *sk : slice_knobs)
              for (const char *pk : part_knobs) {
                const SlicePlan p = slice_plan(blocks, R, docs, NC, cus, sk, pk);
                const int fs = sk && *sk ? std::max(1, atoi(sk)) : 0, fp = pk && *pk ? std::max(1, atoi(pk)) : 0;
                if (check_plan(p, blocks, R, docs, NC, cus, fs, fp)) {
                  printf("  at blocks %u R %u docs %llu NC %u cus %u knobs %s %s -> slices %u x %u docs, parts %u x %u\n", blocks,
                         R, (unsigned long long)docs, NC, cus, sk ? sk : "-", pk ? pk : "-", p.slices, p.slice_docs,
                         p.scan_parts, p.scan_width);
                  return 1;
                }
                if (sk && sk[0] == '1' && !sk[1]) CHECK(p.slices == 1 && p.slice_docs == kPlanBlockDocs);   // today's path
                if (pk && pk[0] == '1' && !pk[1]) CHECK(p.scan_parts == 1);
              }
      }
  printf("ok %d checks\n", checks);
  return 0;
}
