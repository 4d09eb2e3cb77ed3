// compact_plan.h — the host side of tfidf_compact: what the copy kernel moves
// and how the staged ids and the keyless documents' ordinals change.  Plain
// C++ (no HIP), so the planner is tested on its own (tests/compact_plan_check.cpp).
#pragma once

#include <stdint.h>

#include <vector>

namespace tfidf {

constexpr uint64_t kCompactDead = ~0ull;   // old_to_new of a dead document

// A maximal stretch of consecutive live documents with at least one byte:
// text[src .. src + len) moves to [dst .. dst + len).  The runs tile the new
// text exactly: runs[0].dst == 0, runs[i + 1].dst == runs[i].dst + runs[i].len.
struct CompactRun {
  uint64_t src, dst, len;
};

struct CompactPlan {
  std::vector<uint64_t> new_offsets;   // [n_live + 1]
  std::vector<uint64_t> old_to_new;    // [n_staged]: new staged id, kCompactDead for a dead document
  std::vector<CompactRun> runs;        // ascending in dst (and in src); at most n_dead + 1
  uint64_t n_live = 0, live_bytes = 0, dead_bytes = 0;
};

// live[n], offsets[n + 1] (non-decreasing, offsets[0] == 0).
inline void compact_plan(const uint8_t *live, const uint64_t *offsets, uint64_t n, CompactPlan *out) {
  CompactPlan &p = *out;
  p.new_offsets.assign(1, 0);
  p.old_to_new.assign(n, kCompactDead);
  p.runs.clear();
  p.n_live = p.live_bytes = p.dead_bytes = 0;
  bool open = false;                   // the last run ends where document i starts
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t a = offsets[i], len = offsets[i + 1] - a;
    if (!live[i]) {
      p.dead_bytes += len;
      open = false;
      continue;
    }
    p.old_to_new[i] = p.n_live++;
    if (len) {
      if (open) p.runs.back().len += len;
      else p.runs.push_back(CompactRun{a, p.live_bytes, len});
      open = true;
    }
    p.live_bytes += len;
    p.new_offsets.push_back(p.live_bytes);
  }
}

// Keyless documents are named by the ordinal they received when they were
// added (the count of documents staged before them), which compaction must
// keep: the survivors' ordinals in their new order.  ord == nullptr: the
// ordinals are the positions (an index never compacted).
inline std::vector<uint64_t> compact_ordinals(const uint8_t *live, uint64_t n, const uint64_t *ord) {
  std::vector<uint64_t> o;
  for (uint64_t i = 0; i < n; i++)
    if (live[i]) o.push_back(ord ? ord[i] : i);
  return o;
}

// ordinals o[i] == o[0] + i: a base is enough to store them
inline bool ordinals_contiguous(const std::vector<uint64_t> &o) {
  for (uint64_t i = 1; i < o.size(); i++)
    if (o[i] != o[0] + i) return false;
  return true;
}

}  // namespace tfidf
