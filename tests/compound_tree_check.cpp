// compound_tree_check.cpp — stand-alone host checker of csrc/compound_tree_plan.h
// (tests/test_compound_tree_cpu.py builds it with the host compiler under
// AddressSanitizer and UBSan).  It reads one binary case file and prints, for
// test_compound_tree_cpu.py to compare with compound_tree_ref.py:
//
//   queries   every query's hits, computed the way k_cqn_combine computes them
//             with the header's functions: the nodes' rows (a group's is empty)
//             flattened and binned by cq_bin through cq_clause_of; per (query,
//             block) the node table, cqn_count_children and cqn_feasible; per
//             tile of cqn_tile_docs(levels) documents the pre-order walk of
//             cqn_next over a stack of levels, cqn_apply for a leaf's entries,
//             cqn_match and cq_score for a closing group, cq_hit_key for the
//             root's survivors, ordered by descending key.  Each query runs with
//             its own depth's tile and once more with the deepest tile; the two
//             must agree (exit 4).  Beside the hits: cqn_hit_bound, and the
//             number of blocks that cqn_feasible ruled out although they hold a
//             hit (evaluated without the rule)
//   checks    cqn_check_args on each argument case
//
// File (little endian): u32 n_blocks, u32 n_docs, u32 n_q; per query u32 n_nodes,
// per node u8 occur, u8 group, u32 parent, u32 min_should_match, u32 n, n x (u32
// doc, u32 score bits); u32 n_cases, per case u32 n_q, (n_q + 1) u64 query
// offsets, u32 n_nodes, (n_nodes + 1) u64 payload offsets, n_nodes x (u8 occur,
// u8 kind, u32 parent).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "compound_tree_plan.h"

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

struct Case {
  uint32_t n_blocks, n_docs;
  std::vector<uint64_t> q_noff{0}, c_off{0}, start, end;
  std::vector<CqnNode> nodes;
  std::vector<tfidf_qnode> qnodes;
  std::vector<Entry> binned;
};

// one query as one workgroup per block would combine it; *ruled_out_hits: blocks cqn_feasible rules out that hold a hit
static std::vector<uint64_t> combine(const Case &c, uint32_t q, uint32_t levels, uint32_t *ruled_out_hits) {
  const uint32_t c0 = (uint32_t)c.q_noff[q], nc = (uint32_t)(c.q_noff[q + 1] - c.q_noff[q]);
  const uint32_t tile = cqn_tile_docs(levels);
  const CqnNode *nd = c.nodes.data() + c0;
  std::vector<double> must((size_t)levels * tile), shd((size_t)levels * tile);
  std::vector<uint8_t> req((size_t)levels * tile), nsh((size_t)levels * tile), flags((size_t)levels * tile);
  std::vector<CqNeeds> needs(nc ? nc : 1);
  std::vector<uint8_t> live(nc ? nc : 1), bad(nc ? nc : 1), can(nc ? nc : 1);
  cqn_count_children(nd, nc, needs.data());
  std::vector<uint64_t> keys;
  *ruled_out_hits = 0;
  for (uint32_t b = 0; b < c.n_blocks; b++) {
    for (uint32_t i = 0; i < nc; i++) {
      const uint64_t bin = cq_bin(c0 + i, b * kCqBlockDocs, c.n_blocks);
      live[i] = c.end[bin] > c.start[bin];
    }
    const bool go = cqn_feasible(nd, needs.data(), nc, live.data(), bad.data(), can.data());
    const size_t before = keys.size();
    for (uint32_t t = 0; t < kCqBlockDocs / tile; t++) {
      const uint32_t d0 = b * kCqBlockDocs + t * tile;
      if (d0 >= c.n_docs) break;
      CqnWalk w;
      for (;;) {
        uint32_t node = 0, level = 0;
        const int ev = cqn_next(&w, nd, nc, &node, &level);
        if (ev == kCqnEnd || level >= levels || node >= nc) break;
        const uint32_t base = level * tile;
        if (ev == kCqnOpen) {
          for (uint32_t i = 0; i < tile; i++) {
            must[base + i] = shd[base + i] = 0.0;
            req[base + i] = nsh[base + i] = flags[base + i] = 0;
          }
        } else if (ev == kCqnLeaf) {
          const uint64_t bin = cq_bin(c0 + node, b * kCqBlockDocs, c.n_blocks);
          for (uint64_t i = c.start[bin]; i < c.end[bin]; i++) {
            const uint32_t ld = c.binned[i].doc - d0;
            if (ld >= tile) continue;
            float s;
            memcpy(&s, &c.binned[i].bits, 4);
            cqn_apply(nd[node].occur, s, &req[base + ld], &nsh[base + ld], &flags[base + ld], &must[base + ld],
                      &shd[base + ld]);
          }
        } else {
          for (uint32_t ld = 0; ld < tile; ld++) {
            const uint32_t at = base + ld;
            if (!cqn_match(needs[node], nd[node].min_should, req[at], nsh[at], flags[at])) continue;
            const float score = cq_score(needs[node], flags[at], must[at], shd[at]);
            if (level == 0) {
              if (d0 + ld < c.n_docs) keys.push_back(cq_hit_key(score, d0 + ld));
            } else {
              const uint32_t up = base - tile + ld;
              cqn_apply(nd[node].occur, score, &req[up], &nsh[up], &flags[up], &must[up], &shd[up]);
            }
          }
        }
      }
    }
    if (!go && keys.size() > before) ++*ruled_out_hits;
  }
  std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
  return keys;
}

int main(int argc, char **argv) {
  if (argc != 2 || !(g_f = fopen(argv[1], "rb"))) {
    fprintf(stderr, "usage: compound_tree_check case.bin\n");
    return 2;
  }
  Case c;
  c.n_blocks = rd<uint32_t>();
  c.n_docs = rd<uint32_t>();
  const uint32_t n_q = rd<uint32_t>();
  std::vector<Entry> rows;
  std::vector<uint64_t> row_n;
  for (uint32_t q = 0; q < n_q; q++) {
    const uint32_t nn = rd<uint32_t>();
    for (uint32_t i = 0; i < nn; i++) {
      CqnNode nd{};
      tfidf_qnode qn{};
      nd.occur = qn.occur = rd<uint8_t>();
      nd.group = rd<uint8_t>();
      qn.kind = nd.group ? TFIDF_CLAUSE_GROUP : TFIDF_CLAUSE_TEXT;
      nd.parent = qn.parent = rd<uint32_t>();
      nd.min_should = qn.min_should_match = rd<uint32_t>();
      const uint32_t n = rd<uint32_t>();
      for (uint32_t k = 0; k < n; k++) {
        Entry x;
        x.doc = rd<uint32_t>();
        x.bits = rd<uint32_t>();
        rows.push_back(x);
      }
      c.nodes.push_back(nd);
      c.qnodes.push_back(qn);
      row_n.push_back(n);
      c.c_off.push_back(rows.size());
    }
    c.q_noff.push_back(c.nodes.size());
  }
  const uint32_t n_c = (uint32_t)c.nodes.size();
  const uint64_t n_e = rows.size(), n_bins = (uint64_t)n_c * c.n_blocks;

  // count, scan, scatter: as k_cq_bin and the scan between its two passes
  std::vector<uint64_t> cnt(n_bins + 1, 0);
  c.start.assign(n_bins + 1, 0);
  for (uint64_t e = 0; e < n_e; e++) {
    if (rows[e].doc >= c.n_docs) continue;
    const uint64_t bin = cq_bin(cq_clause_of(c.c_off.data(), n_c, e), rows[e].doc, c.n_blocks);
    if (bin >= n_bins) return 3;
    cnt[bin]++;
  }
  for (uint64_t b = 0; b < n_bins; b++) c.start[b + 1] = c.start[b] + cnt[b];
  c.end = c.start;
  c.binned.resize(n_e ? n_e : 1);
  for (uint64_t e = 0; e < n_e; e++) {
    if (rows[e].doc >= c.n_docs) continue;
    const uint64_t bin = cq_bin(cq_clause_of(c.c_off.data(), n_c, e), rows[e].doc, c.n_blocks);
    const uint64_t at = c.end[bin]++;
    if (at >= n_e) return 3;
    c.binned[at] = rows[e];
  }

  for (uint32_t q = 0; q < n_q; q++) {
    const uint64_t n0 = c.q_noff[q];
    const uint32_t nn = (uint32_t)(c.q_noff[q + 1] - n0);
    const uint32_t levels = std::max(1u, cqn_levels(c.qnodes.data() + n0, nn));
    if (levels > kCqnMaxDepth) return 3;
    uint32_t ruled_out = 0, ruled_out_deep = 0;
    const std::vector<uint64_t> keys = combine(c, q, levels, &ruled_out);
    if (keys != combine(c, q, kCqnMaxDepth, &ruled_out_deep)) return 4;   // the result does not depend on the tile
    const uint64_t bound = cqn_hit_bound(c.qnodes.data() + n0, row_n.data() + n0, nn, c.n_docs);
    printf("q %u %zu %llu %u %u\n", q, keys.size(), (unsigned long long)bound, ruled_out, levels);
    for (uint64_t k : keys) printf("%u %u\n", (uint32_t)~(uint32_t)k, (uint32_t)(k >> 32));
  }

  const uint32_t n_cases = rd<uint32_t>();
  for (uint32_t i = 0; i < n_cases; i++) {
    const uint32_t nq = rd<uint32_t>();
    std::vector<uint64_t> qo((size_t)nq + 1);
    for (uint64_t &v : qo) v = rd<uint64_t>();
    const uint32_t nn = rd<uint32_t>();
    std::vector<uint64_t> co((size_t)nn + 1);
    for (uint64_t &v : co) v = rd<uint64_t>();
    std::vector<tfidf_qnode> nd(nn ? nn : 1);
    for (uint32_t k = 0; k < nn; k++) {
      memset(&nd[k], 0, sizeof nd[k]);
      nd[k].occur = rd<uint8_t>();
      nd[k].kind = rd<uint8_t>();
      nd[k].parent = rd<uint32_t>();
    }
    uint64_t at_q = 0, at_n = 0;
    const int rc = cqn_check_args(co.data(), nd.data(), qo.data(), nq, &at_q, &at_n);
    printf("check %d %llu %llu\n", rc, (unsigned long long)at_q, (unsigned long long)at_n);
  }
  printf("sizeof %zu\nok\n", sizeof(tfidf_qnode));
  fclose(g_f);
  return 0;
}
