// compound_tree_plan.h — nested compound queries (tfidf_search_nested*): the
// rules shared by the device pass (k_cqn_combine, kernels_compound.hip), the host
// around it (tfidf_capi.hip) and a stand-alone host checker
// (tests/compound_tree_check.cpp).
//
// A query is a tree of at most 64 nodes in pre-order (DESIGN.md section 2,
// "Nested compound queries").  A leaf is a clause of the flat call and has its
// row; a group (TFIDF_CLAUSE_GROUP) has children and a min_should_match m.  With
// R the group's MUST and FILTER children, N its MUST_NOT children and S its
// SHOULD children, a document matches the group when every R child holds it, no
// N child holds it and at least need = max(m, R empty ? 1 : 0) S children hold
// it.  Its score in the group is the flat rule over the children (cq_score), a
// group child scoring what this rule gave it.  Node 0 is the root group; groups
// sit at depths 0..3, leaves at depths 1..4.
#pragma once

#include "compound_plan.h"

namespace tfidf {

constexpr uint32_t kCqnMaxNodes = kCqMaxClausesPerQuery;   // nodes per query, groups and leaves
constexpr uint64_t kCqnMaxNodesPerCall = kCqMaxClauses;
constexpr uint32_t kCqnMaxDepth = 4;                       // open groups at once: depths 0 .. kCqnMaxDepth - 1
// one document's state on one level: cq_apply's two double sums, its R count and flags, and the SHOULD count
constexpr uint32_t kCqnStateBytes = 8 + 8 + 1 + 1 + 1;

// Documents whose state a workgroup holds at once when the deepest query of the
// chunk opens `levels` groups at once: levels * tile * kCqnStateBytes stays
// within the 2048-document single level of the flat pass (38 912 bytes).
TFIDF_HD uint32_t cqn_tile_docs(uint32_t levels) { return levels <= 1 ? 2048u : levels == 2 ? 1024u : 512u; }
constexpr uint32_t kCqnMinTileDocs = 512;
static_assert(kCqBlockDocs % 2048 == 0 && kCqnMaxDepth * kCqnMinTileDocs * kCqnStateBytes <= kCqTileDocs * kCqnStateBytes,
              "every tile size divides a block and every depth fits the single level's bytes");

// argument validation: 0, or the first rule broken (*at_q: the query, *at_n: the node within it)
enum {
  kCqnOk = 0,
  kCqnTooManyQueries,      // n_q > kCqMaxQueries
  kCqnBadQueryOffsets,     // q_node_offsets[0] != 0 or decreasing
  kCqnTooManyInQuery,      // a query of more than kCqnMaxNodes nodes
  kCqnTooManyNodes,        // more than kCqnMaxNodesPerCall nodes in the call
  kCqnBadPayloadOffsets,   // c_offsets[0] != 0 or decreasing
  kCqnBadOccur,
  kCqnBadKind,             // kind > TFIDF_CLAUSE_GROUP
  kCqnBadRoot,             // node 0 is not a group or its parent is not TFIDF_QNODE_ROOT
  kCqnBadParent,           // parent >= the node, not a group, or neither node i - 1 nor one of its ancestors
  kCqnGroupPayload,        // a group with a payload
  kCqnTooDeep,             // a group deeper than kCqnMaxDepth - 1 or a leaf deeper than kCqnMaxDepth
};

inline int cqn_check_args(const uint64_t *c_offsets, const tfidf_qnode *nodes, const uint64_t *q_node_offsets,
                          uint64_t n_q, uint64_t *at_q, uint64_t *at_n) {
  *at_q = *at_n = 0;
  if (n_q > kCqMaxQueries) return kCqnTooManyQueries;
  if (n_q == 0) return kCqnOk;
  if (q_node_offsets[0] != 0) return kCqnBadQueryOffsets;
  for (uint64_t q = 0; q < n_q; q++) {
    *at_q = q;
    if (q_node_offsets[q + 1] < q_node_offsets[q]) return kCqnBadQueryOffsets;
    if (q_node_offsets[q + 1] - q_node_offsets[q] > kCqnMaxNodes) return kCqnTooManyInQuery;
  }
  const uint64_t n_n = q_node_offsets[n_q];
  *at_q = 0;
  if (n_n > kCqnMaxNodesPerCall) return kCqnTooManyNodes;
  if (n_n == 0) return kCqnOk;
  if (c_offsets[0] != 0) return kCqnBadPayloadOffsets;
  for (uint64_t q = 0; q < n_q; q++) {
    const uint64_t n0 = q_node_offsets[q];
    const uint32_t n = (uint32_t)(q_node_offsets[q + 1] - n0);
    const tfidf_qnode *nd = nodes + n0;
    uint32_t depth[kCqnMaxNodes];
    *at_q = q;
    for (uint32_t i = 0; i < n; i++) {
      *at_n = i;
      if (c_offsets[n0 + i + 1] < c_offsets[n0 + i]) return kCqnBadPayloadOffsets;
      if (nd[i].occur > TFIDF_OCCUR_FILTER) return kCqnBadOccur;
      if (nd[i].kind > TFIDF_CLAUSE_GROUP) return kCqnBadKind;
      const bool group = nd[i].kind == TFIDF_CLAUSE_GROUP;
      if (i == 0) {
        if (!group || nd[0].parent != TFIDF_QNODE_ROOT) return kCqnBadRoot;
        depth[0] = 0;
      } else {
        const uint32_t p = nd[i].parent;
        if (p >= i || nd[p].kind != TFIDF_CLAUSE_GROUP) return kCqnBadParent;
        uint32_t a = i - 1;                                  // pre-order: the parent is node i - 1 or above it
        while (a != p && a != 0) a = nd[a].parent;
        if (a != p) return kCqnBadParent;
        depth[i] = depth[p] + 1;
      }
      if (group && c_offsets[n0 + i + 1] != c_offsets[n0 + i]) return kCqnGroupPayload;
      if (depth[i] > (group ? kCqnMaxDepth - 1 : kCqnMaxDepth)) return kCqnTooDeep;
    }
  }
  *at_q = *at_n = 0;
  return kCqnOk;
}

// A query's node table as the device pass holds it: per node its parent, its
// occur towards the parent, whether it is a group, and the group's m; per group,
// filled by cqn_count_children, what its children ask (CqNeeds).
struct CqnNode {
  uint32_t parent, min_should;
  uint8_t occur, group;
};

// needs[i] of every group i from its children's occurs; nodes that name no valid
// group as their parent are left out (the walk below never reaches them)
TFIDF_HD void cqn_count_children(const CqnNode *nd, uint32_t n, CqNeeds *needs) {
  for (uint32_t i = 0; i < n; i++) needs[i] = CqNeeds{0, 0};
  for (uint32_t i = 1; i < n; i++)
    if (nd[i].parent < i && nd[nd[i].parent].group) cq_needs_add(&needs[nd[i].parent], nd[i].occur);
}

// One child of a group holds the document with this score: cq_apply plus the count of SHOULD children.
TFIDF_HD void cqn_apply(uint32_t occur, float score, uint8_t *req, uint8_t *n_should, uint8_t *flags, double *must,
                        double *should) {
  cq_apply(occur, score, req, flags, must, should);
  if (occur == TFIDF_OCCUR_SHOULD) *n_should = (uint8_t)(*n_should + 1);   // at most kCqnMaxNodes - 1 children
}

// the SHOULD children a document needs in a group; 32 bits, so that no m wraps
TFIDF_HD uint32_t cqn_need(const CqNeeds &n, uint32_t min_should) {
  const uint32_t least = n.n_req == 0 ? 1u : 0u;
  return min_should > least ? min_should : least;
}

TFIDF_HD bool cqn_match(const CqNeeds &n, uint32_t min_should, uint32_t req, uint32_t n_should, uint32_t flags) {
  if (flags & kCqVeto) return false;
  if (req != n.n_req) return false;
  return n_should >= cqn_need(n, min_should);
}

// The pre-order walk over a query's nodes, the same on the host and in the
// kernel: cqn_next gives, one at a time, the opening of a group (clear its
// level), a leaf (apply its row to its parent's level), the closing of a group
// (evaluate its level; apply the result to the level below as one child) and the
// end.  level is the group's depth; a leaf's level is its parent's.  The open
// groups are a chain of parents, so the walk keeps the innermost one and their
// count.  Every step is checked: a table that is not a pre-order tree of at most
// kCqnMaxDepth open groups ends the walk early; a level is always below
// kCqnMaxDepth and a node below n.
enum { kCqnOpen, kCqnLeaf, kCqnClose, kCqnEnd };
struct CqnWalk {
  uint32_t i = 0, sp = 0, top = 0;       // next node; open groups; the innermost of them (sp > 0)
};

TFIDF_HD int cqn_close(CqnWalk *w, const CqnNode *nd, uint32_t n, uint32_t *node, uint32_t *level) {
  *node = w->top;
  *level = --w->sp;
  if (w->sp > 0) {
    const uint32_t up = nd[w->top].parent;
    if (up < w->top) {
      w->top = up;
    } else {                                                   // not a tree: this step is the last
      w->sp = 0;
      w->i = n;
    }
  }
  return kCqnClose;
}

TFIDF_HD int cqn_next(CqnWalk *w, const CqnNode *nd, uint32_t n, uint32_t *node, uint32_t *level) {
  if (w->i >= n) return w->sp ? cqn_close(w, nd, n, node, level) : kCqnEnd;
  const uint32_t i = w->i;
  if (i == 0 ? w->sp != 0 : w->sp == 0) return kCqnEnd;        // a second root, or a node after the root closed
  if (i > 0 && nd[i].parent != w->top) return cqn_close(w, nd, n, node, level);
  *node = i;
  w->i++;
  if (!nd[i].group) {
    if (w->sp == 0) return kCqnEnd;                            // node 0 is a leaf
    *level = w->sp - 1;
    return kCqnLeaf;
  }
  if (w->sp >= kCqnMaxDepth) return kCqnEnd;
  w->top = i;
  *level = w->sp++;
  return kCqnOpen;
}

// groups open at once in a query (1 .. kCqnMaxDepth for validated nodes; 0 for no nodes)
inline uint32_t cqn_levels(const tfidf_qnode *nd, uint32_t n) {
  uint32_t depth[kCqnMaxNodes], levels = 0;
  for (uint32_t i = 0; i < n && i < kCqnMaxNodes; i++) {
    depth[i] = i ? depth[nd[i].parent] + 1 : 0;
    if (nd[i].kind == TFIDF_CLAUSE_GROUP && depth[i] + 1 > levels) levels = depth[i] + 1;
  }
  return levels;
}

// "Can node i match a document of this block": a leaf when its bin of the block
// has an entry, a group when every R child can and at least need S children can
// (MUST_NOT children only take away).  live[i] comes in as the leaves' answer
// and goes out as every node's; children follow their parent in pre-order, so
// one pass from the last node down sees a group after all its children.
// bad / can: scratch of n entries.  -> whether the root can.
TFIDF_HD bool cqn_feasible(const CqnNode *nd, const CqNeeds *needs, uint32_t n, uint8_t *live, uint8_t *bad,
                           uint8_t *can) {
  for (uint32_t i = 0; i < n; i++) bad[i] = can[i] = 0;
  for (uint32_t i = n; i-- > 0;) {
    if (nd[i].group) live[i] = !bad[i] && can[i] >= cqn_need(needs[i], nd[i].min_should);
    if (i == 0 || nd[i].parent >= i) continue;
    const uint32_t p = nd[i].parent, o = nd[i].occur;
    if ((o == TFIDF_OCCUR_MUST || o == TFIDF_OCCUR_FILTER) && !live[i]) bad[p] = 1;
    else if (o == TFIDF_OCCUR_SHOULD && live[i]) can[p] = (uint8_t)(can[p] + 1);
  }
  return n > 0 && live[0];
}

// A query's bound on its hits: a leaf's is its row size (rows[i], unused for
// groups), a group's the smallest bound among its R children, or without R the
// sum of its S children's; never more than n_docs.
inline uint64_t cqn_hit_bound(const tfidf_qnode *nd, const uint64_t *rows, uint32_t n, uint64_t n_docs) {
  if (n == 0 || n > kCqnMaxNodes) return 0;
  uint64_t bound[kCqnMaxNodes], min_req[kCqnMaxNodes], sum_should[kCqnMaxNodes];
  for (uint32_t i = 0; i < n; i++) {
    min_req[i] = UINT64_MAX;
    sum_should[i] = 0;
  }
  for (uint32_t i = n; i-- > 0;) {
    bound[i] = nd[i].kind == TFIDF_CLAUSE_GROUP ? (min_req[i] != UINT64_MAX ? min_req[i] : sum_should[i]) : rows[i];
    if (bound[i] > n_docs) bound[i] = n_docs;
    if (i == 0) break;
    const uint32_t p = nd[i].parent;
    if (nd[i].occur == TFIDF_OCCUR_MUST || nd[i].occur == TFIDF_OCCUR_FILTER) {
      if (bound[i] < min_req[p]) min_req[p] = bound[i];
    } else if (nd[i].occur == TFIDF_OCCUR_SHOULD) {
      sum_should[p] += bound[i];
    }
  }
  return bound[0];
}

}  // namespace tfidf
