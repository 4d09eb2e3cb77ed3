"""Nested compound queries restated in plain Python (DESIGN.md section 2,
"Nested compound queries"; helper of test_compound_tree_cpu.py,
test_gpu_compound_tree.py and test_gpu_node_compound_tree.py).

A query is a group: (GROUP, children, m).  A child is (occur,) + a leaf clause of
compound_ref, (occur, kind, payload, params...), or (occur,) + a group.  A plain
list of occurred clauses is a root group with m = 0.

combine_tree(group, rows) is the rule.  A leaf's set is its row, rows(leaf) ->
{doc: float32 score}; a group child's set is the documents it matches, each
with the float32 score this rule gives it.  With R the group's MUST and FILTER
children, N its MUST_NOT children, S its SHOULD children and need = max(m, 1 if
R is empty else 0), a document matches when every R child holds it, no N child
holds it and at least need S children hold it (plain Python integers: no m
wraps).  must = float32 of the Python-float (double) sum of the MUST children's
scores, should = float32 of the double sum of the scores of the S children that
hold the document, both in child order; the score is must + should in one
float32 addition when both exist, else the one that does, else 0.0.  Nothing is
rewritten: the tree is evaluated as written.  Order: score bits descending, doc
ascending.
"""
import numpy as np

import compound_ref as CR
from compound_ref import FILTER, MUST, MUST_NOT, SHOULD

GROUP = 5
F32 = np.float32


def group(children, m=0):
    return (GROUP, tuple(children), int(m))


def as_root(query):
    if isinstance(query, tuple) and len(query) == 3 and query[0] == GROUP:
        return query
    return group(query)


def is_group(node):
    """node: a child without its occur, or a root."""
    return node[0] == GROUP


def match_tree(node, rows):
    """{doc: float32 score} of a group (GROUP, children, m)."""
    _, children, m = node
    sets = [(c[0], match_tree(c[1:], rows) if is_group(c[1:]) else rows(c)) for c in children]
    req = [s for o, s in sets if o in (MUST, FILTER)]
    opt = [s for o, s in sets if o == SHOULD]
    veto = [s for o, s in sets if o == MUST_NOT]
    need = max(int(m), 0 if req else 1)
    if need > len(opt):
        return {}
    cand = set.intersection(*[set(s) for s in req]) if req else set().union(*[set(s) for s in opt])
    out = {}
    for d in cand:
        if any(d in s for s in veto) or sum(d in s for s in opt) < need:
            continue
        out[d] = CR.score_of([o for o, _ in sets], [s.get(d) for _, s in sets])
    return out


def combine_tree(node, rows):
    """[(doc, float32 score)] of one query; rows(leaf) -> {doc: float32 score}."""
    out = list(match_tree(as_root(node), rows).items())
    out.sort(key=lambda h: (-CR.bits(h[1]), h[0]))
    return out


def leaves(node):
    """The occurred leaf clauses of a query, in pre-order."""
    out = []
    for c in as_root(node)[1]:
        out.extend(leaves(c[1:]) if is_group(c[1:]) else [c])
    return out


def n_nodes(node):
    return 1 + sum(n_nodes(c[1:]) if is_group(c[1:]) else 1 for c in as_root(node)[1])


def depth(node):
    """The deepest leaf or group below this root (the root is depth 0)."""
    return max([0] + [1 + (depth(c[1:]) if is_group(c[1:]) else 0) for c in as_root(node)[1]])


class NestedRef:
    """combine_tree over CompoundRef's clause rows: the same oracle, statistics
    (``global_stats`` as CompoundRef takes them) and row cache."""

    def __init__(self, texts, k1=1.2, b=0.75, global_stats=None, ref=None):
        self.ref = ref if ref is not None else CR.CompoundRef(texts, k1, b, global_stats)
        self._own = ref is None

    def close(self):
        if self._own:
            self.ref.close()

    def row(self, clause):
        return self.ref.row(clause)

    def search(self, query):
        return combine_tree(query, self.ref.row)

    def search_batch(self, queries):
        return [self.search(q) for q in queries]
