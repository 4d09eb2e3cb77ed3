"""Compound queries restated in plain Python ("Compound
queries"; helper of test_compound_cpu.py, test_gpu_compound.py and
test_gpu_node_compound.py).

A clause is the tuple of tfidf_amd.engine: (occur, kind, payload, params...).
Its row {doc: float32 score} comes from the reference of its kind on one
oracle over the documents: the oracle's search(q, 0) for TEXT (a payload that
does not parse has an empty row), phrase_slop_ref for PHRASE (slop 0 is the
exact rule), wildcard_ref / regex_ref expected_docs with score 1.0 for WILDCARD
and REGEX, fuzzy_search_ref's expansion + clause_scores + hits for FUZZY.

combine(occurs, rows) is the rule: with R the MUST and FILTER rows, N the
MUST_NOT rows and S the SHOULD rows, a document matches when it is in every row
of R, in no row of N and, when R is empty, in a row of S.  must = float32 of the
Python-float (double) sum of the MUST scores, should = float32 of the double sum
of the scores of the SHOULD rows that hold the document, both in clause order;
the score is must + should in one float32 addition when both exist, else the one
that does, else 0.0.  Order: score bits descending, doc ascending.
"""
import numpy as np

import fuzzy_search_ref as R
import phrase_ref as P
import phrase_slop_ref as S
import regex_ref as X
import wildcard_ref as W
from oracle import oracle as O

SHOULD, MUST, MUST_NOT, FILTER = 0, 1, 2, 3
TEXT, PHRASE, WILDCARD, REGEX, FUZZY = 0, 1, 2, 3, 4
F32 = np.float32


def bits(x) -> int:
    return int(F32(x).view(np.uint32))


def exact(hits):
    return [(int(d), bits(s)) for d, s in hits]


def score_of(occurs, scores):
    """The score of a matching document: scores[i] is clause i's float32 score, or None when its row lacks the document."""
    must = should = None
    for o, s in zip(occurs, scores):
        if s is None:
            continue
        if o == MUST:
            must = (must or 0.0) + float(F32(s))
        elif o == SHOULD:
            should = (should or 0.0) + float(F32(s))
    if must is not None and should is not None:
        return F32(F32(must) + F32(should))
    if must is not None:
        return F32(must)
    if should is not None:
        return F32(should)
    return F32(0.0)


def combine(occurs, rows):
    """[(doc, float32 score)] of one query: rows[i] = {doc: float32 score} of clause i."""
    req = [r for o, r in zip(occurs, rows) if o in (MUST, FILTER)]
    veto = [r for o, r in zip(occurs, rows) if o == MUST_NOT]
    opt = [r for o, r in zip(occurs, rows) if o == SHOULD]
    if not req and not opt:
        return []
    cand = set.intersection(*[set(r) for r in req]) if req else set().union(*[set(r) for r in opt])
    out = []
    for d in cand:
        if any(d in r for r in veto):
            continue
        out.append((d, score_of(occurs, [r.get(d) for r in rows])))
    out.sort(key=lambda h: (-bits(h[1]), h[0]))
    return out


def merge(lists_with_base):
    """[(hits, doc_base)] of the shards -> one list by (score bits descending, global id ascending)."""
    out = [(d + base, s) for hits, base in lists_with_base for d, s in hits]
    out.sort(key=lambda h: (-bits(h[1]), h[0]))
    return out


class CompoundRef:
    """The clause rows over ``texts`` (the live documents in live order) on one
    oracle, with the shard's own statistics or the GLOBAL ones given as
    (doc_count, sum_ttf, {term: df}); the vocabulary a wildcard, regex or fuzzy
    clause expands on is always the shard's own."""

    def __init__(self, texts, k1=1.2, b=0.75, global_stats=None):
        self.k1, self.b = k1, b
        self.phrase = P.PhraseRef(texts, k1, b, global_stats)
        self.o = self.phrase.o
        self.n = self.o.num_docs
        self.vocab = self.o.vocab()
        rows = [self.o.doc_terms(d) for d in range(self.n)]
        self.term_sets = [set(r) for r in rows]
        norms = [self.o.doc_norm(d) for d in range(self.n)]
        self.shard = R.Shard.from_rows(rows, norms, self.vocab, self.o.doc_count, self.o.sum_ttf)
        self.stats = {}
        if global_stats is not None:
            dc, ttf, df = global_stats
            self.o.set_global_stats(dc, ttf, {t: df.get(t, 0) for t in self.vocab})
            self.stats = dict(df_of=df, doc_count=dc, sum_ttf=ttf)
        self._rows = {}

    def close(self):
        self.phrase.close()

    def row(self, clause):
        key = tuple(clause[1:])
        if key not in self._rows:
            self._rows[key] = self._row(*key)
        return self._rows[key]

    def _row(self, kind, payload, *params):
        if kind == TEXT:
            try:
                return {d: F32(s) for d, s in self.o.search(payload, 0)}
            except (O.QuerySyntaxError, ValueError):
                return {}
        if kind == PHRASE:
            return {d: F32(s) for d, s, _ in S.search(self.phrase, payload, params[0] if params else 0)}
        if kind == WILDCARD:
            return {d: F32(1.0) for d in W.expected_docs(self.term_sets, self.vocab, payload)[0]}
        if kind == REGEX:
            return {d: F32(1.0) for d in X.expected_docs(self.term_sets, self.vocab, payload)[0]}
        if kind == FUZZY:
            e, p, m = (tuple(params) + (2, 0, 50)[len(params):])[:3]
            exp, _ = R.expansion(self.vocab, payload, e, p, m)
            return dict(R.hits(R.clause_scores(self.shard, exp, k1=self.k1, b=self.b, **self.stats)))
        raise ValueError("unknown kind %r" % (kind,))

    def search(self, clauses):
        return combine([c[0] for c in clauses], [self.row(c) for c in clauses])

    def search_batch(self, queries):
        return [self.search(q) for q in queries]
