"""Incremental inversion: a block-major commit keeps the count rows, bases and
postings of the 8192-document blocks whose documents were all present at the
target snapshot's last inversion and builds the later blocks only
(tfidf_commit_inverted_blocks says which; csrc/commit_plan.h decides).

Documents are 3-6 words over <= 400 words, so two full blocks cost about 16 k
short documents: the smallest shape that has a kept block.  Every state is
compared with a FRESH index built in one commit from the same documents and
with the CPU oracle, bit for bit, on tfidf_stats (as test_gpu_incremental_commit
compares them), df of every term, all hits (k = 0: every posting of every
block) and the top 10 of every vocabulary word and a few 2-3-term queries, and
doc_terms / doc_len of every document of the re-inverted blocks and of a seeded
256 of the kept ones.  The fresh index and the oracle's answers are computed
once per document list and shared.
"""
import random

import pytest

from oracle import oracle as O
from tfidf_amd import _lib as L
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

from test_gpu_incremental_commit import add, keyed, published
from test_gpu_parity import assert_hits_equal

pytestmark = pytest.mark.gpu

BLOCK = 8192
_rng = random.Random(20260)
TEXTS = [b" ".join(synth.word(_rng.randint(1, 400)) for _ in range(_rng.randint(3, 6))) for _ in range(25200)]
DOCS = keyed(TEXTS)
MULTI = [synth.word(7) + b" " + synth.word(300), synth.word(1) + b" " + synth.word(2) + b" " + synth.word(399),
         synth.word(120) + b" " + synth.word(121), synth.word(400) + b" " + synth.word(55) + b" " + synth.word(9)]
ESC_DOC = b"zq " * 2100                                # tf 2100 >= 2047: a posting escape


class Expect:
    """What a fresh one-commit index of `docs` and the oracle answer."""

    def __init__(self, docs, extra_queries=(), **ctor):
        self.docs = docs
        self.o = o = O.OracleIndex()
        for k, t in docs:
            o.add_doc(k, t)
        o.commit()
        self.vocab = o.vocab()
        self.queries = sorted(self.vocab) + MULTI + list(extra_queries)
        self.hits = {(q, k): o.search(q, k) for q in self.queries for k in (0, 10)}
        self._rows = {}
        f = ShardIndex(**ctor)
        try:
            add(f, docs)
            f.commit()
            assert f.commit_tokenized_docs() == {"docs": len(docs), "was_full": True}
            n_blocks = (len(docs) + BLOCK - 1) // BLOCK
            assert f.commit_inverted_blocks() == {"first_block": 0, "n_blocks": n_blocks, "remapped": 0}
            self.stats = published(f)
            self.check(f, n_blocks - 1 if n_blocks else 0, stats=False)     # the fresh index against the oracle
        finally:
            f.close()

    def row(self, d):
        if d not in self._rows:
            self._rows[d] = (self.o.doc_terms(d), (self.o.doc_len(d), self.o.doc_norm(d)))
        return self._rows[d]

    def check(self, g, first_block, stats=True, rows=True):
        if stats:
            assert published(g) == self.stats
        s = g.stats()
        assert (s["num_docs"], s["doc_count"], s["sum_ttf"], s["num_terms"], s["nnz"]) == \
            (len(self.docs), self.o.doc_count, self.o.sum_ttf, self.o.num_terms, sum(self.vocab.values()))
        for t, df in self.vocab.items():
            assert g.df(t) == (df, df), t[:40]
        for q in self.queries:
            for k in (0, 10):
                assert_hits_equal(g.search(q, k), self.hits[q, k])
        if not rows:
            return
        kept = min(first_block * BLOCK, len(self.docs))
        ids = list(range(kept, len(self.docs))) + random.Random(first_block).sample(range(kept), min(256, kept))
        for d in ids:
            terms, ln = self.row(d)
            assert g.doc_terms(d) == terms, d
            assert g.doc_len(d) == ln, d


_expect = {}


def expect(docs, extra_queries=(), **ctor):
    key = (len(docs), hash(tuple(k for k, _ in docs[-300:])), hash(tuple(t for _, t in docs[-300:])),
           tuple(extra_queries), tuple(sorted(ctor.items())))
    if key not in _expect:
        _expect[key] = Expect(docs, extra_queries, **ctor)
    return _expect[key]


def commit_and_check(g, docs, first_block, remapped=0, tokenized=None, full=False, extra_queries=(), rows=True, **ctor):
    g.commit()
    n_blocks = (len(docs) + BLOCK - 1) // BLOCK
    assert g.commit_inverted_blocks() == {"first_block": first_block, "n_blocks": n_blocks, "remapped": remapped}
    if tokenized is not None:
        assert g.commit_tokenized_docs() == {"docs": tokenized, "was_full": full}
    expect(docs, extra_queries, **ctor).check(g, first_block, rows=rows)


def twice(docs, **ctor):
    g = ShardIndex(**ctor)
    add(g, docs)
    g.commit()
    g.commit()
    assert g.commit_inverted_blocks()["first_block"] == 0       # each snapshot's first build
    return g


# ---------------------------------------------------------------------------

def test_kept_blocks_across_commits():
    g = twice(DOCS[:16500])
    add(g, DOCS[16500:16700])
    docs = DOCS[:16700]
    commit_and_check(g, docs, 2, tokenized=200)                  # blocks 0 and 1 kept, the tail block built
    commit_and_check(g, docs, 2, tokenized=200)                  # the other snapshot
    commit_and_check(g, docs, 2, tokenized=0)                    # nothing added: the tail block is inverted again
    g.close()


def test_new_documents_fill_the_tail_and_add_two_blocks():
    g = twice(DOCS[:8100])
    add(g, DOCS[8100:16600])
    commit_and_check(g, DOCS[:16600], 0, tokenized=8500)         # no block was full
    # ... in the other snapshot either (every row was read from this document list just above)
    commit_and_check(g, DOCS[:16600], 0, tokenized=8500, rows=False)
    add(g, DOCS[16600:24800])
    commit_and_check(g, DOCS[:24800], 2, tokenized=8200)         # blocks 0, 1 kept; block 2 filled, block 3 new
    commit_and_check(g, DOCS[:24800], 2, tokenized=8200, rows=False)   # the other snapshot, the same
    g.close()


def test_exact_multiple_of_the_block_with_nothing_added():
    g = twice(DOCS[:2 * BLOCK])
    commit_and_check(g, DOCS[:2 * BLOCK], 2, tokenized=0)        # first_block == n_blocks: no tile kernel has work
    add(g, DOCS[2 * BLOCK:2 * BLOCK + 1])
    commit_and_check(g, DOCS[:2 * BLOCK + 1], 2, tokenized=1)    # a one-document block behind them
    g.close()


def test_new_terms_force_the_remap():
    ctor = dict(vocab_capacity_log2=10)
    rng = random.Random(50)
    fresh_words = [synth.word(1000 + j) for j in range(50)]      # absent before: 450 terms in 1024 slots
    later = [b" ".join([fresh_words[i % 50]] + [synth.word(rng.randint(1, 400)) for _ in range(rng.randint(2, 4))])
             for i in range(150)] + [fresh_words[3] + b" " + fresh_words[49]]
    base = DOCS[:16500]
    docs = base + keyed(later, 16500)
    extra = [fresh_words[0] + b" " + synth.word(7), fresh_words[49] + b" " + fresh_words[3], fresh_words[10]]
    g = twice(base, **ctor)
    add(g, docs[16500:])
    commit_and_check(g, docs, 2, remapped=1, tokenized=len(later), extra_queries=extra, **ctor)
    commit_and_check(g, docs, 2, remapped=1, tokenized=len(later), extra_queries=extra, **ctor)   # the other snapshot
    more = keyed(TEXTS[20000:20100], len(docs))                  # no new word
    add(g, more)
    docs = docs + more
    commit_and_check(g, docs, 2, remapped=0, tokenized=100, extra_queries=extra, **ctor)
    g.close()


def test_posting_escapes_in_kept_and_new_blocks():
    texts = list(TEXTS[:16600])
    texts[100] = ESC_DOC                                         # block 0
    texts[8250] = ESC_DOC + b"tail"                              # block 1
    texts[16500] = b"head " + ESC_DOC                            # block 2
    docs = keyed(texts)
    g = twice(docs[:8300])
    # block 0 kept with its escape; the re-inverted tail block holds the second: its entry is not kept twice
    commit_and_check(g, docs[:8300], 1, tokenized=0, extra_queries=[b"zq", b"zq tail"])
    assert g.doc_terms(100) == {b"zq": 2100} and g.doc_terms(8250) == {b"zq": 2100, b"tail": 1}
    add(g, docs[8300:])                                          # ("head" is a new term: the kept rows move as well)
    commit_and_check(g, docs, 1, remapped=1, tokenized=8300, extra_queries=[b"zq", b"zq tail", b"head zq"])
    assert g.doc_terms(16500) == {b"head": 1, b"zq": 2100}
    assert [d for d, _ in g.search(b"zq", 0)] and sorted(d for d, _ in g.search(b"zq", 0)) == [100, 8250, 16500]
    commit_and_check(g, docs, 1, remapped=1, tokenized=8300, extra_queries=[b"zq", b"zq tail", b"head zq"])
    commit_and_check(g, docs, 2, tokenized=0, extra_queries=[b"zq", b"zq tail", b"head zq"])   # two kept escapes, one built again
    g.close()


# ---------------------------------------------------------------------------
# fallbacks: every block inverted, equal results

def test_term_major_inverts_everything():
    ctor = dict(inversion=L.INVERSION_TERM)
    g = twice(DOCS[:16500], **ctor)
    add(g, DOCS[16500:16700])
    commit_and_check(g, DOCS[:16700], 0, tokenized=200, **ctor)
    assert g.stats()["term_major"] == 1
    g.close()


def test_full_inversion_switch(monkeypatch):
    g = twice(DOCS[:16500])
    add(g, DOCS[16500:16700])
    monkeypatch.setenv("TFIDF_FULL_INVERSION", "1")
    commit_and_check(g, DOCS[:16700], 0, tokenized=200)          # the rows are still kept
    monkeypatch.delenv("TFIDF_FULL_INVERSION")
    commit_and_check(g, DOCS[:16700], 2, tokenized=200)          # the other snapshot; nothing kept depends on the switch
    commit_and_check(g, DOCS[:16700], 2, tokenized=0)            # ... nor what the commit under it built
    g.close()


def test_delete_then_commit_inverts_everything():
    g = twice(DOCS[:16500])
    assert g.delete_documents([DOCS[9000][0]]) == 1
    docs = DOCS[:9000] + DOCS[9001:16500]
    g.commit()
    assert g.commit_inverted_blocks() == {"first_block": 0, "n_blocks": 3, "remapped": 0}
    assert g.commit_tokenized_docs()["was_full"]
    e = expect(docs)
    drop = ("text_bytes", "dead_docs", "dead_bytes")             # the fresh index never held the dead text
    assert {k: v for k, v in published(g).items() if k not in drop} == {k: v for k, v in e.stats.items() if k not in drop}
    e.check(g, 0, stats=False)
    g.close()


def test_commit_after_a_failed_one_inverts_everything(monkeypatch):
    monkeypatch.setenv("TFIDF_PACK_DOCS", "1")
    ctor = dict(vocab_capacity_log2=10)
    g = twice(DOCS[:16500], **ctor)
    offender = (b"offender", b" ".join(synth.word(5000 + j) for j in range(700)))    # 400 + 700 > 2^10
    add(g, [offender])
    with pytest.raises(L.TfidfError) as err:
        g.commit()                                               # incremental over the kept dictionary: fails
    assert err.value.code == L.E_CAPACITY
    assert g.delete_documents([b"offender"]) == 1
    g.compact()
    g.commit()                                                   # the failed build left nothing to keep
    assert g.commit_inverted_blocks() == {"first_block": 0, "n_blocks": 3, "remapped": 0}
    assert g.commit_tokenized_docs() == {"docs": 16500, "was_full": True}
    expect(DOCS[:16500], **ctor).check(g, 0)
    g.close()
