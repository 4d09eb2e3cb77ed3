"""Incremental commits: a commit whose build target was built from a prefix of
the same staged corpus tokenizes the documents added since only
(tfidf_commit_tokenized_docs says which kind ran and how many documents it
took) and still rebuilds df, counts and postings from all rows.

Every comparison is against a FRESH index built in one commit from the same
documents, and against the CPU oracle, bit for bit: tfidf_stats (without the
lifetime query counters), malformed ids, df of every term, doc_len / doc_terms
of every document, all hits and the top 10 of 20 queries.  Of tfidf_stats,
device_bytes and compactions are left out everywhere: they describe buffer
capacities and the index's lifetime (an index grown by appends holds
geometrically grown buffers, as the staged corpus always has), not the
published index; after a delete the staged-corpus fields (text_bytes,
dead_docs, dead_bytes) are left out as well, since the fresh index never held
the dead text.  pack_retried counts the documents the packed windows of the
builds that tokenized them handed to the one-document pass; packs start at a
build's first document and their size follows the staged corpus's average
document, so the count depends on where the commits fell (and a full build over dead
documents retries the packs whose sources are not contiguous, which a fresh
index of the live documents never sees).  It is compared where the packs of
the two histories coincide by construction (aligned=True: a fixed pack size,
batches that are multiples of it, no dead documents) and left out elsewhere.
"""
import random

import pytest

from oracle import oracle as O
from tfidf_amd import _lib as L
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

from test_gpu_parity import QUERY_COUNTERS, assert_hits_equal

pytestmark = pytest.mark.gpu

CAPACITY_FIELDS = ("device_bytes", "compactions")
STAGED_FIELDS = ("text_bytes", "dead_docs", "dead_bytes")
QUERIES = synth.queries(20, lo=1, hi=3000)
LONG_TERM = b"supercalifragilisticexpialidocious"          # > 16 bytes: a hashed key with a deferred identity check


def published(g, staged=True, aligned=False):
    drop = QUERY_COUNTERS + CAPACITY_FIELDS + (() if staged else STAGED_FIELDS) + (() if aligned else ("pack_retried",))
    return {k: v for k, v in g.stats().items() if k not in drop}


def keyed(texts, base=0):
    return [(b"k%06d" % (base + i), t) for i, t in enumerate(texts)]


def add(g, docs):
    g.add_documents([t for _, t in docs], [k for k, _ in docs])


def live_docs(docs):
    """updateDocument order: a key added again moves to the end."""
    out = {}
    for k, t in docs:
        out.pop(k, None)
        out[k] = t
    return list(out.items())


def assert_same_as_fresh(g, docs, queries=QUERIES, staged=True, aligned=False, **ctor):
    """g == a new index given `docs` (live, in order) in one commit == the oracle."""
    f = ShardIndex(**ctor)
    add(f, docs)
    f.commit()
    assert f.commit_tokenized_docs() == {"docs": len(docs), "was_full": True}
    o = O.OracleIndex()
    for k, t in docs:
        o.add_doc(k, t)
    o.commit()
    try:
        assert published(g, staged, aligned) == published(f, staged, aligned)
        s = g.stats()
        vocab = o.vocab()
        assert (s["num_docs"], s["doc_count"], s["sum_ttf"], s["num_terms"], s["nnz"]) == \
            (len(docs), o.doc_count, o.sum_ttf, o.num_terms, sum(vocab.values()))
        assert g.malformed_docs() == f.malformed_docs() == o.malformed_docs()
        for t, df in vocab.items():
            assert g.df(t) == f.df(t) == (df, df), t[:40]
        for d in range(len(docs)):
            want = o.doc_terms(d)
            assert g.doc_terms(d) == want and f.doc_terms(d) == want, d
            assert g.doc_len(d) == f.doc_len(d) == (o.doc_len(d), o.doc_norm(d)), d
        assert g.doc_key(len(docs) - 1) == docs[-1][0]
        for q in queries:
            for k in (0, 10):
                want = o.search(q, k)
                assert_hits_equal(g.search(q, k), want)
                assert_hits_equal(f.search(q, k), want)
    finally:
        f.close()
        o.close()


def commit_and_expect(g, docs, n_tok, full, **kw):
    g.commit()
    assert g.commit_tokenized_docs() == {"docs": n_tok, "was_full": full}
    assert_same_as_fresh(g, live_docs(docs), **kw)


# ---------------------------------------------------------------------------

def test_three_batches_four_commits_and_an_empty_fifth():
    b = [keyed(synth.corpus(n, V=3000, len_min=20, len_max=80, doc_base=base), base)
         for base, n in ((0, 300), (300, 310), (610, 290))]
    g = ShardIndex()
    docs = []
    for batch, n_tok, full in ((b[0], 300, True), (b[1], 610, True), (b[2], 600, False)):
        add(g, batch)
        docs += batch
        commit_and_expect(g, docs, n_tok, full)        # 3rd: its target held batch 0 only
    commit_and_expect(g, docs, 290, False)             # 4th, nothing added: the other snapshot lacked batch 2
    commit_and_expect(g, docs, 0, False)               # 5th: nothing to tokenize, the inversion still runs
    assert g.commit_timing()["nnz"] == g.stats()["nnz"] > 0
    g.close()


def test_block_edge_crossed_by_the_new_documents():
    rng = random.Random(8192)
    texts = [b" ".join(synth.word(rng.randint(1, 400)) for _ in range(rng.randint(3, 6))) for _ in range(8300)]
    docs = keyed(texts)
    g = ShardIndex()
    add(g, docs[:8100])
    g.commit()
    g.commit()
    assert g.commit_tokenized_docs() == {"docs": 8100, "was_full": True}
    add(g, docs[8100:])                                # 8192 = kBlockDocs lies inside the new documents
    commit_and_expect(g, docs, 200, False, queries=QUERIES[:6] + [synth.word(7), synth.word(7) + b" " + synth.word(300)])
    g.close()


def path_batch():
    """Documents of every tokenizer path."""
    rng = random.Random(4)
    cdf = synth.zipf_cdf(3000)
    over4k = b" ".join(synth.word(int(r)) for r in synth.doc_ranks(5, 900, 900, 900, cdf))
    book = b" ".join(synth.word(int(r)) for r in synth.doc_ranks(6, 25000, 25000, 25000, cdf))
    assert len(over4k) > 4096 and 120_000 < len(book) < 200_000
    texts = synth.corpus(60, V=3000, len_min=20, len_max=80, doc_base=9000)
    texts += [over4k, book,
              "café naïve élan été crème brûlée".encode(), "it’s “quoted” don’t".encode(),
              "ภาษาไทย 😀 👍🏽 中文 straße".encode(),        # characters the wave rules decline: Unicode wave path
              b"ok \xff\xfe text", b"caf\xe9 fine",          # not UTF-8: indexed empty, listed
              b"", b"  ..  ",
              LONG_TERM + b" first seen here " + LONG_TERM]
    rng.shuffle(texts)
    return texts


def test_later_batch_holds_documents_of_every_path():
    first = keyed(synth.corpus(300, V=3000, len_min=20, len_max=80))
    later = keyed(path_batch(), 300)
    g = ShardIndex()
    add(g, first)
    g.commit()
    g.commit()
    add(g, later)
    qs = QUERIES[:12] + ["café".encode(), "it’s".encode(), "中文".encode(), LONG_TERM, b"fine text"]
    docs = first + later
    commit_and_expect(g, docs, len(later), False, queries=qs)
    s = g.stats()
    assert s["long_docs"] >= 2 and s["unicode_docs"] >= 3 and s["malformed_docs"] == 2
    # the other snapshot takes the same batch over its own dictionary; then both are complete
    commit_and_expect(g, docs, len(later), False, queries=qs)
    commit_and_expect(g, docs, 0, False, queries=qs)
    # and one more batch of every path behind kept long, non-ASCII and malformed documents
    more = keyed(path_batch()[:40] + [b"another bad \xc3 one"], 300 + len(later))
    add(g, more)
    docs += more
    commit_and_expect(g, docs, len(more), False, queries=qs)
    g.close()


def test_packed_windows_with_a_pack_that_retries(monkeypatch):
    monkeypatch.setenv("TFIDF_PACK_DOCS", "4")
    rng = random.Random(44)

    def short(n):
        return [b" ".join(synth.word(rng.randint(1, 500)) for _ in range(rng.randint(1, 12))) for _ in range(n)]
    first = keyed(short(400))
    later_texts = short(40)
    later_texts[9] = b""                               # an empty document inside a pack: the pack retries
    later_texts[22] = "café crème".encode()            # and a non-ASCII one
    later = keyed(later_texts, 400)
    g = ShardIndex()
    add(g, first)
    g.commit()
    g.commit()
    assert g.stats()["pack_docs"] == 4 and g.stats()["pack_retried"] == 0
    add(g, later)
    commit_and_expect(g, first + later, 40, False, aligned=True)
    assert g.stats()["pack_retried"] >= 4
    commit_and_expect(g, first + later, 40, False, aligned=True)
    g.close()


def test_term_major_with_a_csr_escape_appended():
    ctor = dict(inversion=L.INVERSION_TERM)
    first = keyed(synth.corpus(200, V=3000, len_min=20, len_max=80) + [b"zq " * 16500])   # a kept escape (>= 16 383)
    later = keyed(synth.corpus(50, V=3000, len_min=20, len_max=80, doc_base=200) +
                  [b"zq zq " + b"ab " * 17000 + b"tail"], len(first))
    g = ShardIndex(**ctor)
    add(g, first)
    g.commit()
    g.commit()
    assert g.stats()["term_major"] == 1
    add(g, later)
    docs = first + later
    qs = QUERIES[:8] + [b"ab", b"zq", b"ab zq tail"]
    commit_and_expect(g, docs, len(later), False, queries=qs, **ctor)
    assert g.doc_terms(len(docs) - 1) == {b"zq": 2, b"ab": 17000, b"tail": 1}
    commit_and_expect(g, docs, len(later), False, queries=qs, **ctor)
    g.close()


# ---------------------------------------------------------------------------
# fallbacks: a full build, equal results

def two_commits(n=300, **ctor):
    docs = keyed(synth.corpus(n, V=3000, len_min=20, len_max=80))
    g = ShardIndex(**ctor)
    add(g, docs)
    g.commit()
    g.commit()
    return g, docs


def more_docs(base, n=30):
    return keyed(synth.corpus(n, V=3000, len_min=20, len_max=80, doc_base=base), base)


def test_delete_replace_and_compact_fall_back_to_full_builds():
    g, docs = two_commits()
    assert g.delete_documents([docs[17][0]]) == 1
    docs = docs[:17] + docs[18:]
    commit_and_expect(g, docs, 299, True, staged=False)
    commit_and_expect(g, docs, 299, True, staged=False)            # dead documents present: never incremental
    docs += [(docs[5][0], b"replaced text " + synth.word(9))]      # replace by key
    add(g, docs[-1:])
    commit_and_expect(g, docs, 299, True, staged=False)
    assert g.compact()["bytes_reclaimed"] > 0
    commit_and_expect(g, docs, 299, True)                          # the staged ids moved
    commit_and_expect(g, docs, 299, True)                          # ... for the other snapshot too
    extra = more_docs(1000)
    add(g, extra)
    docs += extra
    commit_and_expect(g, docs, 30, False)                          # and incremental again afterwards
    g.close()


def test_clear_and_save_load_fall_back_to_full_builds(tmp_path):
    g, docs = two_commits()
    g.clear()
    docs = more_docs(2000, 250)                                    # other documents at the same staged ids
    add(g, docs)
    commit_and_expect(g, docs, 250, True)
    commit_and_expect(g, docs, 250, True)
    commit_and_expect(g, docs, 0, False)
    path = str(tmp_path / "ix.tfidf")
    g.save(path)
    g.clear()
    g.load(path)
    commit_and_expect(g, docs, 250, True)
    h = ShardIndex()
    h.load(path)
    extra = more_docs(3000)
    add(h, extra)
    h.commit()
    assert h.commit_tokenized_docs() == {"docs": 280, "was_full": True}
    assert_same_as_fresh(h, docs + extra)
    g.close()
    h.close()


def test_weak_hash_rebuilds_every_commit(monkeypatch):
    monkeypatch.setenv("TFIDF_TEST_WEAK_HASH", "1")
    twin = LONG_TERM[:-1] + b"z"                                   # same length, same first bytes: collides under the weak seed
    docs = keyed(synth.corpus(100, V=3000, len_min=20, len_max=80) + [LONG_TERM + b" and " + twin])
    g = ShardIndex()
    add(g, docs)
    qs = QUERIES[:6] + [LONG_TERM, twin]
    commit_and_expect(g, docs, 101, True, queries=qs)
    assert g.stats()["hash_rebuilds"] == 1
    commit_and_expect(g, docs, 101, True, queries=qs)
    # built under seed 1, the next commit starts from the weak seed again: full, one rebuild, as a new index reports
    extra = more_docs(500)
    add(g, extra)
    docs += extra
    commit_and_expect(g, docs, 131, True, queries=qs)
    assert g.stats()["hash_rebuilds"] == 1
    g.close()


def test_a_knob_changed_between_commits(monkeypatch):
    g, docs = two_commits()
    extra = more_docs(700)
    add(g, extra)
    docs += extra
    monkeypatch.setenv("TFIDF_NO_UNIWAVE", "1")
    commit_and_expect(g, docs, 330, True)
    commit_and_expect(g, docs, 330, True)
    commit_and_expect(g, docs, 0, False)
    monkeypatch.setenv("TFIDF_FULL_COMMIT", "1")
    commit_and_expect(g, docs, 330, True)
    monkeypatch.delenv("TFIDF_FULL_COMMIT")
    commit_and_expect(g, docs, 0, False)                           # this snapshot was built without the switch
    commit_and_expect(g, docs, 330, True)                          # the other one under it: not kept
    g.close()


def test_failed_commit_then_recovery(monkeypatch):
    monkeypatch.setenv("TFIDF_PACK_DOCS", "1")
    ctor = dict(vocab_capacity_log2=10)
    docs = keyed([b" ".join(synth.word(20 * i + j + 1) for j in range(20)) for i in range(50)])   # 1000 terms
    g = ShardIndex(**ctor)
    add(g, docs)
    g.commit()
    g.commit()
    before = published(g)
    offender = (b"offender", b" ".join(synth.word(5000 + j) for j in range(100)))                 # 1100 > 2^10
    add(g, [offender])
    for _ in range(2):                 # incremental over the kept dictionary, then full over what that build left
        with pytest.raises(L.TfidfError) as e:
            g.commit()
        assert e.value.code == L.E_CAPACITY
    assert {k: v for k, v in published(g).items() if k not in STAGED_FIELDS} == \
        {k: v for k, v in before.items() if k not in STAGED_FIELDS}
    assert g.delete_documents([b"offender"]) == 1
    qs = [synth.word(1), synth.word(1000) + b" " + synth.word(3), synth.word(5001)]
    commit_and_expect(g, docs, 50, True, queries=qs, staged=False, **ctor)
    g.compact()
    extra = keyed([synth.word(1) + b" " + synth.word(1001)], 50)   # one new term: 1001 <= 1024
    add(g, extra)
    docs += extra
    commit_and_expect(g, docs, 51, True, queries=qs, **ctor)       # the failed build left nothing to keep
    commit_and_expect(g, docs, 51, True, queries=qs, **ctor)
    commit_and_expect(g, docs, 0, False, queries=qs, **ctor)
    g.close()


def test_a_held_reader_keeps_its_snapshot_out_of_the_builds():
    g, docs = two_commits()
    rd = g.reader()                                                # holds generation 2
    held = [rd.search(q, 0) for q in QUERIES]
    gen = rd.generation
    for i in range(4):
        extra = more_docs(5000 + 100 * i)
        add(g, extra)
        docs += extra
        g.commit()
        got = g.commit_tokenized_docs()
        if i == 0:
            # generation 1 is free (the reader holds 2): it covers the first 300 documents
            assert got == {"docs": 30, "was_full": False}
        elif i == 1:
            # generation 2 would be the target but is held: a new snapshot, built in full
            assert got == {"docs": len(docs), "was_full": True}
        else:
            assert got == {"docs": 60, "was_full": False}
        assert_same_as_fresh(g, docs)
        assert [rd.search(q, 0) for q in QUERIES] == held and rd.generation == gen and rd.num_docs == 300
    rd.close()
    g.close()
