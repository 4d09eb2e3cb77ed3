"""The kept df base (csrc/commit_plan.h df_base_plan): a block-major snapshot
keeps, per column, the sum of the counts of the blocks that were full at its
last inversion; an incremental commit's df is that base plus the rows it
inverts (k_df_sum reads no kept row), and the rows that are full now join the
base.  TFIDF_DF_FROM_ROWS=1 sums the kept rows as before (A/B); the base is
kept up under either value.  k_df_sum<true> leaves the row scan's part totals
per workgroup (no atomics), which the forced shapes exercise on two-workgroup
rows with empty parts (test_gpu_inversion_slices has rows of 130 workgroups).

The helpers, documents (3-6 words over <= 400 terms) and block size of
test_gpu_incremental_inversion: every state is compared with a fresh
one-commit index of the same documents and with the CPU oracle, bit for bit, on
tfidf_stats, df of every term, all hits (k = 0) and the top 10 of every word
and a few multi-word queries.  Both snapshots are checked, so every change is
committed twice.  The base itself is not exported: a wrong base shows as a wrong
df in the commit that reads it, which is why each change is followed by a
commit that adds nothing (its df is the base plus the tail row, or the base
alone when the shard ends on a block edge).
"""
import random

import pytest

from tfidf_amd import _lib as L
from tfidf_amd import synth

from test_gpu_incremental_commit import add, keyed, published
from test_gpu_incremental_inversion import BLOCK, DOCS, TEXTS, commit_and_check, expect, twice

pytestmark = pytest.mark.gpu

KNOBS = ("TFIDF_TEST_INV_SLICES", "TFIDF_TEST_SCAN_PARTS")
SHAPES = [None, (7, 4)]                                    # the plan's own shape; forced slices and row parts


def force(monkeypatch, shape):
    for k, v in zip(KNOBS, shape or (None, None)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def both(g, docs, first_block, shape=None, **kw):
    """Commit into either snapshot; with a forced shape, the shape the inversion reports."""
    n_blocks = (len(docs) + BLOCK - 1) // BLOCK
    for _ in range(2):
        commit_and_check(g, docs, first_block, rows=False, **kw)
        if shape:
            want = shape if first_block < n_blocks else (1, 1)     # no block to invert: no tile kernel, no row scan
            assert g.commit_inversion_shape() == {"slices": want[0], "scan_parts": want[1]}


# a. the tail stays partial ---------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_partial_tail_grows_then_nothing_is_added(monkeypatch, shape):
    force(monkeypatch, shape)
    g = twice(DOCS[:16500])
    add(g, DOCS[16500:16700])
    both(g, DOCS[:16700], 2, shape, tokenized=200)               # base = blocks 0, 1; nothing folds
    both(g, DOCS[:16700], 2, shape, tokenized=0)
    g.close()


# b. the tail is filled exactly to a block edge --------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_tail_filled_to_the_block_edge(monkeypatch, shape):
    force(monkeypatch, shape)
    edge = 3 * BLOCK
    g = twice(DOCS[:16500])
    add(g, DOCS[16500:edge])
    both(g, DOCS[:edge], 2, shape, tokenized=edge - 16500)       # block 2 joins the base, once per snapshot
    both(g, DOCS[:edge], 3, shape, tokenized=0)                  # no row inverted: df is the base alone (twice: not folded again)
    add(g, DOCS[edge:edge + 1])
    both(g, DOCS[:edge + 1], 3, shape, tokenized=1)              # a one-document block behind the base
    g.close()


# c. one commit across two block edges ------------------------------------------

def test_commit_across_two_block_edges():
    g = twice(DOCS[:16500])
    add(g, DOCS[16500:25200])
    both(g, DOCS, 2, tokenized=8700)                             # rows 2 and 3 inverted; row 2 folds, the new tail does not
    both(g, DOCS, 3, tokenized=0)                                # base = blocks 0 .. 2, the tail row on top
    g.close()


# d. new terms: the base moves to the new columns with the kept rows ------------

@pytest.mark.parametrize("log2", [10, 17])
def test_new_terms_remap_the_base(log2):
    """50 words absent before, at hashed slots among the 400 old ones in 2^10 and 2^17 slots (that all 50 land
    behind the last old slot has a chance below 400^-50; tests/df_base_plan_check.cpp pins the between case).
    Their columns' base must be 0 and the old columns' unchanged: the commits after the remap read the base
    (df of every word, old and new, against the oracle), the second pair without a remap."""
    ctor = dict(vocab_capacity_log2=log2)
    rng = random.Random(50)
    fresh_words = [synth.word(1000 + j) for j in range(50)]
    later = [b" ".join([fresh_words[i % 50]] + [synth.word(rng.randint(1, 400)) for _ in range(rng.randint(2, 4))])
             for i in range(150)] + [fresh_words[3] + b" " + fresh_words[49]]
    docs = DOCS[:16500] + keyed(later, 16500)
    extra = [fresh_words[0] + b" " + synth.word(7), fresh_words[49] + b" " + fresh_words[3], fresh_words[10]]
    g = twice(DOCS[:16500], **ctor)
    add(g, docs[16500:])
    both(g, docs, 2, remapped=1, tokenized=len(later), extra_queries=extra, **ctor)
    both(g, docs, 2, remapped=0, tokenized=0, extra_queries=extra, **ctor)
    more = keyed(TEXTS[20000:20100], len(docs))                  # no new word
    add(g, more)
    both(g, docs + more, 2, remapped=0, tokenized=100, extra_queries=extra, **ctor)
    g.close()


# e. the A/B switches for one commit each ---------------------------------------

def test_full_inversion_and_df_from_rows_for_one_commit(monkeypatch):
    g = twice(DOCS[:16500])
    add(g, DOCS[16500:16700])
    monkeypatch.setenv("TFIDF_FULL_INVERSION", "1")
    commit_and_check(g, DOCS[:16700], 0, tokenized=200, rows=False)      # the base is rebuilt in the full pass
    monkeypatch.delenv("TFIDF_FULL_INVERSION")
    commit_and_check(g, DOCS[:16700], 2, tokenized=200, rows=False)      # the other snapshot: its own base
    commit_and_check(g, DOCS[:16700], 2, tokenized=0, rows=False)        # ... and the one the full inversion left
    add(g, DOCS[16700:16900])
    monkeypatch.setenv("TFIDF_DF_FROM_ROWS", "1")
    commit_and_check(g, DOCS[:16900], 2, tokenized=200, rows=False)      # df from the kept rows; the base is kept up
    monkeypatch.delenv("TFIDF_DF_FROM_ROWS")
    both(g, DOCS[:16900], 2)                                             # either snapshot's base again
    monkeypatch.setenv("TFIDF_DF_FROM_ROWS", "1")
    commit_and_check(g, DOCS[:16900], 2, tokenized=0, rows=False)
    g.close()


# f. a failed build, then a good one --------------------------------------------

def test_failed_build_leaves_no_base(monkeypatch):
    monkeypatch.setenv("TFIDF_PACK_DOCS", "1")
    ctor = dict(vocab_capacity_log2=10)
    g = twice(DOCS[:16500], **ctor)
    offender = (b"offender", b" ".join(synth.word(5000 + j) for j in range(700)))    # 400 + 700 > 2^10: an input error
    add(g, [offender])
    with pytest.raises(L.TfidfError) as err:
        g.commit()
    assert err.value.code == L.E_CAPACITY
    assert g.delete_documents([b"offender"]) == 1
    g.compact()
    commit_and_check(g, DOCS[:16500], 0, tokenized=16500, full=True, rows=False, **ctor)   # nothing kept, no base read
    commit_and_check(g, DOCS[:16500], 0, rows=False, **ctor)                               # the other snapshot
    add(g, DOCS[16500:16700])
    both(g, DOCS[:16700], 2, tokenized=200, **ctor)                                        # the rebuilt bases
    both(g, DOCS[:16700], 2, tokenized=0, **ctor)
    g.close()


# g. delete, a commit through live_map, a compaction, incremental again -----------

def test_delete_compact_then_incremental():
    drop = ("text_bytes", "dead_docs", "dead_bytes")             # a fresh index never held the dead text

    def check(first_block, docs, tokenized):
        n_blocks = (len(docs) + BLOCK - 1) // BLOCK
        assert g.commit_inverted_blocks() == {"first_block": first_block, "n_blocks": n_blocks, "remapped": 0}
        assert g.commit_tokenized_docs()["docs"] == tokenized
        e = expect(docs)
        assert {k: v for k, v in published(g).items() if k not in drop} == {k: v for k, v in e.stats.items() if k not in drop}
        e.check(g, first_block, stats=False, rows=False)

    g = twice(DOCS[:16500])
    assert g.delete_documents([DOCS[9000][0]]) == 1
    docs = DOCS[:9000] + DOCS[9001:16500]
    g.commit()                                                   # full, through live_map
    check(0, docs, 16499)
    g.compact()
    for _ in range(2):                                           # full: the epoch changed; both snapshots
        g.commit()
        check(0, docs, 16499)
    later = keyed(TEXTS[16500:16700], 20000)
    add(g, later)
    for tokenized in (200, 200, 0, 0):                           # incremental again over the rebuilt bases
        g.commit()
        check(2, docs + later, tokenized)
    g.close()
