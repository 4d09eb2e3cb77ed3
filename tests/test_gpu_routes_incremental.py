"""Every query route on incrementally committed indexes: the sweep of
routes_ref.py (batched scorer, phrases and sloppy phrases, wildcard, regex,
fuzzy lookup / expansion / search, more-like-this, matches, snippets, doc_text;
each against its CPU reference, exactly, and the *_arrays forms against a fresh
one-commit index) on the states test_gpu_incremental_inversion, test_gpu_df_base
and test_gpu_fused_tail reach: kept blocks, kept blocks moved to new columns,
commits that add nothing, a lone tail block built in one launch beside a
snapshot built without it, term-major, a compaction, a held reader.

The routes read what tfidf_term_df and the single-query scorer do not: the
per-slot device df (fuzzy, wildcard, regex, more-like-this), the kept forward
rows (more-like-this), every block's offset rows and bitmaps (wildcard, regex),
the device text behind hashed terms and behind the phrase rescan.  Every state
is committed into both snapshots and swept on both, and says which state it is
through the commit accessors, predicted by the rules of the tests named above.
test_routes_fixture_cpu.py holds the corpus to the cases it was built for.
"""
import pytest

import routes_ref as RR
from routes_ref import APPEND_A, BASE, BLOCK, END_B, FIRST_A, FIRST_B, expected, sweep
from tfidf_amd import _lib as L
from tfidf_amd.engine import ShardIndex

from test_gpu_df_base import force
from test_gpu_fused_tail import predicted
from test_gpu_incremental_commit import add, keyed

pytestmark = pytest.mark.gpu

DOCS = keyed(BASE)
A0, A1 = BASE[:FIRST_A], BASE[:FIRST_A + APPEND_A]
SHAPES = [None, (3, None), (7, 4)]                       # the plan's own; three slices in one launch; sliced, split row scan


def twice(docs, **ctor):
    """Both snapshots built from `docs`: each one's first build is a full one."""
    g = ShardIndex(**ctor)
    add(g, docs)
    for _ in range(2):
        g.commit()
        assert g.commit_tokenized_docs() == {"docs": len(docs), "was_full": True}
        assert g.commit_inverted_blocks()["first_block"] == 0
    return g


def commit(g, n_docs, first_block, tokenized, remapped=0, full=False, shape=None, fused=None):
    """One commit, and what it must report: blocks [first_block, n_blocks) inverted, `tokenized` documents
    tokenized, the forced shape (none where no block was inverted), one launch exactly where fuse_plan says."""
    g.commit()
    n_blocks = (n_docs + BLOCK - 1) // BLOCK
    assert g.commit_inverted_blocks() == {"first_block": first_block, "n_blocks": n_blocks, "remapped": remapped}
    assert g.commit_tokenized_docs() == {"docs": tokenized, "was_full": full}
    if shape:
        slices, parts = shape if first_block < n_blocks else (1, 1)
        got = g.commit_inversion_shape()
        assert got["slices"] == slices and (parts is None or got["scan_parts"] == parts)
    assert g.commit_inversion_fused() is predicted(g)
    if fused is not None:
        assert g.commit_inversion_fused() is fused
    assert g.stats()["num_docs"] == n_docs


def grown(shape=None, **ctor):
    """8300 documents in both snapshots, 200 more in both: block 0 kept, the tail built (not swept)."""
    g = twice(DOCS[:FIRST_A], **ctor)
    add(g, DOCS[FIRST_A:FIRST_A + APPEND_A])
    for _ in range(2):
        commit(g, len(A1), 1, APPEND_A, shape=shape)
    return g


# a. a kept block, a grown tail, no new word -----------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=["plan", "fused3", "sliced7x4"])
def test_kept_block_and_grown_tail(monkeypatch, shape):
    force(monkeypatch, shape)
    fused = None if shape is None else shape[1] is None
    g = twice(DOCS[:FIRST_A])
    add(g, DOCS[FIRST_A:FIRST_A + APPEND_A])
    for _ in range(2):                                   # either snapshot
        commit(g, len(A1), 1, APPEND_A, shape=shape, fused=fused)
        sweep(g, expected(A1))
    g.close()


# b. nothing added: the per-slot df stands ---------------------------------------

def test_commits_that_add_nothing():
    g = grown()
    for _ in range(2):
        commit(g, len(A1), 1, 0)
        sweep(g, expected(A1))
    g.close()


# c. new words: the kept block's columns move -------------------------------------

@pytest.mark.parametrize("log2", [10, 17])
def test_new_words_remap_the_kept_block(log2):
    ctor = dict(vocab_capacity_log2=log2)
    batch = RR.new_batch()
    texts = A0 + batch
    g = twice(DOCS[:FIRST_A], **ctor)
    add(g, keyed(batch, FIRST_A))
    for _ in range(2):                                   # each snapshot moves its own kept rows
        commit(g, len(texts), 1, APPEND_A, remapped=1)
        sweep(g, expected(texts))
    more = BASE[FIRST_A + APPEND_A:FIRST_A + APPEND_A + 100]          # no new word
    add(g, keyed(more, len(texts)))
    texts = texts + more
    for _ in range(2):
        commit(g, len(texts), 1, 100)
        sweep(g, expected(texts))
    g.close()


# d. two kept blocks, one commit across a block edge -------------------------------

def test_two_kept_blocks_and_a_commit_across_the_block_edge():
    texts = BASE[:END_B]
    assert END_B == 3 * BLOCK + 1 and texts[-1] == RR.P_FULL         # a phrase document alone in block 3
    g = twice(DOCS[:FIRST_B])
    add(g, DOCS[FIRST_B:END_B])
    for _ in range(2):
        commit(g, END_B, 2, END_B - FIRST_B, remapped=1)             # block 2 fills and joins the df base; N2 is new
        sweep(g, expected(texts))
    commit(g, END_B, 3, 0)                                           # nothing added: the one-document block again
    sweep(g, expected(texts))
    g.close()


# e. one snapshot built in one launch, the other by the separate kernels -------------

def test_fused_beside_unfused_snapshot(monkeypatch):
    force(monkeypatch, (3, None))
    g = twice(DOCS[:FIRST_A])
    add(g, DOCS[FIRST_A:FIRST_A + APPEND_A])
    monkeypatch.setenv("TFIDF_INV_UNFUSED", "1")
    commit(g, len(A1), 1, APPEND_A, shape=(3, None), fused=False)
    sweep(g, expected(A1))
    monkeypatch.delenv("TFIDF_INV_UNFUSED")
    commit(g, len(A1), 1, APPEND_A, shape=(3, None), fused=True)     # the other snapshot
    sweep(g, expected(A1))
    commit(g, len(A1), 1, 0, shape=(3, None), fused=True)            # one launch over what the separate kernels left
    sweep(g, expected(A1))
    g.close()


# f. term-major: rows kept, everything inverted; the routes read toff / tdf ------------

def test_term_major():
    ctor = dict(inversion=L.INVERSION_TERM)
    g = twice(DOCS[:FIRST_A], **ctor)
    add(g, DOCS[FIRST_A:FIRST_A + APPEND_A])
    for _ in range(2):
        commit(g, len(A1), 0, APPEND_A, fused=False)
        assert g.stats()["term_major"] == 1
        sweep(g, expected(A1))
    g.close()


# g. delete, commit, compact, then incremental again ---------------------------------

def test_delete_compact_then_incremental():
    dead = [0, 4, 13]                                    # document 0; block 0's LONG_TERM; one "zorblet"
    assert BASE[4] == RR.HASH and BASE[8296] == RR.HASH and BASE[13].startswith(RR.FUZ[1])
    live = [d for i, d in enumerate(DOCS[:FIRST_A]) if i not in dead]
    texts = [t for _, t in live]
    g = twice(DOCS[:FIRST_A])
    assert g.delete_documents([DOCS[i][0] for i in dead]) == len(dead)
    commit(g, len(texts), 0, len(texts), full=True)      # a full build through live_map
    sweep(g, expected(texts))
    g.compact()
    for _ in range(2):                                   # the staged ids moved: full, both snapshots
        commit(g, len(texts), 0, len(texts), full=True)
        sweep(g, expected(texts))
    add(g, DOCS[FIRST_A:FIRST_A + APPEND_A])
    texts = texts + BASE[FIRST_A:FIRST_A + APPEND_A]
    assert len(texts) - APPEND_A > BLOCK                 # block 0 is full of live documents: kept
    for _ in range(2):
        commit(g, len(texts), 1, APPEND_A)
        sweep(g, expected(texts))
    g.close()


# h. a reader across the append --------------------------------------------------------

def test_a_reader_across_the_append():
    g = twice(DOCS[:FIRST_A])
    rd = g.reader()
    assert rd.num_docs == FIRST_A
    add(g, DOCS[FIRST_A:FIRST_A + APPEND_A])
    commit(g, len(A1), 1, APPEND_A)                      # the snapshot the reader does not hold
    commit(g, len(A1), 0, len(A1), full=True)            # the held one cannot be the target: a new snapshot, in full
    sweep(rd, expected(A0))
    sweep(g, expected(A1))
    with g.reader() as now:
        sweep(now, expected(A1))
    sweep(rd, expected(A0))
    rd.close()
    g.close()
