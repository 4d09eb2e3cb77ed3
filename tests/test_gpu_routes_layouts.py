"""Every query route on other index layouts: the sweep of routes_ref.py (see
test_gpu_routes_incremental.py) on what the route tests never built -- a 2^21
and a 2^23-slot dictionary (32 ranges, the 4-slot probe groups, AUTO choosing
term-major, 23 / 14 / 19-bit term-major postings and a 9-bit CSR tf field), the
probe groups at high load, tf escapes inside route documents (511 in the scatter
temp word and the CSR, 2047 in a block-major posting, every tf >= 3 in a
term-major one), hash seeds other than 0 (set, met by a collision, and two
snapshots of one index under two seeds), indexes that were saved and loaded
(file versions 1 and 2) and BM25 parameters other than (1.2, 0.75).

Each case builds one index, asserts through the accessors that it reached its
configuration and then sweeps; nothing of the sweep is left out.  Its closing
comparison is with a default-layout one-commit index, so it also says that the
results do not depend on the layout.  The references of A0, A0 + new_batch() and
the list without documents 0, 4 and 13 are the ones test_gpu_routes_incremental.py
has built when the suite runs; test_routes_fixture_cpu.py holds HEAVY and the
(k1, b) references to their cases.
"""
import pytest

import routes_ref as RR
from routes_ref import APPEND_A, BASE, BLOCK, FIRST_A, HEAVY, HEAVY_A, HEAVY_B, expected, sweep
from tfidf_amd import _lib as L
from tfidf_amd.engine import ShardIndex

from test_gpu_delete_compact import HEADER
from test_gpu_incremental_commit import add, keyed
from test_gpu_routes_incremental import A0, A1, DOCS

pytestmark = pytest.mark.gpu

APPENDED = DOCS[FIRST_A:FIRST_A + APPEND_A]
DEAD = [0, 4, 13]                                        # as test_delete_compact_then_incremental
LIVE = [t for i, t in enumerate(A0) if i not in DEAD]


def built(docs, exp, **ctor):
    """An index of `docs` after one commit, a full one, which holds what `exp` was computed from."""
    g = ShardIndex(**ctor)
    add(g, docs)
    full_commit(g, exp)
    return g


def full_commit(g, exp):
    g.commit()
    assert g.commit_tokenized_docs() == {"docs": len(exp.texts), "was_full": True}
    s = g.stats()
    assert (s["num_docs"], s["num_terms"], s["malformed_docs"]) == (len(exp.texts), len(exp.vocab), 0)
    assert (len(exp.texts) + BLOCK - 1) // BLOCK == 2    # block 0 and a tail


def is_at(g, **want):
    s = g.stats()
    assert {k: s[k] for k in want} == want


# a. large dictionaries ------------------------------------------------------------------

@pytest.mark.parametrize("log2,inversion,term_major", [(21, L.INVERSION_BLOCK, 0), (21, L.INVERSION_TERM, 1),
                                                       (23, L.INVERSION_AUTO, 1)], ids=["21-block", "21-term", "23-auto"])
def test_large_dictionary(log2, inversion, term_major):
    exp = expected(A0)
    g = built(DOCS[:FIRST_A], exp, vocab_capacity_log2=log2, inversion=inversion)
    is_at(g, term_major=term_major, hash_seed=0, hash_rebuilds=0)
    sweep(g, exp)
    g.close()


# b. the 4-slot probe groups at high load ----------------------------------------------------

def test_probe_groups_at_high_load(monkeypatch):
    batch = RR.new_batch()
    exp = expected(A0 + batch)
    exp.fresh_arrays()                                   # the fresh index is a default one: before the knob is set
    monkeypatch.setenv("TFIDF_TEST_G4_BITS", "10")
    g = built(DOCS[:FIRST_A] + keyed(batch, FIRST_A), exp, vocab_capacity_log2=10)
    assert g.stats()["num_terms"] / 1024 >= 0.4
    is_at(g, term_major=0, hash_seed=0)
    sweep(g, exp)
    g.close()


# c. tf escapes inside route documents -----------------------------------------------------------

@pytest.mark.parametrize("ctor,knob,term_major", [
    ({}, None, 0),                                                              # temp word 511, posting 2047
    (dict(vocab_capacity_log2=23), None, 1),                                    # a 9-bit CSR tf field: 511
    (dict(vocab_capacity_log2=16, inversion=L.INVERSION_TERM), "2", 1),         # every tf >= 3 is a posting escape
], ids=["default", "23-auto", "16-term-tf2"])
def test_tf_escapes_in_route_documents(monkeypatch, ctor, knob, term_major):
    exp = expected(HEAVY, extra_route=[HEAVY_A, HEAVY_B])
    exp.fresh_arrays()
    if knob:
        monkeypatch.setenv("TFIDF_TEST_TERM_TF_BITS", knob)
    g = built(keyed(HEAVY), exp, **ctor)
    assert g.stats()["long_docs"] >= 2
    is_at(g, term_major=term_major, hash_seed=0)
    sweep(g, exp)
    g.close()


# d. hash seeds other than 0 -------------------------------------------------------------------------

def test_a_set_hash_seed():
    exp = expected(A0)
    g = ShardIndex()
    g.set_hash_attempt(2)
    add(g, DOCS[:FIRST_A])
    full_commit(g, exp)
    assert g.stats()["hash_seed"] != 0
    sweep(g, exp)
    g.close()


def test_a_seed_reached_by_a_collision(monkeypatch):
    batch = RR.new_batch()
    exp = expected(A0 + batch)
    exp.fresh_arrays()
    monkeypatch.setenv("TFIDF_TEST_WEAK_HASH", "1")      # LONG_TERM and N1: hashed keys of one length collide
    g = built(DOCS[:FIRST_A] + keyed(batch, FIRST_A), exp)
    is_at(g, hash_seed=1, hash_rebuilds=1)
    sweep(g, exp)
    g.close()


def test_two_snapshots_under_two_seeds():
    g = ShardIndex()
    add(g, DOCS[:FIRST_A])
    for _ in range(2):
        full_commit(g, expected(A0))
    is_at(g, hash_seed=0, hash_rebuilds=0)
    rd = g.reader()                                      # holds a seed-0 snapshot
    assert rd.num_docs == FIRST_A
    g.set_hash_attempt(2)
    add(g, APPENDED)
    for _ in range(2):                                   # the spare snapshot, then a new one beside the held one:
        full_commit(g, expected(A1))                     # full both times, the signature's seed differs
        assert g.stats()["hash_seed"] != 0
    sweep(rd, expected(A0))
    sweep(g, expected(A1))
    sweep(rd, expected(A0))
    rd.close()
    g.close()


# e. saved and loaded ------------------------------------------------------------------------------------

def version(path):
    with open(path, "rb") as f:
        return HEADER.unpack_from(f.read(HEADER.size))[1]


def append_and_sweep(h, texts, keys, exp):
    """Documents 8300..8499 behind a loaded index: the second commit finds its target built from the loaded
    documents and tokenizes the 200 alone."""
    n = len(exp.texts)
    h.add_documents(texts, keys)
    h.commit()
    assert h.commit_tokenized_docs() == {"docs": n, "was_full": True}           # the first build of the other snapshot
    h.commit()
    assert h.commit_tokenized_docs() == {"docs": APPEND_A, "was_full": False}
    assert h.commit_inverted_blocks()["first_block"] == 1 and h.stats()["num_docs"] == n
    sweep(h, exp)


def same_keys(a, b):
    (ka, oa), (kb, ob) = a.doc_keys(), b.doc_keys()
    return ka.tobytes() == kb.tobytes() and oa.tolist() == ob.tolist()


def test_loaded_version_1(tmp_path):
    path = str(tmp_path / "v1.idx")
    g = built(DOCS[:FIRST_A], expected(A0))
    g.save(path)
    assert version(path) == 1
    h = ShardIndex()
    h.load(path)
    full_commit(h, expected(A0))
    assert same_keys(g, h) and h.doc_key(FIRST_A - 1) == DOCS[FIRST_A - 1][0]
    g.close()
    sweep(h, expected(A0))
    append_and_sweep(h, [t for _, t in APPENDED], [k for k, _ in APPENDED], expected(A1))
    h.close()


def test_loaded_version_2_with_keyless_ordinals(tmp_path):
    path = str(tmp_path / "v2.idx")
    g = ShardIndex()
    g.add_documents(A0)
    assert g.delete_documents([b"%d" % i for i in DEAD]) == len(DEAD)
    g.compact()
    full_commit(g, expected(LIVE))
    is_at(g, compactions=1, dead_docs=0)
    g.save(path)
    assert version(path) == 2                            # the ordinals differ from the positions
    h = ShardIndex()
    h.load(path)
    full_commit(h, expected(LIVE))
    assert same_keys(g, h) and h.doc_key(0) == b"1" and h.doc_key(len(LIVE) - 1) == b"%d" % (FIRST_A - 1)
    g.close()
    sweep(h, expected(LIVE))
    more = BASE[FIRST_A:FIRST_A + APPEND_A]
    assert len(LIVE) > BLOCK                             # block 0 is full of loaded documents: kept
    append_and_sweep(h, more, None, expected(LIVE + more))
    assert h.doc_key(len(LIVE)) == b"%d" % FIRST_A       # ordinals go on behind the saved ones
    h.close()


# f. other BM25 parameters ---------------------------------------------------------------------------------

@pytest.mark.parametrize("k1,b", RR.BM25)
def test_other_bm25_parameters(k1, b):
    exp = expected(A0, k1, b)
    g = built(DOCS[:FIRST_A], exp, k1=k1, b=b)
    is_at(g, term_major=0, hash_seed=0)
    sweep(g, exp)
    g.close()
