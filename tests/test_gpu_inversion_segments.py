"""The block-major inversion's segment loads at their boundaries.

k_df_partial and k_scatter_part (csrc/kernels_index.hip) read a document's
CSR row segment in 16-byte pieces: sixteen lanes per document, four entries
per lane, 64 entries per load instruction, a follow-up loop for the rest, and
components at or past the segment's end masked to "no entry".  The corpora
below are the smallest at which that can go wrong: every segment length
around a lane's four words, the sixteen-lane edge and the follow-up loop; the
longest row first and last in the CSR buffer (the load that may run past the
last row); segments that start at any 4-byte offset (several ranges);
document counts that fill no round of any workgroup size; deleted documents
(live_map).  Each index is held against the CPU oracle on the same
documents: statistics, df of every term used, and the all-hits lists of
chosen terms with scores compared as float32 bit patterns.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tfidf_amd import _lib as L
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

pytestmark = pytest.mark.gpu

BOUNDARY_COUNTS = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 67, 127, 128, 129, 255, 256, 257]


def boundary_doc(n, first=1):
    """n distinct terms (synth ranks first .. first + n - 1), tf 1 .. 3."""
    return b" ".join(b" ".join([synth.word(first + j)] * (1 + j % 3)) for j in range(n)) + b"\n"


def boundary_docs(first=1):
    return [boundary_doc(n, first) for n in BOUNDARY_COUNTS] + [b"", b"_"]


def terms_of(texts):
    return sorted({t for x in texts for t in x.split()} - {b"_"})


def check_against_oracle(texts, cap_log2, queries, n_blocks=1, deleted=()):
    keys = [b"k%d" % i for i in range(len(texts))]
    dead = set(deleted)
    g = ShardIndex(vocab_capacity_log2=cap_log2, inversion=L.INVERSION_BLOCK)
    o = O.OracleIndex()
    try:
        g.add_documents(texts, keys)
        if dead:
            assert g.delete_documents([keys[i] for i in sorted(dead)]) == len(dead)
        g.commit()
        live = [i for i in range(len(texts)) if i not in dead]
        for i in live:
            o.add_doc(keys[i], texts[i])
        o.commit()
        s = g.stats()
        assert s["term_major"] == 0
        assert (s["num_docs"] + 8191) // 8192 == n_blocks
        assert (s["num_docs"], s["doc_count"], s["sum_ttf"], s["num_terms"]) == \
            (o.num_docs, o.doc_count, o.sum_ttf, o.num_terms)
        vocab = o.vocab()
        assert s["nnz"] == sum(vocab.values())
        used = terms_of([texts[i] for i in live])
        assert len(used) == o.num_terms
        bad = [(t, g.df(t)[0], vocab[t]) for t in used if g.df(t)[0] != vocab[t]]
        assert not bad, bad[:10]
        for q in queries:
            docs, scores = g.search_all_arrays(q)
            want = o.search(q, 0)
            assert len(want) == vocab.get(q, 0)
            assert docs.tolist() == [d for d, _ in want], q
            w = np.array([x for _, x in want], np.float32)
            assert np.array_equal(scores.view(np.int32), w.view(np.int32)), q
    finally:
        g.close()
        o.close()


# ---------------------------------------------------------------------------
# one range: a document's whole row is one segment

BOUNDARY_QUERIES = [synth.word(r) for r in (1, 2, 4, 5, 16, 17, 64, 65, 67, 128, 129, 256, 257)]


@pytest.mark.parametrize("longest", ["last", "first"])
def test_one_range_every_boundary_length(longest):
    docs = boundary_docs()
    long_doc = docs.pop(BOUNDARY_COUNTS.index(257))
    texts = docs + [long_doc] if longest == "last" else [long_doc] + docs
    check_against_oracle(texts, 16, BOUNDARY_QUERIES)


# ---------------------------------------------------------------------------
# several ranges: segments start anywhere inside a row

@pytest.fixture(scope="module")
def mixed_corpus():
    texts = synth.corpus(300) + boundary_docs()
    counts = {}
    for x in texts:
        for t in set(x.split()):
            counts[t] = counts.get(t, 0) + 1
    by_df = sorted(counts, key=lambda t: (-counts[t], t))
    rare = next(t for t in reversed(by_df) if counts[t] == 1)
    return texts, [by_df[0], by_df[len(by_df) // 2], rare] + BOUNDARY_QUERIES[:4]


def test_several_ranges(mixed_corpus):
    texts, queries = mixed_corpus
    check_against_oracle(texts, 18, queries)


def test_deleted_documents(mixed_corpus):
    texts, queries = mixed_corpus
    check_against_oracle(texts, 18, queries, deleted=range(0, len(texts), 7))


# ---------------------------------------------------------------------------
# block and round edges: two blocks, the second nearly empty

N_SHORT = 8192 + 5


@pytest.fixture(scope="module")
def short_corpus():
    def doc(i):
        w = [synth.word(1 + i % 50), synth.word(51 + i % 7)]
        if i % 3 == 0:
            w.append(synth.word(100 + i % 11))
        return b" ".join(w)
    return [doc(i) for i in range(N_SHORT)]


@pytest.mark.parametrize("threads", [None, "256", "512", "1024"])
def test_block_and_round_edges(short_corpus, threads, monkeypatch):
    # a round is 4 to 16 documents per wave (one to four quads): no workgroup
    # size's round, and no wave's share of one, divides the document count
    for waves in (4, 8, 16):
        for docs_per_wave in (4, 8, 12, 16):
            assert N_SHORT % (waves * docs_per_wave) and (N_SHORT - 8192) % docs_per_wave
    if threads:
        monkeypatch.setenv("TFIDF_PART_THREADS", threads)
    queries = [synth.word(r) for r in (1, 50, 51, 57, 100, 110)]
    check_against_oracle(short_corpus, 17, queries, n_blocks=2)
