"""The 255-unit token cut on every tokenizer path.  StandardAnalyzer cuts a
token at 255 UTF-16 units and rescans from the cut; the ASCII wave tokenizer,
its <UNI> instantiation, k_tokenize_uwave (sparse and full scan),
k_tokenize_chunk / <UNI>, k_tokenize_uchunk and k_tokenize_long each cut the
token themselves or hand the document to a path that does.

Every test commits one family of token_cut_ref.py (the table of over-long
runs crossed with the placements; test_token_cut_cpu.py holds each family to
the property it is named for) and asserts, for EVERY document, the terms, the
length and the norm against the CPU oracle; the collection statistics; all
hits of the cut term, the remainder term and the over-long query term; that no
hash seed was changed on the way (a false collision that another seed happens
to clear must not pass); and — from the documents alone, expected_paths —
which path took them: a test that cannot say so tests nothing.
"""
import pytest

import token_cut_ref as T
from tfidf_amd import _lib as L
from tfidf_amd.engine import ShardIndex

from test_gpu_parity import assert_hits_equal

pytestmark = pytest.mark.gpu

KNOBS = {
    "default": {},
    "nouniwave": {"TFIDF_NO_UNIWAVE": "1"},      # flagged documents and units: k_tokenize_uwave / k_tokenize_uchunk
    "nouchunk": {"TFIDF_NO_UCHUNK": "1"},        # a book with non-ASCII text: k_tokenize_long, whole
    "uwfull": {"TFIDF_UW_FULL": "1"},            # k_tokenize_uwave without its sparse form
}
PATHS = ("long_docs", "long_chunked", "unicode_docs", "unicode_wave_docs")


def commit(name, monkeypatch, env=(), **kw):
    for k, v in dict(env).items():
        monkeypatch.setenv(k, v)
    g = ShardIndex(**kw)
    g.add_documents(T.texts(name))
    g.commit()
    return g


def check_index(g, name):
    o, texts = T.oracle_index(name), T.texts(name)
    s = g.stats()
    assert (s["hash_rebuilds"], s["hash_seed"]) == (0, 0)
    assert s["malformed_docs"] == 0 and g.malformed_docs() == []
    assert (s["num_docs"], s["doc_count"], s["sum_ttf"], s["num_terms"], s["nnz"]) == \
        (len(texts), o.doc_count, o.sum_ttf, o.num_terms, sum(o.vocab().values()))
    for d in range(len(texts)):
        assert g.doc_terms(d) == o.doc_terms(d), (d, T.family(name)[d].tag, T.family(name)[d].runs)
        assert g.doc_len(d) == (o.doc_len(d), o.doc_norm(d)), d
    for q in T.queries(name):
        assert_hits_equal(g.search(q, 0), o.search(q, 0))


def paths(g):
    s = g.stats()
    return {k: s[k] for k in PATHS}


@pytest.mark.parametrize("cls,config,pack", [
    ("letters", "default", "1"), ("letters", "default", None), ("letters", "default", "6"),
    ("joiners", "default", "1"), ("joiners", "default", "6"),
    ("unicode", "default", "1"), ("unicode", "default", None), ("unicode", "nouniwave", "1"), ("unicode", "uwfull", "1"),
    ("unicode", "nouniwave", "6")])
def test_short_documents(monkeypatch, cls, config, pack):
    """Documents of at most 4 000 bytes: the wave paths.  An ASCII document
    with a token over 255 bytes leaves the wave tokenizer (one per wave, or
    packed: TFIDF_PACK_DOCS, where the whole pack is retried) for the long
    path; a non-ASCII one is cut by k_tokenize_uwave itself (sparse islands,
    full scan) unless the wave rules took it first — those measure bytes, so
    é x 200 goes to the long path too, where it must stay ONE token."""
    env = dict(KNOBS[config])
    if pack:
        env["TFIDF_PACK_DOCS"] = pack
    g = commit(cls, monkeypatch, env)
    check_index(g, cls)
    want = T.expected_paths(T.family(cls), "default" if config == "uwfull" else config)
    assert paths(g) == want
    s = g.stats()
    if pack == "1":
        assert s["pack_docs"] == 1 and s["pack_retried"] == 0
    else:
        # packed (None: the automatic size, kPackBytes = 2 560 over a mean of 600 to 900 bytes).  A pack
        # takes no non-ASCII document and no token over 255 bytes: it is retried one document per wave
        n = len(T.texts(cls))
        assert s["pack_docs"] > 1
        assert (s["pack_retried"] == n) if cls == "unicode" else (want["long_docs"] <= s["pack_retried"] <= n)
    g.close()


@pytest.mark.parametrize("name,config", [
    ("chunk_ascii", "default"),
    ("chunk_unicode", "default"), ("chunk_unicode", "nouniwave"), ("chunk_unicode", "nouchunk"),
    ("chunk_nosplit", "default"), ("chunk_nosplit", "nouniwave"), ("chunk_nosplit", "nouchunk"),
    ("cover", "default"), ("cover", "nouniwave"), ("cover", "nouchunk"),
    ("same_prefix", "default"), ("same_prefix", "nouniwave"), ("same_prefix", "nouchunk")])
def test_book_sized_documents(monkeypatch, name, config):
    """Documents of 4.2 to 8 KB: the chunk paths.  Every document is over 4 096
    bytes, so all start on the long list and none counts as non-ASCII; one
    that holds a cut never stays on the chunk path (long_chunked counts the
    others: expected_paths), whichever unit kernel meets the run — at the end
    of a core, inside the next unit's leading margin, across the end of the
    window's trailing margin, or covering a whole window."""
    g = commit(name, monkeypatch, KNOBS[config])
    check_index(g, name)
    want = T.expected_paths(T.family(name), config)
    assert want["long_docs"] == len(T.texts(name)) and want["unicode_docs"] == want["unicode_wave_docs"] == 0
    assert paths(g) == want
    g.close()


@pytest.mark.parametrize("config", ["default", "nouniwave"])
def test_same_prefix_in_several_chunk_groups(monkeypatch, config):
    """TFIDF_TEST_PAIR_UNITS=7: two or three documents of three units per
    chunk group, so k_tokenize_uchunk runs once per group with its table reset."""
    env = dict(KNOBS[config], TFIDF_TEST_PAIR_UNITS="7")
    for name in ("same_prefix", "chunk_unicode"):
        assert all(len(T.unit_windows(len(t))) >= 3 for t in T.texts(name))
        g = commit(name, monkeypatch, env)
        check_index(g, name)
        assert paths(g) == T.expected_paths(T.family(name), config)
        g.close()


def test_uni_first_recommit(monkeypatch):
    """A corpus of mostly non-ASCII documents committed twice: the second
    commit runs UNI-first (every document starts flagged; k_tokenize_wave<UNI>
    meets the ASCII runs, k_tokenize_uwave the book-sized documents)."""
    name = "unifirst"
    g = commit(name, monkeypatch, {"TFIDF_PACK_DOCS": "1"})
    check_index(g, name)
    want = T.expected_paths(T.family(name))
    s = g.stats()
    assert paths(g) == want
    assert s["pack_docs"] == 1 and want["unicode_docs"] * 2 > s["num_docs"]      # both conditions of UNI-first
    g.commit()
    check_index(g, name)
    assert paths(g) == want
    g.close()


@pytest.mark.parametrize("cap_log2,inversion", [(18, L.INVERSION_BLOCK), (18, L.INVERSION_TERM), (21, L.INVERSION_AUTO)],
                         ids=["block", "term", "g4"])
def test_mixed_corpus_both_inversions(monkeypatch, cap_log2, inversion):
    """Short and book-sized, ASCII and not, in one corpus: block-major and
    term-major rows, and the kernels' 4-slot-group instantiations (2^21 slots)."""
    g = commit("mixed", monkeypatch, {}, inversion=inversion, vocab_capacity_log2=cap_log2)
    check_index(g, "mixed")
    assert paths(g) == T.expected_paths(T.family("mixed"))
    g.close()


@pytest.mark.parametrize("mode", ["first", "unifirst", "nounifirst"])
def test_non_ascii_document_overflowing_the_window(monkeypatch, mode):
    """A non-ASCII document of at most 4 096 bytes whose staged window
    overflows (shift + L > 4 096; documents 1 and 2 of the family, the second
    with a run of 300 z).  The ASCII pass cannot stage it: it goes to the long
    list unflagged and uncounted.  A UNI-first commit leaves it flagged, and
    k_tokenize_uwave (whose window takes shift + 4 096 bytes) tokenizes and
    counts it: unicode_docs and long_docs differ by exactly one per such
    document between the two modes, and the index is the same."""
    name = "overflow"
    if mode == "nounifirst":
        monkeypatch.setenv("TFIDF_NO_UNIFIRST", "1")
    g = commit(name, monkeypatch)
    docs = T.family(name)
    n_over = sum(1 for d in docs if d.tag == "overflow")
    n_plain = len(docs) - n_over
    # first commit: the two documents on the long list; the one without a cut stays on the chunk path
    first = dict(long_docs=n_over, long_chunked=1, unicode_docs=n_plain, unicode_wave_docs=n_plain)
    assert g.stats()["pack_docs"] == 1 and n_over == 2
    check_index(g, name)
    assert paths(g) == first
    if mode != "first":
        g.commit()
        check_index(g, name)
        if mode == "nounifirst":
            assert paths(g) == first
        else:
            assert paths(g) == dict(long_docs=0, long_chunked=0, unicode_docs=n_plain + n_over,
                                    unicode_wave_docs=n_plain)
    g.close()
