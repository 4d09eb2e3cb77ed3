"""Term frequencies on and next to the escape value of every packed tf field.

Each packed word of the build keeps tf in a narrow field whose all-ones value
E means "look the exact value up in an escape list".  For every field, one
document holds three different terms with tf E - 1, E and E + 1 (the first
stored in place, the other two escaped: `>=` against `>`, `min(tf, E)` against
`== E`), next to ordinary terms, and one document shares all those terms at
tf 1, so each has a posting on either side of the escape.

Documents: wave-window documents (<= 4 096 bytes, 1-byte terms; with the
2-byte letters é ü ñ so the non-ASCII wave pass writes the escape too; those
of 2 046 to 2 048 repeats hold more tokens than a wave window takes and go by
the book path), a book that takes the chunk path (k_tokenize_chunk +
k_long_rows: tf 65 536 is also the first value a 16-bit counter there would
wrap at) and a book with a token of more than 255 characters, which
k_tokenize_long takes whole.

Layouts: block-major at 2^18 slots (CSR escape 65 535, R = 4 ranges) and at
2^12 slots (range_shift 12: the CSR field holds 2^20 - 1, so only 511 and
2 047 are live); term-major at 2^18 (16 383), at 2^23 (511) and at 2^18 with
the sort word squeezed to 4 tf bits (15).

Bar: every document's terms and lengths, DF, the index statistics and hits
(k = 0 and 10, float32 bit patterns) equal the CPU oracle's, and the boundary
tfs equal the counts the corpus was built with; again after save / load into
a fresh index.

Out of scope here: the kMaxTf limit (2^24 - 1, tfidf_common.h), which needs
a single document of 33 MB; test_gpu_capacity.py pins it on both sides
(test_tf_at_and_past_the_limit).
"""
import collections
import random

import pytest

from oracle import oracle as O
from tfidf_amd import _lib as L
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

from test_gpu_parity import assert_hits_equal, index_stats

pytestmark = pytest.mark.gpu

BLOCK, TERM = L.INVERSION_BLOCK, L.INVERSION_TERM

# The escape values, each from its definition in csrc/:
TMP_TF_ESC = 511                 # kernels_index.hip kTmpTfEsc = 2^(32 - kTmpTfShift) - 1: block-major scatter temp word
POST_TF_ESC = 2047               # tfidf_internal.h kPostTfEsc: block-major posting (post_word)
RANGE_BITS = 16                  # tfidf_common.h kRangeBits: block-major CSR rows keep slot - range base
WAVE_TOKENS = 1024               # kernels_index.hip kWaveTokens: tokens of a document the wave tokenizers take


def csr_esc(term_major, cap_log2):
    """tfidf_internal.h csr_esc_value(range_shift) = 0xFFFFFFFF >> range_shift;
    range_shift = log2 C for term-major rows, min(log2 C, kRangeBits) for
    block-major ones (tfidf_capi.hip, "CSR rows are grouped by dictionary range")."""
    return 0xFFFFFFFF >> (cap_log2 if term_major else min(cap_log2, RANGE_BITS))


BLOCK_CSR_ESC = csr_esc(False, 18)        # 65 535
TERM_CSR_ESC_18 = csr_esc(True, 18)       # 16 383
TERM_CSR_ESC_23 = csr_esc(True, 23)       # 511
TERM_SORT_BITS = 4                        # TFIDF_TEST_TERM_TF_BITS below (tfidf_capi.hip tp.tf_bits)
TERM_SORT_ESC = (1 << TERM_SORT_BITS) - 1  # kernels_term.hip: the sort word's tf field, all ones

assert (BLOCK_CSR_ESC, TERM_CSR_ESC_18, TERM_CSR_ESC_23, TERM_SORT_ESC) == (65535, 16383, 511, 15)
assert csr_esc(False, 12) == (1 << 20) - 1                  # 2^12 slots, block-major: out of a book's reach

# Every escape value a layout below has: the book carries them all.
LEVELS = sorted({TERM_SORT_ESC, TMP_TF_ESC, TERM_CSR_ESC_23, POST_TF_ESC, TERM_CSR_ESC_18, BLOCK_CSR_ESC})
assert LEVELS == [15, 511, 2047, 16383, 65535]
# the book's boundary terms: level i, tf E - 1 / E / E + 1 -> one letter each
BOOK_TERMS = {(E, j): bytes([ord("a") + 3 * i + j]) for i, E in enumerate(LEVELS) for j in range(3)}
ORDINARY = [synth.word(r) for r in range(1, 301)]           # 4-letter words: none is a boundary term


def shuffled(rng, counts, n_ordinary):
    toks = [t for t, n in counts.items() for _ in range(n)]
    toks += [rng.choice(ORDINARY) for _ in range(n_ordinary)]
    rng.shuffle(toks)
    return toks


def make_corpus():
    """(texts, expected): expected[d] = {boundary term: tf} as built."""
    rng = random.Random(65535)
    texts, expected = [], []

    def add(toks, counts):
        texts.append(b" ".join(toks))
        expected.append(dict(counts))

    # the book: every level through the chunk path
    book = {BOOK_TERMS[E, j]: E - 1 + j for E in LEVELS for j in range(3)}
    add(shuffled(rng, book, 20000), book)
    # the same tfs in a book the chunk path cannot take: a token of > 255 characters
    toks = shuffled(rng, book, 20000)
    toks.insert(len(toks) // 2, b"q" * 300)
    add(toks, book)
    # wave-window documents, 1-byte terms.  The wave tokenizers take a document
    # of at most 1 024 tokens (kernels_index.hip kWaveTokens), so 510 + 511
    # repeats share one document of exactly 1 024 tokens and 512 has its own
    c = {b"a": TERM_SORT_ESC - 1, b"b": TERM_SORT_ESC, b"c": TERM_SORT_ESC + 1}
    add(shuffled(rng, c, 40), c)
    c = {b"a": TMP_TF_ESC - 1, b"b": TMP_TF_ESC}
    add(shuffled(rng, c, WAVE_TOKENS - sum(c.values())), c)
    c = {b"c": TMP_TF_ESC + 1}
    add(shuffled(rng, c, 40), c)
    # 2 047: 2 046, 2 047 and 2 048 repeats fill a window each (4 091, 4 093,
    # 4 095 bytes); with more than 1 024 tokens they go by the book path's units
    for t, n in ((b"d", POST_TF_ESC - 1), (b"e", POST_TF_ESC), (b"f", POST_TF_ESC + 1)):
        add([t] * n, {t: n})
        assert len(texts[-1]) == 2 * n - 1 <= 4096
    # 511 with 2-byte letters: the non-ASCII wave pass writes these rows
    c = {"é".encode(): TMP_TF_ESC - 1, "ü".encode(): TMP_TF_ESC}
    add(shuffled(rng, c, WAVE_TOKENS - sum(c.values())), c)
    c = {"ñ".encode(): TMP_TF_ESC + 1}
    add(shuffled(rng, c, 40), c)
    # every boundary term once: df 2 or more, a posting below the escape
    ones = {t: 1 for e in expected for t in e}
    add(shuffled(rng, ones, 40), ones)
    add([rng.choice(ORDINARY) for _ in range(50)], {})
    assert all(len(t) <= 4096 for t in texts[2:])
    assert all(500_000 <= len(t) <= 700_000 for t in texts[:2])
    return texts, expected


@pytest.fixture(scope="module")
def corpus():
    texts, expected = make_corpus()
    o = O.OracleIndex()
    for i, t in enumerate(texts):
        o.add_doc(str(i).encode(), t)
    o.commit()
    # the oracle agrees with the counts the corpus was built with
    for d, e in enumerate(expected):
        got = o.doc_terms(d)
        for t, n in e.items():
            assert got[t] == n, (d, t)
    yield texts, expected, o
    o.close()


def build(texts, inversion, cap_log2):
    g = ShardIndex(vocab_capacity_log2=cap_log2, inversion=inversion)
    g.add_documents(texts)
    g.commit()
    return g


def check_all(g, o, texts, expected):
    s = g.stats()
    assert (s["doc_count"], s["sum_ttf"], s["num_terms"], s["nnz"]) == \
        (o.doc_count, o.sum_ttf, o.num_terms, sum(o.vocab().values()))
    # the book path: the two books and the three documents of more than 1 024
    # tokens; all by their chunk units but the book with the long token
    assert s["long_docs"] == 5 and s["long_chunked"] == 4
    assert s["unicode_wave_docs"] == 3                      # é ü / ñ / the tf-1 document: by the wave rules
    for d in range(len(texts)):
        got = g.doc_terms(d)
        for t, n in expected[d].items():
            assert got.get(t) == n, (d, t, got.get(t), n)
        assert got == o.doc_terms(d), d
        assert g.doc_len(d) == (o.doc_len(d), o.doc_norm(d)), d
    vocab = o.vocab()
    df = collections.Counter(t for e in expected for t in e)
    terms = sorted(df)
    for t in terms:
        assert g.df(t)[0] == vocab[t] == df[t], t
    queries = terms + [a + b" " + b for a, b in zip(terms, terms[1:])] + \
        [b"o n", b"m AND o", "é ü ñ".encode(), b"q" * 255, ORDINARY[0] + b" o"]
    for q in queries:
        for k in (0, 10):
            assert_hits_equal(g.search(q, k), o.search(q, k))


CASES = [(BLOCK, 18, None), (BLOCK, 12, None), (TERM, 18, None), (TERM, 23, None), (TERM, 18, TERM_SORT_BITS)]
CASE_IDS = ["block-2^18", "block-2^12", "term-2^18", "term-2^23", "term-2^18-tf4"]


@pytest.mark.parametrize("inversion,cap_log2,tf_bits", CASES, ids=CASE_IDS)
def test_tf_on_and_next_to_the_escape_values(monkeypatch, corpus, inversion, cap_log2, tf_bits):
    if tf_bits:
        monkeypatch.setenv("TFIDF_TEST_TERM_TF_BITS", str(tf_bits))
    texts, expected, o = corpus
    g = build(texts, inversion, cap_log2)
    assert g.stats()["term_major"] == (1 if inversion == TERM else 0)
    check_all(g, o, texts, expected)
    g.close()


@pytest.mark.parametrize("inversion,cap_log2", [(BLOCK, 18), (TERM, 18)], ids=["block-2^18", "term-2^18"])
def test_escapes_after_save_and_load(tmp_path, corpus, inversion, cap_log2):
    texts, expected, o = corpus
    g = build(texts, inversion, cap_log2)
    path = str(tmp_path / "tf.tfidf")
    g.save(path)
    h = ShardIndex(vocab_capacity_log2=cap_log2, inversion=inversion)
    h.load(path)
    h.commit()
    assert index_stats(h) == index_stats(g)
    g.close()
    check_all(h, o, texts, expected)
    h.close()
