"""The 4-slot-group dictionary probe ("G4", kernels_index.hip group_probe /
window_probe<16>) under the non-ASCII wave tokenizer, and packed windows with
non-ASCII members.

launch_tokenize_wave / launch_tokenize_wave_uni pick the G4 instantiations of
k_tokenize_wave for dictionaries of >= 2^21 slots (TFIDF_G4_BITS).  The other
modules build non-ASCII corpora at the default 2^18 slots only, and their G4
corpora are ASCII at a load of a few percent, so <false, true, true> never
ran under a test and the probe's overflow rules hardly did.  Here:

  B1  the simple-letter and prose corpora of test_gpu_uni_wave.py at 2^21
      slots (block-major, R = 32 ranges, and term-major) and at 2^23 slots
      (term-major, CSR escape 511), wave rules on and off; one term through
      the G4 probe, k_tokenize_uwave's probe and the query lookup; a
      UNI-first re-commit (one document per window forced: the mode's
      condition).  The other B1 cases leave the pack size to the build,
      which packs two documents per window for these corpora (mean length
      under 1 280 bytes); the flagged members of a pack still reach
      <false, true, true> one per window, so nothing is lost by that.
  B2  TFIDF_TEST_G4_BITS=10 on a 2^12-slot dictionary holding ~3 000 terms
      (load ~0.73: about 2.9 keys per 4-slot group, so by Poisson about one
      group in six holds five or more and overflows): "slots >= s" and the
      advance ((ps | 3) + 1) & dmask, on <false,true,false>,
      <false,true,true> and (TFIDF_PACK_DOCS=4) <true,true,false>.  At this
      load the build can also reach the advance's wrap at the table end (it
      needs the last group to overflow) and the 16-slot retry window; the
      test does not show that this corpus does.  The same corpus without
      the knob (the 2-slot kernels) must equal the oracle too: a difference
      names the probe, not the corpus.
  B3  TFIDF_PACK_DOCS 2, 5, 16 over short documents of which one in five
      holds non-ASCII text: the packed ASCII kernel flags single members of
      a pack, the UNI pass or k_tokenize_uwave picks them up.

Bar, every case: doc_count / sum_ttf / num_terms / nnz, every document's
terms, length and norm, the malformed list, and hits at k = 0 and k = 10 as
float32 bit patterns, all equal to the CPU oracle's (oracle/tfidf_oracle.c).
"""
import random

import pytest

from oracle import oracle as O
from tfidf_amd import _lib as L
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

from test_gpu_pack import BOUNDARY_DOCS
from test_gpu_parity import ALPHABET, assert_hits_equal
from test_gpu_uni_wave import DECLINE, JOIN, PROSE, SIMPLE, WORDS, doc, edge_docs, prose_edge_docs
from test_gpu_unicode_sparse import check

pytestmark = pytest.mark.gpu

BLOCK, TERM, AUTO = L.INVERSION_BLOCK, L.INVERSION_TERM, L.INVERSION_AUTO
LAYOUTS = [(21, BLOCK), (21, TERM), (23, AUTO)]
LAYOUT_IDS = ["2^21-block", "2^21-term", "2^23-auto"]


def oracle_of(texts):
    o = O.OracleIndex()
    for i, t in enumerate(texts):
        o.add_doc(str(i).encode(), t)
    o.commit()
    return o


def gpu_of(texts, cap_log2, inversion):
    g = ShardIndex(vocab_capacity_log2=cap_log2, inversion=inversion)
    g.add_documents(texts)
    g.commit()
    return g


def build_pair(texts, cap_log2, inversion):
    return gpu_of(texts, cap_log2, inversion), oracle_of(texts)


def check_queries(g, o, queries):
    for q in queries:
        qb = q.encode() if isinstance(q, str) else q
        for k in (0, 10):
            assert_hits_equal(g.search(qb, k), o.search(qb, k))


def assert_layout(g, cap_log2, inversion):
    want = {BLOCK: 0, TERM: 1, AUTO: 1 if cap_log2 > 21 else 0}[inversion]
    assert g.stats()["term_major"] == want


# --------------------------------------------------------------------------
# B1: real-size dictionaries

SIMPLE_QUERIES = ["café", "naïve", "über cool", "straße", "ελλάδα", "москва", "résumé déjà", "l'été", "a_1_é",
                  "CAFÉ", "Über", "中文", synth.word(5).decode() + " é", "é"]
PROSE_QUERIES = ["don’t", "l’été", "québec", "École", "rock’n’roll", "a·b", "3’4", "“quote”", "Über", "ΣΟΦΙΑ",
                 "o’neil", "wait", "naïve", "i’m"]


@pytest.fixture(scope="module")
def simple_corpus():
    """test_simple_non_ascii_docs_equal_oracle's corpus (same seed, same size)."""
    rng = random.Random(71)
    texts = edge_docs()
    texts += [doc(rng, rng.randint(20, 500), rng.randint(1, 8), WORDS + JOIN + SIMPLE) for _ in range(900)]
    texts += [doc(rng, rng.randint(20, 300), 1, DECLINE) for _ in range(150)]
    texts += synth.corpus(200, V=3000, len_min=50, len_max=400)     # pure ASCII
    rng.shuffle(texts)
    o = oracle_of(texts)
    yield texts, o
    o.close()


@pytest.fixture(scope="module")
def prose_corpus():
    """test_prose_docs_equal_oracle's corpus (same seed, same size)."""
    rng = random.Random(97)
    texts = prose_edge_docs()
    texts += [doc(rng, rng.randint(20, 500), rng.randint(1, 12), PROSE + WORDS + JOIN) for _ in range(900)]
    texts += [doc(rng, rng.randint(20, 300), 2, PROSE) + " 中文".encode() for _ in range(100)]
    texts += synth.corpus(200, V=3000, len_min=50, len_max=400)
    rng.shuffle(texts)
    o = oracle_of(texts)
    yield texts, o
    o.close()


@pytest.mark.parametrize("uniwave", [True, False])
@pytest.mark.parametrize("cap_log2,inversion", LAYOUTS, ids=LAYOUT_IDS)
def test_simple_non_ascii_docs_g4(monkeypatch, simple_corpus, cap_log2, inversion, uniwave):
    if not uniwave:
        monkeypatch.setenv("TFIDF_NO_UNIWAVE", "1")
    texts, o = simple_corpus
    assert len(texts) >= 1600                                         # (doc 1536 must exist: the round-6 failure)
    g = gpu_of(texts, cap_log2, inversion)
    assert_layout(g, cap_log2, inversion)
    st = g.stats()
    assert st["unicode_docs"] >= 900 + 150
    if uniwave:
        assert st["unicode_wave_docs"] >= 900                         # the simple ones went the wave way
        assert st["unicode_docs"] - st["unicode_wave_docs"] >= 150    # the declined ones did not
    else:
        assert st["unicode_wave_docs"] == 0
    check(g, o, texts)
    check_queries(g, o, SIMPLE_QUERIES)
    g.close()


@pytest.mark.parametrize("uniwave", [True, False])
@pytest.mark.parametrize("cap_log2,inversion", LAYOUTS, ids=LAYOUT_IDS)
def test_prose_docs_g4(monkeypatch, prose_corpus, cap_log2, inversion, uniwave):
    if not uniwave:
        monkeypatch.setenv("TFIDF_NO_UNIWAVE", "1")
    texts, o = prose_corpus
    assert len(texts) >= 1600
    g = gpu_of(texts, cap_log2, inversion)
    assert_layout(g, cap_log2, inversion)
    st = g.stats()
    if uniwave:
        assert st["unicode_wave_docs"] >= 900
        assert st["unicode_docs"] - st["unicode_wave_docs"] >= 100
    else:
        assert st["unicode_wave_docs"] == 0
    check(g, o, texts)
    check_queries(g, o, PROSE_QUERIES)
    g.close()


@pytest.mark.parametrize("inversion", [BLOCK, TERM], ids=["block", "term"])
def test_same_term_across_paths_g4(inversion):
    """One term inserted through the G4 probe (k_tokenize_wave<UNI>), found
    by k_tokenize_uwave's own probe (the document with Han) and by the query
    lookup: df 3 (the fourth document's "cafécafécafé" is another term), one
    posting list."""
    texts = [b"caf\xc3\xa9 au lait", "CAFÉ noir 中".encode(), "Café crème".encode(), "café".encode() * 3]
    g, o = build_pair(texts, 21, inversion)
    st = g.stats()
    assert st["unicode_wave_docs"] >= 2 and st["unicode_docs"] - st["unicode_wave_docs"] >= 1
    check(g, o, texts)
    assert g.df("café".encode())[0] == o.vocab()["café".encode()] == 3
    check_queries(g, o, ["café", "CAFÉ noir", "cafécafécafé", "crème lait"])
    g.close()
    o.close()


def test_uni_first_recommit_g4(monkeypatch, prose_corpus):
    """The prose corpus is mostly non-ASCII, so its re-commit runs UNI-first:
    <false, true, true> takes the ASCII documents too and inserts every term
    of the corpus.  The mode needs one document per window on both commits
    (tfidf_capi.hip: ix->uni_first = pack == 1 && unicode_docs * 2 > N); the
    many short edge documents would make the automatic choice pack two, so
    the pack size is forced to 1."""
    monkeypatch.setenv("TFIDF_PACK_DOCS", "1")
    texts, o = prose_corpus
    g = gpu_of(texts, 21, BLOCK)
    st1 = g.stats()
    # both conditions of the UNI-first mode for the next commit
    assert st1["pack_docs"] == 1 and st1["unicode_docs"] * 2 > st1["num_docs"] == len(texts)
    check(g, o, texts)
    g.commit()
    st2 = g.stats()
    assert st2["pack_docs"] == 1
    check(g, o, texts)
    for k in ("unicode_docs", "unicode_wave_docs", "long_docs", "nnz", "num_terms"):
        assert st1[k] == st2[k], k
    check_queries(g, o, PROSE_QUERIES)
    g.close()


# --------------------------------------------------------------------------
# B2: G4 at high load (2^12 slots, TFIDF_TEST_G4_BITS=10)

def high_load_vocab():
    """~3 000 distinct terms, half of them non-ASCII: pool words, short
    generated ones (<= 8 bytes: short table keys), long ones (> 8 bytes:
    folded, exact 128-bit keys) and very long ones (> 14 bytes: hashed keys,
    the verifying lookup); the other half synth.word ASCII terms."""
    uni = [w for w in WORDS + SIMPLE]
    for i in range(560):
        uni.append("%s%d" % (SIMPLE[i % 12], i))                     # é0 .. : 3 to 5 bytes (2-byte letters)
    for i in range(560):
        uni.append("größe%dmaß" % i)                                  # 13 to 15 bytes
    for i in range(150):
        uni.append("ελλάδα%dмосква" % i)                              # > 24 bytes: hashed
    for i in range(200):
        uni.append("%dé" % i)                                         # a digit first
    asc = [synth.word(r).decode() for r in range(1, 1451)]
    asc += ["longasciiword%d" % i for i in range(50)]                 # > 8 bytes: folded ASCII keys
    return uni, asc


def high_load_docs(rng, len_lo, len_hi, n_extra):
    """Every vocabulary term at least once (dealt out over the documents),
    then random documents; two in five documents are pure ASCII (the ASCII
    pass's probe inserts their terms), the rest mix both halves."""
    uni, asc = high_load_vocab()
    deal_u, deal_a = uni[:], asc[:]
    rng.shuffle(deal_u)
    rng.shuffle(deal_a)
    texts = []
    while deal_u or deal_a or n_extra > 0:
        n = rng.randint(len_lo, len_hi)
        pure = len(texts) % 5 < 2
        words = []
        for _ in range(n):
            if deal_a and (pure or not deal_u or rng.random() < 0.5):
                words.append(deal_a.pop())
            elif deal_u and not pure:
                words.append(deal_u.pop())
            else:
                words.append(rng.choice(asc if pure or rng.random() < 0.5 else uni))
        if not (deal_u or deal_a):
            n_extra -= 1
        texts.append(" ".join(words).encode())
    return texts


@pytest.fixture(scope="module")
def high_load():
    texts = high_load_docs(random.Random(2101), 20, 200, 60)
    texts += [("中文 " + "é12 größe7maß " + synth.word(3).decode()).encode()] * 3      # k_tokenize_uwave's lookup
    o = oracle_of(texts)
    yield texts, o
    o.close()


@pytest.fixture(scope="module")
def high_load_short():
    texts = high_load_docs(random.Random(2102), 1, 12, 400)          # short documents: packed windows
    o = oracle_of(texts)
    yield texts, o
    o.close()


HIGH_LOAD_QUERIES = ["é12", "ş7", "größe7maß", "ελλάδα7москва", "7é", "café straße", synth.word(3).decode(),
                     "longasciiword7 é552", synth.word(1450).decode() + " größe559maß", "ß531", "中文"]


def assert_high_load(o):
    # the test is about a nearly full table: it must not silently run at low load
    assert 2700 <= o.num_terms <= 3300, o.num_terms
    vocab = o.vocab()
    n_uni = sum(1 for t in vocab if any(b >= 0x80 for b in t))
    assert 0.4 * len(vocab) <= n_uni <= 0.6 * len(vocab), (n_uni, len(vocab))
    assert any(len(t) <= 8 for t in vocab if any(b >= 0x80 for b in t))
    assert any(len(t) > 8 for t in vocab if any(b >= 0x80 for b in t))


@pytest.mark.parametrize("g4", [True, False], ids=["g4", "g2"])
@pytest.mark.parametrize("inversion", [BLOCK, TERM], ids=["block", "term"])
def test_high_load_dictionary(monkeypatch, high_load, inversion, g4):
    monkeypatch.setenv("TFIDF_PACK_DOCS", "1")                       # one document per window (AUTO packs these)
    if g4:
        monkeypatch.setenv("TFIDF_TEST_G4_BITS", "10")
    texts, o = high_load
    assert_high_load(o)
    g = gpu_of(texts, 12, inversion)
    st = g.stats()
    assert st["pack_docs"] == 1 and st["unicode_wave_docs"] > len(texts) // 3
    check(g, o, texts)
    vocab = o.vocab()
    for t in sorted(vocab):                                           # every term found where it was inserted
        assert g.df(t)[0] == vocab[t], t
    check_queries(g, o, HIGH_LOAD_QUERIES)
    g.close()


@pytest.mark.parametrize("g4", [True, False], ids=["g4", "g2"])
def test_high_load_dictionary_packed(monkeypatch, high_load_short, g4):
    monkeypatch.setenv("TFIDF_PACK_DOCS", "4")
    if g4:
        monkeypatch.setenv("TFIDF_TEST_G4_BITS", "10")
    texts, o = high_load_short
    assert_high_load(o)
    assert max(len(t) for t in texts) <= 400
    g = gpu_of(texts, 12, BLOCK)
    assert g.stats()["pack_docs"] == 4
    check(g, o, texts)
    vocab = o.vocab()
    for t in sorted(vocab):
        assert g.df(t)[0] == vocab[t], t
    check_queries(g, o, HIGH_LOAD_QUERIES)
    g.close()


# --------------------------------------------------------------------------
# B3: packs with flagged members

FLAGGED = (["café", "naïve tail", "head über", "l'été", "é", "straße " * 20] +            # simple letters
           ["don’t", "“quote”", "a—b", "École", "non\u00a0breaking", "wait…"] +              # prose
           DECLINE)                                                                         # k_tokenize_uwave


def pack_docs(pack):
    rng = random.Random(1000 + pack)
    flagged = [f.encode() for f in FLAGGED]

    def plain():
        if rng.random() < 0.5:
            return "".join(rng.choice(ALPHABET) for _ in range(rng.randint(1, 240))).encode()
        return b" ".join(synth.word(rng.randint(1, 500)) for _ in range(rng.randint(1, 40)))

    texts = []
    for i in range(6 * pack):                                         # the first member of a pack
        texts.append(flagged[i % len(flagged)] if i % pack == 0 else plain())
    for i in range(6 * pack):                                         # the last member
        texts.append(flagged[(i + 3) % len(flagged)] if i % pack == pack - 1 else plain())
    for i, b in enumerate(BOUNDARY_DOCS):                             # joiners at a boundary with a flagged neighbour
        texts += [b, flagged[i % len(flagged)], b]
    for i in range(900):                                              # about one in five, anywhere
        texts.append(rng.choice(flagged) + b" " + synth.word(rng.randint(1, 500)) if rng.random() < 0.2 else plain())
    while len(texts) % pack != 0:
        texts.append(plain())
    texts.append("seul café".encode())                                # alone in the last pack
    assert all(1 <= len(t) <= 240 for t in texts)
    return texts


@pytest.mark.parametrize("uniwave", [True, False])
@pytest.mark.parametrize("pack", [2, 5, 16])
def test_packs_with_flagged_members(monkeypatch, pack, uniwave):
    monkeypatch.setenv("TFIDF_PACK_DOCS", str(pack))
    if not uniwave:
        monkeypatch.setenv("TFIDF_NO_UNIWAVE", "1")
    texts = pack_docs(pack)
    n_flagged = sum(1 for t in texts if any(b >= 0x80 for b in t))
    assert 0.15 * len(texts) <= n_flagged <= 0.35 * len(texts)
    g, o = build_pair(texts, 18, AUTO)
    st = g.stats()
    assert st["pack_docs"] == pack
    assert st["unicode_docs"] == n_flagged
    if not uniwave:
        assert st["unicode_wave_docs"] == 0
    check(g, o, texts)
    check_queries(g, o, ["café", "seul", "don’t", "École", "中文", "über", "abc", "def", "x_", "don't", "1,2",
                         synth.word(7).decode(), "a", "b.c x"])
    g.close()
    o.close()
