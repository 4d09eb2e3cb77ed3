"""The full dictionary, failed commits and the 2^24 - 1 tf limit.

The other modules only ever make a build succeed, at a dictionary load of at
most 0.73 (test_gpu_g4_unicode.py B2).  Here the smallest legal dictionary
(vocab_capacity_log2 = 10, C = 1 024 slots) is filled to its last slot and
one term beyond it, a commit is made to fail over a published snapshot, and
one term of one document reaches tf 2^24 - 1 and 2^24.

A  Exactly C terms (the commit must succeed and equal the oracle) and C + 1
   terms (TFIDF_E_CAPACITY, the message names 2^10) with the last 24 / 25
   terms brought by a document routed to one tokenizer path each (the
   kernels run one after the other, so the later path meets the full
   table): P1 the ASCII wave one document per window, P2 packed, P3
   k_tokenize_wave<UNI>, P4 k_tokenize_uwave (and with TFIDF_NO_UNIWAVE=1),
   P5 the chunk path, P6 its non-ASCII units (k_tokenize_chunk<UNI>,
   k_tokenize_uchunk), P7 k_tokenize_long; P1 - P3 again with the 4-slot
   group probe and the 16-slot retry window (TFIDF_TEST_G4_BITS=10).  Six
   term kinds, one per key / lookup route (pool()).  At load 1.0 every probe
   wraps at the table end, every absent query term scans the whole host
   mirror, and the last claims walk the table to its only free slot.  One
   case of about 3 C terms, and one under TFIDF_TEST_WEAK_HASH=1 with the
   hashed kinds over capacity (collision and capacity flags together: the
   commit must end with TFIDF_E_CAPACITY, not "collisions under 4 seeds").
B  A failed commit publishes nothing (searches, batched searches, an open
   reader, statistics, df, document terms: bit for bit as before), leaves
   the documents staged, and a later commit of a fitting corpus (offenders
   replaced by key, or after clear()) equals the oracle; twice in a row;
   before any success; with a mostly non-ASCII failing corpus (the UNI-first
   mode is chosen from the last build's counters); over a snapshot built
   under hash seed 1.
C  tf 2^24 - 1 is stored, escaped and scored; tf 2^24 is refused
   (UnsupportedInput) and the committed state stays.

Bar: index statistics, every document's terms, length and norm, df of every
term, and hits at k = 0 and k = 10 as float32 bit patterns, all equal to the
CPU oracle's (oracle/tfidf_oracle.c).

Dictionary probe loops and what bounds each on a table without a free slot
(read before the first run; none waits for a slot to become free):

  dict_lookup_multi (dict_device.h)          it < mask + 1 + 4096 bucket steps; then kInvalidSlot
    callers: resolve_terms (folded / hashed keys), k_tokenize_uwave,
    k_tokenize_uchunk, k_tokenize_long, kernels_vocab.hip
  uni_find_verify, probe                     it < mask + 1 + 4096 bucket steps
  uni_find_verify, wait for a published hi   w < 2^20 re-reads, then the slot is probed again (counts as a step)
  resolve_terms, short-key rounds            round > dmask ends them (each round advances every pending
                                             key by one bucket / group); what is left is a capacity error
  resolve_terms, retry queue                 it < dmask + 4096 window steps (entered once, at <= 64 pending)
  bucket_probe / group_probe / window_probe  straight-line code: one aligned 2 / 4 / 16-slot window each
  dict_claim_short                           one CAS, no loop; a lost CAS advances the caller's slot
  dict_verify                                no loop (one load; defers at most kVerifyCap checks)
  k_verify_deferred                          grid-stride loop over min(count, kVerifyCap) entries
  k_tokenize_chunk                           resolve_terms<false, false, UNI>: the bounds above
  k_long_rows                                no dictionary probe (adds up the units' (slot, tf) pairs)
  gtable_insert (k_tokenize_long's own       it < 2 (mask + 1) + 4096; its wait for a reference word
    per-document table, not the dictionary)  w < 2^20
  wave histogram (per-document LDS table)    round / it >= kWaveSlots -> overflow (the long path)
  host_lookup (tfidf_capi.hip)               it <= mask slots

The boundary these tests pin (stated in tfidf.h): a 2^x-slot dictionary holds
exactly 2^x terms.

Durations on an MI355X (pytest --durations=0, call phase; 58 tests, 5.3 s
for the module, nothing in csrc/ changed to make them pass):

  test_exactly_full_dictionary        0.04 s each (22 cases)
  test_one_term_too_many              0.01 s each (22 cases)
  test_three_times_too_many           0.33 / 0.31 s (block / term)
  test_capacity_wins_over_collisions  0.30 / 0.31 s
  test_failed_commit_publishes_nothing_and_recovers   0.17 / 0.18 s
  test_failure_before_any_success     0.05 s each
  test_failed_non_ascii_build_does_not_steer_the_next 0.22 s each
  test_failed_commit_over_a_rebuilt_snapshot          0.52 / 0.53 s
  test_tf_at_and_past_the_limit       0.03 s each, both sides in both layouts
                                      (+ 0.37 s once: the oracle of the 33 MB document)
"""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import oracle as O
from tfidf_amd import _lib as L
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

from test_gpu_identity import LONG as ID_LONG, UNI as ID_UNI, corpus as identity_corpus
from test_gpu_parity import assert_hits_equal, f32bits, index_stats
from test_gpu_unicode_sparse import check

pytestmark = pytest.mark.gpu

BLOCK, TERM = L.INVERSION_BLOCK, L.INVERSION_TERM
LAYOUTS = pytest.mark.parametrize("inversion", [BLOCK, TERM], ids=["block", "term"])

CAP_LOG2 = 10                    # the smallest dictionary tfidf_create takes
CAP = 1 << CAP_LOG2
N_LAST = 24                      # terms the extra documents bring in the exactly-full variant
N_BASE = CAP - N_LAST

# --------------------------------------------------------------------------
# terms

KINDS = ("a8", "a16", "a17", "u7", "u14", "u15")
ASCII_KINDS = KINDS[:3]


def pool(kind, i):
    """Term i (< 1000) of a kind; every kind takes another key and lookup
    route, and each has two lengths, the second at the kind's upper limit:
      a8   ASCII <= 8 bytes            the short-key probes (4 and 8 bytes)
      a16  ASCII 9 - 16 bytes          folded, exact 128-bit key (9 and 16)
      a17  ASCII > 16 bytes            hashed, verified (17 and 20)
      u7   non-ASCII <= 7 bytes        uni_key_from_short (3 - 5 and 7)
      u14  non-ASCII 8 - 14 bytes      exact (8 and 14)
      u15  non-ASCII > 14 bytes        hashed, uni_find_verify (15 and 27)
    All are lower case and made of letters that are their own lower case, so
    the wave rules take a document of them."""
    assert 0 <= i < 1000
    odd = i & 1
    if kind == "a8":
        return b"abcd%04d" % i if odd else synth.word(i + 1)
    if kind == "a16":
        return b"sixteenbytes%04d" % i if odd else b"abcde%04d" % i
    if kind == "a17":
        return b"hashedasciiterm%05d" % i if odd else b"seventeenbyte%04d" % i
    if kind == "u7":
        return ("éé%03d" % i if odd else "é%d" % i).encode()
    if kind == "u14":
        return ("größe%03dßé" % i if odd else "éé%04d" % i).encode()
    if kind == "u15":
        return ("ελλάδα%03dмосква" % i if odd else "größe%03dßéa" % i).encode()
    raise ValueError(kind)


assert [len(pool(k, i)) for k in KINDS for i in (10, 11)] == [4, 8, 9, 16, 17, 20, 4, 7, 8, 14, 15, 27]
assert len({pool(k, i).lower() for k in KINDS for i in range(1000)}) == 6000       # pairwise distinct

BASE_COUNTS = {"a8": 600, "a16": 250, "a17": N_BASE - 850}                        # indices [0, count)
NEW_FROM = 900                                                                     # the last terms: indices [900, 990)
ABSENT = [pool(k, i) for k in KINDS for i in (996, 997)]                           # never in any corpus
FILLER = [pool("a8", i) for i in range(40)]                                        # base terms that pad long documents


def base_terms():
    return [pool(k, i) for k, n in BASE_COUNTS.items() for i in range(n)]


def base_docs(terms, per_doc=12, seed=1024):
    """Short ASCII documents (<= 300 bytes: four fit a packed window) that hold
    every term of `terms` once, plus three earlier ones each (df > 1)."""
    rng = random.Random(seed)
    deal = terms[:]
    rng.shuffle(deal)
    texts = []
    for a in range(0, len(deal), per_doc):
        words = deal[a:a + per_doc] + [rng.choice(deal[:a + 1]) for _ in range(3)]
        rng.shuffle(words)
        texts.append(b" ".join(words))
    assert all(len(t) <= 320 for t in texts)
    return texts


def new_terms(kinds, n, start=NEW_FROM):
    return [pool(kinds[j % len(kinds)], start + j // len(kinds)) for j in range(n)]


def filler(n_bytes, seed):
    rng = random.Random(seed)
    out, size = [], 0
    while size < n_bytes:
        out.append(rng.choice(FILLER))
        size += len(out[-1]) + 1
    return out


def extra_doc(n_new, kinds, fixed="", pad=0, start=NEW_FROM, seed=7):
    """One document that brings exactly n_new terms the base corpus lacks: the
    terms of `fixed` (counted by the oracle's tokenizer) and pool terms of
    `kinds`, shuffled among `pad` bytes of base terms."""
    fixed_b = fixed.encode()
    fixed_terms = set(O.tokenize(fixed_b)) if fixed_b else set()
    assert not fixed_terms & set(base_terms())
    terms = new_terms(kinds, n_new - len(fixed_terms), start)
    assert not fixed_terms & set(terms)
    words = terms + filler(pad, seed) + terms[:3]                  # three of them twice
    random.Random(seed).shuffle(words)
    if fixed_b:
        words.insert(len(words) // 2, fixed_b)
    return b" ".join(words)


# --------------------------------------------------------------------------
# A: the path cases.  name -> (environment, builder of the extra documents for
# n new terms, expected statistics of the build)

def p_ascii(n):
    """The last terms in three ordinary documents."""
    t = new_terms(ASCII_KINDS, n)
    return [b" ".join(t[j::3] + FILLER[j:j + 4]) for j in range(3)]


def p_book(n):
    """Three stretches of more than one 4 096-byte chunk unit each: ASCII,
    simple non-ASCII letters (the wave rules' units), then text the wave
    rules decline (Han, Hebrew: k_tokenize_uchunk)."""
    a, b = n // 3, n // 3
    return [extra_doc(a, ASCII_KINDS, pad=4500, start=900, seed=11) + b" " +
            extra_doc(b, KINDS[3:], pad=4500, start=930, seed=12) + b" " +
            extra_doc(n - a - b, KINDS, fixed="中文 שלום", pad=4500, start=960, seed=13)]


P_CASES = {
    "P1": ({"TFIDF_PACK_DOCS": "1"}, p_ascii,
           dict(pack_docs=1, unicode_docs=0, long_docs=0)),
    "P2": ({"TFIDF_PACK_DOCS": "4"}, p_ascii,
           dict(pack_docs=4, pack_retried=0, unicode_docs=0, long_docs=0)),
    "P3": ({"TFIDF_PACK_DOCS": "1"}, lambda n: [extra_doc(n, KINDS)],
           dict(unicode_docs=1, unicode_wave_docs=1, long_docs=0)),
    "P4": ({"TFIDF_PACK_DOCS": "1"}, lambda n: [extra_doc(n, KINDS, fixed="中文 שלום")],
           dict(unicode_docs=1, unicode_wave_docs=0, long_docs=0)),
    "P4-nouniwave": ({"TFIDF_PACK_DOCS": "1", "TFIDF_NO_UNIWAVE": "1"}, lambda n: [extra_doc(n, KINDS)],
                     dict(unicode_docs=1, unicode_wave_docs=0, long_docs=0)),
    "P5": ({"TFIDF_PACK_DOCS": "1"}, lambda n: [extra_doc(n, ASCII_KINDS, pad=6000)],
           dict(unicode_docs=0, long_docs=1, long_chunked=1)),
    "P6": ({"TFIDF_PACK_DOCS": "1"}, p_book,
           dict(unicode_docs=0, long_docs=1, long_chunked=1)),
    "P7": ({"TFIDF_PACK_DOCS": "1"}, lambda n: [extra_doc(n, KINDS, fixed="q" * 300 + " 中", pad=6000)],
           dict(unicode_docs=0, long_docs=1, long_chunked=0)),
}
for _p in ("P1", "P2", "P3"):
    _env, _mk, _st = P_CASES[_p]
    P_CASES["G4-" + _p] = (dict(_env, TFIDF_TEST_G4_BITS=str(CAP_LOG2)), _mk, _st)
PATHS = pytest.mark.parametrize("case", list(P_CASES))


def case_texts(case, n_new):
    return base_docs(base_terms()) + P_CASES[case][1](n_new)


def case_queries(o):
    """Two present terms of each kind the corpus holds (one of them the last
    the corpus brought), pairs across kinds, and absent terms of every kind:
    on a full table the host lookup of those finds no empty slot to stop at."""
    vocab = set(o.vocab())
    present = []
    for k in KINDS:
        have = [pool(k, i) for i in range(1000) if pool(k, i) in vocab]
        present += have[:1] + have[-1:]
    return present + [a + b" " + b for a, b in zip(present, present[1:])] + ABSENT + \
        [ABSENT[0] + b" " + present[0], "中".encode(), b"q" * 255, "שלום".encode(),
         b" ".join(sorted(vocab)[::25]), b" ".join(FILLER)]           # hits in many documents


@pytest.fixture(scope="module")
def oracles():
    """Oracle indexes by corpus name: built once, shared by both layouts."""
    made = {}

    def get(name, texts, keys=None):
        if name not in made:
            o = O.OracleIndex()
            for i, t in enumerate(texts):
                o.add_doc(keys[i] if keys else str(i).encode(), t)
            o.commit()
            made[name] = o
        return made[name]

    yield get
    for o in made.values():
        o.close()


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def new_index(inversion, cap_log2=CAP_LOG2):
    return ShardIndex(vocab_capacity_log2=cap_log2, inversion=inversion)


def assert_equals_oracle(g, o, texts, queries):
    check(g, o, texts)                                              # statistics, terms, lengths, norms, malformed
    vocab = o.vocab()
    for t in sorted(vocab):
        assert g.df(t)[0] == vocab[t], t
    for q in queries:
        for k in (0, 10):
            assert_hits_equal(g.search(q, k), o.search(q, k))


def commit_fails_with_capacity(g):
    with pytest.raises(L.TfidfError) as e:
        g.commit()
    assert e.value.code == L.E_CAPACITY, e.value
    assert "2^%d dictionary slots" % CAP_LOG2 in str(e.value)     # the message names the slot count


@PATHS
@LAYOUTS
def test_exactly_full_dictionary(monkeypatch, oracles, case, inversion):
    env, _, want_stats = P_CASES[case]
    set_env(monkeypatch, env)
    texts = case_texts(case, N_LAST)
    o = oracles(case + "/fit", texts)
    assert o.num_terms == CAP                                       # load 1.0: not one slot free
    g = new_index(inversion)
    g.add_documents(texts)
    g.commit()
    st = g.stats()
    assert st["term_major"] == (1 if inversion == TERM else 0)
    assert st["num_terms"] == CAP
    for k, v in want_stats.items():                                 # the extra document took the intended path
        assert st[k] == v, (k, st[k], v)
    assert_equals_oracle(g, o, texts, case_queries(o))
    g.close()


@PATHS
@LAYOUTS
def test_one_term_too_many(monkeypatch, oracles, case, inversion):
    env, _, _ = P_CASES[case]
    set_env(monkeypatch, env)
    texts = case_texts(case, N_LAST + 1)
    assert oracles(case + "/over", texts).num_terms == CAP + 1
    g = new_index(inversion)
    g.add_documents(texts)
    commit_fails_with_capacity(g)
    g.close()


def many_terms_docs():
    """3 C terms of all six kinds; the ASCII half in documents of its own as well."""
    terms = [pool(k, i) for k in KINDS for i in range(3 * CAP // 6)]
    asc = [t for t in terms if max(t) < 0x80]
    return base_docs(asc, seed=3) + base_docs(terms, seed=4)


@LAYOUTS
def test_three_times_too_many(monkeypatch, oracles, inversion):
    monkeypatch.setenv("TFIDF_PACK_DOCS", "1")
    texts = many_terms_docs()
    assert oracles("3C", texts).num_terms == 3 * CAP
    g = new_index(inversion)
    g.add_documents(texts)
    commit_fails_with_capacity(g)
    g.close()


@LAYOUTS
def test_capacity_wins_over_collisions(monkeypatch, oracles, inversion):
    """Hashed keys of one byte length collide under the weak seed, and there
    are more terms than slots: the first attempt sees collisions (and may see
    the full table), the rebuild under seed 1 the full table alone."""
    monkeypatch.setenv("TFIDF_TEST_WEAK_HASH", "1")
    monkeypatch.setenv("TFIDF_PACK_DOCS", "1")
    terms = [pool("a17", i) for i in range(700)] + [pool("u15", i) for i in range(400)]
    texts = base_docs(terms, per_doc=8, seed=5)
    assert oracles("weak", texts).num_terms == 1100 > CAP
    g = new_index(inversion)
    g.add_documents(texts)
    commit_fails_with_capacity(g)
    g.close()


# --------------------------------------------------------------------------
# B: failed commits

class Staged:
    """The documents an index holds, as add_documents with keys leaves them:
    a key added again replaces its document, which moves to the end."""

    def __init__(self):
        self.docs = {}
        self.bytes_added = 0

    def add(self, g, keys, texts):
        g.add_documents(texts, keys)
        for k, t in zip(keys, texts):
            self.docs.pop(k, None)
            self.docs[k] = t
            self.bytes_added += len(t)

    def texts(self):
        return list(self.docs.values())

    def oracle(self):
        o = O.OracleIndex()
        for k, t in self.docs.items():
            o.add_doc(k, t)
        o.commit()
        return o


def fit_docs():
    """A mixed corpus of C - 4 terms: the base documents, one document for the
    wave rules and one for k_tokenize_uwave."""
    texts = base_docs(base_terms()) + [extra_doc(10, KINDS, start=900), extra_doc(10, KINDS, fixed="中文 שלום", start=930)]
    return [b"k%03d" % i for i in range(len(texts))], texts


def overflow_docs(start, n=2):
    """n documents of 60 new terms of all kinds each."""
    return ([b"x%d" % j for j in range(n)],
            [extra_doc(60, KINDS, start=start + 10 * j, seed=20 + j) for j in range(n)])


def small_docs(keys):
    return keys, [b"small " + FILLER[j] + " é1".encode() for j in range(len(keys))]


B_QUERIES = [pool("a8", 0), pool("a16", 1), pool("a17", 2), pool("u7", 900), pool("u14", 900), pool("u15", 930),
             pool("a8", 3) + b" " + pool("a17", 5), pool("a8", 1) + b" AND " + pool("a8", 2), "中".encode(), b"small",
             pool("u7", 600), pool("a17", 601), "é1".encode(),
             b" ".join(pool("a8", i) for i in range(60)), b" ".join(FILLER[:5])] + ABSENT[::2]


def bits(hits):
    return [(d, f32bits(s)) for d, s in hits]


def committed_stats(g):
    """tfidf_stats without the fields tfidf.h documents as the builder's:
    text_bytes (the staged corpus) and device_bytes (which includes it)."""
    return {k: v for k, v in index_stats(g).items() if k not in ("text_bytes", "device_bytes")}


def generation(g):
    with g.reader() as rd:
        return rd.generation


def observe(g, rd, terms):
    """Everything a caller can read of the published state, through the
    index and through the reader rd."""
    n = g.stats()["num_docs"]
    d, s, c = g.search_batch(B_QUERIES, 10)
    return {
        "search": [[bits(g.search(q, k)) for k in (0, 10)] for q in B_QUERIES],
        # (row i holds c[i] valid hits; tfidf.h promises nothing about the rest)
        "batch": [list(zip(d[i, :c[i]].tolist(), s.view(np.uint32)[i, :c[i]].tolist())) for i in range(len(B_QUERIES))],
        "batch_all": [bits(h) for h in g.search_batch_all(B_QUERIES)],
        "reader": [[bits(rd.search(q, k)) for k in (0, 10)] for q in B_QUERIES],
        "reader_batch_all": [bits(h) for h in rd.search_batch_all(B_QUERIES)],
        "reader_keys": [x.tobytes() for x in rd.doc_keys()],
        "generation": generation(g),
        "stats": committed_stats(g),
        "df": [g.df(t) for t in terms],
        "docs": [(g.doc_terms(i), g.doc_len(i), g.doc_key(i)) for i in range(n)],
        "malformed": g.malformed_docs(),
    }


def assert_observed_equals_oracle(obs, o, staged):
    """observe()'s record against the oracle of the corpus it was taken on."""
    texts = staged.texts()
    for i, q in enumerate(B_QUERIES):
        want0, want10 = bits(o.search(q, 0)), bits(o.search(q, 10))
        assert obs["search"][i] == [want0, want10], q
        assert obs["reader"][i] == [want0, want10], q
        assert obs["batch_all"][i] == want0 and obs["reader_batch_all"][i] == want0, q
        assert obs["batch"][i] == want10, q
    st = obs["stats"]
    vocab = o.vocab()
    assert (st["num_docs"], st["doc_count"], st["sum_ttf"], st["num_terms"], st["nnz"]) == \
        (len(texts), o.doc_count, o.sum_ttf, o.num_terms, sum(vocab.values()))
    assert [x[0] for x in obs["df"]] == [vocab[t] for t in sorted(vocab)]
    keys = list(staged.docs)
    for i in range(len(texts)):
        assert obs["docs"][i] == (o.doc_terms(i), (o.doc_len(i), o.doc_norm(i)), keys[i]), i
    assert obs["malformed"] == o.malformed_docs()


def assert_fresh_commit_equals_oracle(g, staged):
    o = staged.oracle()
    with g.reader() as rd:
        obs = observe(g, rd, sorted(o.vocab()))
    assert_observed_equals_oracle(obs, o, staged)
    o.close()
    return obs


@LAYOUTS
def test_failed_commit_publishes_nothing_and_recovers(monkeypatch, inversion):
    monkeypatch.setenv("TFIDF_PACK_DOCS", "1")
    g, staged = new_index(inversion), Staged()
    staged.add(g, *fit_docs())
    g.commit()
    o = staged.oracle()
    assert CAP - 8 <= o.num_terms <= CAP
    terms = sorted(o.vocab())
    rd = g.reader()
    before = observe(g, rd, terms)
    assert_observed_equals_oracle(before, o, staged)
    assert before["generation"] == rd.generation == 1
    # 1. the failing commit: nothing published, the documents stay staged
    xkeys, xtexts = overflow_docs(600)
    staged.add(g, xkeys, xtexts)
    commit_fails_with_capacity(g)
    assert observe(g, rd, terms) == before
    assert g.stats()["text_bytes"] == staged.bytes_added            # builder-side: the staged corpus
    # 3. again, over the snapshot the failed build left behind, and with one more document
    commit_fails_with_capacity(g)
    staged.add(g, [b"x9"], [extra_doc(30, KINDS, start=700, seed=29)])
    commit_fails_with_capacity(g)
    assert observe(g, rd, terms) == before
    # 2. recovery without clear(): the offenders replaced by key
    staged.add(g, *small_docs(xkeys + [b"x9"]))
    g.commit()
    after = assert_fresh_commit_equals_oracle(g, staged)
    assert after["generation"] == 2                                 # the failed commits took no generation
    # the reader opened before all this still serves the first commit
    now = observe(g, rd, terms)
    for k in ("reader", "reader_batch_all", "reader_keys"):
        assert now[k] == before[k], k
    rd.close()
    g.close()
    o.close()


@LAYOUTS
def test_failure_before_any_success(monkeypatch, inversion):
    monkeypatch.setenv("TFIDF_PACK_DOCS", "1")
    g, staged = new_index(inversion), Staged()
    staged.add(g, *fit_docs())
    staged.add(g, *overflow_docs(600))
    commit_fails_with_capacity(g)
    with pytest.raises(L.TfidfError) as e:
        g.search(pool("a8", 0), 10)
    assert e.value.code == L.E_STATE
    with pytest.raises(L.TfidfError) as e:
        g.reader()
    assert e.value.code == L.E_STATE
    assert g.stats()["num_docs"] == 0 and g.stats()["text_bytes"] == staged.bytes_added
    g.clear()
    staged = Staged()
    staged.add(g, *fit_docs())
    g.commit()
    assert assert_fresh_commit_equals_oracle(g, staged)["generation"] == 1
    g.close()


def uni_heavy_docs():
    """100 documents of non-ASCII terms and 20 ASCII ones: more than C terms."""
    uni = [pool(k, i) for k in KINDS[3:] for i in range(400)]
    texts = base_docs(uni, seed=6) + base_docs([pool("a8", i) for i in range(240)], seed=7)
    assert len(texts) == 120
    return [b"u%03d" % i for i in range(len(texts))], texts


@LAYOUTS
def test_failed_non_ascii_build_does_not_steer_the_next(monkeypatch, inversion):
    """tfidf_commit chooses the UNI-first mode (k_tokenize_wave<UNI> takes
    every document, the ASCII pass does not run) from the counters of the
    last build: a failed, mostly non-ASCII one must leave the next commits
    with the results and path counters of a fresh index."""
    monkeypatch.setenv("TFIDF_PACK_DOCS", "1")
    g, staged = new_index(inversion), Staged()
    keys, texts = uni_heavy_docs()
    staged.add(g, keys, texts)
    commit_fails_with_capacity(g)
    ascii_docs = base_docs([pool(k, i) for k, n in (("a8", 400), ("a16", 200), ("a17", 100)) for i in range(n)],
                           per_doc=7)
    assert len(ascii_docs) == 100
    for step in ("mostly ASCII", "mixed"):
        if step == "mostly ASCII":                                   # all but four non-ASCII documents replaced
            staged.add(g, keys[4:100], ascii_docs[:96])
        else:                                                        # 74 of 120 non-ASCII again, within capacity
            staged.add(g, keys[30:100], [t + " é7 größe007ßé".encode() for t in ascii_docs[:70]])
        g.commit()
        assert_fresh_commit_equals_oracle(g, staged)
        fresh = new_index(inversion)
        fresh.add_documents(staged.texts(), list(staged.docs))
        fresh.commit()
        st, want = g.stats(), fresh.stats()
        for k in ("unicode_docs", "unicode_wave_docs", "long_docs", "long_chunked", "num_terms", "nnz", "pack_docs"):
            assert st[k] == want[k], (step, k, st[k], want[k])
        assert want["unicode_docs"] == (4 if step == "mostly ASCII" else 74), step
        fresh.close()
    g.close()


@LAYOUTS
def test_failed_commit_over_a_rebuilt_snapshot(monkeypatch, inversion):
    """The published snapshot was built under hash seed 1 (collisions under
    the weak seed); the failing commit starts from the weak seed again.  The
    snapshot keeps its own seed: its hashed terms are still found."""
    monkeypatch.setenv("TFIDF_TEST_WEAK_HASH", "1")
    g, staged = new_index(inversion), Staged()
    texts = identity_corpus(2)
    staged.add(g, [b"i%03d" % i for i in range(len(texts))], texts)
    g.commit()
    o = staged.oracle()
    queries = ID_LONG + [u.encode() for u in ID_UNI] + [b"cafe", b"internationalisation"]
    terms = sorted(o.vocab())

    def snapshot():
        st = g.stats()
        assert (st["hash_seed"], st["hash_rebuilds"]) == (1, 1)
        assert [g.df(t)[0] for t in terms] == [o.vocab()[t] for t in terms]
        for q in queries:
            for k in (0, 10):
                assert_hits_equal(g.search(q, k), o.search(q, k))
        return committed_stats(g), [g.doc_terms(d) for d in range(len(texts))]

    before = snapshot()
    assert before[1] == [o.doc_terms(d) for d in range(len(texts))]
    staged.add(g, [b"big"], [b" ".join(pool(k, i) for k in KINDS for i in range(200))])
    commit_fails_with_capacity(g)
    assert snapshot() == before
    g.close()
    o.close()


# --------------------------------------------------------------------------
# C: kMaxTf = 2^24 - 1 (tfidf_common.h)

MAX_TF = (1 << 24) - 1


def doc_terms_small(g, doc, cap=8):
    """tfidf_doc_terms with buffers for `cap` terms (ShardIndex.doc_terms sizes
    them by the document's length: 800 MB here)."""
    buf = C.create_string_buffer(cap * 1024 + 64)
    tfs = np.zeros(cap, np.uint32)
    n = C.c_uint64()
    L.check(L.load().tfidf_doc_terms(g._h, doc, buf, len(buf), L.ptr(tfs, C.c_uint32), cap, C.byref(n)))
    return dict(zip(buf.raw.split(b"\0")[:n.value], tfs[:n.value].tolist()))


def oracle_doc_terms_small(o, doc, cap=8):
    buf = C.create_string_buffer(cap * 260 + 16)
    tfs = np.zeros(cap, np.uint32)
    n = O.lib().orc_doc_terms(o._ix, doc, buf, len(buf), tfs.ctypes.data_as(C.POINTER(C.c_uint32)), cap)
    assert n >= 0
    return dict(zip(buf.raw.split(b"\0")[:n], tfs[:n].tolist()))


@pytest.fixture(scope="module")
def max_tf():
    texts = [b"a " * MAX_TF + b"b", b"b a"]
    o = O.OracleIndex()
    for i, t in enumerate(texts):
        o.add_doc(str(i).encode(), t)
    o.commit()
    yield texts, o
    o.close()


@LAYOUTS
def test_tf_at_and_past_the_limit(max_tf, inversion):
    texts, o = max_tf
    assert oracle_doc_terms_small(o, 0) == {b"a": MAX_TF, b"b": 1}
    assert (o.doc_len(0), o.doc_norm(0)) == (1 << 24, 199)

    g = new_index(inversion, 18)
    g.add_documents(texts)
    g.commit()

    def legal_state():
        st = g.stats()
        assert st["term_major"] == (1 if inversion == TERM else 0)
        assert (st["num_docs"], st["doc_count"], st["sum_ttf"], st["num_terms"], st["nnz"]) == \
            (2, o.doc_count, o.sum_ttf, o.num_terms, 4)
        assert st["long_docs"] == 1 and st["long_chunked"] == 1      # about 16 k chunk units
        assert doc_terms_small(g, 0) == {b"a": MAX_TF, b"b": 1}
        assert doc_terms_small(g, 1) == oracle_doc_terms_small(o, 1) == {b"a": 1, b"b": 1}
        for d in range(2):
            assert g.doc_len(d) == (o.doc_len(d), o.doc_norm(d)), d
        assert g.doc_len(0) == (1 << 24, 199)
        assert g.df(b"a")[0] == g.df(b"b")[0] == 2 == o.vocab()[b"a"] == o.vocab()[b"b"]
        hits = []
        for q in (b"a", b"b", b"a b"):
            for k in (0, 10):
                got = g.search(q, k)
                assert_hits_equal(got, o.search(q, k))
                hits.append(bits(got))
        return hits

    before = legal_state()
    # one more "a": tf 2^24 does not fit the 24-bit field
    g.add_documents([b"a " * (MAX_TF + 1)])
    with pytest.raises(L.UnsupportedInput):
        g.commit()
    assert legal_state() == before
    g.close()
