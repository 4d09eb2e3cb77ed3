"""Every query route on one corpus (helper of test_routes_fixture_cpu.py,
test_gpu_routes_incremental.py, test_gpu_node_routes_incremental.py and
test_gpu_routes_layouts.py).

The corpus is the 25 200 documents of test_gpu_incremental_inversion (3-6 words
over 400 words, 8 192 documents per block) with a few ROUTE DOCUMENTS put at
fixed positions: at the block edge (8191, 8192), at the ends of the first
commits of the two shapes the tests use (8300 and 16 500 documents), at the
ends of the batches appended to them (8300..8499 and 16 500..24 576) and inside
blocks 0 and 1.  Each family of route documents occurs below 8192, in
8300..8499 and from 16 500 on, so every route has hits on both sides of the
line between the blocks a commit keeps and the ones it builds:

  phrase     mqalpha mqbeta mqgamma mqalpha mqbeta / mqbeta mqalpha / mqalpha mqfill mqbeta
  hashed     LONG_TERM (34 ASCII bytes) from document 4 on; its neighbours N1 in new_batch() only, N2 from 16 501
  non-ASCII  cafe, cafés, the Han and the emoji term of wildcard_ref
  fuzzy      six spellings of "zorblat" whose df order the appended batches change
  mlt        seeds that repeat three common words and two pivot words; the batches move the pivots' df
             across min_df = 5 and max_df = 4
  new words  new_batch(): the batch 8300..8499 with one of 50 words absent before put in front, and N1

Documents 8300..8499 hold no word that the 8300 before them lack (a commit of
them moves no column); new_batch() and the documents from 16 500 on do.

expected(texts) holds the references of every route over one document list,
computed once: the oracle for the scorer, wildcard_ref, regex_ref, fuzzy_ref,
fuzzy_search_ref, phrase_ref, phrase_slop_ref, mlt_ref and highlight_ref for the
rest.  sweep(h, exp) asserts every route of a ShardIndex or a Reader equal to
them (float32 scores by their bits) and the *_arrays forms equal, byte for byte,
to those of a fresh one-commit index of the same documents.  Route documents
are found by their text, so a list from which documents were deleted works too.
expected(texts, k1, b, extra_route) takes the index's BM25 parameters and more
documents to treat as route documents and more-like-this seeds (HEAVY_A and
HEAVY_B of test_gpu_routes_layouts.py); the fresh index is a default-layout one
with the same k1 and b.
"""
import numpy as np

import fuzzy_ref as F
import fuzzy_search_ref as R
import highlight_ref as H
import mlt_ref as M
import phrase_ref as P
import phrase_slop_ref as S
import regex_ref as X
import wildcard_ref as W
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

from test_gpu_incremental_commit import LONG_TERM, keyed
from test_gpu_incremental_inversion import BLOCK, MULTI, TEXTS

c = synth.word

# ---------------------------------------------------------------------------
# the route documents

M1, M2, M3, MX = b"mqalpha", b"mqbeta", b"mqgamma", b"mqfill"
P_FULL = b" ".join([M1, M2, M3, M1, M2])                 # "mqalpha mqbeta" twice
P_REV = M2 + b" " + M1
P_GAP = M1 + b" " + MX + b" " + M2

N1, N2 = LONG_TERM[:-1] + b"z", LONG_TERM + b"x"         # one edit from LONG_TERM each, two from one another
HASH = LONG_TERM + b" first seen here " + LONG_TERM
HASH2 = b"seen " + LONG_TERM + b" here"
N1_DOC, N2_DOC = N1 + b" seen " + c(5), N2 + b" seen " + c(6)

CAFE_ACUTE, CAFE, CAFES = W.CAFES
NA = b" ".join([CAFE_ACUTE, CAFE, W.HAN, W.EMOJI])
NA2 = "Cafés CAFÉ ".encode() + W.HAN

FUZ = [b"zorblat", b"zorblet", b"zorblit", b"zorblats", b"zarblat", b"zorbalt"]


def fuz(i, j=0):
    return FUZ[i] + b" " + c(50 + 7 * i + j)


PIV_A, PIV_B = b"pivotalfa", b"pivotbravo"


def seed(j):
    return b" ".join([c(10 + j)] * 3 + [c(20 + j)] * 2 + [c(30 + j)] * 2 + [PIV_A] * 2 + [PIV_B] * 2)


SEEDS = [seed(j) for j in range(4)]
PIV_A_DOCS = [PIV_A + b" " + c(77), PIV_A + b" " + c(79)]
PIV_B_DOCS = [PIV_B + b" " + c(78), PIV_B + b" " + c(80)]

FIRST_A, APPEND_A = 8300, 200                            # block 0 kept, a 108-document tail, 200 documents added
FIRST_B, END_B = 16500, 3 * BLOCK + 1                    # blocks 0 and 1 kept; block 2 fills, one document behind it
PLAIN = 100                                              # a document that is no route document: a seed too

PLACED = [
    # block 0
    (3, P_FULL), (4, HASH), (5, NA), (6, NA2), (7, P_GAP), (10, SEEDS[0]),
    (11, fuz(0)), (12, fuz(1)), (13, fuz(1, 1)), (14, fuz(2)), (15, fuz(2, 1)), (16, fuz(2, 2)), (17, fuz(3)),
    (18, fuz(4)), (19, fuz(5)), (20, PIV_A_DOCS[0]), (21, PIV_B_DOCS[0]),
    (BLOCK - 1, P_REV),
    # block 1 up to the end of the first commit of 8300
    (BLOCK, P_FULL), (8295, SEEDS[1]), (8296, HASH), (FIRST_A - 1, P_GAP),
    # the 200 documents behind it
    (FIRST_A, P_FULL), (8301, HASH2), (8302, NA2), (8303, P_GAP), (8304, HASH), (8305, fuz(1, 2)), (8306, fuz(1, 3)),
    (8307, fuz(0, 1)), (8310, SEEDS[2]), (8311, PIV_A_DOCS[1]), (8498, NA), (FIRST_A + APPEND_A - 1, P_REV),
    # inside block 1, the end of the first commit of 16 500
    (12000, P_GAP), (FIRST_B - 1, P_FULL),
    # the documents behind it, up to the one-document block
    (FIRST_B, P_FULL), (16501, N2_DOC), (16502, P_REV), (16503, P_GAP), (16504, HASH), (16505, NA2),
    (16506, fuz(4, 1)), (16507, fuz(4, 2)), (16508, fuz(4, 3)), (16509, fuz(4, 4)), (16510, fuz(2, 3)),
    (16513, SEEDS[3]), (16514, PIV_B_DOCS[1]), (16515, NA), (END_B - 1, P_FULL),
]


def _route_texts():
    t = list(TEXTS)
    for pos, text in PLACED:
        t[pos] = text
    return t


BASE = _route_texts()
ROUTE = frozenset([text for _, text in PLACED] + [N1_DOC])
assert len({pos for pos, _ in PLACED}) == len(PLACED) and not ROUTE & set(TEXTS) and TEXTS[PLAIN] not in ROUTE

NEW_WORDS = [c(1000 + j) for j in range(50)]             # absent from TEXTS, as in test_new_terms_remap_the_base


def new_batch():
    """Documents 8300..8499 with a new word in front of every document that is no route document, and
    LONG_TERM's neighbour N1 in place of document 8301."""
    out = [t if t in ROUTE else NEW_WORDS[i % 50] + b" " + t for i, t in enumerate(BASE[FIRST_A:FIRST_A + APPEND_A])]
    assert out[1] == HASH2
    out[1] = N1_DOC
    return out


# Two heavy route documents (test_gpu_routes_layouts.py; test_routes_fixture_cpu.py holds them to these numbers).
# HEAVY_A: over the tokenizer's 4096-byte window (the long-document path), tf 600: past the scatter temp's and a
# 9-bit CSR field's escape value (511), below the block-major posting's (2047).  HEAVY_B: over two 16 384-byte
# highlight items, tf 2100: past the posting's escape too; LONG_TERM's first bytes are written by the long path,
# "mqalpha mqfill mqbeta" matches 2100 times, and the sloppy frequencies are float32 sums over 2099 and more matches.
HEAVY_A = (M1 + b" " + M2 + b" ") * 600 + SEEDS[0]
HEAVY_B = LONG_TERM + b" " + (M1 + b" " + MX + b" " + M2 + b" ") * 2100 + FUZ[0]
HEAVY = BASE[:FIRST_A] + [HEAVY_A, HEAVY_B]
BM25 = [(2.0, 1.0), (1.2, 0.0)]                          # (k1, b) beside the default; b = 0: scores without a length


# ---------------------------------------------------------------------------
# the probes

QUERIES = ([M1, M2, M3, MX, M1 + b" " + M2, LONG_TERM, N1, NEW_WORDS[0], NEW_WORDS[49], NEW_WORDS[3] + b" " + c(7),
            FUZ[0], FUZ[1], FUZ[4], CAFE_ACUTE, CAFE + b" " + W.HAN, PIV_A, PIV_B + b" " + c(10), b"seen here"] +
           MULTI + [c(i) for i in (1, 7, 55, 120, 200, 300, 399, 400)])
PHRASES = [M1 + b" " + M2, M2 + b" " + M1, b" ".join([M1, M2, M3]), P_GAP, M1 + b" " + M3, LONG_TERM + b" first",
           b"here " + LONG_TERM, CAFE_ACUTE + b" " + CAFE, M1,
           MX + b" " + M1]                               # slop 1 in HEAVY_B: 2099 matches of length 1, 1049.5
SLOPS = (0, 1, 2)
OLD_AND_NEW = b"a?m*"                                    # aama .. aamz of the 400 words, abml .. abmz of the new ones
WILDCARDS = [b"*", b"zorbl*", OLD_AND_NEW, LONG_TERM[:12] + b"*", "caf?".encode(), b"mq*", b"z?rb*t", b"pivot*"]
REGEXES = ([X.from_wildcard(p) for p in (b"zorbl*", OLD_AND_NEW, "caf?".encode())] +
           [b"zorbl(a|e)ts?|mqbeta|" + LONG_TERM[:5] + b".*", b"a[ab]m[a-m]|z[ao]r[a-z]{4,5}"])
FUZZY = [FUZ[0], b"zorblot", N1, CAFE, c(7), M1[:-1]]
FUZZY_PARAMS = [(1, 0), (2, 0), (1, 2), (2, 2)]
FUZZY_OUT = (3, 10)
EXPANSIONS = 50
MLT_CROSSED = dict(min_tf=1, min_df=1, max_df=4)         # the pivots' df go from 3 to 5 and from 4 to 6
MLT_PARAMS = [{}, MLT_CROSSED, dict(min_tf=1, min_df=1)]  # the last one selects every word of a plain document too
TEXT_QUERIES = [M1, M2 + b" " + M1, b" ".join([M1, M2, M3]), LONG_TERM + b" first", CAFE_ACUTE + b" " + W.HAN,
                FUZ[1] + b" " + PIV_A]
WIDTH = 160


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def hit_bits(hits):
    return [(int(d), f32bits(s)) for d, s in hits]


# ---------------------------------------------------------------------------
# the references of one document list

class Expected:
    def __init__(self, texts, k1=1.2, b=0.75, extra_route=()):
        self.texts = texts = list(texts)
        self.k1, self.b = k1, b
        n = len(texts)
        extra = [i for i, t in enumerate(texts) if t in extra_route]
        assert len(extra) == len(set(extra_route))
        self.route_ids = sorted([i for i, t in enumerate(texts) if t in ROUTE] + extra)
        self.seeds = [i for i, t in enumerate(texts) if t in SEEDS] + [texts.index(TEXTS[PLAIN])] + extra
        self.mlt = M.MltRef(texts, k1, b)
        self.o = self.mlt.o
        self.vocab = self.o.vocab()
        self.term_sets = [set(r) for r in self.mlt.rows]
        self.shard = R.Shard.from_rows(self.mlt.rows, self.mlt.norm, self.vocab, self.o.doc_count, self.o.sum_ttf)
        self.phrase = P.PhraseRef(texts, k1, b)
        assert self.o.num_docs == n and not self.phrase.bad
        w = self.want = {}
        for q in QUERIES:
            for k in (0, 10):
                w["search", q, k] = hit_bits(self.o.search(q, k))
        for p in PHRASES:
            w["phrase", p] = P.exact(self.phrase.search(p))
            for s in SLOPS:
                w["slop", p, s] = S.exact(S.search(self.phrase, p, s))
        for p in WILDCARDS:
            for m in (5, 1024):
                w["wild_terms", p, m] = W.expected_terms(self.vocab, p, m)
            w["wild_docs", p] = W.expected_docs(self.term_sets, self.vocab, p)
        for p in REGEXES:
            for m in (5, 1024):
                w["regex_terms", p, m] = X.expected_terms(self.vocab, p, m)
            w["regex_docs", p] = X.expected_docs(self.term_sets, self.vocab, p)
        for t in FUZZY:
            for e, p in FUZZY_PARAMS:
                for m in FUZZY_OUT:
                    w["fuzzy_terms", t, e, p, m] = F.expected(self.vocab, t, e, p, m)
                exp, within = R.expansion(self.vocab, t, e, p, EXPANSIONS)
                w["fuzzy_expand", t, e, p] = ([(a, b, d, float(x)) for a, b, d, x in exp], within)
                per_doc = R.clause_scores(self.shard, exp, k1=k1, b=b)
                assert R.sums_are_order_independent(per_doc)         # so the scorer's clause order cannot show
                w["fuzzy_hits", t, e, p] = (R.bits(R.hits(per_doc)), len(exp))
        for i, params in enumerate(MLT_PARAMS):
            for d in self.seeds:
                sel, cands = self.mlt.terms(d, **{**M.DEFAULTS, **params})
                w["mlt_terms", d, i] = (M.exact_terms(sel), cands)
                w["mlt_hits", d, i] = M.exact_hits(self.mlt.more_like_this(d, 10, True, **params))
        for q in TEXT_QUERIES:
            terms = H.plain_terms(q)
            ms = [H.matches(texts[d], terms) for d in self.route_ids]
            w["matches", q] = ms
            w["snippets", q] = [(a, texts[d][a:b], rel) for d, (a, b, rel) in
                                zip(self.route_ids, (H.snippet(texts[d], m, WIDTH) for d, m in zip(self.route_ids, ms)))]
        self._fresh = None

    def fresh_arrays(self):
        """arrays() of a fresh index that took the documents in one commit (built once, closed again)."""
        if self._fresh is None:
            f = ShardIndex(k1=self.k1, b=self.b)
            try:
                f.add_documents(self.texts, [k for k, _ in keyed(self.texts)])
                f.commit()
                assert f.commit_tokenized_docs() == {"docs": len(self.texts), "was_full": True}
                self._fresh = arrays(f, self)
            finally:
                f.close()
        return self._fresh

    def slop_batch(self):
        return [p for p in PHRASES for _ in SLOPS], [s for _ in PHRASES for s in SLOPS]


_expected = {}


def expected(texts, k1=1.2, b=0.75, extra_route=()):
    key = (len(texts), hash(tuple(texts)), k1, b, tuple(extra_route))
    if key not in _expected:
        _expected[key] = Expected(texts, k1, b, extra_route)
    return _expected[key]


# ---------------------------------------------------------------------------
# the sweep

def _canon(result):
    """A *_arrays result without its device time: arrays as (dtype, shape, bytes)."""
    out = []
    for x in result:
        if isinstance(x, np.ndarray):
            out.append((x.dtype.str, x.shape, x.tobytes()))
        elif not isinstance(x, float):
            out.append(x)
    return out


def arrays(h, exp):
    """The *_arrays form of every call that has one on ShardIndex and on Reader."""
    ph, sl = exp.slop_batch()
    return {
        "search_batch_all": _canon(h.search_batch_all_arrays(QUERIES)),
        "search_phrase_batch": _canon(h.search_phrase_batch_arrays(PHRASES)),
        "search_phrase_slop_batch": _canon(h.search_phrase_slop_batch_arrays(ph, sl)),
        "search_wildcard_batch": _canon(h.search_wildcard_batch_arrays(WILDCARDS)),
        "search_regex_batch": _canon(h.search_regex_batch_arrays(REGEXES)),
        "fuzzy_expand_batch": _canon(h.fuzzy_expand_batch_arrays(FUZZY, 2, 0, EXPANSIONS)),
        "search_fuzzy_batch": _canon(h.search_fuzzy_batch_arrays(FUZZY, 2, 0, EXPANSIONS)),
        "more_like_this_batch": _canon(h.more_like_this_batch_arrays(exp.seeds, 10, True)),
        "mlt_terms_batch": _canon(h.mlt_terms_batch_arrays(exp.seeds)),
        "mlt_terms_batch_crossed": _canon(h.mlt_terms_batch_arrays(exp.seeds, **MLT_CROSSED)),
    }


def sweep(h, exp):
    """Every route of `h` (a ShardIndex or a Reader) against the references of exp."""
    w = exp.want
    # 1. the batched scorer
    for q, got in zip(QUERIES, h.search_batch_all(QUERIES)):
        assert hit_bits(got) == w["search", q, 0], q
    if isinstance(h, ShardIndex):                        # a Reader has no top-k batch
        docs, scores, counts = h.search_batch(QUERIES, 10)
        for i, q in enumerate(QUERIES):
            n = int(counts[i])
            assert list(zip(docs[i, :n].tolist(), scores[i, :n].view(np.uint32).tolist())) == w["search", q, 10], q
    # 2. phrases
    for p, got in zip(PHRASES, h.search_phrase_batch(PHRASES)):
        assert P.exact(got) == w["phrase", p], p
    ph, sl = exp.slop_batch()
    for p, s, got in zip(ph, sl, h.search_phrase_slop_batch(ph, sl)):
        assert S.exact(got) == w["slop", p, s], (p, s)
    # 3. wildcards, 4. regular expressions
    for name, pats, terms, docs in (("wild", WILDCARDS, h.wildcard_terms_batch, h.search_wildcard_batch),
                                    ("regex", REGEXES, h.regex_terms_batch, h.search_regex_batch)):
        for m in (5, 1024):
            for p, got in zip(pats, terms(pats, m)):
                assert got == w[name + "_terms", p, m], (p, m)
        for p, got in zip(pats, docs(pats)):
            assert got == w[name + "_docs", p], p
    # 5. fuzzy
    for e, p in FUZZY_PARAMS:
        for m in FUZZY_OUT:
            for t, got in zip(FUZZY, h.fuzzy_terms_batch(FUZZY, e, p, m)):
                assert got == w["fuzzy_terms", t, e, p, m], (t, e, p, m)
        for t, got in zip(FUZZY, h.fuzzy_expand_batch(FUZZY, e, p, EXPANSIONS)):
            assert got == w["fuzzy_expand", t, e, p], (t, e, p)
        d, s, offs, n_exp, _ = h.search_fuzzy_batch_arrays(FUZZY, e, p, EXPANSIONS)
        o = offs.tolist()
        for i, t in enumerate(FUZZY):
            got = list(zip(d[o[i]:o[i + 1]].tolist(), s[o[i]:o[i + 1]].view(np.int32).tolist()))
            assert (got, int(n_exp[i])) == w["fuzzy_hits", t, e, p], (t, e, p)
    # 6. more like this
    for i, params in enumerate(MLT_PARAMS):
        for d, (sel, cands) in zip(exp.seeds, h.mlt_terms_batch(exp.seeds, **params)):
            assert (M.exact_terms(sel), cands) == w["mlt_terms", d, i], (d, params)
        for d, got in zip(exp.seeds, h.more_like_this_batch(exp.seeds, 10, True, **params)):
            assert M.exact_hits(got) == w["mlt_hits", d, i], (d, params)
    # 7. the text routes
    per = [exp.route_ids] * len(TEXT_QUERIES)
    for q, got in zip(TEXT_QUERIES, h.matches_batch(TEXT_QUERIES, per)):
        assert got == w["matches", q], q
    for q, got in zip(TEXT_QUERIES, h.snippets_batch(TEXT_QUERIES, per, WIDTH)):
        assert got == w["snippets", q], q
    for d in exp.route_ids:
        assert h.doc_text(d) == exp.texts[d], d
    # two histories of one corpus are indistinguishable
    got, fresh = arrays(h, exp), exp.fresh_arrays()
    for name in fresh:
        assert got[name] == fresh[name], name
