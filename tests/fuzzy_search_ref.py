"""The specification of the fuzzy search (tfidf_fuzzy_expand*,
tfidf_search_fuzzy*) in Python: Lucene 9.8 FuzzyQuery(term, maxEdits,
prefixLength, maxExpansions, transpositions = true) under
TopTermsBlendedFreqScoringRewrite, restated from DESIGN.md section 2.  No
Lucene is run against it: parity with Lucene is not pinned for this feature.

Candidates: those of the term lookup (fuzzy_ref.osa / term_cps over the
oracle's vocabulary) that also have m > ed, m = min(code points of the
candidate, code points of the term) -- the one rule this restatement chooses
(Lucene would compute boost 0 or less there).  boost = 1 - ed / m in float32.
Expansion: the first max_expansions by (boost descending, bytes ascending).
Weights: boost * idf(largest df of the expansion, docCount) in float32.  Score:
BM25 per clause in float32 (as test_query_operators.py::py_search; k1 = 1.2 and
b = 0.75 unless given), summed in double per document, (score descending, doc
ascending).  Also the fixture."""
import functools
import math

import numpy as np

import fuzzy_ref as F
from oracle import oracle as O

F32 = np.float32

# ---------------------------------------------------------------------------
# the fixture corpus: fuzzy_ref.dense_texts() plus four families

LETTERS = "abcdefghi"
STEM_A = "zqxjkvwypmnbghtr"                     # 16 bytes: + 2 letters = 18, hashed keys
STEM_B = "àéîõüçx"                              # 13 bytes: + 2 letters = 15 non-ASCII bytes, hashed keys
FAMILY_A = [(STEM_A + x + y).encode() for x in LETTERS for y in LETTERS]
FAMILY_B = [(STEM_B + x + y).encode() for x in LETTERS for y in LETTERS]
# equal boost from "qqxqq"; UTF-8 puts U+FF41 first (EF.. < F0..), UTF-16 the supplementary one (D801 < FF41)
PAIR_C = ["qq\U00010428qq".encode(), "qqａqq".encode()]
WORD_D, MISSPELT_D = b"kangaroo", [b"kangarooo", b"kangaro", b"kagnaroo"]
DF_D = 40
assert len(FAMILY_A) == 81 and all(len(t) == 18 for t in FAMILY_A) and all(len(t) == 15 for t in FAMILY_B)
assert PAIR_C[1] < PAIR_C[0] and PAIR_C[0].decode().encode("utf-16-be") < PAIR_C[1].decode().encode("utf-16-be")


def texts():
    out = list(F.dense_texts())
    for fam in (FAMILY_A, FAMILY_B):
        for i, t in enumerate(fam):             # every third term only ever spelt in upper case
            out.append(b"Y " + t.decode().upper().encode() + b" ." if i % 3 == 0 else t)
    out += PAIR_C
    out += [WORD_D + b" zzpad"] * DF_D          # documents of equal length: two tokens each
    out += [m + b" zzpad" for m in MISSPELT_D]
    return out


def probes():
    """The family probes (input terms beyond fuzzy_ref.dense_terms())."""
    return [FAMILY_A[0], FAMILY_A[40].upper(), (STEM_A + "zz").encode(), FAMILY_B[0], (STEM_B + "zz").encode(),
            b"qqxqq", WORD_D, MISSPELT_D[0], MISSPELT_D[2], b"kangaru", b"a", b"b", b"abc", b"ab"]


def terms():
    return F.dense_terms() + probes()


# ---------------------------------------------------------------------------
# the rules

def keep(ed, m):
    return m > ed


def boost(ed, m):
    """One float32 division, one float32 subtraction."""
    if ed == 0:
        return F32(1.0)
    return F32(F32(1.0) - F32(F32(ed) / F32(m)))


@functools.lru_cache(maxsize=None)
def _cps(v: bytes):
    return tuple(ord(c) for c in v.decode("utf-8"))


def candidates(vocab: dict, term: bytes, max_edits, prefix_len):
    """[(term bytes, df, ed, boost)] in (boost descending, bytes ascending) order, uncut."""
    t = F.term_cps(term)
    if t is None:
        return []
    p = min(prefix_len, len(t))
    out = []
    for v, df in vocab.items():
        if df < 1:
            continue
        c = _cps(v)
        if len(c) < p or c[:p] != t[:p] or abs(len(c) - len(t)) > max_edits:
            continue
        d = F._dist(t, c)
        m = min(len(c), len(t))
        if d <= max_edits and keep(d, m):
            out.append((v, df, d, boost(d, m)))
    out.sort(key=lambda x: (-float(x[3]), x[0]))
    return out


def expansion(vocab, term, max_edits, prefix_len, max_expansions):
    """([(term bytes, df, ed, boost)] cut at max_expansions, n_within)."""
    c = candidates(vocab, term, max_edits, prefix_len)
    return c[:max_expansions], len(c)


def straddle(cands, E):
    """The boost group across position E of an uncut candidate list: (first, end) indices, or None."""
    if len(cands) <= E:
        return None
    b = cands[E - 1][3]
    lo = min(i for i, c in enumerate(cands) if c[3] == b)
    hi = max(i for i, c in enumerate(cands) if c[3] == b) + 1
    return (lo, hi)


# ---------------------------------------------------------------------------
# scoring

class Shard:
    """The oracle's view of a list of documents: vocabulary, rows, norms, statistics."""

    def __init__(self, docs):
        ix = O.OracleIndex()
        for i, t in enumerate(docs):
            ix.add_doc(b"%d" % i, t)
        ix.commit()
        self.n = ix.num_docs
        self.vocab = ix.vocab()
        self.rows = [ix.doc_terms(d) for d in range(self.n)]
        self.norms = [ix.doc_norm(d) for d in range(self.n)]
        self.doc_count, self.sum_ttf = ix.doc_count, ix.sum_ttf
        ix.close()
        self._post()

    @classmethod
    def from_rows(cls, rows, norms, vocab, doc_count, sum_ttf):
        """The same view from what a caller already read from an oracle of its own."""
        self = cls.__new__(cls)
        self.n, self.vocab, self.rows, self.norms = len(rows), vocab, rows, norms
        self.doc_count, self.sum_ttf = doc_count, sum_ttf
        self._post()
        return self

    def _post(self):
        self.postings = {}
        for d, row in enumerate(self.rows):
            for t, tf in row.items():
                self.postings.setdefault(t, []).append((d, tf))


def norm_cache(doc_count, sum_ttf, k1=1.2, b=0.75):
    avg = F32(sum_ttf / float(doc_count))
    lens = np.array([O.byte4_to_int(i) for i in range(256)], np.float32)
    k1, b = F32(k1), F32(b)
    with np.errstate(divide="ignore"):          # b = 1: length 0 gives inf, as the oracle's cache has it
        return F32(1) / (k1 * ((F32(1) - b) + b * lens / avg))


def clause_scores(shard, exp, df_of=None, doc_count=None, sum_ttf=None, k1=1.2, b=0.75):
    """{doc: [float32 clause scores in selection order]} of an expansion on a
    shard; df_of / doc_count / sum_ttf: the statistics in force (default: the shard's own); k1 / b: the
    index's BM25 parameters."""
    dc = shard.doc_count if doc_count is None else doc_count
    if dc == 0 or not exp:
        return {}
    cache = norm_cache(dc, shard.sum_ttf if sum_ttf is None else sum_ttf, k1, b)
    max_df = max((df_of[t] if df_of is not None else shard.vocab[t]) for t, _, _, _ in exp)
    idf = F32(np.log(1.0 + (dc - max_df + 0.5) / (max_df + 0.5)))
    per_doc = {}
    for t, _, _, bo in exp:
        w = F32(bo * idf)
        for d, tf in shard.postings.get(t, ()):
            per_doc.setdefault(d, []).append(F32(w - w / (F32(1) + F32(tf) * cache[shard.norms[d]])))
    return per_doc


def hits(per_doc):
    """[(doc, float32 score)] by (score descending, doc ascending); the document's clauses summed in double."""
    out = []
    for d, ss in per_doc.items():
        acc = 0.0
        for s in ss:
            acc += float(s)
        out.append((d, F32(acc)))
    out.sort(key=lambda h: (-float(h[1]), h[0]))
    return out


def sums_are_order_independent(per_doc):
    for ss in per_doc.values():
        acc = 0.0
        for s in ss:
            acc += float(s)
        if acc != math.fsum(float(s) for s in ss):
            return False
    return True


def search(shard, term, max_edits, prefix_len, max_expansions, **stats):
    exp, _ = expansion(shard.vocab, term, max_edits, prefix_len, max_expansions)
    return hits(clause_scores(shard, exp, **stats)), len(exp)


def bits(hit_list):
    return [(int(d), int(np.float32(s).view(np.int32))) for d, s in hit_list]


@functools.lru_cache(maxsize=None)
def fixture():
    return Shard(texts())
