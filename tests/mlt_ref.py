"""More-like-this restated from the oracle alone ("More
like this"): a seed's candidate terms are the terms of its row
(OracleIndex.doc_terms) that pass the tf / df filters on the shard's own df;
score = float32(tf) * idf with idf = float32(log((numDocs + 1) / (df + 1.0)) +
1.0) (math.log, numpy float32 for the product); order: score bits descending,
then term bytes ascending; the first max_terms are the interesting terms.  The
hits are the disjunction of those terms, one clause each in selection order,
BM25 on the statistics in force (O.idf / O.avgdl / O.norm_cache / O.bm25, the
GLOBAL numbers when set), summed in double in clause order and rounded to
float32 once; (score descending, doc ascending)."""
import math
import random

import numpy as np

from oracle import oracle as O

DEFAULTS = dict(min_tf=2, min_df=5, max_df=0, max_terms=25)


def bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def mlt_idf(df, num_docs):
    return np.float32(math.log((num_docs + 1) / float(df + 1)) + 1.0)


def term_score(tf, df, num_docs):
    return np.float32(tf) * mlt_idf(df, num_docs)


class MltRef:
    def __init__(self, texts, k1=1.2, b=0.75):
        self.texts = list(texts)
        self.o = O.OracleIndex(k1, b)
        for i, t in enumerate(self.texts):
            self.o.add_doc(b"%d" % i, t)
        self.o.commit()
        self.k1, self.b = k1, b
        self.n = self.o.num_docs
        self.rows = [self.o.doc_terms(d) for d in range(self.n)]
        self.post = {}
        for d, row in enumerate(self.rows):
            for t, tf in row.items():
                self.post.setdefault(t, []).append((d, tf))
        self.norm = [self.o.doc_norm(d) for d in range(self.n)]
        self.glob = None
        self._stats()

    def close(self):
        self.o.close()

    def _stats(self):
        if self.glob:
            self.doc_count, self.sum_ttf = self.glob[0], self.glob[1]
        else:
            self.doc_count, self.sum_ttf = self.o.doc_count, self.o.sum_ttf
        self.cache = O.norm_cache(self.k1, self.b, O.avgdl(self.sum_ttf, self.doc_count)) if self.doc_count else None

    def set_global_stats(self, doc_count, sum_ttf, df_by_term):
        self.glob = (doc_count, sum_ttf, dict(df_by_term))
        self.o.set_global_stats(doc_count, sum_ttf, df_by_term)
        self._stats()

    def df(self, t):
        return len(self.post.get(t, ()))

    def eff_df(self, t):
        return self.glob[2][t] if self.glob else self.df(t)

    def terms(self, d, min_tf=2, min_df=5, max_df=0, max_terms=25):
        """([(term, tf, df, float32 score)] in selection order, candidates before truncation)."""
        min_tf = max(min_tf, 1)
        cands = []
        for t, tf in self.rows[d].items():
            df = self.df(t)
            if tf >= min_tf and df >= min_df and (max_df == 0 or df <= max_df):
                cands.append((t, tf, df, term_score(tf, df, self.n)))
        cands.sort(key=lambda c: (-bits(c[3]), c[0]))
        return cands[:max_terms], len(cands)

    def hits_of_terms(self, terms, k, drop=None):
        """Top k of the disjunction of `terms` (clause order), without document `drop`."""
        if not self.doc_count:
            return []
        acc = {}
        for t in terms:                                   # clause order: each document's sum runs in this order
            if t not in self.post:
                continue                                  # no scorer on this shard
            w = O.idf(self.eff_df(t), self.doc_count)
            for d, tf in self.post[t]:
                acc[d] = acc.get(d, 0.0) + float(O.bm25(w, tf, float(self.cache[self.norm[d]])))
        out = [(d, float(np.float32(s))) for d, s in acc.items() if d != drop]
        out.sort(key=lambda x: (-bits(x[1]), x[0]))
        return out[:k]

    def more_like_this(self, d, k=10, exclude_seed=True, **params):
        sel, _ = self.terms(d, **{**DEFAULTS, **params})
        return self.hits_of_terms([t for t, _, _, _ in sel], k, d if exclude_seed else None)


def exact_terms(lst):
    return [(bytes(t), int(tf), int(df), bits(s)) for t, tf, df, s in lst]


def exact_hits(lst):
    return [(int(d), bits(s)) for d, s in lst]


def merge(lists_with_base, k, drop=None):
    """[(hits, doc_base)] of the shards -> the top k by (score descending, global id ascending), without `drop`."""
    out = [(d + base, s) for hits, base in lists_with_base for d, s in hits if d + base != drop]
    out.sort(key=lambda x: (-bits(x[1]), x[0]))
    return out[:k]


# ---------------------------------------------------------------------------
# the documents of the more-like-this tests, side by side in one index

def _word(i):
    s = ""
    i += 26
    while i:
        s = chr(97 + i % 26) + s
        i //= 26
    return s


def _skewed(seed, n_docs):
    rng = random.Random(seed)
    vocab = [("w" + _word(i)).encode() for i in range(40)] + [b"x.y", "été".encode(), "straße".encode()]
    weights = [1.0 / (r + 1) for r in range(len(vocab))]
    return [b" ".join(rng.choices(vocab, weights)[0] for _ in range(rng.randrange(5, 60))) for _ in range(n_docs)]


SKEWED = _skewed(11, 60)
# a boundary tie group larger than max_terms = 25: three terms above it, then 48 terms of tf 2 that only this
# document holds: 16 short ones (exact keys), 16 ASCII terms over 16 bytes and 16 non-ASCII terms over 14 bytes
# (hashed keys: their strings are read from the reference occurrence, here in mixed case)
TIE_SHORT = [b"tie" + _word(i).encode() for i in range(16)]
TIE_ASCII = [b"tiegroupasciiterm" + _word(i).encode() for i in range(16)]
TIE_UNI = [("ñandúçedillaétie" + _word(i)).encode() for i in range(16)]
TIE_TOP = [b"toptiea", b"toptieb", b"toptiec"]
TIE_DOC = b" ".join([t for t in TIE_TOP for _ in range(5)] +
                    [(t.upper() if i % 2 else t) for t in (TIE_UNI + TIE_ASCII + TIE_SHORT)[::-1] for i in range(2)])
# a row of more than 4 096 distinct terms, tf 1..3 (about 40 KB)
BIG_WORDS = [("big" + _word(i)).encode() for i in range(4200)]
BIG_DOC = b" ".join(w for i, w in enumerate(BIG_WORDS) for _ in range(1 + i % 3))
# a tf the CSR field cannot hold (65 535 on block-major rows; term-major rows at 2^18 slots escape from 16 383),
# and one of 600; both words also sit in five short documents, so the default min_df keeps them
ESC_DOC = b"zzescape " * 65535 + b"waa wab"
ESC2_DOC = b"zzsixhundred " * 600 + b"zzescape zzescape waa"
ESC_MATES = [b"zzescape zzescape zzsixhundred zzsixhundred waa wab wac"] * 4
EMPTY, MALFORMED = b"", b"waa waa \xff wab wab"

CORPORA = [("empty_front", [EMPTY, MALFORMED]), ("skewed", SKEWED), ("tie", [TIE_DOC]), ("empty_mid", [MALFORMED, EMPTY]),
           ("big", [BIG_DOC]), ("esc", [ESC_DOC, ESC2_DOC] + ESC_MATES), ("empty_end", [EMPTY])]
TEXTS, BASE = [], {}
for _name, _texts in CORPORA:
    BASE[_name] = len(TEXTS)
    TEXTS += list(_texts)


def doc(name, i=0):
    return BASE[name] + i
