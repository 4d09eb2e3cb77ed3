"""Exact phrase search restated from the oracle alone (helper of
test_phrase_cpu.py, test_gpu_phrase.py and test_gpu_node_phrase.py; DESIGN.md
section 2, "Phrase search"): the phrase and the documents are tokenised by the
oracle's tokenizer and lower-casing (through highlight_ref), the statistics come
from an OracleIndex over the live documents, idf / norm cache / BM25 are the
oracle's float functions.  The sum of the positions' idf is taken in Python
floats (doubles) over float32 values and cast to float32 once, as
BM25Similarity.idfExplain(CollectionStatistics, TermStatistics[]) does."""
import numpy as np

import highlight_ref as H
from oracle import oracle as O

_tokens = {}


def terms_of(text: bytes):
    """The lower-cased tokens of ``text`` as the index sees them (cut at 255
    UTF-16 units, the rest of a cut token being the next token); None when the
    text is not valid UTF-8."""
    t = _tokens.get(text)
    if t is None and text not in _tokens:
        toks = H.doc_tokens(text)
        t = _tokens[text] = None if toks is None else tuple(H.lower(text[s:s + l]) for s, l in toks)
    return t


def freq(text: bytes, terms) -> int:
    """#{p : w[p + j] == terms[j] for all j}: overlapping starts all count."""
    w = terms_of(text)
    m = len(terms)
    if w is None or m == 0 or len(w) < m:
        return 0
    terms = tuple(terms)
    first = terms[0]
    return sum(1 for p in range(len(w) - m + 1) if w[p] == first and w[p:p + m] == terms)


class PhraseRef:
    """The expected phrase hits over ``texts`` (the live documents, in live
    order) with the statistics of an OracleIndex over them, or the GLOBAL
    statistics given as (doc_count, sum_ttf, {term: df})."""

    def __init__(self, texts, k1=1.2, b=0.75, global_stats=None):
        self.texts = list(texts)
        self.o = O.OracleIndex(k1, b)
        for i, t in enumerate(self.texts):
            self.o.add_doc(b"d/%07d" % i, t)
        self.o.commit()
        self.bad = set(self.o.malformed_docs())
        if global_stats is None:
            self.doc_count, self.sum_ttf, self.gdf = self.o.doc_count, self.o.sum_ttf, None
        else:
            self.doc_count, self.sum_ttf, self.gdf = global_stats
        self.cache = O.norm_cache(k1, b, O.avgdl(self.sum_ttf, self.doc_count)) if self.doc_count else None
        self.holders = {}

    def close(self):
        self.o.close()

    def df(self, term):
        return self.gdf.get(term, 0) if self.gdf is not None else self.o.df(term)

    def _holders(self, term):
        """The live documents that hold ``term``."""
        h = self.holders.get(term)
        if h is None:
            h = self.holders[term] = frozenset(
                d for d, t in enumerate(self.texts) if d not in self.bad and term in (terms_of(t) or ()))
        return h

    def candidates(self, phrase: bytes):
        """The documents holding every distinct term: the rows a search scans
        ([] for a phrase without work)."""
        terms = terms_of(phrase)
        if not terms or not self.doc_count or any(max(self.o.df(t), 0) == 0 for t in terms):
            return []
        return sorted(frozenset.intersection(*[self._holders(t) for t in set(terms)]))

    def weight(self, terms):
        acc = 0.0
        for t in terms:
            acc += float(np.float32(O.idf(self.df(t), self.doc_count)))
        return float(np.float32(1.0) * np.float32(acc))

    def search(self, phrase: bytes):
        """[(doc, score, freq)] in (score descending, doc ascending)."""
        terms = terms_of(phrase)
        cands = self.candidates(phrase)
        if not cands:
            return []
        w = self.weight(terms)
        out = []
        for d in cands:
            f = freq(self.texts[d], terms)
            if f:
                out.append((d, O.bm25(w, f, float(self.cache[self.o.doc_norm(d)])), f))
        out.sort(key=lambda x: (-x[1], x[0]))
        return out


def bits(score) -> int:
    return int(np.float32(score).view(np.uint32))


def exact(hits):
    """Hits with their float32 score bits, for exact comparison."""
    return [(int(d), bits(s), int(f)) for d, s, f in hits]


def merge(lists_with_base):
    """[(hits, doc_base)] of the shards -> one list by (score descending, global id ascending)."""
    out = [(d + base, s, f) for hits, base in lists_with_base for d, s, f in hits]
    out.sort(key=lambda x: (-x[1], x[0]))
    return out


# ---------------------------------------------------------------------------
# the documents and phrases of the phrase tests: corpora of highlight_ref side
# by side (document ids offset per corpus) and a few new ones

_BACK = H.WORDS70[::-1]
LONG = [b" ".join(_BACK[i % 70] for i in range(1120))]               # the 70 words backwards, 16 times over
PHRASE_1024 = b" ".join(_BACK[i % 70] for i in range(1024))          # starts at tokens 0 and 70 of LONG
PHRASE_1025 = b" ".join(_BACK[i % 70] for i in range(1025))          # the argument error
_EDGE = H.corpus("edge")[0]
CORPORA = [("dense", H.corpus("dense")[0]), ("nosplit", H.corpus("nosplit255")[0]), ("han", H.corpus("han")[0]),
           ("dup", H.corpus("dup")[0]), ("aaa", [b"a a a"]), ("dotted", H.corpus("dotted")[0]),
           ("ops", H.corpus("ops")[0]), ("edge", [_EDGE[29], _EDGE[30], _EDGE[31]]),
           ("unicode", H.corpus("unicode")[0]), ("malformed", H.corpus("malformed")[0]),
           ("seventy", H.corpus("seventy")[0]), ("twins", H.corpus("twins")[0]), ("long", LONG)]
TEXTS, BASE = [], {}
for _name, _texts in CORPORA:
    BASE[_name] = len(TEXTS)
    TEXTS += list(_texts)


def doc(name, i=0):
    return BASE[name] + i


# (phrase, {document: freq} the issue states; every other document's freq comes from freq() alone)
STATED = [
    (b"alpha gamma", {doc("dense"): 2600}),
    (b"gamma alpha", {doc("dense"): 2599}),
    (b"gamma kappa", {doc("dense"): 1}),
    (b"a" * 510, {doc("nosplit", 1): 155}),
    (b"a" * 600, {doc("nosplit", 1): 0, doc("nosplit", 0): 1}),
    ("月星".encode(), {doc("han"): 1366}),
    ("雨山".encode(), {doc("han"): 1365}),
    ("月 星".encode(), {doc("han"): 1366}),
    (b"beta beta", {doc("dup"): 1}),
    (b"a a", {doc("aaa"): 2}),
    (b"beta gamma", {doc("dotted"): 1}),
    (b"beta.gamma beta", {doc("dotted"): 1}),
    (b"alpha beta", {doc("ops", 1): 1, doc("edge", 1): 313, doc("edge", 0): 0, doc("edge", 2): 0}),
    (b"beta alpha", {doc("ops", 1): 1}),
    (b"lambda alpha", {doc("edge", 1): 313, doc("edge", 0): 0, doc("edge", 2): 0}),
]
SINGLE = [b"alpha", b"kappa", b"beta.gamma", "月".encode()]          # m = 1
SEVENTY = b" ".join(H.WORDS70)                                        # hits seventy[2] only
TWINS = H.TWIN_A[0] + b" " + H.TWIN_A[1]
ISTANBUL = "İstanbul is".encode()
NO_WORK = [b"", b", ; . \n", b"alpha zzqqabsent", b"alpha \xff beta"]   # empty, separators, absent term, not UTF-8
PHRASES = [p for p, _ in STATED] + SINGLE + [SEVENTY, TWINS, ISTANBUL, PHRASE_1024, b"AND alpha OR \"beta\"~2"]
