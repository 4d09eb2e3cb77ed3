"""Reference for wildcard and prefix search (tfidf_wildcard_terms*,
tfidf_search_wildcard*), written from the contract in DESIGN.md §2 and the
oracle alone: a pattern is parsed to elements and matched by a plain DP over
code points; the terms of a pattern come from brute force over
OracleIndex.vocab(), its documents from brute force over
OracleIndex.doc_terms(d).  Also the test corpora (the dense one is
fuzzy_ref's)."""
import functools

from oracle import oracle as O

from fuzzy_ref import (ABC, CAFES, EMOJI, HAN, LONG255, SPECIALS, dense_texts, dense_vocab,  # noqa: F401
                       oracle_vocab)

STAR, ANY = "*", "?"          # element markers (a literal is an int code point)
MAX_ELEMS = 255


def parse(pattern: bytes):
    """Elements of a pattern: STAR, ANY or a lower-cased code point; None for
    a pattern that matches nothing (empty, not strict UTF-8, more than 255
    elements after collapsing runs of '*')."""
    try:
        s = pattern.decode("utf-8")
    except UnicodeDecodeError:
        return None
    out, i = [], 0
    while i < len(s):
        c = s[i]
        i += 1
        if c == "*":
            if not out or out[-1] != STAR:
                out.append(STAR)
        elif c == "?":
            out.append(ANY)
        else:
            if c == "\\" and i < len(s):
                c = s[i]
                i += 1
            out.append(ord(O.lower_utf8(c.encode("utf-8")).decode("utf-8")))
    if not out or len(out) > MAX_ELEMS:
        return None
    return out


def match(elems, cps):
    """Does the whole code point sequence match the elements?  DP over
    (elements consumed, code points consumed), no recursion."""
    reach = {0}                                   # elements consumed so far, before any code point
    def close(r):
        r = set(r)
        for i in sorted(r):
            if i < len(elems) and elems[i] == STAR:
                r.add(i + 1)
        return r
    reach = close(reach)
    for ch in cps:
        nxt = set()
        for i in reach:
            if i == len(elems):
                continue
            e = elems[i]
            if e == STAR:
                nxt.add(i)
            elif e == ANY or e == ch:
                nxt.add(i + 1)
        reach = close(nxt)
        if not reach:
            return False
    return len(elems) in reach


@functools.lru_cache(maxsize=None)
def _cps(term: bytes):
    return tuple(ord(c) for c in term.decode("utf-8"))


def matches(pattern: bytes, term: bytes):
    e = parse(pattern)
    return e is not None and match(e, _cps(term))


def expected_terms(vocab: dict, pattern: bytes, max_out):
    """([(term bytes, df)] in (df descending, bytes) order, cut at max_out;
    n_matched before the cut) by brute force over vocab {term: df}."""
    e = parse(pattern)
    if e is None:
        return [], 0
    out = [(t, df) for t, df in vocab.items() if df >= 1 and match(e, _cps(t))]
    out.sort(key=lambda x: (-x[1], x[0]))
    return out[:max_out], len(out)


def expected_docs(doc_term_sets, vocab: dict, pattern: bytes):
    """(ascending doc ids holding a matching term, n_matched) by brute force;
    doc_term_sets[d] = the set of terms of live document d."""
    e = parse(pattern)
    if e is None:
        return [], 0
    hit = {t for t, df in vocab.items() if df >= 1 and match(e, _cps(t))}
    return [d for d, ts in enumerate(doc_term_sets) if not hit.isdisjoint(ts)], len(hit)


def oracle_index(texts):
    ix = O.OracleIndex()
    for i, t in enumerate(texts):
        ix.add_doc(b"%d" % i, t)
    ix.commit()
    return ix


def doc_term_sets(ix, n):
    return [set(ix.doc_terms(d)) for d in range(n)]


# ---------------------------------------------------------------------------
# the block corpus: 3 * 8192 - 5 short documents (three blocks, the last one
# partial); chosen terms sit at block edges and bitmap word edges

N_BLOCKS_DOCS = 3 * 8192 - 5
EDGE_DOCS = [0, 31, 32, 63, 64, 8191, 8192, 16383, N_BLOCKS_DOCS - 1]


def block_texts():
    """Document d holds w<d % 7> and v<d % 3>; the edge documents also hold
    'edgeterm' and 'edge<i>'; document 8191 alone holds 'solo'."""
    texts = [b"w%d v%d" % (d % 7, d % 3) for d in range(N_BLOCKS_DOCS)]
    for i, d in enumerate(EDGE_DOCS):
        texts[d] += b" edgeterm edge%d" % i
    texts[8191] += b" solo"
    return texts


BLOCK_PATTERNS = [b"edge*", b"edgeterm", b"edge?", b"solo", b"w3", b"w*", b"*", b"*0", b"?1", b"nothing*", b"e*0",
                  b"edge8", b"s?l*"]


def block_expected(pattern: bytes):
    """expected_docs for block_texts(), from the construction (every document's terms are known)."""
    sets = []
    for d in range(N_BLOCKS_DOCS):
        sets.append({b"w%d" % (d % 7), b"v%d" % (d % 3)})
    for i, d in enumerate(EDGE_DOCS):
        sets[d] |= {b"edgeterm", b"edge%d" % i}
    sets[8191].add(b"solo")
    vocab = {}
    for s in sets:
        for t in s:
            vocab[t] = vocab.get(t, 0) + 1
    return expected_docs(sets, vocab, pattern), vocab
