"""Sloppy phrase search restated from the oracle alone (helper of
test_phrase_slop_cpu.py, test_gpu_phrase_slop.py and
test_gpu_node_phrase_slop.py; DESIGN.md section 2, "Sloppy phrases").  Analysis,
candidates, statistics and weight are phrase_ref's; the frequency of a phrase
of several distinct terms at slop > 0 is Lucene 9.8's SloppyPhraseMatcher walk
written out with a heap of (position, phrase position), summed in float32 in
match order; the score is the BM25 float formula taken one numpy float32
operation at a time (the oracle's orc_bm25 takes an integer tf)."""
import heapq

import numpy as np

import highlight_ref as H
import phrase_ref as P

F32 = np.float32
INT32_MAX = 2 ** 31 - 1
MAX_SLOPPY_TERMS = 64


class Unsupported(Exception):
    """slop > 0 with a repeated term or more than 64 terms."""


def supported(terms, slop) -> bool:
    return slop == 0 or len(terms) < 2 or (len(terms) <= MAX_SLOPPY_TERMS and len(set(terms)) == len(terms))


def sloppy_matches(words, terms, slop):
    """(float32 freq, [matchLength of every counted match]) of the distinct
    ``terms`` (m >= 2) in the token list ``words``."""
    slop = min(slop, INT32_MAX)
    m = len(terms)
    occ = [[p for p, w in enumerate(words) if w == t] for t in terms]
    if any(not o for o in occ):
        return F32(0), []
    cur = [0] * m
    heap = [(occ[j][0] - j, j) for j in range(m)]
    heapq.heapify(heap)
    end = max(p for p, _ in heap)
    freq, lens = F32(0), []

    def count(length):
        nonlocal freq
        if length <= slop:
            freq = F32(freq + F32(1) / F32(F32(1) + F32(length)))
            lens.append(length)
    pos, pp = heapq.heappop(heap)
    length = end - pos
    nxt = heap[0][0]
    while True:
        cur[pp] += 1
        if cur[pp] == len(occ[pp]):
            break
        pos = occ[pp][cur[pp]] - pp
        if pos > end:
            end = pos
        if pos > nxt:
            heapq.heappush(heap, (pos, pp))
            count(length)
            pos, pp = heapq.heappop(heap)
            nxt = heap[0][0]
            length = end - pos
        else:
            length = min(length, end - pos)
    count(length)
    return freq, lens


def freq_of(text: bytes, terms, slop):
    """The float32 frequency of ``terms`` at ``slop`` in one document."""
    if not supported(terms, slop):
        raise Unsupported
    if slop == 0 or len(terms) < 2:
        return F32(P.freq(text, terms))
    words = P.terms_of(text)
    return F32(0) if words is None else sloppy_matches(words, tuple(terms), slop)[0]


def score_f(w, freq, norm_inverse):
    """weight - weight / (1 + freq * cache[norm]) in float32, operation by operation."""
    w, freq, c = F32(w), F32(freq), F32(norm_inverse)
    t = F32(freq * c)
    u = F32(F32(1) + t)
    v = F32(w / u)
    return F32(w - v)


def search(ref: P.PhraseRef, phrase: bytes, slop: int):
    """[(doc, float32 score, float32 freq)] in (score descending, doc ascending)."""
    terms = P.terms_of(phrase)
    if terms and not supported(terms, slop):
        raise Unsupported
    cands = ref.candidates(phrase)
    if not cands:
        return []
    w = ref.weight(terms)
    out = []
    for d in cands:
        f = freq_of(ref.texts[d], terms, slop)
        if f > 0:
            out.append((d, score_f(w, f, ref.cache[ref.o.doc_norm(d)]), f))
    out.sort(key=lambda x: (-float(x[1]), x[0]))
    return out


def bits(x) -> int:
    return int(F32(x).view(np.uint32))


def exact(hits):
    """Hits with their float32 score and frequency bits, for exact comparison."""
    return [(int(d), bits(s), bits(f)) for d, s, f in hits]


def merge(lists_with_base):
    """[(hits, doc_base)] of the shards -> one list by (score descending, global id ascending)."""
    out = [(d + base, s, f) for hits, base in lists_with_base for d, s, f in hits]
    out.sort(key=lambda x: (-float(x[1]), x[0]))
    return out


# ---------------------------------------------------------------------------
# the documents of the sloppy tests: phrase_ref's corpora without the two whose
# scan is one lane's seconds, the nine documents of the stated table, and a long
# alternation of matches of length 1 and 0

NEAR = [b"a b c", b"a b", b"a b c", b"c b a", b"a b c a b c", b"a x b a b", b"a b x x a x b x x b a", b"a b a b a b",
        b"x a y b z c"]
REPS = 2000
REP = [b" ".join([b"a x b a b"] * REPS)]
_KEEP = ("dense", "dup", "aaa", "dotted", "ops", "edge", "unicode", "seventy", "twins", "long")
CORPORA = [(n, t) for n, t in P.CORPORA if n in _KEEP] + [("near", NEAR), ("rep", REP)]
TEXTS, BASE = [], {}
for _name, _texts in CORPORA:
    BASE[_name] = len(TEXTS)
    TEXTS += list(_texts)


def doc(name, i=0):
    return BASE[name] + i


# (document of NEAR, phrase, slop, freq, the matches' lengths): the stated table
STATED = [
    (0, b"a c", 0, 0.0, []), (0, b"a c", 1, 0.5, [1]),
    (1, b"b a", 1, 0.0, []), (1, b"b a", 2, 0.33333334, [2]),
    (2, b"c a", 3, 0.25, [3]), (2, b"c a", 4, 0.25, [3]),
    (3, b"a b c", 3, 0.0, []), (3, b"a b c", 4, 0.2, [4]),
    (4, b"a c", 1, 1.0, [1, 1]),
    (5, b"a b", 1, 1.5, [1, 0]),
    (6, b"a b", 2, 1.8333334, [0, 1, 2]),
    (7, b"b a", 2, 2.3333333, [0, 0, 2]),
    (8, b"a b c", 1, 0.0, []), (8, b"a b c", 2, 0.33333334, [2]),
]
SLOPS = [0, 1, 2, 3, 7, 2 ** 31 - 1, 2 ** 32 - 1]
M64 = b" ".join(H.WORDS70[::-1][:64])                                 # 64 distinct terms: tokens 0, 70, .. of LONG
M65 = b" ".join(H.WORDS70[::-1][:65])
_DROP = {b"a" * 510, b"a" * 600, "月星".encode(), "雨山".encode(), "月 星".encode()}   # of the corpora left out
PHRASES = ([p for p in P.PHRASES if p not in _DROP] + sorted({p for _, p, _, _, _ in STATED}) +
           [b"a x b", b"b x a", b"gamma alpha beta", M64])
NO_WORK = P.NO_WORK
