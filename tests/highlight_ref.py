"""Hit highlighting restated from the oracle alone (helper of
test_highlight_cpu.py and test_gpu_highlight.py): the matches of (query,
document) from the oracle's tokenizer and lower-casing, the snippet rule in
plain Python, and the corpora both tests use."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as O

_lower = {}


def doc_tokens(text: bytes):
    """[(start, len)] as the index tokenises ``text`` (cut at 255 UTF-16
    units); None for a document that is not valid UTF-8."""
    cap = len(text) // 2 + 2
    st = np.zeros(cap, np.uint32)
    ln = np.zeros(cap, np.uint32)
    n = O.lib().orc_tokenize(text, len(text), 255, st.ctypes.data_as(C.POINTER(C.c_uint32)),
                             ln.ctypes.data_as(C.POINTER(C.c_uint32)), cap)
    if n < 0:
        return None
    return list(zip(st[:n].tolist(), ln[:n].tolist()))


def lower(tok: bytes) -> bytes:
    t = _lower.get(tok)
    if t is None:
        t = _lower[tok] = O.lower_utf8(tok)
    return t


def plain_terms(q: bytes):
    """Positive terms of a query without operator words: the oracle's order."""
    return [t for t, _ in O.query_terms(q)]


def matches(text: bytes, terms):
    """[(start, len, ordinal)] of the document for the positive terms (ordinal = list position)."""
    toks = doc_tokens(text)
    if toks is None:
        return []
    ordinal = {t: i for i, t in enumerate(terms)}
    out = []
    for s, l in toks:
        o = ordinal.get(lower(text[s:s + l]))
        if o is not None:
            out.append((s, l, o))
    return out


def snippet(text: bytes, M, W):
    """(a, b, in-snippet matches relative to a) by the rule of DESIGN.md section 2."""
    L, n = len(text), len(M)
    best = None
    for i, (s, l, _) in enumerate(M):
        if l > W:
            continue
        bits = cnt = end = 0
        j = i
        while j < n and M[j][0] + M[j][1] <= s + W:
            bits |= 1 << min(M[j][2], 63)
            cnt += 1
            end = M[j][0] + M[j][1]
            j += 1
        key = (-bin(bits).count("1"), -cnt, s)
        if best is None or key < best[0]:
            best = (key, s, end)
    a = 0
    if best is not None:
        _, s, end = best
        slack = W - (end - s)
        a = s - min(s, slack // 2)
    b = min(L, a + W)
    while a < b and 0x80 <= text[a] <= 0xBF:
        a += 1
    while b < L and a < b and 0x80 <= text[b] <= 0xBF:
        b -= 1
    return a, b, [(s - a, l, o) for s, l, o in M if s >= a and s + l <= b]


# ---------------------------------------------------------------------------
# corpora: name -> (texts, query, positive terms)

LENGTHS = [0, 1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4095, 4096,
           4097, 16383, 16384, 16385, 20000, 70000]
N_EDGE = 400
WORDS = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta", b"eta", b"theta", b"iota", b"kappa", b"lambda"]


def edge_doc(i, n):
    """n bytes: the document's own number, then words of a small shared vocabulary."""
    parts, size, j = [b"n%d" % i], len(b"n%d" % i), i
    while size < n:
        w = WORDS[j % len(WORDS)]
        parts.append(b" " if j % 13 else b"\n")
        parts.append(w)
        size += 1 + len(w)
        j += 1 + (i % 3)
    return b"".join(parts)[:n]


HAN = "山川草木日月星辰風雨".encode()      # 10 characters, 30 bytes


def han_doc():
    """40 KB of Han characters, no ASCII byte: every character is a token."""
    return HAN * 1366                    # 40 980 bytes


TWIN_A = (b"abcdefghijklmnopqrs1", b"abcdefghijklmnopqrs2")            # 20 bytes, equal first 8 bytes
TWIN_U = ("ééééééééé".encode(), "éééééééèé".encode())                  # 18 bytes each
WORDS70 = [b"w%02dx" % i for i in range(70)]


@functools.lru_cache(maxsize=None)
def corpus(name):
    if name == "edge":
        texts = [edge_doc(i, LENGTHS[i % len(LENGTHS)]) for i in range(N_EDGE)]
        assert [len(t) for t in texts] == [LENGTHS[i % len(LENGTHS)] for i in range(N_EDGE)]
        q = b"alpha gamma Kappa"
        return texts, q, plain_terms(q)
    if name == "nosplit255":
        q = b"a" * 255
        return [b"a" * 600, b"a" * 40000, b"b c"], q, plain_terms(q)
    if name == "nosplit220":
        q = b"a" * 220
        return [b"a" * 600, b"a" * 40000, b"b c"], q, plain_terms(q)
    if name == "han":
        q = "月 雨".encode()
        return [han_doc(), "日月".encode(), b""], q, plain_terms(q)
    if name == "unicode":
        texts = [s.encode() for s in (
            "Été en été, ÉTÉ ou éTé; etc.",
            "İstanbul is big; istanbul, ISTANBUL and İSTANBUL too",
            "Alpha’s beta’s and alpha's, ALPHA’S",
            "ראש צה\"ל אמר צה״ל",
            "hello สวัสดีครับ world สวัสดี ครับ",
            "a 👨‍👩‍👧 family 👨‍👩‍👧‍👦 and 👨 alone",
            "alpha beta gamma beta",
            "x_y and x y; 3,5 or 3, 5; o'neil o' neil O'NEIL x_y",
        )]
        q = "ÉTÉ istanbul alpha’s צה\"ל สวัสดีครับ 👨‍👩‍👧 Beta x_y 3,5 o'neil".encode()
        return texts, q, plain_terms(q)
    if name == "twins":
        texts = [b" ".join([TWIN_A[0], TWIN_A[1], TWIN_U[0], TWIN_U[1], b"x"]),
                 b" ".join([TWIN_A[1], TWIN_U[1], TWIN_A[1]]),
                 b" ".join([TWIN_U[0].upper(), TWIN_A[0].upper(), "ÉÉÉÉÉÉÉÉÉ".encode()])]
        q = TWIN_A[0] + b" " + TWIN_U[0]
        return texts, q, plain_terms(q)
    if name == "ops":
        texts = [b"alpha beta gamma", b"Alpha, beta; alpha", b"gamma only gamma", b"beta gamma", b"delta"]
        return texts, b"alpha AND beta NOT gamma", [b"alpha", b"beta"]
    if name == "dup":
        return [b"beta Beta gamma beta"], b"beta beta", [b"beta"]
    if name == "dotted":
        return [b"beta.gamma Beta beta gamma beta.gamma. BETA.GAMMA"], b"beta.gamma Beta", [b"beta.gamma", b"beta"]
    if name == "seventy":
        # 70 distinct words: ordinals 63..69 share one bit of the ranking
        head = b" ".join(WORDS70[60:70]) + b" " + b"pad " * 60       # 10 terms, 4 distinct bits
        tail = b" ".join(WORDS70[0:6]) + b" " + b"pad " * 60         # 6 terms, 6 distinct bits
        texts = [head + tail, tail + head, b" ".join(WORDS70), b" ".join(WORDS70[63:70]) + b" x " + WORDS70[5]]
        return texts, b" ".join(WORDS70), list(WORDS70)
    if name == "malformed":
        texts = [b"alpha beta", b"alpha \xff beta gamma alpha", "é".encode() * 40 + b"\xc3", b"gamma alpha",
                 b"x" + "é".encode() * 40 + b" alpha \xff"]     # its head ends inside a character at W = 16
        q = b"alpha gamma"
        return texts, q, plain_terms(q)
    if name in ("window", "windowcut"):
        # no split byte for kilobytes: one lane walks every piece boundary, so the
        # scan's lookahead window ends inside every kind of token sooner or later
        import random
        rng = random.Random(20261020)
        pieces = ["abc", "x.y", "o'neil", "3,5", "İstanbul", "日", "🇫🇷", "👨‍👩‍👧", "é́́", "a" * 300,
                  "สวัสดี", "__", "q_r", "a·b", "צה\"ל", "7", "カタカナ", "ひ", "Z" * 1100]
        if name == "window":                 # without the tokens of more than 255 units ("windowcut" has them)
            pieces = [p for p in pieces if len(p) < 256]
        glue = ["\u00a0", "\u00a0\u00a0", "\u2026", "\u3002", "\u2009"]      # separators, none of them ASCII
        docs = []
        for L in (9000, 30000):
            parts, size = [], 0
            while size < L:
                s = rng.choice(pieces) + rng.choice(glue)
                parts.append(s)
                size += len(s.encode())
            docs.append("".join(parts).encode())
        q = "abc x.y o'neil 3,5 istanbul 日 🇫🇷 👨‍👩‍👧 é́́ สวัสดี q_r a·b 7 カタカナ ひ".encode() + \
            b" " + b"a" * 255 + b" " + b"z" * 80 + b" " + b"a" * 45
        return docs, q, plain_terms(q)
    if name == "dense":
        # one document with >= 5000 matches
        q = b"alpha gamma kappa"
        return [b"alpha gamma " * 2600 + b"kappa", b"kappa " * 10], q, plain_terms(q)
    raise KeyError(name)


CPU_CORPORA = ["edge", "nosplit255", "nosplit220", "han", "unicode", "window", "windowcut", "twins", "ops", "dup", "dotted", "seventy",
               "malformed", "dense"]


@functools.lru_cache(maxsize=None)
def expected_matches(name):
    texts, _, terms = corpus(name)
    return [matches(t, terms) for t in texts]


@functools.lru_cache(maxsize=None)
def expected_snippets(name, W):
    texts, _, _ = corpus(name)
    return [snippet(t, m, W) for t, m in zip(texts, expected_matches(name))]
