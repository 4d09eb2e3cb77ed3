"""Reference for the fuzzy term lookup (tfidf_fuzzy_terms*), written from the
contract in DESIGN.md §2 and the oracle alone (OracleIndex.vocab for the
vocabulary, lower_utf8 for LowerCaseFilter): the distance is a plain
full-matrix optimal-string-alignment DP over code points, the candidates of a
term come from brute force over the vocabulary.  Also the test corpora."""
import functools
import itertools

from oracle import oracle as O


def osa(a, b):
    """Optimal string alignment distance of two sequences: insert, delete,
    substitute and transpose two adjacent items cost 1 each, no substring is
    edited twice."""
    n, m = len(a), len(b)
    d = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        d[i][0] = i
    for j in range(m + 1):
        d[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            v = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
            if i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                v = min(v, d[i - 2][j - 2] + 1)
            d[i][j] = v
    return d[n][m]


def term_cps(term: bytes):
    """Lower-cased code points of an input term; None for a term without
    candidates (empty, not strict UTF-8, longer than 255 UTF-16 units)."""
    if not term:
        return None
    try:
        s = term.decode("utf-8")
    except UnicodeDecodeError:
        return None
    if len(s.encode("utf-16-le")) // 2 > 255:
        return None
    return tuple(ord(c) for c in O.lower_utf8(term).decode("utf-8"))


@functools.lru_cache(maxsize=None)
def _vocab_cps(v: bytes):
    return tuple(ord(c) for c in v.decode("utf-8"))


@functools.lru_cache(maxsize=1 << 20)
def _dist(t, v):
    return osa(t, v)


def expected(vocab: dict, term: bytes, max_edits, prefix_len, max_out):
    """([(term bytes, df, dist)] in (dist, df descending, bytes) order, cut at
    max_out; n_within before the cut) by brute force over vocab {term: df}."""
    t = term_cps(term)
    if t is None:
        return [], 0
    p = min(prefix_len, len(t))
    out = []
    for v, df in vocab.items():
        if df < 1:
            continue
        c = _vocab_cps(v)
        if len(c) < p or c[:p] != t[:p]:
            continue
        if abs(len(c) - len(t)) > max_edits:         # the distance is at least the difference of the lengths
            continue
        d = _dist(t, c)
        if d <= max_edits:
            out.append((v, df, d))
    out.sort(key=lambda x: (x[2], -x[1], x[0]))
    return out[:max_out], len(out)


# ---------------------------------------------------------------------------
# corpora

ABC = [("".join(p)).encode() for n in range(1, 7) for p in itertools.product("abc", repeat=n)]   # 1 092 strings

ASCII_SPECIALS = [b"zqxjkvwy", b"zqxjkvwyp", b"zqxjkvwypmnbghtr", b"zqxjkvwypmnbghtrd",
                  b"zqxjkvwypmnbghtrdzqxjkvwypmnbghtrdfghjkl"]                                      # 8, 9, 16, 17, 40 bytes
UNI_SPECIALS = ["àéîõüçñ".encode(), "àéîõüçñz".encode()]                                         # 14, 15 bytes
CAFES = ["café".encode(), b"cafe", "cafés".encode()]
HAN, EMOJI = "中".encode(), "\U0001F600".encode()
LONG255 = b"lmnop" * 51                                                                            # 255 units
SPECIALS = ASCII_SPECIALS + UNI_SPECIALS + CAFES + [HAN, EMOJI, LONG255]
assert [len(s) for s in ASCII_SPECIALS] == [8, 9, 16, 17, 40] and [len(s) for s in UNI_SPECIALS] == [14, 15]


def extra_docs(i):
    """Repeats of ABC[i] beyond its own document: df = 1 + extra_docs(i) in 1..5, with many ties."""
    return (i * 7 + i // 5) % 5


def dense_texts():
    """One document per string of ABC, repeats so that df takes 1..5, and every
    special term twice: spelt in upper case first, then as it is."""
    texts = list(ABC)
    for i, s in enumerate(ABC):
        texts += [s] * extra_docs(i)
    for s in SPECIALS:
        texts.append(b"X " + s.decode().upper().encode() + b" .")
        texts.append(s)
    return texts


def _neighbours(s: bytes):
    """A few strings at one and two edits of s (by code points)."""
    c = s.decode()
    n = len(c)
    out = [c[1:], c[:-1], c[: n // 2] + "q" + c[n // 2:], "w" + c[1:]]
    if n >= 2:
        out += [c[1] + c[0] + c[2:], c[:-2] + c[-1] + c[-2], c[2:], c[1:-1], c[1:] + "q", c[: n // 2] + "qw" + c[n // 2:]]
    if n >= 4:
        out += [c[1] + c[0] + c[2:-2] + c[-1] + c[-2], c[0] + c[2] + c[1] + c[3:-1]]
    return [x.encode() for x in out if x]


def dense_terms():
    """The input terms of the dense corpus: the specials (one also in upper
    case) and their neighbours, a term with hundreds of candidates, absent
    terms, a duplicate, and three terms that cannot have candidates."""
    terms = []
    for s in SPECIALS:
        terms.append(s)
        terms += _neighbours(s)
    terms += [b"a", b"abc", b"ABCA", "CAFÉ".encode(), b"zzzzzzzzzzzz", b"xyz", b"a", b"", b"\xff\xfe", b"ab\xc3",
              b"l" * 256, b"abcabca", b"cb"]
    return terms


def oracle_vocab(texts):
    ix = O.OracleIndex()
    for i, t in enumerate(texts):
        ix.add_doc(b"%d" % i, t)
    ix.commit()
    v = ix.vocab()
    ix.close()
    return v


@functools.lru_cache(maxsize=None)
def dense_vocab():
    return oracle_vocab(dense_texts())
