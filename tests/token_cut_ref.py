"""Corpora for the 255-unit token cut (helper of test_token_cut_cpu.py and
test_gpu_token_cut.py): StandardAnalyzer cuts a token at 255 UTF-16 units and
rescans from the cut, and six device paths restate that rule.  One table of
over-long runs (RUNS), the placements that put each run where a path can go
wrong, and — from the oracle's spans and the window arithmetic of
tfidf_internal.h alone — which path must take each document (expected_paths).
Nothing here touches a device."""
import ctypes as C
import functools
import os
import re
from collections import namedtuple

import numpy as np

from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "tf-idf-distributed-system_amd", "csrc")

MAX_UNITS = 255                     # kMaxTokenLen
CORE, PRE, POST = 2048, 64, 320     # kCoreBytes, kPreBytes, kPostBytes (header_constants() reads them back)
WAVE_WINDOW = 4096                  # kWaveWindow = kUwWindow: longer documents start on the long list
NO_CUT = 1 << 20                    # orc_tokenize max_len that cuts nothing here


def header_constants():
    """(kCoreBytes, kPreBytes, kPostBytes, kMaxTokenLen) as the sources have them."""
    src = ""
    for f in ("tfidf_internal.h", "tfidf_common.h", "analysis.h"):
        with open(os.path.join(CSRC, f)) as fh:
            src += fh.read()

    def const(name):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\w+)\s*;" % name, src)
        assert m, name
        return int(m.group(1)) if m.group(1).isdigit() else const(m.group(1))
    return const("kCoreBytes"), const("kPreBytes"), const("kPostBytes"), const("kMaxTokenLen")


# ---------------------------------------------------------------------------
# the runs

# prose: None for an ASCII run; True when every non-ASCII character is one the
# wave rules take (k_tokenize_wave<UNI>, DESIGN section 5: an ALetter that is
# its own lower case, or whose lower case has the same UTF-8 length in at most
# 3 bytes; class Other); False when the document must go to the Unicode
# scanner (Katakana, Thai, combining marks, 4-byte cased letters).
# sibling: another spelling whose first term is the same and whose raw bytes
# differ (length or case), or None.
Run = namedtuple("Run", "name text sibling prose")

NBSP, FULLSTOP = "\u00a0", "\u3002"        # separators of class Other; neither holds a split byte
DESERET, DESERET_LOW = "\U00010400", "\U00010428"
# what the wave rules take of this module's non-ASCII characters: é 가 𐐨 (ALetters that are their own lower
# case, of any length), É (its lower case has the same length, at most 3 bytes; 𐐀 has 4) and the separators
WAVE_CHARS = set("\u00e9\u00c9\uac00" + DESERET_LOW + NBSP + FULLSTOP)
THAI = "สวัสดี"                              # 6 characters, 3 of them marks


def joined(letters, joiner, k, lead=0):
    """lead extra letters, then k letters alternating and joined: 2 k - 1 + lead units."""
    return letters[0] * lead + joiner.join(letters[i % 2] for i in range(k))


def _runs():
    runs = []
    for n in (255, 256, 257, 300, 510, 511, 1100):
        runs.append(Run("z%d" % n, "z" * n, "Z" * (n + 3), None))
    for n in (255, 256, 257, 300, 510, 511, 1100):
        runs.append(Run("Z%d" % n, "Z" * n, "z" * (n + 2), None))
    runs.append(Run("d300", "0" * 300, "0" * 304, None))
    runs.append(Run("e200", "é" * 200, "É" * 200, True))            # 400 bytes, 200 units: not cut
    runs.append(Run("e255", "é" * 255, "É" * 258, True))
    runs.append(Run("e256", "é" * 256, "é" * 259, True))
    runs.append(Run("E300", "É" * 300, "é" * 301, True))
    runs.append(Run("ga255", "가" * 255, "가" * 256, True))           # 765 bytes: the longest term there is
    runs.append(Run("ga300", "가" * 300, "가" * 305, True))
    runs.append(Run("des128", DESERET * 128, DESERET_LOW * 130, False))   # 256 units: cut after 127 characters
    runs.append(Run("des200", DESERET * 200, DESERET * 201, False))
    runs.append(Run("a254des", "a" * 254 + DESERET + "a" * 10, "A" * 254 + DESERET + "a" * 12, False))
    runs.append(Run("a200e", "a" * 200 + "é" + "a" * 100, "a" * 200 + "É" + "a" * 103, True))   # 302 bytes, 301 units
    for tag, letters, j in (("dot", "ab", "."), ("comma", "12", ","), ("apos", "ab", "'"), ("under", "xy", "_")):
        for lead in (0, 1, 2):      # the unit at the cut: a letter, a joiner, a letter after a doubled start
            runs.append(Run("%s%d" % (tag, lead), joined(letters, j, 160, lead), joined(letters, j, 163, lead), None))
    runs.append(Run("kata300", "カ" * 300, "カ" * 303, False))
    runs.append(Run("thai300", THAI * 50, THAI * 51, False))
    runs.append(Run("acute300", "a" + "́" * 300, "a" + "́" * 310, False))
    return runs


RUNS = _runs()
RUN = {r.name: r for r in RUNS}
CLASSES = {
    "letters": [r for r in RUNS if r.name[0] in "zZ"],
    "joiners": [r for r in RUNS if r.prose is None and r.name[0] not in "zZ"],
    "unicode": [r for r in RUNS if r.prose is not None],
}


def units(s: str) -> int:
    return sum(2 if ord(c) >= 0x10000 else 1 for c in s)


# ---------------------------------------------------------------------------
# documents

Doc = namedtuple("Doc", "text tag runs")     # bytes, what the document is for, names of the runs in it

WORDS = ["alpha", "beta", "gamma", "delta", "eps", "zeta", "eta"]


def filler(n, salt=0, sep=" ", accent=False, mod=89):
    """Exactly n bytes of short words (every word under 16 bytes), each
    followed by sep: one space, or a non-ASCII separator — then the filler
    holds no split byte at all."""
    sp = sep.encode()
    if n <= 0:
        return b""
    assert n >= len(sp), (n, sep)
    out, i = bytearray(), salt
    while True:
        w = WORDS[i % len(WORDS)] + str(i % mod)
        if accent and i % 5 == 0:
            w += "\u00e9"
        w = w.encode() + sp
        if len(out) + len(w) > n - len(sp):
            break
        out += w
        i += 1
    out += b"x" * (n - len(sp) - len(out)) + sp
    assert len(out) == n
    return bytes(out)


def short_docs(cls):
    """Documents of at most 4 000 bytes (the wave paths meet them): each run
    alone, at the first byte, at the last byte, twice with equal bytes, with
    its sibling in one document, and the sibling in a document of its own."""
    docs = []
    for r in CLASSES[cls]:
        t = r.text
        docs += [Doc(t.encode(), "alone", (r.name,)),
                 Doc((t + " tail of words").encode(), "first", (r.name,)),
                 Doc(("head of words " + t).encode(), "last", (r.name,)),
                 Doc((t + " " + t).encode(), "twice", (r.name,))]
        if r.sibling:
            docs += [Doc((t + " mid " + r.sibling + " end").encode(), "differ", (r.name,)),
                     Doc(("sib " + r.sibling).encode(), "sibling", (r.name,))]
    assert all(len(d.text) <= 4000 for d in docs)
    return docs


# starts of a run relative to the end of a 2 KB core (the next core's start)
EDGES = (("hi-1", -1), ("hi", 0), ("hi+1", 1), ("premargin", -40))


def _place(parts, total, sep, accent):
    """parts: [(offset, text bytes)] in order; filler in between and up to total bytes."""
    out = bytearray()
    for k, (off, t) in enumerate(parts):
        assert off >= len(out), (off, len(out))
        out += filler(off - len(out), salt=7 * k + off, sep=sep, accent=accent)
        out += t
        out += sep.encode()
    out += filler(max(total, len(out) + 120) - len(out), salt=3, sep=sep, accent=accent)
    return bytes(out)


def chunk_docs(runs, sep=" ", accent=False):
    """Documents of 4.2 to 8 KB (the chunk paths): two runs each, the first at
    an offset around the end of core 0, the second at the same offset around
    the end of core 1; and, for a run of more than 320 bytes, starting in core
    0 so that the window's 320-byte trailing margin ends inside it."""
    docs = []
    runs = sorted(runs, key=lambda r: units(r.text) > MAX_UNITS)     # the uncut runs share documents: those stay chunked
    pairs = [runs[i:i + 2] for i in range(0, len(runs), 2)]
    for tag, delta in EDGES:
        for pr in pairs:
            parts, at = [], 0
            for k, r in enumerate(pr):
                off = max((k + 1) * CORE + delta, at)
                if off != (k + 1) * CORE + delta:                 # the first run covers the second's place
                    continue
                parts.append((off, r.text.encode()))
                at = off + len(r.text.encode()) + 1
            docs.append(Doc(_place(parts, 4200, sep, accent), tag, tuple(r.name for r in pr[:len(parts)])))
    for r in runs:
        n = len(r.text.encode())
        if n > POST + 32:                                          # starts in core 0, ends past its window
            off = min(CORE + POST - n // 2, CORE - 24)
            docs.append(Doc(_place([(off, r.text.encode())], 4200, sep, accent), "postclip", (r.name,)))
    assert all(4200 <= len(d.text) <= 8192 for d in docs), [len(d.text) for d in docs]
    return docs


def cover_docs():
    """A whole unit window inside one run: 3 000 ASCII letters, 1 600 é."""
    out = []
    for name, t in (("z3000", "z" * 3000), ("e1600", "é" * 1600), ("Z3000z", "Z" * 3000 + "z" * 10)):
        body = _place([(CORE - 148, t.encode())], 4200, " ", name[0] == "e")
        assert CORE - 148 <= CORE - PRE and CORE - 148 + len(t.encode()) >= 2 * CORE + POST
        out.append(Doc(body, "cover", (name,)))
    return out


def same_prefix_docs():
    """Two tokens with the same first 255 units and different raw spans that
    start in ONE core of a document over 4 096 bytes whose window holds
    non-ASCII text — so the unit goes to k_tokenize_uchunk (every unit with 日,
    the others under TFIDF_NO_UNIWAVE) and meets both in its table."""
    z300, z1100, Z1100, Z300 = b"z" * 300, b"z" * 1100, b"Z" * 1100, b"Z" * 300
    e300, E400 = "é" * 300, "É" * 400
    ga300, ga310 = "가" * 300, "가" * 310
    docs = []
    for mark, sep in (("\u65e5", " "), ("\u00e9", " "), ("\u65e5", NBSP), ("\u00e9", FULLSTOP)):
        m = mark.encode()
        for tag, a, b in (("length", z300, Z1100),                 # both whole in the window, lengths differ
                          ("clipped", Z1100, Z1100),               # equal runs; the second clipped by the window's end
                          ("case", z300, Z300),                    # equal lengths: the same term by uc_same_term
                          ("accent", e300.encode(), E400.encode()),
                          ("hangul", ga300.encode(), ga310.encode())):
            second = 1327 if tag == "clipped" else 182 + len(a) + 60
            parts = [(170, m), (182, a), (second, b)]
            docs.append(Doc(_place(parts, 4300, sep, False), "prefix-" + tag, ()))
    return docs


OVERFLOW_L = 4090


def overflow_docs():
    """a non-ASCII document of at most 4 096 bytes whose
    staged window overflows (shift + L > 4 096, shift = the document's corpus
    offset mod 16).  Document 1 and 2 are such documents (offsets 15 and
    4 105); document 2 also holds a run of 300 z.  Both hold few distinct terms
    (k_tokenize_uwave's table takes 512: kUwMaxTerms)."""
    d0 = "é abc defg hij".encode()
    assert len(d0) == 15
    d1 = filler(OVERFLOW_L, salt=1, accent=True, mod=5)
    d2 = (filler(2000, salt=2, accent=True, mod=5) + b"z" * 300 + b" " +
          filler(OVERFLOW_L - 2301, salt=5, accent=True, mod=5))
    rest = [filler(1800 + 16 * i, salt=10 + i, accent=True) for i in range(3)]
    return [Doc(t, "overflow" if i in (1, 2) else "plain", ()) for i, t in enumerate([d0, d1, d2] + rest)]


@functools.lru_cache(maxsize=None)
def family(name):
    if name in CLASSES:
        return short_docs(name)
    if name == "chunk_ascii":
        return chunk_docs(CLASSES["letters"] + CLASSES["joiners"])
    if name == "chunk_unicode":
        return chunk_docs(CLASSES["unicode"], accent=True)
    if name == "chunk_nosplit":                # separators without a split byte: one lane walks everything
        return (chunk_docs(CLASSES["unicode"][0::2], sep=NBSP, accent=True) +
                chunk_docs(CLASSES["unicode"][1::2], sep=FULLSTOP, accent=True))
    if name == "cover":
        return cover_docs()
    if name == "same_prefix":
        return same_prefix_docs()
    if name == "overflow":
        return overflow_docs()
    if name == "mixed":                        # short and book-sized, ASCII and not: one of each kind of document
        pick = lambda f, tags: [d for d in family(f) if d.tag in tags]
        return (pick("letters", ("alone", "differ"))[::3] + pick("joiners", ("twice", "sibling"))[::2] +
                pick("unicode", ("first", "differ")) + pick("chunk_ascii", ("hi", "postclip"))[::2] +
                pick("chunk_unicode", ("hi-1", "premargin"))[::2] + family("same_prefix")[::4] + family("cover")[:2])
    if name == "unifirst":                     # mostly non-ASCII: a second commit of it runs UNI-first
        return family("unicode") + family("same_prefix")[::3] + family("chunk_unicode")[::5] + family("letters")[::9]
    raise KeyError(name)


FAMILIES = ["letters", "joiners", "unicode", "chunk_ascii", "chunk_unicode", "chunk_nosplit", "cover", "same_prefix",
            "overflow", "mixed", "unifirst"]


def texts(name):
    return [d.text for d in family(name)]


# ---------------------------------------------------------------------------
# the oracle's view

def spans(text: bytes, max_len=MAX_UNITS):
    """[(start, byte length)] of the oracle's tokens (max_len = NO_CUT: before the cut)."""
    cap = len(text) // 2 + 2
    st = np.zeros(cap, np.uint32)
    ln = np.zeros(cap, np.uint32)
    n = O.lib().orc_tokenize(text, len(text), max_len, st.ctypes.data_as(C.POINTER(C.c_uint32)),
                             ln.ctypes.data_as(C.POINTER(C.c_uint32)), cap)
    assert n >= 0, "malformed document in a corpus of this module"
    return list(zip(st[:n].tolist(), ln[:n].tolist()))


def span_units(text: bytes, s, n):
    return units(text[s:s + n].decode())


@functools.lru_cache(maxsize=None)
def oracle_index(name):
    """The family's OracleIndex, built once and shared (never modified)."""
    o = O.OracleIndex()
    for i, t in enumerate(texts(name)):
        o.add_doc(str(i).encode(), t)
    o.commit()
    return o


def run_queries(names):
    """For each run: its first term, its second term (the remainder), and the
    raw run as a query term, which the query analyzer must cut the same way."""
    qs = []
    for nm in names:
        t = RUN[nm].text.encode() if nm in RUN else nm
        toks = O.tokenize(t)
        qs.append(toks[0])
        if len(toks) > 1 and toks[1] not in qs:
            qs.append(toks[1])
        qs.append(t)
    return qs


EXTRA_QUERIES = [b"z" * 255, b"z" * 45, b"z" * 300, b"Z" * 1100, "\u00e9".encode() * 255, "\u00c9".encode() * 300,
                 "\uac00".encode() * 255, "\uac00".encode() * 310, b"z" * 3000, b"alpha1 eps4\xc3\xa9"]


@functools.lru_cache(maxsize=None)
def queries(name):
    """The family's all-hits queries: those of every run in it, and the terms of the documents without one."""
    names = sorted({r for d in family(name) for r in d.runs if r in RUN})
    qs = run_queries(names)
    if not names or name in ("mixed", "unifirst", "cover"):
        qs += EXTRA_QUERIES
    return list(dict.fromkeys(qs))


# ---------------------------------------------------------------------------
# which path takes a document (from the spans and the window arithmetic alone)

def unit_windows(L):
    """[(core_lo, core_hi, window start, window end)] of a document's units (chunk_meta)."""
    out = []
    for k in range((L + CORE - 1) // CORE):
        clo, chi = k * CORE, min(L, (k + 1) * CORE)
        out.append((clo, chi, max(clo - PRE, 0), min(L, chi + POST)))
    return out


def _window_chars(text, ws, we):
    """Non-ASCII characters of the window; one cut by the window's edge is dropped (the kernels blank it)."""
    while ws < we and 0x80 <= text[ws] <= 0xBF:
        ws += 1
    return {c for c in text[ws:we].decode(errors="ignore") if ord(c) >= 0x80}


def chunked(text, config):
    """Does the chunk path keep this document (no unit sends it to
    k_tokenize_long)?  A unit fails on a token over 255 units; an ASCII or
    wave-rule unit also on a token over 255 BYTES that starts in its core; a
    unit with any non-ASCII byte when the Unicode chunk kernel is off; a unit
    of k_tokenize_uchunk when its 64-byte leading margin holds no split byte
    or when a token starting in its core reaches the window's end before the
    document's."""
    L = len(text)
    raw = spans(text, NO_CUT)
    if any(span_units(text, s, n) > MAX_UNITS for s, n in raw):
        return False
    for clo, chi, ws, we in unit_windows(L):
        chars = _window_chars(text, ws, we)
        mine = [(s, n) for s, n in raw if clo <= s < chi]
        if not any(b >= 0x80 for b in text[ws:we]):
            continue                                           # ASCII unit: every token is under 256 bytes here
        if config == "nouchunk":
            return False
        if config != "nouniwave" and chars <= WAVE_CHARS:
            if any(n > MAX_UNITS for _, n in mine):            # the wave rules measure bytes
                return False
            continue
        if clo and b" " not in text[clo - PRE:clo]:
            return False
        if any(s + n >= we and we < L for s, n in mine):
            return False
    return True


def expected_paths(docs, config="default"):
    """{long_docs, long_chunked, unicode_docs, unicode_wave_docs} of a first
    commit, one document per wave (pack_docs == 1 or the retry pass).
    config: "default" (also TFIDF_UW_FULL, which changes nothing counted),
    "nouniwave" (TFIDF_NO_UNIWAVE=1), "nouchunk" (TFIDF_NO_UCHUNK=1)."""
    c = dict(long_docs=0, long_chunked=0, unicode_docs=0, unicode_wave_docs=0)
    for d in docs:
        t = d.text
        L = len(t)
        long_ = False
        if L > WAVE_WINDOW:
            long_ = True                                       # not staged: listed unflagged and uncounted
        else:
            assert L <= 4000, "a length whose window may overflow: see overflow_docs"
            over_bytes = any(n > MAX_UNITS for _, n in spans(t, NO_CUT))
            chars = {ch for ch in t.decode() if ord(ch) >= 0x80}
            if not chars:
                long_ = over_bytes                             # the ASCII wave tokenizer hands a long token over
            else:
                c["unicode_docs"] += 1
                if config != "nouniwave" and chars <= WAVE_CHARS:
                    c["unicode_wave_docs"] += 1
                    long_ = over_bytes                         # counted by bytes there too (é x 200 goes on, uncut)
                # else k_tokenize_uwave: it cuts the token itself
        if long_:
            c["long_docs"] += 1
            c["long_chunked"] += chunked(t, config)
    return c
