"""Reference for regular-expression search (tfidf_regex_terms*,
tfidf_search_regex*), written from the contract in DESIGN.md §2 alone: a
recursive-descent parser of the grammar and a matcher by Brzozowski
derivatives over code points, with no automaton anywhere (complement and
intersection are derivative rules of their own).  The terms of a pattern come
from brute force over a vocabulary {term: df}, its documents from brute force
over the documents' term sets."""
import functools

RESERVED = set('|&?*+{}[]().#@"~\\<')
MAX_CP = 0x10FFFF


class RegexSyntax(Exception):
    pass


class RegexUnsupported(Exception):
    pass


# ---------------------------------------------------------------------------
# expressions, hash-consed: an expression is an index into _NODES
_NODES, _IDS = [], {}


def _mk(*t):
    i = _IDS.get(t)
    if i is None:
        i = _IDS[t] = len(_NODES)
        _NODES.append(t)
    return i


NONE = _mk("none")          # the empty language
EPS = _mk("eps")            # the empty string
ANYSTR = _mk("not", NONE)   # every string


def mk_set(ranges, neg=False):
    """one code point in (or, neg, outside) the inclusive ranges"""
    return _mk("set", tuple(sorted(ranges)), bool(neg))


def mk_cat(a, b):
    if a == NONE or b == NONE:
        return NONE
    if a == EPS:
        return b
    if b == EPS:
        return a
    return _mk("cat", a, b)


def _flat(kind, items):
    out = set()
    for x in items:
        if _NODES[x][0] == kind:
            out.update(_NODES[x][1])
        else:
            out.add(x)
    return out


def mk_alt(items):
    s = _flat("alt", items)
    s.discard(NONE)
    if ANYSTR in s:
        return ANYSTR
    if not s:
        return NONE
    if len(s) == 1:
        return next(iter(s))
    return _mk("alt", tuple(sorted(s)))


def mk_and(items):
    s = _flat("and", items)
    s.discard(ANYSTR)
    if NONE in s:
        return NONE
    if not s:
        return ANYSTR
    if len(s) == 1:
        return next(iter(s))
    return _mk("and", tuple(sorted(s)))


def mk_not(a):
    if _NODES[a][0] == "not":
        return _NODES[a][1]
    return _mk("not", a)


def mk_star(a):
    if a in (NONE, EPS):
        return EPS
    if _NODES[a][0] == "star":
        return a
    return _mk("star", a)


def mk_repeat(a, lo, hi):
    """a{lo,hi}; hi None: no upper end"""
    if hi is not None and hi < lo:
        return NONE
    out = mk_star(a) if hi is None else EPS
    if hi is not None:
        opt = mk_alt([a, EPS])
        for _ in range(hi - lo):
            out = mk_cat(opt, out)
    for _ in range(lo):
        out = mk_cat(a, out)
    return out


@functools.lru_cache(maxsize=None)
def nullable(r):
    n = _NODES[r]
    k = n[0]
    if k in ("eps", "star"):
        return True
    if k in ("none", "set"):
        return False
    if k == "cat":
        return nullable(n[1]) and nullable(n[2])
    if k == "alt":
        return any(nullable(x) for x in n[1])
    if k == "and":
        return all(nullable(x) for x in n[1])
    return not nullable(n[1])                     # not


@functools.lru_cache(maxsize=None)
def deriv(r, cp):
    """the expression of {w : cp w in L(r)}"""
    n = _NODES[r]
    k = n[0]
    if k in ("none", "eps"):
        return NONE
    if k == "set":
        inside = any(lo <= cp <= hi for lo, hi in n[1])
        return EPS if inside != n[2] else NONE
    if k == "cat":
        d = mk_cat(deriv(n[1], cp), n[2])
        return mk_alt([d, deriv(n[2], cp)]) if nullable(n[1]) else d
    if k == "alt":
        return mk_alt([deriv(x, cp) for x in n[1]])
    if k == "and":
        return mk_and([deriv(x, cp) for x in n[1]])
    if k == "star":
        return mk_cat(deriv(n[1], cp), r)
    return mk_not(deriv(n[1], cp))                # not


def match(expr, cps):
    """Does the whole code point sequence belong to the expression's language?"""
    for cp in cps:
        expr = deriv(expr, cp)
        if expr == NONE:
            return False
    return nullable(expr)


# ---------------------------------------------------------------------------
# the parser


class _Parser:
    def __init__(self, s):
        self.s, self.i = s, 0

    def more(self):
        return self.i < len(self.s)

    def peek(self, c):
        return self.more() and self.s[self.i] == c

    def take(self, c):
        if self.peek(c):
            self.i += 1
            return True
        return False

    def union(self):
        items = [self.inter()]
        while self.take("|"):
            items.append(self.inter())
        return mk_alt(items) if len(items) > 1 else items[0]

    def inter(self):
        items = [self.concat()]
        while self.take("&"):
            items.append(self.concat())
        return mk_and(items) if len(items) > 1 else items[0]

    def concat(self):
        items = [self.repeat()]                   # one at least: `a|`, `(|a)` and `` inside `(`..`)` are errors
        while self.more() and self.s[self.i] not in ")|&":
            items.append(self.repeat())
        out = EPS
        for x in reversed(items):
            out = mk_cat(x, out)
        return out

    def integer(self):
        j = self.i
        while self.more() and self.s[self.i] in "0123456789":
            self.i += 1
        if j == self.i:
            raise RegexSyntax("'{' without an integer at %d" % j)
        return int(self.s[j:self.i])

    def repeat(self):
        e = self.compl()
        while True:
            if self.take("?"):
                e = mk_repeat(e, 0, 1)
            elif self.take("*"):
                e = mk_repeat(e, 0, None)
            elif self.take("+"):
                e = mk_repeat(e, 1, None)
            elif self.take("{"):
                lo = hi = self.integer()
                if self.take(","):
                    hi = self.integer() if self.more() and self.s[self.i] in "0123456789" else None
                if not self.take("}"):
                    raise RegexSyntax("'{' without '}'")
                e = mk_repeat(e, lo, hi)
            else:
                return e

    def compl(self):
        if self.take("~"):
            return mk_not(self.compl())
        return self.klass()

    def charexp(self, in_class):
        if not self.more():
            raise RegexSyntax("a character expected at the end")
        c = self.s[self.i]
        if c == "\\":
            if self.i + 1 >= len(self.s):
                raise RegexSyntax("a dangling backslash")
            self.i += 2
            return ord(self.s[self.i - 1])
        if not in_class and c in RESERVED:
            if c == "<":
                raise RegexUnsupported("'<' at %d" % self.i)
            raise RegexSyntax("reserved %r at %d" % (c, self.i))
        self.i += 1
        return ord(c)

    def klass(self):
        if not self.take("["):
            return self.simple()
        neg = self.take("^")
        ranges = []
        while True:                               # the first item always, then until ']'
            lo = hi = self.charexp(True)
            if self.take("-"):
                hi = self.charexp(True)
                if hi < lo:
                    raise RegexSyntax("a range that runs down")
            ranges.append((lo, hi))
            if not self.more() or self.peek("]"):
                break
        if not self.take("]"):
            raise RegexSyntax("'[' without ']'")
        return mk_set(ranges, neg)

    PREDEFINED = {"d": [(48, 57)], "s": [(9, 10), (13, 13), (32, 32)], "w": [(48, 57), (65, 90), (95, 95), (97, 122)]}

    def simple(self):
        if not self.more():
            raise RegexSyntax("an expression expected at the end")
        if self.take("."):
            return mk_set([(0, MAX_CP)])
        if self.take("#"):
            return NONE
        if self.take("@"):
            return ANYSTR
        if self.take('"'):
            j = self.s.find('"', self.i)
            if j < 0:
                raise RegexSyntax("'\"' without its partner")
            lit, self.i = self.s[self.i:j], j + 1
            out = EPS
            for c in reversed(lit):
                out = mk_cat(mk_set([(ord(c), ord(c))]), out)
            return out
        if self.take("("):
            if self.take(")"):
                return EPS
            e = self.union()
            if not self.take(")"):
                raise RegexSyntax("'(' without ')'")
            return e
        if self.peek("\\") and self.i + 1 < len(self.s) and self.s[self.i + 1] in "dDsSwW":
            c = self.s[self.i + 1]
            self.i += 2
            return mk_set(self.PREDEFINED[c.lower()], c.isupper())
        c = self.charexp(False)
        return mk_set([(c, c)])


def parse(pattern: bytes):
    """The expression of a pattern; None for one that is not strict UTF-8 (it
    matches nothing).  Raises RegexSyntax / RegexUnsupported."""
    try:
        s = pattern.decode("utf-8")
    except UnicodeDecodeError:
        return None
    if s == "":
        return EPS
    p = _Parser(s)
    e = p.union()
    if p.more():
        raise RegexSyntax("an unbalanced ')' at %d" % p.i)
    return e


OK, SYNTAX, UNSUPPORTED = 0, 1, 2


def status(pattern: bytes):
    try:
        parse(pattern)
    except RegexSyntax:
        return SYNTAX
    except RegexUnsupported:
        return UNSUPPORTED
    return OK


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


def from_wildcard(pattern: bytes):
    """The regular expression of a wildcard pattern of wildcard_ref: `*` -> `.*`,
    `?` -> `.`, `\\x` and literals lower-cased (reserved ones escaped) as the wildcard calls
    lower-case theirs.  None where the pattern is not UTF-8."""
    from oracle import oracle as O
    try:
        s = pattern.decode("utf-8")
    except UnicodeDecodeError:
        return None
    out, i = [], 0
    while i < len(s):
        c = s[i]
        i += 1
        if c == "*":
            out.append(".*")
        elif c == "?":
            out.append(".")
        else:
            if c == "\\" and i < len(s):
                c = s[i]
                i += 1
            c = O.lower_utf8(c.encode("utf-8")).decode("utf-8")
            out.append("\\" + c if c in RESERVED else c)
    return "".join(out).encode("utf-8")
