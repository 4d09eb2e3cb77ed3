"""Regular-expression search without a device: the shared host/device rules of
csrc/regex_plan.h (the parser, the NFA -> DFA -> minimal canonical table, the
table walk, the scan-chunk plan) are compiled into the stand-alone program
regex_check.cpp with the host compiler under AddressSanitizer and UBSan
(nothing is preloaded) and compared with regex_ref.py, which restates the
contract with derivatives over code points and builds no automaton.  Also: the
header's declarations and the library's exports."""
import ctypes as C
import itertools
import os
import re
import shutil
import struct
import subprocess
import time

import pytest

import regex_ref as R
import wildcard_ref as W
from tfidf_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "tf-idf-distributed-system_amd", "csrc")
NEW = ["tfidf_regex_terms_batch", "tfidf_reader_regex_terms_batch", "tfidf_regex_terms", "tfidf_reader_regex_terms",
       "tfidf_search_regex_batch", "tfidf_reader_search_regex_batch", "tfidf_search_regex",
       "tfidf_reader_search_regex", "tfidf_last_regex_stats", "tfidf_node_regex_terms_batch",
       "tfidf_node_search_regex_batch"]
HASHED = b"zqxjkvwypmnbghtrd"                       # 17 bytes: a hashed key


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("rx") / "regex_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "regex_check.cpp"),
                           "-o", exe])
    return exe


def _s(b):
    return struct.pack("<I", len(b)) + b


def _run(exe, mode, path, blob):
    with open(path, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, mode, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.split("\n")


def run_pairs(exe, path, cases):
    """cases: [(pattern, [subject])] -> [(status, states, classes, [matched])]"""
    blob = struct.pack("<I", len(cases))
    blob += b"".join(_s(p) + struct.pack("<I", len(ss)) + b"".join(_s(s) for s in ss) for p, ss in cases)
    lines = _run(exe, "pairs", path, blob)
    assert lines[len(cases)] == "ok %d" % len(cases)
    out = []
    for ln in lines[:len(cases)]:
        st, ns, nc, bits = ln.split()
        out.append((int(st), int(ns), int(nc), [] if bits == "-" else [c == "1" for c in bits]))
    return out


def run_tables(exe, path, patterns):
    """-> [(status, err_at, table hex or '-')]"""
    lines = _run(exe, "table", path, struct.pack("<I", len(patterns)) + b"".join(_s(p) for p in patterns))
    assert lines[len(patterns)] == "ok %d" % len(patterns)
    return [(int(a), int(b), c) for a, b, c in (ln.split() for ln in lines[:len(patterns)])]


def run_lookup(exe, path, vocab, cases, budget, table_budget):
    """cases: [(max_out, pattern)] -> [([(term, df)], n_matched)]"""
    blob = struct.pack("<III", budget, table_budget, len(vocab))
    blob += b"".join(_s(t) + struct.pack("<I", df) for t, df in vocab.items())
    blob += struct.pack("<I", len(cases)) + b"".join(struct.pack("<I", k) + _s(p) for k, p in cases)
    lines = _run(exe, "lookup", path, blob)
    out, at = [], 0
    for i in range(len(cases)):
        head = lines[at].split()
        assert head[0] == "case" and int(head[1]) == i, lines[at]
        matched, n = int(head[2]), int(head[3])
        rows = [lines[at + 1 + k].split() for k in range(n)]
        out.append(([(bytes.fromhex(r[1]) if len(r) > 1 else b"", int(r[0])) for r in rows], matched))
        at += 1 + n
    assert lines[at] == "ok %d" % len(cases)
    return out


def run_plan(exe, path, sizes, budget):
    blob = struct.pack("<II", len(sizes), budget) + b"".join(struct.pack("<I", v) for v in sizes)
    lines = [x for x in _run(exe, "plan", path, blob) if x]
    assert lines[-1] == "ok %d" % (len(lines) - 1)
    return [int(x) for x in lines[:-1]]


def want(pattern, subjects):
    """(status, [matched]) of the reference"""
    st = R.status(pattern)
    if st != R.OK:
        return st, [False] * len(subjects)
    return st, [R.matches(pattern, s) for s in subjects]


def test_every_small_pattern_against_every_small_string(program, tmp_path):
    patterns = [("".join(p)).encode() for n in range(0, 5) for p in itertools.product("ab.*|()?+", repeat=n)]
    strings = [("".join(p)).encode() for n in range(0, 6) for p in itertools.product("ab", repeat=n)]
    assert len(patterns) == 7381 and len(strings) == 63
    got = run_pairs(program, str(tmp_path / "small.bin"), [(p, strings) for p in patterns])
    n_valid = n_re = 0
    for p, g in zip(patterns, got):
        st, m = want(p, strings)
        assert (g[0], g[3]) == (st, m), p
        if st != R.OK:
            continue
        n_valid += 1
        # an independent restatement for this alphabet: Python's re, where the two grammars agree (a quantifier
        # after a quantifier is lazy or possessive there; an empty alternative is an error here already)
        if re.search(rb"[*?+][*?+]", p):
            continue
        n_re += 1
        rx = re.compile(p.decode(), re.S)
        assert m == [rx.fullmatch(s.decode()) is not None for s in strings], p
    assert n_valid > 1000 and n_re > 700 and n_valid > n_re


U = lambda s: s.encode()                                                        # noqa: E731
HAN, EMOJI = "中", "\U0001F600"
NAMED = [
    # escapes
    (b"a\\*b", b"a*b", 1), (b"a\\*b", b"aab", 0), (b"\\a", b"a", 1), (b"a\\\\b", b"a\\b", 1), (b"\\.", b".", 1),
    (b"\\.", b"a", 0), (b"\\<", b"<", 1), (b"\\(\\)", b"()", 1),
    # classes: '-' first is a literal; negation and '.' take a code point whatever its UTF-8 length
    (b"[-a]", b"-", 1), (b"[-a]", b"a", 1), (b"[-a]", b"b", 0), (b"[a\\-c]", b"-", 1), (b"[a\\-c]", b"b", 0),
    (b"[]a]", b"]", 1), (b"[]a]", b"a", 1), (b"[<&]", b"<", 1), (b"[a-cx-z]", b"y", 1), (b"[a-cx-z]", b"d", 0),
    (b"[^a]", U("é"), 1), (b"[^a]", U(HAN), 1), (b"[^a]", U(EMOJI), 1), (b"[^a]", b"a", 0), (b"[^a]", b"bb", 0),
    (b".", U("é"), 1), (b".", U(HAN), 1), (b".", U(EMOJI), 1), (b"..", U(EMOJI), 0), (b"..", U("é"), 0),
    (b"...", U(HAN), 0), (b"a.b", U("a" + EMOJI + "b"), 1), (b"a..b", U("a" + EMOJI + "b"), 0),
    (b"[^a]*", U("é" + HAN + EMOJI), 1), (b"[^a]{3}", U("é" + HAN + EMOJI), 1), (b"[^a]{4}", U("é" + HAN + EMOJI), 0),
    (b"[^^]", b"^", 0), (b"[^^]", b"a", 1), (b"[a^]", b"^", 1),
    # a range across the 1/2/3/4-byte UTF-8 boundaries
    (U("[\x7f-\x80]"), b"\x7f", 1), (U("[\x7f-\x80]"), U("\x80"), 1), (U("[\x7f-\x80]"), b"~", 0),
    (U("[߿-ࠀ]"), U("߿"), 1), (U("[߿-ࠀ]"), U("ࠀ"), 1), (U("[߿-ࠀ]"), U("ࠁ"), 0),
    (U("[￿-\U00010000]"), U("￿"), 1), (U("[￿-\U00010000]"), U("\U00010000"), 1),
    (U("[￿-\U00010000]"), U("￾"), 0), (U("[z-\U0001F600]"), U("é"), 1), (U("[z-\U0001F600]"), U(HAN), 1),
    (U("[z-\U0001F600]"), U(EMOJI), 1), (U("[z-\U0001F600]"), U("\U0001F601"), 0), (U("[z-\U0001F600]"), b"y", 0),
    (U("[à-ÿ]+"), U("éàü"), 1), (U("[à-ÿ]+"), U("éaü"), 0),
    # repeats
    (b"a{2}", b"aa", 1), (b"a{2}", b"a", 0), (b"a{2}", b"aaa", 0), (b"a{2,}", b"a", 0), (b"a{2,}", b"aaaaa", 1),
    (b"a{1,3}", b"", 0), (b"a{1,3}", b"aaa", 1), (b"a{1,3}", b"aaaa", 0), (b"a{2,1}", b"a", 0), (b"a{2,1}", b"aa", 0),
    (b"a{2,1}", b"", 0), (b"a{0}", b"", 1), (b"a{0}", b"a", 0), (b"(ab){2}c", b"ababc", 1), (b"ab{2}", b"abb", 1),
    (b"a+?", b"", 1), (b"a+?", b"aa", 1), (b"a**", b"aaa", 1), (b"a?{2}", b"aa", 1), (b"a?{2}", b"aaa", 0),
    # no anchors
    (b"^a$", b"^a$", 1), (b"^a$", b"a", 0), (b"a$", b"a$", 1),
    # complement, intersection, any string, the empty language, quotes, the empty string
    (b"~a", b"a", 0), (b"~a", b"", 1), (b"~a", b"aa", 1), (b"~a", b"b", 1), (b"~(ab)c", b"c", 1), (b"~(ab)c", b"abc", 0),
    (b"~~a", b"a", 1), (b"~([ab]*)", b"abc", 1), (b"~([ab]*)", b"abab", 0),
    (b"~[ab]*", b"abab", 1), (b"~[ab]*", b"a", 0),                             # the repeat takes the complement
    (b"a.*&.*b", b"ab", 1), (b"a.*&.*b", b"axxb", 1), (b"a.*&.*b", b"ba", 0), (b"[a-c]+&~(abc)", b"abc", 0),
    (b"[a-c]+&~(abc)", b"acb", 1), (b"a|b&c", b"a", 1), (b"a|b&c", b"b", 0), (b"a&b|c", b"c", 1),
    (b"@", b"", 1), (b"@", U("x" + EMOJI), 1), (b"a@", b"a", 1), (b"a@b", b"axyzb", 1), (b"a@b", b"axyz", 0),
    (b"#", b"", 0), (b"#", b"a", 0), (b"a|#", b"a", 1), (b"a#", b"a", 0), (b"#*", b"", 1), (b"~#", b"zz", 1),
    (b'"a*b"', b"a*b", 1), (b'"a*b"', b"aab", 0), (b'"a*b"', b"b", 0), (b'""', b"", 1), (b'"<"', b"<", 1),
    (b'"\\"', b"\\", 1), (b'x"(|"y', b"x(|y", 1),
    (b"()", b"", 1), (b"()", b"a", 0), (b"a()b", b"ab", 1), (b"()*", b"", 1),
    (b"", b"", 1), (b"", b"a", 0),
    # predefined classes, outside brackets only
    (b"\\d", b"7", 1), (b"\\d", b"a", 0), (b"\\d", U("٣"), 0), (b"\\D", b"7", 0), (b"\\D", b"a", 1), (b"\\D", U(EMOJI), 1),
    (b"\\D", b"ab", 0), (b"\\s", b" ", 1), (b"\\s", b"\t", 1), (b"\\s", b"\n", 1), (b"\\s", b"\r", 1), (b"\\s", b"\x0b", 0),
    (b"\\S", b" ", 0), (b"\\S", b"x", 1), (b"\\w", b"_", 1), (b"[A-Z]", b"z", 0), (b"\\w", b"q", 1), (b"\\w", b"5", 1),
    (b"\\w", b"-", 0), (b"\\w", U("é"), 0), (b"\\W", U("é"), 1), (b"\\W", b"a", 0), (b"\\w+\\d{3}", b"err404", 1),
    (b"[\\d]", b"d", 1), (b"[\\d]", b"7", 0), (b"[-\\w]", b"w", 1), (b"[-\\w]", b"a", 0),
    (b"(error|warn)[0-9]{3}", b"warn404", 1), (b"(error|warn)[0-9]{3}", b"warn40", 0), (b"[a-z]+ing", b"testing", 1),
    (b"[a-z]+ing", b"ing", 0), (b".*[0-9]", b"abc7", 1), (b".*[0-9]", b"abc", 0),
    # the pattern is not lower-cased (the subjects are vocabulary terms: lower-case)
    (b"Foo.*", b"foo", 0), (b"foo.*", b"foo", 1), (b"[A-Z]oo", b"foo", 0),
    # not strict UTF-8: matches nothing, no error
    (b"a\xff.*", b"a", 0), (b"\xed\xa0\x80", b"a", 0), (b".*\xc3", b"a", 0), (b"\xc0\xaf", b"/", 0), (b"(\xff", b"", 0),
]
SYNTAX = [b"(", b"(a", b"a)", b")", b"[a", b"[", b"[]", b"[^]", b"[^", b'"a', b'"', b"a{", b"a{}", b"a{x}", b"a{,2}", b"a{2",
          b"a{2,", b"a{2,3", b"a{2 }", b"a\\", b"\\", b"[a\\", b"*", b"*a", b"+a", b"?", b"{2}", b"a|*", b"(*)", b"a|", b"|a",
          b"a||b", b"(|a)", b"(a|)", b"a&", b"&a", b"~", b"a~", b"[a-]", b"[b-a]", b"[z-a]x", b"]", b"}", b"a]", b"a}",
          b"(a))", b"(()"]
UNSUPPORTED = [b"<", b"<1-5>", b"a<b", b"<name>", b"(a|<)", b"~<", b"a{2}<"]


def test_pairs_that_separate_the_rules(program, tmp_path):
    got = run_pairs(program, str(tmp_path / "named.bin"), [(p, [c]) for p, c, _ in NAMED])
    for (p, c, w), g in zip(NAMED, got):
        assert (g[0], g[3]) == (R.OK, [bool(w)]), (p, c)
        assert want(p, [c]) == (R.OK, [bool(w)]), (p, c)                         # and the reference says the same
    bad = SYNTAX + UNSUPPORTED
    got = run_tables(program, str(tmp_path / "bad.bin"), bad)
    for p, g in zip(bad, got):
        assert g[0] == (R.SYNTAX if p in SYNTAX else R.UNSUPPORTED) == R.status(p), p
        assert g[2] == "-" and 0 <= g[1] <= len(p), p                           # no table; the offset lies in the pattern
    assert dict(zip(bad, got))[b"a|"][1] == 2 and dict(zip(bad, got))[b"[b-a]"][1] == 4 and dict(zip(bad, got))[b"a<b"][1] == 1


def test_minimal_tables_are_canonical(program, tmp_path):
    same = [(b"a|a", b"a"), (b"(ab)*(ab)*", b"(ab)*"), (b"[a-c]", b"a|b|c"), (b"~(~a)", b"a"), (b"a&.", b"a"),
            (b"a+?", b"a*"), (b"a{2,}", b"aaa*"), (U("[^é]"), U("[\x00-è]|[ê-\U0010ffff]")), (b"\\w", b"[a-z]|[A-Z_]|\\d"),
            (b"(a|b)*", b"(a*b*)*"), (b"@", b".*"), (b"#", b"a&b"), (b"a{2,1}", b"#"), (b'"ab"', b"ab"), (b"()", b""),
            (b"a.*&.*b", b"a(.*b)?&~a|ab|a.*b")]
    differ = [(b"a", b"b"), (b"a*", b"a+"), (b"[a-c]", b"[a-d]"), (b".", b"[^a]")]
    flat = [p for pair in same + differ for p in pair]
    tabs = run_tables(program, str(tmp_path / "tables.bin"), flat)
    assert all(t[0] == R.OK and t[2] != "-" for t in tabs)
    by = dict(zip(flat, (t[2] for t in tabs)))
    for a, b in same:
        assert by[a] == by[b], (a, b)
    for a, b in differ:
        assert by[a] != by[b], (a, b)
    # 'a': dead + 2 live states; 'a', everything below it and everything above it: 2 classes after merging
    words = [int(by[b"a"][i:i + 8], 16) for i in range(0, len(by[b"a"]), 8)]
    assert words[0] == len(words) and words[1] == 3 | (2 << 16) and words[3] == 1 and words[4:6] == [1, 1]
    words = [int(by[b"#"][i:i + 8], 16) for i in range(0, len(by[b"#"]), 8)]
    assert words[1] == 1 | (1 << 16) and words[3] == 0                          # the empty language: the dead state alone
    words = [int(by[b"a*"][i:i + 8], 16) for i in range(0, len(by[b"a*"]), 8)]
    assert words[4:6] == [0, 0xFFFFFFFF]                                        # no longest member


def test_the_complexity_limit(program, tmp_path):
    def hard(k):
        return b"(a|b)*a(a|b){%d}" % k
    subjects = [("".join(p)).encode() for n in (7, 8, 9, 10) for p in itertools.product("ab", repeat=n)][::7]
    got = run_pairs(program, str(tmp_path / "k7.bin"), [(hard(7), subjects)])[0]
    assert got[0] == R.OK and got[1] == 257 and got[2] == 3                     # 2^8 live states and the dead one
    assert got[3] == want(hard(7), subjects)[1] and 0 < sum(got[3]) < len(subjects)
    # 256 states and 32 classes are within the limit
    wide = b"".join(b"[%c%c]" % (97 + i, 65 + i) for i in range(26)) + b"[0-4][5-9][-_][!?][%:]" + b".{224}"
    got = run_pairs(program, str(tmp_path / "wide.bin"), [(wide, [])])[0]
    assert got[0] == R.OK and got[1] == 257 and got[2] == 32
    # a long chain is within the limits: its table is small, and minimising it costs a step per state
    got = run_pairs(program, str(tmp_path / "chain.bin"), [(b"a{2100}", []), (b"~(a{3000})", [b"a", b""])])
    assert [g[:3] for g in got] == [(R.OK, 2102, 2), (R.OK, 3003, 2)] and got[1][3] == [True, True]

    def nest(depth, stars):
        return b"~(" * depth + b"a" + (b")" + b"*" * stars) * depth
    over = [hard(16), hard(40), b"(a{1000}){1000}", b"((a{100}){100}){100}", b"(((((a*)*b)*c)*d){50}){50}", b"a{99999999999}",
            b".{1000000}", b"(" * 300 + b"a" + b")" * 300, b"~" * 300 + b"a",
            b"[a-b]" + b"".join(U("[%c-%c]" % (0x100 + 3 * i, 0x101 + 3 * i)) for i in range(600)),
            # runs of repeat operators nest a syntax node each, also under complements that start automata of
            # their own: past the height limit, never as deep as the stack
            nest(8, 3000), nest(20, 3000), nest(40, 1000), nest(90, 400), b"a" + b"*" * 3500, b"a" + b"?" * 3500,
            b"a" + b"{1}" * 250, b"(a|b)" + b"+?" * 150, b"~(a&~(b&~(c" + b"*" * 300 + b")))"]
    for i, p in enumerate(over):                                                # each on its own: status and time
        t0 = time.monotonic()
        got = run_tables(program, str(tmp_path / ("over%d.bin" % i)), [p])
        took = time.monotonic() - t0
        print("%-40s %.3f s" % (p[:40], took))
        assert got[0][0] == R.UNSUPPORTED and got[0][2] == "-", p[:60]
        assert took < 0.5, p[:60]                                               # with the process start, sanitizers on
    deep = b"a" + b"*" * 150                                                    # within the height limit
    assert run_pairs(program, str(tmp_path / "deep.bin"), [(deep, [b"aaa", b"b"])])[0][3] == [True, False]


DENSE_PATTERNS = [b".*", b"a.*", b".*c", b"a.c.*", b"..", b"abc", HASHED + b".*", HASHED[:9] + b".*", b"lmnoplmnop.*",
                  b"caf.", b"caf.*", b"", b"\xff.*", b".{256}", b".*nop", b"ZQ.*", "àé.*".encode(), ".*ñ".encode(), b".",
                  b"a.*b.*c", b"x", b"nothing.*", b".*lmnop.*", b"@", b"#", b"[ab]{2,3}", b"(ab|ba)+c?", b"[^a-c]+",
                  "caf[é-ë]".encode(), "[^\x00-\x7f]+".encode(), b"~(a.*)&[a-c]{1,2}", b"(a|b)*a(a|b){3}", b"[a-c]*[^c]",
                  b".{17}", b"\\w{17,}"]


def test_lookup_over_the_dense_vocabulary(program, tmp_path):
    vocab = W.dense_vocab()
    want_all = {p: R.expected_terms(vocab, p, 1 << 30) for p in DENSE_PATTERNS}
    for budget, table_budget in ((1, 1), (50, 2000), (1 << 22, 1 << 20)):
        cases = [(k, p) for k in (1, 5, 1024) for p in DENSE_PATTERNS]
        got = run_lookup(program, str(tmp_path / "lookup.bin"), vocab, cases, budget, table_budget)
        for c, g in zip(cases, got):
            assert g == (want_all[c[1]][0][:c[0]], want_all[c[1]][1]), c
    # the fixture reaches its cases
    assert want_all[b".*"][1] == want_all[b"@"][1] == len(vocab) > 1024
    assert want_all[b"#"] == want_all[b""] == want_all[b"\xff.*"] == want_all[b".{256}"] == want_all[b"ZQ.*"] == ([], 0)
    assert [t for t, _ in want_all[b"caf."][0]] == [b"cafe", "café".encode()]
    assert [t for t, _ in want_all["caf[é-ë]".encode()][0]] == ["café".encode()]
    assert want_all[HASHED + b".*"][1] == 2 and want_all[b".{17}"][1] >= 1          # hashed terms match
    assert all(len(t) >= 17 for t, _ in want_all[b"\\w{17,}"][0]) and want_all[b"\\w{17,}"][1] >= 1
    assert {W.HAN, W.EMOJI} <= {t for t, _ in want_all[b"."][0]}
    ties = want_all[b"a.*"][0]
    assert len({df for _, df in ties}) < len(ties)
    assert 0 < want_all[b"(a|b)*a(a|b){3}"][1] < want_all[b"[a-c]*[^c]"][1]


def test_table_scan_chunk_plan(program, tmp_path):
    path = str(tmp_path / "plan.bin")
    sizes = [700] * 9 + [0, 640] * 200 + [16448, 32768, 32768, 700] + [0] * 300 + [32768]
    for budget in (1, 700, 2000, 32768, 1 << 30):
        cuts = run_plan(program, path, sizes, budget)
        assert cuts[0] == 0 and cuts[-1] == len(sizes) and cuts == sorted(set(cuts))
        for a, z in zip(cuts, cuts[1:]):
            assert z - a <= 128
            assert sum(sizes[a:z]) <= min(budget, 32768) or sum(1 for x in sizes[a:z] if x) == 1
    assert len(run_plan(program, path, sizes, 1)) - 1 >= sum(1 for x in sizes if x)   # one table per scan
    assert run_plan(program, path, sizes, 1 << 30) == run_plan(program, path, sizes, 32768)   # never past the staging area
    assert run_plan(program, path, [], 5) == [0]


def test_header_declares_and_library_exports_the_regex_calls():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "tfidf.h")).read(), flags=re.S)
    lib = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
