"""Batched hit highlighting without a device: the batch side of
csrc/snippet_plan.h (per-query key segments, the row-chunk planner) compiled
into the stand-alone program highlight_batch_check.cpp with the host compiler
under AddressSanitizer and UBSan (nothing is preloaded) and compared with
highlight_ref.py; and the header's declarations, the library's exports and
the Python signatures of the six new calls."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import pytest

import highlight_ref as H
from tfidf_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "tf-idf-distributed-system_amd", "csrc")
NEW = ["tfidf_reader_matches_batch", "tfidf_reader_snippets_batch", "tfidf_matches_batch", "tfidf_snippets_batch",
       "tfidf_node_matches_batch", "tfidf_node_snippets_batch"]
BIG = 1 << 60
EDGE_LENGTHS = [0, 1, 16383, 16384, 16385, 70000]
CORPORA = ["unicode", "ops", "seventy", "malformed", "twins", "dense"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("hlb") / "highlight_batch_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "highlight_batch_check.cpp"),
                           "-o", exe])
    return exe


@pytest.fixture(scope="module")
def case():
    """(documents, queries as term lists, rows (query, document)): every
    query on every document."""
    docs = []
    for name in CORPORA:
        docs += list(H.corpus(name)[0])
    edge = H.corpus("edge")[0]
    for n in EDGE_LENGTHS:
        docs.append(edge[H.LENGTHS.index(n)])
    assert [len(d) for d in docs[-6:]] == EDGE_LENGTHS
    queries = [H.corpus(name)[2] for name in CORPORA + ["edge"]]
    queries.append([])                                              # an empty segment
    queries.append([b"alpha", b"gamma"])                            # one term, two ordinals: alpha 0 here ...
    queries.append([b"gamma", b"zzabsent", b"alpha"])               # ... and 2 here
    rows = [(q, d) for q in range(len(queries)) for d in range(len(docs))]
    return docs, queries, rows


@pytest.fixture(scope="module")
def expected(case):
    docs, queries, rows = case
    return {(q, d): H.matches(docs[d], queries[q]) for q, d in rows}


def run_scan(exe, path, W, budget_items, budget_matches, docs, queries, rows):
    with open(path, "wb") as f:
        f.write(struct.pack("<IQQ", W, budget_items, budget_matches))
        f.write(struct.pack("<I", len(queries)))
        for terms in queries:
            f.write(struct.pack("<I", len(terms)))
            for o, t in enumerate(terms):
                f.write(struct.pack("<II", o, len(t)) + t)
        f.write(struct.pack("<I", len(docs)))
        for t in docs:
            f.write(struct.pack("<IQ", int(H.doc_tokens(t) is None), len(t)) + t)
        f.write(struct.pack("<I", len(rows)))
        for q, d in rows:
            f.write(struct.pack("<II", q, d))
    r = subprocess.run([exe, "scan", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    out, at = [], 0
    for i in range(len(rows)):
        head = lines[at].split()
        assert head[0] == "row" and int(head[1]) == i, lines[at]
        n, a, b = int(head[2]), int(head[3]), int(head[4])
        out.append(([tuple(int(x) for x in lines[at + 1 + k].split()) for k in range(n)], a, b))
        at += 1 + n
    chunks = lines[at].split()
    assert chunks[0] == "chunks" and lines[at + 1] == "ok %d" % len(rows)
    return out, int(chunks[1]), int(chunks[2])


def check(got, W, case, expected, rows=None):
    docs, queries, all_rows = case
    for (q, d), (ms, a, b) in zip(all_rows if rows is None else rows, got):
        want = expected[(q, d)]
        assert ms == want, (W, q, d)
        assert (a, b) == H.snippet(docs[d], want, W)[:2], (W, q, d)


@pytest.mark.parametrize("W", [16, 160, 1024])
def test_segment_scan_gives_every_rows_own_matches_and_snippet(program, tmp_path, case, expected, W):
    got, n_item_chunks, n_match_chunks = run_scan(program, str(tmp_path / "c.bin"), W, BIG, BIG, *case)
    assert (n_item_chunks, n_match_chunks) == (1, 1)
    check(got, W, case, expected)


def test_the_case_list_holds_what_it_is_for(case, expected):
    docs, queries, rows = case
    nq, nd = len(queries), len(docs)
    assert all(expected[(nq - 3, d)] == [] for d in range(nd))                          # the empty segment
    d = docs.index(H.corpus("dense")[0][0])
    a, b = expected[(nq - 2, d)], expected[(nq - 1, d)]
    assert [(s, l) for s, l, _ in a] == [(s, l) for s, l, _ in b] and len(a) > 5000
    assert {o for _, _, o in a} == {0, 1} and {o for _, _, o in b} == {0, 2}            # the same terms, other ordinals
    assert [o for _, _, o in a[:2]] == [0, 1] and [o for _, _, o in b[:2]] == [2, 0]
    own = {name: i for i, name in enumerate(CORPORA)}
    for name in CORPORA:                                                                # own queries find their corpus
        texts = H.corpus(name)[0]
        base = docs.index(texts[0])
        assert [expected[(own[name], base + i)] for i in range(len(texts))] == H.expected_matches(name)
    assert any(expected[(own["ops"], docs.index(t))] for t in H.corpus("unicode")[0])   # and other corpora's documents
    assert expected[(len(CORPORA), nd - 1)] and len(docs[nd - 1]) == 70000


@pytest.mark.parametrize("budget_items, budget_matches", [(1, BIG), (3, BIG), (BIG, 1), (BIG, 7), (3, 100), (1, 1)])
def test_chunked_scan_is_the_unchunked_scan(program, tmp_path, case, expected, budget_items, budget_matches):
    """Chunk edges inside a query's rows and between queries; the 70 000-byte
    document (5 items) and dense's ~5 200-match row are chunks of their own."""
    docs, queries, rows = case
    nd = len(docs)
    keep = [r for r in rows if r[0] in (0, 1, 5, 6, 7, 8, 9)]                           # own, cross, empty, ordinals
    got, n_item_chunks, n_match_chunks = run_scan(program, str(tmp_path / "c.bin"), 160, budget_items, budget_matches,
                                                  docs, queries, keep)
    check(got, 160, case, expected, keep)
    assert n_match_chunks >= n_item_chunks
    if budget_items != BIG:
        assert n_item_chunks > len(queries)
    if budget_matches != BIG:
        assert n_match_chunks > nd


def plan(exe, path, items, matches, bi, bm):
    R = len(items)
    with open(path, "wb") as f:
        f.write(struct.pack("<IQQ", R, bi, bm))
        f.write(struct.pack("<%dQ" % R, *items) + struct.pack("<%dQ" % R, *matches))
    r = subprocess.run([exe, "plan", path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[1] == "ok"
    return [int(x) for x in lines[0].split()]


def check_plan(cuts, items, matches, bi, bm):
    R = len(items)
    assert cuts[0] == 0 and cuts[-1] == R                                               # all rows ...
    assert all(a < b for a, b in zip(cuts, cuts[1:]))                                   # ... once, in order, no empty range
    if R == 0:
        assert cuts == [0]
    for a, b in zip(cuts, cuts[1:]):
        if b - a > 1:                                                                   # both budgets, but for single rows
            assert sum(items[a:b]) <= bi and sum(matches[a:b]) <= bm, (cuts, a, b)
    for k in range(1, len(cuts) - 1):                                                   # greedy: no cut that was not needed
        a, c = cuts[k - 1], cuts[k]
        assert sum(items[a:c + 1]) > bi or sum(matches[a:c + 1]) > bm, (cuts, k)


def test_chunk_planner(program, tmp_path):
    path = str(tmp_path / "p.bin")
    shapes = {0: ([], []), 1: ([2], [5]), 2: ([1, 1], [0, 4]),
              7: ([1, 0, 2, 5, 1, 1, 0], [3, 0, 1, 2, 9, 0, 0])}                         # zero items; 5 items, 9 matches alone
    for R, (items, matches) in shapes.items():
        for bi in (1, 3):
            for bm in (1, 3):
                cuts = plan(program, path, items, matches, bi, bm)
                check_plan(cuts, items, matches, bi, bm)
        assert plan(program, path, items, matches, BIG, BIG) == ([0, R] if R else [0])   # one range
        # one budget alone
        check_plan(plan(program, path, items, matches, 3, BIG), items, matches, 3, BIG)
        check_plan(plan(program, path, items, matches, BIG, 3), items, matches, BIG, 3)
    items, matches = shapes[7]
    assert plan(program, path, items, matches, 3, BIG) == [0, 3, 4, 7]                   # the 5-item row alone
    assert plan(program, path, items, matches, BIG, 3) == [0, 2, 4, 5, 7]                # the 9-match row alone
    assert plan(program, path, items, matches, 1, 1) == [0, 1, 2, 3, 4, 5, 7]


def test_header_declares_library_exports_and_signatures_list_the_new_calls():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "tfidf.h")).read(), flags=re.S)
    lib = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
        # the declaration's parameters and the ctypes list agree in number
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name][1]), name
