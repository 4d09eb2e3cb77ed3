"""Fuzzy search without a device: the shared host/device rules of
csrc/fuzzy_search_plan.h (the m > ed test, the boost float, the sort key, the
byte comparison of two candidates through the dictionary cursors, the
straddling-group selection) are compiled into the stand-alone program
fuzzy_search_check.cpp with the host compiler under AddressSanitizer and UBSan
(nothing is preloaded) and compared with fuzzy_search_ref.py.  Also: the
header's declarations and the library's exports."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import fuzzy_ref as F
import fuzzy_search_ref as R
from tfidf_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "tf-idf-distributed-system_amd", "csrc")
NEW = ["tfidf_fuzzy_expand_batch", "tfidf_reader_fuzzy_expand_batch", "tfidf_fuzzy_expand",
       "tfidf_reader_fuzzy_expand", "tfidf_search_fuzzy_batch", "tfidf_reader_search_fuzzy_batch",
       "tfidf_search_fuzzy", "tfidf_reader_search_fuzzy", "tfidf_node_search_fuzzy_batch"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("fzs") / "fuzzy_search_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "fuzzy_search_check.cpp"), "-o", exe])
    return exe


def _s(b):
    return struct.pack("<I", len(b)) + b


def _run(exe, mode, path=None, blob=None):
    args = [exe, mode]
    if path is not None:
        with open(path, "wb") as f:
            f.write(blob)
        args.append(path)
    r = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.split("\n")


def test_boost_and_keep_for_every_distance_and_length(program):
    lines = _run(program, "boost")
    rows = [x.split() for x in lines[:3 * 255]]
    assert lines[3 * 255] == "ok" and len(rows) == 765
    got = {}
    for ed, m, keep, bits, key in rows:
        got[(int(ed), int(m))] = (keep == "1", int(bits, 16), int(key, 16))
    assert sorted(got) == [(ed, m) for ed in (0, 1, 2) for m in range(1, 256)]
    for (ed, m), (keep, bits, _) in got.items():
        assert keep == R.keep(ed, m) == (m > ed)
        if keep:
            assert bits == int(R.boost(ed, m).view(np.uint32)), (ed, m)
    assert got[(0, 7)][1] == 0x3F800000 and got[(2, 4)][1] == 0x3F000000 == got[(1, 2)][1]
    assert not got[(1, 1)][0] and not got[(2, 2)][0] and not got[(2, 1)][0] and got[(2, 3)][0]


def test_key_order_is_boost_descending(program):
    """Ascending keys = descending boost = ascending ed / m as a rational; equal boosts share a group."""
    from fractions import Fraction
    rows = [x.split() for x in _run(program, "boost")[:765]]
    kept = [(int(ed), int(m), int(key, 16)) for ed, m, keep, _, key in rows if keep == "1"]
    frac = lambda ed, m: Fraction(0) if ed == 0 else Fraction(ed, m)          # noqa: E731
    for ed, m, key in kept:
        assert key >> 40 == 0 and key & 0xFF == ed
    by_key = sorted(kept, key=lambda x: x[2] >> 8)
    for a, b in zip(by_key, by_key[1:]):
        fa, fb = frac(a[0], a[1]), frac(b[0], b[1])
        assert fa <= fb
        assert (a[2] >> 8 == b[2] >> 8) == (fa == fb), (a, b)                 # the float's bits tell the rationals apart
        assert (R.boost(a[0], a[1]) == R.boost(b[0], b[1])) == (fa == fb)
    assert len({k >> 8 for _, _, k in kept}) == len({frac(ed, m) for ed, m, _ in kept})


def _mixed_vocabulary():
    """(as_text, raw spelling, lower-cased bytes): exact ASCII and non-ASCII keys, hashed terms behind the
    text cursor (some spelt in upper case), and short terms forced behind the text cursor too."""
    from oracle import oracle as O
    v = []
    for t in [b"a", b"ab", b"abc", b"b", b"zqxjkvwy", b"zqxjkvwyp", b"zqxjkvwypmnbghtr", "café".encode(), b"cafe",
              "cafés".encode(), "àéîõüçñ".encode(), F.HAN, F.EMOJI, "ａ".encode(), "\U00010428".encode()] + R.PAIR_C:
        v.append((0, t, t))
    for t in R.FAMILY_A[:12] + R.FAMILY_B[:12] + [F.ASCII_SPECIALS[3], F.ASCII_SPECIALS[4], F.UNI_SPECIALS[1], F.LONG255]:
        v.append((1, t, t))
    for t in R.FAMILY_A[12:20] + R.FAMILY_B[12:20] + [b"abd", "cafè".encode()]:
        up = t.decode().upper().encode()
        v.append((1, up, O.lower_utf8(up)))
    return v


def test_byte_comparison_over_all_pairs(program, tmp_path):
    v = _mixed_vocabulary()
    assert any(raw != low for _, raw, low in v) and len({low for _, _, low in v}) == len(v)
    blob = struct.pack("<I", len(v)) + b"".join(struct.pack("<I", a) + _s(raw) for a, raw, _ in v)
    lines = _run(program, "compare", str(tmp_path / "cmp.bin"), blob)
    assert lines[len(v)] == "ok %d" % len(v)
    for i, (_, _, a) in enumerate(v):
        want = "".join("-" if a < b else ("+" if a > b else "0") for _, _, b in v)
        assert lines[i] == want, a
    # bytes order is code-point order, not UTF-16 order
    assert R.PAIR_C[1] < R.PAIR_C[0]


def run_select(exe, path, vocab, cases):
    blob = struct.pack("<I", len(vocab)) + b"".join(_s(t) + struct.pack("<I", df) for t, df in vocab.items())
    blob += struct.pack("<I", len(cases)) + b"".join(struct.pack("<III", e, p, k) + _s(t) for e, p, k, t in cases)
    lines = _run(exe, "select", path, blob)
    out, at = [], 0
    for i in range(len(cases)):
        head = lines[at].split()
        assert head[0] == "case" and int(head[1]) == i, lines[at]
        within, n = int(head[2]), int(head[3])
        rows = [lines[at + 1 + k].split() for k in range(n)]
        out.append(([(bytes.fromhex(r[2]), int(r[0]), int(r[1], 16)) for r in rows], within))
        at += 1 + n
    assert lines[at] == "ok %d" % len(cases)
    return out


def test_selection_over_the_fixture_vocabulary(program, tmp_path):
    vocab = R.fixture().vocab
    cases = [(e, p, k, t) for e in (0, 1, 2) for p in (0, 1, 3) for k in (1, 5, 50, 64) for t in R.terms()]
    got = run_select(program, str(tmp_path / "select.bin"), vocab, cases)
    for c, (g, within) in zip(cases, got):
        exp, n = R.expansion(vocab, c[3], c[0], c[1], c[2])
        assert within == n, c
        assert g == [(t, d, int(b.view(np.uint32))) for t, _, d, b in exp], c


def test_header_declares_and_library_exports_the_fuzzy_search_calls():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "tfidf.h")).read(), flags=re.S)
    lib = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
