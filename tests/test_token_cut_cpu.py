"""The corpora of token_cut_ref.py, checked without a device: the oracle
indexes every family, every run is cut (or not) where its row of the table
says, and every placement has the property it is named for — worked out from
the kCoreBytes / kPreBytes / kPostBytes window arithmetic of tfidf_internal.h,
so an edit of the table or of the constants that empties a family fails here
and not silently on the GPU."""
import pytest

import token_cut_ref as T
from oracle import oracle as O


def test_constants_are_the_sources():
    assert T.header_constants() == (T.CORE, T.PRE, T.POST, T.MAX_UNITS)
    assert T.PRE + T.CORE + T.POST + 16 <= T.WAVE_WINDOW


@pytest.mark.parametrize("name", T.FAMILIES)
def test_oracle_indexes_every_family(name):
    docs = T.family(name)
    o = T.oracle_index(name)
    assert o.num_docs == len(docs) and o.malformed_docs() == []
    assert 1 <= len(docs) <= 200 and all(len(d.text) <= 8192 for d in docs)
    assert o.doc_count == len(docs)                        # no document is empty
    for d in range(len(docs)):
        toks = O.tokenize(docs[d].text)
        assert o.doc_len(d) == len(toks)
        assert all(T.units(t.decode()) <= T.MAX_UNITS for t in toks)
        terms = o.doc_terms(d)                             # (terms of up to 765 bytes through the wrapper's buffers)
        assert sum(terms.values()) == len(toks) and set(terms) == set(toks)
    assert set(o.vocab()) == {t for d in docs for t in O.tokenize(d.text)}
    for q in T.queries(name):
        o.search(q, 0)


def test_runs_cut_where_the_table_says():
    want_uncut = {"z255", "Z255", "e200", "e255", "ga255"}
    for r in T.RUNS:
        b = r.text.encode()
        raw = T.spans(b, T.NO_CUT)
        assert raw == [(0, len(b))], r.name                # one token before the cut
        toks = O.tokenize(b)
        assert (T.spans(b) == raw) == (r.name in want_uncut) == (T.units(r.text) <= T.MAX_UNITS), r.name
        if r.sibling:
            sib = O.tokenize(r.sibling.encode())
            assert sib[0] == toks[0] and r.sibling != r.text, r.name          # the same first term, other bytes
            assert len(T.spans(r.sibling.encode(), T.NO_CUT)) == 1
    tok = lambda name: O.tokenize(T.RUN[name].text.encode())
    assert tok("e200") == ["é".encode() * 200] and len(T.RUN["e200"].text.encode()) == 400 > T.MAX_UNITS
    assert tok("ga300")[0] == "가".encode() * 255 and len(tok("ga300")[0]) == 765
    low = T.DESERET_LOW.encode()
    assert tok("des128") == [low * 127, low]               # the pair that would straddle the cut goes on
    assert tok("a254des") == [b"a" * 254, low + b"a" * 10]
    assert tok("a200e")[0] == b"a" * 200 + "é".encode() + b"a" * 54 and len(T.RUN["a200e"].text.encode()) == 302 < 512
    assert tok("acute300") == [b"a" + "́".encode() * 254]    # extenders count as units; orphan marks are no token
    assert tok("thai300")[0] == (T.THAI * 50)[:255].encode()
    assert tok("kata300") == ["カ".encode() * 255, "カ".encode() * 45]
    # the three alignments of a joiner at the cut: the unit before it and the unit after it
    for tag, j in (("dot", "."), ("comma", ","), ("apos", "'"), ("under", "_")):
        ends = {(T.RUN[tag + str(k)].text[254] == j, T.RUN[tag + str(k)].text[255] == j) for k in (0, 1, 2)}
        assert ends == {(False, True), (True, False)}, tag
        assert len({T.RUN[tag + str(k)].text[253:257] for k in (0, 1, 2)}) == 3


def test_wave_characters():
    """prose = True exactly for the runs whose non-ASCII characters are all in WAVE_CHARS."""
    for r in T.RUNS:
        chars = {c for c in r.text + (r.sibling or "") if ord(c) >= 0x80}
        assert (r.prose is None) == (not chars), r.name
        if chars:
            assert r.prose == (chars <= T.WAVE_CHARS), r.name


@pytest.mark.parametrize("cls", ["letters", "joiners", "unicode"])
def test_short_placements(cls):
    docs = T.family(cls)
    for r in T.CLASSES[cls]:
        mine = {d.tag: d.text for d in docs if d.runs == (r.name,)}
        b = r.text.encode()
        first = O.tokenize(b)[0]
        assert mine["alone"] == b and mine["first"].startswith(b + b" ") and mine["last"].endswith(b" " + b)
        assert T.spans(mine["last"], T.NO_CUT)[-1] == (len(mine["last"]) - len(b), len(b))
        assert mine["twice"] == b + b" " + b
        if r.sibling:
            raw = [(s, n) for s, n in T.spans(mine["differ"], T.NO_CUT) if n >= 255]
            assert len(raw) == 2
            (s1, n1), (s2, n2) = raw
            assert mine["differ"][s1:s1 + n1] != mine["differ"][s2:s2 + n2]
            assert O.tokenize(mine["differ"][s1:s1 + n1])[0] == O.tokenize(mine["differ"][s2:s2 + n2])[0] == first
            assert O.tokenize(mine["sibling"])[1] == first
    assert all(len(d.text) <= 4000 for d in docs)


@pytest.mark.parametrize("name", ["chunk_ascii", "chunk_unicode", "chunk_nosplit"])
def test_chunk_placements(name):
    docs = T.family(name)
    seen = set()
    for d in docs:
        L = len(d.text)
        assert 4200 <= L <= 8192
        raw = T.spans(d.text, T.NO_CUT)
        if d.tag == "postclip":
            (r,) = d.runs
            b = T.RUN[r].text.encode()
            s = d.text.index(b)
            clo, chi, ws, we = T.unit_windows(L)[0]
            assert (s, len(b)) in raw and clo <= s < chi and s < we < s + len(b) and we < L   # the margin ends inside it
        else:
            delta = dict(T.EDGES)[d.tag]
            for k, r in enumerate(d.runs):
                b = T.RUN[r].text.encode()
                s = (k + 1) * T.CORE + delta
                assert d.text[s:s + len(b)] == b and (s, len(b)) in raw, (d.tag, r)
                if d.tag == "premargin":
                    assert (k + 1) * T.CORE - T.PRE <= s < (k + 1) * T.CORE
        seen |= {(d.tag, r) for r in d.runs}
    runs = {r for _, r in seen}
    want = {"chunk_ascii": T.CLASSES["letters"] + T.CLASSES["joiners"]}.get(name, T.CLASSES["unicode"])
    assert runs == {r.name for r in want}                              # every run of the table
    for tag, _ in T.EDGES:
        assert {r for t, r in seen if t == tag} == runs                # at every edge
    assert {r for t, r in seen if t == "postclip"} == {r.name for r in want if len(r.text.encode()) > T.POST + 32}
    if name == "chunk_nosplit":
        for d in docs:
            assert not any(b < 0x80 and not chr(b).isalnum() and chr(b) not in "._',:" for b in d.text)   # no split byte
    else:
        assert all(b" " in d.text[k * T.CORE - T.PRE:k * T.CORE] for d in docs if not d.runs
                   for k in range(1, len(T.unit_windows(len(d.text)))))


def test_cover_holds_a_whole_window():
    for d in T.family("cover"):
        (s, n), = [x for x in T.spans(d.text, T.NO_CUT) if x[1] >= 3000]
        clo, chi, ws, we = T.unit_windows(len(d.text))[1]
        assert s <= ws and we <= s + n and we - ws == T.PRE + T.CORE + T.POST


def test_same_prefix_family_is_the_bug_shape():
    """Two tokens with equal cut terms that START in one core, whose raw spans —
    as the unit sees them, clipped by its window's end — differ in length or
    case; the window holds non-ASCII text, the document is book-sized."""
    by_tag = {}
    for d in T.family("same_prefix"):
        L = len(d.text)
        assert L > T.WAVE_WINDOW
        clo, chi, ws, we = T.unit_windows(L)[0]
        assert any(b >= 0x80 for b in d.text[ws:we])
        big = [(s, n) for s, n in T.spans(d.text, T.NO_CUT) if T.span_units(d.text, s, n) > T.MAX_UNITS]
        assert len(big) == 2 and all(clo <= s < chi for s, _ in big)
        (s1, n1), (s2, n2) = big
        seen1, seen2 = d.text[s1:min(s1 + n1, we)], d.text[s2:min(s2 + n2, we)]
        assert seen1 != seen2
        assert O.tokenize(d.text[s1:s1 + n1])[0] == O.tokenize(d.text[s2:s2 + n2])[0]
        by_tag.setdefault(d.tag, []).append((len(seen1), len(seen2), s2 + n2 > we))
    assert all(a != b for a, b, _ in by_tag["prefix-length"] + by_tag["prefix-clipped"])
    assert all(clip and b == 1041 for _, b, clip in by_tag["prefix-clipped"])       # the `windowcut` layout
    assert all(a == b for a, b, _ in by_tag["prefix-case"])
    marks = {frozenset(c for c in d.text.decode() if ord(c) >= 0x80 and c not in "éÉ가") for d in T.family("same_prefix")}
    assert frozenset() in marks and any("日" in m for m in marks)       # wave-rule windows and scanner windows


def test_overflow_family_overflows_the_window():
    docs = T.family("overflow")
    off = 0
    over = []
    for i, d in enumerate(docs):
        if len(d.text) <= T.WAVE_WINDOW and off % 16 + len(d.text) > T.WAVE_WINDOW:
            over.append(i)
            assert any(b >= 0x80 for b in d.text)
        off += len(d.text)
    assert over == [1, 2] == [i for i, d in enumerate(docs) if d.tag == "overflow"]
    assert any(n > 255 for _, n in T.spans(docs[2].text, T.NO_CUT)) and not any(n > 255 for _, n in T.spans(docs[1].text, T.NO_CUT))
    assert all(len(set(O.tokenize(docs[i].text))) < 100 for i in over)  # far under k_tokenize_uwave's 512 terms
    n_uni = sum(1 for d in docs if d.tag == "plain")
    assert n_uni * 2 > len(docs)                                       # the next commit runs UNI-first
    assert sum(len(d.text) for d in docs) // len(docs) > 1280          # one document per wave (kPackBytes / 2)


def test_expected_paths_of_the_families():
    """The path model on shapes whose answer is plain: a book-sized document
    that holds a cut never stays on the chunk path; é x 200 (400 bytes) is
    handed over by the wave rules, which measure bytes — by the chunk units'
    too, so it ends on k_tokenize_long — and kept by k_tokenize_uwave when the
    wave rules are off."""
    docs = T.family("chunk_ascii")
    cut = [d for d in docs if any(n > 255 for _, n in T.spans(d.text, T.NO_CUT))]
    e = T.expected_paths(docs)
    assert e == dict(long_docs=len(docs), long_chunked=len(docs) - len(cut), unicode_docs=0, unicode_wave_docs=0)
    assert 0 < e["long_chunked"] < len(docs)
    d = [T.Doc(T.RUN["e200"].text.encode(), "alone", ("e200",))]
    assert T.expected_paths(d) == dict(long_docs=1, long_chunked=0, unicode_docs=1, unicode_wave_docs=1)
    assert T.expected_paths(d, "nouniwave") == dict(long_docs=0, long_chunked=0, unicode_docs=1, unicode_wave_docs=0)
    for cfg in ("default", "nouniwave", "nouchunk"):
        for f in ("chunk_unicode", "chunk_nosplit", "same_prefix", "cover"):
            e = T.expected_paths(T.family(f), cfg)
            assert e["long_docs"] == len(T.family(f)) and e["unicode_docs"] == 0
    assert T.expected_paths(T.family("same_prefix"), "nouniwave")["long_chunked"] == 0
