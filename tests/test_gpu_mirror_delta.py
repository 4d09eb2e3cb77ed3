"""Delta mirrors: an incremental block-major commit brings the build target's
host mirrors (dictionary keys, per-slot df, slot -> column words) up to date
with the new slots and the changed df alone, or not at all when nothing
changed (csrc/commit_plan.h mirror_plan; tfidf_commit_host_profile says which
form each mirror took, how many bytes moved and how often the host waited).

Documents are 3-6 words over <= 300 synthetic words, a few thousand of them,
at 2^10 dictionary slots (the smallest the constructor takes).  The mirrors are
what df, the vocabulary export, query analysis (every search) and doc_terms
read, so after every commit the index is compared with a FRESH index built in
one commit from the same documents and with the CPU oracle, bit for bit: df of
every vocabulary word, the vocabulary export, all hits and the top 10 of every
word and a few multi-term queries (test_gpu_incremental_inversion.Expect), and
doc_terms of a seeded sample.  No test measures time.
"""
import random

import numpy as np
import pytest

from tfidf_amd import _lib as L
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

from test_gpu_incremental_commit import STAGED_FIELDS, add, keyed, published
from test_gpu_incremental_inversion import expect
from test_gpu_parity import assert_hits_equal

pytestmark = pytest.mark.gpu

CAP = 10
C = 1 << CAP
CTOR = dict(vocab_capacity_log2=CAP)
WHOLE_BYTES = {"bytes_dict": 2 * C * 8, "bytes_df": C * 4, "bytes_crank": (C // 32 + 1) * 8}
DF_CAP = 4096                                       # kDfDeltaCap (commit_plan.h)
_rng = random.Random(20261021)


def texts(n, lo, hi):
    return [b" ".join(synth.word(_rng.randint(lo, hi)) for _ in range(_rng.randint(3, 6))) for _ in range(n)]


BASE = keyed(texts(3000, 1, 300))
KNOWN = [keyed(texts(n, 1, 300), 3000 + 100 * i) for i, n in enumerate((40, 25, 60, 1))]
# 320 words no earlier document holds: 9-15 bytes and > 16 bytes (hashed keys), short ones, one non-ASCII
NEW_WORDS = [b"nw%03dxyzabc" % i for i in range(150)] + [b"quitelongnewword%04dtail" % i for i in range(100)] + \
            [b"n%03d" % i for i in range(69)] + ["zoë".encode()]
NEW_DOCS = keyed([b" ".join(NEW_WORDS[i:i + 4]) + b" " + synth.word(1 + i % 300) for i in range(0, 320, 4)], 5000)

_fresh_export = {}


def fresh_export(docs, **ctor):
    key = (len(docs), hash(tuple(docs[-300:])), tuple(sorted(ctor.items())))
    if key not in _fresh_export:
        f = ShardIndex(**ctor)
        try:
            add(f, docs)
            f.commit()
            _fresh_export[key] = f.vocab_export()
        finally:
            f.close()
    return _fresh_export[key]


def check(g, docs, stats=True, extra_queries=(), **ctor):
    """g against a fresh one-commit index of docs and the oracle, through every reader of the mirrors."""
    ctor = ctor or CTOR
    e = expect(docs, extra_queries, **ctor)
    e.check(g, 0, stats=stats, rows=False)          # stats, df of every word, all hits and top 10 of every word + MULTI
    for got, want in zip(g.vocab_export(), fresh_export(docs, **ctor)):
        assert np.array_equal(got, want)
    for d in random.Random(len(docs)).sample(range(len(docs)), 64):
        assert g.doc_terms(d) == e.row(d)[0], d
    return e


def profile(g, dict_, df, crank, syncs=None, **fields):
    p = g.commit_host_profile()
    assert (p["mirror_dict"], p["mirror_df"], p["mirror_crank"]) == (dict_, df, crank), p
    if syncs is not None:
        # 2: the counter read and the final one; 3: + the df list.  A commit that tokenizes short documents
        # in packs also reads the packs' retry count (the tokenizer's own wait, as the long path's are)
        if syncs == 3 and g.stats()["pack_docs"] > 1:
            syncs += 1
        assert p["stream_syncs"] == syncs, p
    for k, v in fields.items():
        assert p[k] == v, (k, p)
    assert 0 < p["ms_counters"] <= p["ms_enqueued"] <= p["ms_synced"] <= p["ms_published"] <= p["ms_wall"], p
    return p


def whole(g, **fields):
    return profile(g, "whole", "whole", "whole", **WHOLE_BYTES, dict_delta_entries=0, df_delta_entries=0, **fields)


def twice(docs, **ctor):
    g = ShardIndex(**(ctor or CTOR))
    add(g, docs)
    for _ in range(2):                              # each snapshot's first build: everything is copied whole
        g.commit()
        assert g.commit_tokenized_docs() == {"docs": len(docs), "was_full": True}
        if not ctor:
            whole(g, col_rank_runs=1)
    return g


def df_changes(new, old):
    """Words whose df differs between two oracle vocabularies."""
    return sum(1 for w in set(new) | set(old) if new.get(w, 0) != old.get(w, 0))


# ---------------------------------------------------------------------------

def test_nothing_added_moves_nothing():
    g = twice(BASE)
    check(g, BASE)
    for _ in range(3):                              # both snapshots
        g.commit()
        assert g.commit_tokenized_docs() == {"docs": 0, "was_full": False}
        profile(g, "none", "none", "none", syncs=2, col_rank_runs=0, bytes_dict=0, bytes_df=0, bytes_crank=0,
                dict_delta_entries=0, df_delta_entries=0)
        check(g, BASE)
    g.close()


def test_known_words_move_the_changed_df_only():
    g = twice(BASE)
    docs = list(BASE)
    vocabs = [check(g, docs).vocab] * 2             # the oracle's df at each snapshot's last build
    for batch in KNOWN:                             # each snapshot applies a delta over the batch it missed as well
        add(g, batch)
        docs = docs + batch                         # (a new list: expect() keeps the one it was given)
        g.commit()
        assert g.commit_tokenized_docs()["was_full"] is False
        e = check(g, docs)
        n = df_changes(e.vocab, vocabs[-2])
        assert 0 < n <= DF_CAP
        profile(g, "none", "delta", "none", syncs=3, col_rank_runs=1, bytes_dict=0, bytes_crank=0, bytes_df=8 * n,
                df_delta_entries=n, dict_delta_entries=0)
        vocabs.append(e.vocab)
    g.commit()                                      # nothing added: the other snapshot still lacks the last batch
    e = check(g, docs)
    n = df_changes(e.vocab, vocabs[-2])
    profile(g, "none", "delta", "none", syncs=3, bytes_df=8 * n, df_delta_entries=n)
    g.commit()
    profile(g, "none", "none", "none", syncs=2, col_rank_runs=0, bytes_df=0)
    check(g, docs)
    g.close()


def test_new_words_move_their_slots_and_the_column_words():
    g = twice(BASE)
    docs = BASE + NEW_DOCS
    add(g, NEW_DOCS)
    for _ in range(2):                              # both snapshots take the 320 new slots
        g.commit()
        assert g.commit_tokenized_docs() == {"docs": len(NEW_DOCS), "was_full": False}
        e = check(g, docs, extra_queries=NEW_WORDS[:3] + NEW_WORDS[-3:])
        assert all(w in e.vocab for w in NEW_WORDS)          # every new word is searched (Expect: the whole vocabulary)
        n = df_changes(e.vocab, expect(BASE, **CTOR).vocab)
        assert n >= len(NEW_WORDS) == 320
        profile(g, "delta", "delta", "whole", syncs=3, col_rank_runs=1, dict_delta_entries=320, bytes_dict=320 * 24,
                bytes_crank=WHOLE_BYTES["bytes_crank"], df_delta_entries=n, bytes_df=8 * n)
    for w in NEW_WORDS[::7]:
        i = NEW_WORDS.index(w)
        assert [d for d, _ in g.search(w, 0)] == [len(BASE) + i // 4]
    g.commit()
    profile(g, "none", "none", "none", syncs=2, col_rank_runs=0)
    check(g, docs, extra_queries=NEW_WORDS[:3] + NEW_WORDS[-3:])
    g.close()


@pytest.mark.parametrize("cap", [100, 10])          # the list overflows on the device / the whole copy is planned
def test_df_list_cap_falls_back_to_the_whole_copy(monkeypatch, cap):
    g = twice(BASE)
    docs = BASE + KNOWN[2]
    add(g, KNOWN[2])
    e = expect(docs, **CTOR)
    n = df_changes(e.vocab, expect(BASE, **CTOR).vocab)
    nnz = sum(len(set(t.split())) for _, t in KNOWN[2])
    assert cap < n and (nnz <= 4 * cap) == (cap == 100)      # 100: the delta is tried (kDfDeltaTry) and overflows
    monkeypatch.setenv("TFIDF_TEST_DF_DELTA_CAP", str(cap))
    for _ in range(2):
        g.commit()
        assert g.commit_tokenized_docs() == {"docs": len(KNOWN[2]), "was_full": False}
        profile(g, "none", "whole", "none", bytes_dict=0, bytes_crank=0, bytes_df=WHOLE_BYTES["bytes_df"],
                df_delta_entries=0)
        check(g, docs)
    g.close()


def test_delete_falls_back_to_whole_mirrors():
    g = twice(BASE)
    add(g, KNOWN[0])
    g.commit()
    profile(g, "none", "delta", "none")
    assert g.delete_documents([BASE[17][0]]) == 1
    docs = BASE[:17] + BASE[18:] + KNOWN[0]
    for _ in range(2):
        g.commit()
        assert g.commit_tokenized_docs()["was_full"] is True
        whole(g)
        check(g, docs, stats=False)
    g.close()


def test_failed_commit_falls_back_to_whole_mirrors():
    g = twice(BASE)
    before = published(g)
    add(g, [(b"offender", b" ".join(b"off%04d" % j for j in range(1100)))])      # 300 + 1100 terms > 2^10 slots
    for _ in range(2):
        with pytest.raises(L.TfidfError) as err:
            g.commit()
        assert err.value.code == L.E_CAPACITY
    assert {k: v for k, v in published(g).items() if k not in STAGED_FIELDS} == \
        {k: v for k, v in before.items() if k not in STAGED_FIELDS}
    check(g, BASE, stats=False)                     # the published snapshot's mirrors were not touched
    assert g.delete_documents([b"offender"]) == 1
    g.compact()
    add(g, KNOWN[0])
    docs = BASE + KNOWN[0]
    for _ in range(2):
        g.commit()
        assert g.commit_tokenized_docs() == {"docs": len(docs), "was_full": True}
        whole(g)
        check(g, docs)
    g.commit()
    profile(g, "none", "none", "none", syncs=2)
    check(g, docs)
    g.close()


def test_term_major_mirrors_whole():
    ctor = dict(vocab_capacity_log2=CAP, inversion=2)
    g = twice(BASE, **ctor)
    docs = BASE + KNOWN[0]
    add(g, KNOWN[0])
    for n_tok in (len(KNOWN[0]), len(KNOWN[0]), 0):
        g.commit()
        assert g.commit_tokenized_docs() == {"docs": n_tok, "was_full": False}
        profile(g, "whole", "whole", "none", bytes_dict=WHOLE_BYTES["bytes_dict"], bytes_df=WHOLE_BYTES["bytes_df"],
                bytes_crank=0, col_rank_runs=0)
        check(g, docs, **ctor)
    g.close()


@pytest.mark.parametrize("knob", ["TFIDF_FULL_COMMIT", "TFIDF_FULL_MIRROR"])
def test_ab_switches_mirror_whole(monkeypatch, knob):
    g = twice(BASE)
    docs = BASE + KNOWN[0]
    add(g, KNOWN[0])
    monkeypatch.setenv(knob, "1")
    for _ in range(2):
        g.commit()
        assert g.commit_tokenized_docs()["was_full"] is (knob == "TFIDF_FULL_COMMIT")
        whole(g, col_rank_runs=1)
        check(g, docs)
    monkeypatch.delenv(knob)
    add(g, KNOWN[1])
    docs = docs + KNOWN[1]
    g.commit()
    if knob == "TFIDF_FULL_MIRROR":                 # outside the signature: the whole copies left valid mirrors
        assert g.commit_tokenized_docs() == {"docs": len(KNOWN[1]), "was_full": False}
        profile(g, "none", "delta", "none", syncs=3)
    else:                                           # the snapshot was built under another knob value: a full build
        assert g.commit_tokenized_docs()["was_full"] is True
        whole(g)
    check(g, docs)
    g.close()


def test_global_view_after_a_delta_commit_reads_the_mirrored_df():
    g = twice(BASE)
    docs = BASE + KNOWN[0] + NEW_DOCS[:10]
    add(g, KNOWN[0] + NEW_DOCS[:10])
    g.commit()
    profile(g, "delta", "delta", "whole")
    e = check(g, docs)
    # a GLOBAL view that names no key takes every df from the host mirror; with the shard's own
    # doc_count and sum_ttf it must score as the shard's own statistics do
    g.set_global_stats(np.zeros((0, 2), np.uint64), np.zeros(0, np.uint64), e.o.doc_count, e.o.sum_ttf)
    for q in e.queries:
        assert_hits_equal(g.search(q, 0), e.hits[q, 0])
    for t, df in e.vocab.items():
        assert g.df(t) == (df, df)
    g.clear_global_stats()
    g.commit()                                      # the other snapshot; the view handling moved ahead of the inversion
    profile(g, "delta", "delta", "whole")
    check(g, docs)
    g.close()
