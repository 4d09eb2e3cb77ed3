"""The device-resident results of INTEGRATION.md 3c through their public entry
points: tfidf_search_batch_keys_device (n_q x k packed merge keys) and
tfidf_search_all_keys_device (every hit of one query, ordered), against the CPU
oracle, on the index's own stream and on a caller's stream (a torch stream
installed with tfidf_set_stream; the keys are then written on that stream).

A key is (float32 score bits << 32) | ~(doc_base + doc) as u64, 0 = empty:
descending key order is (score desc, doc asc), the oracle's order.  The keys
go into a torch.int64 device tensor pre-filled with a sentinel, with slack
behind the part the call may write: every key of the n_q x k rows must have
been written (a hit or 0), and nothing behind them, or behind the n hits of the
all-hits form.  Every comparison is exact: doc ids and float32 score bits.

Corpus: 3000 synthetic documents (one 8192-document block), 2^18 dictionary
slots.  k = 64 and 65 are the two sides of the query-unit limit (k <= 64 scores
plain disjunctions by query units, above it by a wave per (block, query)), 1024
is the largest k the entry takes; doc_base = 1 << 20 is a shard that is not the
first of its node.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tfidf_amd import _lib as L
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
SLACK = 64
KS = [1, 10, 64, 65, 1024]
BASES = [0, 1 << 20]
NO_PARSE = b"AND"
ABSENT = b"zzzzqq qqqqzz"
LONG_QUERY = b" ".join(synth.word(r) for r in range(1, 80))         # more than 64 terms


@pytest.fixture(scope="module")
def fx():
    texts = synth.corpus(3000, V=6000, len_min=20, len_max=120)
    g = ShardIndex()
    g.add_documents(texts)
    g.commit()
    o = O.OracleIndex()
    for i, t in enumerate(texts):
        o.add_doc(str(i).encode(), t)
    o.commit()
    vocab = o.vocab()
    rare = min((t for t, df in vocab.items() if 2 <= df <= 9), default=None)      # fewer than 10 hits
    assert rare is not None
    dense = synth.word(1)
    assert len(o.search(dense, 0)) > 1024 and 1 < len(o.search(rare, 0)) < 10
    queries = [dense, rare, ABSENT, NO_PARSE, LONG_QUERY, rare + b" " + ABSENT, b"", dense + b" " + synth.word(2)] + \
        synth.queries(24, lo=1, hi=3000)
    st = torch.cuda.Stream()
    fx = {"g": g, "o": o, "queries": queries, "stream": st, "n_docs": len(texts), "want": {}}
    assert not parses(fx, NO_PARSE) and parses(fx, ABSENT) and parses(fx, LONG_QUERY)
    yield fx
    g.set_stream(None)
    g.close()
    o.close()


def want(fx, q, k):
    """The oracle's [(doc, score bits)] of search(q, k); a query that does not parse has no hits."""
    if (q, k) not in fx["want"]:
        try:
            hits = fx["o"].search(q, k)
        except O.QuerySyntaxError:
            hits = []
        fx["want"][q, k] = [(int(d), int(np.float32(s).view(np.uint32))) for d, s in hits]
    return fx["want"][q, k]


def parses(fx, q):
    try:
        fx["o"].search(q, 1)
        return True
    except O.QuerySyntaxError:
        return False


class on_stream:
    """The index on its own stream (None) or on the fixture's torch stream; the own stream again on exit."""

    def __init__(self, fx, caller):
        self.g, self.st = fx["g"], fx["stream"] if caller else None

    def __enter__(self):
        if self.st is not None:
            self.g.set_stream(self.st.cuda_stream)
        return self

    def __exit__(self, *exc):
        self.g.set_stream(None)

    def sentinel_tensor(self, n):
        """n int64 sentinels on the device, written before any work the index queues after this."""
        if self.st is None:
            t = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()                 # the index's own stream is not ordered behind torch's
            return t
        with torch.cuda.stream(self.st):
            return torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda:0")

    def read(self, t):
        # (both entries return with their stream synchronised: the keys are there)
        if self.st is None:
            return t.cpu().numpy().view(np.uint64)
        with torch.cuda.stream(self.st):
            return t.cpu().numpy().view(np.uint64)


def decode(keys, doc_base):
    """[(doc, score bits)] of non-zero keys."""
    keys = [int(x) for x in keys]
    return [((~x & 0xFFFFFFFF) - doc_base, x >> 32) for x in keys]


@pytest.mark.parametrize("caller", [False, True], ids=["own", "caller"])
@pytest.mark.parametrize("doc_base", BASES)
@pytest.mark.parametrize("k", KS)
def test_batch_keys_equal_the_oracle(fx, k, doc_base, caller):
    g, qs = fx["g"], fx["queries"]
    with on_stream(fx, caller) as s:
        t = s.sentinel_tensor(len(qs) * k + SLACK)
        g.search_batch_keys_device(qs, k, doc_base, t.data_ptr())
        got = s.read(t)
    assert (got[len(qs) * k:] == SENTINEL).all()               # nothing behind the rows
    rows = got[:len(qs) * k].reshape(len(qs), k)
    for q, row in zip(qs, rows):
        n = int(np.count_nonzero(row))
        assert (row[n:] == 0).all(), q                         # the hits first, then empty keys
        assert n <= 1 or (row[:n - 1] > row[1:n]).all(), q     # strictly descending
        assert decode(row[:n], doc_base) == want(fx, q, k), (q, k)
    i = qs.index(NO_PARSE)
    assert not rows[i].any() and not rows[qs.index(ABSENT)].any() and not rows[qs.index(b"")].any()
    if k >= 10:
        assert 0 < np.count_nonzero(rows[1]) < k               # the rare word: fewer than k hits, the rest 0
    assert np.count_nonzero(rows[0]) == k                      # the dense word fills its row


@pytest.mark.parametrize("caller", [False, True], ids=["own", "caller"])
@pytest.mark.parametrize("doc_base", BASES)
def test_all_keys_equal_the_oracle(fx, doc_base, caller):
    g, n_docs = fx["g"], fx["n_docs"]
    with on_stream(fx, caller) as s:
        for q in fx["queries"]:
            t = s.sentinel_tensor(n_docs + SLACK)
            if not parses(fx, q):
                with pytest.raises(L.QuerySyntaxError):            # the single-query form says so; nothing is written
                    g.search_all_keys_device(q, doc_base, t.data_ptr(), n_docs)
                assert (s.read(t) == SENTINEL).all()
                continue
            n = g.search_all_keys_device(q, doc_base, t.data_ptr(), n_docs)
            got = s.read(t)
            assert n == len(want(fx, q, 0)), q
            assert (got[n:] == SENTINEL).all(), q              # nothing behind the hits
            assert n <= 1 or (got[:n - 1] > got[1:n]).all(), q
            assert decode(got[:n], doc_base) == want(fx, q, 0), q


@pytest.mark.parametrize("caller", [False, True], ids=["own", "caller"])
def test_argument_checks(fx, caller):
    g, qs, n_docs = fx["g"], fx["queries"][:3], fx["n_docs"]
    with on_stream(fx, caller) as s:
        t = s.sentinel_tensor(max(len(qs) * 1025, n_docs) + SLACK)
        for k in (0, 1025):
            with pytest.raises(L.TfidfError) as e:
                g.search_batch_keys_device(qs, k, 0, t.data_ptr())
            assert e.value.code == L.E_INVALID_ARG
        with pytest.raises(L.TfidfError) as e:
            g.search_batch_keys_device(qs, 10, 0, None)        # NULL keys with queries to answer
        assert e.value.code == L.E_INVALID_ARG
        g.search_batch_keys_device([], 10, 0, None)            # no query: nothing to write
        for cap in (0, n_docs - 1):
            with pytest.raises(L.TfidfError) as e:
                g.search_all_keys_device(qs[0], 0, t.data_ptr(), cap)
            assert e.value.code == L.E_BUFFER and str(n_docs) in str(e.value)
        with pytest.raises(L.TfidfError) as e:
            g.search_all_keys_device(qs[0], 0, None, n_docs)
        assert e.value.code == L.E_BUFFER
        assert (s.read(t) == SENTINEL).all()                   # a refused call writes nothing
        # and the index still answers
        assert g.search_all_keys_device(qs[0], 0, t.data_ptr(), n_docs) == len(want(fx, qs[0], 0))
