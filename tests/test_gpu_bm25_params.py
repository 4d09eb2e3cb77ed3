"""BM25 k1 / b beyond the defaults on every scorer, select and merge path.

Every other GPU test runs at (k1, b) = (1.2, 0.75): positive, finite, mostly
distinct scores of similar magnitude.  The Lucene-legal sets below give the
score shapes where selection goes wrong, out of the corpora the suite already
has:

  plain   (2.0, 1.0)         ordinary non-default values
  nolen   (1.2, 0.0)         length-free scores: few distinct values, long ties
  idf     (0.0, 0.75)        norm cache +inf: every hit of a term scores its
                             weight, a tie group is the term's posting list
  mixed0  (16777216.0, 0.75) tf * norm_inverse <= 2^-24 rounds 1 + x to 1: the
                             score is exactly 0.0f; zero and positive mixed
  all0    (1e9, 0.75)        every score 0.0f: the order is the doc id alone

A zero score is a hit (Lucene's collector starts at -inf), so its key
(score bits << 32 | ~doc) has zero score bits and is non-zero only by ~doc.

Corpus A is test_gpu_units.py's shape (four 8192-document blocks: block
candidates, unit ranges and merge levels cross blocks).  Batches of plain
disjunctions take the unit path; a batch that holds an operator query goes,
whole, through the kOps instantiations, so the operator queries ride in a
batch of their own (alone: grid mode; with the plain queries: wave per pair).

Corpus Z is crafted for k_score_blocks' radix select: per block, wave 0's
documents (the block's first 1024) hold the only positive scores of `alpha`
and every other wave's hits score 0.0f.  The block min / max of the score bits
must come from every wave with a hit; taken from the waves with a non-zero
maximum alone, the zero-score hits are never counted and the block returns
only its 5 positive candidates for any k > 5.  At Z's (2^24, 0) every tf = 1
posting scores 0.0f whatever its term, so `alpha beta` adds zero-score hits to
wave 0 as well (the block min is then 0 on any build): it checks the sum and
the order of 16 384 hits of which 10 are positive.

Bar: doc ids and float32 score bit patterns identical to the oracle built
with the same (k1, b).  No tolerance.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tfidf_amd import _lib as L
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

pytestmark = pytest.mark.gpu

SETS = {
    "plain": (2.0, 1.0),
    "nolen": (1.2, 0.0),
    "idf": (0.0, 0.75),
    "mixed0": (16777216.0, 0.75),
    "all0": (1e9, 0.75),
}
TERM_SETS = ("nolen", "mixed0")
KTOP = 65                       # the largest k of a batch check


@functools.lru_cache(maxsize=None)
def texts_a():
    return synth.corpus(26_000, V=6_000, len_min=20, len_max=120)


PLAIN = synth.queries(1500, lo=1, hi=3000) + synth.queries(200, n_terms=1, lo=1, hi=200)
OPS = [b"aaaa AND aaab", b"aaab NOT aaaa", b"aaaa OR aaab AND aaac"]
ALL = PLAIN + OPS
SAMPLE = list(range(0, len(PLAIN), 34))[:50]          # 45 three-term queries, 5 dense single terms
SINGLE_TERM = [i for i in SAMPLE if i >= 1500]


def bits_of(scores):
    return np.asarray(scores, np.float32).view(np.uint32)


class Want:
    """The oracle's answers for one (k1, b): top-KTOP of every query of ALL as
    arrays, every hit of the sample and of the operator queries as lists."""

    def __init__(self, texts, queries, k1, b, full_idx):
        o = O.OracleIndex(k1, b)
        for i, t in enumerate(texts):
            o.add_doc(str(i).encode(), t)
        o.commit()
        n = len(queries)
        self.docs = np.zeros((n, KTOP), np.uint32)
        self.bits = np.zeros((n, KTOP), np.uint32)
        self.count = np.zeros(n, np.uint32)
        self.full = {}
        for i, q in enumerate(queries):
            hits = o.search(q, 0) if i in full_idx else o.search(q, KTOP)
            if i in full_idx:
                self.full[i] = hits
            top = hits[:KTOP]
            self.count[i] = len(top)
            self.docs[i, :len(top)] = [d for d, _ in top]
            self.bits[i, :len(top)] = bits_of([s for _, s in top])
        o.close()


@functools.lru_cache(maxsize=None)
def want_a(name):
    full_idx = frozenset(SAMPLE) | frozenset(range(len(PLAIN), len(ALL)))
    return Want(texts_a(), ALL, *SETS[name], full_idx)


def assert_hits(got, want, what=None):
    assert [d for d, _ in got] == [d for d, _ in want], what
    assert bits_of([s for _, s in got]).tolist() == bits_of([s for _, s in want]).tolist(), what


def assert_batch(res, W, k, idx, queries):
    """Rows of a search_batch result (queries idx of W) against W's top-k."""
    docs, scores, counts = res
    wc = np.minimum(W.count[idx], k)
    wd, wb = W.docs[idx, :k], W.bits[idx, :k]
    live = np.arange(k)[None, :] < wc[:, None]
    bad = (counts != wc) | ((docs != wd) & live).any(1) | ((scores.view(np.uint32) != wb) & live).any(1)
    rows = np.nonzero(bad)[0]
    if rows.size:
        r = int(rows[0])
        raise AssertionError("%d of %d rows differ; first: query %r, got %d hits %s / %s, want %d hits %s / %s" % (
            rows.size, len(idx), queries[r], counts[r], docs[r, :counts[r]][:12].tolist(),
            scores.view(np.uint32)[r, :counts[r]][:12].tolist(), wc[r], wd[r, :wc[r]][:12].tolist(),
            wb[r, :wc[r]][:12].tolist()))


def gpu_index(texts, k1, b, inversion=L.INVERSION_AUTO):
    g = ShardIndex(k1=k1, b=b, vocab_capacity_log2=16, inversion=inversion)
    g.add_documents(texts)
    g.commit()
    return g


class Env:
    def __init__(self, name, inversion=L.INVERSION_AUTO):
        self.name = name
        self.W = want_a(name)
        self.g = gpu_index(texts_a(), *SETS[name], inversion)


@pytest.fixture(scope="module", params=list(SETS))
def env(request):
    e = Env(request.param)
    assert e.g.stats()["term_major"] == 0
    yield e
    e.g.close()


@pytest.fixture(scope="module", params=list(TERM_SETS))
def term_env(request):
    e = Env(request.param, L.INVERSION_TERM)
    assert e.g.stats()["term_major"] == 1
    yield e
    e.g.close()


# ---------------------------------------------------------------------------
# preconditions, on the oracle alone: the sets produce the regimes they are for

@pytest.mark.parametrize("name", list(SETS))
def test_regime_preconditions(name):
    W = want_a(name)
    with_hits = [i for i in SAMPLE if W.full[i]]
    assert len(with_hits) >= 45
    scores = {i: bits_of([s for _, s in W.full[i]]) for i in with_hits}
    assert all((s >> 31 == 0).all() for s in scores.values())          # no negative score, no -0.0
    if name == "mixed0":
        for i in with_hits:
            assert (scores[i] == 0).any() and (scores[i] != 0).any(), PLAIN[i]
    elif name == "all0":
        assert all((s == 0).all() for s in scores.values())
        assert (W.bits == 0).all()
        for i in with_hits:                                            # the order is the doc id alone
            d = [x for x, _ in W.full[i]]
            assert d == sorted(d)
    elif name == "idf":
        assert len(SINGLE_TERM) >= 5
        for i in SINGLE_TERM:
            assert len(W.full[i]) > 1024 and len(set(scores[i].tolist())) == 1, PLAIN[i]
    elif name == "nolen":
        # length-free: a single term's scores take one value per tf
        assert all(len(set(scores[i].tolist())) <= 8 for i in SINGLE_TERM)
    else:
        assert all((s != 0).all() for s in scores.values())
        assert all(len(set(scores[i].tolist())) > 8 for i in SINGLE_TERM)   # one value per (tf, norm byte)


# ---------------------------------------------------------------------------
# single queries

@pytest.mark.parametrize("k", [1, 10, 64])
def test_single_fused(env, k):
    g, W = env.g, env.W
    f0 = g.stats()["fused_queries"]
    for i in SAMPLE:
        assert_hits(g.search(PLAIN[i], k), W.full[i][:k], PLAIN[i])
    present = sum(1 for i in SAMPLE if W.full[i])
    assert g.stats()["fused_queries"] - f0 >= present                  # the one-launch path ran


@pytest.mark.parametrize("k,knob", [(100, None), (1024, None), (10, "TFIDF_NO_FUSED")])
def test_single_unfused(env, k, knob, monkeypatch):
    g, W = env.g, env.W
    if knob:
        monkeypatch.setenv(knob, "1")
    f0 = g.stats()["fused_queries"]
    for i in SAMPLE:
        assert_hits(g.search(PLAIN[i], k), W.full[i][:k], PLAIN[i])
    assert g.stats()["fused_queries"] == f0                            # run_scoring + the device merge


@pytest.mark.parametrize("force", [None, "TFIDF_HITS_GROUPS", "TFIDF_HITS_PAIRWISE"])
def test_single_all_hits(env, force, monkeypatch):
    g, W = env.g, env.W
    if force:
        monkeypatch.setenv(force, "1")
    for i in SAMPLE:
        assert_hits(g.search(PLAIN[i], 0), W.full[i], PLAIN[i])


# ---------------------------------------------------------------------------
# batches

@pytest.mark.parametrize("light", [None, "0", "1000000000"])
@pytest.mark.parametrize("k", [1, 10, 64])
def test_batch_units(env, k, light, monkeypatch):
    """Wave units and workgroup units as the host splits them, every query on
    workgroup units (0), every query on wave units (10^9)."""
    g = env.g
    if light is not None:
        monkeypatch.setenv("TFIDF_WUNIT_LIGHT", light)
    u0 = g.stats()["unit_batches"]
    res = g.search_batch(PLAIN, k)
    assert g.stats()["unit_batches"] == u0 + 1                         # the unit path ran
    assert_batch(res, env.W, k, np.arange(len(PLAIN)), PLAIN)


@pytest.mark.parametrize("k,knob", [(65, None), (10, "TFIDF_NO_UNITS")])
def test_batch_pairs(env, k, knob, monkeypatch):
    """Wave per (query, block) pair, k_score_blocks for the pairs it leaves."""
    g = env.g
    if knob:
        monkeypatch.setenv(knob, "1")
    u0 = g.stats()["unit_batches"]
    res = g.search_batch(PLAIN, k)
    assert g.stats()["unit_batches"] == u0
    assert_batch(res, env.W, k, np.arange(len(PLAIN)), PLAIN)


def test_batch_all_hits(env):
    g, W = env.g, env.W
    idx = SAMPLE + list(range(len(PLAIN), len(ALL)))
    got = g.search_batch_all([ALL[i] for i in idx])
    for i, hits in zip(idx, got):
        assert_hits(hits, W.full[i], ALL[i])


# ---------------------------------------------------------------------------
# operator queries (the kOps instantiations)

def test_operator_queries(env):
    g, W = env.g, env.W
    ops = list(range(len(PLAIN), len(ALL)))
    for i in ops:
        assert len(W.full[i]) > 64
        for k in (1, 10, 64, 100, 0):
            assert_hits(g.search(ALL[i], k), W.full[i][:k] if k else W.full[i], (ALL[i], k))
    for k in (10, 65):
        # alone: too few (query, block) pairs for a batch, grid mode
        assert_batch(g.search_batch(OPS, k), W, k, np.array(ops), OPS)
        # with the plain queries: one operator query sends the batch through kOps
        u0 = g.stats()["unit_batches"]
        res = g.search_batch(ALL, k)
        assert g.stats()["unit_batches"] == u0
        assert_batch(res, W, k, np.arange(len(ALL)), ALL)


# ---------------------------------------------------------------------------
# term-major build (the kTerm instantiations)

def test_term_major_single(term_env):
    g, W = term_env.g, term_env.W
    f0 = g.stats()["fused_queries"]
    for i in SAMPLE:
        for k in (1, 10, 64):
            assert_hits(g.search(PLAIN[i], k), W.full[i][:k], (PLAIN[i], k))
    assert g.stats()["fused_queries"] - f0 >= 3 * sum(1 for i in SAMPLE if W.full[i])
    for i in SAMPLE:
        for k in (100, 1024, 0):
            assert_hits(g.search(PLAIN[i], k), W.full[i][:k] if k else W.full[i], (PLAIN[i], k))


def test_term_major_batches(term_env):
    g, W = term_env.g, term_env.W
    for k in (1, 10, 64, 65):
        assert_batch(g.search_batch(PLAIN, k), W, k, np.arange(len(PLAIN)), PLAIN)
    assert_batch(g.search_batch(ALL, 10), W, 10, np.arange(len(ALL)), ALL)
    idx = SAMPLE + list(range(len(PLAIN), len(ALL)))
    for i, hits in zip(idx, g.search_batch_all([ALL[i] for i in idx])):
        assert_hits(hits, W.full[i], ALL[i])


# ---------------------------------------------------------------------------
# corpus Z: zero-score waves beside one positive wave

Z_PARAMS = (16777216.0, 0.0)
Z_OFFSETS = (3, 200, 511, 700, 1023)
Z_QUERIES = [b"alpha", b"alpha beta", b"beta"]
Z_KS = [1, 5, 6, 12, 64, 100, 0]


def texts_z():
    block = [b"beta"] * 1024 + [b"alpha"] * 7168
    for off in Z_OFFSETS:
        block[off] = b"alpha alpha"
    return block * 2


@pytest.fixture(scope="module")
def zed():
    texts = texts_z()
    full = frozenset(range(len(Z_QUERIES)))
    W = Want(texts, Z_QUERIES, *Z_PARAMS, full)
    g = gpu_index(texts, *Z_PARAMS, L.INVERSION_BLOCK)
    gt = gpu_index(texts, *Z_PARAMS, L.INVERSION_TERM)
    yield g, gt, W
    g.close()
    gt.close()


def test_z_preconditions(zed):
    _, _, W = zed
    alpha = W.full[0]
    assert len(alpha) == 14346
    assert sum(1 for _, s in alpha if s == 0.0) == 14336
    pos = [off + 8192 * b for b in range(2) for off in Z_OFFSETS]
    assert [d for d, _ in alpha[:12]] == pos + [1024, 1025]
    assert bits_of([s for _, s in alpha[:12]]).tolist() == [bits_of([1.4901161e-08])[0]] * 10 + [0, 0]
    both = W.full[1]
    assert len(both) == 16384 and sum(1 for _, s in both if s == 0.0) == 16374
    assert [d for d, _ in both[:12]] == pos + [0, 1]


@pytest.mark.parametrize("k", Z_KS)
def test_z_single(zed, k, monkeypatch):
    g, gt, W = zed
    for i, q in enumerate(Z_QUERIES):
        want = W.full[i][:k] if k else W.full[i]
        assert_hits(g.search(q, k), want, (q, k, "block-major"))
        assert_hits(gt.search(q, k), want, (q, k, "term-major"))
    if k:
        monkeypatch.setenv("TFIDF_NO_FUSED", "1")
        for i, q in enumerate(Z_QUERIES):
            assert_hits(g.search(q, k), W.full[i][:k], (q, k, "unfused"))


@pytest.mark.parametrize("k", Z_KS)
def test_z_batch(zed, k):
    """A batch of three queries (grid mode), and one of 2100: the unit path for
    k <= 64, the wave-per-pair path for k = 100, which leaves these blocks (more
    postings than a wave's table holds) to k_score_blocks' list mode."""
    g, gt, W = zed
    if k == 0:
        qs = Z_QUERIES + [b"alpha"]
        for ix in (g, gt):
            for j, hits in enumerate(ix.search_batch_all(qs)):
                assert_hits(hits, W.full[j % 3], (qs[j], ix is gt))
        return
    want = [[(d, int(b)) for (d, _), b in zip(W.full[i][:k], bits_of([s for _, s in W.full[i][:k]]).tolist())]
            for i in range(3)]

    def rows(res, i):
        docs, scores, counts = res
        return list(zip(docs[i, :counts[i]].tolist(), scores.view(np.uint32)[i, :counts[i]].tolist()))

    for ix in (g, gt):
        res = ix.search_batch(Z_QUERIES, k)
        for i in range(3):
            assert rows(res, i) == want[i], (Z_QUERIES[i], k, ix is gt)
    big = Z_QUERIES * 700
    u0 = g.stats()["unit_batches"]
    res = g.search_batch(big, k)
    assert g.stats()["unit_batches"] == u0 + (1 if k <= 64 else 0)
    for i in range(len(big)):
        assert rows(res, i) == want[i % 3], (big[i], k, i)


# ---------------------------------------------------------------------------
# persistence: a file's (k1, b) must be the loading index's

def test_load_refuses_other_parameters(tmp_path):
    texts = texts_a()[:3000]
    path = str(tmp_path / "plain.tfidf")
    qs = [PLAIN[i] for i in SAMPLE] + OPS
    with ShardIndex(k1=2.0, b=1.0, vocab_capacity_log2=16) as g:
        g.add_documents(texts)
        g.commit()
        saved = [g.search(q, 0) for q in qs]
        g.save(path)
    assert sum(1 for h in saved if h) >= 40
    with ShardIndex(vocab_capacity_log2=16) as d:
        with pytest.raises(L.TfidfError) as e:
            d.load(path)
        assert e.value.code == L.E_INVALID_ARG
        msg = str(e.value)
        assert "k1" in msg and "(2, 1)" in msg and "(1.20000005, 0.75)" in msg, msg
        assert d.stats()["num_docs"] == 0                              # nothing was staged
        d.add_documents(texts[:10])                                    # and the index is still usable
        d.commit()
        assert d.stats()["num_docs"] == 10
    with ShardIndex(k1=2.0, b=0.99999994, vocab_capacity_log2=16) as d:   # one ulp off: bit patterns decide
        with pytest.raises(L.TfidfError) as e:
            d.load(path)
        assert e.value.code == L.E_INVALID_ARG
    with ShardIndex(k1=2.0, b=1.0, vocab_capacity_log2=16) as g2:
        g2.load(path)
        g2.commit()
        assert g2.stats()["num_docs"] == len(texts)
        for q, want in zip(qs, saved):
            assert_hits(g2.search(q, 0), want, q)
