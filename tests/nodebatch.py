"""Helpers of the node-level all-hits batch tests (test_gpu_node_batch_all.py):
corpora, single-index and per-worker oracles, nodes on one device, rank
threads under a join timeout."""
import threading

from oracle import oracle as O
from tfidf_amd import distributed as D
from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

# corpus C: hand-routed shards.  Under GLOBAL statistics the five "tie word"
# documents score identically (same tf, same length, same global df): the merge
# must order them by global doc id across ranks.  "left" hits only shard 0 and
# "right" only shard 2: (rank, query) segments empty at the last / first ranks.
C_SHARDS = [
    [b"left common", b"tie word", b"tie word", b"common filler"],
    [b"tie word", b"common filler filler", b"tie word"],
    [b"right common", b"tie word", b"right right"],
]
C_QUERIES = [b"left", b"right", b"tie", b"common", b"left right", b"nothing", b"tie word"]


def corpus_b():
    """20 000 short documents: 2 shards of 2 blocks, or 3 of one; names repeat
    across shards (i and i + 10 000), never within one at world 2 or 3."""
    texts = synth.corpus(20_000, V=2000, len_min=2, len_max=12)
    names = [b"f%05d.txt" % (i % 10000) for i in range(len(texts))]
    return texts, names


def oracle_hits(o, q):
    try:
        return o.search(q, 0)
    except O.QuerySyntaxError:
        return []                                     # Worker.java:182-185: the request answers []


def oracle_global(texts, queries):
    """search(q, 0) of every query on one index of all the documents."""
    o = O.OracleIndex()
    for i, t in enumerate(texts):
        o.add_doc(str(i).encode(), t)
    o.commit()
    out = [oracle_hits(o, q) for q in queries]
    o.close()
    return out


def oracle_shard(texts, names, world, queries, skip=()):
    """Per-worker oracles over the contiguous shards + the Leader merge, per
    query; also, per query, the number of names that sum two workers' scores."""
    workers = []
    for r in range(world):
        if r in skip:
            continue
        lo, hi = D.shard_range(len(texts), r, world)
        o = O.OracleIndex()
        for n, t in zip(names[lo:hi], texts[lo:hi]):
            o.add_doc(n, t)
        o.commit()
        workers.append(o)
    merged, shared = [], []
    for q in queries:
        resp = [[(o.doc_key(d), float(s)) for d, s in oracle_hits(o, q)] for o in workers]
        merged.append(O.leader_merge(resp))
        seen = {}
        for rs in resp:
            for n in {n for n, _ in rs}:
                seen[n] = seen.get(n, 0) + 1
        shared.append(sum(1 for v in seen.values() if v >= 2))
    for o in workers:
        o.close()
    return merged, shared


def make_node(texts, names, shards, mode):
    n = D.Node(devices=[0] * shards, stats_mode=mode)
    n.add_documents(texts, names)
    n.commit()
    return n


def make_ranks(texts, names, world, bases=None):
    """SPMD over Comm.inproc(world): one committed ShardIndex per rank on device 0."""
    comms = D.Comm.inproc(world)
    idx, ads = [], []
    for r in range(world):
        lo, hi = D.shard_range(len(texts), r, world)
        ix = ShardIndex(device=0)
        ix.add_documents(texts[lo:hi], names[lo:hi])
        ix.commit()
        idx.append(ix)
        ads.append(D.DistShard(ix, comms[r], doc_base=lo if bases is None else bases[r]))
    return comms, idx, ads


def close_ranks(comms, idx):
    for c in comms:
        c.close()
    for i in idx:
        i.close()


def run_ranks(fns, timeout=60):
    """fns[r]() on one thread per rank; per-rank (result, exception).  A rank
    left in a collective is a failed assertion, not a stuck suite."""
    out = [None] * len(fns)

    def body(r):
        try:
            out[r] = (fns[r](), None)
        except Exception as e:            # noqa: BLE001 - reported per rank
            out[r] = (None, e)

    th = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(len(fns))]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout)
    assert not any(t.is_alive() for t in th), "a rank is still waiting in a collective"
    return out
