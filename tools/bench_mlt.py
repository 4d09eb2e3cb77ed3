#!/usr/bin/env python3
"""More-like-this (tfidf_reader_more_like_this_batch) against the route a
caller had without it, through calls that exist without the feature: per seed
tfidf_doc_terms (five small blocking copies and a host decode of every term
string of the row), tfidf_term_df for every term not seen before, the
selection in Python, a query string per seed and one tfidf_search_batch with
k + 1 (the seed dropped afterwards).

Shapes:
  cfg2-mlt-N   N in {1, 64, 1024} seeds on the cfg-2 synthetic corpus (--docs documents)
  book-mlt-N   the same seed counts on --books ~1 MB book-like documents (seeds repeat)
Seeds are drawn with a fixed seed.  The host route runs on a seeded subset of
the seeds (--host-seeds; the JSON says how many), and both routes must give the
same hits and score bits on that subset before anything is timed.  Per shape,
median and [min, max] over --runs timed rounds after --warmup (a round
alternates the two routes):
  device.wall_ms     host clock around the batched call
  device.device_ms   HIP events around the whole call on its stream (tfidf_last_search_ms total)
  device.terms_wall_ms / terms_device_ms   the same for tfidf_reader_mlt_terms_batch alone
  host.wall_ms       the host route over its subset, with its steps: doc_terms, df, select, search
plus the forward-row entries the device scanned, the candidate chunks, and
idf_table_first_call_ms: the first call on the fresh index (which builds and
uploads the snapshot's idf table, and also creates the search context's buffers
and loads the sort's code) minus the median later call of the same seed; the
book corpus' 260-byte table shows how much of it is not the table.
One JSON file per shape under --out-dir, one line per shape on stdout.
"""
import argparse
import ctypes as C
import json
import math
import os
import random
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tf-idf-distributed-system_amd"))

from tfidf_amd import _lib as L  # noqa: E402
from tfidf_amd import synth  # noqa: E402
from tfidf_amd.engine import ShardIndex, mlt_params  # noqa: E402

SEED = 20261020
K = 10


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def bits(x):
    return int(np.float32(x).view(np.uint32))


class HostRoute:
    """doc_terms per seed, df per new term, selection in Python, search_batch."""

    def __init__(self, g, n_docs):
        self.g, self.n = g, n_docs
        self.t = {"doc_terms": 0.0, "df": 0.0, "select": 0.0, "search": 0.0}

    def run(self, seeds, p):
        g, t = self.g, self.t
        df_of, queries = {}, []                           # a caller would keep the df of a batch's terms
        for d in seeds:
            t0 = time.perf_counter()
            row = g.doc_terms(d)                          # {term: tf}
            t1 = time.perf_counter()
            for term in row:
                if term not in df_of:
                    df_of[term] = g.df(term)[0]
            t2 = time.perf_counter()
            cands = []
            for term, tf in row.items():
                df = df_of[term]
                if tf >= max(p.min_tf, 1) and df >= p.min_df and (p.max_df == 0 or df <= p.max_df):
                    idf = np.float32(math.log((self.n + 1) / float(df + 1)) + 1.0)
                    cands.append((-bits(np.float32(tf) * idf), term))
            cands.sort()
            queries.append(b" ".join(term for _, term in cands[:p.max_terms]))
            t3 = time.perf_counter()
            t["doc_terms"] += t1 - t0
            t["df"] += t2 - t1
            t["select"] += t3 - t2
        t0 = time.perf_counter()
        docs, scores, counts = g.search_batch(queries, K + 1)
        t["search"] += time.perf_counter() - t0
        lists = [list(zip(docs[i, :c].tolist(), scores[i, :c].tolist())) for i, c in enumerate(counts.tolist())]
        return [[(e, s) for e, s in h if e != d][:K] for h, d in zip(lists, seeds)]


class RawMlt:
    """tfidf_reader_more_like_this_batch / _mlt_terms_batch into buffers allocated once."""

    def __init__(self, rd, seeds, p):
        self.rd, self.p, self.n = rd, p, len(seeds)
        self.seeds = np.array(seeds, np.uint32)
        self.docs = np.zeros((self.n, K), np.uint32)
        self.scores = np.zeros((self.n, K), np.float32)
        self.cnt = np.zeros(self.n, np.uint32)
        cap = self.n * p.max_terms
        self.t_offs, self.cand = np.zeros(self.n + 1, np.uint64), np.zeros(self.n, np.uint64)
        self.b_offs, self.blob = np.zeros(cap + 1, np.uint64), np.zeros(cap * 64, np.uint8)
        self.tf, self.df, self.sc = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.float32)
        self.nt, self.nb, self.cap = C.c_uint64(), C.c_uint64(), cap

    def call(self):
        L.check(L.load().tfidf_reader_more_like_this_batch(
            self.rd._h, L.ptr(self.seeds, C.c_uint32), self.n, C.byref(self.p), K, L.MLT_EXCLUDE_SEED,
            L.ptr(self.docs, C.c_uint32), L.ptr(self.scores, C.c_float), L.ptr(self.cnt, C.c_uint32)))

    def call_terms(self):
        L.check(L.load().tfidf_reader_mlt_terms_batch(
            self.rd._h, L.ptr(self.seeds, C.c_uint32), self.n, C.byref(self.p), L.ptr(self.t_offs, C.c_uint64),
            L.ptr(self.cand, C.c_uint64), L.ptr(self.b_offs, C.c_uint64), self.blob.ctypes.data_as(C.c_void_p),
            len(self.blob), L.ptr(self.tf, C.c_uint32), L.ptr(self.df, C.c_uint32), L.ptr(self.sc, C.c_float), self.cap,
            C.byref(self.nt), C.byref(self.nb)))

    def hits(self, i):
        c = int(self.cnt[i])
        return list(zip(self.docs[i, :c].tolist(), self.scores[i, :c].tolist()))


def shape(name, g, rd, n_seeds, n_host, runs, warmup, extra):
    rng = random.Random(SEED + n_seeds)
    seeds = [rng.randrange(rd.num_docs) for _ in range(n_seeds)]
    sub = sorted(rng.sample(range(n_seeds), min(n_host, n_seeds)))
    p = mlt_params()
    raw = RawMlt(rd, seeds, p)
    raw.call()
    entries, chunks = g.last_mlt_stats()
    host = HostRoute(g, rd.num_docs)
    # the same hits and score bits on the subset, before anything is timed
    want = host.run([seeds[i] for i in sub], p)
    for i, w in zip(sub, want):
        got = raw.hits(i)
        assert [(d, bits(s)) for d, s in got] == [(d, bits(s)) for d, s in w], (name, seeds[i], got[:3], w[:3])
    host.t = dict.fromkeys(host.t, 0.0)
    wall, dev, twall, tdev, hwall = [], [], [], [], []
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        raw.call()
        t1 = time.perf_counter()
        ms = g.last_search_ms()[1]
        t2 = time.perf_counter()
        raw.call_terms()
        t3 = time.perf_counter()
        tms = g.last_search_ms()[1]
        if r == warmup:
            host.t = dict.fromkeys(host.t, 0.0)
        t4 = time.perf_counter()
        host.run([seeds[i] for i in sub], p)
        t5 = time.perf_counter()
        if r >= warmup:
            wall.append((t1 - t0) * 1e3)
            dev.append(ms)
            twall.append((t3 - t2) * 1e3)
            tdev.append(tms)
            hwall.append((t5 - t4) * 1e3)
    res = {"shape": name, "seeds": n_seeds, "k": K, "runs": runs, "warmup": warmup,
           "params": {f: getattr(p, f) for f, _ in L.MltParams._fields_},
           "row_entries_scanned": int(entries), "cand_chunks": int(chunks), "terms_selected": int(raw.nt.value),
           "candidates": int(raw.cand.sum()),
           "device": {"wall_ms": spread(wall), "device_ms": spread(dev), "terms_wall_ms": spread(twall),
                      "terms_device_ms": spread(tdev)},
           "host": {"seeds": len(sub), "wall_ms": spread(hwall),
                    "steps_ms_per_round": {k: v * 1e3 / runs for k, v in host.t.items()}},
           "note": "the host route ran on a seeded subset of %d of the %d seeds" % (len(sub), n_seeds)}
    res["device"]["wall_ms_per_seed"] = res["device"]["wall_ms"]["median"] / n_seeds
    res["host"]["wall_ms_per_seed"] = res["host"]["wall_ms"]["median"] / len(sub)
    res["wall_per_seed_speedup_over_host"] = res["host"]["wall_ms_per_seed"] / res["device"]["wall_ms_per_seed"]
    res.update(extra)
    return res


def first_call_cost(g, rd):
    """The first more-like-this call on a fresh snapshot against later calls of the same seed (wall ms)."""
    raw = RawMlt(rd, [0], mlt_params())
    t0 = time.perf_counter()
    raw.call_terms()
    first = (time.perf_counter() - t0) * 1e3
    later = []
    for _ in range(5):
        t0 = time.perf_counter()
        raw.call_terms()
        later.append((time.perf_counter() - t0) * 1e3)
    return {"idf_table_first_call_ms": first - float(np.median(later)), "first_call_ms": first,
            "later_call_ms": float(np.median(later)), "idf_table_bytes": 4 * (rd.num_docs + 1)}


def corpus(n, lo, hi, seed=None):
    dc = synth.DeviceCorpus(n, V=100_000, len_min=lo, len_max=hi, **({} if seed is None else {"seed": seed}))
    g = ShardIndex(vocab_capacity_log2=19)
    g.add_documents_device(dc.d_text, dc.d_offsets, n, dc.total_bytes)
    g.commit()
    return dc, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000, help="documents of the cfg-2 corpus")
    ap.add_argument("--book-tokens", type=int, default=200_000, help="tokens per book-like document (~1 MB)")
    ap.add_argument("--books", type=int, default=64)
    ap.add_argument("--host-seeds", type=int, default=64, help="seeds the host route runs on (cfg2)")
    ap.add_argument("--host-book-seeds", type=int, default=2, help="seeds the host route runs on (books)")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "mlt"))
    ap.add_argument("--skip", default="", help="comma-separated shapes to leave out (cfg2, book)")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    skip = set(args.skip.split(",")) if args.skip else set()
    batches = [int(x) for x in args.batches.split(",")]

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        with open(os.path.join(args.out_dir, res["shape"] + ".json"), "w") as f:
            f.write(line + "\n")

    def run(tag, dc, g, n_host, extra):
        with g.reader() as rd:
            extra = dict(extra, **first_call_cost(g, rd))
            for n in batches:
                emit(shape("%s-mlt-%d" % (tag, n), g, rd, n, n_host, args.runs, args.warmup, extra))
        g.close()
        dc.free()

    if "cfg2" not in skip:
        dc, g = corpus(args.docs, 400, 600)
        run("cfg2", dc, g, args.host_seeds, {"corpus": "cfg2: %d docs x U[400,600] tokens, V=100000" % args.docs})
    if "book" not in skip:
        T = args.book_tokens
        dc, g = corpus(args.books, T, T, synth.SEED + 29)
        run("book", dc, g, args.host_book_seeds, {"corpus": "books: %d docs x %d tokens, V=100000" % (args.books, T)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
