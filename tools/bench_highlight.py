#!/usr/bin/env python3
"""Hit highlighting (tfidf_reader_snippets) against the only route without it:
download every hit document (tfidf_reader_doc_text) and run the host scanner
over its bytes (tfidf_analyze).  The match lookup and the passage step of that
route are left out, which flatters it.

Shapes (max_bytes 160, one three-term query):
  cfg2-top10      the top-10 hits on the cfg-2 synthetic corpus (--docs documents)
  cfg2-top1024    1024 hits of the same query
  book-1          one ~1 MB book-like document (--book-tokens tokens)
  book-64         64 of them
Per shape, median and [min, max] over --runs timed calls after --warmup:
  snippets.device_ms   ms_device of the call (HIP events on the call's stream)
  snippets.wall_ms     host clock around the call (it ends in a device synchronise)
  download_scan.wall_ms  the doc_text + analyze route on the same documents
plus the bytes of the documents, bytes returned, bytes scanned per device
second, and the commit's tokenizer time over the same corpus for comparison.
One JSON file per shape under --out-dir, and one line per shape on stdout.

Batch shapes (tfidf_reader_snippets_batch against the only route without it,
one tfidf_reader_snippets call per query on the same reader; a round alternates
the two, buffers allocated once):
  cfg2-batch-Q        Q in {1, 64, 1024} three-term queries (fixed seed), top-10 rows each
  cfg2-batch-1024x100 1024 queries, top-100 rows each
  node2-batch-1024    tfidf_node_snippets_batch on two shards of one device
                      (--node-docs documents) against one tfidf_snippets call
                      per (query, shard), routed by hand
Per shape: device and wall median [min, max] of both routes, bytes scanned per
device second of both, the row chunks of the batched call, and whether the
batch's slowest round beat the loop's fastest.  The loop of single calls is
still the route to compare against: Q chains of launches against one.  At
Q = 1 the two are the same code (the library serves a single-query call as the
batch of one query), so cfg2-batch-1 measures the ctypes call path alone.
The single-query shapes record item_chunks / row_chunks through a one-query
batch call over the same rows: a single-form call does not report its chunks.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tf-idf-distributed-system_amd"))

from tfidf_amd import _lib as L  # noqa: E402
from tfidf_amd import synth  # noqa: E402


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def download_scan(rd, docs, buf):
    """The parent route: every document's bytes to the host, the host scanner over them."""
    lib = L.load()
    nt, nb = C.c_uint64(), C.c_uint64()
    total = 0
    for d in docs:
        text = rd.doc_text(int(d))
        L.check(lib.tfidf_analyze(text, len(text), buf, len(buf), C.byref(nt), C.byref(nb)))
        total += nt.value
    return total


def measure(name, g, rd, q, docs, runs, warmup, extra):
    docs = np.ascontiguousarray(docs, dtype=np.uint32)
    sizes = [len(rd.doc_text(int(d))) for d in docs]
    buf = C.create_string_buffer(2 * max(sizes + [1]) + 64)
    dev, wall, par = [], [], []
    out = None
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        out = rd.snippets_arrays(q, docs, 160)
        t1 = time.perf_counter()
        download_scan(rd, docs, buf)
        t2 = time.perf_counter()
        if r >= warmup:
            dev.append(out[7])
            wall.append((t1 - t0) * 1e3)
            par.append((t2 - t1) * 1e3)
    text, _, _, st, _, _, _, _ = out
    rd.snippets_batch_arrays([q], [docs], 160)             # the same rows as a batch of one: only batched calls
    item_chunks, row_chunks = g.last_highlight_chunks()    # report their row chunks
    nbytes = int(sum(sizes))
    res = {"shape": name, "query": q.decode(), "hits": int(len(docs)), "runs": runs, "warmup": warmup,
           "document_bytes": nbytes, "snippet_bytes": len(text), "snippet_matches": int(len(st)),
           "returned_bytes": len(text) + 16 * int(len(st)) + 24 * int(len(docs)),
           "snippets": {"device_ms": spread(dev), "wall_ms": spread(wall)},
           "download_scan": {"wall_ms": spread(par)}, "item_chunks": item_chunks, "row_chunks": row_chunks}
    res["scan_GBs_device"] = nbytes / (res["snippets"]["device_ms"]["median"] * 1e-3) / 1e9
    res["wall_speedup_over_download_scan"] = res["download_scan"]["wall_ms"]["median"] / \
        res["snippets"]["wall_ms"]["median"]
    res.update(extra)
    return res


class RawSnippets:
    """tfidf_*_snippets[_batch] through ctypes into buffers allocated once, so
    neither route of measure_batch pays for Python-side allocation."""

    def __init__(self, n_rows, W, docs_dtype=np.uint32):
        self.W = W
        self.t_cap, self.m_cap = n_rows * W, n_rows * (W // 2 + 1)     # a match and its separator: >= 2 bytes
        self.text = np.empty(max(self.t_cap, 1), np.uint8)
        self.t_offs = np.zeros(n_rows + 1, np.uint64)
        self.m_offs = np.zeros(n_rows + 1, np.uint64)
        self.d_starts = np.zeros(max(n_rows, 1), np.uint64)
        self.st = np.empty(max(self.m_cap, 1), np.uint64)
        self.ln = np.empty(max(self.m_cap, 1), np.uint32)
        self.od = np.empty(max(self.m_cap, 1), np.uint32)
        self.nt, self.nm, self.ms = C.c_uint64(), C.c_uint64(), C.c_float()
        self.dt = np.ctypeslib.as_ctypes_type(docs_dtype)

    def tail(self):
        return (self.W, self.text.ctypes.data_as(C.c_void_p), self.t_cap, L.ptr(self.t_offs, C.c_uint64),
                L.ptr(self.d_starts, C.c_uint64), L.ptr(self.st, C.c_uint64), L.ptr(self.ln, C.c_uint32),
                L.ptr(self.od, C.c_uint32), self.m_cap, L.ptr(self.m_offs, C.c_uint64), C.byref(self.nt),
                C.byref(self.nm), C.byref(self.ms))

    def batch(self, fn, handle, blob, q_offs, n_q, docs, d_offs):
        L.check(fn(handle, blob, L.ptr(q_offs, C.c_uint64), n_q, L.ptr(docs, self.dt), L.ptr(d_offs, C.c_uint64),
                   *self.tail()))
        return self.ms.value

    def single(self, fn, handle, q, docs):
        L.check(fn(handle, q, len(q), L.ptr(docs, C.c_uint32), len(docs), *self.tail()))
        return self.ms.value


def measure_batch(name, batch_call, loop_call, chunks, n_q, rows, nbytes, runs, warmup, extra):
    """A round alternates the two routes: one batched call, and the only route
    without it, one single-query call per query (per query and shard on a
    node).  Each returns (device ms, snippet bytes, in-snippet matches)."""
    dev, wall, ldev, lwall = [], [], [], []
    out = lout = None
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        out = batch_call()
        t1 = time.perf_counter()
        lout = loop_call()
        t2 = time.perf_counter()
        if r >= warmup:
            dev.append(out[0])
            wall.append((t1 - t0) * 1e3)
            ldev.append(lout[0])
            lwall.append((t2 - t1) * 1e3)
    assert out[1:] == lout[1:], (out, lout)                # the same snippets and matches in total
    res = {"shape": name, "queries": n_q, "rows": rows, "runs": runs, "warmup": warmup, "document_bytes": nbytes,
           "snippet_bytes": out[1], "snippet_matches": out[2],
           "batch": {"device_ms": spread(dev), "wall_ms": spread(wall)},
           "loop_of_single_calls": {"device_ms": spread(ldev), "wall_ms": spread(lwall)},
           "item_chunks": chunks()[0], "row_chunks": chunks()[1]}
    res["scan_GBs_device"] = nbytes / (res["batch"]["device_ms"]["median"] * 1e-3) / 1e9
    res["loop_scan_GBs_device"] = nbytes / (res["loop_of_single_calls"]["device_ms"]["median"] * 1e-3) / 1e9
    res["wall_speedup_over_loop"] = res["loop_of_single_calls"]["wall_ms"]["median"] / res["batch"]["wall_ms"]["median"]
    res["batch_max_below_loop_min"] = res["batch"]["wall_ms"]["max"] < res["loop_of_single_calls"]["wall_ms"]["min"]
    res.update(extra)
    return res


def top_rows(docs, offs, k):
    """The first k hits of every query of a search_batch_all result, CSR."""
    o = offs.astype(np.int64)
    per = [docs[o[i]:min(o[i + 1], o[i] + k)] for i in range(len(o) - 1)]
    d_offs = np.zeros(len(per) + 1, np.uint64)
    d_offs[1:] = np.cumsum([len(p) for p in per], dtype=np.uint64)
    return per, np.ascontiguousarray(np.concatenate(per)), d_offs


def doc_lengths(dc):
    """Byte length of every document of a DeviceCorpus (its offsets alone come to the host)."""
    offs = np.zeros(dc.n_docs + 1, np.uint64)
    synth._d2h(offs, dc.d_offsets, (dc.n_docs + 1) * 8, dc.device)
    return np.diff(offs.astype(np.int64))


def batch_shape(name, g, rd, queries, k, lens, runs, warmup, extra):
    lib = L.load()
    docs, _, offs = rd.search_batch_all_arrays(queries)
    per, flat, d_offs = top_rows(docs.astype(np.uint32), offs, k)
    per = [np.ascontiguousarray(p) for p in per]
    blob = b"".join(queries)
    q_offs = np.zeros(len(queries) + 1, np.uint64)
    q_offs[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
    raw = RawSnippets(len(flat), 160)
    nbytes = int(lens[flat.astype(np.int64)].sum())

    def batch_call():
        ms = raw.batch(lib.tfidf_reader_snippets_batch, rd._h, blob, q_offs, len(queries), flat, d_offs)
        return ms, raw.nt.value, raw.nm.value

    def loop_call():
        ms = nt = nm = 0
        for q, p in zip(queries, per):
            ms += raw.single(lib.tfidf_reader_snippets, rd._h, q, p)
            nt += raw.nt.value
            nm += raw.nm.value
        return ms, nt, nm
    return measure_batch(name, batch_call, loop_call, g.last_highlight_chunks, len(queries), int(len(flat)), nbytes,
                         runs, warmup, extra)


def node_shape(name, n_docs, n_q, k, runs, warmup):
    """Two shards on device 0, in-process, GLOBAL statistics; the loop is one
    tfidf_snippets call per (query, shard with rows), routed by hand."""
    from tfidf_amd import distributed as D
    lib = L.load()
    dc = synth.DeviceCorpus(n_docs, V=100_000, len_min=400, len_max=600)
    text, offsets = dc.to_host()
    dc.free()
    node = D.Node(devices=[0, 0], stats_mode=L.STATS_GLOBAL)
    half = n_docs // 2
    for g, (a, z) in enumerate(((0, half), (half, n_docs))):
        offs = np.ascontiguousarray(offsets[a:z + 1] - offsets[a])
        L.check(lib.tfidf_node_add_docs(node._h, g, C.cast(text[int(offsets[a]):].ctypes.data, C.c_char_p),
                                        L.ptr(offs, C.c_uint64), z - a, None, None))
    node.commit()
    queries = synth.queries(n_q, n_terms=3)
    docs, _, offs = node.search_batch_all_arrays(queries)
    per, flat, d_offs = top_rows(docs.astype(np.uint64), offs, k)
    blob = b"".join(queries)
    q_offs = np.zeros(n_q + 1, np.uint64)
    q_offs[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
    raw = RawSnippets(len(flat), 160, np.uint64)
    lens = np.diff(offsets.astype(np.int64))
    nbytes = int(lens[flat.astype(np.int64)].sum())
    shards = [node.shard(0), node.shard(1)]
    routed = [[np.ascontiguousarray(p[p < half], dtype=np.uint32),
               np.ascontiguousarray(p[p >= half] - half, dtype=np.uint32)] for p in per]

    def batch_call():
        ms = raw.batch(lib.tfidf_node_snippets_batch, node._h, blob, q_offs, n_q, flat, d_offs)
        return ms, raw.nt.value, raw.nm.value

    def loop_call():
        ms = nt = nm = 0
        for q, parts in zip(queries, routed):
            for h, p in zip(shards, parts):
                if len(p):
                    ms += raw.single(lib.tfidf_snippets, h, q, p)
                    nt += raw.nt.value
                    nm += raw.nm.value
        return ms, nt, nm

    def chunks():
        a, b = C.c_uint64(), C.c_uint64()
        tot = [0, 0]
        for h in shards:
            L.check(lib.tfidf_last_highlight_chunks(h, C.byref(a), C.byref(b)))
            tot = [tot[0] + a.value, tot[1] + b.value]
        return tot
    res = measure_batch(name, batch_call, loop_call, chunks, n_q, int(len(flat)), nbytes, runs, warmup,
                        {"corpus": "node of 2 shards on one device: %d docs x U[400,600] tokens, V=100000" % n_docs,
                         "note": "batch device_ms is the larger of the two shards' device times; chunks summed over shards"})
    node.close()
    return res


def commit_rates(g):
    t = g.commit_timing()
    return {"commit_ms_tokenize": t["ms_tokenize"], "commit_ms_long": t["ms_long"],
            "commit_text_bytes": int(t["text_bytes"]),
            "commit_tokenize_GBs": t["text_bytes"] / max((t["ms_tokenize"] + t["ms_long"]) * 1e-3, 1e-9) / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000, help="documents of the cfg-2 corpus")
    ap.add_argument("--book-tokens", type=int, default=200_000, help="tokens per book-like document (~1 MB)")
    ap.add_argument("--books", type=int, default=64)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "highlight"))
    ap.add_argument("--node-docs", type=int, default=200_000, help="documents of the two-shard node (host staged)")
    ap.add_argument("--skip", default="", help="comma-separated shapes to leave out (cfg2, book, batch, node)")
    args = ap.parse_args()
    from tfidf_amd.engine import ShardIndex
    os.makedirs(args.out_dir, exist_ok=True)
    skip = set(args.skip.split(",")) if args.skip else set()

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        with open(os.path.join(args.out_dir, res["shape"] + ".json"), "w") as f:
            f.write(line + "\n")

    if "cfg2" not in skip:
        n = args.docs
        dc = synth.DeviceCorpus(n, V=100_000, len_min=400, len_max=600)
        g = ShardIndex(vocab_capacity_log2=19)
        g.add_documents_device(dc.d_text, dc.d_offsets, n, dc.total_bytes)
        g.commit()
        q = synth.queries(1, n_terms=3)[0]
        extra = dict(commit_rates(g), corpus="cfg2: %d docs x U[400,600] tokens, V=100000" % n)
        with g.reader() as rd:
            top = rd.search_arrays(q, 1024)[0]
            # a single top-10 search for scale: wall p50 of the same query
            lat = []
            for _ in range(args.warmup + 200):
                t0 = time.perf_counter()
                rd.search_arrays(q, 10)
                lat.append((time.perf_counter() - t0) * 1e3)
            extra["search_top10_wall_ms_p50"] = float(np.median(lat[args.warmup:]))
            emit(measure("cfg2-top10", g, rd, q, top[:10], args.runs, args.warmup, extra))
            emit(measure("cfg2-top1024", g, rd, q, top, args.runs, args.warmup, extra))
            if "batch" not in skip:
                lens = doc_lengths(dc)
                bx = {"corpus": extra["corpus"]}
                for nq in (1, 64, 1024):
                    emit(batch_shape("cfg2-batch-%d" % nq, g, rd, synth.queries(nq, n_terms=3), 10, lens, args.runs,
                                     args.warmup, bx))
                emit(batch_shape("cfg2-batch-1024x100", g, rd, synth.queries(1024, n_terms=3), 100, lens, args.runs,
                                 args.warmup, bx))
        g.close()
        dc.free()
    if "node" not in skip:
        emit(node_shape("node2-batch-1024", args.node_docs, 1024, 10, args.runs, args.warmup))
    if "book" not in skip:
        nb, T = args.books, args.book_tokens
        dc = synth.DeviceCorpus(nb, V=100_000, len_min=T, len_max=T, seed=synth.SEED + 29)
        g = ShardIndex(vocab_capacity_log2=19)
        g.add_documents_device(dc.d_text, dc.d_offsets, nb, dc.total_bytes)
        g.commit()
        q = synth.queries(1, n_terms=3)[0]
        extra = dict(commit_rates(g), corpus="books: %d docs x %d tokens, V=100000" % (nb, T))
        with g.reader() as rd:
            emit(measure("book-1", g, rd, q, [0], args.runs, args.warmup, extra))
            emit(measure("book-%d" % nb, g, rd, q, list(range(nb)), args.runs, args.warmup, extra))
        g.close()
        dc.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
