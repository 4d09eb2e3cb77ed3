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


def measure(name, rd, q, docs, runs, warmup, extra):
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
    nbytes = int(sum(sizes))
    res = {"shape": name, "query": q.decode(), "hits": int(len(docs)), "runs": runs, "warmup": warmup,
           "document_bytes": nbytes, "snippet_bytes": len(text), "snippet_matches": int(len(st)),
           "returned_bytes": len(text) + 16 * int(len(st)) + 24 * int(len(docs)),
           "snippets": {"device_ms": spread(dev), "wall_ms": spread(wall)},
           "download_scan": {"wall_ms": spread(par)}}
    res["scan_GBs_device"] = nbytes / (res["snippets"]["device_ms"]["median"] * 1e-3) / 1e9
    res["wall_speedup_over_download_scan"] = res["download_scan"]["wall_ms"]["median"] / \
        res["snippets"]["wall_ms"]["median"]
    res.update(extra)
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
    ap.add_argument("--skip", default="", help="comma-separated shapes to leave out (cfg2, book)")
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
            emit(measure("cfg2-top10", rd, q, top[:10], args.runs, args.warmup, extra))
            emit(measure("cfg2-top1024", rd, q, top, args.runs, args.warmup, extra))
        g.close()
        dc.free()
    if "book" not in skip:
        nb, T = args.books, args.book_tokens
        dc = synth.DeviceCorpus(nb, V=100_000, len_min=T, len_max=T, seed=synth.SEED + 29)
        g = ShardIndex(vocab_capacity_log2=19)
        g.add_documents_device(dc.d_text, dc.d_offsets, nb, dc.total_bytes)
        g.commit()
        q = synth.queries(1, n_terms=3)[0]
        extra = dict(commit_rates(g), corpus="books: %d docs x %d tokens, V=100000" % (nb, T))
        with g.reader() as rd:
            emit(measure("book-1", rd, q, [0], args.runs, args.warmup, extra))
            emit(measure("book-%d" % nb, rd, q, list(range(nb)), args.runs, args.warmup, extra))
        g.close()
        dc.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
