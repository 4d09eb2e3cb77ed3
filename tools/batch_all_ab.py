#!/usr/bin/env python3
"""All hits of 256 queries on the cfg-2 index (1 M documents generated on the
device): (a) 256 x tfidf_search(k = 0), (b) one tfidf_search_batch_all.

Per variant: warm-up rounds, then --runs timed rounds; wall time of the C calls
alone (ctypes, preallocated result arrays) and device time (the library's HIP
events: tfidf_last_search_ms, summed over the 256 calls for (a)), reported as
median and [min, max] over the rounds, plus the hits returned.  One JSON line.

--lib PATH times another build of the library (the parent commit's, for the
yardstick of (a)); exports that build lacks are skipped, and (b) is timed only
where tfidf_search_batch_all exists.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="libtfidf.so to time (default: this tree's build)")
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--label", default="")
    ap.add_argument("--chunk", type=int, default=0,
                    help="queries per chunk of (b) (TFIDF_ALLHITS_CHUNK; 0 = the library's scratch budget decides)")
    ap.add_argument("--skip-single", action="store_true", help="time (b) only (one (a) round for the hit count)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.lib:
        L.LIB_PATH = os.path.abspath(args.lib)
        probe = C.CDLL(L.LIB_PATH)
        for name in list(L.SIGNATURES):
            if not hasattr(probe, name):
                del L.SIGNATURES[name]
    if args.chunk:
        os.environ["TFIDF_DEBUG"] = "1"
        os.environ["TFIDF_ALLHITS_CHUNK"] = str(args.chunk)
    from tfidf_amd.engine import ShardIndex
    lib = L.load()
    dc = synth.DeviceCorpus(args.docs)
    g = ShardIndex()
    g.add_documents_device(dc.d_text, dc.d_offsets, dc.n_docs, dc.total_bytes)
    g.commit()
    qs = synth.queries(args.queries)                  # 3 terms, ranks in [100, 10 000)
    nq = len(qs)
    a, b = C.c_float(), C.c_float()
    n = C.c_uint64()
    res = {"label": args.label, "lib": os.path.relpath(L.LIB_PATH, REPO), "docs": args.docs, "queries": nq, "warmup": args.warmup,
           "runs": args.runs, "n_blocks": (args.docs + 8191) // 8192}

    # (a) one tfidf_search(k = 0) per query
    docs = np.empty(args.docs, np.uint32)
    scores = np.empty(args.docs, np.float32)
    pd, ps = L.ptr(docs, C.c_uint32), L.ptr(scores, C.c_float)
    wall, dev, hits = [], [], 0
    rounds = 1 if args.skip_single else args.warmup + args.runs
    for r in range(rounds):
        t_dev, hits = 0.0, 0
        t0 = time.perf_counter()
        for q in qs:
            L.check(lib.tfidf_search(g._h, q, len(q), 0, pd, ps, args.docs, C.byref(n)))
            lib.tfidf_last_search_ms(g._h, C.byref(a), C.byref(b))
            t_dev += b.value
            hits += n.value
        t1 = time.perf_counter()
        if r >= args.warmup or args.skip_single:
            wall.append((t1 - t0) * 1e3)
            dev.append(t_dev)
    res["single"] = {"hits": hits, "wall_ms": spread(wall), "device_ms": spread(dev),
                     "wall_us_per_query": float(np.median(wall)) * 1e3 / nq}

    # (b) one tfidf_search_batch_all
    if "tfidf_search_batch_all" in L.SIGNATURES:
        offs = np.zeros(nq + 1, np.uint64)
        offs[1:] = np.cumsum([len(q) for q in qs], dtype=np.uint64)
        blob = b"".join(qs)
        ho = np.zeros(nq + 1, np.uint64)
        bd = np.empty(max(hits, 1), np.uint32)
        bs = np.empty(max(hits, 1), np.float32)
        wall, dev = [], []
        for r in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            L.check(lib.tfidf_search_batch_all(g._h, blob, L.ptr(offs, C.c_uint64), nq, L.ptr(bd, C.c_uint32),
                                               L.ptr(bs, C.c_float), len(bd), L.ptr(ho, C.c_uint64), C.byref(n)))
            t1 = time.perf_counter()
            lib.tfidf_last_search_ms(g._h, C.byref(a), C.byref(b))
            if r >= args.warmup:
                wall.append((t1 - t0) * 1e3)
                dev.append(b.value)
        # the last single search's hits are still in docs / scores: the batch's last query must equal them
        last = slice(int(ho[nq - 1]), int(ho[nq]))
        m = last.stop - last.start
        same = bool(n.value == hits and (bd[last] == docs[:m]).all() and (bs[last] == scores[:m]).all())
        res["batch_all"] = {"hits": int(n.value), "wall_ms": spread(wall), "device_ms": spread(dev),
                            "wall_us_per_query": float(np.median(wall)) * 1e3 / nq,
                            "chunk_budget_bytes": 1 << 30, "chunk_queries_forced": args.chunk, "equals_single": same,
                            "device_spans_chunks": "first chunk's scoring start to last chunk's merge end"}
        res["wall_ratio_single_over_batch"] = res["single"]["wall_ms"]["median"] / res["batch_all"]["wall_ms"]["median"]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    g.close()
    dc.free()


if __name__ == "__main__":
    main()
