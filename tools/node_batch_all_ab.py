#!/usr/bin/env python3
"""All hits of 256 queries on a node (tfidf_node_*) over device 0, 1 M
documents in total generated on the device, in two node shapes: 1 shard with
the RCCL transport, and 2 shards with the in-process transport.

GLOBAL statistics: (a) 256 x tfidf_node_search(k = 0), (b) one
tfidf_node_search_batch_all.  SHARD statistics: (a) 256 x
tfidf_node_search_names (one call each, into buffers that always suffice),
(b) one tfidf_node_search_names_batch + tfidf_node_last_names_batch.

(a) runs on the library given with --lib (the parent commit's build, the
yardstick), (b) on this tree's build, both loaded into this process, each with
its own node over the same device-resident corpus.  The two alternate round by
round: warm-up rounds, then --runs timed rounds; wall time of the C calls alone
(ctypes, preallocated arrays), reported per query as median and [min, max] over
the rounds, with the hit (name) totals of both.  One JSON line per node shape
and statistics mode, also written under --out-dir.

RCCL with more than one rank is not measured here (one device).
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


def load_lib(path):
    """A libtfidf.so with the signatures it exports (another build may lack the newest)."""
    lib = C.CDLL(path)
    for name, (res, args) in L.SIGNATURES.items():
        if hasattr(lib, name):
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
    return lib


def check(lib, rc):
    if rc:
        raise RuntimeError("libtfidf error %d: %s" % (rc, lib.tfidf_last_error().decode(errors="replace")))


def build_node(lib, devices, mode, corpora):
    cfg = L.Config()
    check(lib, lib.tfidf_config_init(C.byref(cfg)))
    cfg.stats_mode = mode
    dev = (C.c_int32 * len(devices))(*devices)
    h = C.c_void_p()
    check(lib, lib.tfidf_node_create_devices(C.byref(cfg), dev, len(devices), 0, C.byref(h)))
    for g, dc in enumerate(corpora):
        ix = C.c_void_p()
        check(lib, lib.tfidf_node_shard(h, g, C.byref(ix), None))
        check(lib, lib.tfidf_add_docs_device(ix, dc.d_text, dc.d_offsets, dc.n_docs, dc.total_bytes))
    check(lib, lib.tfidf_node_commit(h))
    return h


def spread_us(ms, nq):
    xs = [x * 1e3 / nq for x in ms]
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def measure(args, base, new, devices, mode, corpora, qs):
    nq, nd = len(qs), sum(dc.n_docs for dc in corpora)
    offs = np.zeros(nq + 1, np.uint64)
    offs[1:] = np.cumsum([len(q) for q in qs], dtype=np.uint64)
    blob = b"".join(qs)
    hb, hn = build_node(base, devices, mode, corpora), build_node(new, devices, mode, corpora)
    n, nb = C.c_uint64(), C.c_uint64()
    wall_a, wall_b, wall_b_search, tot_a, tot_b = [], [], [], 0, 0
    if mode == L.STATS_GLOBAL:
        docs = np.empty(nd, np.uint64)
        scores = np.empty(nd, np.float32)
        pd, ps = L.ptr(docs, C.c_uint64), L.ptr(scores, C.c_float)
        ho = np.zeros(nq + 1, np.uint64)
        bd, bs = np.empty(1, np.uint64), np.empty(1, np.float32)
        for r in range(args.warmup + args.runs):
            tot_a = 0
            t0 = time.perf_counter()
            for q in qs:
                check(base, base.tfidf_node_search(hb, q, len(q), 0, pd, ps, nd, C.byref(n)))
                tot_a += n.value
            t1 = time.perf_counter()
            if len(bd) < tot_a:
                bd, bs = np.empty(tot_a, np.uint64), np.empty(tot_a, np.float32)
            t2 = time.perf_counter()
            check(new, new.tfidf_node_search_batch_all(hn, blob, L.ptr(offs, C.c_uint64), nq, L.ptr(bd, C.c_uint64),
                                                       L.ptr(bs, C.c_float), len(bd), L.ptr(ho, C.c_uint64), C.byref(n)))
            t3 = time.perf_counter()
            tot_b = n.value
            if r >= args.warmup:
                wall_a.append((t1 - t0) * 1e3)
                wall_b.append((t3 - t2) * 1e3)
        # the last single search's hits are still in docs / scores: the batch's last query must equal them
        last = slice(int(ho[nq - 1]), int(ho[nq]))
        m = last.stop - last.start
        same_last = bool((bd[last] == docs[:m]).all() and (bs[last] == scores[:m]).all())
        calls = ("tfidf_node_search(k=0)", "tfidf_node_search_batch_all")
    else:
        cap_b = 16 * nd                                        # decimal ordinals: at most 7 bytes a name
        buf = C.create_string_buffer(cap_b)
        no = np.zeros(nd + 1, np.uint64)
        sc = np.zeros(nd, np.float64)
        qo = np.zeros(nq + 1, np.uint64)
        bbuf, bo, bsc = C.create_string_buffer(1), np.zeros(1, np.uint64), np.zeros(1, np.float64)
        for r in range(args.warmup + args.runs):
            tot_a = 0
            t0 = time.perf_counter()
            for q in qs:
                check(base, base.tfidf_node_search_names(hb, q, len(q), buf, cap_b, L.ptr(no, C.c_uint64),
                                                         L.ptr(sc, C.c_double), nd, C.byref(n), C.byref(nb)))
                tot_a += n.value
            t1 = time.perf_counter()
            t2 = time.perf_counter()
            check(new, new.tfidf_node_search_names_batch(hn, blob, L.ptr(offs, C.c_uint64), nq, C.byref(n), C.byref(nb)))
            t_mid = time.perf_counter()
            if len(bsc) < n.value or len(bbuf) < nb.value:
                bbuf = C.create_string_buffer(max(nb.value, 1))
                bo, bsc = np.zeros(n.value + 1, np.uint64), np.zeros(max(n.value, 1), np.float64)
            check(new, new.tfidf_node_last_names_batch(hn, bbuf, len(bbuf), L.ptr(bo, C.c_uint64), L.ptr(bsc, C.c_double),
                                                       len(bsc), L.ptr(qo, C.c_uint64), C.byref(n), C.byref(nb)))
            t3 = time.perf_counter()
            tot_b = n.value
            if r >= args.warmup:
                wall_a.append((t1 - t0) * 1e3)
                wall_b.append((t3 - t2) * 1e3)
                wall_b_search.append((t_mid - t2) * 1e3)
        m = int(qo[nq] - qo[nq - 1])
        same_last = bool((bsc[int(qo[nq - 1]):int(qo[nq])] == sc[:m]).all())
        calls = ("tfidf_node_search_names", "tfidf_node_search_names_batch + tfidf_node_last_names_batch")
    base.tfidf_node_destroy(hb)
    new.tfidf_node_destroy(hn)
    a, b = spread_us(wall_a, nq), spread_us(wall_b, nq)
    extra = {"search_call_alone_wall_us_per_query": spread_us(wall_b_search, nq)} if wall_b_search else {}
    return {"label": args.label, "mode": "GLOBAL" if mode == L.STATS_GLOBAL else "SHARD", "shards": len(devices),
            "transport": "rccl" if len(devices) == 1 else "inproc", "docs": nd, "queries": nq,
            "warmup": args.warmup, "runs": args.runs,
            "loop": {"call": calls[0], "lib": os.path.relpath(args.lib, REPO), "total": tot_a, "wall_us_per_query": a},
            "batch": {"call": calls[1], "lib": os.path.relpath(L.LIB_PATH, REPO), "total": tot_b,
                      "wall_us_per_query": b, **extra},
            "totals_equal": bool(tot_a == tot_b), "last_query_equal": same_last,
            "wall_ratio_loop_over_batch": a["median"] / b["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the parent commit's libtfidf.so: the loop (a) runs on it")
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--label", default="")
    ap.add_argument("--modes", default="global,shard", help="statistics modes to measure")
    ap.add_argument("--host-timing", action="store_true",
                    help="the SHARD batch prints its stages' wall times to stderr (TFIDF_HOST_TIMING)")
    ap.add_argument("--out-dir", default=None, help="also write each JSON line to <out-dir>/<mode>_<shards>shard.json")
    args = ap.parse_args()
    args.lib = os.path.abspath(args.lib)
    if args.host_timing:
        os.environ["TFIDF_DEBUG"] = "1"
        os.environ["TFIDF_HOST_TIMING"] = "1"
    new = L.load()                                            # the corpus generator runs on this build too
    base = load_lib(args.lib)
    qs = synth.queries(args.queries)                          # 3 terms, ranks in [100, 10 000)
    for shards in (1, 2):
        corpora, at = [], 0
        for g in range(shards):
            nd = (g + 1) * args.docs // shards - g * args.docs // shards
            corpora.append(synth.DeviceCorpus(nd, doc_base=at))
            at += nd
        for mode in [m for name, m in (("global", L.STATS_GLOBAL), ("shard", L.STATS_SHARD))
                     if name in args.modes.split(",")]:
            res = measure(args, base, new, [0] * shards, mode, corpora, qs)
            line = json.dumps(res)
            print(line, flush=True)
            if args.out_dir:
                os.makedirs(args.out_dir, exist_ok=True)
                with open(os.path.join(args.out_dir, "%s_%dshard.json" % (res["mode"].lower(), shards)), "w") as f:
                    f.write(line + "\n")
        for dc in corpora:
            dc.free()


if __name__ == "__main__":
    main()
