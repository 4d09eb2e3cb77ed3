#!/usr/bin/env python3
"""Nested compound queries (tfidf_reader_search_nested_batch) on the benchmark
shard of bench_compound.py (same corpus, same words), in two cases.  Per case,
median and [min, max] over --runs timed calls after --warmup.

  flat-as-root   bench_compound's mixed batch, every query sent as a root group
                 through the nested call, beside the flat call on the same
                 library: the price of the general kernel.  The two must agree
                 byte for byte (asserted).
  nested         +(w w abc*)~2 +("w w" w~1) -(w w) per query: a conjunction of
                 two disjunctions, the first asking for two of its three
                 clauses, and a negated disjunction.  Beside it the only way to
                 answer it without the nested call: one flat compound batch that
                 holds, per query, the first group's three clauses as queries of
                 their own (the flat call has no minimumShouldMatch) and the
                 other two groups as one query each, and a numpy combine of the
                 five hit lists.  The two must agree bit for bit (asserted).

For the nested call: wall_ms, device_ms (ms_device), combine_ms
(tfidf_last_compound_ms) and its share of the device time; for the baseline
wall_ms, call_ms, numpy_ms, device_ms.  --baseline-only with --lib runs the
baseline alone on another library (one from before the nested call).  One JSON
file under --out-dir, one line per case on stdout."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tf-idf-distributed-system_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from tfidf_amd import _lib as L  # noqa: E402
from tfidf_amd import engine as E  # noqa: E402
from tfidf_amd import synth  # noqa: E402
from bench_compound import make_queries, ranks, timed_compound  # noqa: E402
from bench_fuzzy import misspelt, spread  # noqa: E402

SHOULD, MUST, MUST_NOT, FILTER = 0, 1, 2, 3


def nested_parts(n, V):
    """Per query the three groups' clause lists: (first, second, third)."""
    w = [synth.word(r) for r in ranks(5 * n, 2000, 20000, 21)]
    pw = [synth.word(r) for r in ranks(2 * n, 300, 1500, 22)]
    fz = misspelt(n, V)
    out = []
    for i in range(n):
        a, b, c, d, e = w[5 * i:5 * i + 5]
        out.append(([E.should(E.text(a)), E.should(E.text(b)), E.should(E.wildcard(c[:3] + b"*"))],
                    [E.should(E.phrase(pw[2 * i] + b" " + pw[2 * i + 1], 0)), E.should(E.fuzzy(fz[i], 1, 0, 50))],
                    [E.should(E.text(d)), E.should(E.text(e))]))
    return out


def nested_queries(parts):
    return [E.group([E.must(E.group(p1, 2)), E.must(E.group(p2)), E.must_not(E.group(p3))]) for p1, p2, p3 in parts]


def np_group(children, m):
    """The group rule on host arrays: children = [(occur, docs uint32[], scores float32[])] -> (docs, scores)."""
    req = [c for c in children if c[0] in (MUST, FILTER)]
    opt = [c for c in children if c[0] == SHOULD]
    need = max(m, 0 if req else 1)
    if need > len(opt):
        return np.empty(0, np.uint32), np.empty(0, np.float32)
    if req:
        cand = None
        for _, d, _ in req:
            cand = np.unique(d) if cand is None else np.intersect1d(cand, d)
    else:
        cand = np.unique(np.concatenate([d for _, d, _ in opt]))
    for o, d, _ in children:
        if o == MUST_NOT and len(cand):
            cand = cand[~np.isin(cand, d)]
    n = len(cand)
    must, should = np.zeros(n, np.float64), np.zeros(n, np.float64)
    count = np.zeros(n, np.int64)
    for o, d, s in children:                              # child order
        if o not in (MUST, SHOULD) or n == 0 or len(d) == 0:
            continue
        order = np.argsort(d, kind="stable")
        ds, ss = d[order], s[order]
        at = np.searchsorted(ds, cand)
        at[at >= len(ds)] = 0
        held = ds[at] == cand
        if o == MUST:
            must += ss[at].astype(np.float64)
        else:
            should[held] += ss[at][held].astype(np.float64)
            count += held
    keep = count >= need
    cand, must, should, count = cand[keep], must[keep], should[keep], count[keep]
    m32, s32 = must.astype(np.float32), should.astype(np.float32)
    if any(o == MUST for o, _, _ in children):
        score = np.where(count > 0, m32 + s32, m32)
    else:
        score = np.where(count > 0, s32, np.float32(0.0))
    score = score.astype(np.float32)
    order = np.lexsort((cand, -score.view(np.uint32).astype(np.int64)))
    return cand[order].astype(np.uint32), score[order]


def baseline(rd, parts, cap):
    flat = []
    for p1, p2, p3 in parts:
        flat += [[c] for c in p1] + [p2, p3]
    t0 = time.perf_counter()
    d, s, o, ms = rd.search_compound_batch_arrays(flat, cap)
    t1 = time.perf_counter()
    o = o.tolist()
    row = lambda i: (d[o[i]:o[i + 1]], s[o[i]:o[i + 1]])   # noqa: E731
    out = []
    for q in range(len(parts)):
        first = np_group([(SHOULD,) + row(5 * q + j) for j in range(3)], 2)
        out.append(np_group([(MUST,) + first, (MUST,) + row(5 * q + 3), (MUST_NOT,) + row(5 * q + 4)], 0))
    t2 = time.perf_counter()
    return out, ms, (t1 - t0) * 1e3, (t2 - t1) * 1e3, len(d)


def timed_baseline(rd, parts, args):
    cap = baseline(rd, parts, None)[4]
    dev, calls, comb, wall, out = [], [], [], [], None
    for r in range(args.warmup + args.runs):
        out, ms, c_ms, n_ms, _ = baseline(rd, parts, cap)
        if r >= args.warmup:
            dev.append(ms)
            calls.append(c_ms)
            comb.append(n_ms)
            wall.append(c_ms + n_ms)
    return out, {"wall_ms": spread(wall), "call_ms": spread(calls), "numpy_ms": spread(comb), "device_ms": spread(dev)}


def timed_nested(rd, g, queries, args):
    cap = len(rd.search_nested_batch_arrays(queries)[0])                 # sized once: no timed call runs twice
    dev, comb, share, wall, out = [], [], [], [], None
    for r in range(args.warmup + args.runs):
        t0 = time.perf_counter()
        out = rd.search_nested_batch_arrays(queries, cap)
        t1 = time.perf_counter()
        if r >= args.warmup:
            dev.append(out[3])
            comb.append(g.last_compound_stats()[3])
            share.append(comb[-1] / out[3] if out[3] > 0 else 0.0)
            wall.append((t1 - t0) * 1e3)
    entries, chunks, pairs, _ = g.last_compound_stats()
    return out, {"wall_ms": spread(wall), "device_ms": spread(dev), "combine_ms": spread(comb),
                 "combine_share": spread(share), "row_entries": entries, "chunks": chunks, "pairs": pairs}


def main():
    from bench import default_cap
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--lib", default=None, help="libtfidf.so to load instead of the tree's")
    ap.add_argument("--name", default=None, help="file name under --out-dir (default: nested / baseline)")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "compound_nested"))
    args = ap.parse_args()
    if args.lib:
        L.LIB_PATH = os.path.abspath(args.lib)
        have = C.CDLL(L.LIB_PATH)
        for name in [n for n in L.SIGNATURES if ("compound" in n or "nested" in n) and not hasattr(have, n)]:
            del L.SIGNATURES[name]                        # a library from before the call
    L.load()
    V = 100_000
    corpus = synth.DeviceCorpus(args.docs, V=V, len_min=400, len_max=600)
    g = E.ShardIndex(vocab_capacity_log2=default_cap(V))
    g.add_documents_device(corpus.d_text, corpus.d_offsets, args.docs, corpus.total_bytes)
    g.commit()
    print("index: %d documents committed" % args.docs, flush=True)
    cases = []
    with g.reader() as rd:
        if not args.baseline_only:
            queries = make_queries(args.queries, V)
            flat, f = timed_compound(rd, g, queries, args)
            nest, k = timed_nested(rd, g, queries, args)                  # a plain list is a root group with m = 0
            for a, b in zip(flat[:3], nest[:3]):
                assert a.tobytes() == b.tobytes()
            cases.append({"case": "flat-as-root", "queries": len(queries), "hits": int(len(flat[0])), "flat": f,
                          "nested": k, "agree": True})
            print("flat-as-root   q=%d hits=%d  flat wall %.2f ms [%.2f, %.2f] combine %.3f  nested wall %.2f ms "
                  "[%.2f, %.2f] combine %.3f [%.3f, %.3f]" % (
                      len(queries), len(flat[0]), f["wall_ms"]["median"], f["wall_ms"]["min"], f["wall_ms"]["max"],
                      f["combine_ms"]["median"], k["wall_ms"]["median"], k["wall_ms"]["min"], k["wall_ms"]["max"],
                      k["combine_ms"]["median"], k["combine_ms"]["min"], k["combine_ms"]["max"]), flush=True)
        parts = nested_parts(args.queries, V)
        base, b = timed_baseline(rd, parts, args)
        c = {"case": "nested", "queries": len(parts), "hits": int(sum(len(d) for d, _ in base)), "baseline": b}
        line = "nested         q=%d hits=%d  baseline wall %.2f ms [%.2f, %.2f] (call %.2f, numpy %.2f, device %.2f)" % (
            len(parts), c["hits"], b["wall_ms"]["median"], b["wall_ms"]["min"], b["wall_ms"]["max"],
            b["call_ms"]["median"], b["numpy_ms"]["median"], b["device_ms"]["median"])
        if not args.baseline_only:
            got, k = timed_nested(rd, g, nested_queries(parts), args)
            d, s, o, _ = got
            o = o.tolist()
            for i, (bd, bs) in enumerate(base):          # bit for bit
                assert d[o[i]:o[i + 1]].tobytes() == bd.tobytes(), i
                assert s[o[i]:o[i + 1]].tobytes() == bs.tobytes(), i
            c["nested"], c["agree"] = k, True
            line += "  nested wall %.2f ms [%.2f, %.2f] device %.2f combine %.3f (share %.3f) entries %d chunks %d" % (
                k["wall_ms"]["median"], k["wall_ms"]["min"], k["wall_ms"]["max"], k["device_ms"]["median"],
                k["combine_ms"]["median"], k["combine_share"]["median"], k["row_entries"], k["chunks"])
        cases.append(c)
        print(line, flush=True)
    res = {"docs": args.docs, "V": V, "tokens": [400, 600], "runs": args.runs, "warmup": args.warmup,
           "baseline_only": bool(args.baseline_only), "library": L.load().tfidf_version().decode(), "cases": cases}
    g.close()
    corpus.free()
    os.makedirs(args.out_dir, exist_ok=True)
    name = args.name or ("baseline" if args.baseline_only else "nested")
    with open(os.path.join(args.out_dir, name + ".json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
