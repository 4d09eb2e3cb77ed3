#!/usr/bin/env python3
"""Compound queries (tfidf_reader_search_compound_batch) beside today's way of
answering them: one batch call per query kind, the hit lists brought to the
host, and the Boolean combination, the score and the order done in numpy.

Corpus: the cfg-2 synthetic shard (--docs documents x U[400, 600] tokens, V =
100 k, block-major).  A mixed batch of --queries compound queries in three
shapes, by turns:
  text+phrase    MUST word, SHOULD word, SHOULD "word word"
  text#wildcard  SHOULD word, SHOULD word, FILTER abc* (26 words)
  text-fuzzy     MUST word, MUST_NOT misspelt~1
Words are of ranks uniform in [2 000, 20 000) (rows of a few thousand
documents), the phrase words of ranks in [300, 1 500): a pair's candidate rows
are a few thousand documents (the phrase scan reads every candidate's text, so
a pair of the most frequent words would scan most of the corpus per phrase).
Each shape is also timed alone.  Per case, median and [min, max] over --runs
timed calls after --warmup:
  wall_ms      host clock around the call (end to end)
  device_ms    the call's device time (ms_device: its clause routes and the combine pass)
  combine_ms   the combine pass's own device time (tfidf_last_compound_ms)
and for the baseline
  wall_ms      host clock around the separate calls and the numpy combine
  calls_ms     ... the calls alone
  numpy_ms     ... the combine alone
  device_ms    the routes' device times, summed
The two ways must agree bit for bit (asserted).  --baseline-only runs the
separate calls and the numpy combine alone, with --lib naming the library to
load: a library built from the commit before the compound call, for the
"before" numbers.  One JSON file under --out-dir, one line per case on stdout."""
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
from bench_fuzzy import misspelt, spread  # noqa: E402

SHOULD, MUST, MUST_NOT, FILTER = 0, 1, 2, 3
TEXT, PHRASE, WILDCARD, REGEX, FUZZY = 0, 1, 2, 3, 4
SHAPES = ("text+phrase", "text#wildcard", "text-fuzzy")


def ranks(n, lo, hi, seed):
    s2 = synth.mix64(seed)
    return [lo + synth.mix64(s2 ^ i) % (hi - lo) for i in range(n)]


def make_queries(n, V, only=None):
    """n queries, the three shapes by turns (or one shape only)."""
    w = [synth.word(r) for r in ranks(4 * n, 2000, 20000, 11)]
    pw = [synth.word(r) for r in ranks(2 * n, 300, 1500, 12)]
    fz = misspelt(n, V)
    out = []
    for i in range(n):
        shape = only if only is not None else i % 3
        a, b = w[4 * i], w[4 * i + 1]
        if shape == 0:
            out.append([E.must(E.text(a)), E.should(E.text(b)), E.should(E.phrase(pw[2 * i] + b" " + pw[2 * i + 1], 0))])
        elif shape == 1:
            out.append([E.should(E.text(a)), E.should(E.text(b)), E.filter_(E.wildcard(w[4 * i + 2][:3] + b"*"))])
        else:
            out.append([E.must(E.text(a)), E.must_not(E.fuzzy(fz[i], 1, 0, 50))])
    return out


# ---------------------------------------------------------------------------
# today's way

def route_rows(rd, g, queries):
    """One batch call per kind -> ({clause: (docs, scores or None)}, device ms)."""
    flat = sorted({c[1:] for q in queries for c in q})
    rows, ms = {}, 0.0
    by = {k: [c for c in flat if c[0] == k] for k in (TEXT, PHRASE, WILDCARD, FUZZY)}
    if by[TEXT]:
        d, s, o = rd.search_batch_all_arrays([c[1] for c in by[TEXT]])
        ms += max(g.last_search_ms()[1], 0.0)
        for i, c in enumerate(by[TEXT]):
            rows[c] = (d[int(o[i]):int(o[i + 1])], s[int(o[i]):int(o[i + 1])])
    if by[PHRASE]:
        d, s, _, o = rd.search_phrase_slop_batch_arrays([c[1] for c in by[PHRASE]], [c[2] for c in by[PHRASE]])
        ms += max(g.last_search_ms()[1], 0.0)
        for i, c in enumerate(by[PHRASE]):
            rows[c] = (d[int(o[i]):int(o[i + 1])], s[int(o[i]):int(o[i + 1])])
    if by[WILDCARD]:
        d, o, _, m = rd.search_wildcard_batch_arrays([c[1] for c in by[WILDCARD]])
        ms += m
        for i, c in enumerate(by[WILDCARD]):
            rows[c] = (d[int(o[i]):int(o[i + 1])], None)
    groups = {}
    for c in by[FUZZY]:
        groups.setdefault(c[2:], []).append(c)
    for (e, p, x), cs in groups.items():
        d, s, o, _, m = rd.search_fuzzy_batch_arrays([c[1] for c in cs], e, p, x)
        ms += m
        for i, c in enumerate(cs):
            rows[c] = (d[int(o[i]):int(o[i + 1])], s[int(o[i]):int(o[i + 1])])
    return rows, ms


def numpy_combine(query, rows):
    """The rule of include/tfidf.h on host arrays -> (docs uint32[], scores float32[])."""
    req = [c for c in query if c[0] in (MUST, FILTER)]
    opt = [c for c in query if c[0] == SHOULD]
    if not req and not opt:
        return np.empty(0, np.uint32), np.empty(0, np.float32)
    if req:
        cand = None
        for c in req:
            d = rows[c[1:]][0]
            cand = np.unique(d) if cand is None else np.intersect1d(cand, d, assume_unique=False)
    else:
        cand = np.unique(np.concatenate([rows[c[1:]][0] for c in opt]))
    for c in query:
        if c[0] == MUST_NOT and len(cand):
            cand = cand[~np.isin(cand, rows[c[1:]][0])]
    n = len(cand)
    must, should = np.zeros(n, np.float64), np.zeros(n, np.float64)
    has_should = np.zeros(n, bool)
    for c in query:                                       # clause order
        if c[0] not in (MUST, SHOULD) or n == 0:
            continue
        d, s = rows[c[1:]]
        if len(d) == 0:
            continue
        order = np.argsort(d, kind="stable")
        ds = d[order]
        ss = np.ones(len(d), np.float32) if s is None else s[order]
        at = np.searchsorted(ds, cand)
        at[at >= len(ds)] = 0
        held = ds[at] == cand if len(ds) else np.zeros(n, bool)
        if c[0] == MUST:
            must += ss[at].astype(np.float64)             # every candidate is in a MUST row
        else:
            should[held] += ss[at][held].astype(np.float64)
            has_should |= held
    has_must = any(c[0] == MUST for c in query)
    m32, s32 = must.astype(np.float32), should.astype(np.float32)
    if has_must:
        score = np.where(has_should, m32 + s32, m32)
    else:
        score = np.where(has_should, s32, np.float32(0.0))
    score = score.astype(np.float32)
    order = np.lexsort((cand, -score.view(np.uint32).astype(np.int64)))
    return cand[order].astype(np.uint32), score[order]


def baseline(rd, g, queries):
    t0 = time.perf_counter()
    rows, ms = route_rows(rd, g, queries)
    t1 = time.perf_counter()
    out = [numpy_combine(q, rows) for q in queries]
    t2 = time.perf_counter()
    return out, ms, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def timed_baseline(rd, g, queries, args):
    dev, calls, comb, wall, out = [], [], [], [], None
    for r in range(args.warmup + args.runs):
        out, ms, c_ms, n_ms = baseline(rd, g, queries)
        if r >= args.warmup:
            dev.append(ms)
            calls.append(c_ms)
            comb.append(n_ms)
            wall.append(c_ms + n_ms)
    return out, {"wall_ms": spread(wall), "calls_ms": spread(calls), "numpy_ms": spread(comb), "device_ms": spread(dev)}


def timed_compound(rd, g, queries, args):
    cap = len(rd.search_compound_batch_arrays(queries)[0])               # sized once: no timed call runs twice
    dev, comb, wall, out = [], [], [], None
    for r in range(args.warmup + args.runs):
        t0 = time.perf_counter()
        out = rd.search_compound_batch_arrays(queries, cap)
        t1 = time.perf_counter()
        if r >= args.warmup:
            dev.append(out[3])
            comb.append(g.last_compound_stats()[3])
            wall.append((t1 - t0) * 1e3)
    entries, chunks, pairs, _ = g.last_compound_stats()
    return out, {"wall_ms": spread(wall), "device_ms": spread(dev), "combine_ms": spread(comb), "row_entries": entries,
                 "chunks": chunks, "pairs": pairs}


def main():
    from bench import default_cap
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--lib", default=None, help="libtfidf.so to load instead of the tree's")
    ap.add_argument("--name", default=None, help="file name under --out-dir (default: compound / baseline)")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "compound"))
    args = ap.parse_args()
    if args.lib:
        L.LIB_PATH = os.path.abspath(args.lib)
        have = C.CDLL(L.LIB_PATH)
        for name in [n for n in L.SIGNATURES if "compound" in n and not hasattr(have, n)]:
            del L.SIGNATURES[name]                        # a library from before the compound call
    L.load()
    V = 100_000
    corpus = synth.DeviceCorpus(args.docs, V=V, len_min=400, len_max=600)
    g = E.ShardIndex(vocab_capacity_log2=default_cap(V))
    g.add_documents_device(corpus.d_text, corpus.d_offsets, args.docs, corpus.total_bytes)
    g.commit()
    print("index: %d documents committed" % args.docs, flush=True)
    cases = []
    with g.reader() as rd:
        for label, only in [("mixed", None)] + [(s, i) for i, s in enumerate(SHAPES)]:
            queries = make_queries(args.queries, V, only)
            base, b = timed_baseline(rd, g, queries, args)
            print("%-14s baseline timed: wall %.2f ms" % (label, b["wall_ms"]["median"]), flush=True)
            c = {"case": label, "queries": len(queries), "hits": int(sum(len(d) for d, _ in base)), "baseline": b}
            if not args.baseline_only:
                got, c["compound"] = timed_compound(rd, g, queries, args)
                d, s, o, _ = got
                o = o.tolist()
                for i, (bd, bs) in enumerate(base):      # bit for bit
                    assert d[o[i]:o[i + 1]].tobytes() == bd.tobytes(), (label, i)
                    assert s[o[i]:o[i + 1]].tobytes() == bs.tobytes(), (label, i)
                c["agree"] = True
            cases.append(c)
            line = "%-14s q=%d hits=%d  baseline wall %.2f ms (calls %.2f, numpy %.2f, device %.2f)" % (
                label, len(queries), c["hits"], b["wall_ms"]["median"], b["calls_ms"]["median"], b["numpy_ms"]["median"],
                b["device_ms"]["median"])
            if "compound" in c:
                k = c["compound"]
                line += "  compound wall %.2f ms [%.2f, %.2f] device %.2f combine %.3f entries %d chunks %d" % (
                    k["wall_ms"]["median"], k["wall_ms"]["min"], k["wall_ms"]["max"], k["device_ms"]["median"],
                    k["combine_ms"]["median"], k["row_entries"], k["chunks"])
            print(line, flush=True)
    res = {"docs": args.docs, "V": V, "tokens": [400, 600], "runs": args.runs, "warmup": args.warmup,
           "baseline_only": bool(args.baseline_only), "library": L.load().tfidf_version().decode(), "cases": cases}
    g.close()
    corpus.free()
    os.makedirs(args.out_dir, exist_ok=True)
    name = args.name or ("baseline" if args.baseline_only else "compound")
    with open(os.path.join(args.out_dir, name + ".json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
