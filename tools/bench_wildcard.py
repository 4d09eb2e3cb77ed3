#!/usr/bin/env python3
"""Wildcard search (tfidf_reader_search_wildcard_batch) against the route a
caller has without it: match the vocabulary's strings on the host with Python
``re``, OR the matching terms through search_batch_all in slices of at most
1 024 clauses (the scorer's clause limit) and union the slices' doc ids with
numpy.  The host route's export of the vocabulary is not counted, which
flatters it.

Shapes: the cfg-2 corpus (--docs documents x U[400, 600] tokens, V = 100 k,
block-major) and the cfg-5 shape (--docs5 documents x U[48, 80] tokens, V =
5 M, term-major).  Patterns: a one-letter prefix, a three-letter prefix, a
leading ``*`` (``*`` + a three-letter suffix) and ``*``, each as a batch of 1,
64 and 1 024 patterns (distinct letters cycled from a fixed seed; ``*`` is
repeated).  Per case, median and [min, max] over --runs timed calls after
--warmup:
  device_ms   ms_device of the call (HIP events on the call's stream)
  wall_ms     host clock around the call
  host_ms     the host route, run on at most --host-patterns patterns of the
              batch and --host-terms matching terms per pattern and scaled up
              (host_extrapolated says so); --host-patterns 0 skips it
and the matching terms, the hits, the chunks of the device call and whether
both routes agree on the hits where the host route ran in full.  One JSON file
per shape under --out-dir, one line per case on stdout."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tf-idf-distributed-system_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from tfidf_amd import _lib as L  # noqa: E402
from tfidf_amd import synth  # noqa: E402
from tfidf_amd.engine import ShardIndex  # noqa: E402

from bench_fuzzy import spread, vocab_strings  # noqa: E402

KINDS = ("prefix1", "prefix3", "leading", "star")


def patterns(kind, n, V, seed=20261020):
    """n patterns of a kind; the letters come from vocabulary words of ranks uniform in [0, V)."""
    out = []
    s2 = synth.mix64(seed)
    for i in range(n):
        w = synth.word(synth.mix64(s2 ^ i) % V)
        w = (w + b"aaa")[:max(len(w), 3)]
        out.append({"prefix1": w[:1] + b"*", "prefix3": w[:3] + b"*", "leading": b"*" + w[-3:], "star": b"*"}[kind])
    return out


def to_regex(p):
    return re.compile(b"".join(b".*" if c == 42 else b"." if c == 63 else re.escape(bytes([c])) for c in p), re.S)


def host_route(rd, vocab, pats, max_terms):
    """-> (ms, [hit arrays or None when the terms were cut], terms run, terms matched)"""
    t0 = time.perf_counter()
    hits, run, matched = [], 0, 0
    for p in pats:
        rx = to_regex(p)
        terms = [v for v in vocab if rx.fullmatch(v)]
        matched += len(terms)
        cut = terms[:max_terms]
        run += len(cut)
        qs = [b" ".join(cut[i:i + 1024]) for i in range(0, len(cut), 1024)]
        docs = [np.fromiter((d for d, _ in h), np.uint32) for h in rd.search_batch_all(qs)] if qs else []
        u = np.unique(np.concatenate(docs)) if docs else np.zeros(0, np.uint32)
        hits.append(u if len(cut) == len(terms) else None)
    return (time.perf_counter() - t0) * 1e3, hits, run, matched


def shape(name, docs, V, len_min, len_max, cap, inversion, args):
    corpus = synth.DeviceCorpus(docs, V=V, len_min=len_min, len_max=len_max)
    g = ShardIndex(vocab_capacity_log2=cap, inversion=inversion)
    g.add_documents_device(corpus.d_text, corpus.d_offsets, docs, corpus.total_bytes)
    g.commit()
    st = g.stats()
    vocab = vocab_strings(g) if args.host_patterns else []
    cases = []
    with g.reader() as rd:
        for kind in KINDS:
            for n in (1, 64, 1024):
                pats = patterns(kind, n, V)
                # the hits of a batch are held on the host: bound them (a case over the bound is named, not run)
                docs1, offs1, m1, _ = rd.search_wildcard_batch_arrays(pats[:1])
                if len(docs1) * n > args.max_hits:
                    cases.append({"kind": kind, "patterns": n, "unmeasured": "more than %d hits" % args.max_hits})
                    print("%s %s n=%d: unmeasured (hit bound)" % (name, kind, n), flush=True)
                    continue
                dev, wall, out = [], [], None
                for r in range(args.warmup + args.runs):
                    t0 = time.perf_counter()
                    out = rd.search_wildcard_batch_arrays(pats)
                    t1 = time.perf_counter()
                    if r >= args.warmup:
                        dev.append(out[3])
                        wall.append((t1 - t0) * 1e3)
                stats = g.last_wildcard_stats()
                c = {"kind": kind, "patterns": n, "first_pattern": pats[0].decode(), "matched_terms": int(out[2].sum()),
                     "hits": int(len(out[0])), "scan_chunks": stats[0], "union_chunks": stats[2],
                     "device_ms": spread(dev), "wall_ms": spread(wall)}
                if args.host_patterns:
                    nh = min(n, args.host_patterns)
                    h_ms, h_hits, run, matched = host_route(rd, vocab, pats[:nh], args.host_terms)
                    scale = (n / nh) * (matched / run if run else 1.0)
                    o = out[1].tolist()
                    agree = [bool(np.array_equal(h, out[0][o[i]:o[i + 1]])) for i, h in enumerate(h_hits) if h is not None]
                    c.update({"host_ms": h_ms * scale, "host_ms_run": h_ms, "host_patterns_run": nh,
                              "host_terms_run": run, "host_extrapolated": scale != 1.0,
                              "agree": all(agree) if agree else None,
                              "host_over_device": h_ms * scale / c["device_ms"]["median"]})
                cases.append(c)
                print("%s %-7s n=%4d: device %.3f ms [%.3f, %.3f]  wall %.3f ms  terms %d  hits %d  host %s"
                      % (name, kind, n, c["device_ms"]["median"], c["device_ms"]["min"], c["device_ms"]["max"],
                         c["wall_ms"]["median"], c["matched_terms"], c["hits"],
                         "%.1f ms%s agree=%s" % (c["host_ms"], "*" if c["host_extrapolated"] else "", c["agree"])
                         if "host_ms" in c else "-"), flush=True)
    res = {"shape": name, "docs": docs, "V": V, "tokens": [len_min, len_max], "vocab_capacity_log2": cap,
           "term_major": int(st["term_major"]), "num_terms": int(st["num_terms"]), "runs": args.runs,
           "warmup": args.warmup, "cases": cases}
    g.close()
    corpus.free()
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, name + ".json"), "w") as f:
        json.dump(res, f, indent=1)
    return res


def main():
    from bench import default_cap
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--docs", type=int, default=1_000_000, help="documents of the cfg-2 corpus (0 = skip)")
    ap.add_argument("--docs5", type=int, default=6_250_000, help="documents of the cfg-5 shape (0 = skip)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-patterns", type=int, default=1, help="patterns of a batch the host route runs (0 = none)")
    ap.add_argument("--host-terms", type=int, default=4096, help="matching terms per pattern the host route scores")
    ap.add_argument("--max-hits", type=int, default=300_000_000, help="hits of a batch held on the host at most")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "wildcard"))
    args = ap.parse_args()
    L.load()
    if args.docs:
        shape("cfg2", args.docs, 100_000, 400, 600, default_cap(100_000), L.INVERSION_AUTO, args)
    if args.docs5:
        shape("cfg5-shape", args.docs5, 5_000_000, 48, 80, default_cap(5_000_000), L.INVERSION_TERM, args)


if __name__ == "__main__":
    main()
