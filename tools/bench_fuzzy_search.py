#!/usr/bin/env python3
"""Fuzzy search (tfidf_reader_search_fuzzy_batch) beside the term lookup it
shares its dictionary scans with (tfidf_reader_fuzzy_terms_batch, max_out 10)
and the expansion alone (tfidf_reader_fuzzy_expand_batch: the scans, the sort
and the device selection, no scoring).

Shapes: the vocabulary of the cfg-2 corpus (--docs documents x U[400, 600]
tokens, V = 100 k, block-major) and of the cfg-5 shape (--docs5 documents x
U[48, 80] tokens, V = 5 M, term-major).  Per shape and max_edits in {1, 2}:
1, 64 and 1 024 input terms (bench_fuzzy.misspelt: vocabulary words with one
letter changed or two letters swapped, fixed seed), max_expansions 50.  Then
the case the selection kernel exists for: one short term (the 4-letter word of
rank 0) at 2 edits, whose boost groups hold thousands of candidates.  Per case,
median and [min, max] over --runs timed calls after --warmup:
  search_ms   ms_device of the search: scans, sort, selection and all-hits scoring
  expand_ms   ms_device of the expansion alone
  lookup_ms   ms_device of the term lookup on the same terms
  wall_ms     host clock around the search
and the candidates (n_within summed), the expansion sizes, the hits and the
chunks of the scan.  --short-only runs the short-term expansion alone (for a
kernel trace of k_fzs_select).  One JSON file per shape under --out-dir, one
line per case on stdout."""
import argparse
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
from tfidf_amd import synth  # noqa: E402
from tfidf_amd.engine import ShardIndex  # noqa: E402
from bench_fuzzy import misspelt, spread  # noqa: E402

E = 50


def timed(fn, ms_index, warmup, runs):
    dev, wall, out = [], [], None
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        if r >= warmup:
            dev.append(out[ms_index])
            wall.append((t1 - t0) * 1e3)
    return out, spread(dev), spread(wall)


def case(rd, g, terms, max_edits, args, label):
    runs = args.runs
    cap = len(rd.search_fuzzy_batch_arrays(terms, max_edits, 0, E)[0])      # sized once: no timed call runs twice
    hits, search_ms, wall_ms = timed(lambda: rd.search_fuzzy_batch_arrays(terms, max_edits, 0, E, cap), 4,
                                     args.warmup, runs)
    chunks = g.last_fuzzy_chunks()
    exp, expand_ms, _ = timed(lambda: rd.fuzzy_expand_batch_arrays(terms, max_edits, 0, E), 7, args.warmup, runs)
    _, lookup_ms, _ = timed(lambda: rd.fuzzy_terms_batch_arrays(terms, max_edits, 0, 10), 6, args.warmup, runs)
    c = {"case": label, "max_edits": max_edits, "terms": len(terms), "max_expansions": E,
         "candidates": int(exp[1].sum()), "expanded": int(hits[3].sum()), "hits": int(len(hits[0])),
         "scan_chunks": chunks[0], "cand_chunks": chunks[1], "search_ms": search_ms, "expand_ms": expand_ms,
         "lookup_ms": lookup_ms, "wall_ms": wall_ms}
    c["selection_and_scoring_ms"] = search_ms["median"] - lookup_ms["median"]
    return c


def shape(name, docs, V, len_min, len_max, cap, inversion, args):
    corpus = synth.DeviceCorpus(docs, V=V, len_min=len_min, len_max=len_max)
    g = ShardIndex(vocab_capacity_log2=cap, inversion=inversion)
    g.add_documents_device(corpus.d_text, corpus.d_offsets, docs, corpus.total_bytes)
    g.commit()
    st = g.stats()
    cases = []
    short = [synth.word(0)]
    with g.reader() as rd:
        if args.short_only:
            for _ in range(args.warmup + args.runs):
                out = rd.fuzzy_expand_batch_arrays(short, 2, 0, E)
            print("%s short term %r: %d candidates, expand %.3f ms" % (name, short[0], int(out[1].sum()), out[7]))
        else:
            todo = [(e, misspelt(n, V), "misspelt") for e in (1, 2) for n in (1, 64, 1024)] + [(2, short, "short")]
            for max_edits, terms, label in todo:
                c = case(rd, g, terms, max_edits, args, label)
                cases.append(c)
                print("%s %-8s e=%d terms=%4d: search %.3f ms [%.3f, %.3f]  expand %.3f  lookup %.3f  wall %.3f  "
                      "cands %d  expanded %d  hits %d" % (name, label, max_edits, len(terms), c["search_ms"]["median"],
                                                         c["search_ms"]["min"], c["search_ms"]["max"],
                                                         c["expand_ms"]["median"], c["lookup_ms"]["median"],
                                                         c["wall_ms"]["median"], c["candidates"], c["expanded"],
                                                         c["hits"]), flush=True)
    res = {"shape": name, "docs": docs, "V": V, "tokens": [len_min, len_max], "vocab_capacity_log2": cap,
           "term_major": int(st["term_major"]), "num_terms": int(st["num_terms"]), "runs": args.runs,
           "warmup": args.warmup, "cases": cases}
    g.close()
    corpus.free()
    if not args.short_only:
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, name + ".json"), "w") as f:
            json.dump(res, f, indent=1)
    return res


def main():
    from bench import default_cap
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--docs", type=int, default=1_000_000, help="documents of the cfg-2 corpus (0 = skip)")
    ap.add_argument("--docs5", type=int, default=6_250_000, help="documents of the cfg-5 shape (0 = skip)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--short-only", action="store_true", help="only the short-term expansion (for a kernel trace)")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "fuzzy_search"))
    args = ap.parse_args()
    L.load()
    if args.docs:
        shape("cfg2", args.docs, 100_000, 400, 600, default_cap(100_000), L.INVERSION_AUTO, args)
    if args.docs5:
        shape("cfg5-shape", args.docs5, 5_000_000, 48, 80, default_cap(5_000_000), L.INVERSION_TERM, args)


if __name__ == "__main__":
    main()
