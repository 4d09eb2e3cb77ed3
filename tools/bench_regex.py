#!/usr/bin/env python3
"""Regular-expression search (tfidf_reader_regex_terms_batch,
tfidf_reader_search_regex_batch) against the wildcard calls on the patterns
both can say, on the same index and the same build, and alone on patterns only
a regular expression can say.

Shapes: the cfg-2 corpus (--docs documents x U[400, 600] tokens, V = 100 k,
block-major) and the cfg-5 shape (--docs5 documents x U[48, 80] tokens, V =
5 M, term-major), as tools/bench_wildcard.py builds them.  Families (letters
from vocabulary words of ranks drawn from a fixed seed):
  prefix    inter.*      / inter*      (three letters)
  suffix    .*ion        / *ion        (three letters)
  stars     a.*b.*c      / a*b*c
  dots      a....*       / a???*
  dots5     .....        / ?????
  only the regex: (abc|xyz)[a-z]{2,}   [a-m]+   .*[aeiou]{2}.*   ~(.*a.*)&.{4,6}
each as a batch of 1 and 64 patterns.  Per case, median and [min, max] over
--runs timed calls after --warmup of ms_device (HIP events on the call's
stream):
  scan_ms   the terms call with max_out 1: the counting scan, the filling scan,
            the sort and the selection (the scans dominate)
  docs_ms   the document call: the same plus the posting union
for the regex form and, where there is one, for the wildcard twin, with the
matching terms, the hits, the scans, the staged table bytes and whether the two
forms returned equal arrays.  One JSON file per shape under --out-dir, one line
per case on stdout."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tf-idf-distributed-system_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from tfidf_amd import _lib as L  # noqa: E402
from tfidf_amd import engine as E  # noqa: E402
from tfidf_amd import synth  # noqa: E402
from tfidf_amd.engine import ShardIndex  # noqa: E402

from bench_fuzzy import spread  # noqa: E402

TWINS = ("prefix", "suffix", "stars", "dots", "dots5")
ONLY = ("alt_class", "class_plus", "inner_class", "compl_and")


def patterns(kind, n, V, seed=20261020):
    """n (regex, wildcard twin or None) pairs of a family"""
    out = []
    s2 = synth.mix64(seed)
    for i in range(n):
        w = synth.word(synth.mix64(s2 ^ i) % V)
        w = (w + b"aaa")[:max(len(w), 3)]
        v = synth.word(synth.mix64(s2 ^ (i + 7919)) % V)
        v = (v + b"eee")[:max(len(v), 3)]
        a, b, c = w[:1], w[1:2], w[-1:]
        out.append({
            "prefix": (w[:3] + b".*", w[:3] + b"*"),
            "suffix": (b".*" + w[-3:], b"*" + w[-3:]),
            "stars": (a + b".*" + b + b".*" + c, a + b"*" + b + b"*" + c),
            "dots": (a + b"....*", a + b"???*"),
            "dots5": (b".....", b"?????"),
            "alt_class": (b"(" + w[:3] + b"|" + v[:3] + b")[a-z]{2,}", None),
            "class_plus": (b"[" + a + b"-" + bytes([min(a[0] + 12, 122)]) + b"]+", None),
            "inner_class": (b".*[aeiou]{2}.*" + c, None),
            "compl_and": (b"~(.*" + a + b".*)&.{4,6}", None),
        }[kind])
    return out


def timed(fn, args, ms_of):
    ms, out = [], None
    for r in range(args.warmup + args.runs):
        out = fn()
        if r >= args.warmup:
            ms.append(ms_of(out))
    return spread(ms), out


def shape(name, docs, V, len_min, len_max, cap, inversion, args):
    corpus = synth.DeviceCorpus(docs, V=V, len_min=len_min, len_max=len_max)
    g = ShardIndex(vocab_capacity_log2=cap, inversion=inversion)
    g.add_documents_device(corpus.d_text, corpus.d_offsets, docs, corpus.total_bytes)
    g.commit()
    st = g.stats()
    lib = L.load()
    cases = []
    with g.reader() as rd:
        for kind in TWINS + ONLY:
            for n in (1, 64):
                pairs = patterns(kind, n, V)
                rx = [p for p, _ in pairs]
                wc = [q for _, q in pairs] if pairs[0][1] is not None else None
                docs1 = rd.search_regex_batch_arrays(rx[:1])[0]
                if len(docs1) * n > args.max_hits:
                    cases.append({"kind": kind, "patterns": n, "unmeasured": "more than %d hits" % args.max_hits})
                    print("%s %s n=%d: unmeasured (hit bound)" % (name, kind, n), flush=True)
                    continue
                c = {"kind": kind, "patterns": n, "first_regex": rx[0].decode()}
                c["regex_scan_ms"], rt = timed(lambda: E._wildcard_terms_arrays(lib.tfidf_reader_regex_terms_batch, rd._h,
                                                                                rx, 1), args, lambda o: o[5])
                c["regex_docs_ms"], rdoc = timed(lambda: rd.search_regex_batch_arrays(rx), args, lambda o: o[3])
                stats = g.last_regex_stats()
                c.update({"matched_terms": int(rdoc[2].sum()), "hits": int(len(rdoc[0])), "scan_chunks": stats[0],
                          "union_chunks": stats[2], "table_bytes": stats[3]})
                line = "regex scan %.3f docs %.3f" % (c["regex_scan_ms"]["median"], c["regex_docs_ms"]["median"])
                if wc is not None:
                    c["first_wildcard"] = wc[0].decode()
                    c["wildcard_scan_ms"], wt = timed(lambda: E._wildcard_terms_arrays(
                        lib.tfidf_reader_wildcard_terms_batch, rd._h, wc, 1), args, lambda o: o[5])
                    c["wildcard_docs_ms"], wdoc = timed(lambda: rd.search_wildcard_batch_arrays(wc), args, lambda o: o[3])
                    c["equal_arrays"] = bool(all(np.array_equal(x, y) for x, y in zip(rdoc[:3], wdoc[:3])) and
                                             all(np.array_equal(x, y) for x, y in zip(rt[:3], wt[:3])) and rt[3] == wt[3])
                    c["regex_over_wildcard_scan"] = c["regex_scan_ms"]["median"] / c["wildcard_scan_ms"]["median"]
                    c["regex_over_wildcard_docs"] = c["regex_docs_ms"]["median"] / c["wildcard_docs_ms"]["median"]
                    line += "  wildcard scan %.3f docs %.3f  equal=%s" % (c["wildcard_scan_ms"]["median"],
                                                                          c["wildcard_docs_ms"]["median"], c["equal_arrays"])
                cases.append(c)
                print("%s %-11s n=%3d: %s  terms %d  hits %d  tables %d B" % (name, kind, n, line, c["matched_terms"],
                                                                             c["hits"], c["table_bytes"]), flush=True)
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
    ap.add_argument("--max-hits", type=int, default=300_000_000, help="hits of a batch held on the host at most")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "regex"))
    args = ap.parse_args()
    L.load()
    if args.docs:
        shape("cfg2", args.docs, 100_000, 400, 600, default_cap(100_000), L.INVERSION_AUTO, args)
    if args.docs5:
        shape("cfg5-shape", args.docs5, 5_000_000, 48, 80, default_cap(5_000_000), L.INVERSION_TERM, args)


if __name__ == "__main__":
    main()
