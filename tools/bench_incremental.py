#!/usr/bin/env python3
"""Commit cost when documents arrive, the shape of real use (the reference
commits after every upload, Worker.java:136-139): bench.py's timed steps add
nothing, so they show the limiting case only.

Starts from the cfg-2 device corpus with --base documents committed twice (both
snapshots built), then
  one commit after adding --big documents, and
  --small-commits commits adding --small documents each,
and reports per commit the host wall time, the device phases
(tfidf_get_commit_timing) and what the commit tokenized
(tfidf_commit_tokenized_docs; null with a library that has no such call, which
tokenizes everything every time) and which blocks its inversion built
(tfidf_commit_inverted_blocks: first_block, n_blocks, remapped; null with a
library that has no such call, which inverts every block every time), and the host
side (tfidf_commit_host_profile: host times, stream synchronisations, the form and
bytes of each mirror; null with a library that has no such call).  Commits alternate between two snapshots, so
every new document is tokenized once for each of them: a commit that adds n
documents tokenizes about 2n (the n of the commit before, and its own).
TFIDF_DEBUG=1 TFIDF_FULL_COMMIT=1 gives the full-build numbers on the same library,
TFIDF_DEBUG=1 TFIDF_FULL_INVERSION=1 those of incremental tokenizing with every block inverted.
TFIDF_DEBUG=1 TFIDF_FULL_MIRROR=1 those with the host mirrors copied whole by every commit.
One JSON line on stdout; --out writes it to a file as well.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tf-idf-distributed-system_amd"))

from tfidf_amd import _lib as L  # noqa: E402
from tfidf_amd import synth  # noqa: E402
from tfidf_amd.engine import ShardIndex  # noqa: E402

PHASES = ("ms_tokenize", "ms_long", "ms_df", "ms_blockscan", "ms_colscan", "ms_scatter", "ms_total")


ACCESSORS = ("tfidf_commit_host_profile", "tfidf_commit_inverted_blocks", "tfidf_commit_tokenized_docs")   # newest first
HOST_MS = ("ms_wall", "ms_counters", "ms_enqueued", "ms_synced", "ms_published")


def load_library():
    """The accessors the library has (A/B against an older build: it may predate either)."""
    have = list(ACCESSORS)
    while True:
        try:
            L.load()
            return set(have)
        except AttributeError:
            if not have:
                raise
            L.SIGNATURES.pop(have.pop(0))


def commit(idx, have):
    t0 = time.perf_counter()
    idx.commit()
    wall = (time.perf_counter() - t0) * 1e3
    t = idx.commit_timing()
    tok = idx.commit_tokenized_docs() if "tfidf_commit_tokenized_docs" in have else None
    inv = idx.commit_inverted_blocks() if "tfidf_commit_inverted_blocks" in have else {}
    host = idx.commit_host_profile() if "tfidf_commit_host_profile" in have else None
    return {"wall_ms": wall, **{k: t[k] for k in PHASES}, "host": host,
            "tokenized_docs": tok and tok["docs"], "was_full": tok and tok["was_full"],
            "first_block": inv.get("first_block"), "n_blocks": inv.get("n_blocks"), "remapped": inv.get("remapped")}


def summary(rows):
    out = {k: float(np.median([r[k] for r in rows])) for k in ("wall_ms",) + PHASES}
    out["wall_ms_min_max"] = [float(min(r["wall_ms"] for r in rows)), float(max(r["wall_ms"] for r in rows))]
    out["tokenized_docs"] = [r["tokenized_docs"] for r in rows]
    for k in ("first_block", "n_blocks", "remapped"):
        out[k] = [r[k] for r in rows]
    # the host side (tfidf_commit_host_profile; null with a library that has no such call): medians of the
    # points and of the bytes mirrored, the synchronisation counts and how often each mirror took which form
    hosts = [r["host"] for r in rows]
    if all(hosts):
        h = {k: float(np.median([x[k] for x in hosts])) for k in HOST_MS}
        for k in ("bytes_dict", "bytes_df", "bytes_crank", "dict_delta_entries", "df_delta_entries"):
            h[k] = float(np.median([x[k] for x in hosts]))
        h["stream_syncs"] = sorted(set(x["stream_syncs"] for x in hosts))
        h["col_rank_runs"] = sorted(set(x["col_rank_runs"] for x in hosts))
        for m in ("mirror_dict", "mirror_df", "mirror_crank"):
            h[m] = {f: sum(x[m] == f for x in hosts) for f in ("none", "delta", "whole")}
        out["host"] = h
    else:
        out["host"] = None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", type=int, default=990_000)
    ap.add_argument("--big", type=int, default=10_000)
    ap.add_argument("--small", type=int, default=200)
    ap.add_argument("--small-commits", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--len-min", type=int, default=400)
    ap.add_argument("--len-max", type=int, default=600)
    ap.add_argument("--cap-log2", type=int, default=18)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    has_accessor = load_library()           # (the set of accessors the library has)

    def corpus(n, base):
        return synth.DeviceCorpus(n, V=args.vocab, len_min=args.len_min, len_max=args.len_max, doc_base=base)

    def add(idx, c):
        idx.add_documents_device(c.d_text, c.d_offsets, c.n_docs, c.total_bytes)
        c.free()

    idx = ShardIndex(vocab_capacity_log2=args.cap_log2)
    add(idx, corpus(args.base, 0))
    first = [commit(idx, has_accessor) for _ in range(2)]
    add(idx, corpus(args.big, args.base))
    big = commit(idx, has_accessor)
    small, at = [], args.base + args.big
    for _ in range(args.small_commits):
        add(idx, corpus(args.small, at))
        at += args.small
        small.append(commit(idx, has_accessor))
    s = idx.stats()
    res = {"bench": "incremental_commit", "library_has_accessor": "tfidf_commit_tokenized_docs" in has_accessor,
           "library_reports_inverted_blocks": "tfidf_commit_inverted_blocks" in has_accessor,
           "library_reports_host_profile": "tfidf_commit_host_profile" in has_accessor,
           "full_mirror_forced": bool(os.environ.get("TFIDF_DEBUG")) and os.environ.get("TFIDF_FULL_MIRROR", "0") not in ("", "0"),
           "full_inversion_forced": bool(os.environ.get("TFIDF_DEBUG")) and os.environ.get("TFIDF_FULL_INVERSION", "0") not in ("", "0"),
           "full_commit_forced": bool(os.environ.get("TFIDF_DEBUG")) and os.environ.get("TFIDF_FULL_COMMIT", "0") not in ("", "0"),
           "config": {k: v for k, v in vars(args).items() if k != "out"}, "num_docs": s["num_docs"], "nnz": s["nnz"], "text_bytes": s["text_bytes"],
           "first_two_commits": first, "commit_after_big": big, "small_commits": summary(small),
           "note": "each new document is tokenized once per snapshot, so by two successive commits"}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    idx.close()


if __name__ == "__main__":
    main()
