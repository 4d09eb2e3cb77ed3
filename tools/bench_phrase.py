#!/usr/bin/env python3
"""Exact phrase search (tfidf_reader_search_phrase_batch) against the only
route without it: tfidf_reader_search_batch_all of the conjunction of the
phrase's words, then per candidate tfidf_reader_doc_text, tfidf_analyze on the
host and a count of the occurrences (one call and one copy per document).

Phrases are 2 and 3 consecutive tokens drawn (fixed seed) from committed
documents read back with doc_text: every phrase has at least one hit.

Shapes:
  cfg2-phrase-N   N in {1, 64, 1024} phrases on the cfg-2 synthetic corpus (--docs documents)
  book-phrase-N   --book-phrases phrases on --books ~1 MB book-like documents
The host route runs on a seeded subset of the phrases (--host-phrases; the
JSON says how many), and both routes must give the same hits and frequencies
on that subset before anything is timed.  Per shape, median and [min, max]
over --runs timed rounds after --warmup (a round alternates the two routes):
  device.wall_ms    host clock around the batched call
  device.device_ms  HIP events around the whole call on its stream (tfidf_last_search_ms total)
  host.wall_ms      the host route over its subset; host.wall_ms_per_phrase
plus the candidates (phrase, document) scanned, their document bytes, bytes
scanned per device second and the row chunks of the call.  One JSON file per
shape under --out-dir, one line per shape on stdout.

--slop N times tfidf_reader_search_phrase_slop_batch with slop N for every
phrase instead (phrases that repeat a word are not drawn; N = 0 is the exact
rule through the sloppy call).  The host route stays the exact count: before
anything is timed its hits must be among the sloppy hits (all of them at N =
0).  The shapes and files are then named slopN_<shape>, and the JSON says
"slop": N.
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tf-idf-distributed-system_amd"))

from tfidf_amd import _lib as L  # noqa: E402
from tfidf_amd import synth  # noqa: E402
from tfidf_amd.engine import ShardIndex, analyze  # noqa: E402

SEED = 20261020


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def draw_phrases(rd, n, rng, distinct=False):
    """n phrases of 2 and 3 consecutive tokens of randomly chosen documents -> [(bytes, [terms])];
    distinct: none that repeats a token."""
    out = []
    while len(out) < n:
        toks = analyze(rd.doc_text(rng.randrange(rd.num_docs)))
        m = 2 + len(out) % 2
        if len(toks) < m:
            continue
        at = rng.randrange(len(toks) - m + 1)
        if distinct and len(set(toks[at:at + m])) < m:
            continue
        out.append((b" ".join(toks[at:at + m]), toks[at:at + m]))
    return out


def count(tokens, terms):
    m = len(terms)
    return sum(1 for p in range(len(tokens) - m + 1) if tokens[p:p + m] == terms)


def host_route(rd, phrases):
    """The route a user has without the call -> ([{doc: freq}], candidates, document bytes)."""
    queries = [b" AND ".join(dict.fromkeys(terms)) for _, terms in phrases]
    docs, _, offs = rd.search_batch_all_arrays(queries)
    o = offs.astype(np.int64)
    out, n_cand, n_bytes = [], 0, 0
    for i, (_, terms) in enumerate(phrases):
        hits = {}
        for d in docs[o[i]:o[i + 1]].tolist():
            text = rd.doc_text(d)
            n_bytes += len(text)
            f = count(analyze(text), terms)
            if f:
                hits[d] = f
        n_cand += int(o[i + 1] - o[i])
        out.append(hits)
    return out, n_cand, n_bytes


class RawPhrase:
    """tfidf_reader_search_phrase_batch (slop None) or tfidf_reader_search_phrase_slop_batch
    into buffers allocated once."""

    def __init__(self, rd, phrases, slop=None):
        self.rd, self.n_p = rd, len(phrases)
        self.slops = None if slop is None else np.full(self.n_p, slop, np.uint32)
        self.blob = b"".join(p for p, _ in phrases)
        self.offs = np.zeros(self.n_p + 1, np.uint64)
        self.offs[1:] = np.cumsum([len(p) for p, _ in phrases], dtype=np.uint64)
        self.hit_offs = np.zeros(self.n_p + 1, np.uint64)
        self.n = C.c_uint64()
        self.size(1)
        if self.call() == L.E_BUFFER:
            self.size(self.n.value)
            L.check(self.call())

    def size(self, cap):
        self.cap = cap
        self.docs, self.scores = np.empty(cap, np.uint32), np.empty(cap, np.float32)
        self.freqs = np.empty(cap, np.uint32 if self.slops is None else np.float32)

    def call(self):
        if self.slops is not None:
            rc = L.load().tfidf_reader_search_phrase_slop_batch(
                self.rd._h, self.blob, L.ptr(self.offs, C.c_uint64), L.ptr(self.slops, C.c_uint32), self.n_p,
                L.ptr(self.docs, C.c_uint32), L.ptr(self.scores, C.c_float), L.ptr(self.freqs, C.c_float), self.cap,
                L.ptr(self.hit_offs, C.c_uint64), C.byref(self.n))
            if rc not in (L.OK, L.E_BUFFER):
                L.check(rc)
            return rc
        rc = L.load().tfidf_reader_search_phrase_batch(
            self.rd._h, self.blob, L.ptr(self.offs, C.c_uint64), self.n_p, L.ptr(self.docs, C.c_uint32),
            L.ptr(self.scores, C.c_float), L.ptr(self.freqs, C.c_uint32), self.cap, L.ptr(self.hit_offs, C.c_uint64),
            C.byref(self.n))
        if rc not in (L.OK, L.E_BUFFER):
            L.check(rc)
        return rc

    def hits(self, i):
        a, z = int(self.hit_offs[i]), int(self.hit_offs[i + 1])
        return dict(zip(self.docs[a:z].tolist(), self.freqs[a:z].tolist()))


def shape(name, g, rd, lens, n_p, n_host, runs, warmup, extra, slop=None):
    rng = random.Random(SEED + n_p)
    phrases = draw_phrases(rd, n_p, rng, distinct=slop is not None)
    sub = sorted(rng.sample(range(n_p), min(n_host, n_p)))
    sub_phrases = [phrases[i] for i in sub]
    raw = RawPhrase(rd, phrases, slop)
    # the same hits and frequencies on the subset, before anything is timed
    want, host_cand, host_bytes = host_route(rd, sub_phrases)
    for i, w in zip(sub, want):
        if slop:
            assert set(w) <= set(raw.hits(i)) and w, (name, phrases[i][0])
        else:
            assert raw.hits(i) == w and w, (name, phrases[i][0])
    cand, row_chunks = g.last_phrase_stats()
    # document bytes of the candidates: the conjunctions' hits
    docs, _, _ = rd.search_batch_all_arrays([b" AND ".join(dict.fromkeys(t)) for _, t in phrases])
    assert len(docs) == cand
    nbytes = int(lens[docs.astype(np.int64)].sum())
    wall, dev, hwall = [], [], []
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        L.check(raw.call())
        t1 = time.perf_counter()
        ms = g.last_search_ms()[1]
        t2 = time.perf_counter()
        host_route(rd, sub_phrases)
        t3 = time.perf_counter()
        if r >= warmup:
            wall.append((t1 - t0) * 1e3)
            dev.append(ms)
            hwall.append((t3 - t2) * 1e3)
    res = {"shape": name, "phrases": n_p, "runs": runs, "warmup": warmup, "hits": int(raw.n.value),
           "candidates": int(cand), "candidate_document_bytes": nbytes, "row_chunks": int(row_chunks),
           "device": {"wall_ms": spread(wall), "device_ms": spread(dev)},
           "host": {"phrases": len(sub), "candidates": host_cand, "candidate_document_bytes": host_bytes,
                    "wall_ms": spread(hwall)},
           "note": "the host route ran on a seeded subset of %d of the %d phrases" % (len(sub), n_p)}
    res["device"]["wall_ms_per_phrase"] = res["device"]["wall_ms"]["median"] / n_p
    res["host"]["wall_ms_per_phrase"] = res["host"]["wall_ms"]["median"] / len(sub)
    res["scan_GBs_device"] = nbytes / max(res["device"]["device_ms"]["median"] * 1e-3, 1e-9) / 1e9
    res["host_scan_GBs_wall"] = host_bytes / max(res["host"]["wall_ms"]["median"] * 1e-3, 1e-9) / 1e9
    res["wall_per_phrase_speedup_over_host"] = res["host"]["wall_ms_per_phrase"] / res["device"]["wall_ms_per_phrase"]
    res.update(extra)
    if slop is not None:
        res["slop"] = slop
    return res


def doc_lengths(dc):
    offs = np.zeros(dc.n_docs + 1, np.uint64)
    synth._d2h(offs, dc.d_offsets, (dc.n_docs + 1) * 8, dc.device)
    return np.diff(offs.astype(np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000, help="documents of the cfg-2 corpus")
    ap.add_argument("--book-tokens", type=int, default=200_000, help="tokens per book-like document (~1 MB)")
    ap.add_argument("--books", type=int, default=64)
    ap.add_argument("--book-phrases", type=int, default=64)
    ap.add_argument("--host-phrases", type=int, default=4, help="phrases the host route runs on")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "phrase"))
    ap.add_argument("--slop", type=int, default=None,
                    help="time the sloppy call with this slop for every phrase (default: the exact call)")
    ap.add_argument("--skip", default="", help="comma-separated shapes to leave out (cfg2, book)")
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    skip = set(args.skip.split(",")) if args.skip else set()
    pre = "" if args.slop is None else "slop%d_" % args.slop

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
        lens = doc_lengths(dc)
        extra = {"corpus": "cfg2: %d docs x U[400,600] tokens, V=100000" % n}
        with g.reader() as rd:
            for n_p in [int(x) for x in args.batches.split(",")]:
                emit(shape(pre + "cfg2-phrase-%d" % n_p, g, rd, lens, n_p, args.host_phrases, args.runs, args.warmup, extra,
                           args.slop))
        g.close()
        dc.free()
    if "book" not in skip:
        nb, T = args.books, args.book_tokens
        dc = synth.DeviceCorpus(nb, V=100_000, len_min=T, len_max=T, seed=synth.SEED + 29)
        g = ShardIndex(vocab_capacity_log2=19)
        g.add_documents_device(dc.d_text, dc.d_offsets, nb, dc.total_bytes)
        g.commit()
        lens = doc_lengths(dc)
        extra = {"corpus": "books: %d docs x %d tokens, V=100000" % (nb, T)}
        with g.reader() as rd:
            emit(shape(pre + "book-phrase-%d" % args.book_phrases, g, rd, lens, args.book_phrases, args.host_phrases,
                       args.runs, args.warmup, extra, args.slop))
        g.close()
        dc.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
