#!/usr/bin/env python3
"""Fuzzy term lookup (tfidf_reader_fuzzy_terms_batch) against the only route
without it: export the vocabulary to the host and run the same rules
(csrc/fuzzy_plan.h: length and prefix filter, banded OSA distance) over its
strings on one thread (tools/fuzzy_host_scan.cpp, built with the host compiler
at -O2 into tools/bin/).  The host route's time is its scan alone: neither the
export of the vocabulary nor the ordering of the candidates is counted, which
flatters it.

Shapes: the vocabulary of the cfg-2 corpus (--docs documents x U[400, 600]
tokens, V = 100 k, block-major) and of the cfg-5 shape (--docs5 documents x
U[48, 80] tokens, V = 5 M, term-major).  Per shape and max_edits in {1, 2}:
1, 64 and 1 024 input terms (vocabulary words with one letter changed or two
letters swapped, fixed seed), max_out 10.  Per case, median and [min, max]
over --runs timed calls after --warmup:
  device_ms   ms_device of the call (HIP events on the call's stream)
  wall_ms     host clock around the call
  host_ms     the one-thread host scan (--host-runs runs, 1 when long; over
              --host-pairs pairs it runs on the first terms only and is scaled
              by the number of terms, marked host_extrapolated)
and the ratio host_ms / device_ms, the vocabulary size, the candidates found
by both routes (they must agree) and the chunks of the device call.  One JSON
file per shape under --out-dir, one line per case on stdout."""
import argparse
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tf-idf-distributed-system_amd"))
sys.path.insert(0, REPO)

from tfidf_amd import _lib as L  # noqa: E402
from tfidf_amd import synth  # noqa: E402
from tfidf_amd.engine import ShardIndex  # noqa: E402

HOST_EXE = os.path.join(REPO, "tools", "bin", "fuzzy_host_scan")


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def host_program():
    if not os.path.exists(HOST_EXE):
        cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        os.makedirs(os.path.dirname(HOST_EXE), exist_ok=True)
        subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", os.path.join(REPO, "tf-idf-distributed-system_amd", "csrc"),
                               os.path.join(REPO, "tools", "fuzzy_host_scan.cpp"), "-o", HOST_EXE])
    return HOST_EXE


def vocab_strings(g):
    """The vocabulary as strings from the exported keys.  The synthetic
    corpora hold ASCII words of <= 16 bytes only, whose keys are their bytes; a
    real caller would also have to read every hashed key's term from a document."""
    keys, _, _ = g.vocab_export()
    lo, hi = keys[:, 0].copy(), keys[:, 1].copy()
    long_ = (lo >> np.uint64(63)).astype(bool)
    assert not ((lo >> np.uint64(55)) & np.uint64(1)).any()                     # no hashed key
    assert not (long_ & ((lo >> np.uint64(47)) & np.uint64(1)).astype(bool)).any()   # no exact non-ASCII key
    lo &= np.uint64((1 << 63) - 1)
    hi &= np.uint64((1 << 63) - 1)
    hi[~long_] = 0
    raw = np.stack([lo, hi], axis=1).view(np.uint8).reshape(-1, 16)
    lens = (raw != 0).sum(axis=1)
    return [raw[i, :lens[i]].tobytes() for i in range(len(raw))]


def misspelt(n, V, seed=20261020):
    """n vocabulary words of ranks uniform in [100, V), each with two adjacent
    letters swapped (even draws) or one letter replaced (odd draws)."""
    out = []
    s2 = synth.mix64(seed)
    for i in range(n):
        h = synth.mix64(s2 ^ i)
        w = bytearray(synth.word(100 + h % (V - 100)))
        at = (h >> 32) % max(len(w) - 1, 1)
        if h & (1 << 20) and len(w) >= 2:
            w[at], w[at + 1] = w[at + 1], w[at]
        else:
            w[at] = 97 + (w[at] - 97 + 1 + (h >> 40) % 25) % 26
        out.append(bytes(w))
    return out


def host_scan(vblob, nv, terms, max_edits, runs, tmp):
    path = os.path.join(tmp, "scan.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<III", max_edits, 0, nv))
        f.write(vblob)
        f.write(struct.pack("<I", len(terms)) + b"".join(struct.pack("<I", len(t)) + t for t in terms))
    ms, found = [], None
    for _ in range(runs):
        out = subprocess.run([host_program(), path], capture_output=True, text=True, check=True).stdout.split()
        ms.append(float(out[0]))
        found = int(out[1])
    return ms, found


def shape(name, docs, V, len_min, len_max, cap, inversion, args, tmp):
    corpus = synth.DeviceCorpus(docs, V=V, len_min=len_min, len_max=len_max)
    g = ShardIndex(vocab_capacity_log2=cap, inversion=inversion)
    g.add_documents_device(corpus.d_text, corpus.d_offsets, docs, corpus.total_bytes)
    g.commit()
    st = g.stats()
    vocab = vocab_strings(g)
    vblob = b"".join(struct.pack("<I", len(v)) + v for v in vocab)
    cases = []
    with g.reader() as rd:
        for max_edits in (1, 2):
            for n in (1, 64, 1024):
                terms = misspelt(n, V)
                dev, wall, out = [], [], None
                runs = args.runs if n * len(vocab) <= 1_000_000_000 else min(args.runs, 3)
                for r in range(args.warmup + runs):
                    t0 = time.perf_counter()
                    out = rd.fuzzy_terms_batch_arrays(terms, max_edits, 0, 10)
                    t1 = time.perf_counter()
                    if r >= args.warmup:
                        dev.append(out[6])
                        wall.append((t1 - t0) * 1e3)
                chunks = g.last_fuzzy_chunks()
                # the host scan is linear in the terms (every pair is tested on its own): above
                # --host-pairs pairs it runs over the first terms that fit and is scaled up, and says so
                n_host = max(1, min(n, args.host_pairs // max(len(vocab), 1)))
                h_ms, h_found = host_scan(vblob, len(vocab), terms[:n_host], max_edits,
                                          1 if n_host * len(vocab) > args.host_pairs // 4 else args.host_runs, tmp)
                h_ms = [x * n / n_host for x in h_ms]
                found = int(out[1][:n_host].sum())
                c = {"max_edits": max_edits, "terms": n, "max_out": 10, "candidates": found,
                     "host_candidates": h_found, "agree": found == h_found, "scan_chunks": chunks[0],
                     "cand_chunks": chunks[1], "device_ms": spread(dev), "wall_ms": spread(wall),
                     "host_ms": spread(h_ms), "host_runs": len(h_ms),
                     "host_terms_run": n_host, "host_extrapolated": n_host < n, "all_candidates": int(out[1].sum())}
                c["host_over_device"] = c["host_ms"]["median"] / c["device_ms"]["median"]
                c["host_over_wall"] = c["host_ms"]["median"] / c["wall_ms"]["median"]
                cases.append(c)
                print("%s e=%d terms=%4d: device %.3f ms [%.3f, %.3f]  wall %.3f ms  host %.1f ms  x%.0f  cands %d %s"
                      % (name, max_edits, n, c["device_ms"]["median"], c["device_ms"]["min"], c["device_ms"]["max"],
                         c["wall_ms"]["median"], c["host_ms"]["median"], c["host_over_device"], found,
                         "ok" if c["agree"] else "MISMATCH %d" % h_found), flush=True)
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
    ap.add_argument("--docs", type=int, default=1_000_000, help="documents of the cfg-2 corpus")
    ap.add_argument("--docs5", type=int, default=6_250_000, help="documents of the cfg-5 shape (0 = skip)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--host-pairs", type=int, default=400_000_000,
                    help="(term, vocabulary term) pairs the host scan runs at most; beyond, it is scaled from fewer terms")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "fuzzy"))
    args = ap.parse_args()
    L.load()
    with tempfile.TemporaryDirectory() as tmp:
        if args.docs:
            shape("cfg2", args.docs, 100_000, 400, 600, default_cap(100_000), L.INVERSION_AUTO, args, tmp)
        if args.docs5:
            shape("cfg5-shape", args.docs5, 5_000_000, 48, 80, default_cap(5_000_000), L.INVERSION_TERM, args, tmp)


if __name__ == "__main__":
    main()
