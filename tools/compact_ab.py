#!/usr/bin/env python3
"""tfidf_compact against a plain device-to-device copy, and the commit with
and without the dead documents.

One shape per run (a corpus generated on the device, keyless):
  cfg2-1pct     1 M documents x U[400, 600] tokens, 1 % dead at random
  cfg2-tenth    the same corpus, every tenth document dead
  cfg2-half     the same corpus, every other document dead
  cfg5-half     the cfg-5 shape (6.25 M documents x U[48, 80] tokens, V = 5 M), every other dead

Recorded per shape, median and [min, max] over --runs rounds:
  kernel_ms       k_compact_text (tfidf_compact's ms_device: HIP events on the index's stream)
  compact_ms      the whole tfidf_compact call (wall: plan, allocation, copy, host tables)
  memcpy_ms       a contiguous hipMemcpyAsync device-to-device copy of the same number of
                  bytes (tfidf_device_copy_ms: HIP events, same process) -- the yardstick
  commit_dead_ms  tfidf_commit with the dead documents in place (what the parent commit
                  does for the same calls): device time of the build and wall time
  commit_compacted_ms  tfidf_commit after the compaction
Each round stages the corpus again (clear, add, delete), since a compaction
cannot be repeated on a compacted index.  One JSON line; --out writes it to a file.
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

SHAPES = {
    "cfg2-1pct": dict(docs=1_000_000, vocab=100_000, len_min=400, len_max=600, cap=19, dead="random", frac=0.01),
    "cfg2-tenth": dict(docs=1_000_000, vocab=100_000, len_min=400, len_max=600, cap=19, dead="every", every=10),
    "cfg2-half": dict(docs=1_000_000, vocab=100_000, len_min=400, len_max=600, cap=19, dead="every", every=2),
    "cfg5-half": dict(docs=6_250_000, vocab=5_000_000, len_min=48, len_max=80, cap=23, dead="every", every=2),
}


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    ap.add_argument("--docs", type=int, default=0, help="override the shape's document count")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sh = dict(SHAPES[args.shape])
    if args.docs:
        sh["docs"] = args.docs
    from tfidf_amd.engine import ShardIndex
    lib = L.load()
    n = sh["docs"]
    dc = synth.DeviceCorpus(n, V=sh["vocab"], len_min=sh["len_min"], len_max=sh["len_max"])
    offs = np.zeros(n + 1, np.uint64)
    synth._d2h(offs, dc.d_offsets, (n + 1) * 8)
    lens = np.diff(offs.astype(np.int64))
    dead = np.zeros(n, bool)
    if sh["dead"] == "random":
        dead[np.random.default_rng(20251019).random(n) < sh["frac"]] = True
    else:
        dead[::sh["every"]] = True
    dead_ids = np.nonzero(dead)[0]
    keys = [b"%d" % i for i in dead_ids.tolist()]
    koffs = np.zeros(len(keys) + 1, np.uint64)
    koffs[1:] = np.cumsum([len(k) for k in keys], dtype=np.uint64)
    kblob = b"".join(keys)
    live_bytes = int(lens[~dead].sum())
    dead_bytes = int(lens[dead].sum())
    # runs of the plan: a live document with bytes that follows a dead one (or starts the corpus)
    starts = ~dead & (lens > 0)
    n_runs = int((starts & np.concatenate([[True], dead[:-1]])).sum())
    res = {"shape": args.shape, "docs": n, "runs": args.runs, "dead_docs": int(dead.sum()), "live_bytes": live_bytes,
           "dead_bytes": dead_bytes, "plan_runs": n_runs,
           "mean_run_bytes": live_bytes / max(n_runs, 1)}

    g = ShardIndex(vocab_capacity_log2=sh["cap"])
    nd, nb, ms = C.c_uint64(), C.c_uint64(), C.c_float()

    def stage():
        g.clear()
        g.add_documents_device(dc.d_text, dc.d_offsets, n, dc.total_bytes)
        L.check(lib.tfidf_delete_docs(g._h, kblob, L.ptr(koffs, C.c_uint64), len(keys), C.byref(nd)))
        assert nd.value == len(keys), (nd.value, len(keys))

    def commit():
        t0 = time.perf_counter()
        g.commit()
        t1 = time.perf_counter()
        return g.commit_timing()["ms_total"], (t1 - t0) * 1e3

    # the plain copy of as many bytes as the compaction moves
    cp = np.zeros(args.runs, np.float32)
    L.check(lib.tfidf_device_copy_ms(0, C.c_void_p(dc.d_text), live_bytes, args.runs, L.ptr(cp, C.c_float)))
    res["memcpy_ms"] = spread(cp.tolist())

    kern, call, cd_dev, cd_wall, cc_dev, cc_wall = [], [], [], [], [], []
    for r in range(args.runs + 1):           # round 0 warms up
        stage()
        a = commit()
        t0 = time.perf_counter()
        L.check(lib.tfidf_compact(g._h, C.byref(nb), C.byref(ms)))
        t1 = time.perf_counter()
        assert nb.value == dead_bytes
        b = commit()
        if r:
            kern.append(ms.value)
            call.append((t1 - t0) * 1e3)
            cd_dev.append(a[0]); cd_wall.append(a[1])
            cc_dev.append(b[0]); cc_wall.append(b[1])
    st = g.stats()
    assert st["num_docs"] == n - len(keys) and st["text_bytes"] == live_bytes and st["dead_docs"] == 0
    res["kernel_ms"] = spread(kern)
    res["compact_ms"] = spread(call)
    res["commit_dead_ms"] = {"device": spread(cd_dev), "wall": spread(cd_wall)}
    res["commit_compacted_ms"] = {"device": spread(cc_dev), "wall": spread(cc_wall)}
    res["kernel_over_memcpy"] = res["kernel_ms"]["median"] / res["memcpy_ms"]["median"]
    res["memcpy_spread"] = res["memcpy_ms"]["max"] / res["memcpy_ms"]["min"]
    res["kernel_GBs_read_plus_write"] = 2 * live_bytes / (res["kernel_ms"]["median"] * 1e-3) / 1e9
    res["memcpy_GBs_read_plus_write"] = 2 * live_bytes / (res["memcpy_ms"]["median"] * 1e-3) / 1e9
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
