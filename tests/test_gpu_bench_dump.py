"""bench.py on the GPU: a plain run prints the result line for the timed steps
alone, and --dump-outputs writes the index of the last timed step as float
arrays that equal what an index built here from the same (host-generated,
bit-identical) corpus answers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tfidf_amd import synth
from tfidf_amd.engine import ShardIndex

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS, V, LMIN, LMAX = 1500, 5000, 40, 80
NAMES = ["stats", "df", "doc_len", "doc_terms", "top10_docs", "top10_scores", "top10_counts"] + \
        ["hits%d_%s" % (i, k) for i in range(4) for k in ("docs", "scores")]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--docs", str(DOCS), "--vocab", str(V), "--len-min", str(LMIN), "--len-max", str(LMAX),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    return json.loads(lines[0]), {n: np.load(out / (n + ".npy")) for n in NAMES}, sorted(os.listdir(out))


def test_plain_result_line(run):
    r, _, _ = run
    assert r["steps"] == 3 and r["warmup"] == 1 and r["n_gpus"] == 1
    assert r["unit"] == "docs/s" and r["higher_is_better"] is True and "dtype" in r and "metric" in r
    assert r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(DOCS / (r["ms_per_step"] * 1e-3), rel=1e-9)
    for leg in ("queries", "end_to_end", "cpu_baseline"):
        assert leg not in r
    assert r["roofline"]["measured_copy_GBs"] is None


def test_dump_is_float_arrays_of_the_built_index(run):
    _, a, files = run
    assert files == sorted(n + ".npy" for n in NAMES)
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    texts = synth.corpus(DOCS, V=V, len_min=LMIN, len_max=LMAX)
    with ShardIndex(device=0) as g:
        g.add_documents(texts)
        g.commit()
        st = g.stats()
        assert a["stats"].tolist() == [st[k] for k in ("num_docs", "doc_count", "sum_ttf", "num_terms", "nnz",
                                                       "text_bytes", "long_docs")]
        assert a["df"].shape == (V, 3)
        for r, dl, de in a["df"][[0, 1, 99, 1234, V - 1]].tolist():
            assert (dl, de) == g.df(synth.word(int(r)))
        assert a["doc_len"].shape == (DOCS, 3) and a["doc_len"][:, 0].tolist() == list(range(DOCS))
        for d in (0, 7, DOCS - 1):
            assert tuple(a["doc_len"][d, 1:].tolist()) == g.doc_len(d)
        d0 = a["doc_terms"][a["doc_terms"][:, 0] == 0]
        assert d0[:, 2].tolist() == [tf for _, tf in sorted(g.doc_terms(0).items())]
        qs = synth.queries(1024)
        docs, scores, counts = g.search_batch(qs, 10)
        assert np.array_equal(a["top10_docs"], docs) and np.array_equal(a["top10_counts"], counts)
        assert np.array_equal(a["top10_scores"].view(np.uint32), scores.view(np.uint32))
        assert counts.max() > 0
        for i in range(4):
            d, s = g.search_all_arrays(qs[i])
            assert np.array_equal(a["hits%d_docs" % i], d)
            assert np.array_equal(a["hits%d_scores" % i].view(np.uint32), s.view(np.uint32))
