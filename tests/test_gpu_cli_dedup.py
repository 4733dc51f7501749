"""`dashing2 cmp --presketched --greedy T[E]` end to end: the files are byte-equal to the files tests/dedup_ref.py writes from the
reference's loop on the oracle's floats (the text and binary forms of dedup_emit, src/dedup_core.cpp:423-449)."""
import json
import os
import subprocess

import numpy as np
import pytest

import dedup_ref as R
import knn_ref as K
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
KMER = 21
N, S = 300, 256
T = 0.25


def _run(args, **kw):
    r = subprocess.run([EXE] + args, capture_output=True, **kw)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


@pytest.fixture(scope="module")
def stacked(tmp_path_factory, oracle, d2g):
    """a presketched stack of 300 sketches of 256 registers (families in shuffled order + an identical group) with its names file;
    -> (path, names, (ids, constituents) of the reference's loop at T on the oracle's floats)"""
    d = tmp_path_factory.mktemp("dedup")
    sigs = K.family_sigs(N, S, seed=2027)
    sigs[100:112] = sigs[100]                                   # twelve identical sketches
    sigs = sigs[np.random.default_rng(3).permutation(N)]
    names = ["genome_%03d.fna" % i for i in range(N)]
    path = d / "stack.bin"
    with open(path, "wb") as f:
        np.array(sigs.shape, np.uint64).tofile(f)
        np.ones(N).tofile(f)
        sigs.tofile(f)
    with open(str(path) + ".names.txt", "w") as f:
        f.write("#Path\tSize\n" + "".join("%s\t1\n" % n for n in names))
    ids, cons = R.dedup_reference(K.oracle_values(oracle, sigs, d2g.SIMILARITY, k=KMER), T)
    assert 2 <= len(ids) <= N - 1 and max(len(c) for c in cons) >= 11
    return str(path), names, (ids, cons)


@pytest.mark.parametrize("arg", ["0.25", "0.25E"])
def test_cli_greedy_text_and_binary(stacked, tmp_path, arg):
    path, names, (ids, cons) = stacked
    out = tmp_path / "clusters.txt"
    _run(["cmp", "--presketched", "-k", str(KMER), "--greedy", arg, "--cmpout", str(out), path])
    assert out.read_bytes() == R.clusters_text(ids, cons, names, T)
    r = _run(["cmp", "--presketched", "-k", str(KMER), "--greedy", arg, path])                       # stdout
    assert r.stdout == R.clusters_text(ids, cons, names, T)
    out = tmp_path / "clusters.bin"
    _run(["cmp", "--presketched", "-k", str(KMER), "--greedy", arg, "--binary-output", "--cmpout", str(out), path])
    assert out.read_bytes() == R.clusters_bytes(ids, cons)
    indptr, indices = R.read_clusters_bytes(out.read_bytes())
    assert indptr.size == len(ids) + 1 and sorted(indices.tolist()) == list(range(N))


def test_cli_greedy_gpu_stats_and_devices_notice(stacked, tmp_path):
    path, names, (ids, cons) = stacked
    js = tmp_path / "stats.json"
    r = _run(["cmp", "--presketched", "-k", str(KMER), "--greedy", "0.25", "--gpu-stats", str(js), "--binary-output", "--cmpout", str(tmp_path / "o.bin"), path],
             env=dict(os.environ, D2G_DEVICES="0,0"))
    assert b"D2G_DEVICES ignored for this job (" in r.stderr and b"runs on GPU 0 alone" in r.stderr
    cmp = json.loads(js.read_text())["cmp"]
    assert cmp["shape"] == "greedy" and cmp["sketches"] == N and cmp["sketchsize"] == S and cmp["threshold"] == 0.25
    assert cmp["clusters"] == len(ids) and cmp["bytes_to_host"] == 4 * N
    dev = cmp["devices"][0]
    assert dev["dedup"]["launches"] >= 2 and dev["dedup"]["total_ms"] > 0          # 300 rows: two bands
    assert dev["k2"]["launches"] >= 1 and dev["k2"]["total_ms"] > 0 and "k2prep" in dev
    assert (tmp_path / "o.bin").read_bytes() == R.clusters_bytes(ids, cons)
