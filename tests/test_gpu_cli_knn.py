"""`dashing2 cmp --presketched --topk K | --similarity-threshold T` end to end: the files are byte-equal to the files built from
tests/knn_ref.py (knn_intended on the oracle's floats; the CSR layout of emitnn.cpp:7-11; the text through "%.8g")."""
import json
import os
import subprocess

import numpy as np
import pytest

import knn_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
K = 21
N, S = 300, 256


def _run(args, **kw):
    r = subprocess.run([EXE] + args, capture_output=True, **kw)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


@pytest.fixture(scope="module")
def stacked(tmp_path_factory, oracle, d2g):
    """a presketched stack of 300 sketches of 256 registers (families + an identical group + unrelated rows) with its names file;
    -> (path, names, {measure: N x N oracle floats})"""
    d = tmp_path_factory.mktemp("knn")
    sigs = R.family_sigs(N, S, seed=2026)
    sigs[100:112] = sigs[100]                                   # twelve identical sketches: ties beyond K = 7
    sigs[280:] = R.unrelated_sigs(20, S, seed=4) + 2.0          # twenty sketches that share nothing with anybody
    names = ["genome_%03d.fna" % i for i in range(N)]
    path = d / "stack.bin"
    with open(path, "wb") as f:
        np.array(sigs.shape, np.uint64).tofile(f)
        np.ones(N).tofile(f)
        sigs.tofile(f)
    with open(str(path) + ".names.txt", "w") as f:
        f.write("#Path\tSize\n" + "".join("%s\t1\n" % n for n in names))
    values = {m: R.oracle_values(oracle, sigs, m, k=K) for m in (d2g.SIMILARITY, d2g.POISSON_LLR)}
    return str(path), names, values


def test_cli_topk_binary(stacked, tmp_path, d2g):
    path, names, values = stacked
    out = tmp_path / "knn.bin"
    _run(["cmp", "--presketched", "-k", str(K), "--topk", "7", "--binary-output", "--cmpout", str(out), path])
    exp = R.knn_intended(values[d2g.SIMILARITY], K=7)
    assert out.read_bytes() == R.csr_bytes(exp)
    rows = R.csr_rows(R.read_csr_bytes(out.read_bytes()))
    assert len(rows[100][0]) == 11 and len(rows[290][0]) == 0   # the identical group lists itself whole; unrelated sketches list nobody
    out2 = tmp_path / "knn2.bin"
    _run(["cmp", "--presketched", "-k", str(K), "--top-k", "7", "--binary-output", "--cmpout", str(out2), path])    # the alias
    assert out2.read_bytes() == out.read_bytes()


def test_cli_similarity_threshold_binary(stacked, tmp_path, d2g):
    path, names, values = stacked
    out = tmp_path / "thr.bin"
    _run(["cmp", "--presketched", "-k", str(K), "--similarity-threshold", "0.3", "--binary-output", "--cmpout", str(out), path])
    exp = R.knn_intended(values[d2g.SIMILARITY], T=0.3)
    assert exp[1].size > N
    assert out.read_bytes() == R.csr_bytes(exp)


def test_cli_mash_distance_topk_binary_and_threshold(stacked, tmp_path, d2g):
    path, names, values = stacked
    out = tmp_path / "mash.bin"
    _run(["cmp", "--presketched", "-k", str(K), "--mash-distance", "--topk", "7", "--binary-output", "--cmpout", str(out), path])
    exp = R.knn_intended(values[d2g.POISSON_LLR], K=7, isdist=True)
    assert out.read_bytes() == R.csr_bytes(exp)
    assert np.isinf(exp[2]).any()                               # the unrelated sketches list everybody at inf, all tied
    _run(["cmp", "--presketched", "-k", str(K), "--mash-distance", "--similarity-threshold", "0.05", "--binary-output", "--cmpout", str(out), path])
    assert out.read_bytes() == R.csr_bytes(R.knn_intended(values[d2g.POISSON_LLR], T=0.05, isdist=True))


def test_cli_text_output_and_stdout(stacked, tmp_path, d2g):
    path, names, values = stacked
    out = tmp_path / "knn.txt"
    _run(["cmp", "--presketched", "-k", str(K), "--topk", "7", "--cmpout", str(out), path])
    exp = R.knn_text(R.knn_intended(values[d2g.SIMILARITY], K=7), names)
    assert out.read_bytes() == exp
    r = _run(["cmp", "--presketched", "-k", str(K), "--mash-distance", "--topk", "3", path])          # stdout
    assert r.stdout == R.knn_text(R.knn_intended(values[d2g.POISSON_LLR], K=3, isdist=True), names)
    assert b":inf" in r.stdout


def test_cli_knn_gpu_stats_and_devices_notice(stacked, tmp_path, d2g):
    path, names, values = stacked
    js = tmp_path / "stats.json"
    r = _run(["cmp", "--presketched", "-k", str(K), "--topk", "7", "--gpu-stats", str(js), "--binary-output", "--cmpout", str(tmp_path / "o.bin"), path],
             env=dict(os.environ, D2G_DEVICES="0,0"))
    assert b"D2G_DEVICES ignored for this job (" in r.stderr
    st = json.loads(js.read_text())
    cmp = st["cmp"]
    assert cmp["shape"] == "topk" and cmp["topk"] == 7 and cmp["sketches"] == N and cmp["sketchsize"] == S
    assert cmp["neighbours"] == R.knn_intended(values[d2g.SIMILARITY], K=7)[1].size
    dev = cmp["devices"][0]
    assert dev["knn"]["launches"] >= 1 and dev["knn"]["total_ms"] > 0        # the selection kernel, next to the pair kernel
    assert dev["k2"]["launches"] >= 1 and dev["k2"]["total_ms"] > 0
    assert (tmp_path / "o.bin").read_bytes() == R.csr_bytes(R.knn_intended(values[d2g.SIMILARITY], K=7))
