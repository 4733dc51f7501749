"""`dashing2 sketch / cmp --bed` end to end on a GPU: the stacked file and the names against the restatement of tests/bed_ref.py
finalised by the oracle, the cache files (always written, loaded with --cache, recomputed when truncated), cmp from interval files
against the oracle's all-pairs values over the reference signatures, --multiset and --normalize-intervals against BagMinHash over the
reference lists, one nearest-neighbour job, the gzip refusal, --gpu-stats."""
import json
import os
import subprocess

import numpy as np
import pytest

import bed_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
S = 64


def _run(args, env=None, ok=True):
    e = dict(os.environ)
    for k in ("D2G_DEVICES", "D2G_DEVICE_PARSE"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([EXE] + args, capture_output=True, env=e)
    assert (r.returncode == 0) == ok, r.stderr.decode()[-2000:]
    return r


def _stacked(cards, sigs):
    sigs = np.asarray(sigs, np.float64)
    return np.array(sigs.shape, np.uint64).tobytes() + np.asarray(cards, np.float64).tobytes() + sigs.tobytes()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """peaks over three chromosomes, a shifted copy, a file that shares a third of them, a small file with a comment and CRLF"""
    d = tmp_path_factory.mktemp("bed_cli")
    rng = np.random.default_rng(30)
    chroms = [b"chr1", b"chr2", b"chrX"]

    def peaks(n, shift=0):
        out = []
        for _ in range(n):
            a = int(rng.integers(0, 200000)) + shift
            out.append((chroms[int(rng.integers(0, 3))], a, a + int(rng.integers(1, 400))))
        return out
    base = peaks(60)
    beds = [base, [(c, a + 40, b + 40) for c, a, b in base], base[:20] + peaks(40, 500000), [(b"1", 5, 3000), (b"chr1", 100, 200)]]
    texts = [b"".join(b"%s\t%d\t%d\tpeak\n" % l for l in bed) for bed in beds]
    texts[3] = b"#small\r\n" + texts[3].replace(b"\n", b"\r\n")
    paths = []
    for i, t in enumerate(texts):
        p = d / f"p{i}.bed"
        p.write_bytes(t)
        paths.append(str(p))
    return d, texts, paths


@pytest.fixture(scope="module")
def ref(oracle, case):
    """the reference sketches in set space: (sigs [4][S], cards [4])"""
    regs = R.oph_registers_files(case[1], S)
    fin = [oracle.regs_finalize(r) for r in regs]
    return np.stack([f[0][:S] for f in fin]), np.array([f[1] for f in fin])


def _lines(text):
    return [(R.chrom_hash(n), a, b) for n, a, b in R.parse(text)]


def test_stack_names_and_cache_files(case, ref, tmp_path):
    d, texts, paths = case
    sigs, cards = ref
    out = tmp_path / "s.bin"
    _run(["sketch", "--bed", "-S", str(S), "-k", "17", "-w", "30", "-C", "-o", str(out)] + paths)      # -k, -w, -C play no part
    assert out.read_bytes() == _stacked(cards, sigs)
    names = (tmp_path / "s.bin.names.txt").read_text().splitlines()
    assert names[0] == "#Name\tCardinality" and [l.split("\t")[0] for l in names[1:]] == paths
    assert [float(l.split("\t")[1]) for l in names[1:]] == cards.tolist()
    # written without --cache, next to the inputs: [f64 card][f64 x S]
    for i, p in enumerate(paths):
        blob = np.fromfile(p + ".opss", np.float64)
        assert blob.size == S + 1 and blob[0] == cards[i] and np.array_equal(blob[1:].view(np.uint64), sigs[i].view(np.uint64))
    # --cache loads what is there: a card changed in a cache file shows in the next stack; a truncated file is sketched again
    pre = tmp_path / "pre"
    pre.mkdir()
    args = ["sketch", "--bed", "-S", str(S), "--outprefix", str(pre), "--cache", "-o", str(out)] + paths
    _run(args)
    c1 = pre / "p1.bed.opss"
    blob = np.fromfile(c1, np.float64)
    blob[0] = 777.0
    blob.tofile(c1)
    with open(pre / "p2.bed.opss", "r+b") as f:
        f.truncate(8 * S)
    r = _run(args)
    want = cards.copy()
    want[1] = 777.0
    assert out.read_bytes() == _stacked(want, sigs)
    assert r.stderr.decode().count("does not hold a sketch of size") == 1 and os.path.getsize(pre / "p2.bed.opss") == 8 * (S + 1)
    # without --cache the files are not read
    _run(["sketch", "--bed", "-S", str(S), "--outprefix", str(pre), "-o", str(out)] + paths)
    assert out.read_bytes() == _stacked(cards, sigs) and np.fromfile(c1, np.float64)[0] == cards[1]


def test_cmp_square_and_triangle_against_the_oracle(oracle, case, ref, tmp_path):
    d, texts, paths = case
    sigs, cards = ref
    N = len(paths)
    for flags, meas in (([], oracle.SIMILARITY), (["--containment"], oracle.CONTAINMENT), (["--mash-distance"], oracle.POISSON_LLR)):
        sq, ut = tmp_path / "sq.bin", tmp_path / "ut.bin"
        _run(["cmp", "--bed", "-S", str(S), "-k", "31", "--square", "--binary-output", "--outprefix", str(tmp_path), "--cmpout", str(sq)] + flags + paths)
        _run(["sketch", "--bed", "-S", str(S), "-k", "31", "--binary-output", "--outprefix", str(tmp_path), "--cmpout", str(ut)] + flags + paths)
        want = oracle.allpairs_ut(sigs, cards, measure=meas, k=31)
        got = np.fromfile(sq, np.float32).reshape(N, N)
        if meas != oracle.CONTAINMENT:                                     # containment is not symmetric: its triangle is the (i, j) half
            assert np.array_equal(got, got.T)
        assert np.array_equal(got[np.triu_indices(N, 1)].view(np.uint32), want.view(np.uint32)), flags
        assert np.array_equal(np.fromfile(ut, np.float32).view(np.uint32), want.view(np.uint32)), flags
    sim = oracle.allpairs_ut(sigs, cards)
    assert sim[0] > 0.5 and sim[1] > 0.1                                   # the shifted copy, the file that shares a third of the peaks
    # the options line says BED where Fastx stands
    text = _run(["cmp", "--bed", "-S", str(S), "-k", "31", "--outprefix", str(tmp_path)] + paths).stdout.decode()
    assert f"#Dashing2Options: Dashing2Options;k:31;parsebyfile;trimchr;sketchsize:{S};sketchtype:onepermsetsketch;BED;outprefix:" in text and "Fastx" not in text


@pytest.mark.parametrize("normalize", [False, True], ids=["counts", "normalized"])
def test_multiset_and_normalized_stacks(oracle, case, tmp_path, normalize):
    d, texts, paths = case
    out = tmp_path / "m.bin"
    _run(["sketch", "--bed", "--multiset", "-S", str(S), "--outprefix", str(tmp_path), "-o", str(out)] + (["--normalize-intervals"] if normalize else []) + paths)
    sigs, tws = [], []
    for t in texts:
        ids, ws, total = R.multiset_lists(_lines(t), normalize)
        sigs.append(oracle.bmh_from_weighted(ids, ws, S)[0])
        tws.append(total)
    assert out.read_bytes() == _stacked(tws, sigs)
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith("bmh")) == [f"p{i}.bed.d2gbmh" for i in range(4)]
    b = tmp_path / "m.cmp"
    _run(["cmp", "--bed", "--multiset", "-S", str(S), "--binary-output", "--outprefix", str(tmp_path), "--cmpout", str(b)] + (["--normalize-intervals"] if normalize else []) + paths)
    p = tmp_path / "p.cmp"
    _run(["cmp", "--presketched", "--multiset", "--binary-output", "--cmpout", str(p), str(out)])
    assert b.read_bytes() == p.read_bytes() and np.fromfile(b, np.float32)[0] > 0


def test_topk_comes_for_free(case, ref, tmp_path):
    d, texts, paths = case
    stack, a, b = tmp_path / "s.bin", tmp_path / "a.bin", tmp_path / "b.bin"
    _run(["sketch", "--bed", "-S", str(S), "--outprefix", str(tmp_path), "-o", str(stack)] + paths)
    _run(["cmp", "--bed", "-S", str(S), "--outprefix", str(tmp_path), "--topk", "2", "--binary-output", "--cmpout", str(a)] + paths)
    _run(["cmp", "--presketched", "--topk", "2", "--binary-output", "--cmpout", str(b), str(stack)])
    blob = a.read_bytes()
    nids, nnz = np.frombuffer(blob[:16], np.uint64)
    assert blob == b.read_bytes() and nids == 4 and nnz == 9                # two each, and file 3's second place is a tie: both are kept
    indptr = np.frombuffer(blob[16:16 + 8 * 5], np.uint64)
    indices = np.frombuffer(blob[16 + 8 * 5:16 + 8 * 5 + 4 * int(nnz)], np.uint32)
    assert indices[int(indptr[0])] == 1 and indices[int(indptr[1])] == 0 and indptr[4] - indptr[3] == 3


def test_gzip_and_malformed_inputs_are_refused_by_name(case, tmp_path):
    gz = tmp_path / "x.bed.gz"
    gz.write_bytes(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03rest")
    r = _run(["sketch", "--bed", "-S", str(S), "-o", str(tmp_path / "o.bin"), str(gz)], ok=False)
    assert "gzip" in r.stderr.decode() and str(gz) in r.stderr.decode() and not os.path.exists(tmp_path / "o.bin")
    bad = tmp_path / "bad.bed"
    bad.write_bytes(b"chr1\t1\t2\nchr1 3 4\n")
    r = _run(["sketch", "--bed", "-S", str(S), "-o", str(tmp_path / "o.bin"), str(bad)], ok=False)
    assert "Malformed line: chr1 3 4" in r.stderr.decode() and not os.path.exists(str(bad) + ".opss")


def test_gpu_stats_has_the_new_keys(case, tmp_path):
    d, texts, paths = case
    js = tmp_path / "stats.json"
    _run(["sketch", "--bed", "-S", str(S), "--outprefix", str(tmp_path), "-o", str(tmp_path / "s.bin"), "--gpu-stats", str(js)] + paths)
    st = json.loads(js.read_text())
    dev, iv = st["sketch"]["devices"][0], st["sketch"]["intervals"]
    assert dev["k1i"]["launches"] == 1 and dev["k1i"]["total_ms"] > 0 and dev["k1iexpand"]["launches"] == 0 and dev["k1ibmh"]["launches"] == 0
    lines = [R.parse(t) for t in texts]
    assert iv["lines"] == sum(len(l) for l in lines) and iv["positions"] == sum(b - a for l in lines for _, a, b in l) and iv["runs"] == 0
    assert "K1i" in st["sketch"]["space"] and st["sketch"]["sketched"] == 4
    _run(["sketch", "--bed", "--multiset", "-S", str(S), "--outprefix", str(tmp_path), "-o", str(tmp_path / "m.bin"), "--gpu-stats", str(js)] + paths)
    st = json.loads(js.read_text())
    dev, iv = st["sketch"]["devices"][0], st["sketch"]["intervals"]
    assert dev["k1i"]["launches"] == 0 and dev["k1iexpand"]["launches"] >= 1 and dev["k1ibmh"]["launches"] >= 1 and iv["runs"] >= 4
