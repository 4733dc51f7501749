"""`dashing2 sketch|cmp --set / --countdict` on a GPU: the files they write, byte for byte, and every cmp output against exact_ref.py
(k3_seam_cases' pure-Python k-mer enumerator, the literal merge's closed form, CORRECT_RES in NumPy doubles) rendered with the float
text of oracle/textfmt.py.  Four tiny inputs -- FASTA, FASTA with every record twice, FASTQ, gzipped FASTA -- that share stretches, so
that intersections, counts and thresholds all bite; -k 21."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import exact_ref as X
import k3_seam_cases as C
from conftest import ROOT
from oracle import textfmt

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
K = 21
MEASURE_FLAGS = {X.SIMILARITY: [], X.CONTAINMENT: ["--containment"], X.SYMMETRIC_CONTAINMENT: ["--symmetric-containment"],
                 X.POISSON_LLR: ["--mash-distance"], X.INTERSECTION: ["--intersection"], X.UNION_SIZE: ["--union-size"]}


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("D2G_DEVICES", None)
    e.update(env or {})
    r = subprocess.run([EXE] + args, capture_output=True, timeout=120, env=e)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def fastq(records, name):
    return b"".join(b"@%s_%d\n%s\n+\n%s\n" % (name.encode(), i, r.encode(), b"I" * len(r)) for i, r in enumerate(records))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """-> (paths, batch, filter path, filter keys)"""
    rng = np.random.default_rng(5200)
    base, other = C.random_bases(rng, 1500), C.random_bases(rng, 900)
    genomes = [[base], [base[:750], base[:750], other[:300]], [base[400:1200], other, other[100:400], other[100:400]], [other[200:], "ACGTNNACGT", base[1300:]]]
    d = tmp_path_factory.mktemp("exact_fa")
    paths = [str(d / "g0.fa"), str(d / "g1.fa"), str(d / "g2.fq"), str(d / "g3.fa.gz")]
    open(paths[0], "wb").write(C.fasta(genomes[0], "g0"))
    open(paths[1], "wb").write(C.fasta(genomes[1], "g1"))
    open(paths[2], "wb").write(fastq(genomes[2], "g2"))
    with gzip.open(paths[3], "wb") as f:
        f.write(C.fasta([genomes[3][0], genomes[3][2]], "g3"))
    genomes[3] = [genomes[3][0], genomes[3][2]]
    fpath = str(d / "filter.fa")
    open(fpath, "wb").write(C.fasta([base[600:1000]], "filter"))
    fkeys = C.key_counts((base[600:1000],), K, True, 0)[0]
    return paths, C.Batch("cli_exact", K, 16, True, 0, genomes), fpath, fkeys


def opts_string(weighted, c=0, outprefix=None, cmp=True, extra=""):
    return ("Dashing2Options;k:%d;parsebyfile;trimchr;sketchsize:1024%s;sketchtype:mmerset64%s;Fastx%s;canon%s"
            % (K, ";%d" % c if c else "", ",kmercountsf64" if weighted else "", ";outprefix:" + outprefix if outprefix else "", extra))


def expected(sets, weighted, measure, names):
    iszm = X.isz_matrix(sets, weighted)
    cards = [X.card(k, c, weighted) for k, c in sets]
    return iszm, cards, X.measure_ut(iszm, cards, measure, K)


def test_the_inputs_bite(inputs):
    _, batch, _, fkeys = inputs
    sets = X.exact_sets(batch)
    m = X.isz_matrix(sets, False)
    assert (X.ut(m) > 0).all() and len({int(v) for v in X.ut(m)}) == 6
    assert any((c > 1).any() for _, c in sets) and (X.isz_matrix(sets, True) >= m).all() and not np.array_equal(X.isz_matrix(sets, True), m)
    assert sum(len(k) for k, _ in X.exact_sets(batch, 1.0)) < sum(len(k) for k, _ in sets)
    assert np.isin(sets[0][0], fkeys).sum() == 380


@pytest.mark.parametrize("weighted", [False, True], ids=["set", "countdict"])
def test_sketch_writes_the_per_input_files(inputs, tmp_path, weighted):
    paths, batch, _, _ = inputs
    pre = str(tmp_path / "pre")
    os.mkdir(pre)
    _run(["sketch", "--countdict" if weighted else "--set", "-k", str(K), "--outprefix", pre] + paths)
    sets = X.exact_sets(batch)
    want = {os.path.basename(X.makedest(p, K, outprefix=pre)) for p in paths}
    if weighted:
        want |= {os.path.basename(X.counts_path(X.makedest(p, K, outprefix=pre))) for p in paths}
    assert set(os.listdir(pre)) == want and all(".sketchsize" not in n for n in want)
    for p, (keys, counts) in zip(paths, sets):
        kf = X.makedest(p, K, outprefix=pre)
        assert open(kf, "rb").read() == X.key_file_bytes(keys, counts, weighted), kf
        if weighted:
            assert open(X.counts_path(kf), "rb").read() == X.count_file_bytes(counts)


@pytest.mark.parametrize("weighted", [False, True], ids=["set", "countdict"])
@pytest.mark.parametrize("measure", X.MEASURES)
def test_cmp_tsv_of_every_measure(inputs, tmp_path, measure, weighted):
    paths, batch, _, _ = inputs
    pre = str(tmp_path / "pre")
    os.mkdir(pre)
    out = tmp_path / "out.tsv"
    _run(["cmp", "-J" if weighted else "-H", "-k", str(K), "--outprefix", pre, "--cmpout", str(out)] + MEASURE_FLAGS[measure] + paths)
    _, _, vals = expected(X.exact_sets(batch), weighted, measure, paths)
    assert out.read_text() == textfmt.render_symmetric(paths, vals, False, opts_string(weighted, outprefix=pre))


@pytest.mark.parametrize("weighted", [False, True], ids=["set", "countdict"])
def test_phylip_binary_square_and_panel(inputs, tmp_path, weighted):
    paths, batch, _, _ = inputs
    pre = str(tmp_path / "pre")
    os.mkdir(pre)
    flag = "--countdict" if weighted else "--set"
    sets = X.exact_sets(batch)
    iszm, cards, vals = expected(sets, weighted, X.CONTAINMENT, paths)
    full = np.array([[X.measure_value(int(iszm[i, j]), cards[i], cards[j], X.CONTAINMENT, K) for j in range(4)] for i in range(4)], np.float32)
    common = [flag, "-k", str(K), "--outprefix", pre, "--containment"]
    _run(["sketch"] + common + ["--cmpout", str(tmp_path / "p.phy"), "--phylip"] + paths)                  # sketch --cmpout emits too
    assert (tmp_path / "p.phy").read_text() == textfmt.render_symmetric(paths, vals, True)
    _run(["cmp"] + common + ["--cmpout", str(tmp_path / "b.bin"), "--binary-output"] + paths)
    assert (tmp_path / "b.bin").read_bytes() == vals.tobytes()
    _run(["cmp"] + common + ["--cmpout", str(tmp_path / "sq.tsv"), "--square"] + paths, env={"D2G_CMP_SLOT_VALUES": "5"})       # several row batches
    assert (tmp_path / "sq.tsv").read_text() == textfmt.render_rect(paths, paths, full, "Asymmetric pairwise", opts_string(weighted, outprefix=pre))
    q = tmp_path / "q.txt"
    q.write_text("\n".join(paths[2:]) + "\n")
    _run(["cmp"] + common + ["--cmpout", str(tmp_path / "panel.tsv"), "-Q", str(q)] + paths[:2])
    assert (tmp_path / "panel.tsv").read_text() == textfmt.render_rect(paths, paths[:2], full[:2, 2:], "Panel (Query/Refernce)", opts_string(weighted, outprefix=pre))
    _run(["cmp"] + common + ["--cmpout", str(tmp_path / "ut.bin"), "--binary-output"] + paths, env={"D2G_CMP_SLOT_VALUES": "2", "D2G_GROUP_BYTES": "1"})
    assert (tmp_path / "ut.bin").read_bytes() == vals.tobytes()                                                # one input per batch, tiny row batches


def test_presketched_round_trip_and_the_card_on_load(inputs, tmp_path):
    """files written by --countdict (header: the sum of the counts), compared as --set from the same files (F16: |E| from the size) and
    as --countdict; then the key files rewritten by --set (header |E|) and --countdict --cache loading them with the old count files"""
    paths, batch, _, _ = inputs
    pre = str(tmp_path / "pre")
    os.mkdir(pre)
    sets = X.exact_sets(batch)
    kfs = [X.makedest(p, K, outprefix=pre) for p in paths]
    enames = ["E%d" % i for i in range(4)]
    _run(["sketch", "--countdict", "-k", str(K), "--outprefix", pre] + paths)
    for weighted in (False, True):
        _, _, vals = expected(sets, weighted, X.SIMILARITY, paths)
        out = tmp_path / ("pres%d.tsv" % weighted)
        _run(["cmp", "--presketched", "-k", str(K), "--cmpout", str(out)] + (["--countdict"] if weighted else []) + kfs)
        assert out.read_text() == textfmt.render_symmetric(enames, vals, False, opts_string(weighted))
    _, _, set_vals = expected(sets, False, X.UNION_SIZE, paths)
    _, _, cd_vals = expected(sets, True, X.UNION_SIZE, paths)
    assert not np.array_equal(set_vals, cd_vals)
    st = tmp_path / "st.json"
    _run(["cmp", "--set", "--cache", "-k", str(K), "--outprefix", pre, "--union-size", "--binary-output", "--cmpout", str(tmp_path / "c1.bin"), "--gpu-stats", str(st)] + paths)
    assert (tmp_path / "c1.bin").read_bytes() == set_vals.tobytes()                  # a --countdict key file picked up by --set
    j = json.loads(st.read_text())
    assert j["sketch"]["from_cache"] == 4 and j["sketch"]["sketched"] == 0
    assert j["cmp"]["resident_bytes"] > 8 * sum(len(k) for k, _ in sets) and j["cmp"]["devices"][0]["kset"]["launches"] >= 1
    _run(["sketch", "--set", "-k", str(K), "--outprefix", pre] + paths)              # without --cache: written again, header |E|
    assert open(kfs[1], "rb").read() == X.key_file_bytes(sets[1][0], sets[1][1], False)
    _run(["cmp", "--countdict", "--cache", "-k", str(K), "--outprefix", pre, "--union-size", "--binary-output", "--cmpout", str(tmp_path / "c2.bin"), "--gpu-stats", str(st)] + paths)
    assert (tmp_path / "c2.bin").read_bytes() == cd_vals.tobytes()                   # a --set key file picked up by --countdict
    assert json.loads(st.read_text())["sketch"]["from_cache"] == 4
    os.remove(X.counts_path(kfs[2]))                                                 # an incomplete file set is computed again
    _run(["cmp", "--countdict", "--cache", "-k", str(K), "--outprefix", pre, "--union-size", "--binary-output", "--cmpout", str(tmp_path / "c3.bin"), "--gpu-stats", str(st)] + paths)
    assert (tmp_path / "c3.bin").read_bytes() == cd_vals.tobytes() and json.loads(st.read_text())["sketch"]["from_cache"] == 3
    assert open(kfs[2], "rb").read() == X.key_file_bytes(sets[2][0], sets[2][1], True)


@pytest.mark.parametrize("weighted", [False, True], ids=["set", "countdict"])
def test_count_threshold_and_filterset(inputs, tmp_path, weighted):
    paths, batch, fpath, fkeys = inputs
    pre = str(tmp_path / "pre")
    os.mkdir(pre)
    flag = "--countdict" if weighted else "--set"
    sets = X.exact_sets(batch, 2.0)                                                 # -m 2 keeps count > 2 (counter.h:87)
    assert 0 < sum(len(k) for k, _ in sets) < sum(len(k) for k, _ in X.exact_sets(batch, 1.0))
    out = tmp_path / "m2.tsv"
    _run(["cmp", flag, "-m", "2", "-k", str(K), "--outprefix", pre, "--intersection", "--cmpout", str(out)] + paths)
    _, _, vals = expected(sets, weighted, X.INTERSECTION, paths)
    assert out.read_text() == textfmt.render_symmetric(paths, vals, False, opts_string(weighted, c=2, outprefix=pre))
    for p, (keys, counts) in zip(paths, sets):
        kf = X.makedest(p, K, count_threshold=2.0, outprefix=pre)
        assert ".ct_threshold2.FullMmerSet" in kf and open(kf, "rb").read() == X.key_file_bytes(keys, counts, weighted)
    fsets = []
    for keys, counts in X.exact_sets(batch):
        keep = ~np.isin(keys, fkeys)
        fsets.append((keys[keep], counts[keep]))
    pre2 = str(tmp_path / "pre2")
    os.mkdir(pre2)
    out = tmp_path / "f.bin"
    _run(["cmp", flag, "--filterset", fpath, "-k", str(K), "--outprefix", pre2, "--binary-output", "--cmpout", str(out)] + paths)
    _, _, vals = expected(fsets, weighted, X.SIMILARITY, paths)
    assert out.read_bytes() == vals.tobytes()
    assert open(X.makedest(paths[0], K, outprefix=pre2), "rb").read() == X.key_file_bytes(fsets[0][0], fsets[0][1], weighted)
