"""`dashing2 sketch -s / -N` (and `cmp` when it sketches) on a GPU: the files it writes, byte for byte against the reference writers of
oph_kmers_ref.py fed with its closed form.  Three small FASTA files, -k 11 -S 63 (m = 64: the last register of every sketch is dropped)."""
import json
import os
import subprocess

import numpy as np
import pytest

import k3_seam_cases as C
import oph_kmers_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
K, S = 11, 63


def _run(args, **kw):
    r = subprocess.run([EXE] + args, capture_output=True, timeout=120, **kw)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """-> (paths, genomes): a plain genome, one with a unit repeated three times (counts above 1) and a k-mer with its reverse
    complement, and a tiny one with fewer k-mers than registers"""
    rng = np.random.default_rng(1701)
    unit = C.random_bases(rng, 60)
    x = C.random_bases(rng, K)
    rc = x[::-1].translate(str.maketrans("ACGT", "TGCA"))
    genomes = [[C.random_bases(rng, 900)], [C.random_bases(rng, 300), unit, unit + x, unit, rc + C.random_bases(rng, 40)],
               [C.random_bases(rng, 30), "ACGT"]]
    d = tmp_path_factory.mktemp("kmers_fa")
    paths = []
    for i, g in enumerate(genomes):
        p = d / f"g{i}.fa"
        p.write_bytes(C.fasta(g, f"g{i}"))
        paths.append(str(p))
    return paths, genomes


@pytest.fixture(scope="module")
def want(inputs):
    paths, genomes = inputs
    e = R.expected_files(paths, genomes, S, K, K)                       # sketch: w_ = -1, written as k
    assert int(e["counts"].max()) >= 3 and (e["regs"][2] == R.M64).sum() > 30
    return e


def sketch(d, name, paths, *flags, cmd="sketch", env=None):
    out = d / name
    _run([cmd, "-k", str(K), "-S", str(S), "-o", str(out), "--gpu-stats", str(d / (name + ".json"))] + list(flags) + paths,
         env=dict(os.environ, **(env or {})))
    return out, json.loads((d / (name + ".json")).read_text())


def read(p):
    return open(str(p), "rb").read()


def third_column(out):
    lines = read(str(out) + ".names.txt").decode().split("\n")
    assert lines[0] == "#Name\tCardinality" and lines[-1] == ""
    return [l.split("\t")[2:] for l in lines[1:-1]]


def check_files(out, want):
    assert read(str(out) + ".kmer64") == want["kmer64"]
    assert read(str(out) + ".kmer64.names.txt") == want["names"]
    assert read(str(out) + ".kmercounts.f64") == want["kmercounts"]
    assert third_column(out) == [[c] for c in want["column"]]


def test_save_kmercounts_writes_the_reference_files(inputs, want, tmp_path):
    paths, _ = inputs
    plain, st0 = sketch(tmp_path, "plain", paths)
    out, st = sketch(tmp_path, "counted", paths, "-N")
    check_files(out, want)
    assert read(out) == read(plain)                                    # the sketches themselves do not change
    assert not any(os.path.exists(c) for c in want["column"])          # named, never written
    dev = st["sketch"]["devices"][0]
    assert dev["k1count"]["launches"] == dev["k1"]["launches"] >= 1
    assert "k1count" not in st0["sketch"]["devices"][0]
    assert third_column(plain) == [[], [], []] and not os.path.exists(str(plain) + ".kmer64")
    out2, _ = sketch(tmp_path, "counted_long", paths, "--save-kmercounts")
    check_files(out2, want)


def test_save_kmers_alone_writes_no_counts(inputs, want, tmp_path):
    paths, _ = inputs
    out, st = sketch(tmp_path, "ids", paths, "-s")
    assert read(str(out) + ".kmer64") == want["kmer64"] and read(str(out) + ".kmer64.names.txt") == want["names"]
    assert not os.path.exists(str(out) + ".kmercounts.f64")
    assert third_column(out) == [[], [], []]
    assert "k1count" not in st["sketch"]["devices"][0] and st["sketch"]["devices"][0]["k1"]["launches"] >= 1


def test_cmp_that_sketches_writes_them_too(inputs, want, tmp_path):
    """cmp carries w = 0 where sketch carries -1 (src/cmp_main.cpp:202): the header says 0 instead of k, nothing else differs"""
    paths, genomes = inputs
    out, st = sketch(tmp_path, "viacmp", paths, "-N", "--cmpout", str(tmp_path / "m.bin"), cmd="cmp")
    e = R.expected_files(paths, genomes, S, K, 0)
    assert e["kmer64"][24:] == want["kmer64"][24:] and e["kmer64"][:24] != want["kmer64"][:24]
    check_files(out, e)
    assert os.path.getsize(tmp_path / "m.bin") > 0
    assert st["sketch"]["devices"][0]["k1count"]["launches"] >= 1


def test_cache_with_save_kmercounts_sketches_again(inputs, want, tmp_path):
    paths, _ = inputs
    pre = str(tmp_path / "cache")
    os.mkdir(pre)
    for name in ("first", "second"):
        out, st = sketch(tmp_path, name, paths, "-N", "--cache", "--outprefix", pre)
        assert st["sketch"]["from_cache"] == 0 and st["sketch"]["sketched"] == 3
        assert st["sketch"]["devices"][0]["k1"]["launches"] >= 1 and st["sketch"]["devices"][0]["k1count"]["launches"] >= 1
        assert read(str(out) + ".kmer64") == want["kmer64"] and read(str(out) + ".kmercounts.f64") == want["kmercounts"]
    assert sorted(os.listdir(pre)) == sorted(os.path.basename(R.cache_name(p, S, K)) for p in paths)       # caches are still written
    _, st = sketch(tmp_path, "third", paths, "--cache", "--outprefix", pre)                                # ... and still read without -N
    assert st["sketch"]["from_cache"] == 3


def test_device_parsed_inputs_give_the_same_files(inputs, want, tmp_path):
    paths, _ = inputs
    out, st = sketch(tmp_path, "devparse", paths, "-N", env={"D2G_DEVICE_PARSE": "1"})
    assert st["sketch"]["groups_parsed_on_device"] >= 1
    check_files(out, want)


def test_without_an_output_file_nothing_is_written(inputs, tmp_path):
    paths, _ = inputs
    st = tmp_path / "st" / "s.json"
    os.mkdir(tmp_path / "st")
    os.mkdir(tmp_path / "cwd")
    before = sorted(os.listdir(os.path.dirname(paths[0])))
    _run(["sketch", "-k", str(K), "-S", str(S), "-N", "--gpu-stats", str(st)] + paths, cwd=str(tmp_path / "cwd"))
    assert os.listdir(tmp_path / "cwd") == [] and sorted(os.listdir(os.path.dirname(paths[0]))) == before
    dev = json.loads(st.read_text())["sketch"]["devices"][0]
    assert "k1count" not in dev and dev["k1"]["launches"] >= 1        # the count pass is skipped with nothing to write it to
