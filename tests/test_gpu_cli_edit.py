"""`dashing2 cmp / sketch --cmpout` with --parse-by-seq --edit-distance --compute-edit-distance, end to end on the GPU: the TSV triangle,
--square, --phylip and --binary-output of a 30-record FASTA and a gzipped FASTQ, byte for byte against the text the reference's writer
gives for edit_ref's distances (oracle.textfmt); the options line and the names; the reference's exit on an empty record; a record above
the cap; the --gpu-stats keys.  A binary matrix is the flat float32 array the reference's python/parse.py:173-177 (parse_binary_distmat)
maps; that file cannot travel to the GPU machine, so np.fromfile stands for it."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import edit_ref as E
from conftest import ROOT
from oracle import textfmt

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
EDIT = ["--parse-by-seq", "--edit-distance", "--compute-edit-distance"]
OPTIONS = "Dashing2Options;k:32;parsebyseq;trimchr;sketchsize:1024;sketchtype:orderminhash;Fastx;canon"


def _cli(args, env=None):
    e = dict(os.environ)
    e.pop("D2G_DEVICES", None)
    e.update(env or {})
    return subprocess.run([EXE] + args, capture_output=True, timeout=120, env=e)


def _run(args, env=None):
    r = _cli(args, env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """30 records, 1 .. 400 symbols, mixed case and N; the same records as FASTA (60-column lines) and as gzipped FASTQ"""
    rng = np.random.default_rng(7400)
    alphabet = np.frombuffer(b"ACGTacgtN", np.uint8)
    base = bytes(rng.choice(alphabet[:4], 400).tolist())
    recs = []
    for i in range(30):
        n = int(rng.integers(1, 401)) if i else 1
        x = bytearray(base[:n])
        for _ in range(n // 15):
            x[int(rng.integers(n))] = int(rng.choice(alphabet))
        recs.append(bytes(x))
    names = [f"read{i}" for i in range(30)]
    d = tmp_path_factory.mktemp("edit_cli")
    fa = b"".join(b">%s some description\n" % n.encode() + b"".join(r[k:k + 60] + b"\n" for k in range(0, len(r), 60)) for n, r in zip(names, recs))
    fq = b"".join(b"@%s\n%s\n+\n%s\n" % (n.encode(), r, b"I" * len(r)) for n, r in zip(names, recs))
    (d / "reads.fa").write_bytes(fa)
    (d / "reads.fq.gz").write_bytes(gzip.compress(fq))
    return {"fa": str(d / "reads.fa"), "fq": str(d / "reads.fq.gz"), "names": names, "want": E.edit_matrix(recs)}


@pytest.mark.parametrize("cmd", ["cmp", "sketch"])
@pytest.mark.parametrize("kind", ["fa", "fq"])
def test_triangle_square_phylip_and_binary(tmp_path, reads, cmd, kind):
    want, names = reads["want"], reads["names"]
    tri = E.triangle(want).astype(np.float32)
    out = tmp_path / "o"
    r = _run([cmd] + EDIT + ["--cmpout", str(out), reads[kind]])
    assert out.read_text() == textfmt.render_symmetric(names, tri, False, OPTIONS)
    assert b"OMH sketching" not in r.stderr and b"Edit distance LSH" not in r.stderr
    _run([cmd] + EDIT + ["--square", "--cmpout", str(out), reads[kind]])
    assert out.read_text() == textfmt.render_rect(names, names, want.astype(np.float32), "Asymmetric pairwise", OPTIONS)
    _run([cmd] + EDIT + ["--phylip", "--cmpout", str(out), reads[kind]])
    assert out.read_text() == textfmt.render_symmetric(names, tri, True)
    _run([cmd] + EDIT + ["--binary-output", "--cmpout", str(out), reads[kind]])
    np.testing.assert_array_equal(np.fromfile(out, np.float32), tri)
    _run([cmd] + EDIT + ["--binary-output", "--square", "--cmpout", str(out), reads[kind]])
    np.testing.assert_array_equal(np.fromfile(out, np.float32).reshape(30, 30), want.astype(np.float32))


def test_small_row_batches_and_the_flags_that_play_no_part(tmp_path, reads):
    """D2G_CMP_SLOT_VALUES: many row batches; -k, -w, -S, -C and a protein flag only show in the options line"""
    want, names = reads["want"], reads["names"]
    out = tmp_path / "o"
    _run(["cmp"] + EDIT + ["--cmpout", str(out), reads["fa"]], env={"D2G_CMP_SLOT_VALUES": "40"})
    assert out.read_text() == textfmt.render_symmetric(names, E.triangle(want).astype(np.float32), False, OPTIONS)
    _run(["cmp"] + EDIT + ["--square", "--binary-output", "--cmpout", str(out), reads["fa"]], env={"D2G_CMP_SLOT_VALUES": "70"})
    np.testing.assert_array_equal(np.fromfile(out, np.float32).reshape(30, 30), want.astype(np.float32))
    r = _run(["cmp"] + EDIT + ["-k", "40", "-S", "64", "-C", "--protein", "--cmpout", str(out), reads["fa"]])
    opts = "Dashing2Options;k:40;parsebyseq;trimchr;sketchsize:64;sketchtype:orderminhash;Fastx"
    assert out.read_text() == textfmt.render_symmetric(names, E.triangle(want).astype(np.float32), False, opts)
    assert r.stderr.count(b"the protein alphabet plays no part in an edit distance") == 1


def test_an_empty_record_ends_the_job_in_the_references_words(tmp_path):
    p = tmp_path / "e.fa"
    p.write_bytes(b">a\nACGT\n>b\nAC\n>hollow\n")
    r = _cli(["cmp"] + EDIT + ["--cmpout", str(tmp_path / "o"), str(p)])
    assert r.returncode == 1 and f"EMPTY SEQ at idx 2 for hollow in path {p}".encode() in r.stderr


def test_a_record_above_the_cap_is_refused_with_its_name_and_one_at_the_cap_runs(tmp_path):
    p = tmp_path / "long.fa"
    body = b"ACGTTGCA" * 8192
    p.write_bytes(b">short\nACGT\n>giant\n" + body + b"\n")
    r = _cli(["cmp"] + EDIT + ["--cmpout", str(tmp_path / "o"), str(p)])
    assert r.returncode == 1 and b"record giant of 65536 symbols" in r.stderr and b"hot-path scope" in r.stderr
    p.write_bytes(b">short\nACGT\n>giant\n" + body[:-1] + b"\n")
    _run(["cmp"] + EDIT + ["--binary-output", "--cmpout", str(tmp_path / "o"), str(p)])
    assert np.fromfile(tmp_path / "o", np.float32).tolist() == [65531.0]              # ACGT is a subsequence: only insertions


def test_gpu_stats_keys(tmp_path, reads):
    st = tmp_path / "stats.json"
    _run(["cmp"] + EDIT + ["--cmpout", str(tmp_path / "o"), "--gpu-stats", str(st), reads["fa"]])
    j = json.loads(st.read_text())
    assert j["command"] == "cmp" and "context" in j and "in_process_s" in j
    e = j["cmp"]["edit"]
    assert set(e) == {"records", "symbols", "alphabet", "cells", "batches", "resident_bytes"}
    assert e["records"] == 30 and e["alphabet"] == 9 and e["batches"] == 1 and e["resident_bytes"] > e["symbols"] > 30
    dev = j["cmp"]["devices"][0]
    assert dev["edit"]["launches"] == 1 and dev["editprep"]["launches"] == 1 and dev["edit"]["total_ms"] > 0
    # cells = the sum of m_i n_j over the pairs computed
    recs_len = _lengths(reads["fa"])
    want_cells = sum(recs_len[i] * recs_len[k] for i in range(30) for k in range(i + 1, 30))
    assert e["cells"] == want_cells and e["symbols"] == sum(recs_len)


def _lengths(fa):
    lens, cur = [], None
    for line in open(fa, "rb").read().split(b"\n"):
        if line.startswith(b">"):
            if cur is not None:
                lens.append(cur)
            cur = 0
        elif cur is not None:
            cur += len(line)
    lens.append(cur)
    return lens
