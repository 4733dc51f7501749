"""The host side of `cmp / sketch --parse-by-seq --edit-distance --compute-edit-distance` without a GPU: the raw record reader,
d2g_seqset_check and the recoding table in a stand-alone program under ASan + UBSan; what the CLI no longer refuses and every
combination it refuses by name before it asks for a GPU context; the usage text, the options line and the C ABI.  On the commit before
the flags existed the parser answers "option --edit-distance is outside the hot-path scope of this build" to all of them, and the library
lacks the names."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
SCOPE = "hot-path scope"
EDIT = ["--parse-by-seq", "--edit-distance", "--compute-edit-distance"]


def test_reader_check_and_recoding_under_the_sanitizers():
    csrc = os.path.join(ROOT, "dashing2_amd", "csrc")
    r = subprocess.run(["make", "-s", "-C", csrc, "../bin/edit_selftest_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "dashing2_amd", "bin", "edit_selftest_asan")], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "edit selftest OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def _cli(cmd, *args, env=None):
    e = dict(os.environ)
    for k in ("D2G_DEVICES", "D2G_DEVICE_PARSE", "D2G_HOST_PARSE"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([EXE, cmd, *args], capture_output=True, text=True, env=e)


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    p = tmp_path_factory.mktemp("edit_host") / "reads.fa"
    p.write_bytes(b">r1\nACGTACGT\n>r2\nACGTTCGT\n>r3\nacgt\n")
    return str(p)


@pytest.mark.parametrize("extra", [[], ["-k", "40", "-w", "50", "-S", "64", "-C"], ["--protein"], ["--square"], ["--phylip"], ["--binary-output"]],
                         ids=["plain", "kwSC", "protein", "square", "phylip", "binary"])
@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
def test_cli_no_longer_refuses_the_job(tmp_path, fasta, cmd, extra):
    """past the parser and the reading of the file the job asks for a GPU: without one it ends there, with one it runs"""
    r = _cli(cmd, *EDIT, *extra, "--cmpout", str(tmp_path / "o.tsv"), fasta)
    assert "outside" not in r.stderr and SCOPE not in r.stderr, r.stderr
    assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr
    if extra == ["--protein"]:
        assert r.stderr.count("the protein alphabet plays no part in an edit distance") == 1


REFUSALS = [
    (["--edit-distance"], None, ["no --parse-by-seq"]),
    (["--edit-distance", "--compute-edit-distance"], None, ["no --parse-by-seq"]),
    (["--parse-by-seq", "--edit-distance"], None, ["no --compute-edit-distance", "OrderMinHash"]),
    (["--parse-by-seq", "--compute-edit-distance"], None, ["--compute-edit-distance together with no --edit-distance"]),
    (["--compute-edit-distance"], None, ["--compute-edit-distance together with no --edit-distance"]),
    (EDIT + ["-o", "stack.bin"], None, ["-o/--outfile", "OrderMinHash registers"]),
    (EDIT + ["--cache"], None, ["--cache"]),
    (EDIT + ["-s", "-o", "x"], None, ["-o/--outfile"]),
    (EDIT + ["-s"], None, ["-s/--save-kmers or -N/--save-kmercounts"]),
    (EDIT + ["-N"], None, ["-s/--save-kmers or -N/--save-kmercounts"]),
    (EDIT + ["--multiset"], None, ["--multiset"]),
    (EDIT + ["--set"], None, ["--set/-H or --countdict/-J"]),
    (EDIT + ["--countdict"], None, ["--set/-H or --countdict/-J"]),
    (EDIT + ["-m", "2"], None, ["-m/--count-threshold"]),
    (EDIT + ["-c", "1000"], None, ["-c/--countsketch-size/--countmin-size"]),
    (EDIT + ["--filterset", "f.fa"], None, ["--filterset"]),
    (EDIT + ["--bed"], None, ["--bed"]),
    (EDIT + ["--fastcmp", "4"], None, ["--fastcmp/--regsize/--regbytes below 8"]),
    (EDIT + ["--fastcmp", "1"], None, ["--fastcmp/--regsize/--regbytes below 8"]),
    (EDIT + ["--mash-distance"], None, ["a second measure flag"]),
    (EDIT + ["--containment"], None, ["a second measure flag"]),
    (EDIT + ["--intersection"], None, ["a second measure flag"]),
    (EDIT, {"D2G_DEVICES": "0,1"}, ["D2G_DEVICES naming several GPUs"]),
    (EDIT, {"D2G_DEVICES": "all"}, ["D2G_DEVICES naming several GPUs"]),
]
IDS = ["alone", "nobyseq", "nocompute", "noedit", "computealone", "o", "cache", "s_o", "s", "N", "multiset", "set", "countdict", "m", "c", "filterset", "bed",
       "fastcmp4", "fastcmp1", "mash", "containment", "intersection", "devices01", "devicesall"]


@pytest.mark.parametrize("args,env,words", REFUSALS, ids=IDS)
@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
def test_cli_refuses_by_name_before_a_gpu_is_asked_for(tmp_path, fasta, cmd, args, env, words):
    r = _cli(cmd, *args, "--cmpout", str(tmp_path / "o.tsv"), fasta, env=env)
    assert r.returncode == 1 and SCOPE in r.stderr and "together with" in r.stderr, r.stderr
    assert all(w in r.stderr for w in words), r.stderr
    assert "gfx950" not in r.stderr and not os.path.exists(tmp_path / "o.tsv")


@pytest.mark.parametrize("args,words", [
    (["--presketched"], ["--presketched"]),
    (["-Q", "q.txt"], ["-Q/--qfile"]),
    (["--topk", "3"], ["--topk / --similarity-threshold"]),
    (["--similarity-threshold", "0.5"], ["--topk / --similarity-threshold"]),
    (["--greedy", "0.9"], ["--greedy"]),
], ids=["presketched", "Q", "topk", "threshold", "greedy"])
def test_cmp_only_combinations_are_refused_by_name(tmp_path, fasta, args, words):
    r = _cli("cmp", *EDIT, *args, "--cmpout", str(tmp_path / "o.tsv"), fasta)
    assert r.returncode == 1 and SCOPE in r.stderr and "--edit-distance together with" in r.stderr, r.stderr
    assert all(w in r.stderr for w in words), r.stderr
    assert "gfx950" not in r.stderr and not os.path.exists(tmp_path / "o.tsv")


def test_a_sketch_job_without_cmpout_is_refused(fasta):
    r = _cli("sketch", *EDIT, fasta)
    assert r.returncode == 1 and SCOPE in r.stderr and "a sketch job without --cmpout" in r.stderr and "gfx950" not in r.stderr, r.stderr


@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
def test_more_than_one_input_gives_the_parse_by_seq_message(tmp_path, fasta, cmd):
    r = _cli(cmd, *EDIT, "--cmpout", str(tmp_path / "o.tsv"), fasta, fasta)
    assert r.returncode == 1 and "parse-by-seq currently only handles one file at a time" in r.stderr and "gfx950" not in r.stderr, r.stderr


@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
def test_an_empty_record_is_refused_in_the_references_words_before_a_gpu_is_asked_for(tmp_path, cmd):
    p = tmp_path / "e.fa"
    p.write_bytes(b">a\nACGT\n>hollow\n>b\nAC\n")
    r = _cli(cmd, *EDIT, "--cmpout", str(tmp_path / "o.tsv"), str(p))
    assert r.returncode == 1 and f"EMPTY SEQ at idx 1 for hollow in path {p}" in r.stderr and "gfx950" not in r.stderr, r.stderr


@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
def test_a_record_above_the_cap_is_refused_with_its_name_before_a_gpu_is_asked_for(tmp_path, cmd):
    p = tmp_path / "long.fa"
    p.write_bytes(b">short\nACGT\n>giant some text\n" + b"ACGTACGT" * 8192 + b"\n")
    r = _cli(cmd, *EDIT, "--cmpout", str(tmp_path / "o.tsv"), str(p))
    assert r.returncode == 1 and SCOPE in r.stderr and "record giant of 65536 symbols" in r.stderr and "gfx950" not in r.stderr, r.stderr


def test_usage_names_the_flags():
    r = _cli("sketch", "-h")
    assert "--edit-distance --compute-edit-distance" in r.stderr and "Levenshtein" in r.stderr and "65535" in r.stderr


# ---------------------------------------------------------------- the library's host half through the ctypes mirror
def test_c_abi_exports_the_new_symbols(d2g):
    lib = d2g.lib()
    for name in ("d2g_seqrecs_create", "d2g_seqrecs_add_path", "d2g_seqrecs_add_fastx", "d2g_seqrecs_off", "d2g_seqset_check", "d2g_seqset_recode_map",
                 "d2g_seqset_create", "d2g_seqset_destroy", "d2g_seqset_device_bytes", "d2g_seqset_alphabet_size", "d2g_seqset_nrecords",
                 "d2g_edit_ut_dev", "d2g_edit_rect_dev", "d2g_edit_ut", "d2g_edit_rect"):
        assert getattr(lib, name) is not None
    assert d2g.EDIT_MAX_LEN == 65535 and d2g.TIME_EDIT == 2048


def test_reader_keeps_raw_bytes_with_the_seqpack_readers_names(d2g, tmp_path):
    fq = b"@q1 desc\nACGTNNacgt\n+\nIIIIIIIIII\n@q2\nGG\n+\nII\n>f3\nTT\nTT\n"
    sr, sp = d2g.SeqRecs(), d2g.SeqPack(4)
    sr.add_fastx(fq)
    sp.add_fastx_by_record(fq)
    assert sr.nrecords == sp.ngenomes == 3
    assert [sr.name(i) for i in range(3)] == [sp.name(i) for i in range(3)] == ["q1", "q2", "f3"]
    assert sr.records() == [b"ACGTNNacgt", b"GG", b"TTTT"]
    import gzip
    p = tmp_path / "x.fq.gz"
    p.write_bytes(gzip.compress(fq))
    sr2 = d2g.SeqRecs()
    sr2.add_path(str(p))
    assert sr2.records() == sr.records()
    data, off = sr.arrays()
    d2g.seqset_check(data, off)


def test_seqset_check_and_recode_map(d2g):
    data = np.frombuffer(b"ACGTacgt", np.uint8)
    d2g.seqset_check(data, np.array([0, 4, 4, 8], np.uint64))
    for off, word in [([1, 8], "begin at 0"), ([0, 5, 3, 8], "decreases"), ([0, 4, 7], "ends at 7")]:
        with pytest.raises(d2g.D2GError, match=word) as e:
            d2g.seqset_check(data, np.array(off, np.uint64))
        assert e.value.status == -1
    big = np.full(65536, 65, np.uint8)
    with pytest.raises(d2g.D2GError, match="65536") as e:
        d2g.seqset_check(big, np.array([0, 65536], np.uint64))
    assert e.value.status == -5
    d2g.seqset_check(big[:-1], np.array([0, 65535], np.uint64))
    m, sigma = d2g.seqset_recode_map(data)
    assert sigma == 8 and [int(m[c]) for c in b"ACGTacgt"] == list(range(8))
    m, sigma = d2g.seqset_recode_map(np.array([255, 0], np.uint8))
    assert sigma == 2 and m[0] == 0 and m[255] == 1
