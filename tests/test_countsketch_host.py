"""The host side of `--multiset -c/--countsketch-size/--countmin-size <cells>` without a GPU: the remainder by reciprocal, the table
groups and the workgroup tables of BagMinHash over lists in a stand-alone program under ASan + UBSan; what the CLI no longer refuses
and what it refuses before it asks for a GPU context; the usage text; the C ABI.  On the commit before the flag existed
test_cli_no_longer_refuses_the_count_sketch fails with the parser's "option -c is outside the hot-path scope of this build" (the long
forms: "option --countsketch-size is outside ..."), the refusals are never reached, the usage text and the library lack the names."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
SCOPE = "hot-path scope"
OLD_REFUSAL = "outside"


def test_remainder_groups_and_block_tables_under_the_sanitizers():
    csrc = os.path.join(ROOT, "dashing2_amd", "csrc")
    r = subprocess.run(["make", "-s", "-C", csrc, "../bin/countsketch_selftest_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "dashing2_amd", "bin", "countsketch_selftest_asan")], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "countsketch selftest OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def _cli(cmd, *args, env=None):
    e = dict(os.environ)
    e.pop("D2G_DEVICES", None)
    e.update(env or {})
    return subprocess.run([EXE, cmd, *args], capture_output=True, text=True, env=e)


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    p = tmp_path_factory.mktemp("cs_host") / "x.fa"
    rng = np.random.default_rng(5)
    p.write_bytes(b">x\n" + bytes(b"ACGT"[i] for i in rng.integers(0, 4, 400)) + b"\n")
    return str(p)


@pytest.mark.parametrize("flag", ["-c", "--countsketch-size", "--countmin-size"])
@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
def test_cli_no_longer_refuses_the_count_sketch(tmp_path, fasta, cmd, flag):
    """past the option parser the job asks for a GPU: without one it ends there, with one it runs -- neither way is -c out of scope"""
    r = _cli(cmd, "--multiset", flag, "1000", "-S", "64", "-k", "21", "-o", str(tmp_path / "o.bin"), fasta)
    assert OLD_REFUSAL not in r.stderr and SCOPE not in r.stderr, r.stderr
    assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr


def test_set_space_and_the_largest_table_pass_the_parser(tmp_path, fasta):
    for args in (["-c", "1000"], ["--multiset", "-c", str(1 << 31)], ["--multiset", "-c", "0"]):
        r = _cli("sketch", *args, "-S", "64", "-k", "21", "-o", str(tmp_path / "o.bin"), fasta)
        assert SCOPE not in r.stderr and (r.returncode == 0 or "gfx950" in r.stderr), r.stderr


@pytest.mark.parametrize("args,env,words", [
    (["-c", "100", "--set"], None, ["--set/-H or --countdict/-J", "maskfn(cell)"]),
    (["-c", "100", "--countdict"], None, ["--set/-H or --countdict/-J"]),
    (["--multiset", "-c", "100", "--parse-by-seq"], None, ["--parse-by-seq", "table per record"]),
    (["--multiset", "--countsketch-size", "100"], {"D2G_DEVICES": "0,1"}, ["D2G_DEVICES naming several GPUs"]),
    (["--multiset", "--countmin-size", "100"], {"D2G_DEVICES": "all"}, ["D2G_DEVICES naming several GPUs"]),
    (["--multiset", "-c", str((1 << 31) + 1)], None, ["more than 2^31 cells"]),
], ids=["set", "countdict", "byseq", "devices01", "devicesall", "cells"])
def test_cli_refuses_before_a_gpu_is_asked_for(tmp_path, fasta, args, env, words):
    r = _cli("sketch", *args, "-S", "64", "-k", "21", "--cmpout", str(tmp_path / "o.tsv"), fasta, env=env)
    assert r.returncode == 1 and SCOPE in r.stderr and "-c/--countsketch-size/--countmin-size" in r.stderr, r.stderr
    assert all(w in r.stderr for w in words), r.stderr
    assert "gfx950" not in r.stderr and not os.path.exists(tmp_path / "o.tsv")


def test_usage_names_the_flag():
    r = _cli("sketch", "-h")
    assert "-c/--countsketch-size/--countmin-size" in r.stderr and "fixed memory usage" in r.stderr and "CountMinCounting" in r.stderr


def test_c_abi_exports_the_new_symbols(d2g):
    lib = d2g.lib()
    for name in ("d2g_bmh_sketch_cs", "d2g_bmh_sketch_cs_dev", "d2g_sketcher_run_bmh_cs", "d2g_countsketch_table", "d2g_countsketch_cells",
                 "d2g_countsketch_lds_cells", "d2g_countsketch_stats"):
        assert getattr(lib, name) is not None
    L = d2g.countsketch_lds_cells()
    assert 1 <= L <= 40960                                                # a row of L int32 cells fits the 160 KiB of LDS
