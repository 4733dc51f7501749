"""The host side of `sketch / cmp --bed` without a GPU: d2g_xxh3_64, the line parser, the launch plan of K1i and the --multiset sweep in
a stand-alone program under ASan + UBSan; what the CLI no longer refuses and what it refuses before it asks for a GPU context; the
usage text, the options line and the C ABI.  On the commit before the flag existed test_cli_no_longer_refuses_bed fails with the
parser's "option --bed is outside the hot-path scope of this build", the refusals are never reached, the library lacks the names."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
SCOPE = "hot-path scope"


def test_xxh3_parser_plan_and_sweep_under_the_sanitizers():
    csrc = os.path.join(ROOT, "dashing2_amd", "csrc")
    r = subprocess.run(["make", "-s", "-C", csrc, "../bin/bed_selftest_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "dashing2_amd", "bin", "bed_selftest_asan"), os.path.join(GOLDEN, "xxh3_names.json")],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "bed selftest OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def _cli(cmd, *args, env=None):
    e = dict(os.environ)
    for k in ("D2G_DEVICES", "D2G_DEVICE_PARSE", "D2G_HOST_PARSE"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([EXE, cmd, *args], capture_output=True, text=True, env=e)


@pytest.fixture(scope="module")
def bed(tmp_path_factory):
    p = tmp_path_factory.mktemp("bed_host") / "x.bed"
    p.write_bytes(b"#peaks\nchr1\t5\t100\nchr2\t7\t12\n")
    return str(p)


@pytest.mark.parametrize("extra", [[], ["--multiset"], ["--multiset", "--normalize-intervals"], ["-m", "3"], ["-k", "31", "-w", "40", "-C"]],
                         ids=["set", "multiset", "normalize", "m", "kwC"])
@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
def test_cli_no_longer_refuses_bed(tmp_path, bed, cmd, extra):
    """past the option parser the job asks for a GPU: without one it ends there, with one it runs -- neither way is --bed out of scope"""
    r = _cli(cmd, "--bed", *extra, "-S", "64", "--outprefix", str(tmp_path), "--cmpout", str(tmp_path / "o.tsv"), bed, bed)
    assert "outside" not in r.stderr and SCOPE not in r.stderr, r.stderr
    assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr
    if extra == ["-m", "3"]:
        assert r.stderr.count("-m/--count-threshold has no effect with --bed") == 1


@pytest.mark.parametrize("args,env,words", [
    (["--parse-by-seq"], None, ["--parse-by-seq"]),
    (["-s", "-o", "x"], None, ["-s/--save-kmers or -N/--save-kmercounts"]),
    (["-N", "-o", "x"], None, ["-s/--save-kmers or -N/--save-kmercounts"]),
    (["--set"], None, ["--set/-H or --countdict/-J"]),
    (["--countdict"], None, ["--set/-H or --countdict/-J"]),
    (["--filterset", "f.fa"], None, ["--filterset"]),
    (["--multiset", "-c", "100"], None, ["-c/--countsketch-size/--countmin-size", "signed cells"]),
    (["--protein"], None, ["a protein alphabet"]),
    (["--protein14"], None, ["a protein alphabet"]),
    (["--protein8"], None, ["a protein alphabet"]),
    (["--protein6"], None, ["a protein alphabet"]),
    ([], {"D2G_DEVICES": "0,1"}, ["D2G_DEVICES naming several GPUs"]),
    ([], {"D2G_DEVICES": "all"}, ["D2G_DEVICES naming several GPUs"]),
], ids=["byseq", "s", "N", "set", "countdict", "filterset", "c", "protein", "protein14", "protein8", "protein6", "devices01", "devicesall"])
@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
def test_cli_refuses_before_a_gpu_is_asked_for(tmp_path, bed, cmd, args, env, words):
    r = _cli(cmd, "--bed", *args, "-S", "64", "--outprefix", str(tmp_path), "--cmpout", str(tmp_path / "o.tsv"), bed, env=env)
    assert r.returncode == 1 and SCOPE in r.stderr and "--bed together with" in r.stderr, r.stderr
    assert all(w in r.stderr for w in words), r.stderr
    assert "gfx950" not in r.stderr and not os.path.exists(tmp_path / "o.tsv")


@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
def test_normalize_intervals_in_set_space_is_refused_in_the_references_words(tmp_path, bed, cmd):
    r = _cli(cmd, "--bed", "--normalize-intervals", "-S", "64", "--outprefix", str(tmp_path), bed)
    assert r.returncode == 1 and "Can't normalize BED rows in set space. Use SPACE_MULTISET or SPACE_PSET" in r.stderr, r.stderr
    assert "gfx950" not in r.stderr


def test_device_parse_is_ignored_with_one_line(tmp_path, bed):
    r = _cli("sketch", "--bed", "-S", "64", "--outprefix", str(tmp_path), bed, env={"D2G_DEVICE_PARSE": "1"})
    assert r.stderr.count("D2G_DEVICE_PARSE ignored with --bed") == 1 and SCOPE not in r.stderr, r.stderr


@pytest.mark.parametrize("flag", ["--bigwig", "--leafcutter", "--by-chrom"])
def test_the_other_interval_inputs_stay_refused(bed, flag):
    r = _cli("sketch", flag, bed)
    assert r.returncode == 1 and f"option {flag} is outside the hot-path scope" in r.stderr and "gfx950" not in r.stderr, r.stderr


def test_usage_names_the_flags():
    r = _cli("sketch", "-h")
    assert "--bed" in r.stderr and "--normalize-intervals" in r.stderr and "XXH3_64bits" in r.stderr and ".opss" in r.stderr


def test_c_abi_exports_the_new_symbols(d2g):
    lib = d2g.lib()
    for name in ("d2g_xxh3_64", "d2g_bed_parse", "d2g_interval_plan_create", "d2g_interval_plan_destroy", "d2g_interval_plan_npositions",
                 "d2g_interval_oph_sketch", "d2g_interval_oph_sketch_dev", "d2g_interval_bmh_sketch", "d2g_interval_runs"):
        assert getattr(lib, name) is not None
