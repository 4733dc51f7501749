"""The host side of windowed minimizers (-w > k), without a GPU: the windowed launch plan, the walker's register queue and the .w<w>
file names in a stand-alone program under ASan + UBSan; the emission count through the library; what the CLI still refuses, and no
longer refuses, before it asks for a GPU context (`contain` over a database of minimizers stays refused: tests/test_contain_host.py)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
SCOPE = "hot-path scope"
OLD_REFUSAL = "windowed minimizers"


def test_plan_queue_and_names_under_the_sanitizers():
    csrc = os.path.join(ROOT, "dashing2_amd", "csrc")
    r = subprocess.run(["make", "-s", "-C", csrc, "../bin/window_selftest_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "dashing2_amd", "bin", "window_selftest_asan")], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "window selftest OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def test_run_emissions_counts_window_positions(d2g):
    for k, w in [(21, 30), (5, 7), (32, 33), (15, 1038)]:
        for length in (0, k - 1, k, w - 1, w, w + 1, w + 63, w + 64, 70000):
            assert d2g.run_emissions(length, k, w) == max(0, length - w + 1)
            for off in (0, 1, k - 1, k):                                   # no window: every k-mer
                assert d2g.run_emissions(length, k, off) == max(0, length - k + 1)
    assert d2g.run_emissions(100, 21) == 80


def _cli(cmd, *args):
    e = dict(os.environ)
    e.pop("D2G_DEVICES", None)
    return subprocess.run([EXE, cmd, *args], capture_output=True, text=True, env=e)


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    p = tmp_path_factory.mktemp("win_host") / "g.fa"
    rng = np.random.default_rng(3)
    p.write_bytes(b">g\n" + bytes(b"ACGT"[i] for i in rng.integers(0, 4, 400)) + b"\n")
    return str(p)


@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
def test_cli_no_longer_refuses_a_window(tmp_path, fasta, cmd):
    """past the option parser the job asks for a GPU: without one it ends there, with one it runs -- neither way is -w out of scope"""
    r = _cli(cmd, "-k", "21", "-w", "30", "-S", "64", "-o", str(tmp_path / "o.bin"), fasta)
    assert OLD_REFUSAL not in r.stderr and SCOPE not in r.stderr, r.stderr
    assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr


def test_usage_mentions_the_window():
    r = _cli("sketch", "-h")
    assert "-w/--window-size" in r.stderr and "minimizer" in r.stderr


@pytest.mark.parametrize("args,words", [
    (["-k", "21", "-w", "30", "--entmin"], ["entmin"]),
    (["-k", "21", "-w", "30", "--spacing", "1"], ["spacing"]),
    (["-k", "33", "-w", "40"], ["k = 33 > 32"]),
    (["-k", "21", "-w", str(21 + 4096)], ["4096 k-mers"]),
], ids=["entmin", "spacing", "k33", "cap"])
def test_cli_still_refuses_before_a_gpu_is_asked_for(tmp_path, fasta, args, words):
    r = _cli("sketch", *args, "-S", "64", "-o", str(tmp_path / "o.bin"), fasta)
    assert r.returncode == 1 and SCOPE in r.stderr and all(w in r.stderr for w in words), r.stderr
    assert "gfx950" not in r.stderr and not os.path.exists(tmp_path / "o.bin")


def test_cap_is_the_widest_window_the_parser_lets_through(tmp_path, fasta):
    r = _cli("sketch", "-k", "21", "-w", str(21 + 4095), "-S", "64", "-o", str(tmp_path / "o.bin"), fasta)
    assert SCOPE not in r.stderr and (r.returncode == 0 or "gfx950" in r.stderr), r.stderr


def _write_db(path, k, w, S=4, nrefs=2):
    keys = np.arange(1, nrefs * S + 1, dtype=np.uint64).reshape(nrefs, S)
    hdr = np.array([0 | 1 << 8, S, k, w], np.uint32).tobytes() + np.array([0], np.uint64).tobytes()
    with open(path, "wb") as f:
        f.write(hdr + keys.tobytes())
    with open(str(path) + ".names.txt", "w") as f:
        f.write("a\nb\n")
    return str(path)


@pytest.mark.parametrize("w", [0, 5, 21])
def test_contain_takes_a_header_without_a_window(tmp_path, fasta, w):
    """header w <= k, 0 included: every k-mer -- no longer out of scope.  A database of minimizers (w > k) stays refused by the command
    (tests/test_contain_host.py holds that); the library screens them (tests/test_gpu_minimizers.py::test_screen)"""
    r = _cli("contain", _write_db(tmp_path / "db.kmer64", 21, w), fasta)
    assert OLD_REFUSAL not in r.stderr and SCOPE not in r.stderr and (r.returncode == 0 or "gfx950" in r.stderr), r.stderr
