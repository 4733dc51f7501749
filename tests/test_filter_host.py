"""--filterset on the command line, as far as it goes without a GPU: the flag is in scope for `sketch` and `cmp`, its argument is
parsed as Dashing2Options::filterset parses it (reference src/d2.cpp:45-49), the binary-k-mer-file arm is refused before a
context is asked for, the usage texts name it, and `cmp --presketched` ignores it.  What a filtered sketch holds is
tests/test_gpu_filter.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _cli(*args):
    exe = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("filter_cli")
    g, f = d / "x.fa", d / "f.fa"
    g.write_text(">r\nACGTTGCATGCAGTCGATCGATCGTAGCTAGCTAGCATCGATCAGCTAGCATCG\n")
    f.write_text(">adapter\nGATCGATCGTAGCTAGCTAGCATCGATC\n")
    return str(g), str(f)


@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
@pytest.mark.parametrize("suffix", ["", ":K", ":k", ":Kmers", ":k=21"])
def test_cli_accepts_filterset(files, cmd, suffix):
    """in scope: no refusal; without a GPU it stops where every compute entry point does, at the creation of the context.  A suffix
    after the last ':' that begins with K or k selects the sequence arm, whatever else it says"""
    g, f = files
    r = _cli(cmd, "-k", "21", "--filterset", f + suffix, g)
    assert "outside the hot-path scope" not in r.stderr, r.stderr
    assert "not found in expected set" not in r.stderr and "Failed to open" not in r.stderr, r.stderr
    assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr


@pytest.mark.parametrize("cmd", ["sketch", "cmp"])
@pytest.mark.parametrize("arg", ["f.bin:x", "f.bin:", "kmers.u64:B", "a:K:b"])
def test_cli_refuses_binary_kmer_files(files, cmd, arg):
    r = _cli(cmd, "--filterset", arg, files[0])
    assert r.returncode == 1, r.stderr
    assert "outside the hot-path scope" in r.stderr and "--filterset" in r.stderr and arg in r.stderr, r.stderr
    assert "gfx950" not in r.stderr                                    # refused before a context was asked for


def test_usage_names_the_flag():
    for cmd in ("sketch", "cmp"):
        assert "--filterset" in _cli(cmd, "-h").stderr


def test_cmp_presketched_ignores_filterset(tmp_path):
    p = tmp_path / "stack.bin"
    p.write_bytes(np.array([2, 4], np.uint64).tobytes() + np.ones(2).tobytes() + np.arange(8, dtype=np.float64).tobytes())
    for arg in ("/nonexistent/f.fa", "f.bin:x"):                       # nothing is sketched there: not even looked at
        r = _cli("cmp", "--presketched", "--filterset", arg, str(p))
        assert "outside the hot-path scope" not in r.stderr and "Failed to open" not in r.stderr, r.stderr
        assert "FilterSet" not in r.stdout
        assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr
