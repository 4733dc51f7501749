"""sketch -s / -N, the parts that need no GPU: the host half of the C ABI (d2g_wang_hash_inverse, d2g_oph_kmer_ids), the .kmer64
writer against what the reference's own reader reads back (tests/golden/kmer64_small.*), and the CLI's parsing and refusals, which
happen before a GPU context exists."""
import json
import os
import subprocess

import numpy as np
import pytest

import oph_kmers_ref as R
from conftest import GOLDEN, ROOT

M64 = R.M64
KATS = [133348, 0, 1, 2 ** 64 - 1, 0x724526e320f9967d, 0xdeadbeefcafebabe]      # test_oracle.py's values


def test_wang_hash_inverse_inverts_wang_hash(d2g, oracle):
    rng = np.random.default_rng(3)
    for x in KATS + [int(v) for v in rng.integers(0, 1 << 63, 500, dtype=np.uint64) * np.uint64(2) + np.uint64(1)]:
        assert d2g.wang_hash_inverse(d2g.wang_hash(x)) == x
        assert d2g.wang_hash(d2g.wang_hash_inverse(x)) == x
        assert d2g.wang_hash_inverse(x) == oracle.wang_inverse(x)
    assert d2g.wang_hash_inverse(0x77cfa1eef01bca90) == 0 and d2g.wang_hash_inverse(0x1f89206e3f8ec794) == M64
    assert d2g.oph_xor_const() == R.OPHXOR


@pytest.mark.parametrize("S", [1, 2, 5, 63, 64, 1000])
def test_oph_kmer_ids_equals_decode(d2g, S):
    """the first S of every m: an odd S drops the last register of every sketch; ~0 and 0 decode like any other value"""
    m, n = d2g.oph_m(S), 4
    rng = np.random.default_rng(S)
    regs = rng.integers(0, 1 << 63, (n, m), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, m), dtype=np.uint64)
    regs[1] = M64                                                       # an empty sketch
    regs[2, 0], regs[2, m - 1] = 0, M64
    ids = d2g.oph_kmer_ids(regs, S)
    assert ids.shape == (n, S) and np.array_equal(ids, R.decode(regs)[:, :S])
    assert int(ids[1, 0]) == (d2g.wang_hash_inverse(M64) ^ R.OPHXOR)
    for i, r in ((0, 0), (3, S - 1)):                                   # the id of the decoded k-mer is the register
        assert d2g.wang_hash(int(ids[i, r]) ^ d2g.oph_xor_const()) == int(regs[i, r])
    assert d2g.oph_kmer_ids(np.zeros((0, m), np.uint64), S).shape == (0, S)


def test_kmer64_writer_against_what_the_reference_reader_read():
    """kmer64_small.bin was read by the reference's parse_binary_kmers when the fixture was made (make_kmer64_golden.py); the writer
    of oph_kmers_ref.py, fed with the closed form of the same genomes, gives that file byte for byte, and its fields are the JSON's.
    This pins the PYTHON writer, the reference of the tests; the CLI's own writer (write_kmer_files, sketch_cmd.cpp) needs a GPU to
    have anything to write and is held to this Python writer byte for byte in test_gpu_cli_kmers.py"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_kmer64_golden", os.path.join(GOLDEN, "make_kmer64_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    want = json.load(open(os.path.join(GOLDEN, "kmer64_small.json")))
    blob = open(os.path.join(GOLDEN, "kmer64_small.bin"), "rb").read()
    exp = R.expected_files(["g%d.fa" % i for i in range(len(G.GENOME_LENS))], G.genomes(), G.S, G.K, G.W, G.CANON, G.SEED)
    assert exp["kmer64"] == blob
    d, s, k, w = np.frombuffer(blob[:16], np.uint32).tolist()
    assert (k, w, bool((d >> 8) & 1), d & 0xFF, s) == (want["k"], want["w"], want["canon"], 0, want["sketchsize"]) and want["alphabet"] == "DNA"
    assert int(np.frombuffer(blob[16:24], np.uint64)[0]) == want["seed"]
    kmers = np.frombuffer(blob[24:], np.uint64).reshape(-1, s)
    assert list(kmers.shape) == want["shape"] and kmers[0].tolist() == want["first_row"]
    # and the k-mers are k-mers: every decoded id of a non-empty register is maskfn of a k-mer of its genome (xormask 0: wang64)
    import k3_seam_cases as C
    for i, g in enumerate(G.genomes()):
        have = set(R.wang64_int(x) for x in C.kmers_of(g, G.K, G.CANON))
        for r in range(s):
            if exp["regs"][i, r] != M64:
                assert int(kmers[i, r]) in have


# ---- the CLI ------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    exe = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    p = tmp_path_factory.mktemp("kmers_cli") / "x.fa"
    p.write_text(">r\nACGTTGCATGCAGTCGATCGATCGTAGCTAGCTAGCATCGATCAGCTAGCATCG\n")
    return str(p)


@pytest.mark.parametrize("args", [["sketch", "-s"], ["sketch", "-N"], ["sketch", "--save-kmers"], ["cmp", "--save-kmercounts"],
                                  ["cmp", "-N"], ["cmp", "-s"]])
def test_cli_accepts_save_kmers(fasta, args):
    """in scope: no refusal; without a GPU it stops later, where every compute entry point does, at the creation of the context"""
    r = _cli(*args, fasta)
    assert "outside the hot-path scope" not in r.stderr, r.stderr
    assert "not found in expected set" not in r.stderr
    assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr


@pytest.mark.parametrize("args,flag,other", [
    (["sketch", "-N", "--multiset"], "--save-kmercounts", "--multiset"), (["sketch", "-s", "--parse-by-seq"], "--save-kmers", "--parse-by-seq"),
    (["sketch", "-s", "-B"], "--save-kmers", "--multiset"), (["sketch", "--save-kmercounts", "--parse-by-seq"], "--save-kmercounts", "--parse-by-seq"),
    (["cmp", "-N", "--multiset"], "--save-kmercounts", "--multiset"), (["cmp", "--save-kmers", "--parse-by-seq"], "--save-kmers", "--parse-by-seq"),
])
def test_cli_refuses_save_kmers_outside_oph_sketches_of_whole_inputs(fasta, args, flag, other):
    r = _cli(*args, fasta)
    assert r.returncode == 1, r.stderr
    assert "outside the hot-path scope" in r.stderr and flag in r.stderr and other in r.stderr, r.stderr
    assert "gfx950" not in r.stderr                                    # refused before a context was asked for


def test_cli_ignores_save_kmers_with_presketched_and_help_names_the_flags(tmp_path):
    p = tmp_path / "stack.bin"
    p.write_bytes(np.array([2, 4], np.uint64).tobytes() + np.ones(2).tobytes() + np.arange(8, dtype=np.float64).tobytes())
    r = _cli("cmp", "--presketched", "-N", "--multiset", str(p))       # nothing is sketched there
    assert "outside the hot-path scope" not in r.stderr, r.stderr
    assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr
    h = _cli("sketch", "-h").stderr
    assert "--save-kmers" in h and "--save-kmercounts" in h and ".kmer64" in h
