"""The host side of --set / --countdict, without a GPU: the CLI accepts the flags and refuses, by message and exit status, what they do
not combine with; d2g_kset_check (what d2g_kset_create asks of host arrays first); d2g_epilogue_exact* against exact_ref's measure
table at 0 ulp; the goldens of tests/golden/exact (written by exact_ref) against today's exact_ref."""
import os
import subprocess

import numpy as np
import pytest

import exact_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
SCOPE = "outside the hot-path scope"


def _cli(*args, env=None):
    e = dict(os.environ)
    e.pop("D2G_DEVICES", None)
    e.update(env or {})
    return subprocess.run([EXE, *args], capture_output=True, text=True, env=e)


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    p = tmp_path_factory.mktemp("exact_cli") / "x.fa"
    p.write_text(">r\nACGTTGCATGCAGTCGATCGATCGTAGCTAGCTAGCATCGATCAGCTAGCATCG\n")
    return str(p)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "exact", "sets.npz"))


# ---------------------------------------------------------------- flags
@pytest.mark.parametrize("args", [["sketch", "--set"], ["sketch", "-H"], ["sketch", "--countdict"], ["sketch", "-J"], ["cmp", "--set"], ["cmp", "-H"],
                                  ["cmp", "--countdict"], ["cmp", "-J"], ["sketch", "--set", "-m", "2"], ["cmp", "-J", "--filterset", "FASTA"],
                                  ["cmp", "--set", "--square"], ["cmp", "-J", "--phylip"], ["sketch", "--set", "--cache", "--outprefix", "."]])
def test_cli_accepts_the_exact_flags(fasta, args):
    """in scope: no refusal; without a GPU it stops later, where every compute entry point does, at the creation of the context"""
    r = _cli(*[fasta if a == "FASTA" else a for a in args], fasta)
    assert SCOPE not in r.stderr and "not found in expected set" not in r.stderr, r.stderr
    assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr


REFUSED = [
    (["sketch", "--set", "--countdict"], ["--set", "--countdict"]),
    (["cmp", "-H", "-J"], ["--set", "--countdict"]),
    (["sketch", "--set", "-o", "out.bin"], ["--set", "-o", "bottomk", "--cmpout"]),
    (["cmp", "--countdict", "-o", "out.bin"], ["--countdict", "-o"]),
    (["sketch", "--set", "--multiset"], ["--set", "--multiset"]),
    (["sketch", "-J", "-B"], ["--countdict", "--multiset"]),
    (["sketch", "--set", "--parse-by-seq"], ["--set", "--parse-by-seq", "Not yet supported"]),
    (["sketch", "--countdict", "-s"], ["--countdict", "--save-kmers"]),
    (["cmp", "--set", "-N"], ["--set", "--save-kmercounts"]),
    (["cmp", "--set", "--fastcmp", "4"], ["--set", "--fastcmp"]),
    (["cmp", "-J", "--regsize", "1"], ["--countdict", "--fastcmp"]),
    (["cmp", "--set", "--topk", "3"], ["--set", "--topk", "LSH"]),
    (["cmp", "--set", "--similarity-threshold", "0.5"], ["--set", "--similarity-threshold", "LSH"]),
    (["cmp", "--countdict", "--greedy", "0.8"], ["--countdict", "--greedy", "LSH"]),
]


@pytest.mark.parametrize("args,words", REFUSED, ids=[" ".join(a) for a, _ in REFUSED])
def test_cli_refuses_what_the_exact_flags_do_not_combine_with(fasta, args, words):
    r = _cli(*args, fasta)
    assert r.returncode == 1, r.stderr
    assert SCOPE in r.stderr and all(w in r.stderr for w in words), r.stderr
    assert "gfx950" not in r.stderr                                    # refused before a context was asked for


@pytest.mark.parametrize("devs", ["all", "0,1"])
def test_cli_refuses_exact_jobs_over_several_gpus(fasta, devs):
    r = _cli("cmp", "--set", fasta, env={"D2G_DEVICES": devs})
    assert r.returncode == 1 and SCOPE in r.stderr and "D2G_DEVICES" in r.stderr and "gfx950" not in r.stderr, r.stderr
    r = _cli("cmp", "--set", fasta, env={"D2G_DEVICES": "0"})
    assert SCOPE not in r.stderr


@pytest.mark.parametrize("flag", ["--seq", "--full", "--prob", "--128bit", "--long-kmers"])
def test_the_other_out_of_scope_flags_stay_refused(fasta, flag):
    r = _cli("sketch", flag, fasta)
    assert r.returncode == 1 and SCOPE in r.stderr and flag in r.stderr, r.stderr


def test_presketched_k_mer_sets(tmp_path):
    """*.kmerset64 is --set; --countdict wants the sibling count file of every path and names the missing one; 128-bit sets stay out"""
    keys = np.array([3, 9, 27], np.uint64)
    a, b = tmp_path / "a.FullMmerSet.DNA.kmerset64", tmp_path / "b.FullMmerSet.DNA.kmerset64"
    a.write_bytes(X.key_file_bytes(keys, None, False))
    b.write_bytes(X.key_file_bytes(keys[:2], None, False))
    (tmp_path / "a.FullMmerSet.DNA.kmercounts.f64").write_bytes(X.count_file_bytes([1, 2, 3]))
    r = _cli("cmp", "--presketched", "--countdict", str(a), str(b))
    assert r.returncode == 1 and "b.FullMmerSet.DNA.kmercounts.f64" in r.stderr and "gfx950" not in r.stderr, r.stderr
    r = _cli("cmp", "--presketched", str(a), str(b))
    assert SCOPE not in r.stderr and (r.returncode == 0 or "gfx950" in r.stderr), r.stderr
    r = _cli("cmp", "--presketched", "--topk", "2", str(a), str(b))
    assert r.returncode == 1 and SCOPE in r.stderr and "exact k-mer sets" in r.stderr
    r = _cli("cmp", "--presketched", str(tmp_path / "a.kmerset128"))
    assert r.returncode == 1 and "128-bit" in r.stderr


def test_help_names_the_flags():
    h = _cli("sketch", "-h").stderr
    assert "--set/-H" in h and "--countdict/-J" in h and "kmerset64" in h and "kmercounts.f64" in h


# ---------------------------------------------------------------- d2g_kset_check
def test_kset_check_accepts_sorted_sets(d2g, golden):
    d2g.kset_check(golden["keys"], golden["counts"], golden["set_off"])
    d2g.kset_check(golden["keys"], None, golden["set_off"])
    d2g.kset_check(np.empty(0, np.uint64), None, np.zeros(1, np.uint64))
    d2g.kset_check(np.array([5, 1], np.uint64), None, np.array([0, 1, 2], np.uint64))       # descending across a set boundary is fine


def test_kset_check_refuses_unsorted_duplicated_and_zero_counts(d2g, golden):
    keys, off = golden["keys"].copy(), golden["set_off"]
    lo = int(off[3])
    keys[lo + 10], keys[lo + 11] = keys[lo + 11], keys[lo + 10]
    with pytest.raises(d2g.D2GError, match=r"set 3 is not sorted \(entry 11\)"):
        d2g.kset_check(keys, None, off)
    keys = golden["keys"].copy()
    keys[int(off[6]) + 1] = keys[int(off[6])]
    with pytest.raises(d2g.D2GError, match=r"set 6 holds a key twice \(entry 1\)"):
        d2g.kset_check(keys, None, off)
    counts = golden["counts"].copy()
    counts[int(off[2]) + 5] = 0
    with pytest.raises(d2g.D2GError, match=r"set 2 has a count of 0 \(entry 5\)"):
        d2g.kset_check(golden["keys"], counts, off)
    with pytest.raises(d2g.D2GError, match="set_off decreases"):
        d2g.kset_check(golden["keys"], None, np.array([0, 5, 3], np.uint64))


# ---------------------------------------------------------------- the epilogue, 0 ulp
CARD_CASES = [(0, 0, 0), (0, 5, 7), (1, 1, 1), (30, 100, 60), (30, 60, 100), (7, 7, 900), (12345, 54321, 12345), (2 ** 40 + 1, 2 ** 41, 2 ** 40 + 3),
              (3, 10 ** 9, 4), (2 ** 53 + 2, 2 ** 54, 2 ** 53 + 2)]


@pytest.mark.parametrize("k", [1, 21, 31])
def test_epilogue_equals_the_measure_table_bit_for_bit(d2g, k):
    for isz, a, b in CARD_CASES:
        for m in X.MEASURES:
            got, want = np.float32(d2g.epilogue_exact(isz, float(a), float(b), m, k)), X.measure_value(isz, a, b, m, k)
            assert got.tobytes() == want.tobytes(), (isz, a, b, m, k, got, want)


def test_epilogue_arrays_follow_the_condensed_and_the_block_order(d2g, golden):
    for name, col in (("isz_set", 0), ("isz_countdict", 1)):
        iszm, cards = golden[name], golden["cards"][:, col].astype(np.float64)
        n = iszm.shape[0]
        for m in X.MEASURES:
            for r0, r1 in ((0, n), (2, 5), (n - 1, n), (3, 3)):
                got = d2g.host_epilogue_exact_ut(X.ut(iszm, r0, r1), cards, n, r0, r1, m, 31, nthreads=3)
                assert got.tobytes() == X.measure_ut(iszm, cards, m, 31, r0, r1).tobytes(), (name, m, r0, r1)
            a0, a1, b0, b1 = 1, 6, 2, 7
            got = d2g.host_epilogue_exact_rect(iszm[a0:a1, b0:b1], cards, n, a0, a1, b0, b1, m, 31, nthreads=2)
            want = np.array([[X.measure_value(int(iszm[i, j]), cards[i], cards[j], m, 31) for j in range(b0, b1)] for i in range(a0, a1)], np.float32)
            assert got.tobytes() == want.tobytes(), (name, m)
    with pytest.raises(d2g.D2GError):
        d2g.host_epilogue_exact_ut(np.zeros(3, np.uint64), np.zeros(3), 3, 2, 1)


# ---------------------------------------------------------------- the goldens against today's exact_ref
def test_goldens_are_what_exact_ref_computes(golden):
    off = golden["set_off"].astype(np.int64)
    sets = [(golden["keys"][off[i]:off[i + 1]], golden["counts"][off[i]:off[i + 1]]) for i in range(off.size - 1)]
    assert [len(k) for k, _ in sets] == [0, 1, 37, 120, 120, 64, 250]
    np.testing.assert_array_equal(X.isz_matrix(sets, False), golden["isz_set"])
    np.testing.assert_array_equal(X.isz_matrix(sets, True), golden["isz_countdict"])
    np.testing.assert_array_equal(X.flat(sets)[3], golden["cards"])
    assert int(golden["isz_countdict"][5, 5]) == 64 * (2 ** 32 - 1) and int(golden["isz_set"][3, 4]) == 120
