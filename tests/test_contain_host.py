"""The host side of `dashing2 contain`, without a GPU: d2g_epilogue_contain against contain_ref's restatement; the database loader,
both writers and the text of every value of tests/golden/contain_fmt.txt (fmt 12.1.0's own) in a stand-alone program under ASan + UBSan;
what the CLI refuses, by message and exit status, before it asks for a GPU context."""
import os
import subprocess

import numpy as np
import pytest

import contain_ref as R
from conftest import GOLDEN, ROOT

EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
SCOPE = "outside the hot-path scope"
USAGE = "Usage: dashing2 contain <flags> database.kmers <input.fq> <input2.fq>..."


def _cli(*args, env=None):
    e = dict(os.environ)
    e.pop("D2G_DEVICES", None)
    e.update(env or {})
    return subprocess.run([EXE, "contain", *args], capture_output=True, text=True, env=e)


def _write_db(path, nrefs=2, S=4, k=21, w=None, dtype=0, canon=True, seed=0, extra=b"", names=None):
    keys = np.arange(1, nrefs * S + 1, dtype=np.uint64).reshape(nrefs, S) if S else np.zeros((nrefs, 0), np.uint64)
    hdr = np.array([dtype | int(canon) << 8, S, k, k if w is None else w], np.uint32).tobytes() + np.array([seed], np.uint64).tobytes()
    with open(path, "wb") as f:
        f.write(hdr + keys.tobytes() + extra)
    if names is not None:
        with open(str(path) + ".names.txt", "w") as f:
            f.write("".join(n + "\n" for n in names))
    return str(path)


@pytest.fixture(scope="module")
def query(tmp_path_factory):
    p = tmp_path_factory.mktemp("contain_q") / "q.fa"
    p.write_text(">r\nACGTTGCATGCAGTCGATCGATCGTAGCTAGCTAGCATCGATCAGCTAGCATCG\n")
    return str(p)


# ---------------------------------------------------------------- the epilogue
def test_epilogue_equals_the_restatement(d2g):
    rng = np.random.default_rng(11)
    for S in (1, 10, 63, 1000, 1024):
        m = np.concatenate([np.arange(S + 1), rng.integers(0, S + 1, 200)]).astype(np.uint32)
        s = np.concatenate([rng.integers(0, 50, S + 1) * np.arange(S + 1), rng.integers(0, 1 << 32, 200)]).astype(np.uint32)
        s[5:9] = [0, 1, 0xFFFFFFFF, (3 << 32) + 7 & 0xFFFFFFFF]                         # sums that wrapped past 2^32
        cov, dep = d2g.epilogue_contain(m, s, S)
        ecov, edep = R.epilogue(m, s, S)
        assert np.array_equal(cov.view(np.uint32), ecov.view(np.uint32)) and np.array_equal(dep.view(np.uint32), edep.view(np.uint32))
        assert cov[0] == 0 and dep[0] == 0                                            # matches = 0, whatever the sum says
    cov, dep = d2g.epilogue_contain(np.array([3], np.uint32), np.array([10], np.uint32), 1024)
    assert dep[0] == 3.0 and cov[0] == np.float32(3 / 1024)                           # integer division: 10 / 3 = 3
    with pytest.raises(d2g.D2GError):
        d2g.epilogue_contain(np.array([3], np.uint32), np.array([10], np.uint32), 0)


# ---------------------------------------------------------------- loader, writers and value text under the sanitizers
def test_contain_host_code_under_sanitizers_and_against_the_fmt_golden():
    csrc = os.path.join(ROOT, "dashing2_amd", "csrc")
    r = subprocess.run(["make", "-s", "-C", csrc, "../bin/contain_selftest_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(ROOT, "dashing2_amd", "bin", "contain_selftest_asan"), os.path.join(GOLDEN, "contain_fmt.txt")],
                       capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "contain selftest OK (2562 golden entries)" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


def test_golden_covers_every_match_count_of_its_sketch_sizes():
    seen = {10: set(), 1000: set(), 1024: set()}
    ints = set()
    with open(os.path.join(GOLDEN, "contain_fmt.txt")) as f:
        for line in f:
            kind, a, b, _ = line.split()
            (seen[int(a)] if kind == "g" else ints).add(int(b))
    assert all(seen[S] == set(range(S + 1)) for S in seen) and set(range(300)) <= ints


# ---------------------------------------------------------------- the CLI in front of the GPU
@pytest.mark.parametrize("args", [["-h"], [], ["-b"], ["-o", "x"]])
def test_usage_and_exit_status_without_a_database(args):
    r = _cli(*args)
    assert r.returncode == 1 and USAGE in r.stderr and "-F: read input paths from file at <arg>" in r.stderr and "gfx950" not in r.stderr


def test_main_usage_lists_contain_in_scope_and_printmin_stays_refused():
    r = subprocess.run([EXE], capture_output=True, text=True)
    last = r.stderr.strip().split("\n")[-1]
    assert r.returncode == 1 and "contain" in last and "printmin is out of scope" in last and "contain/printmin" not in last
    r = subprocess.run([EXE, "printmin"], capture_output=True, text=True)
    assert r.returncode == 1 and SCOPE in r.stderr


REFUSED = [("protein", dict(dtype=1), ["not DNA"]), ("k33", dict(k=33), ["k = 33"]), ("window", dict(k=21, w=30), ["windowed minimizers", "30"]),
           ("S0", dict(S=0), ["sketch size 0"])]


@pytest.mark.parametrize("name,kw,words", REFUSED, ids=[r[0] for r in REFUSED])
def test_cli_refuses_databases_out_of_scope_before_a_context(tmp_path, query, name, kw, words):
    db = _write_db(tmp_path / "db.kmer64", names=["a", "b"], **kw)
    r = _cli(db, query)
    assert r.returncode == 1 and SCOPE in r.stderr and all(w in r.stderr for w in words), r.stderr
    assert "gfx950" not in r.stderr


@pytest.mark.parametrize("devs", ["all", "0,1"])
def test_cli_refuses_several_gpus(tmp_path, query, devs):
    db = _write_db(tmp_path / "db.kmer64", names=["a", "b"])
    r = _cli(db, query, env={"D2G_DEVICES": devs})
    assert r.returncode == 1 and SCOPE in r.stderr and "D2G_DEVICES" in r.stderr and "gfx950" not in r.stderr, r.stderr


def test_corrupt_database_and_wrong_names_count(tmp_path, query):
    db = _write_db(tmp_path / "odd.kmer64", S=4, extra=b"\0" * 4, names=["a", "b"])     # 4 more bytes: a multiple of S, not of 8 S
    r = _cli(db, query)
    assert r.returncode == 1 and "Database corrupted (not a multiple of uint64_t size). Regenerate?" in r.stderr and "gfx950" not in r.stderr
    db = _write_db(tmp_path / "row.kmer64", S=4, extra=b"\0" * 8, names=["a", "b"])     # one key more: not a whole row
    r = _cli(db, query)
    assert r.returncode == 1 and "Database corrupted (not a multiple" in r.stderr and "gfx950" not in r.stderr
    db = _write_db(tmp_path / "names.kmer64", names=["a", "b", "c"])
    r = _cli(db, query)
    assert r.returncode == 1 and "Database corrupted; wrong number of names." in r.stderr and "gfx950" not in r.stderr
    r = _cli(str(tmp_path / "missing.kmer64"), query)
    assert r.returncode == 1 and "missing.kmer64" in r.stderr and "gfx950" not in r.stderr


def test_database_without_a_names_file_passes_the_loader(tmp_path, query):
    """the reference always throws here; this build names the references 0 .. nrefs-1 and goes on to the GPU"""
    db = _write_db(tmp_path / "nonames.kmer64", nrefs=3)
    r = _cli(db, query)
    assert "wrong number of names" not in r.stderr and "Database corrupted" not in r.stderr and SCOPE not in r.stderr, r.stderr
    assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr
    if r.returncode == 0:
        assert r.stdout.split("\n")[2] == "##References:\t0\t1\t2"


# ---------------------------------------------------------------- the table's size limit
def test_table_slots_stay_nameable_in_32_bits(d2g):
    """the probe names a slot in a uint32 and sets two values aside: ~0 (not found) and `slots` (the all-ones k-mer, behind the slots).
    Every table the library will build has slots <= 2^31, so slots - 1 is no sentinel and slots does not wrap; more keys are refused."""
    assert [d2g.screen_table_slots(d) for d in (0, 1, 8, 9, 2047, 2048, 2049)] == [16, 16, 16, 32, 4096, 4096, 8192]
    top = d2g.SCREEN_MAX_KEYS
    assert top == 1 << 30
    for d in (top - 1, top):
        s = d2g.screen_table_slots(d)
        assert s == 1 << 31 and s >= 2 * d and s < 0xFFFFFFFF and (s & 0xFFFFFFFF) == s
    assert d2g.screen_table_slots((1 << 29) + 1) == 1 << 31 and d2g.screen_table_slots(1 << 29) == 1 << 30
    for d in (top + 1, 1 << 31, (1 << 64) - 1):
        with pytest.raises(d2g.D2GError) as e:
            d2g.screen_table_slots(d)
        assert e.value.status == -5
