"""cmp --greedy, the parts that need no GPU: the checker itself (tests/dedup_ref.py), d2g_dedup_clusters, format_double (through
`fmtcheck --double`), the CLI's parsing and its refusals -- all of which happen before a GPU context exists."""
import os
import subprocess

import numpy as np
import pytest

import dedup_ref as R
import knn_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the checker ------------------------------------------------------------------------------------------------------------
def test_reference_forms_agree_and_separate_from_single_linkage():
    v = (K.eqcounts(K.family_sigs(60, 64, seed=1).view(np.uint64)) / 64).astype(np.float32)
    for T in (0.1, 0.3, 0.9, 0, -1):
        assert R.dedup_reference(v, T) == R.dedup_reference_loop(v, T)
    assert R.dedup_reference(v, 0) == R.dedup_reference(v, 0.9)       # the default cut-off
    # A~B, B~C, A!~C: {A, B}, {C} -- C is never compared with the non-representative B
    chain = np.array([[1, .6, 0], [.6, 1, .6], [0, .6, 1]], np.float32)
    assert R.dedup_reference(chain, 0.5) == ([0, 2], [[1], []])
    # equal values: the smaller cluster index; a value below the threshold by one float ulp does not join
    tie = np.array([[1, 0, .5], [0, 1, .5], [.5, .5, 1]], np.float32)
    assert R.dedup_reference(tie, 0.5) == ([0, 1], [[2], []])
    up = float(np.nextafter(np.float32(0.5), np.float32(1)))
    assert R.dedup_reference(tie, up) == ([0, 1, 2], [[], [], []])


def test_cluster_files_round_trip():
    ids, cons = [0, 2, 3], [[1, 5], [], [4]]
    names = ["g%d" % i for i in range(6)]
    assert R.clusters_text(ids, cons, names, 0.25) == (b"#Clustering 6 items yielded 3 clusters of average size 2, separated by minimum similarity 0.25\n"
                                                        b"Cluster-0\tg0:0\tg1:1\tg5:5\nCluster-1\tg2:2\nCluster-2\tg3:3\tg4:4\n")
    b = R.clusters_bytes(ids, cons)
    indptr, indices = R.read_clusters_bytes(b)
    assert indptr.tolist() == [0, 3, 4, 6] and indices.tolist() == [0, 1, 5, 2, 3, 4] and len(b) == 16 + 8 * 4 + 4 * 6
    a = R.assign_of(ids, cons, 6)
    assert a.tolist() == [0, 0, 2, 3, 3, 0] and R.clusters_of(a) == (ids, cons)


# ---- d2g_dedup_clusters ---------------------------------------------------------------------------------------------------------
def test_dedup_clusters_against_the_restatement(d2g):
    for N in (1, 2, 17, 300):
        v = (K.eqcounts(K.family_sigs(N, 64, seed=N).view(np.uint64)) / 64).astype(np.float32)
        for T in (0.05, 0.2, 2.0):
            ids, cons = R.dedup_reference(v, T)
            indptr, indices = d2g.dedup_clusters(R.assign_of(ids, cons, N))
            assert indptr.size == len(ids) + 1 and indices.size == N
            got = [indices[int(indptr[c]):int(indptr[c + 1])].tolist() for c in range(len(ids))]
            assert got == [[r] + m for r, m in zip(ids, cons)], f"N {N} T {T}"
    indptr, indices = d2g.dedup_clusters(np.zeros(0, np.uint32))
    assert indptr.tolist() == [0] and indices.size == 0


@pytest.mark.parametrize("assign", [[1, 1], [0, 2, 2], [0, 0, 1], [0, 5], [0, 1, 1, 2]])
def test_dedup_clusters_refuses_a_malformed_assignment(d2g, assign):
    """a representative after its member, a member of a non-representative, an index past the end"""
    with pytest.raises(d2g.D2GError):
        d2g.dedup_clusters(np.array(assign, np.uint32))


# ---- format_double ----------------------------------------------------------------------------------------------------------
DOUBLES = [(3.0, "3"), (-17.0, "-17"), (1e15, "1000000000000000"), (1.0 / 3.0, "0.3333333333333333"), (0.1 + 0.2, "0.30000000000000004"),
           (1e-5, "1e-05"), (1e16, "1e+16"), (2.5e-4, "0.00025"), (0.0, "0"), (257.0 / 75.0, "3.4266666666666667"), (1e300, "1e+300"),
           (1.5e-7, "1.5e-07"), (0.9, "0.9")]


def test_format_double_on_hand_made_cases():
    exe = os.path.join(ROOT, "dashing2_amd", "bin", "fmtcheck")
    out = subprocess.run([exe, "--double"] + [x.hex() for x, _ in DOUBLES], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    assert out.stdout.split("\n")[:-1] == [e for _, e in DOUBLES]
    assert [R.fmt_double(x) for x, _ in DOUBLES] == [e for _, e in DOUBLES]        # the checker's own formatter agrees


# ---- the CLI ------------------------------------------------------------------------------------------------------------------
def _cli(*args):
    exe = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


@pytest.fixture(scope="module")
def stacked(tmp_path_factory):
    """presketched stacks: S = 64 and S = 100 (u64 N, u64 S, f64 cards, f64 registers)"""
    d = tmp_path_factory.mktemp("dedup_cli")
    out = {}
    for S in (64, 100):
        p = d / f"stack{S}.bin"
        sig = K.family_sigs(6, S, seed=S)
        with open(p, "wb") as f:
            f.write(np.array([6, S], np.uint64).tobytes() + np.ones(6).tobytes() + sig.tobytes())
        out[S] = str(p)
    return out


@pytest.mark.parametrize("arg", ["0.5", "0.5E", "0.5e", "0", ".25E"])
def test_cli_accepts_greedy(stacked, arg):
    """`cmp --presketched stack.bin --greedy T[E]` is in scope: no refusal; without a GPU it stops later, where every compute entry
    point does, at the creation of the context (with one, the six sketches are clustered)."""
    r = _cli("cmp", "--presketched", stacked[64], "--greedy", arg)
    assert "outside the hot-path scope" not in r.stderr, r.stderr
    assert "not found in expected set" not in r.stderr
    assert r.returncode == 0 or "gfx950" in r.stderr, r.stderr          # no device: the context is refused, loudly


@pytest.mark.parametrize("extra,word", [
    (["--greedy", "0.5F"], "F suffix"), (["--greedy", "0.5EF"], "F suffix"), (["--greedy", "0.5f"], "F suffix"),
    (["--greedy", "0.5", "--mash-distance"], "--mash-distance"), (["--distance", "--greedy", "0.5E"], "--mash-distance"),
    (["--greedy", "0.5", "--containment"], "cardinality"), (["--greedy", "0.5", "--symmetric-containment"], "cardinality"),
    (["--greedy", "0.5", "--intersection"], "cardinality"), (["--greedy", "0.5", "--union-size"], "cardinality"),
    (["--greedy", "0.5", "--fastcmp", "4"], "--fastcmp"), (["--greedy", "0.5", "--fastcmp", "2"], "--fastcmp"),
    (["--greedy", "0.5", "--fastcmp", "1", "--bbit-sigs"], "--fastcmp"),
    (["--greedy", "0.5", "--square"], "--square"), (["--square", "--greedy", "0.5"], "--square"),
    (["--greedy", "0.5", "--phylip"], "--phylip"),
    (["--greedy", "0.5", "--topk", "3"], "--topk"), (["--top-k", "3", "--greedy", "0.5"], "--topk"),
    (["--greedy", "0.5", "--similarity-threshold", "0.5"], "--similarity-threshold"),
])
def test_cli_refuses_out_of_scope_combinations(stacked, extra, word):
    r = _cli("cmp", "--presketched", stacked[64], *extra)
    assert r.returncode == 1, r.stderr
    assert "outside the hot-path scope" in r.stderr and word in r.stderr, r.stderr
    assert "gfx950" not in r.stderr                                    # refused before a context was asked for


def test_cli_refuses_a_query_panel_and_non_power_of_two_set_sketches(stacked, tmp_path):
    q = tmp_path / "q.txt"
    q.write_text("x.fa\n")
    r = _cli("cmp", "--greedy", "0.5", "-Q", str(q), "a.fa")
    assert r.returncode == 1 and "outside the hot-path scope" in r.stderr and "-Q" in r.stderr and "gfx950" not in r.stderr
    r = _cli("cmp", "--greedy", "0.5", "-S", "100", "a.fa")               # set space, S = 100: the value needs (gt, lt)
    assert r.returncode == 1 and "outside the hot-path scope" in r.stderr and "power of two" in r.stderr and "gfx950" not in r.stderr
    r = _cli("cmp", "--presketched", stacked[100], "--greedy", "0.5")     # ... also when the size comes from the file
    assert r.returncode == 1 and "outside the hot-path scope" in r.stderr and "power of two" in r.stderr and "gfx950" not in r.stderr
    r = _cli("cmp", "--presketched", stacked[100], "--greedy", "0.5", "--multiset")   # multiset space: any S is in scope
    assert "outside the hot-path scope" not in r.stderr


def test_cli_sketch_greedy_stays_refused_and_help_names_the_flag():
    r = _cli("sketch", "--greedy", "0.5", "x.fa")
    assert r.returncode == 1 and "outside the hot-path scope" in r.stderr and "gfx950" not in r.stderr
    r = _cli("cmp", "-h")
    assert r.returncode == 1 and "--greedy T[E]" in r.stderr
