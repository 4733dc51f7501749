"""The model of greedy clustering by edit distance (edit_dedup_ref.py) against itself, without a GPU: its two statements of the rule
agree on every family the device tests use, the batched distance matrix equals edit_ref's, and the censuses say what each family
exercises (test_gpu_edit_dedup.py relies on those numbers)."""
import numpy as np
import pytest

import edit_dedup_cases as C
import edit_dedup_ref as R
import edit_ref as E


def both(d, T):
    a = R.greedy_assign(d, T)
    np.testing.assert_array_equal(a, R.greedy_assign_loop(d, T))
    return a


def test_the_batched_matrix_is_edit_refs():
    recs, d = C.seam_family()
    np.testing.assert_array_equal(R.edit_matrix_batch(recs), d)
    recs, d = C.ragged()
    pick = list(range(0, len(recs), 5))
    np.testing.assert_array_equal(d[np.ix_(pick, pick)], E.edit_matrix([recs[i] for i in pick]))
    assert R.edit_matrix_batch([]).shape == (0, 0) and R.edit_matrix_batch([b"", b"AC", b""]).tolist() == [[0, 2, 0], [2, 0, 2], [0, 2, 0]]


def test_the_rule_on_cases_known_by_construction():
    x = b"ACGTACGTAC"
    # an equidistant pair of representatives: the smaller index wins, in both input orders
    for recs in ([b"AAGTACGTAC", b"ACGTACGTAA", x], [b"ACGTACGTAA", b"AAGTACGTAC", x]):
        d = E.edit_matrix(recs)
        assert d[2, 0] == d[2, 1] == 1 and d[0, 1] == 2
        assert both(d, 1).tolist() == [0, 1, 0]
    # A ~ B ~ C, A !~ C: B joins A, C founds a cluster although B is within the bound
    d = E.edit_matrix([b"AAAA", b"AAAT", b"AATT"])
    assert both(d, 1).tolist() == [0, 0, 2]
    # duplicates at T = 0; empty records
    assert both(E.edit_matrix([b"AC", b"AG", b"AC", b"AG", b"AC"]), 0).tolist() == [0, 1, 0, 1, 0]
    assert both(E.edit_matrix([b"", b"A", b""]), 0).tolist() == [0, 1, 0]
    assert both(E.edit_matrix([b"", b"A", b""]), 1).tolist() == [0, 0, 0]


@pytest.mark.parametrize("T,clusters", list(zip([0, 1, 2, 15, 30, 31, 32, 33], [57, 48, 39, 21, 8, 8, 9, 8])))
def test_the_seam_family(T, clusters):
    recs, d = C.seam_family()
    assert len(recs) == 70 and R.n_clusters(both(d, T)) == clusters


def test_the_chains_exercise_what_greedy_can_get_wrong():
    recs, d = C.chains()
    assert len(recs) == 300
    seen = {k: [] for k in ("ties", "nearer_nonrep", "rep_despite_nonrep", "joins_same_band", "joins_earlier_band")}
    same0 = []
    for T in (1, 2, 3, 5, 8):
        both(d[:120, :120], T)
        c = R.census(d, T, 32)
        assert 1 < c["clusters"] < 300
        for k in seen:
            assert c[k] > 0, (T, k)
            seen[k].append(c[k])
        same0.append(R.census(d, T, 256)["joins_same_band"])
    assert (min(seen["ties"]), max(seen["ties"])) == (10, 41)
    assert (min(seen["nearer_nonrep"]), max(seen["nearer_nonrep"])) == (53, 208)
    assert (min(seen["rep_despite_nonrep"]), max(seen["rep_despite_nonrep"])) == (9, 36)
    assert (min(seen["joins_same_band"]), max(seen["joins_same_band"])) == (11, 22)
    assert (min(seen["joins_earlier_band"]), max(seen["joins_earlier_band"])) == (169, 254)
    assert (min(same0), max(same0)) == (147, 232)


def test_the_band_family():
    recs, d = C.band_family()
    assert len(recs) == 513
    got = {n: R.census(d[:n, :n], 2, 256) for n in (255, 256, 257, 513)}
    assert [got[n]["clusters"] for n in (255, 256, 257, 513)] == [108, 108, 108, 129]
    assert got[256]["joins_earlier_band"] == 0 and got[257]["joins_earlier_band"] == 1
    assert R.n_clusters(R.greedy_assign(d, 1)) == 206
    both(d[:150, :150], 2)


def test_the_ragged_and_the_mixed_family():
    recs, d = C.ragged()
    assert len(recs) == 120 and R.n_clusters(both(d, 3)) == 58
    recs, d = C.mixed()
    lens = sorted(map(len, recs))
    assert len(recs) == 40 and lens[-2] >= 1997 and lens[-3] <= 160 and d[7, 29] == 3
    a = both(d, 7)
    assert a[29] == 7 and 1 < R.n_clusters(a) < 40
    assert len(set(recs[7])) > 64, "the long records must have an alphabet whose table does not fit"


def test_the_random_sets_are_mostly_non_trivial():
    sets = C.random_sets()
    assert len(sets) == 200 and all(len(r) <= 48 and max(map(len, r)) <= 40 and 0 <= T <= 6 for r, T, _ in sets)
    nontrivial = 0
    for (recs, T, _), d in zip(sets, C.random_matrices()):
        nontrivial += 1 < R.n_clusters(both(d, T)) < len(recs)
    assert nontrivial >= 100
