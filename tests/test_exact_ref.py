"""exact_ref.py held to its own properties: the literal merge of wcompare.cpp:145-187 against the closed form at every end-of-input
case, the measure table, two empty inputs, the two file layouts and the names of makedest.  No GPU, nothing of the product."""
import math

import numpy as np
import pytest

import exact_ref as X
import k3_seam_cases as C

U64 = np.uint64


def both(lk, lc, rk, rc):
    m, d = X.merge_isz(lk, lc, rk, rc), X.dict_isz(lk, lc, rk, rc)
    assert m == d, (lk, lc, rk, rc)
    assert X.merge_isz(rk, rc, lk, lc) == d
    return d


# ---------------------------------------------------------------- (b) against (c)
END_CASES = {
    "both_empty": ([], [], 0),
    "left_empty": ([], [3, 9], 0),
    "right_empty": ([3, 9], [], 0),
    "last_smaller": ([1, 5], [5, 7, 9], 1),            # the left side's last element is below the right side's current one after the match
    "last_equal": ([1, 9], [5, 9], 1),
    "last_larger": ([1, 9], [5, 7], 0),
    "single_equal": ([4], [4], 1),
    "single_differ": ([4], [5], 0),
    "identical": ([1, 2, 3, 8], [1, 2, 3, 8], 4),
    "disjoint_interleaved": ([1, 3, 5], [2, 4, 6], 0),
    "extremes": ([0, 2 ** 64 - 1], [0, 7, 2 ** 64 - 1], 2),
}


@pytest.mark.parametrize("name", sorted(END_CASES))
def test_literal_merge_equals_closed_form_at_every_end_of_input(name):
    lk, rk, want = END_CASES[name]
    assert both(lk, None, rk, None) == want
    lc, rc = [2 + i for i in range(len(lk))], [5 - i for i in range(len(rk))]
    w = both(lk, lc, rk, rc)
    assert w == sum(min(lc[lk.index(x)], rc[rk.index(x)]) for x in lk if x in rk)


def test_literal_merge_equals_closed_form_on_random_sets():
    rng = np.random.default_rng(77)
    for trial in range(60):
        nl, nr = rng.integers(0, 40, 2)
        lk = np.unique(rng.integers(0, 60, nl)).astype(U64)
        rk = np.unique(rng.integers(0, 60, nr)).astype(U64)
        lc, rc = rng.integers(1, 9, lk.size), rng.integers(1, 9, rk.size)
        both(lk, None, rk, None)
        both(lk, lc, rk, rc)
        assert X.dict_isz(lk, lc, rk, rc) == int(X.isz_matrix([(lk, lc.astype(np.uint32)), (rk, rc.astype(np.uint32))], True)[0, 1])


def test_min_is_taken_on_either_side_and_sums_pass_32_bits():
    big = 2 ** 32 - 1
    lk = rk = [10, 20, 30]
    assert both(lk, [big, 1, big - 1], rk, [big - 2, big, big]) == (big - 2) + 1 + (big - 1)


def test_sets_come_from_the_seam_cases_enumerator():
    b = C.planted_counts()
    for thr, per_unit in ((0.0, 4), (1.0, 3), (3.0, 1), (4.0, 0)):
        keys, counts = X.exact_sets(b, thr)[0]
        assert keys.size == 40 * per_unit and (np.diff(keys.astype(object)) > 0).all()
        assert counts.size == keys.size and (counts > thr).all()
        assert X.card(keys, counts, True) == sum(40 * c for c in (1, 2, 3, 4) if c > thr)
    k2, c2 = X.exact_sets(b, 1.0)[1]
    assert (c2 == 2).all() and X.card(k2, c2, False) == k2.size


# ---------------------------------------------------------------- the measure table
def test_measure_table():
    isz, a, b, k = 30, 100.0, 60.0, 21
    sim = 30 / (100 + 60 - 30)
    want = {X.SIMILARITY: sim, X.CONTAINMENT: 30 / 100, X.SYMMETRIC_CONTAINMENT: 30 / 60, X.INTERSECTION: 30.0,
            X.UNION_SIZE: 130.0, X.POISSON_LLR: math.log(2 * sim / (1 + sim)) * (-1 / 21)}
    for m, v in want.items():
        assert X.measure_value(isz, a, b, m, k) == np.float32(v), m
    assert X.measure_value(isz, b, a, X.CONTAINMENT, k) == np.float32(30 / 60)           # containment is not symmetric


def test_union_size_is_the_union_not_the_intersection():
    """finding F15: CORRECT_RES has no arm for UNION_SIZE; weighted_compare's lhsum + rhsum - isz is what is emitted"""
    assert X.measure_value(7, 10, 20, X.UNION_SIZE, 31) == np.float32(23.0)
    assert X.measure_value(0, 10, 20, X.UNION_SIZE, 31) == np.float32(30.0)


def test_two_empty_inputs_take_the_maximum():
    with np.errstate(over="ignore"):
        fmax = np.float32(np.finfo(np.longdouble).max)                                # what float(LDBL_MAX) gives
    for m in (X.SIMILARITY, X.CONTAINMENT, X.SYMMETRIC_CONTAINMENT, X.POISSON_LLR):
        v = X.measure_value(0, 0, 0, m, 31)
        assert v.tobytes() == fmax.tobytes(), m
    assert X.measure_value(0, 0, 0, X.INTERSECTION, 31) == 0 and X.measure_value(0, 0, 0, X.UNION_SIZE, 31) == 0
    assert X.measure_value(0, 5, 7, X.POISSON_LLR, 31).tobytes() == fmax.tobytes()         # disjoint: distance inf -> the maximum
    assert X.measure_value(0, 5, 7, X.SIMILARITY, 31) == 0


def test_condensed_order():
    m = np.arange(25, dtype=np.uint64).reshape(5, 5)
    assert X.ut(m).tolist() == [1, 2, 3, 4, 7, 8, 9, 13, 14, 19]
    assert X.ut(m, 1, 3).tolist() == [7, 8, 9, 13, 14]


# ---------------------------------------------------------------- files and names
def test_file_layouts_round_trip():
    keys, counts = np.array([3, 9, 2 ** 64 - 1], U64), np.array([2, 1, 7], np.uint32)
    kb_set, kb_cd, cb = X.key_file_bytes(keys, counts, False), X.key_file_bytes(keys, counts, True), X.count_file_bytes(counts)
    assert len(kb_set) == 8 + 24 and np.frombuffer(kb_set[:8], np.float64)[0] == 3.0      # --set header: |E|
    assert np.frombuffer(kb_cd[:8], np.float64)[0] == 10.0 and kb_cd[8:] == kb_set[8:]    # --countdict header: the sum; same keys
    assert len(cb) == 24 and np.frombuffer(cb, np.float64).tolist() == [2.0, 1.0, 7.0]
    # loaded: the card never comes from the header (F16) -- a --set run that picks up a --countdict key file and vice versa
    for kb in (kb_set, kb_cd):
        k, c, card = X.read_set(kb)
        assert np.array_equal(k, keys) and c is None and card == 3
        k, c, card = X.read_set(kb, cb)
        assert np.array_equal(k, keys) and np.array_equal(c, counts) and card == 10
    k, c, card = X.read_set(X.key_file_bytes([], [], False))
    assert k.size == 0 and card == 0


def test_names_of_makedest():
    assert X.makedest("d/a.fa", 31) == "d/a.fa.rc_canon.k31.FullMmerSet.DNA.kmerset64"
    assert X.makedest("d/a.fa", 21, canon=False) == "d/a.fa.k21.FullMmerSet.DNA.kmerset64"
    assert X.makedest("d/a.fa", 31, seed=13, count_threshold=2.0) == "d/a.fa.seed13.rc_canon.k31.ct_threshold2.FullMmerSet.DNA.kmerset64"
    assert X.makedest("d/a.fa", 31, count_threshold=1.5) == "d/a.fa.rc_canon.k31.ct_threshold1.500000.FullMmerSet.DNA.kmerset64"
    assert X.makedest("d/a.fa", 31, outprefix="out") == "out/a.fa.rc_canon.k31.FullMmerSet.DNA.kmerset64"
    assert "sketchsize" not in X.makedest("a.fa", 31)
    assert X.makedest("x/a.fa x/b.fa", 31) == "x/a.fa.rc_canon.k31.FullMmerSet.DNA.kmerset64"  # several files on a line: the first names it
    assert X.counts_path(X.makedest("d/a.fa", 31)) == "d/a.fa.rc_canon.k31.FullMmerSet.DNA.kmercounts.f64"


def test_rng_keys_are_distinct_sorted_and_in_range():
    k = X.rng_keys(5, 1000, lo=2 ** 63, hi=2 ** 63 + 5000)
    assert k.size == 1000 and (np.diff(k.astype(object)) > 0).all() and int(k[0]) >= 2 ** 63 and int(k[-1]) < 2 ** 63 + 5000
