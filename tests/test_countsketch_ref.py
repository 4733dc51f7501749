"""The count-sketch model (tests/countsketch_ref.py) held to hand-worked cases and to its own two forms, without a GPU: the integer
table the device computes against the reference's float row added to one k-mer at a time (src/counter.h:68-77), the `>=` of the
finalisation (counter.h:135) and the k-mer enumerators the GPU tests feed it with."""
import numpy as np
import pytest

import countsketch_ref as CS
import filter_ref as FR
import k0_ref
import k3_seam_cases as C
import oph_kmers_ref as R
import protein_ref as PR


def _rng_kmers(seed, n, distinct):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 42, distinct, dtype=np.uint64)[rng.integers(0, distinct, n)]


def test_one_cell_is_plus_minus_minus():
    km = _rng_kmers(1, 5000, 700)
    hv = CS.hashes(km, 0x1234)
    plus = int(((hv >> np.uint64(63)) == 1).sum())
    assert 0 < plus < km.size
    t = CS.table(km, 1, 0x1234)
    assert t.tolist() == [plus - (km.size - plus)]
    ids, w, tot = CS.lists(km, 1, 0x1234)
    assert ids.tolist() == [0] and w.tolist() == [abs(2 * plus - km.size)] and tot == abs(2 * plus - km.size)


def test_two_kmers_that_cancel_in_one_cell():
    """hand-worked: the first two k-mers of opposite sign that share a cell of seven leave it 0, and a cell of 0 is not an element"""
    cells = 7
    x = np.arange(1, 400, dtype=np.uint64)
    idx, sign = CS.cells_and_signs(x, cells)
    a = b = None
    for i in range(x.size):
        for j in range(i + 1, x.size):
            if idx[i] == idx[j] and sign[i] == -sign[j]:
                a, b = int(x[i]), int(x[j])
                break
        if a is not None:
            break
    assert a is not None
    # the arithmetic spelled out in Python integers for these two
    for v, i in ((a, int(np.flatnonzero(x == a)[0])), (b, int(np.flatnonzero(x == b)[0]))):
        hv = R.wang64_int(R.wang64_int(v))
        assert hv % cells == idx[i] and (1 if hv >> 63 else -1) == sign[i]
    t = CS.table([a, b], cells)
    assert not t.any()
    assert CS.lists([a, b], cells)[0].size == 0 and CS.lists([a, b], cells)[2] == 0
    t = CS.table([a, b, a], cells)                                      # a once more: its cell holds its sign
    assert t[idx[np.flatnonzero(x == a)[0]]] == sign[np.flatnonzero(x == a)[0]] and np.abs(t).sum() == 1


def test_xormask_enters_before_the_first_mix():
    km = _rng_kmers(2, 100, 100)
    assert np.array_equal(CS.hashes(km, 77), k0_ref.wang64(k0_ref.wang64(km ^ np.uint64(77))))
    assert not np.array_equal(CS.table(km, 64, 0), CS.table(km, 64, 77))


@pytest.mark.parametrize("cells", [1, 2, 3, 64, 1000, 1024])
@pytest.mark.parametrize("seed", [3, 4])
def test_float_form_equals_integer_form_below_2_24(cells, seed):
    """20 000 k-mers, a few of them hundreds of times: far below 2^24 per input, so every float add is exact"""
    km = np.concatenate([_rng_kmers(seed, 18000, 3000), np.repeat(_rng_kmers(seed + 10, 4, 4), 500)])
    np.random.default_rng(seed).shuffle(km)
    ti, tf = CS.table(km, cells, seed), CS.table_float(km, cells, seed)
    assert tf.dtype == np.float32 and np.array_equal(ti.astype(np.float64), tf.astype(np.float64))
    assert int(np.abs(ti).max()) < 2 ** 24
    for thr in (0.0, 1.0, 2.0, 3.0):
        a, b = CS.lists_dense(ti, thr), CS.lists_dense(tf, thr)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        s = CS.lists(km, cells, seed, thr)
        assert np.array_equal(a[0], s[0]) and np.array_equal(a[1], s[1]) and a[2] == s[2]


def test_the_float_row_stops_counting_at_2_24():
    """why F28 is a divergence: a float32 cell at 2^24 no longer moves by 1, the integer does"""
    c = np.float32(2 ** 24)
    assert np.float32(c + np.float32(1)) == c and np.float32(-c + np.float32(-1)) == -c
    assert np.float32(np.float32(2 ** 24 - 1) + np.float32(1)) == c


def test_the_seam_is_greater_or_equal():
    ids, sums = np.arange(6, dtype=np.uint64), np.array([0, 1, -1, 2, -2, 3])
    assert CS.compact(ids, sums, 0.0)[0].tolist() == [1, 2, 3, 4, 5]    # threshold 0: every cell but the empty one (weight 0 is ignored)
    assert CS.compact(ids, sums, 1.0)[0].tolist() == [1, 2, 3, 4, 5]    # |c| = 1 passes `>= 1` (the exact mode's `> 1` would drop it)
    assert CS.compact(ids, sums, 2.0)[0].tolist() == [3, 4, 5]
    i, w, t = CS.compact(ids, sums, 2.0)
    assert w.tolist() == [2.0, 2.0, 3.0] and t == 7 and w.dtype == np.float64
    assert CS.compact(ids, sums, 4.0)[0].size == 0 and CS.compact(ids, sums, 4.0)[2] == 0


def test_batch_lists_layout():
    kms = [_rng_kmers(5, 300, 50), np.empty(0, np.uint64), _rng_kmers(6, 10, 10)]
    ids, w, off, tot = CS.batch_lists(kms, 97, 9, 1.0)
    assert off[0] == 0 and off[1] == off[2] and off[3] == ids.size == w.size and tot[1] == 0
    for g, km in enumerate(kms):
        e = CS.lists(km, 97, 9, 1.0)
        lo, hi = int(off[g]), int(off[g + 1])
        assert np.array_equal(ids[lo:hi], e[0]) and np.array_equal(w[lo:hi], e[1]) and tot[g] == e[2]
        assert (np.diff(ids[lo:hi].astype(np.int64)) > 0).all()


def test_collision_free_is_about_distinct_kmers():
    km = np.array([5, 5, 5, 9], np.uint64)
    big = 1 << 40
    assert CS.collision_free(km, big)
    idx, _ = CS.cells_and_signs(np.array([5, 9], np.uint64), 2)
    assert CS.collision_free(km, 2) == (idx[0] != idx[1]) and not CS.collision_free(np.arange(10, dtype=np.uint64), 3)


# ---- the enumerators are the existing ones
def test_dna_enumerator_equals_the_record_roller():
    rng = np.random.default_rng(7)
    recs = [C.random_bases(rng, 300), C.random_bases(rng, 40) + "N" + C.random_bases(rng, 25) + "NN" + C.random_bases(rng, 90), "ACGT"]
    fa = C.fasta(recs)
    for k, canon in ((5, True), (21, False), (32, True)):
        want = [x for r in recs for part in r.replace("N", " ").split() for x in C.kmers_of((part,), k, canon)]
        assert CS.kmers_dna(fa, k, canon).tolist() == want
        assert [R.wang64_int(x ^ 3) for x in want] == R.masked_stream([p for r in recs for p in r.replace("N", " ").split()], k, canon, 3)


def test_window_and_filter_and_protein_enumerators():
    rng = np.random.default_rng(8)
    s = C.random_bases(rng, 500).encode()
    fa = b">a\n" + s + b"\n"
    plain, win = CS.kmers_dna(fa, 11, True), CS.kmers_dna(fa, 11, True, w=20)
    assert plain.size == 490 and win.size == 481 and set(win.tolist()) < set(plain.tolist())
    filt = [b">f\n" + s[100:200] + b"\n"]
    kept = CS.kmers_filtered(fa, filt, 11, True)
    fset = {FR.encode(w) for w in FR.filter_set(filt, 11, True)[0]}
    assert kept.tolist() == [x for x in plain.tolist() if x not in fset] and kept.size < plain.size
    p = PR.fa(PR.random_protein(9, 200) + b"X" + PR.random_protein(10, 50))
    assert CS.kmers_protein(p, 7, PR.PROTEIN20).size == (200 - 6) + (50 - 6)


def test_names():
    assert CS.cache_name("x.fa", 64, 21, 4096) == "x.fa.rc_canon.sketchsize64.k21.CountMinCounting4096.MultisetSpace.DNA.d2gbmh"
    assert CS.cache_name("x.fa", 64, 7, 5, canon=False, alphabet="PROTEIN20", seedseed=3, count_threshold=2) == \
        "x.fa.seed3.sketchsize64.k7.ct_threshold2.CountMinCounting5.MultisetSpace.PROTEIN20.d2gbmh"
    assert CS.options_tail(1000) == ";counting=countsketch1000\n"
