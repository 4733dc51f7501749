"""k3_seam_cases.py held to what it promises, on the reference alone (no GPU): every case plants what its docstring says, the
seams sit where the kernel's constants put them, and the cases have detection power -- a kernel that made the mistake a case is
aimed at would return other registers than the expected ones."""

import numpy as np
import pytest

import k0_ref
import k3_seam_cases as C

ONES = np.uint64(C.M64)
INF_BITS = np.float64(np.inf).view(np.uint64)


def count_of(keys, counts, key):
    hit = np.flatnonzero(keys == key)
    return int(counts[hit[0]]) if hit.size else 0


def assert_nothing_left(exp):
    kk, cc, sig, tw = exp
    assert kk.size == 0 and cc.size == 0 and tw == 0.0 and (sig.view(np.uint64) == INF_BITS).all()


# ---------------------------------------------------------------- a
@pytest.mark.parametrize("which", ["backbone", "unit"])
def test_all_ones_key_is_planted_with_its_count(oracle, which):
    b = C.all_ones_generic(which)
    (keys, counts, nk), = b.counts()
    assert nk == 20_000 - 20 + 3 * 20 and b.nkmers() == [nk]
    assert count_of(keys, counts, ONES) == b.note["count"] == {"backbone": 1, "unit": 3}[which]
    # the oracle's own k-mer walk agrees on the whole set (the mask moves keys, it does not merge them)
    ok, oc, onk = oracle.kmer_count_buffer(b.fastas()[0], b.k, canon=True, xormask=b.xormask)
    assert onk == nk and np.array_equal(ok, keys) and np.array_equal(oc, counts)
    plain = C.key_counts(tuple(b.genomes[0]), b.k, True, 0)
    assert plain[0].size == keys.size and np.array_equal(np.sort(plain[1]), np.sort(counts)) and ONES not in plain[0]
    assert sorted(set(counts.tolist())) == [1, 3] and int((counts == 3).sum()) == 20
    for thr in b.thresholds:
        (kk, cc, sig, tw), = b.expected(thr)
        assert tw == float(cc.sum()) and (ONES in kk) == (b.note["count"] > thr)
        assert kk.size == {0.0: keys.size, 1.0: 20, 2.0: 20, 3.0: 0}[thr]
        if thr < 3.0:
            assert np.isfinite(sig).all() and (sig > 0).all()
    assert_nothing_left(b.expected(3.0)[0])


def test_a_genome_of_the_all_ones_key_alone(oracle):
    b = C.all_ones_only()
    (k0, c0, n0), (k1, c1, n1), (k2, c2, n2) = b.counts()
    assert k0.tolist() == [C.M64] and c0.tolist() == [180] and n0 == 180
    assert count_of(k1, c1, ONES) == 10 and k1.size > 1000 and int((c1 > 1).sum()) == 1
    assert k2.size == 0 and n2 == 0
    ok, oc, _ = oracle.kmer_count_buffer(b.fastas()[0], b.k, canon=True, xormask=b.xormask)
    assert ok.tolist() == [C.M64] and oc.tolist() == [180]
    e0 = b.expected(0.0)
    assert np.isfinite(e0[0][2]).all() and e0[0][3] == 180.0 and np.isfinite(e0[1][2]).all()
    assert_nothing_left(e0[2])
    assert b.expected(9.0)[1][0].tolist() == [C.M64] and b.expected(9.0)[1][3] == 10.0      # the key ~0 is all that is left
    assert_nothing_left(b.expected(10.0)[1])
    assert_nothing_left(b.expected(180.0)[0])
    assert_nothing_left(b.expected(180.0)[1])


# ---------------------------------------------------------------- b
@pytest.mark.parametrize("k", [16, 17, 21])
def test_all_ones_stored_words_are_planted(oracle, k):
    b = C.all_ones_compact(k)
    assert not b.canon
    all_t = int(k0_ref.wang64(np.array([(1 << (2 * k)) - 1], np.uint64) ^ np.uint64(b.xormask))[0])
    (k0, c0, _), (k1, c1, n1), (k2, c2, _) = b.counts()
    assert k1.tolist() == [all_t] and c1.tolist() == [6] and n1 == 6
    # two runs of k + 4 T: ten all-T k-mers; at k = 16 the eight sixteen-T runs behind the random prefixes are that k-mer too
    assert count_of(k0, c0, np.uint64(all_t)) == (18 if k == 16 else 10)
    ends = [C.ends_in_sixteen_t(b, g) for g in range(3)]
    # the distinct k-mers that end in sixteen T differ in their prefix of k - 16 bases: (prefix, T...) inside the first run, the
    # planted prefixes (three different last bases: all there is at k = 17), the all-T k-mer
    assert ends[0].size == {16: 1, 17: 4, 21: 14}[k] and ends[1].size == 1 and ends[2].size == 0
    assert np.isin(ends[0], k0).all()
    ok, oc, _ = oracle.kmer_count_buffer(b.fastas()[0], k, canon=False, xormask=b.xormask)
    assert np.array_equal(ok, k0) and np.array_equal(oc, c0)
    for thr in b.thresholds:
        exp = b.expected(thr)
        assert (np.uint64(all_t) in exp[0][0]) == ((18 if k == 16 else 10) > thr)
        assert np.isfinite(exp[2][2]).all() == (thr < 1.0)
    assert_nothing_left(b.expected(9.0)[1])


# ---------------------------------------------------------------- c
def test_table_round_seams_follow_the_constants():
    """restated from d2g_internal.h: a changed constant fails here instead of silently moving the seam away from ROUND_SIZES"""
    c = C.k3_constants()
    assert c == {"K3_ROUND_KEYS": 1400, "K3_TARGET": 1024, "K3_SPLIT_MIN": 5600, "K3_MAXBBITS": 12, "K3_TAB": 2048}
    got = {nk: C.table_rounds(nk, c) for nk in C.ROUND_SIZES}
    assert got == {1399: (1, True), 1400: (1, True), 1401: (2, False), 2047: (2, False), 2048: (2, False), 2049: (2, False),
                   2799: (2, False), 2800: (2, False), 2801: (4, False), 5600: (4, False), 5601: ("split", 3)}
    # one bucket per genome under ROUND_ENV: ceil_log2(ceil(nk / bucket_keys)) = 0
    assert all(nk <= int(C.ROUND_ENV["D2G_K3_BUCKET_KEYS"]) for nk in C.ROUND_SIZES)
    for seam in (c["K3_ROUND_KEYS"], 2 * c["K3_ROUND_KEYS"], c["K3_SPLIT_MIN"]):
        assert seam in C.ROUND_SIZES and seam + 1 in C.ROUND_SIZES
    assert all(c["K3_TAB"] + d in C.ROUND_SIZES for d in (-1, 0, 1))


def test_table_round_genomes_hold_distinct_kmers():
    b = C.table_round_genomes()
    assert b.nkmers() == list(C.ROUND_SIZES)
    for (keys, counts, nk), want in zip(b.counts(), C.ROUND_SIZES):
        assert nk == want and keys.size == want and (counts == 1).all()
    for kk, cc, sig, tw in b.expected(0.0):
        assert np.isfinite(sig).all() and tw == float(kk.size)


# ---------------------------------------------------------------- d
def test_planted_counts_and_thresholds():
    b = C.planted_counts()
    (k0, c0, n0), (k1, c1, n1) = b.counts()
    assert [int((c0 == c).sum()) for c in (1, 2, 3, 4)] == [40] * 4 and k0.size == 160 and n0 == 400
    assert (c1 == 2).all() and k1.size == 313
    assert set(b.thresholds) >= {-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 1e10, 4294967295.0}
    kept = {-1.0: 160, 0.0: 160, 0.5: 160, 1.0: 120, 1.5: 120, 2.0: 80, 2.5: 80, 3.0: 40, 4.0: 0, 1e10: 0, 4294967295.0: 0}
    for thr, n in kept.items():
        e0, e1 = b.expected(thr)
        assert e0[0].size == n and (e0[1].astype(np.float64) > thr).all()
        assert e1[0].size == (313 if thr < 2.0 else 0)
        if n == 0:
            assert_nothing_left(e0)
        else:
            assert np.isfinite(e0[2]).all() and e0[3] == float(e0[1].sum())
    assert_nothing_left(b.expected(2.0)[1])
    # every step of the threshold changes the registers: the cases can tell a threshold that is off by one
    sigs = [b.expected(t)[0][2].view(np.uint64) for t in (0.0, 1.0, 2.0, 3.0, 4.0)]
    assert all(not np.array_equal(x, y) for x, y in zip(sigs, sigs[1:]))


# ---------------------------------------------------------------- e
def test_strip_edges_are_the_kernels():
    """top_edge / top_count of d2g_k3_bmh.hip: 16 unit strips, then octaves up to 2^53"""
    assert C.TOP_EDGES[:17] == [float(t) for t in range(17)] and C.TOP_EDGES[17] == 32.0 and C.TOP_EDGES[65] == 2.0 ** 53
    assert all(a < b for a, b in zip(C.TOP_EDGES, C.TOP_EDGES[1:]))
    for e in (16.0, 32.0, 64.0, 1024.0):
        assert all(x in C.EDGE_COUNTS for x in (e - 1, e, e + 1))
    assert [C.top_strip_floor(w) for w in (1, 2, 15, 16, 17, 31, 32, 33, 1024, 1025, 4096, 4097, 0.5, 16.5)] == \
        [0, 1, 14, 15, 16, 16, 16, 32, 512, 1024, 2048, 4096, 0, 16]


def test_strip_edge_batches_take_both_forms_of_the_first_pass():
    full, big, small = C.strip_edge_counts(), C.strip_edge_counts("big"), C.strip_edge_counts("small")
    assert C.predicted_light(full.nkmers(), full.S) and C.predicted_light(big.nkmers(), big.S)
    assert not C.predicted_light(small.nkmers(), small.S)
    assert len(full.genomes) == 17 and len(big.genomes) == 18 and len(small.genomes) == 15
    for b in (full, big, small):
        for (keys, counts, nk), c in zip(b.counts(), b.note["counts"]):
            assert keys.size == 8 and (counts == c).all() and nk == 8 * c
    assert big.counts()[-1][0].size > 299_000


def test_strip_edge_counts_detect_a_dropped_top_strip(oracle):
    """what a kernel that walks one strip too few returns for an element of count c is the sketch of weight = the lower edge of
    c's top strip; for every c at an edge or just below one that differs from the expected sketch"""
    b = C.strip_edge_counts()
    for (keys, cc, sig, tw), c in zip(b.expected(0.0), b.note["counts"]):
        if float(c) in C.TOP_EDGES or float(c + 1) in C.TOP_EDGES:
            floor = C.top_strip_floor(float(c))
            wrong, _ = oracle.bmh_from_weighted(keys, np.full(keys.size, floor), b.S)
            assert not np.array_equal(wrong.view(np.uint64), sig.view(np.uint64)), c
            # ... and one too many changes nothing: strips above the weight hold no point of the element
    for (keys, cc, sig, tw), (keys2, *_r) in zip(b.expected(0.0), C.strip_edge_counts("small").expected(0.0)):
        assert np.array_equal(keys, keys2)                               # the same genomes in both batches


# ---------------------------------------------------------------- f
def test_level_weights_cover_every_edge():
    ws, below = C.level_weights()
    assert ws.size == 203 and ws.min() == C.WEIGHT_FLOOR and ws.max() == 2.0 ** 53
    for e in C.TOP_EDGES[1:]:
        assert e in ws and np.nextafter(e, 0.0) in ws and (e == 2.0 ** 53 or np.nextafter(e, np.inf) in ws)
    assert all(x in ws for x in (2.0 ** -200, 2.0 ** -64, 0.5, 0.75, 1.5, 15.5, 16.5, 24.0, 3e9))
    assert int(np.isfinite(below).sum()) == 65
    assert C.TOO_LARGE == 2.0 ** 53 * (1 + 2.0 ** -52)


def test_every_weighted_set_passes_the_librarys_check(d2g):
    for sets in [C.weights_one_per_set(S) for S in (1, 2, 3, 64, 255)] + [C.weights_one_set(), C.weights_in_a_crowd()]:
        d2g.bmh_check_weights(sets.weights, sets.off, sets.S)
        d2g.bmh_check_weights(sets.weights, sets.off, sets.S, 0.001)
        assert sets.weights.min() >= C.WEIGHT_FLOOR
        assert np.isfinite(sets.sig).all() and np.array_equal(sets.tw > 0, np.ones(sets.tw.size, bool))
    with pytest.raises(d2g.D2GError):
        d2g.bmh_check_weights(np.array([C.TOO_LARGE]), np.array([0, 1], np.uint64), 64)


def test_below_edge_weights_detect_a_dropped_top_strip(oracle):
    """S = 64: the sketch of the double below an edge differs from the sketch of the next lower edge, which is what a kernel
    that walks one strip too few would return for it"""
    ws, below = C.level_weights()
    sets = C.weights_one_per_set(64)
    for i in np.flatnonzero(below > 0):
        wrong, _ = oracle.bmh_from_weighted(sets.ids[i:i + 1], below[i:i + 1], 64)
        assert not np.array_equal(wrong.view(np.uint64), sets.sig[i].view(np.uint64)), ws[i]


def test_weighted_set_shapes():
    one = C.weights_one_set()
    assert one.sig.shape == (1, 64) and np.unique(one.own[0]).size > 1 and one.own.max() < 203
    # the heaviest elements own the registers: 2^53 and its neighbours outweigh the rest together
    assert np.isin(one.own[0], np.flatnonzero(one.weights >= 2.0 ** 51)).mean() > 0.5
    for S in (1, 2, 3, 64, 255):
        s = C.weights_one_per_set(S)
        assert s.sig.shape == (203, S) and (s.own == 0).all() and np.array_equal(s.tw, s.weights)
    crowd = C.weights_in_a_crowd()
    assert crowd.sig.shape == (203, 64) and (np.diff(crowd.off.astype(np.int64)) == 2050).all()
    assert 2050 > 2048                                                   # the seam element is the second workgroup's
    ws, _ = C.level_weights()
    base = crowd.sig[int(np.argmin(ws))].view(np.uint64)                 # the seam element of weight 2^-200 owns nothing
    differs = np.array([not np.array_equal(base, s.view(np.uint64)) for s in crowd.sig])
    assert differs[ws >= 2.0 ** 12].all() and not differs[ws <= 2.0 ** -64].any()
