"""query_stream_cases.py held to its conditions Q1 .. Q5 on the CPU: the cases of test_gpu_query_streams.py are such that a launch on
the wrong stream, a stale decoy or a poisoned output cannot pass.  Conditions, not measurements; the figures are printed beside them."""
import numpy as np
import pytest

import query_stream_cases as Q

P32, P64 = np.uint32(Q.POISON), np.uint64(Q.POISON64)


def written_words_of_a_selection(sel):
    """rowcnt, and the slots a row fills (the others are expected to keep the poison)"""
    rowcnt, ids, cts = sel
    used = np.arange(ids.shape[1])[None, :] < np.minimum(rowcnt, ids.shape[1])[:, None]
    assert (ids[~used] == P32).all() and (cts[~used] == P32).all()
    return [rowcnt, ids[used], cts[used]]


def check_selection(sel, N, cap, what):
    """Q2 and Q5"""
    rowcnt = sel[0].astype(np.int64)
    nnz = int(rowcnt.sum())
    print(f"{what}: nnz {nnz} of {N * (N - 1)}, widest row {int(rowcnt.max())}, cap {cap}")
    assert 0 < nnz < N * (N - 1), what
    assert rowcnt.max() > cap, f"{what}: no row overflows its cap"
    for w in written_words_of_a_selection(sel):
        assert not (w == P32).any(), what


def check_clustering(assign, what):
    """Q3 and Q5"""
    n = Q.n_clusters(assign)
    print(f"{what}: {n} clusters of {assign.size}")
    assert 2 <= n <= assign.size - 1, what
    assert not (assign == P32).any()


# ---------------------------------------------------------------- 1. sketches
@pytest.mark.parametrize("name", sorted(Q.sketch_selections()))
def test_sketch_selections(name):
    """Q2 and Q5 over exactly the expectations the GPU module asks for by name"""
    N, S, K, mc, cls, cap, sel = Q.sketch_selections()[name]
    check_selection(sel, N, cap, name)
    assert sel[1].shape == (N, cap)


@pytest.mark.parametrize("name", sorted(Q.sketch_clusterings()))
def test_sketch_clusterings(name):
    """Q3 and Q5, likewise"""
    N, S, mc, cls, assign = Q.sketch_clusterings()[name]
    assert mc == S // 4 and assign.size == N
    check_clustering(assign, name)


def test_the_class_table_is_an_input_that_matters():
    """Q1 for the one device input of the sketch side, in both of its users"""
    cnt = Q.sketches(Q.SK_N, Q.SK_S)[1]
    a = Q.selection(cnt, Q.SK_K, 1, Q.cls_real(Q.SK_S), Q.SK_CAP)
    b = Q.selection(cnt, Q.SK_K, 1, Q.cls_decoy_select(Q.SK_S), Q.SK_CAP)
    f = Q.differing_fraction(a, b)
    print("selection, class table A against the decoy:", f)
    assert f >= 0.25 and Q.nnz_of(b) == 0
    plain = Q.selection(cnt, Q.SK_K, 1, None, Q.SK_CAP)
    assert Q.nnz_of(a) > Q.nnz_of(plain), "the classes of four counts list nobody that the identity would not"
    mc = Q.dedup_min_count(Q.SK_S, Q.cls_real(Q.SK_S))
    assert mc == Q.SK_S // 4
    ca = Q.clustering(cnt, Q.SK_S, Q.cls_real(Q.SK_S), mc)
    cb = Q.clustering(cnt, Q.SK_S, Q.cls_decoy_dedup(Q.SK_S), mc)
    f = Q.differing_fraction([ca], [cb])
    print("clustering, class table A against the decoy:", f)
    assert f >= 0.25 and (cb == np.arange(Q.SK_N)).all()
    assert a[0].tobytes() == Q.sketch_selections()["classed topk 257"][6][0].tobytes()
    assert ca.tobytes() == Q.sketch_clusterings()["classed clusters 257"][4].tobytes()


# ---------------------------------------------------------------- 2. codes
def test_code_sets():
    a, b = Q.code_expect("A"), Q.code_expect("B")
    for name in ("topk", "threshold"):
        check_selection(a[name], Q.CODE_N, Q.CODE_CAP, "codes " + name)
        f = Q.differing_fraction(a[name], b[name])
        print("codes", name, "A against B:", f)
        assert f >= 0.25
    for name in ("eq", "gt", "lt"):
        f = Q.differing_fraction([a[name]], [b[name]])
        print("codes", name, "A against B:", f)
        assert f >= 0.25 and not (a[name] == P32).any()
    np.testing.assert_array_equal(a["eq"].astype(np.int64) + a["gt"] + a["lt"], Q.CODE_S)


# ---------------------------------------------------------------- 3. exact sets
@pytest.mark.parametrize("weighted", [False, True], ids=["set", "countdict"])
def test_exact_sets(weighted):
    a, b = Q.exact_expect("A", weighted), Q.exact_expect("B", weighted)
    for k, name in enumerate(("triangle", "square")):
        f = Q.differing_fraction([a[k]], [b[k]])
        print("exact", name, "A against B:", f)
        assert f >= 0.25 and not (a[k] == P64).any()
    assert a[1][0, 1] == 3980 and a[1][0, 3] == 0                                   # the batch of test_gpu_exact_cmp.py
    h = Q.host_expect(weighted)
    assert (h[0] > 0).sum() >= h[0].size // 2 and not (h[0] == P64).any() and not (h[1] == P64).any()
    assert max(len(k) for k, _ in Q.host_sets()) <= 2500 and len(Q.host_sets()) == Q.HOST_SETS


# ---------------------------------------------------------------- 4. edit distances
def test_the_edit_set_has_every_class_and_alternating_routes():
    """Q4"""
    recs, d = Q.edit_set()
    lens = [len(r) for r in recs]
    sigma = len(set(b"".join(recs)))
    assert sigma == 4 and 44 <= len(recs) <= 50 and min(lens) >= 1
    assert any(n <= 32 for n in lens) and any(33 <= n <= 256 for n in lens) and any(n >= 289 for n in lens)
    classes = {s: sorted({Q.launch_class(n, s) for n in lens}) for s in (2, Q.EDIT_STRIP_ALL)}
    print("launch classes by strip:", classes)
    assert classes[Q.EDIT_STRIP_ALL] == [0, 1, 2]
    assert classes[2] == [0, 2]                                                       # class 1 needs 8 < blocks <= strip
    changes = {T: Q.route_changes(lens, sigma, T) for T in Q.NEAR_BOUNDS}
    print("route changes along the rows:", changes)
    assert changes[7] >= 3 and changes[32] == 0
    full = [n for n in lens if not Q.near_takes_the_band_route(n, sigma, 7)]
    assert full and all(9 <= n <= 32 for n in full)
    # ... and inside every band of within_dev (7 rows) and of dedup_dev (16 rows) there is at least one band with both routes
    for band in (Q.WITHIN_BAND, Q.EDIT_DEDUP_BAND):
        assert any(Q.route_changes(lens[a:a + band], sigma, 7) for a in range(0, len(lens), band))


def test_edit_expectations():
    recs, d = Q.edit_set()
    n = len(recs)
    assert not (Q.edit_triangle() == P32).any() and not (Q.edit_rect() == P32).any()
    assert np.unique(Q.edit_triangle()).size > 50
    for T in Q.NEAR_BOUNDS:
        c = Q.near(T)
        assert 0 < int((c > 0).sum()) - n < n * (n - 1) and c.max() == T + 1 and not (c == Q.POISON).any()
    for K, T in Q.WITHIN_MODES:
        check_selection(Q.within(K, T), n, Q.WITHIN_CAP, f"within K {K} T {T}")
    for T in (3, 32):
        check_clustering(Q.edit_clusters(T), f"edit clustering T {T}")
    assert Q.n_clusters(Q.edit_clusters(3)) != Q.n_clusters(Q.edit_clusters(32))
