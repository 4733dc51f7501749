"""cmp --topk / --similarity-threshold, the parts that need no GPU: the checker itself (tests/knn_ref.py: the contract against
the reference's heap loop), d2g_knn_finish, the CSR file format and the CLI's refusals."""
import os
import subprocess

import numpy as np
import pytest

import knn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tied_matrix(rng, N, levels):
    v = rng.integers(0, levels, (N, N)).astype(np.float32) / np.float32(levels)
    return v


@pytest.mark.parametrize("isdist", [False, True])
def test_heap_is_a_subset_of_the_intended_lists_with_the_same_first_k(isdist):
    """F12: on rows with heavy ties the reference's heap loop loses some neighbours tied with the K-th best -- never anything
    else: its list is a subset of the intended one, and the first K values are the same"""
    rng = np.random.default_rng(20260 + isdist)
    differ = rows = 0
    for trial in range(12):
        N = int(rng.integers(8, 40))
        v = _tied_matrix(rng, N, int(rng.integers(2, 6)))
        for K in (1, 2, 5, N - 1, N + 3):
            a = R.csr_rows(R.knn_reference_heap(v, K=K, isdist=isdist))
            b = R.csr_rows(R.knn_intended(v, K=K, isdist=isdist))
            for (ai, ad), (bi, bd) in zip(a, b):
                rows += 1
                assert set(ai.tolist()) <= set(bi.tolist())
                assert np.array_equal(ad[:K], bd[:K])
                assert len(ai) >= min(K, len(bi))
                differ += len(ai) != len(bi)
    assert 0 < differ < rows          # the defect is real, and it is not every row


@pytest.mark.parametrize("isdist", [False, True])
def test_heap_equals_intended_on_distinct_values(isdist):
    rng = np.random.default_rng(7 + isdist)
    for N in (2, 9, 33):
        v = (rng.permutation(N * N).reshape(N, N) + 1).astype(np.float32) / np.float32(N * N + 1)
        for K in (1, 3, N - 1, N + 2):
            R.assert_csr_equal(R.knn_reference_heap(v, K=K, isdist=isdist), R.knn_intended(v, K=K, isdist=isdist), f"N={N} K={K}")
        for T in (0.25, 0.5):
            R.assert_csr_equal(R.knn_reference_heap(v, T=T, isdist=isdist), R.knn_intended(v, T=T, isdist=isdist), f"N={N} T={T}")


def test_frozen_case_2_2_1():
    """row values (2, 2, 1), K = 2, smaller is better: the heap gives {1, 2(id 0)}, the stated intent {1, 2(id 0), 2(id 1)}"""
    v = np.zeros((4, 4), np.float32)
    v[3, :3] = (2, 2, 1)
    v[:3] = 9
    heap = R.csr_rows(R.knn_reference_heap(v, K=2, isdist=True))[3]
    want = R.csr_rows(R.knn_intended(v, K=2, isdist=True))[3]
    assert heap[0].tolist() == [2, 0] and heap[1].tolist() == [1.0, 2.0]
    assert want[0].tolist() == [2, 0, 1] and want[1].tolist() == [1.0, 2.0, 2.0]


def test_thresholds_have_no_zero_rule_and_no_trimming():
    v = np.array([[0, 0.5, 0.25], [0.5, 0, 0.75], [0.25, 0.75, 0]], np.float32)
    got = R.csr_rows(R.knn_intended(v, T=0.25))
    assert [g[0].tolist() for g in got] == [[1, 2], [2, 0], [1, 0]]
    got = R.csr_rows(R.knn_intended(v, T=0.5, isdist=True))
    assert [g[0].tolist() for g in got] == [[2, 1], [0], [0]]


# ---- d2g_knn_finish --------------------------------------------------------------------------------------------------
def _candidates(cnt, K, T, lut, isdist, cap=None):
    """what the device hands over for a count matrix (the contract on counts), padded with junk behind every row's entries"""
    cls = R.class_table(lut)
    m = R.min_count_for(lut, K=K, T=T, isdist=isdist)
    rowcnt, mask = R.select_by_count(cnt, K or 0, m, cls if K else None)
    N = cnt.shape[0]
    cap = int(max(1, rowcnt.max())) if cap is None else cap
    ids = np.full((N, cap), 0xDEADBEEF, np.uint32)
    cts = np.full((N, cap), 0xDEADBEEF, np.uint32)
    for i in range(N):
        js = np.nonzero(mask[i])[0][:cap]
        ids[i, :js.size] = js
        cts[i, :js.size] = cnt[i, js]
    return rowcnt, ids, cts, cap


@pytest.mark.parametrize("isdist", [False, True])
def test_knn_finish_against_the_contract(d2g, isdist):
    """synthetic candidate lists -> CSR: empty rows, a table that merges two counts into one value, inf distances"""
    S = 12
    rng = np.random.default_rng(99 + isdist)
    if isdist:      # non-increasing, inf at count 0, counts 7 and 8 share a value
        lut = np.array([np.inf, 3.0, 2.5, 2.0, 1.75, 1.5, 1.25, 1.0, 1.0, 0.5, 0.25, 0.125, 0.0], np.float32)
    else:           # non-decreasing, 0 at counts 0 and 1, counts 5 and 6 share a value
        lut = np.array([0, 0, 0.1, 0.2, 0.3, 0.45, 0.45, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0], np.float32)
    for N in (1, 2, 17, 40):
        cnt = rng.integers(0, S + 1, (N, N))
        cnt[rng.random((N, N)) < 0.5] = 0                      # many pairs share nothing
        if N > 3:
            cnt[3, :] = 0                                      # an empty row for similarities
        values = lut[cnt]
        for K, T in ((1, None), (2, None), (5, None), (N + 4, None), (None, 0.45), (None, 1.0), (None, 1e-6), (None, 100.0)):
            rowcnt, ids, cts, cap = _candidates(cnt, K, T, lut, isdist)
            got = d2g.knn_finish(rowcnt, ids, cts, cap, lut, isdist)
            R.assert_csr_equal(got, R.knn_intended(values, K=K, T=T, isdist=isdist), f"N={N} K={K} T={T}")


def test_knn_finish_reports_rows_beyond_their_slots_and_short_outputs(d2g):
    lib = d2g.lib()
    lut = np.linspace(0, 1, 5).astype(np.float32)
    rowcnt = np.array([2, 5, 0], np.uint32)                    # row 1 holds 5 candidates, its slots 3
    ids = np.array([4, 7, 99, 1, 2, 3, 0, 0, 0], np.uint32)
    cts = np.array([1, 4, 77, 2, 2, 3, 0, 0, 0], np.uint32)   # 77 > S sits behind row 0's entries: never read
    with pytest.raises(d2g.KnnOverflow) as e:
        d2g.knn_finish(rowcnt, ids, cts, 3, lut)
    assert e.value.rows == 1
    import ctypes as C
    indptr = np.full(4, 7, np.uint64)
    over, need = C.c_size_t(99), C.c_size_t(99)
    rc = lib.d2g_knn_finish(rowcnt.ctypes.data, ids.ctypes.data, cts.ctypes.data, 3, 3, lut.ctypes.data, 4, 0, indptr.ctypes.data, None, None, 0,
                            C.byref(need), C.byref(over))
    assert rc == -1 and over.value == 1 and indptr.tolist() == [7, 7, 7, 7]     # nothing else written
    rowcnt[1] = 3
    indices, data = np.full(6, 0xABCD, np.uint32), np.full(6, -5, np.float32)
    rc = lib.d2g_knn_finish(rowcnt.ctypes.data, ids.ctypes.data, cts.ctypes.data, 3, 3, lut.ctypes.data, 4, 0, indptr.ctypes.data,
                            indices.ctypes.data, data.ctypes.data, 4, C.byref(need), C.byref(over))
    assert rc == -4 and need.value == 5 and over.value == 0 and indptr.tolist() == [0, 2, 5, 5]    # D2G_ERR_NOMEM: capacity 4, 5 needed
    assert np.all(indices == 0xABCD) and np.all(data == -5)
    rc = lib.d2g_knn_finish(rowcnt.ctypes.data, ids.ctypes.data, cts.ctypes.data, 3, 3, lut.ctypes.data, 4, 0, indptr.ctypes.data,
                            indices.ctypes.data, data.ctypes.data, 5, C.byref(need), C.byref(over))
    assert rc == 0 and indices.tolist() == [7, 4, 3, 1, 2, 0xABCD] and data[:5].tolist() == [1.0, 0.25, 0.75, 0.5, 0.5] and data[5] == -5
    cts[3] = 5                                                 # a count above S inside a row's entries is refused
    assert lib.d2g_knn_finish(rowcnt.ctypes.data, ids.ctypes.data, cts.ctypes.data, 3, 3, lut.ctypes.data, 4, 0, indptr.ctypes.data,
                              indices.ctypes.data, data.ctypes.data, 6, None, None) == -1


def test_csr_bytes_round_trip():
    rng = np.random.default_rng(5)
    v = _tied_matrix(rng, 23, 4)
    v[7] = 0                                                   # an empty row
    for csr in (R.knn_intended(v, K=3), R.knn_intended(v, T=0.5), R.knn_intended(v[:1, :1], K=1)):
        b = R.csr_bytes(csr)
        assert len(b) == 16 + 8 * csr[0].size + 8 * csr[1].size
        R.assert_csr_equal(R.read_csr_bytes(b), csr)
    names = ["g%d" % i for i in range(23)]
    text = R.knn_text(R.knn_intended(v, K=2), names)
    lines = text.split(b"\n")
    assert lines[0] + b"\n" == R.HEADER_TEXT and lines[8] == b"g7" and len(lines) == 25 and lines[1].startswith(b"g0\tg")


# ---- the CLI's refusals: all before a GPU context exists (this test runs without a GPU) --------------------------
def _cli(*args):
    exe = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


@pytest.fixture(scope="module")
def stacked(tmp_path_factory):
    """presketched stacks: S = 64 and S = 100 (u64 N, u64 S, f64 cards, f64 registers)"""
    d = tmp_path_factory.mktemp("knn_cli")
    out = {}
    for S in (64, 100):
        p = d / f"stack{S}.bin"
        sig = R.family_sigs(6, S, seed=S)
        with open(p, "wb") as f:
            f.write(np.array([6, S], np.uint64).tobytes() + np.ones(6).tobytes() + sig.tobytes())
        out[S] = str(p)
    return out


def test_cli_refuses_both_flags_with_the_reference_text(stacked):
    r = _cli("cmp", "--presketched", stacked[64], "--topk", "3", "--similarity-threshold", "0.5")
    assert r.returncode == 1
    assert "Exception invalid: nn > 0 and minsim > 0. Pick either top-k or minimum similarity. (Can't do both.)" in r.stderr   # cmp_main.h:103


@pytest.mark.parametrize("extra,word", [
    (["--topk", "0"], "K >= 1"), (["--top-k", "-2"], "K >= 1"),
    (["--similarity-threshold", "0"], "T > 0"), (["--similarity-threshold", "-0.5"], "T > 0"),
    (["--topk", "3", "--containment"], "cardinality"), (["--topk", "3", "--symmetric-containment"], "cardinality"),
    (["--topk", "3", "--intersection"], "cardinality"), (["--similarity-threshold", "0.5", "--union-size"], "cardinality"),
    (["--topk", "3", "--fastcmp", "4"], "--fastcmp"), (["--topk", "3", "--fastcmp", "2"], "--fastcmp"),
    (["--similarity-threshold", "0.5", "--fastcmp", "1", "--bbit-sigs"], "--fastcmp"),
    (["--topk", "3", "--square"], "--square"), (["--square", "--similarity-threshold", "0.5"], "--square"),
    (["--topk", "3", "--phylip"], "--phylip"),
])
def test_cli_refuses_out_of_scope_combinations(stacked, extra, word):
    r = _cli("cmp", "--presketched", stacked[64], *extra)
    assert r.returncode == 1, r.stderr
    assert "outside the hot-path scope" in r.stderr and word in r.stderr, r.stderr
    assert "gfx950" not in r.stderr                            # refused before a context was asked for


def test_cli_refuses_a_query_panel_and_non_power_of_two_set_sketches(stacked, tmp_path):
    q = tmp_path / "q.txt"
    q.write_text("x.fa\n")
    r = _cli("cmp", "--topk", "3", "-Q", str(q), "a.fa")
    assert r.returncode == 1 and "outside the hot-path scope" in r.stderr and "-Q" in r.stderr
    r = _cli("cmp", "--topk", "3", "-S", "100", "a.fa")           # set space, S = 100: the value needs (gt, lt)
    assert r.returncode == 1 and "outside the hot-path scope" in r.stderr and "power of two" in r.stderr
    r = _cli("cmp", "--presketched", stacked[100], "--similarity-threshold", "0.5")   # ... also when the size comes from the file
    assert r.returncode == 1 and "outside the hot-path scope" in r.stderr and "power of two" in r.stderr and "gfx950" not in r.stderr


def test_cli_sketch_topk_stays_refused_and_help_names_the_flags():
    r = _cli("sketch", "--topk", "3", "x.fa")
    assert r.returncode == 1 and "outside" in r.stderr
    r = _cli("sketch", "--similarity-threshold", "0.5", "x.fa")
    assert r.returncode == 1 and "outside" in r.stderr
    r = _cli("cmp", "-h")
    assert r.returncode == 1 and "--topk/--top-k K" in r.stderr and "--similarity-threshold T" in r.stderr
