"""K2e on the GPU: d2g_cmp_knn_dev against blocked NumPy equality counts + the contract on counts (tests/knn_ref.py), and d2g_cmp_knn
end to end against knn_intended on the oracle's floats.  The shapes are small so that every seam of the selection kernel is inside
them: N in {67, 257, 1000} is no multiple of the wave (64), the workgroup (256) or a wave's quarter of the row; band_rows in
{1, 33, default} cuts the rows into bands; S = 8192 takes the bisection instead of the LDS histogram (S <= 4096)."""
import numpy as np
import pytest

import knn_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xDEADBEEF


class Matrix:
    """a planted matrix, its NumPy counts (computed once, never changed) and the device sets made from it"""
    def __init__(self, sigs):
        self.sigs = np.ascontiguousarray(sigs, np.float64)
        self.N, self.S = self.sigs.shape
        self.cnt = R.eqcounts(self.sigs.view(np.uint64))
        self.cnt.setflags(write=False)
        self.sets = {}

    def set(self, ctx, D, algo):
        if algo not in self.sets:
            self.sets[algo] = ctx.cmp_set(self.sigs.view(np.uint64), algo=algo)
        return self.sets[algo]


_CACHE = {}


def matrix(kind, N, S):
    key = (kind, N, S)
    if key not in _CACHE:
        if kind == "families":
            sigs = R.family_sigs(N, S, seed=N * 7 + S)
        elif kind == "identical":
            sigs = np.tile(R.family_sigs(1, S, seed=3), (N, 1))
        elif kind == "unrelated":
            sigs = R.unrelated_sigs(N, S, seed=11)
        elif kind == "duplicates":
            # one sketch copied to positions on both sides of a band seam (33), of a wave's share of the row and of a 64-column step
            sigs = R.unrelated_sigs(N, S, seed=12)
            for j in DUP_POS(N):
                sigs[j] = sigs[0]
        _CACHE[key] = Matrix(sigs)
    return _CACHE[key]


def DUP_POS(N):
    q = (N + 255) // 256 * 64                                   # columns per wave of the selection kernel
    return sorted({0, 32, 33, 63, 64, q - 1, q, 2 * q - 1, 2 * q, N - 1} & set(range(N)))


def run_dev(ctx, cs, K, min_count, cls, cap, r0, r1, band_rows):
    """d2g_cmp_knn_dev into guarded buffers -> (rowcnt, ids [n][cap], counts [n][cap]); the guard words must be untouched"""
    n = r1 - r0
    nslot = n * cap
    bufs = []
    for words in (n, nslot, nslot):
        p = ctx.malloc((words + GUARD) * 4)
        ctx.h2d(p, np.full(words + GUARD, FILL, np.uint32))
        bufs.append((p, words))
    d_cls = None
    if cls is not None:
        d_cls = ctx.malloc(cls.size * 4)
        ctx.h2d(d_cls, np.ascontiguousarray(cls, np.uint32))
    try:
        cs.knn_dev(bufs[0][0], bufs[1][0], bufs[2][0], cap, K=K, min_count=min_count, cls_dev_ptr=d_cls, r0=r0, r1=r1, band_rows=band_rows)
        ctx.sync()
        out = []
        for p, words in bufs:
            a = np.empty(words + GUARD, np.uint32)
            ctx.d2h(a, p)
            assert np.all(a[words:] == FILL), "guard words behind an output buffer were written"
            out.append(a[:words])
    finally:
        for p, _ in bufs:
            ctx.free(p)
        if d_cls is not None:
            ctx.free(d_cls)
    return out[0], out[1].reshape(n, cap), out[2].reshape(n, cap)


_EXPECTED = {}


def expected_dev(cnt, K, min_count, cls, cap, r0, r1):
    """the contract on counts, computed once per case (the same expectation serves every algorithm and band size)"""
    key = (id(cnt), K, min_count, None if cls is None else cls.tobytes(), cap, r0, r1)
    if key not in _EXPECTED:
        exp_cnt, mask = R.select_by_count(cnt, K, min_count, cls, r0, r1)
        # expected slots: the listed columns in ascending j, cut at cap; everything behind them still holds the fill
        order = np.argsort(~mask, axis=1, kind="stable")[:, :cap]
        if order.shape[1] < cap:
            order = np.pad(order, ((0, 0), (0, cap - order.shape[1])))
        used = np.arange(cap)[None, :] < np.minimum(exp_cnt, cap)[:, None]
        exp_ids = np.where(used, order, FILL).astype(np.uint32)
        exp_cts = np.where(used, np.take_along_axis(np.asarray(cnt[r0:r1]), order, axis=1), FILL).astype(np.uint32)
        _EXPECTED[key] = (exp_cnt, exp_ids, exp_cts)
    return _EXPECTED[key]


def check_dev(ctx, cs, cnt, K, min_count, cls, cap, r0=0, r1=None, band_rows=0, what=""):
    N = cnt.shape[0]
    r1 = N if r1 is None else r1
    exp_cnt, exp_ids, exp_cts = expected_dev(cnt, K, min_count, cls, cap, r0, r1)
    rowcnt, ids, cts = run_dev(ctx, cs, K, min_count, cls, cap, r0, r1, band_rows)
    assert np.array_equal(rowcnt, exp_cnt), f"{what}: rowcnt differs (the true number, also beyond cap)"
    assert np.array_equal(ids, exp_ids), f"{what}: ids differ (ascending j inside a row, nothing past a row's entries)"
    assert np.array_equal(cts, exp_cts), f"{what}: counts differ"
    return rowcnt


def lut_and_classes(D, S, measure):
    lut = D.epilogue_lut(S, measure, 31, False)
    return lut, R.class_table(lut)


@pytest.mark.parametrize("S", [64, 128, 1024])
@pytest.mark.parametrize("N", [67, 257, 1000])
def test_knn_dev_families(gpu_ctx, d2g, N, S):
    """top-K at K in {1, 5, 64, N - 1, N + 10} and three thresholds, bands of 1 / 33 / default rows, a partial row range, on
    bit-sliced and direct sets: rowcnt, ids and counts exact, guard words untouched with a cap that is too small"""
    m = matrix("families", N, S)
    lut, cls = lut_and_classes(d2g, S, d2g.SIMILARITY)
    for algo in (d2g.CMP_BITSLICE, d2g.CMP_DIRECT):
        cs = m.set(gpu_ctx, d2g, algo)
        assert cs.algo == algo
        for band in (1, 33, 0):
            for K in (1, 5, 64, N - 1, N + 10):
                for min_count in ((1, 0) if band == 33 else (1,)):  # similarities / distances
                    check_dev(gpu_ctx, cs, m.cnt, K, min_count, cls, cap=min(N - 1, K + 8), band_rows=band, what=f"algo {algo} band {band} K {K} m {min_count}")
            for t in (0, S // 4, S + 1):                            # everybody passes / some / nobody
                check_dev(gpu_ctx, cs, m.cnt, 0, t, None, cap=N - 1 if t else 40, band_rows=band, what=f"algo {algo} band {band} threshold {t}")
        # a row range that is not the whole matrix, a cap far too small, counting only (cap = 0)
        check_dev(gpu_ctx, cs, m.cnt, 5, 1, cls, cap=3, r0=13, r1=N - 7, band_rows=33, what=f"algo {algo} rows 13..N-7")
        check_dev(gpu_ctx, cs, m.cnt, 0, 1, None, cap=1, r0=N - 3, r1=N, band_rows=0, what=f"algo {algo} last rows")
        n = N - 20
        p = gpu_ctx.malloc(n * 4)
        try:
            cs.knn_dev(p, None, None, 0, K=7, min_count=1, r0=20, r1=N)
            got = np.empty(n, np.uint32)
            gpu_ctx.d2h(got, p)
        finally:
            gpu_ctx.free(p)
        assert np.array_equal(got, R.select_by_count(m.cnt, 7, 1, None, 20, N)[0])


def test_knn_dev_class_table_merges_counts(gpu_ctx, d2g):
    """two counts with one value: the K-th best's tie class spans both, t is lowered to the class minimum"""
    N, S = 257, 64
    m = matrix("families", N, S)
    cs = m.set(gpu_ctx, d2g, d2g.CMP_BITSLICE)
    cls = np.arange(S + 1, dtype=np.uint32)
    cls[:] = cls // 4 * 4                                           # classes of four counts
    for K in (1, 5, 64):
        for min_count in (0, 1, 6):
            with_cls = check_dev(gpu_ctx, cs, m.cnt, K, min_count, cls, cap=N - 1, band_rows=33, what=f"classes K {K} m {min_count}")
            without = R.select_by_count(m.cnt, K, min_count, None)[0]
            assert np.all(with_cls >= without)
    assert np.any(R.select_by_count(m.cnt, 5, 1, cls)[0] > R.select_by_count(m.cnt, 5, 1, None)[0])   # the table matters on this matrix


@pytest.mark.parametrize("kind", ["identical", "unrelated", "duplicates"])
def test_knn_dev_degenerate_matrices(gpu_ctx, d2g, kind):
    """all identical: N - 1 ties in every row, far beyond cap; all unrelated: nothing for similarities, everything (count 0, tied)
    for distances; duplicates of one sketch on both sides of the band and wave seams list each other -- self is excluded by index"""
    N, S = 257, 128
    m = matrix(kind, N, S)
    _, cls = lut_and_classes(d2g, S, d2g.SIMILARITY)
    for algo in (d2g.CMP_BITSLICE, d2g.CMP_DIRECT):
        cs = m.set(gpu_ctx, d2g, algo)
        for band in (1, 33, 0):
            for K, min_count, cap in ((1, 1, 4), (5, 1, 16), (5, 0, 16), (N + 10, 0, N - 1)):
                rowcnt = check_dev(gpu_ctx, cs, m.cnt, K, min_count, cls, cap, band_rows=band, what=f"{kind} algo {algo} band {band} K {K} m {min_count}")
                if kind == "identical":
                    assert np.all(rowcnt == N - 1)
                if kind == "unrelated":
                    assert np.all(rowcnt == (0 if min_count else N - 1))
                if kind == "duplicates" and min_count == 1:
                    dup = DUP_POS(N)
                    assert np.all(rowcnt[dup] == len(dup) - 1) and rowcnt.sum() == len(dup) * (len(dup) - 1)
            check_dev(gpu_ctx, cs, m.cnt, 0, S, None, cap=8, band_rows=band, what=f"{kind} algo {algo} band {band} threshold S")


@pytest.mark.parametrize("S", [4096, 8192])
def test_knn_dev_histogram_and_bisection_forms(gpu_ctx, d2g, S):
    """S = 4096 is the largest sketch the LDS histogram takes, S = 8192 selects t by bisection on the count"""
    N = 67
    m = matrix("families", N, S)
    cls = np.arange(S + 1, dtype=np.uint32)
    cs = m.set(gpu_ctx, d2g, d2g.CMP_BITSLICE)
    for K in (1, 5, 64, N - 1, N + 10):
        for min_count in (1, 0, S // 2):
            check_dev(gpu_ctx, cs, m.cnt, K, min_count, cls, cap=N - 1, band_rows=33, what=f"S {S} K {K} m {min_count}")
    for kind in ("identical", "unrelated"):
        mm = matrix(kind, N, S)
        cs2 = mm.set(gpu_ctx, d2g, d2g.CMP_DIRECT)
        for K, min_count in ((3, 1), (3, 0), (N + 10, 0)):
            check_dev(gpu_ctx, cs2, mm.cnt, K, min_count, None, cap=5, what=f"S {S} {kind} K {K} m {min_count}")


def test_knn_dev_code_plane_sets(gpu_ctx, d2g):
    """a set of 1-byte codes (D2G_CMP_PLANES): counts only, against NumPy counts of the codes"""
    rng = np.random.default_rng(8)
    N, S = 257, 100
    codes = rng.integers(0, 4, (N, S)).astype(np.uint8)             # four code values: heavy ties
    codes[40:60] = codes[40]
    cnt = R.eqcounts(codes)
    cs = gpu_ctx.cmp_set_codes(codes)
    assert cs.algo == d2g.CMP_PLANES
    for band in (1, 33, 0):
        for K, min_count in ((1, 0), (5, 1), (64, 0), (N + 10, 0)):
            check_dev(gpu_ctx, cs, cnt, K, min_count, None, cap=80, band_rows=band, what=f"codes band {band} K {K}")
        check_dev(gpu_ctx, cs, cnt, 0, 30, None, cap=N - 1, band_rows=band, what=f"codes band {band} threshold")
    cs.close()


def test_knn_dev_rejects_bad_arguments(gpu_ctx, d2g):
    m = matrix("families", 67, 64)
    cs = m.set(gpu_ctx, d2g, d2g.CMP_BITSLICE)
    p = gpu_ctx.malloc(67 * 4)
    try:
        with pytest.raises(d2g.D2GError):
            cs.knn_dev(p, None, None, 4, K=1, min_count=1)          # cap > 0 without candidate buffers
        with pytest.raises(d2g.D2GError):
            cs.knn_dev(p, p, p, 1, K=1, r0=5, r1=68)                # rows past N
        with pytest.raises(d2g.D2GError):
            cs.knn(np.linspace(1, 0, 65, dtype=np.float32), isdist=False, K=3)          # a table that is not monotone the right way
        with pytest.raises(d2g.D2GError):
            cs.knn(np.linspace(0, 1, 65, dtype=np.float32), isdist=False, K=3, threshold=0.5)   # both modes
        with pytest.raises(d2g.D2GError):
            gpu_ctx.cmp_knn(m.sigs.view(np.uint64), K=3, measure=d2g.CONTAINMENT)
    finally:
        gpu_ctx.free(p)


# ---- end to end: d2g_cmp_knn against knn_intended on the oracle's floats -----------------------------------------------
_VALUES = {}


def oracle_values(oracle, m, measure):
    key = (id(m), measure)
    if key not in _VALUES:
        v = R.oracle_values(oracle, m.sigs, measure, k=31)
        v.setflags(write=False)
        _VALUES[key] = v
    return _VALUES[key]


@pytest.mark.parametrize("S", [64, 128, 1024])
@pytest.mark.parametrize("N", [67, 257, 1000])
def test_cmp_knn_end_to_end_families(gpu_ctx, d2g, oracle, N, S):
    """indices equal, values at 0 ulp, for Jaccard similarity and Mash distance; caps small enough to force the re-run of rows"""
    m = matrix("families", N, S)
    for measure, isdist in ((d2g.SIMILARITY, False), (d2g.POISSON_LLR, True)):
        v = oracle_values(oracle, m, measure)
        for K in ((1, 5, 64, N - 1, N + 10) if N <= 257 else (1, 5, N + 10)):
            got = gpu_ctx.cmp_knn(m.sigs.view(np.uint64), K=K, measure=measure, k=31, cap=3 if K == 5 else 0, band_rows=33 if K == 1 else 0)
            R.assert_csr_equal(got, R.knn_intended(v, K=K, isdist=isdist), f"measure {measure} K {K}")
        for T in ((0.3, 2.0) if not isdist else (0.05, float("inf"), 1e-12)):     # some / nobody; some / everybody / nobody
            got = gpu_ctx.cmp_knn(m.sigs.view(np.uint64), threshold=T, measure=measure, k=31, cap=2)
            R.assert_csr_equal(got, R.knn_intended(v, T=T, isdist=isdist), f"measure {measure} T {T}")
    # a row range, the direct kernel
    got = gpu_ctx.cmp_knn(m.sigs.view(np.uint64), K=4, r0=9, r1=N - 5, algo=d2g.CMP_DIRECT, cap=2, band_rows=1 if N == 67 else 33)
    R.assert_csr_equal(got, R.knn_intended(oracle_values(oracle, m, d2g.SIMILARITY), K=4, rows=(9, N - 5)), "row range")


@pytest.mark.parametrize("kind", ["identical", "unrelated", "duplicates"])
def test_cmp_knn_end_to_end_degenerate(gpu_ctx, d2g, oracle, kind):
    """identical sketches force the overflow and re-run path at any cap < N - 1; unrelated ones give empty similarity lists and, for
    Mash distance, rows that list everybody at inf; duplicates list each other"""
    N, S = 257, 128
    m = matrix(kind, N, S)
    for measure, isdist in ((d2g.SIMILARITY, False), (d2g.POISSON_LLR, True)):
        v = oracle_values(oracle, m, measure)
        for K, cap in ((1, 0), (5, 7), (N + 10, 0)):
            got = gpu_ctx.cmp_knn(m.sigs.view(np.uint64), K=K, measure=measure, cap=cap)
            exp = R.knn_intended(v, K=K, isdist=isdist)
            R.assert_csr_equal(got, exp, f"{kind} measure {measure} K {K}")
            if kind == "identical" or (kind == "unrelated" and isdist):
                assert exp[1].size == N * (N - 1)
            if kind == "unrelated" and not isdist:
                assert exp[1].size == 0
        T = 1.0 if not isdist else 1e-30                              # identical sketches: everybody passes
        got = gpu_ctx.cmp_knn(m.sigs.view(np.uint64), threshold=T, measure=measure, cap=3)
        R.assert_csr_equal(got, R.knn_intended(v, T=T, isdist=isdist), f"{kind} measure {measure} T {T}")


def test_cmp_knn_multiset_space_any_sketch_size(gpu_ctx, d2g, oracle):
    """--multiset: the value is a function of the equality count at any S; set space at the same S is refused"""
    N, S = 67, 100
    m = matrix("families", N, S)
    v = R.oracle_values(oracle, m.sigs, d2g.SIMILARITY, k=31, multiset=True)
    got = gpu_ctx.cmp_knn(m.sigs.view(np.uint64), K=5, multiset_space=True)
    R.assert_csr_equal(got, R.knn_intended(v, K=5), "multiset S=100")
    with pytest.raises(d2g.D2GError):
        gpu_ctx.cmp_knn(m.sigs.view(np.uint64), K=5, multiset_space=False)


def test_knn_kernel_is_timed(gpu_ctx, d2g):
    m = matrix("families", 257, 64)
    gpu_ctx.set_timing(d2g.TIME_KNN | d2g.TIME_K2)
    try:
        gpu_ctx.kernel_ms("knn")
        gpu_ctx.cmp_knn(m.sigs.view(np.uint64), K=5, band_rows=100)
        n = gpu_ctx.kernel_ms("knn")
    finally:
        gpu_ctx.set_timing(0)
    assert n[0] >= 3 and n[1] > 0                                   # three bands: at least three selection launches


# ---- rows longer than one trip of the selection kernel's unrolled loops ------------------------------------------------
# knn_select_kernel and count_at_least advance by UNROLL * THREADS = 1024 columns: N = 2500 takes two full trips and a third that
# is partly past the end of the row.  (Every matrix above has N <= 1000: one trip.)
LONG_N, LONG_S = 2500, 64


def long_matrix(shuffled):
    key = ("families-long", shuffled)
    if key not in _CACHE:
        sigs = R.family_sigs(LONG_N, LONG_S, seed=LONG_N * 7 + LONG_S)
        if shuffled:
            sigs = sigs[np.random.default_rng(LONG_N + LONG_S).permutation(LONG_N)]
        _CACHE[key] = Matrix(sigs)
    return _CACHE[key]


@pytest.mark.parametrize("shuffled", [False, True], ids=["generator-order", "shuffled"])
def test_knn_dev_rows_of_more_than_one_trip(gpu_ctx, d2g, shuffled):
    """top-K at K in {1, 5, 64}, the thresholds S / 4 and 0, bands of 33 rows and the default, a row range that starts past column
    1024, on bit-sliced and direct sets.  In generator order a family is a run of neighbouring rows, so every row from 1024 on
    lists columns of the second or third trip; after the shuffle the rows below 1024 do too."""
    N, S = LONG_N, LONG_S
    m = long_matrix(shuffled)
    _, cls = lut_and_classes(d2g, S, d2g.SIMILARITY)
    listed = R.select_by_count(m.cnt, 5, 1, cls)[1]
    assert listed[:, 1024:2048].any(axis=1).sum() >= 400 and listed[:, 2048:].any(axis=1).sum() >= 400
    assert listed[:1024, 1024:].any(axis=1).sum() >= (500 if shuffled else 1)
    for algo in (d2g.CMP_BITSLICE, d2g.CMP_DIRECT):
        cs = m.set(gpu_ctx, d2g, algo)
        assert cs.algo == algo
        for band in ((33, 0) if algo == d2g.CMP_BITSLICE else (0,)):
            for K in (1, 5, 64):
                check_dev(gpu_ctx, cs, m.cnt, K, 1, cls, cap=K + 8, band_rows=band, what=f"algo {algo} band {band} K {K}")
            check_dev(gpu_ctx, cs, m.cnt, 0, S // 4, None, cap=48, band_rows=band, what=f"algo {algo} band {band} threshold S / 4")
            check_dev(gpu_ctx, cs, m.cnt, 0, 0, None, cap=40, band_rows=band, what=f"algo {algo} band {band} threshold 0")
        check_dev(gpu_ctx, cs, m.cnt, 5, 1, cls, cap=3, r0=1030, r1=N - 7, band_rows=33, what=f"algo {algo} rows 1030..N-7")
