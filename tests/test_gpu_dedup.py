"""K2f on the GPU: d2g_cmp_dedup_dev / d2g_cmp_set_dedup against the restatement of the reference's loop (tests/dedup_ref.py) on values
count / S, and d2g_cmp_dedup end to end against the same loop on the oracle's floats.  The shapes are small so that every seam is
inside them: N in {67, 257, 1000} is no multiple of the wave (64) or the workgroup (256); band_rows in {1, 33, default} cuts the rows
into bands (default = 256 rows here: N = 257 and 1000 have a second band); every matrix is also clustered after a row shuffle, which
moves the representatives of a family into earlier bands than its members."""
import numpy as np
import pytest

import dedup_ref as R
import knn_ref as K

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xDEADBEEF
SHAPES = [(67, 64), (257, 128), (1000, 64), (257, 1024)]
THRESHOLDS = (0.1, 0.25, 0.5, 1.0)
BANDS = (1, 33, 0)


class Matrix:
    """a planted matrix, its NumPy counts (computed once, never changed) and the device sets made from it"""
    def __init__(self, sigs):
        self.sigs = np.ascontiguousarray(sigs, np.float64)
        self.N, self.S = self.sigs.shape
        self.cnt = K.eqcounts(self.sigs.view(np.uint64))
        self.cnt.setflags(write=False)
        self.values = (self.cnt / self.S).astype(np.float32)         # count / S as float32
        self.values.setflags(write=False)
        self.lut = (np.arange(self.S + 1) / self.S).astype(np.float32)
        self.sets = {}
        self.refs = {}

    def set(self, ctx, algo):
        if algo not in self.sets:
            self.sets[algo] = ctx.cmp_set(self.sigs.view(np.uint64), algo=algo)
        return self.sets[algo]

    def ref(self, T, values=None, tag="count"):
        """the reference's assignment, computed once per (values, T)"""
        if (tag, T) not in self.refs:
            ids, cons = R.dedup_reference(self.values if values is None else values, T)
            self.refs[(tag, T)] = R.assign_of(ids, cons, self.N)
        return self.refs[(tag, T)]


_CACHE = {}


def families(N, S, shuffled=False):
    key = ("families", N, S, shuffled)
    if key not in _CACHE:
        sigs = K.family_sigs(N, S, seed=N * 7 + S)
        if shuffled:
            sigs = sigs[np.random.default_rng(N + S).permutation(N)]
        _CACHE[key] = Matrix(sigs)
    return _CACHE[key]


def run_dev(ctx, cs, N, min_count, cls=None, band_rows=0):
    """d2g_cmp_dedup_dev into a guarded buffer -> assign [N]; the guard words behind it must be untouched"""
    p = ctx.malloc((N + GUARD) * 4)
    ctx.h2d(p, np.full(N + GUARD, FILL, np.uint32))
    d_cls = None
    if cls is not None:
        d_cls = ctx.malloc(cls.size * 4)
        ctx.h2d(d_cls, np.ascontiguousarray(cls, np.uint32))
    try:
        cs.dedup_dev(p, min_count, cls_dev_ptr=d_cls, band_rows=band_rows)
        ctx.sync()
        a = np.empty(N + GUARD, np.uint32)
        ctx.d2h(a, p)
    finally:
        ctx.free(p)
        if d_cls is not None:
            ctx.free(d_cls)
    assert np.all(a[N:] == FILL), "guard words behind assign_dev were written"
    return a[:N]


def min_count_of(lut, T):
    """the smallest count whose value reaches simt (float comparison), S + 1 if none does"""
    hit = np.nonzero(np.asarray(lut, np.float32) >= R.simt_of(T))[0]
    return int(hit[0]) if hit.size else int(len(lut))


def same(got, exp, what):
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{what}: {bad.size} sketches differ, first at {bad[0]}: got representative {got[bad[0]]}, expected {exp[bad[0]]}"


# the cases the issue names as exercising every property, in generator order (checked on the reference result alone)
CENSUS_CASES = {(67, 64): (0.1,), (257, 128): (0.1, 0.25), (1000, 64): (0.1, 0.25, 0.5)}


@pytest.mark.parametrize("shuffled", [False, True], ids=["generator-order", "shuffled"])
@pytest.mark.parametrize("N,S", SHAPES)
def test_dedup_families(gpu_ctx, d2g, N, S, shuffled):
    """assign exact against the reference's loop on count / S, for every band size and threshold, on bit-sliced and direct sets,
    through the device entry (guard words untouched) and the host-pointer entry"""
    m = families(N, S, shuffled)
    if not shuffled:
        for T in CENSUS_CASES.get((N, S), ()):
            c = R.census(m.values, T, 33)
            assert 2 <= c["clusters"] <= N - 1, c
            assert c["joins_earlier_band"] >= 1 and c["joins_same_band"] >= 1 and c["ties"] >= 1, c
            assert c["better_nonrep"] >= 1 and c["rep_despite_nonrep"] >= 1, c
    cls = K.class_table(m.lut)
    for algo in (d2g.CMP_BITSLICE, d2g.CMP_DIRECT):
        cs = m.set(gpu_ctx, algo)
        assert cs.algo == algo
        for band in (BANDS if algo == d2g.CMP_BITSLICE else (33,)):
            for T in THRESHOLDS:
                got = run_dev(gpu_ctx, cs, N, min_count_of(m.lut, T), cls if band else None, band)   # the identity table, given and NULL
                same(got, m.ref(T), f"dev algo {algo} band {band} T {T}")
        for T in THRESHOLDS:
            same(cs.dedup(m.lut, T, band_rows=33 if algo == d2g.CMP_DIRECT else 0), m.ref(T), f"set_dedup algo {algo} T {T}")


@pytest.mark.parametrize("shuffled", [False, True], ids=["generator-order", "shuffled"])
@pytest.mark.parametrize("N,S", SHAPES)
def test_cmp_dedup_end_to_end_families(gpu_ctx, d2g, oracle, N, S, shuffled):
    """d2g_cmp_dedup (upload, prepare, table, clustering) against the reference's loop on the oracle's floats: bit for bit"""
    m = families(N, S, shuffled)
    v = K.oracle_values(oracle, m.sigs, d2g.SIMILARITY, k=31)
    for T in THRESHOLDS:
        exp = m.ref(T, v, "oracle")
        same(gpu_ctx.cmp_dedup(m.sigs.view(np.uint64), T, band_rows=33 if T == 0.25 else 0), exp, f"T {T}")
    same(gpu_ctx.cmp_dedup(m.sigs.view(np.uint64), 0.0), m.ref(0.9, v, "oracle"), "T = 0: the default cut-off of 0.9")


def test_dedup_identical_and_unrelated(gpu_ctx, d2g):
    N, S = 257, 128
    one = Matrix(np.tile(K.family_sigs(1, S, seed=3), (N, 1)))
    none = Matrix(K.unrelated_sigs(N, S, seed=11))
    for band in BANDS:
        for T in (0.1, 1.0):
            got = run_dev(gpu_ctx, one.set(gpu_ctx, d2g.CMP_BITSLICE), N, min_count_of(one.lut, T), None, band)
            assert np.all(got == 0) and np.all(one.ref(T) == 0)
        got = run_dev(gpu_ctx, none.set(gpu_ctx, d2g.CMP_BITSLICE), N, 1, None, band)          # any shared register would join
        assert np.array_equal(got, np.arange(N)) and np.array_equal(none.ref(1 / S), np.arange(N))


def _planted(N, S, seed, shares):
    """unrelated sketches, then for every (b, a, regs): sketch b takes the registers `regs` of sketch a AS IT IS BY THEN"""
    sigs = K.unrelated_sigs(N, S, seed=seed)
    for b, a, regs in shares:
        sigs[b, regs] = sigs[a, regs]
    return Matrix(sigs)


def test_dedup_duplicates_across_the_seams(gpu_ctx, d2g):
    """copies of sketch 0 on both sides of the band seam (32 / 33), of the 64-column step of a wave and of the 256-row band, and
    copies of a representative that is not the first sketch: each joins its original at T = 1"""
    N, S = 300, 64
    every = slice(0, S)
    pos0, pos40 = (32, 33, 63, 64, 255, 256, 257, 299), (70, 260)
    m = _planted(N, S, 12, [(b, 0, every) for b in pos0] + [(b, 40, every) for b in pos40])
    exp = np.arange(N)
    exp[list(pos0)] = 0
    exp[list(pos40)] = 40
    assert np.array_equal(m.ref(1.0), exp)
    for algo in (d2g.CMP_BITSLICE, d2g.CMP_DIRECT):
        for band in BANDS + (64,):
            same(run_dev(gpu_ctx, m.set(gpu_ctx, algo), N, S, None, band), exp, f"algo {algo} band {band}")


def test_dedup_threshold_at_a_table_value_and_one_ulp_above(gpu_ctx, d2g, oracle):
    N, S = 100, 64
    m = _planted(N, S, 13, [(70, 3, slice(0, 21))])                   # one pair at 21 / 64
    at = float(m.lut[21])
    above = float(np.nextafter(np.float32(at), np.float32(2)))
    cs = m.set(gpu_ctx, d2g.CMP_BITSLICE)
    for band in BANDS:
        got = cs.dedup(m.lut, at, band_rows=band)
        assert got[70] == 3 and np.array_equal(got, m.ref(at)) and np.sum(got != np.arange(N)) == 1
        got = cs.dedup(m.lut, above, band_rows=band)
        assert np.array_equal(got, np.arange(N)) and np.array_equal(m.ref(above), np.arange(N))
    v = K.oracle_values(oracle, m.sigs, d2g.SIMILARITY, k=31)          # ... and with the product's own table
    at = float(v[70, 3])
    above = float(np.nextafter(np.float32(at), np.float32(2)))
    assert gpu_ctx.cmp_dedup(m.sigs.view(np.uint64), at)[70] == 3 and R.dedup_reference(v, at)[1][3] == [70]
    assert gpu_ctx.cmp_dedup(m.sigs.view(np.uint64), above)[70] == 70 and len(R.dedup_reference(v, above)[0]) == N


def test_dedup_chain_is_not_single_linkage(gpu_ctx, d2g):
    """A ~ B ~ C, A !~ C: B joins A, and C -- never compared with the non-representative B -- founds a cluster"""
    N, S = 100, 64
    A, B, C = 10, 40, 45                                            # with bands of 33: B and C share a band, A lies in an earlier one
    m = _planted(N, S, 14, [(B, A, slice(0, 40)), (C, B, slice(40, 64))])
    assert m.cnt[B, A] == 40 and m.cnt[C, B] == 24 and m.cnt[C, A] == 0
    exp = np.arange(N)
    exp[B] = A
    assert np.array_equal(m.ref(0.3), exp)
    for band in BANDS:
        same(run_dev(gpu_ctx, m.set(gpu_ctx, d2g.CMP_BITSLICE), N, min_count_of(m.lut, 0.3), None, band), exp, f"band {band}")


def test_dedup_tie_between_an_earlier_band_and_the_rows_own_band(gpu_ctx, d2g):
    """two representatives at one value, index 5 (an earlier band of 33) and index 40 (the row's own band): the smaller index wins;
    one count more on either side decides for that side"""
    N, S = 100, 64
    m = _planted(N, S, 15, [(50, 5, slice(0, 16)), (50, 40, slice(16, 32)),
                            (51, 5, slice(0, 16)), (51, 40, slice(16, 33)),
                            (52, 5, slice(0, 17)), (52, 40, slice(17, 33))])
    assert (m.cnt[50, 5], m.cnt[50, 40], m.cnt[51, 5], m.cnt[51, 40], m.cnt[52, 5], m.cnt[52, 40]) == (16, 16, 16, 17, 17, 16)
    exp = np.arange(N)
    exp[[50, 51, 52]] = (5, 40, 5)
    assert np.array_equal(m.ref(0.25), exp)
    for algo in (d2g.CMP_BITSLICE, d2g.CMP_DIRECT):
        for band in BANDS + (45,):                                    # 45: both representatives in the band before the rows'
            same(run_dev(gpu_ctx, m.set(gpu_ctx, algo), N, 16, None, band), exp, f"algo {algo} band {band}")


def test_dedup_class_table_merges_counts(gpu_ctx, d2g):
    """a table with four counts to a value: two representatives whose counts differ inside one class tie, and the tie goes to the
    smaller index -- not to the larger count"""
    N, S = 257, 128
    m = families(N, S)
    lut = (np.arange(S + 1) // 4 * 4 / S).astype(np.float32)
    cls = K.class_table(lut)
    assert not np.array_equal(cls, np.arange(S + 1))
    values = lut[m.cnt]
    cs = m.set(gpu_ctx, d2g.CMP_BITSLICE)
    for T in (0.1, 0.25):
        exp = m.ref(T, values, "merged")
        # on this matrix the table matters: some row joins a representative that does not hold its largest COUNT
        isrep = exp == np.arange(N)
        by_count = [int(np.nonzero(isrep[:i])[0][np.argmax(m.cnt[i, :i][isrep[:i]])]) for i in range(N) if not isrep[i]]
        assert np.any(np.array(by_count) != exp[~isrep])
        mc = min_count_of(lut, T)
        assert cls[mc] == mc
        for band in BANDS:
            same(run_dev(gpu_ctx, cs, N, mc, cls, band), exp, f"classes T {T} band {band}")
        same(cs.dedup(lut, T), exp, f"set_dedup classes T {T}")


def test_dedup_code_plane_sets(gpu_ctx, d2g):
    """a set of 1-byte codes (D2G_CMP_PLANES) through the device entry, against NumPy counts of the codes"""
    rng = np.random.default_rng(8)
    N, S = 257, 100
    codes = rng.integers(0, 4, (N, S)).astype(np.uint8)             # four code values: counts around S / 4
    codes[40:60] = codes[40]
    cnt = K.eqcounts(codes)
    cs = gpu_ctx.cmp_set_codes(codes)
    assert cs.algo == d2g.CMP_PLANES
    for mc in (30, 34, S):
        ids, cons = R.dedup_reference(cnt.astype(np.float32), float(mc))
        exp = R.assign_of(ids, cons, N)
        if mc < S:
            assert 2 <= len(ids) <= N - 1
        for band in BANDS:
            same(run_dev(gpu_ctx, cs, N, mc, None, band), exp, f"codes min_count {mc} band {band}")
    cs.close()


def test_dedup_small_sets_multiset_space_and_refusals(gpu_ctx, d2g, oracle):
    assert gpu_ctx.cmp_dedup(np.zeros((0, 64), np.uint64), 0.5).size == 0
    one = K.family_sigs(1, 64, seed=1)
    assert gpu_ctx.cmp_dedup(one.view(np.uint64), 0.5).tolist() == [0]
    two = np.tile(one, (2, 1))
    assert gpu_ctx.cmp_dedup(two.view(np.uint64), 0.5).tolist() == [0, 0]
    # --multiset: the value is a function of the equality count at any S; set space at the same S, distances and
    # cardinality-dependent measures are refused
    N, S = 67, 100
    sigs = K.family_sigs(N, S, seed=N * 7 + S)
    v = K.oracle_values(oracle, sigs, d2g.SIMILARITY, k=31, multiset=True)
    ids, cons = R.dedup_reference(v, 0.1)
    assert 2 <= len(ids) <= N - 1
    assert np.array_equal(gpu_ctx.cmp_dedup(sigs.view(np.uint64), 0.1, multiset_space=True), R.assign_of(ids, cons, N))
    for kw in (dict(multiset_space=False), dict(multiset_space=True, measure=d2g.POISSON_LLR), dict(multiset_space=True, measure=d2g.CONTAINMENT)):
        with pytest.raises(d2g.D2GError):
            gpu_ctx.cmp_dedup(sigs.view(np.uint64), 0.1, **kw)
    m = families(67, 64)
    with pytest.raises(d2g.D2GError):
        m.set(gpu_ctx, d2g.CMP_BITSLICE).dedup(m.lut[::-1].copy(), 0.5)          # a table that decreases
    with pytest.raises(d2g.D2GError):
        m.set(gpu_ctx, d2g.CMP_BITSLICE).dedup_dev(None, 1)                      # null assignment


def test_dedup_kernels_are_timed(gpu_ctx, d2g):
    m = families(257, 64)
    gpu_ctx.set_timing(d2g.TIME_DEDUP | d2g.TIME_K2)
    try:
        gpu_ctx.kernel_ms("dedup")
        gpu_ctx.kernel_ms("k2")
        gpu_ctx.cmp_dedup(m.sigs.view(np.uint64), 0.25, band_rows=100)
        resolve = gpu_ctx.kernel_ms("dedup_resolve", reset=False)
        both = gpu_ctx.kernel_ms("dedup")
        walk = gpu_ctx.kernel_ms("k2")
    finally:
        gpu_ctx.set_timing(0)
    assert resolve[0] == 3 and both[0] == 5 and both[1] > 0       # three bands: three in-order steps, two per-row launches (the first band has no earlier column)
    assert walk[0] >= 3
    assert gpu_ctx.kernel_ms("dedup")[0] == 0 and gpu_ctx.kernel_ms("dedup_resolve")[0] == 0


# ---- rows longer than one trip of dedup_best_kernel's unrolled loop ------------------------------------------------------
# the per-row kernel advances by UNROLL * THREADS = 1024 columns: N = 2500 takes two full trips and a third that is partly past
# the end of the row.  (Every matrix above has N <= 1000: one trip.)
LONG_N, LONG_S = 2500, 64


def far_representatives(values, assign, T, band):
    """from the REFERENCE result: rows whose representative lies at an index >= 1024 in an earlier band, and rows that join a
    representative below 1024 although a qualifying representative at >= 1024 precedes them"""
    N = values.shape[0]
    isrep = assign == np.arange(N)
    simt = R.simt_of(T)
    far = near_despite_far = 0
    for i in np.nonzero(~isrep)[0]:
        r = int(assign[i])
        if r >= 1024:
            far += r // band < i // band
        else:
            reps = np.nonzero(isrep[1024:i])[0] + 1024
            near_despite_far += bool(np.any(values[i, reps] >= simt))
    return far, near_despite_far


@pytest.mark.parametrize("shuffled", [False, True], ids=["generator-order", "shuffled"])
def test_dedup_rows_of_more_than_one_trip(gpu_ctx, d2g, shuffled):
    """T in {0.1, 0.25}, bands of 33 rows and the default (and of one row for one T), bit-sliced and direct sets.  After the
    shuffle the best representative of a row is found in the second or third trip, or must win against qualifying ones there."""
    N, S = LONG_N, LONG_S
    m = families(N, S, shuffled)
    cls = K.class_table(m.lut)
    for T in (0.1, 0.25):
        exp = m.ref(T)
        assert 2 <= np.sum(exp == np.arange(N)) <= N - 1
        if shuffled:
            for band in (33, 256):
                far, near_despite_far = far_representatives(m.values, exp, T, band)
                assert far >= 10 and near_despite_far >= 10, (T, band, far, near_despite_far)
        for algo in (d2g.CMP_BITSLICE, d2g.CMP_DIRECT):
            cs = m.set(gpu_ctx, algo)
            assert cs.algo == algo
            for band in ((33, 0, 1) if algo == d2g.CMP_BITSLICE and T == 0.25 else (33, 0)):
                got = run_dev(gpu_ctx, cs, N, min_count_of(m.lut, T), cls if band else None, band)
                same(got, exp, f"dev algo {algo} band {band} T {T}")
