"""The bit-sliced compare (d2g_k2_bitslice.hip: transpose -> bs_rank_kernel -> bs_colplan_kernel -> bs_planes_kernel -> pair kernel) at the
exact collection sizes and register values where its code changes behaviour, on matrices whose equality counts are known by construction
(k2_seam_cases.py: the expected count of a pair comes from the recipe's LABELS, never from the 64-bit values), each case also on a
CMP_DIRECT set as a second opinion.  Every comparison is exact.

Which parameter hits which seam:
  rank kernel, registers vs general (N <= 12 * 1024)            test_k2_rank_kernel_seams[12287 / 12288 / 12289]
  one LDS table at load 2/3 vs two hash partitions               ...[21845 / 21846]
  two -> four partitions, nsplit 4                               test_k2_rank_kernel_seams_split[43690 / 43691 x D2G_BS_NSPLIT 1, 2, 4]
  the table doubles (fullest just below)                         ...[5461 / 5462 / 10922 / 10923]
  index / tag field of an owner slot (ib = 32 - clz(N)),
  the sparse path's default threshold                            ...[8191 / 8192 / 16383 / 16384]
  live_planes / plane_class at D2 = 2^b - 2, 2^b - 1, 2^b        test_k2_plane_class_seams (the group's MAXIMUM is the seam value, sort off)
  the column plan's sort, padding slots                          test_k2_one_busy_column_per_group
  nbits_cap, every group at the cap, the stream's slack block    test_k2_stream_at_the_cap (N = 2^(c+1) - 4 / - 2)
  Npad, BS_SLACK, wave tiles from any i_lo, tile_of_block        test_k2_every_wanted_cell_is_written_and_nothing_else
  no reserved sentinel value                                     test_k2_sentinel_values, and the `specials` columns of the seam matrices

Run time on the MI355X, one visit: this file 25.3 s (pytest's total; measured before test_k2_one_busy_column_per_group was added, 25.7 s with it), tests/test_gpu_k2_sparse_edges.py at the parent commit 49.2 s -- 0.51 x, under the
1.5 x the suite allows itself, so every seam size up to 21 846 keeps its whole triangle."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import k2_seam_cases as kc

pytestmark = pytest.mark.gpu

WORKERS = max(1, min(16, os.cpu_count() or 1))
PATTERN, GUARD = 0xA5A5A5A5, 1024


# ---------------------------------------------------------------- helpers
def _assert_ut(got, case, r0, r1, what):
    """got == the label counts of rows [r0, r1), block of rows by block of rows (the blocks on a few threads)"""
    N = case.N
    off = kc.ut_offsets(N)
    assert got.size == int(off[r1] - off[r0]), what
    rows = max(1, (1 << 22) // N)
    blocks = [(a, min(a + rows, r1)) for a in range(r0, r1, rows)]

    def one(ab):
        a, b = ab
        return ab if not np.array_equal(got[int(off[a] - off[r0]):int(off[b] - off[r0])], case.counts_ut(a, b)) else None

    with ThreadPoolExecutor(WORKERS) as ex:
        bad = [x for x in ex.map(one, blocks) if x is not None]
    if bad:
        a, b = bad[0]
        np.testing.assert_array_equal(got[int(off[a] - off[r0]):int(off[b] - off[r0])], case.counts_ut(a, b), err_msg=f"{what}: rows {a}:{b}")


def _lut(d2g, S):
    """the similarity table of the fused epilogue.  In set space the library has one only where S is a power of two (elsewhere the value is
    not a function of the equality count alone and d2g_epilogue_lut refuses); S = 40, 96, 100 take the multiset-space table"""
    return d2g.epilogue_lut(S, d2g.SIMILARITY, 31, multiset_space=bool(S & (S - 1)))


def _both_sets(gpu_ctx, d2g, case):
    cs = gpu_ctx.cmp_set(case.matrix, algo=d2g.CMP_BITSLICE)
    assert cs.algo == d2g.CMP_BITSLICE
    return cs, gpu_ctx.cmp_set(case.matrix, algo=d2g.CMP_DIRECT)


def _check_ranges(cs, dr, case, ranges, what):
    for r0, r1 in ranges:
        got = cs.eqcount_ut(r0, r1)
        _assert_ut(got, case, r0, r1, f"{what} rows {r0}:{r1}")
        assert np.array_equal(dr.eqcount_ut(r0, r1), got), f"{what} rows {r0}:{r1}: the direct kernel disagrees with the labels"


def _check_planes(cs, case):
    md, nb, _ = cs.planes()
    assert md == int(case.d2.max()) + 1
    assert nb == (int(case.d2.max()) + 1).bit_length()
    cs.status()


def _seam_matrix(N, S, seed):
    recs = [kc.distinct, kc.pairs, kc.constant, kc.two_values, kc.shared(2 ** 10 - 1, 2)]
    return kc.striped(N, S, recs, ("random", "specials", "twins", "low_only", "high_only"), seed=seed)


def _seam_ranges(N):
    if N * (N - 1) // 2 < 2 ** 28:
        r = [(0, N)]
    else:
        r = [(0, 40), (N // 2 - 20, N // 2 + 20), (N - 300, N)]
    return r + [(x - 9, x + 7) for x in (12_288, 21_845) if x + 7 <= N]     # launches that start off every tile grid and straddle the seam row


# ---------------------------------------------------------------- rank-kernel seams
@pytest.mark.parametrize("N", [5_461, 5_462, 8_191, 8_192, 10_922, 10_923, 12_287, 12_288, 12_289, 16_383, 16_384, 21_845, 21_846])
def test_k2_rank_kernel_seams(gpu_ctx, d2g, N):
    """S = 64, columns striped over distinct / pairs / constant / two values / 1023 shared values, five columns per value pool (random, specials,
    twins, low word only, high word only: every recipe meets every pool).  Whole triangle against the labels and the direct kernel, two row
    ranges that straddle rows 12 288 and 21 845; the set's plane counts are those of the `pairs` columns (D2 = N // 2)."""
    case = _seam_matrix(N, 64, seed=N)
    assert int(case.d2.max()) == N // 2 and {"specials", "twins"} <= set(case.pools)
    cs, dr = _both_sets(gpu_ctx, d2g, case)
    _check_planes(cs, case)
    _check_ranges(cs, dr, case, _seam_ranges(N), f"N={N}")
    cs.close(); dr.close()


@pytest.mark.parametrize("nsplit", ["1", "2", "4"])
@pytest.mark.parametrize("N", [43_690, 43_691])
def test_k2_rank_kernel_seams_split(gpu_ctx, d2g, monkeypatch, N, nsplit):
    """43 690 sketches: 2 hash partitions of 32 768 slots at load 2/3; 43 691: 4 partitions, and a column may be split over 4 workgroups.
    S = 32; row ranges (the triangle has 2^29.8 pairs): first rows, middle, last 300, and across rows 12 288 and 21 845."""
    monkeypatch.setenv("D2G_BS_NSPLIT", nsplit)
    case = _seam_matrix(N, 32, seed=N + int(nsplit))
    assert int(case.d2.max()) == N // 2 and case.pools.count("specials") >= 2 and case.pools.count("twins") >= 2
    cs, dr = _both_sets(gpu_ctx, d2g, case)
    _check_planes(cs, case)
    _check_ranges(cs, dr, case, _seam_ranges(N), f"N={N} nsplit={nsplit}")
    cs.close(); dr.close()


# ---------------------------------------------------------------- plane-class seams
def _plane_class_columns(b, S):
    """group 0's busiest column shares 2^b - 2 values, group 1's 2^b - 1, group 2's 2^b (a fourth group: 2^b - 1 again); every other column
    fewer (the seam values of the smaller b, in turn)"""
    tops = [2 ** b - 2, 2 ** b - 1, 2 ** b, 2 ** b - 1]
    small = sorted({d for c in range(1, b) for d in (2 ** c - 2, 2 ** c - 1, 2 ** c) if d < 2 ** b - 2} | {0})
    rec = lambda d: kc.distinct if d == 0 else kc.shared(d, 2)
    pools = ("random", "specials", "twins", "low_only")
    cols = []
    for t in range(S):
        g, x = divmod(t, 32)
        top_at = (5 * g + 1) % min(32, S - 32 * g)
        d = tops[g] if x == top_at else small[(t + g) % len(small)]
        cols.append((rec(d), pools[t % 4]))
    return cols, tops[:-(-S // 32)]


@pytest.mark.parametrize("S", [96, 100])
@pytest.mark.parametrize("b", range(1, 10))
def test_k2_plane_class_seams(gpu_ctx, d2g, monkeypatch, b, S):
    """live_planes / plane_class = bit_length(D2 + 1): with one plane too few, rank 2^b - 1 -- the LAST shared value of a column with
    D2 = 2^b - 1 -- is all ones, the column coding of "unique", and a unique sketch would count as equal to every holder of that value.
    N = 2 100; every b with 2^b <= N/2 - N/8; shared values are held twice, so at least N/4 sketches of every column are unique.  With the
    sort off a group's plane count is that of its busiest column, which the recipe places: the mean over the groups is known exactly."""
    N = 2_100
    assert 2 ** b <= N // 2 - N // 8
    cols, tops = _plane_class_columns(b, S)
    case = kc.from_columns(N, cols, seed=100 * b + S)
    assert case.group_max_d2().tolist() == tops and int((case.labels < 0).sum(axis=1).min()) >= N // 4
    dr = gpu_ctx.cmp_set(case.matrix, algo=d2g.CMP_DIRECT)
    want = dr.eqcount_ut()
    dr.close()
    _assert_ut(want, case, 0, N, f"b={b} S={S} direct")
    for sort in ("0", "1"):
        monkeypatch.setenv("D2G_BS_SORT", sort)
        cs = gpu_ctx.cmp_set(case.matrix, algo=d2g.CMP_BITSLICE)
        got = cs.eqcount_ut()
        assert np.array_equal(got, want), f"b={b} S={S} sort={sort}: {int((got != want).sum())} pairs differ from the label counts"
        # said once more for the pairs the seam is about: per column with D2 >= 1, a holder of the last shared value against a unique sketch
        off = kc.ut_offsets(N)
        for t in np.flatnonzero(case.d2):
            h = int(np.flatnonzero(case.labels[t] == case.d2[t] - 1)[0])
            u = int(np.flatnonzero(case.labels[t] < 0)[0])
            i, j = min(h, u), max(h, u)
            assert int(got[off[i] + j - i - 1]) == int(case.counts_rect(i, i + 1, j, j + 1)[0, 0]), (b, S, sort, int(t), i, j)
        md, nb, mean = cs.planes()
        emd, enb, emean = case.planes_expected(sorted_columns=sort == "1")
        assert (md, nb) == (emd, enb) == (max(tops) + 1, (max(tops) + 1).bit_length())
        if sort == "0":
            assert np.float32(mean) == emean == np.float32(sum(int(x + 1).bit_length() for x in tops) / len(tops)), (mean, emean)
        cs.status()
        cs.close()


@pytest.mark.parametrize("S", [96, 100, 1000])
def test_k2_one_busy_column_per_group(gpu_ctx, d2g, monkeypatch, S):
    """One column with 2^9 - 1 shared values in every 32-column group, all others without any: with the sort off every group pays the busy
    column's 10 planes, with it on the busy columns share the first group and every other group has one plane -- padding slots of the
    last group (S = 100, 1000) sort behind every real column.  The mean over the groups follows from the recipe either way."""
    N = 2_100
    case = kc.one_busy_column_per_group(N, S, kc.shared(2 ** 9 - 1, 2), pool="twins", seed=S)
    ng = -(-S // 32)
    assert case.group_max_d2().tolist() == [511] * ng
    cs_d = gpu_ctx.cmp_set(case.matrix, algo=d2g.CMP_DIRECT)
    want = cs_d.eqcount_ut()
    cs_d.close()
    _assert_ut(want, case, 0, N, f"S={S} direct")
    for sort in ("0", "1"):
        monkeypatch.setenv("D2G_BS_SORT", sort)
        cs = gpu_ctx.cmp_set(case.matrix, algo=d2g.CMP_BITSLICE)
        assert np.array_equal(cs.eqcount_ut(), want), f"S={S} sort={sort}"
        md, nb, mean = cs.planes()
        assert (md, nb) == (512, 10)
        assert np.float32(mean) == case.planes_expected(sorted_columns=sort == "1")[2] == np.float32(10 if sort == "0" else (10 + ng - 1) / ng)
        cs.status()
        cs.close()


# ---------------------------------------------------------------- the plane stream used to its last block
@pytest.mark.parametrize("S", [32, 96, 100])
@pytest.mark.parametrize("N", [60, 62, 508, 510, 4_092, 4_094])
def test_k2_stream_at_the_cap(gpu_ctx, d2g, N, S):
    """A collection made of duplicate pairs: every value of every column occurs exactly twice, D2 = N / 2 in every column, so EVERY group uses
    nbits_cap planes (2^cap >= N/2 + 2: N = 2^(c+1) - 4 fills cap = c exactly, N = 2^(c+1) - 2 needs c + 1) and the plane stream is used to its
    last allocated block; the pair kernel's prefetch of one plane ahead reads the block of slack behind it.  Whole triangle, the full square
    (rectangular launch: the diagonal holds S) and the table store bit for bit."""
    case = kc.uniform(N, S, kc.pairs, {32: "random", 96: "twins", 100: "specials"}[S], seed=N + S)
    cap = 1
    while (1 << cap) < N // 2 + 2:
        cap += 1
    cs, dr = _both_sets(gpu_ctx, d2g, case)
    md, nb, mean = cs.planes()
    assert (md, nb) == (N // 2 + 1, cap) and np.float32(mean) == np.float32(cap)
    cs.status()
    _check_ranges(cs, dr, case, [(0, N)], f"N={N} S={S}")
    want = case.counts_ut()
    square = case.counts_rect(0, N, 0, N)
    assert (np.diag(square) == S).all()
    np.testing.assert_array_equal(cs.eqcount_rect(0, N, 0, N), square)
    np.testing.assert_array_equal(dr.eqcount_rect(0, N, 0, N), square)
    lut = _lut(d2g, S)
    np.testing.assert_array_equal(cs.lut_ut(lut).view(np.uint32), lut[want].view(np.uint32))
    cs.close(); dr.close()


# ---------------------------------------------------------------- register values that look like the rank kernel's own marks
@pytest.mark.parametrize("pool", ["specials", "twins", "low_only", "high_only"])
@pytest.mark.parametrize("recipe", ["shared5", "distinct"])
@pytest.mark.parametrize("N", [700, 12_289])
def test_k2_sentinel_values(gpu_ctx, d2g, N, recipe, pool):
    """The owner table stores sketch indices, not values: no register value is reserved.  S = 33; five shared values per column, the first one
    held by a third of the sketches -- or no shared value at all -- from pools of values that look like the kernel's marks (0, ~0 = an EMPTY
    register, 0xFFFFFFFF = BS_EMPTY, 0x80000000 = BS_DUP / BS_UNIQ, 0x40000000 = BS_PENDING, in either half) or that agree in one 32-bit half
    only.  Equal halves with different other halves are not equal; ~0 held by a third of the sketches is equal to itself."""
    S = 33
    rec = kc.shared(5, [N // 3, 2, 3, 2, 7]) if recipe == "shared5" else kc.distinct
    case = kc.uniform(N, S, rec, pool, seed=N + len(pool))
    cs, dr = _both_sets(gpu_ctx, d2g, case)
    _check_planes(cs, case)
    got = cs.eqcount_ut()
    _assert_ut(got, case, 0, N, f"N={N} {recipe} {pool}")
    assert np.array_equal(dr.eqcount_ut(), got)
    if recipe == "distinct":
        assert not got.any()
    elif pool == "specials":
        for t in range(10):                                            # column t: label 0 is SPECIALS[t], held by N // 3 sketches
            assert int(case.shared[t][0]) == kc.SPECIALS[t]
            i, j = (int(x) for x in np.flatnonzero(case.labels[t] == 0)[:2])
            assert (case.matrix[i, t], case.matrix[j, t]) == (np.uint64(kc.SPECIALS[t]),) * 2
            c = int(got[kc.ut_offsets(N)[i] + j - i - 1])
            assert c >= 1 and c == int(case.counts_rect(i, i + 1, j, j + 1)[0, 0]), (t, i, j, c)
    cs.close(); dr.close()


# ---------------------------------------------------------------- every wanted cell written, nothing else
def _guarded(gpu_ctx, n, launch, skew=0):
    """`launch(ptr)` writes n 32-bit words at ptr; the buffer around and under them is pre-set to PATTERN from the host.  Both guards must come
    back untouched, and every one of the n words written (no result can be the pattern).  -> the n words"""
    lo = GUARD + skew
    words = lo + n + GUARD
    d = gpu_ctx.malloc(words * 4)
    buf = np.empty(words, np.uint32)
    try:
        gpu_ctx.h2d(d, np.full(words, PATTERN, np.uint32))
        launch(d + 4 * lo)
        gpu_ctx.sync()
        gpu_ctx.d2h(buf, d)
    finally:
        gpu_ctx.free(d)
    assert (buf[:lo] == PATTERN).all(), f"{int((buf[:lo] != PATTERN).sum())} words written in front of the output"
    assert (buf[lo + n:] == PATTERN).all(), f"{int((buf[lo + n:] != PATTERN).sum())} words written behind the output"
    mid = buf[lo:lo + n]
    assert not (mid == PATTERN).any(), f"{int((mid == PATTERN).sum())} of {n} wanted cells never written (first: {int(np.flatnonzero(mid == PATTERN)[0])})"
    return mid


def _guard_matrix(N, S, sparse):
    if sparse:                                                         # few shared values, each sketch placed afresh per column: no families, a short pair list
        return kc.uniform(N, S, kc.shared(8, [2, 2, 3, 2, 5, 2, 2, 4]), "random", seed=N)
    recs = [kc.pairs, kc.constant, kc.two_values, kc.shared(3, [N // 4, 2, 5]), kc.distinct] if N >= 16 else [kc.constant, kc.pairs, kc.distinct]
    return kc.striped(N, S, recs, ("random", "specials", "twins"), seed=N)


def _ut_ranges(N):
    return [(a, b) for a, b in ((0, N), (0, 1), (N - 1, N), (15, 17), (31, 33), (250, 262)) if b <= N]


def _rects(N):
    h = N // 2
    r = [(h, h + 1, 0, N), (0, N, N // 3, N // 3 + 1), (N - 1, N, N - 1, N),       # one row, one column, one cell on the diagonal
         (h + 1, N, 0, h), (0, h, h + 1, N),                                       # wholly below, wholly above the diagonal
         (17, min(N, 67), 5, min(N, 305)), (33, min(N, 50), 257, min(N, 300))]     # across the diagonal off both grids; off-grid above it
    for b0 in (0, 1, 256):
        for w in (1, 255, 256, 257):
            r.append((3, min(N, 23), b0, b0 + w))
            r.append((N - min(N, 40), N, b0, b0 + w))
    return [x for x in dict.fromkeys(r) if x[0] < x[1] <= N and x[2] < x[3] <= N]


GUARD_SIZES = [1, 2, 255, 256, 257, 511, 777, 2_049]


@pytest.mark.parametrize("N,mode", [(n, "shipped") for n in GUARD_SIZES] + [(n, "sparse") for n in GUARD_SIZES if n >= 256])   # (forced from 256 sketches on)
def test_k2_every_wanted_cell_is_written_and_nothing_else(gpu_ctx, d2g, monkeypatch, N, mode):
    """Every K2 test reads its result from a fresh allocation: a tile the kernel never writes shows whatever was there -- possibly the right
    answer of the previous call.  Here the output lies between two guards of 1 024 words, all of it pre-set to 0xA5A5A5A5 (no count reaches it:
    counts are <= S = 40; the table does not hold that float).  Upper-triangle launches on whole, single-row, empty and off-grid row ranges
    (counts and table), rectangles on and off the 16-row / 256-column grid; as shipped, and (N >= 256) with the sparse path forced, where the
    fill + pair list must obey the same rule -- also when the fill was enqueued ahead (prefill) or carried by the prepare's riders (announce)."""
    S = 40
    sparse = mode == "sparse"
    if sparse:
        monkeypatch.setenv("D2G_BS_SPARSE_MIN_N", "256")
        monkeypatch.setenv("D2G_SP_PREDICT", "0")
        monkeypatch.setenv("D2G_SP_REMEMBER", "0")
    case = _guard_matrix(N, S, sparse)
    lut = _lut(d2g, S)
    assert PATTERN not in lut.view(np.uint32).tolist() and S < PATTERN
    d_lut, d_rows = gpu_ctx.malloc(lut.nbytes), gpu_ctx.malloc(case.matrix.nbytes)
    gpu_ctx.h2d(d_lut, lut)
    gpu_ctx.h2d(d_rows, case.matrix)
    off = kc.ut_offsets(N)
    sets = [("bitslice", gpu_ctx.cmp_set(case.matrix, algo=d2g.CMP_BITSLICE))]
    if not sparse:
        sets.append(("direct", gpu_ctx.cmp_set(case.matrix, algo=d2g.CMP_DIRECT)))
    try:
        for name, cs in sets:
            for k, (r0, r1) in enumerate(_ut_ranges(N)):
                n = int(off[r1] - off[r0])
                want = case.counts_ut(r0, r1)
                ways = [("plain", lambda p: cs.eqcount_ut_dev(p, r0, r1), lambda p: cs.lut_ut_dev(d_lut, p, r0, r1))]
                if sparse:
                    def pre_eq(p): cs.prefill_ut_dev(p, r0, r1); cs.eqcount_ut_dev(p, r0, r1)
                    def pre_lut(p): cs.prefill_ut_dev(p, r0, r1, lut_dev_ptr=d_lut); cs.lut_ut_dev(d_lut, p, r0, r1)
                    def ann_eq(p): cs.announce_ut_dev(p, r0, r1); cs.update_dev(d_rows); cs.eqcount_ut_dev(p, r0, r1)
                    def ann_lut(p): cs.announce_ut_dev(p, r0, r1, lut_dev_ptr=d_lut); cs.update_dev(d_rows); cs.lut_ut_dev(d_lut, p, r0, r1)
                    ways += [("prefill", pre_eq, pre_lut), ("announce", ann_eq, ann_lut)]
                for way, eq, fl in ways:
                    what = f"{name} N={N} {mode} rows {r0}:{r1} {way}"
                    np.testing.assert_array_equal(_guarded(gpu_ctx, n, eq, skew=k % 4), want, err_msg=what)
                    if sparse and way == "plain" and (r0, r1) == (0, N):
                        info = cs.sparse_info()
                        assert info["tiles_and_pair_list"] and not info["dense_kernel_ran"] and info["pairs_listed"] > 0, (what, info)
                    np.testing.assert_array_equal(_guarded(gpu_ctx, n, fl, skew=(k + 1) % 4), lut[want].view(np.uint32), err_msg=what + " table")
            for k, (a0, a1, b0, b1) in enumerate(_rects(N)):
                want = case.counts_rect(a0, a1, b0, b1)
                if (a0, a1, b0, b1) == (N - 1, N, N - 1, N):
                    assert want.tolist() == [[S]]
                got = _guarded(gpu_ctx, want.size, lambda p: cs.eqcount_rect_dev(p, a0, a1, b0, b1), skew=k % 4)
                np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=f"{name} N={N} {mode} rect {a0}:{a1} x {b0}:{b1}")
    finally:
        for _, cs in sets:
            cs.close()
        gpu_ctx.free(d_lut)
        gpu_ctx.free(d_rows)
