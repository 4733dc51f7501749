"""(gt, lt) counts of the direct K2 kernel -- k2_direct_kernel<true> behind d2g_cmp_gtlt_ut_dev / d2g_cmp_gtlt_rect_dev -- and what is
built on them.  Set space at a sketch size that is not a power of two takes this path: the reference computes eq = (1 - gt/S) - lt/S
in long double (cmp_core.cpp:461-476), so the value depends on the split of S - eq into gt and lt and on its orientation.  Pairs that
share no register (gt + lt = S) are where it shows: their union size is 0 or lh + rh depending on the split.

Integer counts are checked exactly against the oracle's batched count (oracle.gtlt_rect), S - gt - lt against the bit-sliced
equality counts, floats bit for bit.  Every float-level case first shows that its data hold pairs whose union size changes under
(lt, gt) and under (S - eq, 0): without them a swapped orientation or the equality-count path would pass unseen."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HI = np.uint64(0xFFFFFFFF00000000)
LO = np.uint64(0x00000000FFFFFFFF)
INF_BITS = np.uint64(0x7FF0000000000000)
NT = min(16, int(os.environ.get("OMP_NUM_THREADS") or 0) or (os.cpu_count() or 1))


def _gen(rng, N, S, nvals=4, families=0):
    """N x S non-negative doubles (the domain of every OPH and BMH register) with the orders a (gt, lt) kernel can get wrong.
    Returns (matrix, indices of the unrelated rows)."""
    vals = rng.random((nvals, S))
    m = vals[rng.integers(0, nvals, (N, S)), np.arange(S)[None, :]]      # planted columns: many equal and many ordered pairs
    if families:                                                           # rows of a family share most registers
        fam = rng.integers(0, families, N)
        own = rng.random((N, S)) < rng.uniform(0.02, 0.5, (N, 1))
        fm = np.where(own, rng.random((N, S)), rng.random((families, S))[fam])
        pick = rng.random(N) < 0.5
        m[pick] = fm[pick]
    m[rng.random((N, S)) < 0.01] = np.inf
    bits = m.view(np.uint64)
    unrelated = np.unique(rng.integers(0, N, max(1, N // 32) + 1))
    m[unrelated] = rng.random((unrelated.size, S))                        # share no register with any other row
    rest = np.setdiff1d(np.arange(N), unrelated)
    rng.shuffle(rest)
    k = min(max(1, N // 32), rest.size // 11)
    # disjoint rows for each kind of pair: a[q], b[q] is pair kind q
    a, b = rest[:5 * k].reshape(5, k), rest[5 * k:10 * k].reshape(5, k)
    m[b[0]] = m[a[0]]                                                      # identical rows: gt = lt = 0
    src = np.where(np.isinf(m[a[1]]), 0.5, m[a[1]])
    m[a[1]], m[b[1]] = src, src + 1.0                                      # b above a in every register: gt = S
    half = lambda x: rng.random(x.shape) < 0.5
    x = bits[a[2]]
    step = np.where(half(x), 1, -1)
    step[x == 0] = 1
    step[x == INF_BITS] = -1
    bits[b[2]] = np.where(half(x), x, (x.astype(np.int64) + step).astype(np.uint64))   # neighbours one ULP apart
    x = bits[a[3]]
    y = np.where((x & HI) == INF_BITS, x, (x & HI) | rng.integers(0, 1 << 32, x.shape, dtype=np.uint64))
    bits[b[3]] = np.where(half(x), x, y)                                   # high dwords equal, low dwords differ
    x = bits[a[4]]
    bits[b[4]] = np.where(half(x), x, (rng.random(x.shape).view(np.uint64) & HI) | (x & LO))   # low dwords equal, high dwords differ
    if rest.size > 10 * k:
        m[rest[10 * k]] = 0.0                                              # an empty sketch after densify
    assert not np.isnan(m).any() and not np.signbit(m).any()
    return m, unrelated


def _union_bits(oracle, gt, lt, S, lhc, rhc):
    return np.float32(oracle.compare_from_gtlt(int(gt), int(lt), S, lhc, rhc, oracle.UNION_SIZE, 31)).view(np.uint32)


def _assert_sensitive(oracle, sigs, cards, pairs, need=5):
    """the precondition of every float-level case: at least `need` of `pairs` (i, j) in compare(i, j) order change their union size
    under (lt, gt) and under (S - eq, 0); counts from the oracle, not from the device"""
    S = sigs.shape[1]
    nswap = neqp = 0
    for i, j in pairs:
        g, l = oracle.count_gtlt(sigs[i], sigs[j])
        v = _union_bits(oracle, g, l, S, cards[i], cards[j])
        nswap += v != _union_bits(oracle, l, g, S, cards[i], cards[j])
        neqp += v != _union_bits(oracle, g + l, 0, S, cards[i], cards[j])
    assert nswap >= need and neqp >= need, f"the data cannot show the bugs this test is for: {nswap} swap-, {neqp} eq-sensitive pairs"


def _unrelated_pairs(unrelated, limit=400):
    u = np.sort(unrelated)
    return [(int(u[a]), int(u[b])) for a in range(u.size) for b in range(a + 1, u.size)][:limit]


def _ut_of_square(sq):
    return sq[np.triu_indices(sq.shape[0], 1)]


UT_CASES = [(1, 1), (1, 1000), (2, 1), (2, 3), (2, 1023), (33, 1), (33, 3), (33, 33), (33, 1025), (255, 100), (255, 4095),
            (257, 3), (257, 1000), (257, 1023), (1000, 33), (1000, 1025), (4097, 100), (4097, 1023), (40, 16385), (300, 16385)]


@pytest.mark.parametrize("N,S", UT_CASES)
def test_gtlt_ut_exact(gpu_ctx, d2g, oracle, N, S):
    """(gt, lt) of the upper triangle and of row ranges that start off the 32-row tile grid, exact against the oracle; S - gt - lt
    against the equality counts of the bit-sliced algorithm"""
    rng = np.random.default_rng(N * 131 + S)
    sigs, _ = _gen(rng, N, S)
    egt, elt = oracle.gtlt_rect(sigs, 0, N, 0, N, nthreads=NT)
    egt, elt = _ut_of_square(egt), _ut_of_square(elt)
    cs = gpu_ctx.cmp_set(sigs.view(np.uint64), algo=d2g.CMP_DIRECT)
    assert cs.algo == d2g.CMP_DIRECT
    gt, lt = cs.gtlt_ut()
    np.testing.assert_array_equal(gt, egt)
    np.testing.assert_array_equal(lt, elt)
    if N >= 33:                          # the generator's orders all occur
        assert ((gt == 0) & (lt == 0)).any() and ((gt == S) | (lt == S)).any() and (S == 1 or ((gt > 0) & (lt > 0)).any())
    b = d2g.ut_partition(N, 3)
    ranges = [(b[i], b[i + 1]) for i in range(3)] + [(31, 33), (255, N), (1, 2), (N // 2 + 1, N - 1), (N - 1, N)]
    for r0, r1 in ranges:
        if not 0 <= r0 <= r1 <= N:
            continue
        o0, o1 = d2g.ut_count(N, 0, r0), d2g.ut_count(N, 0, r1)
        g, l = cs.gtlt_ut(r0, r1)
        np.testing.assert_array_equal(g, gt[o0:o1], err_msg=f"rows {r0}:{r1}")
        np.testing.assert_array_equal(l, lt[o0:o1], err_msg=f"rows {r0}:{r1}")
    cs.close()
    bs = gpu_ctx.cmp_set(sigs.view(np.uint64), algo=d2g.CMP_BITSLICE)
    assert bs.algo == d2g.CMP_BITSLICE
    np.testing.assert_array_equal(S - gt.astype(np.int64) - lt, bs.eqcount_ut())
    bs.close()


@pytest.mark.parametrize("N,S", [(1, 1000), (33, 3), (257, 1025), (600, 1023), (1000, 100), (70, 16385)])
def test_gtlt_rect_exact(gpu_ctx, d2g, oracle, N, S):
    """(gt, lt) of rectangles, gt = #(row sketch > column sketch): the full square, blocks off the 32-row and 256-column tile grids,
    a panel split at a row that is not a tile edge, one row, one column"""
    rng = np.random.default_rng(N * 17 + S)
    sigs, _ = _gen(rng, N, S)
    cs = gpu_ctx.cmp_set(sigs.view(np.uint64), algo=d2g.CMP_DIRECT)
    g, l = cs.gtlt_rect(0, N, 0, N)
    eg, el = oracle.gtlt_rect(sigs, 0, N, 0, N, nthreads=NT)
    np.testing.assert_array_equal(g, eg)
    np.testing.assert_array_equal(l, el)
    np.testing.assert_array_equal(g, l.T)
    assert not np.diag(g).any() and not np.diag(l).any()
    ugt, ult = cs.gtlt_ut()
    iu = np.triu_indices(N, 1)
    np.testing.assert_array_equal(g[iu], ugt)                # (i, j), i < j: the triangle's orientation
    np.testing.assert_array_equal(l[iu], ult)
    np.testing.assert_array_equal(g.T[iu], ult)              # (j, i): the other one
    np.testing.assert_array_equal(l.T[iu], ugt)
    nf = N - N // 3
    blocks = [(5, 5 + 97, 3, N), (N // 3 + 1, N - 2, N // 2 + 7, N - 1), (33, N, 257, N), (0, nf, nf, N), (nf, N, 0, nf),
              (N - 1, N, 0, N), (0, 1, 0, N), (0, N, N - 1, N), (0, N, N // 2, N // 2 + 1)]
    for a0, a1, b0, b1 in blocks:
        a1, b1 = min(a1, N), min(b1, N)
        if not (0 <= a0 < a1 and 0 <= b0 < b1):
            continue
        bg, bl = cs.gtlt_rect(a0, a1, b0, b1)
        xg, xl = oracle.gtlt_rect(sigs, a0, a1, b0, b1, nthreads=NT)
        np.testing.assert_array_equal(bg, xg, err_msg=str((a0, a1, b0, b1)))
        np.testing.assert_array_equal(bl, xl, err_msg=str((a0, a1, b0, b1)))
    cs.close()


def test_gtlt_scale_n10000_s1000(gpu_ctx, d2g, oracle):
    """config 3's sketch count at a sketch size that is not a power of two, families and unrelated rows mixed in: every row's total of
    #(row > other) against a per-column searchsorted count; union size and containment of the whole triangle and of two row ranges
    bit for bit against the oracle"""
    N, S = 10_000, 1000
    rng = np.random.default_rng(10_000)
    sigs, unrelated = _gen(rng, N, S, nvals=6, families=40)
    cards = rng.uniform(1e3, 1e7, N)
    cards[unrelated[::2]] = 1234.5
    _assert_sensitive(oracle, sigs, cards, _unrelated_pairs(unrelated))
    bits = sigs.view(np.uint64)
    # independent of the oracle: per column, #(sig[i] > sig[j]) over j = the rank of sig[i] among the column's values
    egt, elt = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for t in range(S):
        col = np.sort(sigs[:, t])
        egt += np.searchsorted(col, sigs[:, t], side="left")
        elt += N - np.searchsorted(col, sigs[:, t], side="right")
    cs = gpu_ctx.cmp_set(bits, algo=d2g.CMP_DIRECT)
    rgt, rlt = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for a0 in range(0, N, 1250):
        g, l = cs.gtlt_rect(a0, a0 + 1250, 0, N)
        rgt[a0:a0 + 1250], rlt[a0:a0 + 1250] = g.sum(axis=1, dtype=np.int64), l.sum(axis=1, dtype=np.int64)
        del g, l
    cs.close()
    np.testing.assert_array_equal(rgt, egt)
    np.testing.assert_array_equal(rlt, elt)
    b = d2g.ut_partition(N, 3)
    for meas in (d2g.UNION_SIZE, d2g.CONTAINMENT):
        exp = oracle.allpairs_ut(sigs, cards, measure=meas, k=21, nthreads=NT)
        got = gpu_ctx.cmp_dist_ut(bits, cards, measure=meas, k=21, nthreads=NT)
        np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32), err_msg=f"measure {meas}")
        del got
        for r0, r1 in [(b[1], b[2]), (4099, 6001)]:
            o0, o1 = d2g.ut_count(N, 0, r0), d2g.ut_count(N, 0, r1)
            got = gpu_ctx.cmp_dist_ut(bits, cards, measure=meas, k=21, r0=r0, r1=r1, nthreads=NT)
            np.testing.assert_array_equal(got.view(np.uint32), exp[o0:o1].view(np.uint32), err_msg=f"measure {meas} rows {r0}:{r1}")


def test_dist_gpu_compute_union_size_row_ranges(gpu_ctx, d2g, oracle):
    """dashing2_amd.dist.gpu_compute on the row ranges of a torch-resident matrix: (gt, lt) on the device, capi.host_epilogue_ut on the
    host; the slabs concatenate to the oracle's triangle"""
    import torch
    from dashing2_amd import dist as DD
    N, S = 700, 1000
    rng = np.random.default_rng(700)
    sigs, unrelated = _gen(rng, N, S, nvals=3)
    cards = rng.uniform(1e3, 1e6, N)
    _assert_sensitive(oracle, sigs, cards, _unrelated_pairs(unrelated))
    sig_t = torch.from_numpy(sigs.view(np.int64)).to(torch.device("cuda", 0))
    run = DD.gpu_compute(gpu_ctx, d2g.UNION_SIZE, 31)
    b = d2g.ut_partition(N, 3)
    got = np.concatenate([run(sig_t, cards, N, S, b[i], b[i + 1]) for i in range(3)])
    exp = oracle.allpairs_ut(sigs, cards, measure=oracle.UNION_SIZE, k=31, nthreads=NT)
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_gtlt_refusals_leave_the_output_alone(gpu_ctx, d2g):
    """(gt, lt) need the raw patterns: sets created with CMP_AUTO (bit-sliced here) or CMP_BITSLICE refuse; so do rectangles out of
    bounds.  Nothing is written."""
    N, S = 300, 1000
    sigs, _ = _gen(np.random.default_rng(3), N, S)
    bits = sigs.view(np.uint64)
    sentinel = np.full(N * N, 0xA5A5A5A5, np.uint32)
    dg, dl = gpu_ctx.malloc(sentinel.nbytes), gpu_ctx.malloc(sentinel.nbytes)

    def untouched():
        for d in (dg, dl):
            back = np.empty_like(sentinel)
            gpu_ctx.d2h(back, d)
            np.testing.assert_array_equal(back, sentinel)

    try:
        gpu_ctx.h2d(dg, sentinel)
        gpu_ctx.h2d(dl, sentinel)
        for algo in (d2g.CMP_AUTO, d2g.CMP_BITSLICE):
            cs = gpu_ctx.cmp_set(bits, algo=algo)
            assert cs.algo == d2g.CMP_BITSLICE
            with pytest.raises(d2g.D2GError):
                cs.gtlt_ut_dev(dg, dl)
            with pytest.raises(d2g.D2GError):
                cs.gtlt_rect_dev(dg, dl, 0, N, 0, N)
            with pytest.raises(d2g.D2GError):
                cs.gtlt_ut()
            cs.close()
            untouched()
        cs = gpu_ctx.cmp_set(bits, algo=d2g.CMP_DIRECT)
        for a0, a1, b0, b1 in [(0, N + 1, 0, N), (5, 3, 0, N), (0, N, 10, 9), (0, N, 0, N + 1)]:
            with pytest.raises(d2g.D2GError):
                cs.gtlt_rect_dev(dg, dl, a0, a1, b0, b1)
        with pytest.raises(d2g.D2GError):
            cs.gtlt_ut_dev(dg, dl, 0, N + 1)
        gpu_ctx.sync()
        untouched()
        cs.close()
    finally:
        gpu_ctx.free(dg)
        gpu_ctx.free(dl)
