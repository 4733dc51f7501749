"""Sets of truncated codes on the GPU: the bit-plane (gt, lt) kernel of d2g_k2_planes.hip behind d2g_cmp_gtlt_* / d2g_cmp_eqcount_*,
and d2g_cmp_dist_trunc_ut on top of it.

The integer counts are pinned to implementations that share no code with the kernel: blocked NumPy comparisons of the codes
(tests/trunc_ref.py), counts known by construction, the direct 64-bit kernel on the widened codes, per-column rank sums.  The float
values are compared bit for bit with the NumPy restatement of the reference, computed LIVE in the test process (powl/logl/expl belong to
the machine's libm).  Both epilogue formulas are symmetric in (gt, lt): a swapped orientation can only be caught by the integer tests;
the float tests first show that their data tell (gt, lt) from (gt + lt, 0), which an equality-only kernel would deliver."""
import os

import numpy as np
import pytest

import trunc_cases as TC
import trunc_ref as R

pytestmark = pytest.mark.gpu
NT = min(16, int(os.environ.get("OMP_NUM_THREADS") or 0) or (os.cpu_count() or 1))
DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}

# (N, S): S in {1, 3, 33, 1000, 1023, 1025} is no multiple of the 32-register group, N in {1, 2, 33, 257, 4097} is off the 32 x 256 tile grid
UT_CASES = [(1, 1), (1, 1000), (2, 1), (2, 3), (2, 1023), (33, 1), (33, 3), (33, 33), (33, 1025), (257, 3), (257, 1000), (257, 1023),
            (600, 1025), (1000, 33), (4097, 3)]


def _ut(sq):
    return sq[np.triu_indices(sq.shape[0], 1)]


@pytest.mark.parametrize("regbytes", [1, 2, 4])
@pytest.mark.parametrize("N,S", UT_CASES)
def test_codes_gtlt_ut_exact(gpu_ctx, d2g, N, S, regbytes):
    """(gt, lt) of the triangle and of row ranges that start off the tile grid; S - gt - lt from the equality-count entry point; the
    same counts from the direct kernel on the codes widened to 64 bits"""
    rng = np.random.default_rng(N * 131 + S * 7 + regbytes)
    codes = TC.gen_codes(rng, N, S, DTYPES[regbytes])
    eg, el = R.gtlt_rect(codes, 0, N, 0, N)
    egt, elt = _ut(eg), _ut(el)
    cs = gpu_ctx.cmp_set_codes(codes)
    assert cs.algo == d2g.CMP_PLANES
    assert cs.operand_bytes <= ((N + 255) // 256 * 256 + 64) * ((S + 31) // 32 * 32) * regbytes      # about N * S * regbytes, not N * S * 8
    gt, lt = cs.gtlt_ut()
    np.testing.assert_array_equal(gt, egt)
    np.testing.assert_array_equal(lt, elt)
    np.testing.assert_array_equal(cs.eqcount_ut(), S - egt.astype(np.int64) - elt)
    if N >= 33:
        assert ((gt == 0) & (lt == 0)).any() and ((gt == S) | (lt == S)).any() and (S == 1 or ((gt > 0) & (lt > 0)).any())
    b = d2g.ut_partition(N, 3)
    for r0, r1 in [(b[i], b[i + 1]) for i in range(3)] + [(31, 33), (255, N), (1, 2), (N // 2 + 1, N - 1), (N - 1, N)]:
        if not 0 <= r0 <= r1 <= N:
            continue
        o0, o1 = d2g.ut_count(N, 0, r0), d2g.ut_count(N, 0, r1)
        g, l = cs.gtlt_ut(r0, r1)
        np.testing.assert_array_equal(g, egt[o0:o1], err_msg=f"rows {r0}:{r1}")
        np.testing.assert_array_equal(l, elt[o0:o1], err_msg=f"rows {r0}:{r1}")
        np.testing.assert_array_equal(cs.eqcount_ut(r0, r1), S - egt[o0:o1].astype(np.int64) - elt[o0:o1], err_msg=f"rows {r0}:{r1}")
    cs.close()
    ds = gpu_ctx.cmp_set(codes.astype(np.uint64), algo=d2g.CMP_DIRECT)           # a second implementation, tested on its own
    dg, dl = ds.gtlt_ut()
    ds.close()
    np.testing.assert_array_equal(gt, dg)
    np.testing.assert_array_equal(lt, dl)


@pytest.mark.parametrize("regbytes", [1, 2, 4])
@pytest.mark.parametrize("N,S", [(1, 1000), (33, 3), (257, 1025), (600, 1023), (1000, 33)])
def test_codes_gtlt_rect_exact(gpu_ctx, d2g, N, S, regbytes):
    """rectangles, gt = #(row code > column code): the square with its orientation checks, blocks off the tile grids, a panel split at a
    row that is no tile edge, one row, one column"""
    rng = np.random.default_rng(N * 17 + S + regbytes)
    codes = TC.gen_codes(rng, N, S, DTYPES[regbytes])
    cs = gpu_ctx.cmp_set_codes(codes)
    g, l = cs.gtlt_rect(0, N, 0, N)
    eg, el = R.gtlt_rect(codes, 0, N, 0, N)
    np.testing.assert_array_equal(g, eg)
    np.testing.assert_array_equal(l, el)
    np.testing.assert_array_equal(g, l.T)
    assert not np.diag(g).any() and not np.diag(l).any()
    np.testing.assert_array_equal(cs.eqcount_rect(0, N, 0, N), S - eg.astype(np.int64) - el)
    ugt, ult = cs.gtlt_ut()
    iu = np.triu_indices(N, 1)
    np.testing.assert_array_equal(g[iu], ugt)
    np.testing.assert_array_equal(l[iu], ult)
    nf = N - N // 3
    for a0, a1, b0, b1 in [(5, 5 + 97, 3, N), (N // 3 + 1, N - 2, N // 2 + 7, N - 1), (33, N, 257, N), (0, nf, nf, N), (nf, N, 0, nf),
                           (N - 1, N, 0, N), (0, 1, 0, N), (0, N, N - 1, N), (0, N, N // 2, N // 2 + 1)]:
        a1, b1 = min(a1, N), min(b1, N)
        if not (0 <= a0 < a1 and 0 <= b0 < b1):
            continue
        bg, bl = cs.gtlt_rect(a0, a1, b0, b1)
        np.testing.assert_array_equal(bg, eg[a0:a1, b0:b1], err_msg=str((a0, a1, b0, b1)))
        np.testing.assert_array_equal(bl, el[a0:a1, b0:b1], err_msg=str((a0, a1, b0, b1)))
        np.testing.assert_array_equal(cs.eqcount_rect(a0, a1, b0, b1), S - eg[a0:a1, b0:b1].astype(np.int64) - el[a0:a1, b0:b1])
    cs.close()


@pytest.mark.parametrize("regbytes", [1, 2, 4])
def test_codes_planted_pairs_by_construction(gpu_ctx, regbytes):
    """pairs whose counts follow from how they were built: identical rows, one row above the other in every register, codes that differ
    in the lowest bit only, in the highest bit only, 0 against the largest code, and -- 2 and 4 bytes -- high halves equal with low
    halves different and the reverse (a comparator that drops, repeats or reverses a plane gets these wrong)"""
    P, S, K = 8 * regbytes, 70, 9
    top = (1 << P) - 1
    rng = np.random.default_rng(regbytes)
    a = rng.integers(0, top + 1, (7, K, S), dtype=np.uint64)
    b = a.copy()
    a[1] = np.minimum(a[1], np.uint64(top - 1))
    b[1] = a[1] + np.uint64(1)
    b[2] = a[2] ^ np.uint64(1)
    b[3] = a[3] ^ np.uint64(1 << (P - 1))
    a[4], b[4] = 0, top
    lo_mask = np.uint64((1 << (P // 2)) - 1)
    hi_mask = np.uint64(top) ^ lo_mask
    b[5] = (a[5] & hi_mask) | ((a[5] + np.uint64(1) + rng.integers(0, int(lo_mask), a[5].shape, dtype=np.uint64)) & lo_mask)    # low halves differ everywhere
    hi_new = ((a[6] >> np.uint64(P // 2)) + np.uint64(1) + rng.integers(0, int(lo_mask), a[6].shape, dtype=np.uint64)) & lo_mask
    b[6] = (a[6] & lo_mask) | (hi_new << np.uint64(P // 2))                                                                    # high halves differ everywhere
    want_gt = [np.zeros(K, np.int64), np.zeros(K, np.int64), (a[2] & np.uint64(1)).sum(-1).astype(np.int64),
               ((a[3] >> np.uint64(P - 1)) & np.uint64(1)).sum(-1).astype(np.int64), np.zeros(K, np.int64),
               ((a[5] & lo_mask) > (b[5] & lo_mask)).sum(-1).astype(np.int64), ((a[6] & hi_mask) > (b[6] & hi_mask)).sum(-1).astype(np.int64)]
    want_lt = [np.zeros(K, np.int64), np.full(K, S)] + [S - w for w in want_gt[2:4]] + [np.full(K, S)] + [S - w for w in want_gt[5:]]
    codes = np.concatenate([a.reshape(-1, S), b.reshape(-1, S)]).astype(DTYPES[regbytes])
    n = 7 * K
    cs = gpu_ctx.cmp_set_codes(codes)
    g, l = cs.gtlt_rect(0, n, n, 2 * n)                       # rows a against columns b
    g2, l2 = cs.gtlt_rect(n, 2 * n, 0, n)                     # and the other way round
    cs.close()
    for q in range(7):
        d = np.arange(q * K, (q + 1) * K)
        np.testing.assert_array_equal(g[d, d], want_gt[q], err_msg=f"kind {q}")
        np.testing.assert_array_equal(l[d, d], want_lt[q], err_msg=f"kind {q}")
        np.testing.assert_array_equal(g2[d, d], want_lt[q], err_msg=f"kind {q} reversed")
        np.testing.assert_array_equal(l2[d, d], want_gt[q], err_msg=f"kind {q} reversed")


def test_codes_scale_n10000_s1024(gpu_ctx, d2g):
    """the flagship shape at one byte: every row's total of #(row > other) and #(row < other) against per-column rank counts"""
    N, S = 10_000, 1024
    rng = np.random.default_rng(10_000)
    codes = TC.gen_codes(rng, N, S, np.uint8)
    egt, elt = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for t in range(S):
        col = np.sort(codes[:, t])
        egt += np.searchsorted(col, codes[:, t], side="left")
        elt += N - np.searchsorted(col, codes[:, t], side="right")
    cs = gpu_ctx.cmp_set_codes(codes)
    rgt, rlt = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for a0 in range(0, N, 1250):
        g, l = cs.gtlt_rect(a0, a0 + 1250, 0, N)
        rgt[a0:a0 + 1250], rlt[a0:a0 + 1250] = g.sum(axis=1, dtype=np.int64), l.sum(axis=1, dtype=np.int64)
        del g, l
    np.testing.assert_array_equal(rgt, egt)
    np.testing.assert_array_equal(rlt, elt)
    # the triangle's addressing at this size: its last rows and one range in the middle against the rectangle
    for r0, r1 in [(N - 300, N), (4099, 4140)]:
        g, l = cs.gtlt_ut(r0, r1)
        rg, rl = cs.gtlt_rect(r0, r1, 0, N)
        i, j = R.ut_index(N, r0, r1)
        np.testing.assert_array_equal(g, rg[i - r0, j])
        np.testing.assert_array_equal(l, rl[i - r0, j])
    cs.close()


_FLOAT_DATA = {}


def _float_data():
    if not _FLOAT_DATA:
        rng = np.random.default_rng(2026)
        _FLOAT_DATA["sigs"], _FLOAT_DATA["cards"] = TC.oph_shaped(rng, 300, 100, families=3, unrelated=10, empty_rows=2)
    return _FLOAT_DATA["sigs"], _FLOAT_DATA["cards"]


@pytest.mark.parametrize("bbit", [False, True])
@pytest.mark.parametrize("regbytes", [1, 2, 4])
def test_dist_trunc_ut_bit_exact(gpu_ctx, d2g, regbytes, bbit):
    """d2g_cmp_dist_trunc_ut (truncate, upload, count, epilogue) for every measure, families and unrelated rows and empty sketches
    mixed, S = 100: bit for bit against the restatement computed here.  The formulas are symmetric in (gt, lt) -- orientation is the
    integer tests' business -- but not linear: each setsketch case first shows at least five pairs whose value changes under
    (gt + lt, 0)"""
    sigs, cards = _float_data()
    N, S = sigs.shape
    codes, a, b, _, _ = R.truncate(sigs, regbytes, bbit)
    g, l = R.gtlt_ut(codes)
    i, j = R.ut_index(N)
    r0, r1 = 37, 211
    o0, o1 = d2g.ut_count(N, 0, r0), d2g.ut_count(N, 0, r1)
    for meas in range(6):
        if bbit:
            exp = R.epilogue_bbit(S - g.astype(np.int64) - l, S, regbytes, cards[i], cards[j], meas, 21)
        else:
            exp = R.epilogue_gtlt(g, l, S, b, cards[i], cards[j], meas, 21)
            merged = R.epilogue_gtlt(g.astype(np.int64) + l, np.zeros_like(l), S, b, cards[i], cards[j], meas, 21)
            nsens = int((merged.view(np.uint32) != exp.view(np.uint32)).sum())
            assert nsens >= 5, f"the data cannot tell (gt, lt) from (gt + lt, 0): {nsens} sensitive pairs (measure {meas})"
        got = gpu_ctx.cmp_dist_trunc_ut(sigs, cards, measure=meas, k=21, regbytes=regbytes, bbit=bbit, nthreads=NT)
        np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32), err_msg=f"measure {meas}")
        part = gpu_ctx.cmp_dist_trunc_ut(sigs, cards, measure=meas, k=21, regbytes=regbytes, bbit=bbit, r0=r0, r1=r1, nthreads=NT)
        np.testing.assert_array_equal(part.view(np.uint32), exp[o0:o1].view(np.uint32), err_msg=f"measure {meas} rows {r0}:{r1}")


def test_code_set_refusals_leave_the_output_alone(gpu_ctx, d2g):
    """what needs 64-bit patterns, ids or the sparse path refuses a set of codes and writes nothing; so do bad shapes"""
    N, S = 300, 100
    codes = TC.gen_codes(np.random.default_rng(3), N, S, np.uint16)
    sentinel = np.full(N * N, 0xA5A5A5A5, np.uint32)
    d1, d2 = gpu_ctx.malloc(sentinel.nbytes), gpu_ctx.malloc(sentinel.nbytes)
    cs = gpu_ctx.cmp_set_codes(codes)
    try:
        gpu_ctx.h2d(d1, sentinel)
        gpu_ctx.h2d(d2, sentinel)
        for call in (lambda: cs.lut_ut_dev(d2, d1), lambda: cs.prefill_ut_dev(d1), lambda: cs.prefill_ut_dev(d1, lut_dev_ptr=d2),
                     lambda: cs.announce_ut_dev(d1), lambda: cs.export_operand_dev(d1, d2), lambda: cs.update_dev(d1),
                     lambda: cs.gtlt_ut_dev(d1, d2, 0, N + 1), lambda: cs.gtlt_rect_dev(d1, d2, 0, N, 0, N + 1),
                     lambda: cs.eqcount_rect_dev(d1, 5, 3, 0, N), lambda: cs.eqcount_ut_dev(d1, 0, N + 1)):
            with pytest.raises(d2g.D2GError):
                call()
        for call in (cs.sparse_info, cs.sparse_detail, lambda: cs.debug_pairs(cap=16)):
            with pytest.raises(d2g.D2GError):
                call()
        info = np.full(4, 0xA5A5A5A5, np.uint32)
        assert d2g.lib().d2g_cmp_set_sparse_info(gpu_ctx._h, cs._h, None, info.ctypes.data) == -1 and (info == 0xA5A5A5A5).all()
        gpu_ctx.sync()
        for d in (d1, d2):
            back = np.empty_like(sentinel)
            gpu_ctx.d2h(back, d)
            np.testing.assert_array_equal(back, sentinel)
        with pytest.raises(d2g.D2GError):
            gpu_ctx.cmp_set_codes_dev(d1, N, S, 3)
        with pytest.raises(d2g.D2GError):
            gpu_ctx.cmp_dist_trunc_ut(np.zeros((4, 8)), np.ones(4), regbytes=1)          # no positive register
    finally:
        cs.close()
        gpu_ctx.free(d1)
        gpu_ctx.free(d2)
