"""GPU parity tests for K2 (dense all-pairs comparison) through the C ABI.
Integer counts are compared BIT-EXACTLY with the oracle and with the reference's own NumPy
implementation (frozen golden vectors); float32 outputs are compared bit-exactly too
(tolerance stated by north_star: 1e-6; we hold 0)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from dashing2_amd import synth

pytestmark = pytest.mark.gpu

ALGOS = ["direct", "bitslice"]


def _algo(d2g, name):
    return {"direct": d2g.CMP_DIRECT, "bitslice": d2g.CMP_BITSLICE, "auto": d2g.CMP_AUTO}[name]


def _planted(rng, N, S, nvals=5, zero_frac=0.05):
    vals = rng.random((nvals, S))
    m = vals[rng.integers(0, nvals, (N, S)), np.arange(S)[None, :]]
    m[rng.random((N, S)) < zero_frac] = 0.0
    return m


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", ["eqcount_n7_s16", "eqcount_n33_s64", "eqcount_n64_s128", "eqcount_n40_s100"])
def test_k2_golden_reference_numpy(gpu_ctx, d2g, algo, name):
    """expected = python/parse.py:128-156 pairwise_equality_compare (the reference's own code)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    got = gpu_ctx.cmp_eqcount_ut(z["sigs"].view(np.uint64), algo=_algo(d2g, algo))
    np.testing.assert_array_equal(got, z["expected"])


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("N,S", [(1, 16), (2, 2), (3, 1024), (65, 32), (257, 64), (300, 1000), (513, 96), (700, 33)])
def test_k2_eqcount_vs_oracle(gpu_ctx, d2g, oracle, algo, N, S):
    rng = np.random.default_rng(N * 7 + S)
    sigs = _planted(rng, N, S, nvals=int(rng.integers(2, 9)))
    exp = oracle.eqcounts_ut(sigs)
    cs = gpu_ctx.cmp_set(sigs.view(np.uint64), algo=_algo(d2g, algo))
    assert cs.algo == _algo(d2g, algo)
    got = cs.eqcount_ut()
    np.testing.assert_array_equal(got, exp)
    # row ranges (what a rank computes when the triangle is sharded) concatenate to the full result
    b = d2g.ut_partition(N, 3)
    parts = [cs.eqcount_ut(b[i], b[i + 1]) for i in range(3)]
    np.testing.assert_array_equal(np.concatenate(parts), exp)
    # rectangular blocks (asymmetric all-pairs / panel: emitrect.cpp:211-268)
    full = cs.eqcount_rect(0, N, 0, N)
    iu = np.triu_indices(N, 1)
    np.testing.assert_array_equal(full[iu], exp)
    np.testing.assert_array_equal(full, full.T)
    np.testing.assert_array_equal(np.diag(full), np.full(N, S, np.uint32))
    if N > 10:
        a0, a1, b0, b1 = 3, N // 2, N // 3, N - 1
        np.testing.assert_array_equal(cs.eqcount_rect(a0, a1, b0, b1), full[a0:a1, b0:b1])
    cs.close()


def test_k2_gtlt_vs_oracle(gpu_ctx, d2g, oracle):
    rng = np.random.default_rng(99)
    for N, S in [(37, 100), (130, 64), (260, 1000)]:
        sigs = _planted(rng, N, S, nvals=4)
        cs = gpu_ctx.cmp_set(sigs.view(np.uint64), algo=d2g.CMP_DIRECT)
        gt, lt = cs.gtlt_ut()
        idx = 0
        for i in range(N):
            for j in range(i + 1, N):
                if (idx % 37) == 0 or N < 50:
                    eg, el = oracle.count_gtlt(sigs[i], sigs[j])
                    assert (gt[idx], lt[idx]) == (eg, el)
                idx += 1
        eq = oracle.eqcounts_ut(sigs)
        np.testing.assert_array_equal(S - gt - lt, eq)          # cmp_core.cpp:465 invariant
        cs.close()


@pytest.mark.parametrize("S,multiset", [(64, False), (100, False), (128, True), (100, True)])
def test_k2_dist_all_measures_bit_exact(gpu_ctx, d2g, oracle, S, multiset):
    """full compare(): every measure, power-of-two and non-power-of-two S, set and multiset space."""
    rng = np.random.default_rng(S)
    N = 61
    sigs = _planted(rng, N, S, nvals=3, zero_frac=0.0)
    sigs[7] = sigs[3]                                 # identical pair: sim 1, mash distance 0
    sigs[9] = rng.random(S) + 2.0                     # disjoint from everything: sim 0, mash distance inf
    cards = rng.random(N) * 1e6 + 10
    for meas in range(6):
        got = gpu_ctx.cmp_dist_ut(sigs.view(np.uint64), cards, measure=meas, k=31, multiset_space=multiset, nthreads=2)
        if multiset:
            eq = oracle.eqcounts_ut(sigs)
            exp = np.empty(eq.size, np.float32)
            idx = 0
            for i in range(N):
                for j in range(i + 1, N):
                    exp[idx] = oracle.compare_from_neq(int(eq[idx]), S, cards[i], cards[j], meas, 31)
                    idx += 1
        else:
            exp = oracle.allpairs_ut(sigs, cards, measure=meas, k=31, nthreads=2)
        np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32), err_msg=f"measure {meas}")


def test_k2_lut_fused_epilogue(gpu_ctx, d2g, oracle):
    rng = np.random.default_rng(4)
    N, S = 300, 1024
    sigs = _planted(rng, N, S, nvals=6)
    cards = np.ones(N)
    for algo in ALGOS:
        cs = gpu_ctx.cmp_set(sigs.view(np.uint64), algo=_algo(d2g, algo))
        for meas in (d2g.SIMILARITY, d2g.POISSON_LLR):
            got = cs.lut_ut(d2g.epilogue_lut(S, meas, 31))
            exp = oracle.allpairs_ut(sigs, cards, measure=meas, k=31, nthreads=4)
            np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
        cs.close()


def _column_pair_totals(bits):
    """independent O(N S log N) check values: sum over all pairs of neq, and per-row sums."""
    N, S = bits.shape
    row = np.zeros(N, np.int64)
    total = 0
    for t in range(S):
        _, inv, cnt = np.unique(bits[:, t], return_inverse=True, return_counts=True)
        total += int((cnt.astype(np.int64) * (cnt - 1) // 2).sum())
        row += cnt[inv] - 1
    return total, row


@pytest.mark.parametrize("algo", ALGOS)
def test_k2_full_size_properties(gpu_ctx, d2g, algo):
    """BASELINE config 3 size (N = 10 000, S = 1024): size-independent properties.
    checksum of checksums: sum_pairs neq == sum_t sum_v C(count_v, 2); row sums likewise;
    sharded rows == unsharded; symmetric rect block == transposed UT entries."""
    N, S = 10_000, 1024
    regs = synth.synthetic_registers(N, S, nclusters=50, seed=7)
    sigs, _ = d2g.oph_finalize(regs, S, nthreads=8)
    bits = sigs.view(np.uint64)
    cs = gpu_ctx.cmp_set(bits, algo=_algo(d2g, algo))
    neq = cs.eqcount_ut()
    assert neq.size == N * (N - 1) // 2
    total, rowsum = _column_pair_totals(bits)
    assert int(neq.sum(dtype=np.int64)) == total
    # per-row sums: row i of the symmetric matrix = UT row i + UT column i
    off = np.concatenate([[0], np.cumsum(N - 1 - np.arange(N))])
    got_row = np.zeros(N, np.int64)
    for i in range(N - 1):
        seg = neq[off[i]:off[i + 1]]
        got_row[i] += int(seg.sum(dtype=np.int64))       # pairs (i, j>i)
        got_row[i + 1:] += seg                            # the same pairs seen from j
    np.testing.assert_array_equal(got_row, rowsum)
    assert neq.max() <= S
    # sharding invariance on a few row ranges
    b = d2g.ut_partition(N, 8)
    for p in (0, 3, 7):
        part = cs.eqcount_ut(b[p], b[p + 1])
        np.testing.assert_array_equal(part, neq[off[b[p]]:off[b[p + 1]]])
    # rect block consistency
    blk = cs.eqcount_rect(100, 164, 5000, 5300)
    for ii in (100, 131, 163):
        np.testing.assert_array_equal(blk[ii - 100], neq[off[ii] + (5000 - ii - 1): off[ii] + (5300 - ii - 1)])
    cs.close()


def test_k2_direct_equals_bitslice_midsize(gpu_ctx, d2g):
    N, S = 3000, 2048
    regs = synth.synthetic_registers(N, S, nclusters=10, seed=11, share_lo=0.5, share_hi=1.0)
    bits = regs            # raw u64 ids are valid operands too (cmp_core.cpp:497-505 compares k-mers)
    a = gpu_ctx.cmp_eqcount_ut(bits, algo=d2g.CMP_DIRECT)
    b = gpu_ctx.cmp_eqcount_ut(bits, algo=d2g.CMP_BITSLICE)
    np.testing.assert_array_equal(a, b)
    assert a.max() > S // 2 and a.min() < S // 4


def test_k2_rejects_bad_input(gpu_ctx, d2g):
    sigs = np.zeros((4, 8), np.uint64)
    cs = gpu_ctx.cmp_set(sigs)
    with pytest.raises(d2g.D2GError):
        cs.eqcount_ut(3, 2)
    with pytest.raises(d2g.D2GError):
        cs.eqcount_ut(0, 5)
    with pytest.raises(d2g.D2GError):
        gpu_ctx.cmp_dist_ut(sigs, np.ones(4), measure=17)
    cs.close()


@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_k2_sharded_prepare_single_gpu(gpu_ctx, d2g, oracle, W):
    """multi-GPU prepare simulated rank by rank on one GPU: every 'rank' builds the bit-sliced
    groups of its S/W columns from its column slice; the concatenation (what the all-gather produces)
    wrapped by d2g_cmp_set_from_planes_dev must give the oracle's counts for every row range."""
    rng = np.random.default_rng(W)
    N, S = (264 if W == 8 else 260), 256
    sigs = _planted(rng, N, S, nvals=5)
    bits = sigs.view(np.uint64)
    gw, ng = d2g.operand_layout(N, S)
    S_loc = S // W
    gw_l, ng_l = d2g.operand_layout(N, S_loc)
    assert gw_l == gw and ng_l * W == ng
    planes_all = gpu_ctx.malloc(ng * gw * 4)
    meta_all = gpu_ctx.malloc(ng * 4)
    n_loc = N // W
    # pack + "all-to-all" emulated on the host: rank q receives columns [q*S_loc, (q+1)*S_loc) of all rows
    rows_dev = gpu_ctx.malloc(n_loc * S * 8)
    send_dev = gpu_ctx.malloc(n_loc * S * 8)
    sends = []
    for r in range(W):
        gpu_ctx.h2d(rows_dev, np.ascontiguousarray(bits[r * n_loc:(r + 1) * n_loc]))
        gpu_ctx.pack_column_slices_dev(rows_dev, n_loc, S, W, send_dev)
        buf = np.empty((W, n_loc, S_loc), np.uint64)
        gpu_ctx.d2h(buf, send_dev)
        sends.append(buf)
    for q in range(W):
        colslice = np.concatenate([sends[r][q] for r in range(W)], axis=0)          # [N][S_loc]
        np.testing.assert_array_equal(colslice, bits[:n_loc * W, q * S_loc:(q + 1) * S_loc])
    if N % W:
        pytest.skip("N not divisible")
    for q in range(W):
        cs = gpu_ctx.cmp_set(np.ascontiguousarray(bits[:, q * S_loc:(q + 1) * S_loc]), algo=d2g.CMP_BITSLICE)
        cs.export_operand_dev(planes_all + q * ng_l * gw * 4, meta_all + q * ng_l * 4)
        gpu_ctx.sync()
        cs.close()
    full = gpu_ctx.cmp_set_from_planes(N, S, planes_all, meta_all)
    exp = oracle.eqcounts_ut(sigs)
    np.testing.assert_array_equal(full.eqcount_ut(), exp)
    b = d2g.ut_partition(N, 3)
    np.testing.assert_array_equal(np.concatenate([full.eqcount_ut(b[i], b[i + 1]) for i in range(3)]), exp)
    with pytest.raises(d2g.D2GError):
        full.gtlt_ut()                      # a gathered operand has no raw patterns
    full.close()
    for p_ in (planes_all, meta_all, rows_dev, send_dev):
        gpu_ctx.free(p_)


def test_row_sharded_allpairs_world1(gpu_ctx, d2g, oracle):
    """the torch-facing multi-GPU driver (dashing2_amd.dist.RowShardedAllPairs) in its degenerate
    single-rank form: same library calls and buffers as the N>1 path, no process group."""
    import torch
    from dashing2_amd import dist as DD
    rng = np.random.default_rng(77)
    N, S = 384, 1024
    sigs = _planted(rng, N, S, nvals=6)
    dev = torch.device("cuda", 0)
    rows = torch.from_numpy(sigs.view(np.int64)).to(dev)
    eng = DD.RowShardedAllPairs(gpu_ctx, N, S, dev)
    out = torch.empty(N * (N - 1) // 2, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(2):                                   # second pass reuses every buffer (update path)
        eng.step_eqcount(rows, out, stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), oracle.eqcounts_ut(sigs))
    lut = torch.from_numpy(d2g.epilogue_lut(S, d2g.POISSON_LLR, 31)).to(dev)
    fout = torch.empty(N * (N - 1) // 2, dtype=torch.float32, device=dev)
    eng.step_lut(rows, lut, fout, stream)
    torch.cuda.synchronize()
    exp = oracle.allpairs_ut(sigs, np.ones(N), measure=oracle.POISSON_LLR, k=31, nthreads=4)
    np.testing.assert_array_equal(fout.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    eng.close()


@pytest.mark.parametrize("N,tagbits", [(23_000, None), (23_000, "9"), (14_000, None), (14_000, "9")])
def test_k2_large_n_multi_partition(gpu_ctx, d2g, monkeypatch, N, tagbits):
    """N > 21 845 takes the multi-partition rank kernel (hash space walked in LDS-sized pieces), 12 288 < N <= 21 845 the
    general single-partition one; with D2G_BS_TAGBITS=9 a few hundred values per column collide on their tag and go
    through the exact serial chain.  Checked against the independent DIRECT algorithm and the column-count checksum."""
    if tagbits:
        monkeypatch.setenv("D2G_BS_TAGBITS", tagbits)
    S = 64
    regs = synth.synthetic_registers(N, S, nclusters=120, seed=3)
    cs = gpu_ctx.cmp_set(regs, algo=d2g.CMP_BITSLICE)
    a = cs.eqcount_ut()
    md, nb, mean = cs.planes()
    assert 2 <= md <= N and 1 <= nb <= 15
    cs.close()
    total, _ = _column_pair_totals(regs)
    assert int(a.sum(dtype=np.int64)) == total
    b = gpu_ctx.cmp_eqcount_ut(regs, algo=d2g.CMP_DIRECT)
    np.testing.assert_array_equal(a, b)


def test_k2_sharded_prepare_8gpu_bench_shape(gpu_ctx, d2g):
    """the operand the 8-GPU bench step assembles (N = 28288 = 10000*sqrt(8) rounded to 8, S = 1024:
    each rank prepares 128 columns with the two-partition rank kernel, 15+1 plane slots per group),
    simulated rank by rank on one GPU, must count exactly like the unsharded operand."""
    from dashing2_amd import synth
    N, S, W = 28288, 1024, 8
    regs = synth.synthetic_registers(N, S, nclusters=N // 150, seed=8)
    bits = d2g.oph_finalize(regs, S, nthreads=16)[0].view(np.uint64)
    gw, ng = d2g.operand_layout(N, S)
    S_loc = S // W
    gw_l, ng_l = d2g.operand_layout(N, S_loc)
    assert gw_l == gw and ng_l * W == ng
    planes_all = gpu_ctx.malloc(ng * gw * 4)
    meta_all = gpu_ctx.malloc(ng * 4)
    for q in range(W):
        cs = gpu_ctx.cmp_set(np.ascontiguousarray(bits[:, q * S_loc:(q + 1) * S_loc]), algo=d2g.CMP_BITSLICE)
        cs.export_operand_dev(planes_all + q * ng_l * gw * 4, meta_all + q * ng_l * 4)
        gpu_ctx.sync()
        cs.close()
    full = gpu_ctx.cmp_set_from_planes(N, S, planes_all, meta_all)
    ref = gpu_ctx.cmp_set(bits, algo=d2g.CMP_BITSLICE)
    b = d2g.ut_partition(N, W)
    for r0, r1 in ((0, 1500), (b[3], b[3] + 1200), (N - 4000, N)):
        np.testing.assert_array_equal(full.eqcount_ut(r0, r1), ref.eqcount_ut(r0, r1))
    full.close()
    ref.close()
    gpu_ctx.free(planes_all)
    gpu_ctx.free(meta_all)


def test_row_sharded_pipelined_steps_keep_order(gpu_ctx, d2g, oracle):
    """enqueue_lut overlaps the exchange + prepare of step i+1 with the pair kernel of step i over two
    operand buffers.  Seven steps over DIFFERENT inputs, each result copied out on the main stream right
    after its step was enqueued, must equal the plain per-step results (no buffer is reused too early)."""
    import torch
    from dashing2_amd import dist as DD
    rng = np.random.default_rng(99)
    N, S = 512, 1024
    dev = torch.device("cuda", 0)
    eng = DD.RowShardedAllPairs(gpu_ctx, N, S, dev)
    lut = torch.from_numpy(d2g.epilogue_lut(S, d2g.SIMILARITY, 31)).to(dev)
    out = torch.empty(N * (N - 1) // 2, dtype=torch.float32, device=dev)
    inputs = [_planted(rng, N, S, nvals=3 + i) for i in range(7)]
    rows = [torch.from_numpy(x.view(np.int64)).to(dev) for x in inputs]
    got = []
    for r in rows:
        eng.enqueue_lut(r, lut, out)
        got.append(out.clone())                        # main stream: ordered after this step's pair kernel
    torch.cuda.synchronize()
    for x, g in zip(inputs, got):
        exp = oracle.allpairs_ut(x, np.ones(N), measure=oracle.SIMILARITY, k=31, nthreads=4)
        np.testing.assert_array_equal(g.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    eng.close()


def test_k2_config4_size_vs_oracle(gpu_ctx, d2g, oracle):
    """BASELINE config 4's size on ONE GPU (N = 50 000, S = 1024: 410 MB operand, 1 249 975 000 pairs, 5 GB
    of output).  The whole triangle is checked through size-independent properties (checksum of checksums
    from per-column value counts; every per-row sum) and sampled row ranges are compared value for value
    with the ORACLE (equality counts through its float32 SIMILARITY = neq/1024, exact for S = 2^10):
    the first rows, the seam between two of the 8 row shards, the middle, and the last rows.  The whole output again through the announced
    path (the 5 GB fill on a second stream)."""
    import torch
    N, S = 50_000, 1024
    regs = synth.synthetic_registers(N, S, nclusters=N // 150, seed=20260929)
    ncpu = os.cpu_count() or 1
    sigs, cards = d2g.oph_finalize(regs, S, nthreads=ncpu)
    del regs
    bits = sigs.view(np.uint64)
    dev = torch.device("cuda", 0)
    t_dev = torch.from_numpy(bits.view(np.int64)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    npairs = N * (N - 1) // 2
    out = torch.empty(npairs, dtype=torch.int32, device=dev)
    cs.eqcount_ut_dev(out.data_ptr(), 0, N, stream)
    torch.cuda.synchronize()
    md, nb, mean = cs.planes(stream)
    assert 2 <= md and nb <= 16
    # checksum of checksums + per-row sums, reduced on the device (plumbing only: sums of the kernel's output)
    total, rowsum = _column_pair_totals(bits)
    assert int(out.sum(dtype=torch.int64).item()) == total
    assert int(out.max().item()) <= S
    off = np.concatenate([[0], np.cumsum(N - 1 - np.arange(N, dtype=np.int64))])
    neq = out.cpu().numpy().view(np.uint32)
    # the same through the ANNOUNCED path (round 6: an output of 1 GB and more is filled by a kernel on a second stream, beside the rank kernel,
    # joined before the launch): announce -> update -> launch twice into a buffer pre-set to garbage, all 1 249 975 000 words equal to the first
    # computation (which the checks below hold against the per-column totals and the oracle)
    out2 = torch.empty(npairs, dtype=torch.int32, device=dev)
    for rep in range(2):
        out2.fill_(-7 - rep)
        cs.announce_ut_dev(out2.data_ptr(), 0, N)
        cs.update_dev(t_dev.data_ptr(), stream)
        cs.eqcount_ut_dev(out2.data_ptr(), 0, N, stream)
        torch.cuda.synchronize()
        assert torch.equal(out, out2), f"announced step {rep}"
    del out2
    # ... and the table form (the fill value comes from lut[0] on the device)
    lut_dev = torch.from_numpy(d2g.epilogue_lut(S, d2g.SIMILARITY, 31)).to(dev)
    fout = torch.full((npairs,), float("nan"), dtype=torch.float32, device=dev)
    cs.announce_ut_dev(fout.data_ptr(), 0, N, lut_dev_ptr=lut_dev.data_ptr())
    cs.update_dev(t_dev.data_ptr(), stream)
    cs.lut_ut_dev(lut_dev.data_ptr(), fout.data_ptr(), 0, N, stream)
    torch.cuda.synchronize()
    CH = 1 << 28
    for a in range(0, npairs, CH):
        assert torch.equal(fout[a:a + CH].view(torch.int32), lut_dev[out[a:a + CH].to(torch.int64)].view(torch.int32)), f"announced table step, words from {a}"
    del out, fout
    got_row = np.zeros(N, np.int64)
    cs_all = np.concatenate([[0], np.cumsum(neq, dtype=np.int64)])
    got_row[:N - 1] = cs_all[off[1:N]] - cs_all[off[:N - 1]]          # pairs (i, j>i)
    del cs_all
    for i in range(N - 1):                                            # the same pairs seen from j
        got_row[i + 1:] += neq[off[i]:off[i + 1]]
    np.testing.assert_array_equal(got_row, rowsum)
    # oracle on sampled row ranges (incl. the seam of the 8-way row partition)
    b = d2g.ut_partition(N, 8)
    lut = d2g.epilogue_lut(S, d2g.SIMILARITY, 31)
    for r0, r1 in ((0, 48), (b[4] - 24, b[4] + 24), (N // 2, N // 2 + 32), (N - 600, N)):
        exp = oracle.allpairs_ut(sigs, cards, measure=oracle.SIMILARITY, k=31, nthreads=ncpu, rows=(r0, r1))
        seg = neq[off[r0]:off[r1]]
        np.testing.assert_array_equal(lut[seg].view(np.uint32), exp.view(np.uint32))
        np.testing.assert_array_equal(cs.eqcount_ut(r0, r1), seg)    # a shard's launch == the whole-triangle launch
        got = cs.lut_ut(lut, r0, r1)                                  # fused float epilogue, bit-exact
        np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32))
    cs.close()


def test_row_sharded_pipelined_input_produced_on_main_stream(gpu_ctx, d2g, oracle):
    """every step's rows are PRODUCED on the caller's stream immediately before enqueue_lut (a long chain of
    device copies ending in the real input, into a buffer that held the previous step's input): the exchange
    stream must wait for the producer (it only did so on the first step)."""
    import torch
    from dashing2_amd import dist as DD
    rng = np.random.default_rng(5)
    N, S = 512, 1024
    dev = torch.device("cuda", 0)
    eng = DD.RowShardedAllPairs(gpu_ctx, N, S, dev)
    lut = torch.from_numpy(d2g.epilogue_lut(S, d2g.SIMILARITY, 31)).to(dev)
    out = torch.empty(N * (N - 1) // 2, dtype=torch.float32, device=dev)
    inputs = [_planted(rng, N, S, nvals=3 + i) for i in range(5)]
    staged = [torch.from_numpy(x.view(np.int64)).to(dev) for x in inputs]
    big = torch.zeros(64 << 20, dtype=torch.int64, device=dev)           # 512 MB: a slow producer
    rows = torch.zeros((N, S), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    got = []
    for st in staged:
        big.add_(1)                                      # main stream: delay, then the real input lands in `rows`
        big.mul_(3)
        rows.copy_(st)
        eng.enqueue_lut(rows, lut, out)
        got.append(out.clone())
    torch.cuda.synchronize()
    for x, g in zip(inputs, got):
        exp = oracle.allpairs_ut(x, np.ones(N), measure=oracle.SIMILARITY, k=31, nthreads=4)
        np.testing.assert_array_equal(g.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    eng.close()


@pytest.mark.parametrize("tagbits", ["8", "0"])
def test_k2_rank_tag_collisions(gpu_ctx, d2g, oracle, monkeypatch, tagbits):
    """The rank kernel stops a probe chain at the first slot whose hash TAG matches and confirms the owner's value
    afterwards; a tag collision resumes the exact chain through a small fix list.  D2G_BS_TAGBITS (test hook) narrows the
    tag: 8 bits -> a handful of collisions per column, all through the list, same exact result; 0 bits -> every occupied
    slot is a candidate, the list overflows, the status word is raised: AUTO falls back to DIRECT, an explicit BITSLICE
    request fails loudly."""
    monkeypatch.setenv("D2G_BS_TAGBITS", tagbits)
    rng = np.random.default_rng(77)
    N, S = 3000, 64
    sigs = _planted(rng, N, S, nvals=40)
    fresh = rng.random((N, S)) < 0.6                     # most values occur once: many occupied slots with other values
    sigs[fresh] = rng.random(int(fresh.sum()))
    exp = oracle.eqcounts_ut(sigs)
    if tagbits == "8":
        cs = gpu_ctx.cmp_set(sigs.view(np.uint64), algo=d2g.CMP_BITSLICE)
        assert cs.algo == d2g.CMP_BITSLICE
    else:
        with pytest.raises(d2g.D2GError):
            gpu_ctx.cmp_set(sigs.view(np.uint64), algo=d2g.CMP_BITSLICE)
        cs = gpu_ctx.cmp_set(sigs.view(np.uint64), algo=d2g.CMP_AUTO)
        assert cs.algo == d2g.CMP_DIRECT
    np.testing.assert_array_equal(cs.eqcount_ut(), exp)
    cs.close()


def test_timing_mask_brackets_only_what_is_asked(gpu_ctx, d2g):
    """d2g_set_timing(mask): an event pair costs device time, so a caller brackets only the kernels it reports
    (bench.py: the pair kernel inside the timed region, the prepare chain on the warmup steps)."""
    rng = np.random.default_rng(5)
    sigs = _planted(rng, 300, 64)
    for mask, want in ((d2g.TIME_K2, (2, 0)), (d2g.TIME_K2PREP, (0, 1)), (True, (2, 1)), (False, (0, 0))):
        gpu_ctx.set_timing(False)
        gpu_ctx.kernel_ms("k2"), gpu_ctx.kernel_ms("k2prep")
        gpu_ctx.set_timing(mask)
        cs = gpu_ctx.cmp_set(sigs.view(np.uint64), algo=d2g.CMP_BITSLICE)       # one prepare
        cs.eqcount_ut(), cs.eqcount_ut()                                         # two pair-kernel launches
        gpu_ctx.set_timing(False)
        n2, avg2, _ = gpu_ctx.kernel_ms("k2")
        np_, avgp, _ = gpu_ctx.kernel_ms("k2prep")
        assert (n2, np_) == want, (mask, n2, np_)
        assert (avg2 > 0) == (n2 > 0) and (avgp > 0) == (np_ > 0)
        cs.close()


def test_k2_column_sort_reduces_planes_counts_unchanged(gpu_ctx, d2g, oracle, monkeypatch):
    """meta[tb] is a per-group MAX, so one busy column used to tax the 31 quiet ones that happened to share
    its group.  bs_colplan_kernel sorts the columns by their live-plane class before grouping (equality counts are sums
    over columns -- reference src/cmp_core.cpp:461,506 -- so any permutation is exact).  On a matrix whose columns share
    between 0 and 64 values (log-uniform) the mean plane count must drop by >= 25 % and every count must stay bit-exact."""
    N, S = 1500, 1024
    regs = synth.skewed_registers(N, S, seed=5)
    exp = oracle.eqcounts_ut(regs.view(np.float64))
    res = {}
    for sort in ("0", "1"):
        monkeypatch.setenv("D2G_BS_SORT", sort)
        cs = gpu_ctx.cmp_set(regs, algo=d2g.CMP_BITSLICE)
        np.testing.assert_array_equal(cs.eqcount_ut(), exp, err_msg=f"sort={sort}")
        res[sort] = cs.planes()
        cs.close()
    assert res["1"][0] == res["0"][0] and res["1"][1] == res["0"][1]         # the busiest column is the same column
    assert res["1"][2] <= 0.75 * res["0"][2], res
    # odd sketch sizes: the padding slots of the last group sort behind every real column
    for S2 in (1000, 33, 31):
        monkeypatch.setenv("D2G_BS_SORT", "1")
        r2 = np.ascontiguousarray(regs[:300, :S2])
        np.testing.assert_array_equal(gpu_ctx.cmp_eqcount_ut(r2, algo=d2g.CMP_BITSLICE), oracle.eqcounts_ut(r2.view(np.float64)))


@pytest.mark.parametrize("N,S,nsplit", [(23_000, 64, "2"), (44_000, 32, "4"), (44_000, 40, "2"), (44_000, 32, "1")])
def test_k2_split_rank_kernel(gpu_ctx, d2g, monkeypatch, N, S, nsplit):
    """Narrow column slices of large N (one chunk of one rank of the 8-GPU exchange: 50 000 x 64) gave the multi-partition
    rank kernel 64 workgroups of one per CU.  Several workgroups now share a column, each walking its share of the hash
    partitions and ranking from 1; the planes kernel adds the offsets.  Checked against DIRECT and the column checksum."""
    monkeypatch.setenv("D2G_BS_NSPLIT", nsplit)
    regs = synth.synthetic_registers(N, S, nclusters=150, seed=int(nsplit) + S)
    cs = gpu_ctx.cmp_set(regs, algo=d2g.CMP_BITSLICE)
    rows = [(0, 300), (N // 2, N // 2 + 300), (N - 2000, N)]
    got = [cs.eqcount_ut(a, b) for a, b in rows]
    md, nb, mean = cs.planes()
    cs.close()
    # the largest number of shared values in any column, counted independently
    want_md = 0
    for t in range(S):
        _, cnt = np.unique(regs[:, t], return_counts=True)
        want_md = max(want_md, int((cnt >= 2).sum()))
    assert md == want_md + 1
    ref = gpu_ctx.cmp_set(regs, algo=d2g.CMP_DIRECT)
    for (a, b), g in zip(rows, got):
        np.testing.assert_array_equal(g, ref.eqcount_ut(a, b))
    ref.close()


@pytest.mark.parametrize("nsplit", ["1", "2"])
def test_k2_multi_partition_rank_kernel_crowded_partitions(gpu_ctx, d2g, monkeypatch, nsplit):
    """The multi-partition rank kernel compacts the values of a pass's hash partition into a queue in LDS (2560 entries) and ranks
    from the queue.  Columns whose values crowd ONE partition -- a constant column, a column of two values, a column where every
    value occurs twice -- fill the queue several times per batch of 8192 values; checked against DIRECT on row ranges."""
    monkeypatch.setenv("D2G_BS_NSPLIT", nsplit)
    N, S = 30_000, 32
    rng = np.random.default_rng(77)
    regs = rng.random((N, S))
    regs[:, 0] = 0.25                                                   # one value: one partition, 30 000 repeats
    regs[:, 1] = np.where(rng.random(N) < 0.5, 0.125, 0.375)           # two values
    half = rng.random(N // 2)
    regs[:, 2] = np.concatenate([half, half])[rng.permutation(N)]      # every value twice: the table at its fullest
    regs[:, 3] = regs[rng.integers(0, 40, N), 3]                        # forty values
    bits = np.ascontiguousarray(regs).view(np.uint64)
    cs = gpu_ctx.cmp_set(bits, algo=d2g.CMP_BITSLICE)
    ref = gpu_ctx.cmp_set(bits, algo=d2g.CMP_DIRECT)
    for a, b in ((0, 200), (N // 2, N // 2 + 200), (N - 1500, N)):
        np.testing.assert_array_equal(cs.eqcount_ut(a, b), ref.eqcount_ut(a, b))
    cs.close(); ref.close()


@pytest.mark.parametrize("S", [4096, 4100, 8200])
def test_k2_column_plan_large_sketch_sizes(gpu_ctx, d2g, oracle, S):
    """the column plan sorts up to 4096 register slots in LDS; larger sketches keep the caller's column order (identity plan).
    Both sides of that limit, with a padded last group, against the oracle."""
    N = 70
    regs = synth.skewed_registers(N, S, seed=S, max_shared=20)
    exp = oracle.eqcounts_ut(regs.view(np.float64))
    cs = gpu_ctx.cmp_set(regs, algo=d2g.CMP_BITSLICE)
    np.testing.assert_array_equal(cs.eqcount_ut(), exp)
    md, nb, mean = cs.planes()
    assert 1 <= nb <= 6 and mean <= nb
    cs.close()


def _ut_offsets(N):
    return np.concatenate([[0], np.cumsum(N - 1 - np.arange(N, dtype=np.int64))])


@pytest.mark.parametrize("variant", ["default", "table_link", "no_link", "short_list", "emit_big", "entry_by_entry", "binned"])
def test_k2_sparse_tiles_and_pair_list_equal_the_direct_kernel_and_the_oracle(gpu_ctx, d2g, oracle, monkeypatch, variant):
    """Round 5: from 8192 sketches on, an upper-triangle launch on a bit-sliced set fills the output with the value of "0 equal", walks
    only the tiles of the FAMILIES the prepare found (sketches that agree in many registers) and adds a list of the pairs of different
    families that share a value -- or, decided on the device, walks every tile.  Whatever it decides, the counts are those of the
    direct 64-bit kernel (itself pinned to the oracle elsewhere) and of 64+ oracle rows per matrix: a family collection, the same with
    1 / 10 / 100 chance collisions per sketch (round 4 listed every tile at 10), an adversarial matrix (a random pairing per column:
    no families, the pair list alone), skewed columns (one family: dense walk), unrelated sketches (the fill alone), chains whose
    neighbours share one register (pair list), one chain of N; whole triangle and row ranges, counts and the fused float epilogue; a
    set RE-LOADED with another matrix.  Variants: no families at all (D2G_SP_LINK=0), a pair list of pairs / 4096 entries (overflow ->
    dense walk), the pair-list kernel with two count words per value, and the two forms the list is applied in (round 6): entry by entry
    (short lists: atomic adds + a leader's table store) and binned by output region + composed in LDS (long lists) -- by default the
    length of the set's last list picks one, here each is forced for every matrix."""
    import torch
    monkeypatch.setenv("D2G_SP_REMEMBER", "0")                         # nine different matrices through ONE set: every prepare decides afresh
    if variant == "table_link":                                        # the form the multi-GPU engine's gathered operand takes: tables in LDS
        monkeypatch.setenv("D2G_SP_OLINK", "0")
    if variant == "no_link":
        monkeypatch.setenv("D2G_SP_LINK", "0")
        monkeypatch.setenv("D2G_SP_LIST_DIV", "2")                     # every equal register pair of the families becomes a list entry: ~20 million
    elif variant == "entry_by_entry":
        monkeypatch.setenv("D2G_SP_LIST_FORM", "1")
    elif variant == "binned":
        monkeypatch.setenv("D2G_SP_LIST_FORM", "2")
    elif variant == "short_list":
        monkeypatch.setenv("D2G_SP_LIST_DIV", "4096")
    elif variant == "emit_big":                                        # the pair list's kernel in the form it takes from 65 536 sketches on
        monkeypatch.setenv("D2G_SP_EMIT_BIG", "1")
    N, S = 12_000, 96
    rng = np.random.default_rng(11)
    chains = rng.random((N, S))
    one_chain = rng.random((N, S))                                     # sketch i shares one register with i + 1, for every i
    for i in range(N - 1):
        one_chain[i + 1, i % S] = one_chain[i, i % S]
        if (i + 1) % 50:
            chains[i + 1, i % S] = chains[i, i % S]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    fam = synth.synthetic_registers(N, S, nclusters=N // 150, seed=3)
    mats = {"families": fam.view(np.float64),
            "families+1": synth.add_chance_collisions(fam, 1, seed=21).view(np.float64),
            "families+10": synth.add_chance_collisions(fam, 10, seed=22).view(np.float64),
            "families+100": synth.add_chance_collisions(fam, S, seed=23).view(np.float64),
            "paired": synth.paired_registers(N, S, seed=4).view(np.float64),
            "skewed": synth.skewed_registers(N, S, seed=5).view(np.float64),
            "unrelated": synth.unrelated_registers(N, S, seed=6).view(np.float64), "chains": chains, "one_chain": one_chain}
    npairs = N * (N - 1) // 2
    out = torch.empty(npairs, dtype=torch.int32, device=dev)
    ref = torch.empty(npairs, dtype=torch.int32, device=dev)
    fout = torch.empty(npairs, dtype=torch.float32, device=dev)
    lut_np = d2g.epilogue_lut(S, d2g.POISSON_LLR, 31, multiset_space=True)     # lut[0] = +inf: the filled word is not zero (S = 96: a table exists in multiset space)
    lut = torch.from_numpy(lut_np).to(dev)
    cs = None
    seen = {}
    off = _ut_offsets(N)
    sample = np.unique(np.concatenate([np.arange(0, 8), rng.integers(0, N - 1, 48), np.arange(N - 10, N - 1)]))
    for name, m in mats.items():
        bits = np.ascontiguousarray(m).view(np.uint64)
        t_dev = torch.from_numpy(bits.view(np.int64)).to(dev)
        if cs is None:
            cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
        else:
            cs.update_dev(t_dev.data_ptr(), stream)                   # same set, another matrix
        out.fill_(-1)
        cs.eqcount_ut_dev(out.data_ptr(), 0, N, stream)
        info = cs.sparse_info(stream)
        seen[name] = info
        fout.fill_(-1.0)
        cs.lut_ut_dev(lut.data_ptr(), fout.data_ptr(), 0, N, stream)
        dr = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_DIRECT, stream=stream)
        dr.eqcount_ut_dev(ref.data_ptr(), 0, N, stream)
        torch.cuda.synchronize()
        assert torch.equal(out, ref), name
        assert torch.equal(fout.view(torch.int32), lut[ref.long()].view(torch.int32)), name     # the table epilogue after the counts: no leader flag survives
        dr.close()
        # row ranges (a shard, a CLI batch): the same values as the whole-triangle launch
        host = out.cpu().numpy().view(np.uint32)
        for r0, r1 in ((0, 1), (5, 700), (N // 3, N // 3 + 1111), (N - 300, N)):
            np.testing.assert_array_equal(cs.eqcount_ut(r0, r1), host[off[r0]:off[r1]], err_msg=f"{name} rows {r0}:{r1}")
        fpart = torch.empty(int(off[N // 3 + 1111] - off[N // 3]), dtype=torch.float32, device=dev)
        cs.lut_ut_dev(lut.data_ptr(), fpart.data_ptr(), N // 3, N // 3 + 1111, stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(fpart.cpu().numpy().view(np.uint32), lut_np[host[off[N // 3]:off[N // 3 + 1111]]].view(np.uint32), err_msg=name)
        # and the ORACLE on 64+ rows (first rows, random rows, last rows)
        for i in sample:
            want = oracle.eqcounts_rows(m, int(i), int(i) + 1)
            np.testing.assert_array_equal(host[off[i]:off[i + 1]], want, err_msg=f"{name} row {i}")
        del t_dev
    cs.close()
    f = seen["families"]
    assert f["sorted_operand"]
    if variant != "short_list":                                        # (a list of pairs / 4096 entries may not even hold the families' stragglers)
        assert not f["dense_kernel_ran"] and f["tiles_and_pair_list"]
    if variant == "no_link":
        assert f["tiles_listed"] == 0 and f["pairs_listed"] > 100_000                           # every equal register pair of the matrix is a list entry
    elif variant != "short_list":
        assert f["tiles_listed"] > 0
    if variant in ("default", "table_link", "emit_big", "entry_by_entry", "binned"):
        # ten chance collisions per sketch used to list every tile; now the families keep their tiles and the strangers go to the list
        # (S = 96: one collision per sketch is 1 % of the registers, ten are 10 % -- heavy noise at this sketch size)
        assert 0 < seen["families+1"]["tiles_listed"] <= 2 * f["tiles_listed"] and seen["families+1"]["pairs_listed"] > 10_000
        assert not seen["families+1"]["dense_kernel_ran"]
        # no families: (nearly) every equal register pair is a list entry -- a few pairs land in one segment by chance and come from tiles
        assert seen["paired"]["tiles_and_pair_list"] and 0.99 * (N // 2 * S) <= seen["paired"]["pairs_listed"] <= N // 2 * S
        assert seen["chains"]["pairs_listed"] > 0 and not seen["chains"]["dense_kernel_ran"]
        assert seen["skewed"]["dense_kernel_ran"]                                                # one family takes everything
        assert seen["unrelated"]["tiles_listed"] == 0 and seen["unrelated"]["pairs_listed"] == 0 and not seen["unrelated"]["dense_kernel_ran"]
    if variant == "short_list":
        assert seen["paired"]["dense_kernel_ran"] and seen["paired"]["dense_decided_by_prepare"]  # the list overflowed: dense walk, same counts


def test_k2_fill_ahead_of_the_launch(gpu_ctx, d2g):
    """d2g_cmp_ut_prefill_dev: the fill of the next upper-triangle launch enqueued ahead of it -- before the operand is even prepared,
    on a second stream -- and the launch skips its own.  Same output as the plain launch: counts and table values, whole triangle and
    a row range; a launch that takes the dense walk after an early fill; an early fill with another value than the launch's (the launch
    fills again); a set too small to fill (no-op)."""
    import torch
    N, S = 9_000, 64
    dev = torch.device("cuda", 0)
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    st = main.cuda_stream
    fam = synth.synthetic_registers(N, S, nclusters=N // 150, seed=8)
    mats = [fam, synth.skewed_registers(N, S, seed=9)]                   # the second one: dense walk decided on the device
    lut_np = d2g.epilogue_lut(S, d2g.SIMILARITY, 31)
    lut = torch.from_numpy(lut_np).to(dev)
    npairs = N * (N - 1) // 2
    want = torch.empty(npairs, dtype=torch.int32, device=dev)
    got = torch.empty(npairs, dtype=torch.int32, device=dev)
    fgot = torch.empty(npairs, dtype=torch.float32, device=dev)
    cs = None
    for k, m in enumerate(mats):
        t_dev = torch.from_numpy(np.ascontiguousarray(m).view(np.int64)).to(dev)
        if cs is None:
            cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=st)
        else:
            cs.update_dev(t_dev.data_ptr(), st)
        cs.eqcount_ut_dev(want.data_ptr(), 0, N, st)                      # the plain launch
        info = cs.sparse_info(st)
        assert info["dense_kernel_ran"] == (k == 1), info
        torch.cuda.synchronize()
        # fill first (second stream), then prepare again, then the launch
        got.fill_(-1)
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        cs.prefill_ut_dev(got.data_ptr(), 0, N, stream=side.cuda_stream)
        ev.record(side)
        cs.update_dev(t_dev.data_ptr(), st)
        main.wait_event(ev)
        cs.eqcount_ut_dev(got.data_ptr(), 0, N, st)
        torch.cuda.synchronize()
        assert torch.equal(got, want), k
        # the table path, a row range, same stream
        r0, r1 = N // 4, N // 4 + 1500
        off = _ut_offsets(N)
        cnt = int(off[r1] - off[r0])
        fgot.fill_(-1.0)
        cs.prefill_ut_dev(fgot.data_ptr(), r0, r1, lut_dev_ptr=lut.data_ptr(), stream=st)
        cs.lut_ut_dev(lut.data_ptr(), fgot.data_ptr(), r0, r1, st)
        torch.cuda.synchronize()
        assert torch.equal(fgot[:cnt].view(torch.int32), lut[want[int(off[r0]):int(off[r1])].long()].view(torch.int32)), k
        # and the launch after it fills for itself again
        got.fill_(-1)
        cs.eqcount_ut_dev(got.data_ptr(), 0, N, st)
        torch.cuda.synchronize()
        assert torch.equal(got, want), k
        if k == 0:
            # an early fill with ANOTHER value (a table whose first entry is not the bits of the count 0), then a count launch into the
            # same output and rows: the launch fills for itself
            lut2 = torch.arange(S + 1, dtype=torch.float32, device=dev) + 0.5
            got.fill_(-1)
            cs.prefill_ut_dev(got.data_ptr(), 0, N, lut_dev_ptr=lut2.data_ptr(), stream=st)
            cs.update_dev(t_dev.data_ptr(), st)
            cs.eqcount_ut_dev(got.data_ptr(), 0, N, st)
            torch.cuda.synchronize()
            assert torch.equal(got, want)
        del t_dev
    cs.close()
    small = synth.synthetic_registers(300, S, nclusters=3, seed=1)
    cs = gpu_ctx.cmp_set(small, algo=d2g.CMP_BITSLICE)
    buf = torch.full((300 * 299 // 2,), -1, dtype=torch.int32, device=dev)
    cs.prefill_ut_dev(buf.data_ptr(), 0, 300, stream=st)                  # below 8192 sketches nothing is filled ...
    torch.cuda.synchronize()
    forced = int(os.environ.get("D2G_BS_SPARSE_MIN_N", "8192")) <= 300       # ... unless the suite runs with the sparse path forced on at every size
    assert int((buf != -1).sum()) == (buf.numel() if forced else 0)
    cs.close()


def test_k2_fill_carried_by_the_prepare(gpu_ctx, d2g, oracle):
    """d2g_cmp_ut_announce_dev: the output of the next upper-triangle launch announced ahead of update_dev -- the prepare's latency-bound
    kernels carry the fill as extra workgroups, the launch skips its own.  Same output as the plain launch (every word of a buffer
    pre-set to garbage): counts and table values, a whole triangle and a row range (unaligned output pointer), oracle rows; a matrix
    whose launch takes the dense walk; the remembered give-up (nothing rides, the launch writes everything); an announcement that the
    launch does not match (other rows / other output / other fill value) is simply not used; an announcement serves one prepare only; a
    cancelled announcement writes nothing; what riders wrote is void once another prepare has run."""
    import torch
    N, S = 9_000, 64
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    fam = synth.synthetic_registers(N, S, nclusters=N // 150, seed=18)
    noisy = synth.add_chance_collisions(fam, 1, seed=19)
    mats = [fam, noisy, synth.skewed_registers(N, S, seed=9)]           # the last one: dense walk decided on the device
    lut_np = d2g.epilogue_lut(S, d2g.SIMILARITY, 31)
    lut = torch.from_numpy(lut_np).to(dev)
    npairs = N * (N - 1) // 2
    want = torch.empty(npairs, dtype=torch.int32, device=dev)
    got = torch.empty(npairs + 3, dtype=torch.int32, device=dev)
    fgot = torch.empty(npairs + 3, dtype=torch.float32, device=dev)
    off = _ut_offsets(N)
    cs = None
    for k, m in enumerate(mats):
        bits = np.ascontiguousarray(m).view(np.uint64)
        t_dev = torch.from_numpy(bits.view(np.int64)).to(dev)
        if cs is None:
            cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=st)
        else:
            cs.update_dev(t_dev.data_ptr(), st)
        cs.eqcount_ut_dev(want.data_ptr(), 0, N, st)                      # the plain launch
        info = cs.sparse_info(st)
        assert info["dense_kernel_ran"] == (k == 2), info
        torch.cuda.synchronize()
        if k == 0:                                                        # pin the plain launch itself on oracle rows
            w = want.cpu().numpy().view(np.uint32)
            for r in (0, 1, 4_499, N - 2):
                np.testing.assert_array_equal(w[off[r]:off[r + 1]], oracle.eqcounts_rows(bits.view(np.float64), r, r + 1), err_msg=f"row {r}")
        for rep in range(3):                                              # (the third prepare of the skewed matrix has remembered the give-up)
            # counts, whole triangle, output pointer 4 bytes past a 16-byte boundary
            got.fill_(-1)
            o1 = got[1:1 + npairs]
            cs.announce_ut_dev(o1.data_ptr(), 0, N)
            cs.update_dev(t_dev.data_ptr(), st)
            cs.eqcount_ut_dev(o1.data_ptr(), 0, N, st)
            torch.cuda.synchronize()
            assert torch.equal(o1, want), (k, rep)
            assert int(got[0]) == -1 and int(got[1 + npairs]) == -1, (k, rep)
        # the table path, a row range
        r0, r1 = N // 4, N // 4 + 1500
        cnt = int(off[r1] - off[r0])
        fgot.fill_(-1.0)
        o2 = fgot[2:2 + cnt]
        cs.announce_ut_dev(o2.data_ptr(), r0, r1, lut_dev_ptr=lut.data_ptr())
        cs.update_dev(t_dev.data_ptr(), st)
        cs.lut_ut_dev(lut.data_ptr(), o2.data_ptr(), r0, r1, st)
        torch.cuda.synchronize()
        assert torch.equal(o2.view(torch.int32), lut[want[int(off[r0]):int(off[r1])].long()].view(torch.int32)), k
        assert float(fgot[1]) == -1.0 and float(fgot[2 + cnt]) == -1.0, k
        # announced rows that the launch does not take: the launch fills for itself, and the announced range was (harmlessly) filled
        got.fill_(-1)
        cs.announce_ut_dev(got.data_ptr(), 0, 10)
        cs.update_dev(t_dev.data_ptr(), st)
        cs.eqcount_ut_dev(got.data_ptr(), 0, N, st)
        torch.cuda.synchronize()
        assert torch.equal(got[:npairs], want), k
        # ... and the next prepare carries nothing: the launch after it still writes every output
        got.fill_(-1)
        cs.update_dev(t_dev.data_ptr(), st)
        cs.eqcount_ut_dev(got.data_ptr(), 0, N, st)
        torch.cuda.synchronize()
        assert torch.equal(got[:npairs], want), k
        if k == 0:
            buf = got[:npairs]
            # another fill value: the riders fill with the first entry of a table (not the bits of the count 0), then a COUNT launch
            # into the same output and rows -- it fills for itself
            lut2 = torch.arange(S + 1, dtype=torch.float32, device=dev) + 0.5
            got.fill_(-1)
            cs.announce_ut_dev(buf.data_ptr(), 0, N, lut_dev_ptr=lut2.data_ptr())
            cs.update_dev(t_dev.data_ptr(), st)
            cs.eqcount_ut_dev(buf.data_ptr(), 0, N, st)
            torch.cuda.synchronize()
            assert torch.equal(buf, want)
            # a cancelled announcement (all three pointers null): the next prepare writes nothing into the buffer
            got.fill_(-1)
            cs.announce_ut_dev(buf.data_ptr(), 0, N)
            gpu_ctx._check(d2g.lib().d2g_cmp_ut_announce_dev(gpu_ctx._h, cs._h, 0, N, None, None, None))
            cs.update_dev(t_dev.data_ptr(), st)
            torch.cuda.synchronize()
            assert bool((got == -1).all())
            # what the riders of one prepare wrote is void after another prepare: the buffer was used in between
            cs.announce_ut_dev(buf.data_ptr(), 0, N)
            cs.update_dev(t_dev.data_ptr(), st)
            got.fill_(-1)
            cs.update_dev(t_dev.data_ptr(), st)
            cs.eqcount_ut_dev(buf.data_ptr(), 0, N, st)
            torch.cuda.synchronize()
            assert torch.equal(buf, want)
        del t_dev
    cs.close()


def test_k2_sparse_path_beyond_65535_sketches(gpu_ctx, d2g, oracle):
    """70 000 sketches: the sizes where 16-bit fields end -- the pair-list kernel counts with two words per value from 65 536 sketches
    on, sorted positions, launch rows and segment ends no longer fit 16 bits, the rank kernel walks four hash partitions.  A family
    collection with one chance collision per sketch: whole triangle (2.4 * 10^9 pairs) and row ranges against the direct 64-bit
    kernel, 40 rows against the oracle; the sparse path must have been taken."""
    import torch
    N, S = 70_000, 64
    fam = synth.synthetic_registers(N, S, nclusters=N // 150, seed=65)
    m = synth.add_chance_collisions(fam, 1, seed=66).view(np.float64)
    bits = np.ascontiguousarray(m).view(np.uint64)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    t_dev = torch.from_numpy(bits.view(np.int64)).to(dev)
    npairs = N * (N - 1) // 2
    out = torch.empty(npairs, dtype=torch.int32, device=dev)
    ref = torch.empty(npairs, dtype=torch.int32, device=dev)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    out.fill_(-1)
    cs.eqcount_ut_dev(out.data_ptr(), 0, N, stream)
    info = cs.sparse_info(stream)
    dr = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_DIRECT, stream=stream)
    dr.eqcount_ut_dev(ref.data_ptr(), 0, N, stream)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert info["sorted_operand"] and info["tiles_and_pair_list"] and not info["dense_kernel_ran"], info
    assert info["tiles_listed"] > 0 and info["pairs_listed"] > N // 2, info
    off = _ut_offsets(N)
    for r0, r1 in ((0, 3), (65_530, 65_600), (N - 700, N)):
        a = cs.eqcount_ut(r0, r1)
        np.testing.assert_array_equal(a, dr.eqcount_ut(r0, r1), err_msg=f"rows {r0}:{r1}")
    rng = np.random.default_rng(5)
    host_rows = np.unique(np.concatenate([[0, 65_535, 65_536, N - 2], rng.integers(0, N - 1, 36)]))
    for i in host_rows:
        got = out[int(off[i]):int(off[i + 1])].cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got, oracle.eqcounts_rows(m, int(i), int(i) + 1), err_msg=f"row {i}")
    cs.close(); dr.close()


def test_k2_bench_matrix_rows_vs_oracle(gpu_ctx, d2g, oracle):
    """the EXACT matrix bench.py times (config 3: synthetic_registers(10000, 1024, nclusters=66, seed=20260928), finalised)
    on the sparse path (asserted), ~200 rows -- first rows, the seams of an 8-way pair-balanced partition, random rows, last rows --
    value for value against the oracle: equality counts and the fused float epilogue; then the same matrix with three and with ten chance
    collisions per sketch (bench.py's noise family; VERDICT r5 #1: at ten the list holds ~4 million entries and goes through the binned +
    composed form -- asserted -- where round 5 took the dense walk)."""
    import torch
    N, S = 10_000, 1024
    regs = synth.synthetic_registers(N, S, nclusters=66, seed=20260928)
    off = _ut_offsets(N)
    rng = np.random.default_rng(5)
    seams = [int(x) for x in d2g.ut_partition(N, 8)]
    rows = sorted(set(list(range(0, 24)) + [min(N - 2, max(0, b + d)) for b in seams for d in (-2, -1, 0, 1)] + [int(x) for x in rng.integers(0, N - 1, 120)] + list(range(N - 25, N - 1))))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    for label, rr in (("stated", regs), ("stated + 3 collisions", synth.add_chance_collisions(regs, 3, seed=20260929)),
                      ("stated + 10 collisions", synth.add_chance_collisions(regs, 10, seed=20260929))):
        sig, cards = d2g.oph_finalize(rr, S, nthreads=8)
        t_dev = torch.from_numpy(sig.view(np.int64)).to(dev)
        cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_AUTO, stream=stream)
        out = torch.empty(N * (N - 1) // 2, dtype=torch.int32, device=dev)
        cs.eqcount_ut_dev(out.data_ptr(), 0, N, stream)
        info = cs.sparse_info(stream)
        assert info["sorted_operand"] and info["tiles_listed"] > 0 and info["tiles_and_pair_list"] and not info["dense_kernel_ran"], (label, info)
        if label != "stated":
            assert info["pairs_listed"] > 0
        if label.endswith("10 collisions"):
            assert info["pairs_listed"] > 786_432, info                 # (D2G_SP_LONG_LIST: the binned + composed form from here on)
        fout = torch.empty(N * (N - 1) // 2, dtype=torch.float32, device=dev)
        lut = torch.from_numpy(d2g.epilogue_lut(S, d2g.SIMILARITY, 31)).to(dev)
        cs.lut_ut_dev(lut.data_ptr(), fout.data_ptr(), 0, N, stream)
        torch.cuda.synchronize()
        host, fhost = out.cpu().numpy().view(np.uint32), fout.cpu().numpy()
        for i in rows:
            want = oracle.eqcounts_rows(sig, i, i + 1)
            np.testing.assert_array_equal(host[off[i]:off[i + 1]], want, err_msg=f"{label} row {i}")
            fwant = oracle.allpairs_ut(sig, cards, measure=oracle.SIMILARITY, k=31, rows=(i, i + 1), nthreads=4)
            np.testing.assert_array_equal(fhost[off[i]:off[i + 1]].view(np.uint32), fwant.view(np.uint32), err_msg=f"{label} row {i}")
        cs.close()
        del t_dev, out, fout


def test_k2_sparse_give_up_is_remembered_per_set(gpu_ctx, d2g, oracle, monkeypatch):
    """where the sparse path does not pay, the ordering that finds it out is not paid again by the next prepares of the same
    set (CLI batches, a re-loaded matrix): the kernels that decide for the dense walk leave a word in host-visible memory, the next prepare
    skips the ordering (retried every 16th prepare).  Results are those of the oracle either way; a family matrix loaded afterwards is
    walked densely until the retry -- correct, only slower."""
    import torch
    monkeypatch.setenv("D2G_SP_PREDICT", "0")                          # (the first look at the matrix would decide before the ordering: test_k2_first_look_decides_before_the_ordering)
    monkeypatch.setenv("D2G_SP_LIST_DIV", "256")                       # a list of pairs / 256 entries: the adversarial matrix's N S / 2 = 288 000 do not fit, the families' few do
    N, S = 9000, 64
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    paired = synth.paired_registers(N, S, seed=8)
    fam = synth.synthetic_registers(N, S, nclusters=60, seed=9)
    off = _ut_offsets(N)
    out = torch.empty(N * (N - 1) // 2, dtype=torch.int32, device=dev)
    t_dev = torch.from_numpy(paired.view(np.int64)).to(dev)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    seen = []
    for step, m in enumerate([paired, paired, fam] + [fam] * 16):
        t_dev.copy_(torch.from_numpy(m.view(np.int64)))
        if step:
            cs.update_dev(t_dev.data_ptr(), stream)
        cs.eqcount_ut_dev(out.data_ptr(), 0, N, stream)
        info = cs.sparse_info(stream)                                  # (synchronises: the word is written by now)
        seen.append(info)
        if step in (0, 1, 2, 18):
            host = out.cpu().numpy().view(np.uint32)
            for i in (0, 17, N // 2, N - 2):
                np.testing.assert_array_equal(host[off[i]:off[i + 1]], oracle.eqcounts_rows(m.view(np.float64), i, i + 1), err_msg=f"step {step} row {i}")
    cs.close()
    assert seen[0]["dense_kernel_ran"] and not seen[0]["ordering_skipped"]      # the list does not fit: dense walk, found out by the ordering
    assert seen[1]["ordering_skipped"] and seen[1]["dense_kernel_ran"]
    assert seen[2]["ordering_skipped"] and seen[2]["dense_kernel_ran"]          # another matrix, same set: still remembered
    assert any(not x["ordering_skipped"] and x["tiles_listed"] > 0 and not x["dense_kernel_ran"] for x in seen[3:])   # the 16th prepare tried again and found the families


def test_k2_first_look_decides_before_the_ordering(gpu_ctx, d2g, oracle):
    """VERDICT r5 #1b: a set's FIRST prepare looks at its matrix before it orders it -- sixteen sampled sketches against all, on the rank kernel's ids:
    list entries and family pairs the ordering would find, scaled, into a cost model -- and a matrix the sparse path cannot help (a random pairing
    per column, one family, a hundred chance collisions per sketch) goes to the dense walk without link / sort / emit (ordering_skipped on the very
    first launch); a family collection, clean or with a few chance collisions, keeps its tiles and its list.  Whatever is decided, the counts are the
    oracle's; d2g_cmp_set_forget makes the next prepare look again."""
    import torch
    N, S = 10_000, 1024                                                 # (config 3's shape: the cost model's constants were measured there)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    fam = synth.synthetic_registers(N, S, nclusters=N // 150, seed=31)
    cases = [("families", fam, False), ("families+1", synth.add_chance_collisions(fam, 1, seed=32), False),
             ("families+10", synth.add_chance_collisions(fam, 10, seed=36), False),
             ("families+100", synth.add_chance_collisions(fam, 100, seed=33), True), ("paired", synth.paired_registers(N, S, seed=34), True),
             ("skewed", synth.skewed_registers(N, S, seed=35), True),
             ("unrelated", synth.unrelated_registers(N, S, seed=37), False)]     # (nothing shared: the fill alone -- the dense walk would cost a whole pair kernel)
    off = _ut_offsets(N)
    out = torch.empty(N * (N - 1) // 2, dtype=torch.int32, device=dev)
    rows = [0, 1, 77, N // 2, N - 3, N - 2]
    for name, m, want_dense in cases:
        bits = np.ascontiguousarray(m).view(np.uint64)
        t_dev = torch.from_numpy(bits.view(np.int64)).to(dev)
        cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)     # the set's first prepare
        out.fill_(-1)
        cs.eqcount_ut_dev(out.data_ptr(), 0, N, stream)
        info = cs.sparse_info(stream)
        assert info["dense_kernel_ran"] == want_dense and info["ordering_skipped"] == want_dense, (name, info)
        host = out.cpu().numpy().view(np.uint32)
        for i in rows:
            np.testing.assert_array_equal(host[off[i]:off[i + 1]], oracle.eqcounts_rows(bits.view(np.float64), i, i + 1), err_msg=f"{name} row {i}")
        # later prepares go by what is remembered; after forget() the next one looks again (and decides the same)
        cs.update_dev(t_dev.data_ptr(), stream)
        cs.forget()
        cs.update_dev(t_dev.data_ptr(), stream)
        out.fill_(-1)
        cs.eqcount_ut_dev(out.data_ptr(), 0, N, stream)
        info2 = cs.sparse_info(stream)
        assert info2["dense_kernel_ran"] == want_dense, (name, info2)
        host = out.cpu().numpy().view(np.uint32)
        for i in rows[:3]:
            np.testing.assert_array_equal(host[off[i]:off[i + 1]], oracle.eqcounts_rows(bits.view(np.float64), i, i + 1), err_msg=f"{name} (again) row {i}")
        cs.close()
        del t_dev


def test_k2_timed_sequence_at_config3_vs_oracle(gpu_ctx, d2g, oracle):
    """exactly the sequence bench.py times -- announce_ut_dev -> update_dev -> lut_ut_dev on synthetic_registers(10000, 1024, 66, 20260928),
    finalised -- three prepares in a row into a buffer pre-set to garbage, ~200 rows (first rows, the seams of an 8-way partition, random rows, last
    rows) of the float output bit for bit against the oracle after every one."""
    import torch
    N, S = 10_000, 1024
    regs = synth.synthetic_registers(N, S, nclusters=66, seed=20260928)
    sig, cards = d2g.oph_finalize(regs, S, nthreads=8)
    off = _ut_offsets(N)
    rng = np.random.default_rng(6)
    seams = [int(x) for x in d2g.ut_partition(N, 8)]
    rows = sorted(set(list(range(0, 24)) + [min(N - 2, max(0, b + d)) for b in seams for d in (-2, -1, 0, 1)] + [int(x) for x in rng.integers(0, N - 1, 120)] + list(range(N - 25, N - 1))))
    want = {i: oracle.allpairs_ut(sig, cards, measure=oracle.SIMILARITY, k=31, rows=(i, i + 1), nthreads=4).view(np.uint32) for i in rows}
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    t_dev = torch.from_numpy(sig.view(np.int64)).to(dev)
    lut = torch.from_numpy(d2g.epilogue_lut(S, d2g.SIMILARITY, 31)).to(dev)
    fout = torch.empty(N * (N - 1) // 2, dtype=torch.float32, device=dev)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_AUTO, stream=stream)
    for rep in range(3):
        fout.view(torch.int32).fill_(0x7FC12345)                          # garbage (a NaN pattern no table holds)
        cs.announce_ut_dev(fout.data_ptr(), 0, N, lut_dev_ptr=lut.data_ptr())
        cs.update_dev(t_dev.data_ptr(), stream)
        cs.lut_ut_dev(lut.data_ptr(), fout.data_ptr(), 0, N, stream)
        info = cs.sparse_info(stream)
        assert info["sorted_operand"] and info["tiles_listed"] > 0 and not info["dense_kernel_ran"], (rep, info)
        host = fout.cpu().numpy().view(np.uint32)
        assert not (host == 0x7FC12345).any(), rep                        # every output word was written
        for i in rows:
            np.testing.assert_array_equal(host[off[i]:off[i + 1]], want[i], err_msg=f"prepare {rep} row {i}")
    cs.close()


def test_bench_plain_run_dumps_the_timed_steps_output(d2g, oracle, tmp_path):
    """a plain `bench.py --gpus 1` run prints the headline line without any --full part, and --dump-outputs writes what its last timed step
    computed: at N = 3000 (below DUMP_VALUES pairs) the whole float32 triangle, bit for bit the oracle's all-pairs of the same seeded matrix"""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    N, S = 3000, 1024
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--sketches", str(N), "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 3 and line["config"]["pairs"] == N * (N - 1) // 2
    assert all(line[k] is None for k in ("cpu_baseline", "checked_vs_oracle", "config4_1gpu", "sketch", "multiset_sketch"))
    assert "matrices" not in line["compute"] and line["roofline"]["traffic"] is None
    got = np.load(tmp_path / "jaccard_ut_sample.npy")
    regs = synth.synthetic_registers(N, S, nclusters=max(8, N // 150), seed=20260928)
    sig, cards = d2g.oph_finalize(regs, S, nthreads=8)
    want = oracle.allpairs_ut(sig, cards, measure=oracle.SIMILARITY, k=31, nthreads=4)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
