"""The merged schedule of the bit-sliced prepare (d2g_bitslice_prepare + sp_prepare_order): behind the rank kernel the column plan runs as block 0
of the launch that holds link pass 0 (sp_link0_plan_kernel), the planes workgroups share a launch with flatten (bs_planes_flatten_kernel), and the
ordering's start-of-prepare initialisation is carried by the transpose in front of the prepare.

Every prepare is checked the same way: equality counts of the whole triangle against a CMP_DIRECT set, sixteen or more rows (the first and the
last among them) against the oracle, and `sparse_detail` says which schedule ran and how many kernels the prepare enqueued -- a silent fallback
to the classic chain shows as a wrong schedule or count, not as a pass.

Kernel counts (D2G_SP_LIST_FORM=1: the pair list entry by entry, nothing enqueued for its bins):
    classic   transpose, rank, plan, planes, link 0, flatten, link 1, count, attach, scan, place, emit, permute             13
    merged    transpose, rank, [plan + link 0], [flatten + planes], link 1, count, attach, scan, place, emit, permute       11
    one column (no link pass, no flatten, no attach): transpose, rank, [plan], [planes], count, scan, place, emit, permute  9
    a first look adds its two kernels; a prepare that gives up on the host runs transpose, rank, (look,) plan, planes, give-up."""
import numpy as np
import pytest

from dashing2_amd import synth

pytestmark = pytest.mark.gpu

CLASSIC, MERGED, ONE_COLUMN = 13, 11, 9


def _ut_offsets(N):
    return np.concatenate([[0], np.cumsum(N - 1 - np.arange(N, dtype=np.int64))])


def _rows(N):
    """sixteen rows or more: the first and the last that have pairs, and the seams of the 32-row bands and 256-column tiles"""
    want = [0, 1, 31, 32, 33, 255, 256, 257, N // 2, N // 2 + 1, N - 258, N - 257, N - 34, N - 33, N - 3, N - 2]
    rows = sorted({min(max(r, 0), N - 2) for r in want})
    extra = iter(range(2, N - 2))
    while len(rows) < 16:
        rows = sorted(set(rows) | {next(extra)})
    return rows


def _not_degenerate(regs, nclusters, collided):
    """the input really has what the ordering is about: a family of two or more members, and -- with collisions -- a pair of different families that shares a register"""
    N, S = regs.shape
    cl = np.arange(N) % nclusters
    fam = cross = False
    for j in range(min(N, 4 * nclusters)):                               # (a few sketches against all: enough to see both)
        c = (regs == regs[j]).sum(1)
        c[j] = 0
        fam |= bool((c[cl == cl[j]] >= min(S, 4)).any())
        cross |= bool((c[cl != cl[j]] >= 1).any())
    assert fam, "no family of two or more members"
    assert cross or not collided, "no cross-family entry"


def _to_dev(torch, regs):
    bits = np.ascontiguousarray(regs).view(np.uint64)
    return bits, torch.from_numpy(bits.view(np.int64)).to(torch.device("cuda", 0))


def _reference(torch, gpu_ctx, d2g, oracle, bits, t_dev, label, stream):
    """whole-triangle counts of a CMP_DIRECT set, pinned on the oracle's rows; computed once per matrix and shared"""
    N, S = bits.shape
    ref = torch.empty(N * (N - 1) // 2, dtype=torch.int32, device=t_dev.device)
    dr = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_DIRECT, stream=stream)
    dr.eqcount_ut_dev(ref.data_ptr(), 0, N, stream)
    torch.cuda.synchronize()
    dr.close()
    off = _ut_offsets(N)
    m = bits.view(np.float64)
    for i in _rows(N):
        np.testing.assert_array_equal(ref[int(off[i]):int(off[i + 1])].cpu().numpy().view(np.uint32), oracle.eqcounts_rows(m, int(i), int(i) + 1),
                                      err_msg=f"{label}: direct kernel, row {i}")
    return ref


def _check_counts(torch, cs, ref, N, label, stream):
    """the prepared set's whole triangle into a buffer of garbage == the reference; -> (sparse_info, sparse_detail)"""
    out = torch.full((N * (N - 1) // 2,), -7, dtype=torch.int32, device=ref.device)
    cs.eqcount_ut_dev(out.data_ptr(), 0, N, stream)
    info, detail = cs.sparse_info(stream), cs.sparse_detail(stream)
    torch.cuda.synchronize()
    print(label, info, {k: detail[k] for k in ("looked", "looked_dense", "schedule", "prepare_kernels")})
    bad = torch.nonzero(out != ref)
    assert bad.numel() == 0, (label, "first differing pair index", int(bad[0]), "of", int(bad.numel()))
    return info, detail


def _force_small(monkeypatch):
    monkeypatch.setenv("D2G_BS_SPARSE_MIN_N", "1")
    monkeypatch.setenv("D2G_SP_TILE_FRAC", "1")                         # (matrices this small have few tiles: the families' share of them is large)
    monkeypatch.setenv("D2G_SP_PREDICT", "0")                           # (no first look: the set's first prepare already knows its path)
    monkeypatch.setenv("D2G_SP_LIST_FORM", "1")
    monkeypatch.setenv("D2G_SP_LIST_DIV", "1")                          # (a few columns and large families: the list may hold an entry per pair)
    monkeypatch.setenv("D2G_SP_REMEMBER", "0")                          # (where the ordering still gives up, the next prepare runs it again: no remembered skip)
    monkeypatch.setenv("D2G_K2_MERGE", "1")                             # (whatever the suite runs with)


# N, S, families -- what each shape is for:
SHAPES = [
    (1300, 70, 8),      # two x-blocks in the link grid, Spad = 96: padding columns (BS_NOCOL) in the plan, a partly filled last group
    (300, 2, 3),        # one column pair
    (300, 1, 3),        # no link pass: the link launch is the column plan alone, the planes launch has no flatten
    (260, 4100, 3),     # Spad > BS_PLAN_MAXS: the plan's identity branch in a 256-thread block
    (2100, 64, 14),     # several position blocks in the planes grid (9 x 2 workgroups behind flatten's 9)
]


@pytest.mark.parametrize("collisions", [0, 1])
@pytest.mark.parametrize("N,S,nfam", SHAPES)
def test_k2_merged_prepare_smallest_shapes(gpu_ctx, d2g, oracle, monkeypatch, N, S, nfam, collisions):
    """the smallest shapes at which the merged launches can still go wrong, family matrices with and without a chance collision per sketch"""
    import torch
    _force_small(monkeypatch)
    stream = torch.cuda.current_stream().cuda_stream
    regs = synth.synthetic_registers(N, S, nclusters=nfam, seed=100 * S + N)
    if collisions:
        regs = synth.add_chance_collisions(regs, 1, seed=N + S)
    _not_degenerate(regs, nfam, bool(collisions))
    label = f"N={N} S={S} collisions={collisions}"
    bits, t_dev = _to_dev(torch, regs)
    ref = _reference(torch, gpu_ctx, d2g, oracle, bits, t_dev, label, stream)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    try:
        for rep in range(2):                                            # (creation, then an update: the transpose initialises behind a launch too)
            if rep:
                cs.update_dev(t_dev.data_ptr(), stream)
            info, detail = _check_counts(torch, cs, ref, N, f"{label} prepare {rep + 1}", stream)
            assert info["sorted_operand"], info
            assert detail["schedule"] == "merged", detail
            assert detail["prepare_kernels"] == (ONE_COLUMN if S == 1 else MERGED), detail
    finally:
        cs.close()


def test_k2_merged_prepare_initialisation_rides_on_the_transpose(gpu_ctx, d2g, oracle, monkeypatch):
    """One set, four prepares through update_dev, each launched into garbage: a family matrix (the set's first prepare takes the first look: classic),
    an unrelated one, the families with collisions, the families again (merged, all three).  Labels, hints, counters, bitmap or list cursor left over
    from the prepare before would show in the counts: the transpose in front of every prepare resets them."""
    import torch
    monkeypatch.setenv("D2G_SP_LIST_FORM", "1")
    monkeypatch.setenv("D2G_K2_MERGE", "1")
    N, S, nfam = 9_000, 64, 60                                          # (the sparse path's own size: the first look decides for it, as in production)
    stream = torch.cuda.current_stream().cuda_stream
    fam = synth.synthetic_registers(N, S, nclusters=nfam, seed=18)
    noisy = synth.add_chance_collisions(fam, 1, seed=19)
    _not_degenerate(fam, nfam, False)
    _not_degenerate(noisy, nfam, True)
    mats = {"families": fam, "unrelated": synth.unrelated_registers(N, S, seed=5), "families+1": noisy}
    refs, devs = {}, {}
    for name, regs in mats.items():
        bits, devs[name] = _to_dev(torch, regs)
        refs[name] = _reference(torch, gpu_ctx, d2g, oracle, bits, devs[name], name, stream)
    cs = None
    try:
        for k, name in enumerate(["families", "unrelated", "families+1", "families"]):
            if cs is None:
                cs = gpu_ctx.cmp_set_dev(devs[name].data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
            else:
                cs.update_dev(devs[name].data_ptr(), stream)
            info, detail = _check_counts(torch, cs, refs[name], N, f"prepare {k + 1} ({name})", stream)
            assert not info["dense_kernel_ran"] and info["tiles_and_pair_list"], info
            if k == 0:
                assert detail["looked"] and not detail["looked_dense"], detail
                assert (detail["schedule"], detail["prepare_kernels"]) == ("classic", CLASSIC + 2), detail
            else:
                assert not detail["looked"], detail
                assert (detail["schedule"], detail["prepare_kernels"]) == ("merged", MERGED), detail
    finally:
        if cs is not None:
            cs.close()


@pytest.mark.parametrize("ride", ["0", "1", "2", "3", "63"])
def test_k2_merged_prepare_carries_the_announced_fill(gpu_ctx, d2g, oracle, monkeypatch, ride):
    """announce -> update -> launch (the benchmark's step) with the table epilogue and lut[0] != 0: bit 1 of D2G_SP_RIDE is the launch that contains
    the column plan, bit 2 the one that contains flatten.  The whole triangle and a row range (output 4 bytes past a 16-byte boundary), into garbage."""
    import torch
    _force_small(monkeypatch)
    monkeypatch.setenv("D2G_SP_RIDE", ride)
    N, S, nfam = 1300, 70, 8
    stream = torch.cuda.current_stream().cuda_stream
    regs = synth.add_chance_collisions(synth.synthetic_registers(N, S, nclusters=nfam, seed=100 * S + N), 1, seed=N + S)
    _not_degenerate(regs, nfam, True)
    bits, t_dev = _to_dev(torch, regs)
    ref = _reference(torch, gpu_ctx, d2g, oracle, bits, t_dev, f"ride {ride}", stream)
    lut_np = d2g.epilogue_lut(S, d2g.POISSON_LLR, 31, multiset_space=True)
    assert lut_np.view(np.uint32)[0] != 0                               # (the filled word is not zero)
    lut = torch.from_numpy(lut_np).to(t_dev.device)
    off = _ut_offsets(N)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    try:
        for r0, r1 in ((0, N), (N // 4 + 3, N // 4 + 500)):
            cnt = int(off[r1] - off[r0])
            buf = torch.full((cnt + 2,), -3.0, dtype=torch.float32, device=t_dev.device)
            out = buf[1:1 + cnt]
            cs.announce_ut_dev(out.data_ptr(), r0, r1, lut_dev_ptr=lut.data_ptr())
            cs.update_dev(t_dev.data_ptr(), stream)
            cs.lut_ut_dev(lut.data_ptr(), out.data_ptr(), r0, r1, stream)
            detail = cs.sparse_detail(stream)
            torch.cuda.synchronize()
            want = lut[ref[int(off[r0]):int(off[r0]) + cnt].long()]
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (ride, r0, r1)
            assert float(buf[0]) == -3.0 and float(buf[1 + cnt]) == -3.0, (ride, r0, r1)
            assert (detail["schedule"], detail["prepare_kernels"]) == ("merged", MERGED), detail
    finally:
        cs.close()


@pytest.mark.parametrize("switch,value,N,S,nfam", [("D2G_SP_OLINK", "0", 1300, 70, 8), ("D2G_K2_MERGE", "0", 1300, 70, 8), ("D2G_BS_NSPLIT", "2", 23_000, 64, 150)])
def test_k2_merged_prepare_falls_back_to_the_classic_chain(gpu_ctx, d2g, oracle, monkeypatch, switch, value, N, S, nfam):
    """the table form of the link passes, the switch, and rank passes split over two workgroups per column keep the chain kernel by kernel"""
    import torch
    _force_small(monkeypatch)
    monkeypatch.setenv(switch, value)
    stream = torch.cuda.current_stream().cuda_stream
    regs = synth.synthetic_registers(N, S, nclusters=nfam, seed=100 * S + N)
    _not_degenerate(regs, nfam, False)
    bits, t_dev = _to_dev(torch, regs)
    ref = _reference(torch, gpu_ctx, d2g, oracle, bits, t_dev, switch, stream)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    try:
        for rep in range(2):
            if rep:
                cs.update_dev(t_dev.data_ptr(), stream)
            info, detail = _check_counts(torch, cs, ref, N, f"{switch}={value} prepare {rep + 1}", stream)
            assert info["sorted_operand"], info
            assert (detail["schedule"], detail["prepare_kernels"]) == ("classic", CLASSIC), detail
    finally:
        cs.close()


def test_k2_merged_prepare_keeps_a_remembered_give_up_classic(gpu_ctx, d2g, oracle, monkeypatch):
    """a matrix the first look sends to the dense walk, prepared twice: the second prepare remembers, runs no ordering and no merged launch"""
    import torch
    monkeypatch.setenv("D2G_SP_LIST_FORM", "1")
    monkeypatch.setenv("D2G_K2_MERGE", "1")
    N, S = 9_000, 64
    stream = torch.cuda.current_stream().cuda_stream
    regs = synth.skewed_registers(N, S, seed=9)
    bits, t_dev = _to_dev(torch, regs)
    ref = _reference(torch, gpu_ctx, d2g, oracle, bits, t_dev, "skewed", stream)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    try:
        info, detail = _check_counts(torch, cs, ref, N, "skewed prepare 1", stream)
        assert detail["looked"] and info["dense_kernel_ran"], (info, detail)
        # the look decides for the dense walk: transpose, rank, the look's two, plan, planes, give-up; it does not: the whole chain, and the ordering gives up on the device
        assert (detail["schedule"], detail["prepare_kernels"]) == ("classic", 7 if detail["looked_dense"] else CLASSIC + 2), detail
        cs.update_dev(t_dev.data_ptr(), stream)
        info, detail = _check_counts(torch, cs, ref, N, "skewed prepare 2", stream)
        assert info["ordering_skipped"] and info["dense_kernel_ran"] and not detail["looked"], (info, detail)
        assert (detail["schedule"], detail["prepare_kernels"]) == ("classic", 5), detail       # transpose, rank, plan, planes, give-up
    finally:
        cs.close()
