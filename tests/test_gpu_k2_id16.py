"""16-bit column ids in the bit-sliced prepare (D2G_BS_ID16, d2g_cmp_set::id_bits): a set whose rank kernel is single-partition (N <= 21 845) keeps
its per-column ids as 16-bit words -- 0 = padding, 0x8000 = unique, 1 .. 0x7FFF = rank -- and every kernel that touches them (the two single-partition
rank kernels, both link forms, the planes body, emit, the first look's sample) is instantiated for that word.  The counts do not depend on the width
of an intermediate word.

Every case is checked the same way: the equality counts of the prepared set (the whole triangle, or three bands of 64 rows from N = 4000 on) against a
CMP_DIRECT set, a handful of rows of that against the oracle, the same matrix prepared with D2G_BS_ID16=1 and =0 compared bit for bit, `id_bits` says
which word the set holds, and `sparse_info` / `sparse_detail` say that the ordering, the schedule and the tile + list launch really ran -- a silent
fall-back to the dense walk or to the classic chain does not pass as success."""
import numpy as np
import pytest

from dashing2_amd import synth

pytestmark = pytest.mark.gpu

NCLUSTERS_511 = 51                # families of the N = 511 seam (ten sketches each)
CLASSIC, MERGED = 13, 11          # kernels a prepare enqueues (D2G_SP_LIST_FORM=1), as in test_gpu_k2_prepare_merge.py


def _ut_offsets(N):
    return np.concatenate([[0], np.cumsum(N - 1 - np.arange(N, dtype=np.int64))])


def _bands(N):
    """the whole triangle below 4000 sketches; the first 64 rows, a middle band and the last 64 from there on"""
    if N < 4000:
        return [(0, N)]
    return [(0, 64), (N // 2 - 32, N // 2 + 32), (N - 64, N)]


def _to_dev(torch, regs):
    bits = np.ascontiguousarray(regs).view(np.uint64)
    return bits, torch.from_numpy(bits.view(np.int64)).to(torch.device("cuda", 0))


def _launch_bands(torch, cs, N, stream, device):
    off = _ut_offsets(N)
    outs = []
    for r0, r1 in _bands(N):
        out = torch.full((int(off[r1] - off[r0]),), -7, dtype=torch.int32, device=device)    # (launched into garbage)
        cs.eqcount_ut_dev(out.data_ptr(), r0, r1, stream)
        outs.append(out)
    torch.cuda.synchronize()
    return outs


def _reference(torch, gpu_ctx, d2g, oracle, bits, t_dev, label, stream):
    """the bands' counts of a CMP_DIRECT set, pinned on the oracle's rows (first, second, a middle one, the last two with pairs); once per matrix"""
    N, S = bits.shape
    dr = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_DIRECT, stream=stream)
    assert dr.id_bits == 0                                                # (a DIRECT set keeps no ids)
    refs = _launch_bands(torch, dr, N, stream, t_dev.device)
    dr.close()
    off = _ut_offsets(N)
    m = bits.view(np.float64)
    for (r0, r1), ref in zip(_bands(N), refs):
        for i in sorted({r0, r0 + 1, (r0 + r1) // 2, min(r1, N - 1) - 2, min(r1, N - 1) - 1}):
            a, b = int(off[i] - off[r0]), int(off[i + 1] - off[r0])
            np.testing.assert_array_equal(ref[a:b].cpu().numpy().view(np.uint32), oracle.eqcounts_rows(m, int(i), int(i) + 1), err_msg=f"{label}: direct kernel, row {i}")
    return refs


def _prepare_and_check(torch, gpu_ctx, d2g, t_dev, N, S, refs, label, stream, want_bits, update=False):
    """one BITSLICE set over the matrix: its bands against the reference; -> (outputs, sparse_info, sparse_detail, planes)"""
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    try:
        assert cs.id_bits == want_bits, (label, cs.id_bits, want_bits)
        if update:
            cs.update_dev(t_dev.data_ptr(), stream)
        outs = _launch_bands(torch, cs, N, stream, t_dev.device)
        info, detail, planes = cs.sparse_info(stream), cs.sparse_detail(stream), cs.planes(stream)
        cs.status(stream)
        print(label, f"id_bits={cs.id_bits}", info, {k: detail[k] for k in ("looked", "looked_dense", "schedule", "prepare_kernels")}, planes)
        for (r0, r1), out, ref in zip(_bands(N), outs, refs):
            bad = torch.nonzero(out != ref)
            assert bad.numel() == 0, (label, "rows", r0, r1, "first differing pair index", int(bad[0]), "of", int(bad.numel()))
        return outs, info, detail, planes
    finally:
        cs.close()


def _both_widths(torch, gpu_ctx, d2g, oracle, monkeypatch, regs, label, narrow_bits=16, update=False):
    """the matrix prepared with D2G_BS_ID16=1 and =0: each against the reference, the two bit for bit, the same plane counts; -> the narrow run's (info, detail, planes)"""
    N, S = regs.shape
    stream = torch.cuda.current_stream().cuda_stream
    bits, t_dev = _to_dev(torch, regs)
    refs = _reference(torch, gpu_ctx, d2g, oracle, bits, t_dev, label, stream)
    monkeypatch.setenv("D2G_BS_ID16", "1")
    o16, info16, detail16, planes16 = _prepare_and_check(torch, gpu_ctx, d2g, t_dev, N, S, refs, f"{label} ID16=1", stream, narrow_bits, update)
    monkeypatch.setenv("D2G_BS_ID16", "0")
    o32, info32, detail32, planes32 = _prepare_and_check(torch, gpu_ctx, d2g, t_dev, N, S, refs, f"{label} ID16=0", stream, 32, update)
    for a, b in zip(o16, o32):
        assert torch.equal(a, b), label
    assert planes16 == planes32, (label, planes16, planes32)
    assert (detail16["schedule"], detail16["prepare_kernels"]) == (detail32["schedule"], detail32["prepare_kernels"]), (detail16, detail32)
    for k in ("sorted_operand", "dense_decided_by_prepare", "ordering_skipped"):      # (what a LAUNCH decides goes by the families found: racing stores, run to run)
        assert info16[k] == info32[k], (label, k, info16, info32)
    return info16, detail16, planes16


def _sparse_env(monkeypatch, small):
    monkeypatch.setenv("D2G_SP_PREDICT", "0")                           # (no first look: the set's first prepare already knows its path)
    monkeypatch.setenv("D2G_SP_LIST_FORM", "1")
    monkeypatch.setenv("D2G_SP_REMEMBER", "0")
    monkeypatch.setenv("D2G_K2_MERGE", "1")                             # (whatever the suite runs with)
    monkeypatch.setenv("D2G_SP_OLINK", "1")
    if small:
        monkeypatch.setenv("D2G_BS_SPARSE_MIN_N", "1")
        monkeypatch.setenv("D2G_SP_TILE_FRAC", "1")                     # (matrices this small have few tiles: the families' share of them is large)
        monkeypatch.setenv("D2G_SP_LIST_DIV", "1")                      # (the list may hold an entry per pair)


def _families(N, S, collisions, seed, nclusters=None, share_lo=0.0):
    regs = synth.synthetic_registers(N, S, nclusters=nclusters or max(3, N // 150), seed=seed, share_lo=share_lo)
    return synth.add_chance_collisions(regs, 1, seed=seed + 1) if collisions else regs


def _assert_sparse_ran(info, detail, N, merged=True, launch=None):
    """the PREPARE ordered the sketches and kept its order (no give-up, no skip) in the expected schedule; a whole-triangle launch then used tiles + list.
    (A LAUNCH decides for itself whether its listed tiles pay -- more than 40 % of its candidates: the dense kernel over the sorted operand.  A band of 64
    rows may say so -- `info` is the last band's launch -- and `launch=False` names the whole-triangle cases that must: there the prepare's flags are asserted.)"""
    assert info["sorted_operand"] and not info["dense_decided_by_prepare"] and not info["callers_order_kept"] and not info["ordering_skipped"], info
    if _bands(N) == [(0, N)] if launch is None else launch:
        assert info["tiles_and_pair_list"] and not info["dense_kernel_ran"], info
    assert (detail["schedule"], detail["prepare_kernels"]) == (("merged", MERGED) if merged else ("classic", CLASSIC)), detail


# ---- kernel and width seams
@pytest.mark.parametrize("N,S,bits,multi", [
    (257, 64, 16, False),        # one sketch into the second position block: 255 padding ids per column
    (511, 64, 16, False),        # an odd N: the last pair of ids straddles N
    (12288, 32, 16, False),      # the last set of the FAST rank kernel
    (12289, 32, 16, False),      # the first set of the general single-partition kernel
    (21845, 32, 16, False),      # the last 16-bit set
    (21846, 32, 32, True),       # the first MULTI set: 32-bit ids, whatever the switch says
])
def test_k2_id16_kernel_and_width_seams(gpu_ctx, d2g, oracle, monkeypatch, N, S, bits, multi):
    import torch
    _sparse_env(monkeypatch, small=N < 8192)
    regs = _families(N, S, collisions=True, seed=7 * N + S, nclusters=NCLUSTERS_511 if N == 511 else None)
    info, detail, _ = _both_widths(torch, gpu_ctx, d2g, oracle, monkeypatch, regs, f"seam N={N} S={S}", narrow_bits=bits)
    # (the first MULTI set of 32 columns splits its rank passes over two workgroups per column to fill the chip: the classic chain)
    # (N = 511: 512 positions are 24 candidate tiles, and families on adjacent positions list the 16 on the diagonal at least -- the launch walks them all;
    # what the prepare built from the narrow ids -- order, list, sorted stream -- is what that walk reads)
    _assert_sparse_ran(info, detail, N, merged=not multi, launch=False if N == 511 else None)


# ---- the highest rank: every value of a column occurs exactly twice, D2 = N / 2
@pytest.mark.parametrize("N", [4096, 21844])
def test_k2_id16_highest_rank_does_not_meet_the_unique_flag(gpu_ctx, d2g, oracle, monkeypatch, N):
    """eight paired columns (ranks 1 .. N / 2: 10 922 at N = 21 844) beside clustered ones: the plane counts say D2 + 1 = N / 2 + 1 at either width"""
    import torch
    _sparse_env(monkeypatch, small=N < 8192)
    S = 32
    regs = _families(N, S, collisions=False, seed=N)
    regs[:, 3:11] = synth.paired_registers(N, 8, seed=N + 5)
    info, detail, planes = _both_widths(torch, gpu_ctx, d2g, oracle, monkeypatch, regs, f"paired N={N}")
    assert planes[0] == N // 2 + 1, planes                               # max over the columns of (shared values + 1)
    assert planes[1] == (N // 2 + 1).bit_length(), planes                # smallest nb with 2^nb >= D2 + 2
    _assert_sparse_ran(info, detail, N)


# ---- extremes: a column of all-distinct values (every id the unique flag), a column of ONE value (one rank, N holders)
@pytest.mark.parametrize("collisions", [0, 1])
@pytest.mark.parametrize("N,S", [(1300, 64), (1300, 32)])
def test_k2_id16_extreme_columns_beside_clustered_ones(gpu_ctx, d2g, oracle, monkeypatch, N, S, collisions):
    """Three families whose members all keep half of their parent's registers or more (every member is linked: the family columns add nothing to the list).
    The one-value column makes EVERY pair of different families a list entry, and every pair of its outsiders (two families of three) a slot: with
    n0 = N / 3 insiders and nO = 2 N / 3 outsiders, n0 nO + nO (nO - 1) / 2 slots -- 8 / 9 of the triangle.  Without chance collisions that fits the list
    (D2G_SP_LIST_DIV=1: an entry per pair of the triangle): pass B and the pair list run on narrow ids with one value of N holders, asserted by the list's
    length (families this large list more than 40 % of the tiles: the launch itself may walk them all).  A chance collision per sketch with a stranger's
    family adds N x ~0.75 x N / 3 entries, more than the ninth that is left: emit gives up and the dense walk is the right answer, at both widths alike;
    the all-distinct column is then checked beside collisions on a matrix of smaller families, where list and tiles are used."""
    import torch
    _sparse_env(monkeypatch, small=True)
    base = _families(N, S, collisions=bool(collisions), seed=N + S + collisions, nclusters=3, share_lo=0.5)
    distinct = (np.arange(N, dtype=np.uint64) << np.uint64(20)) + np.uint64(1 << 50)
    regs = base.copy()
    regs[:, 4] = distinct                                                # all distinct: every id the unique flag
    regs[:, 9] = np.uint64(0x1234567890)                                 # one value: one rank, N holders
    info, detail, planes = _both_widths(torch, gpu_ctx, d2g, oracle, monkeypatch, regs, f"extremes N={N} S={S} collisions={collisions}")
    assert info["sorted_operand"] and not info["ordering_skipped"], info
    assert (detail["schedule"], detail["prepare_kernels"]) == ("merged", MERGED), detail
    if not collisions:
        _assert_sparse_ran(info, detail, N, launch=False)
        assert info["pairs_listed"] >= (N // 3) * (N - N // 3 - 1), info  # (an entry per pair of different families at least)
    else:
        assert info["dense_decided_by_prepare"] and info["dense_kernel_ran"], info      # (more list entries than the list holds)
        regs = _families(N, S, collisions=True, seed=N + S)
        regs[:, 4] = distinct
        info, detail, _ = _both_widths(torch, gpu_ctx, d2g, oracle, monkeypatch, regs, f"all-distinct column N={N} S={S} collisions=1")
        _assert_sparse_ran(info, detail, N)


# ---- both link forms and both schedules
@pytest.mark.parametrize("merge,olink", [("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")])
def test_k2_id16_both_link_forms_and_both_schedules(gpu_ctx, d2g, oracle, monkeypatch, merge, olink):
    import torch
    _sparse_env(monkeypatch, small=True)
    monkeypatch.setenv("D2G_K2_MERGE", merge)
    monkeypatch.setenv("D2G_SP_OLINK", olink)
    N, S = 1300, 70                                                       # two x-blocks in the link grid, padding columns in the plan
    regs = _families(N, S, collisions=True, seed=99)
    info, detail, _ = _both_widths(torch, gpu_ctx, d2g, oracle, monkeypatch, regs, f"MERGE={merge} OLINK={olink}", update=True)
    _assert_sparse_ran(info, detail, N, merged=(merge, olink) == ("1", "1"))


def test_k2_id16_link_grid_of_several_blocks(gpu_ctx, d2g, oracle, monkeypatch):
    """N = 2100: three position blocks of the streaming link form (1024 sketches each), ten of the planes body behind flatten's nine"""
    import torch
    _sparse_env(monkeypatch, small=True)
    N, S = 2100, 64
    regs = _families(N, S, collisions=True, seed=2100)
    info, detail, _ = _both_widths(torch, gpu_ctx, d2g, oracle, monkeypatch, regs, "N=2100", update=True)
    _assert_sparse_ran(info, detail, N)


# ---- a set's first prepare: the first look's sample kernel reads the ids
def test_k2_id16_first_look_reads_narrow_ids(gpu_ctx, d2g, oracle, monkeypatch):
    """forget() then one step: the prepare looks at its matrix (sp_sample_kernel on 16-bit ids) and decides for the sparse path, as the 32-bit set does"""
    import torch
    monkeypatch.setenv("D2G_SP_LIST_FORM", "1")
    monkeypatch.setenv("D2G_K2_MERGE", "1")
    N, S = 9_000, 64
    stream = torch.cuda.current_stream().cuda_stream
    regs = synth.synthetic_registers(N, S, nclusters=60, seed=18)
    bits, t_dev = _to_dev(torch, regs)
    refs = _reference(torch, gpu_ctx, d2g, oracle, bits, t_dev, "first look", stream)
    sums = {}
    for id16, want in (("1", 16), ("0", 32)):
        monkeypatch.setenv("D2G_BS_ID16", id16)
        cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
        try:
            assert cs.id_bits == want
            for step in range(2):                                         # (creation looks; an update does not; forget() + update looks again)
                cs.forget()
                cs.update_dev(t_dev.data_ptr(), stream)
                outs = _launch_bands(torch, cs, N, stream, t_dev.device)
                info, detail = cs.sparse_info(stream), cs.sparse_detail(stream)
                print("first look", id16, step, info, detail)
                for out, ref in zip(outs, refs):
                    assert torch.equal(out, ref), (id16, step)
                assert detail["looked"] and not detail["looked_dense"], detail
                assert (detail["schedule"], detail["prepare_kernels"]) == ("classic", CLASSIC + 2), detail
                assert info["sorted_operand"] and not info["ordering_skipped"], info
                sums[id16, step] = tuple(detail[k] for k in ("entries", "family_pairs", "shared_values", "planes"))
        finally:
            cs.close()
    assert sums["1", 0] == sums["0", 0] == sums["1", 1] == sums["0", 1], sums       # the sample sees the same matrix through either word
