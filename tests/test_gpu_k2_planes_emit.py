"""Schedule 2 of the bit-sliced prepare (D2G_K2_MERGE=2; d2g_bitslice_prepare + sp_prepare_order): the caller's-order planes leave the launch they shared
with flatten and stand BEHIND the workgroups of the pair-list kernel -- sp_emit_kernel<IdT, true>: blocks [0, S) are emit, block S + b takes items 2 b
and 2 b + 1 of the planes' (position block, register group) grid, 256 threads each.  Nobody reads that stream before the permute kernel; the dense walk
and every rectangular launch read it afterwards, also when emit gave up and its own blocks left at once.

Every case runs under D2G_K2_MERGE = 0, 1 and 2 on the same matrix, and the three runs must agree:
  * the whole triangle's equality counts, launched into garbage, bit for bit the direct kernel's (a CMP_DIRECT set, itself pinned on oracle rows);
  * `planes()` -- what the column plan and the rank kernel left -- equal in all three;
  * `sparse_detail` names the schedule asked for and the kernels it enqueued (a silent fallback to another schedule passes nothing here);
  * a rectangular launch behind the prepare -- it reads the caller's-order stream, the one the moved workgroups write -- equal to the direct kernel's.
Kernels a prepare enqueues, the transpose included (D2G_SP_LIST_FORM=1):
    0 classic      transpose, rank, plan, planes, link 0, flatten, link 1, count, attach, scan, place, emit, permute              13
    1 merged       transpose, rank, [plan + link 0], [flatten + planes], link 1, count, attach, scan, place, emit, permute        11
    2 planes-emit  transpose, rank, [plan + link 0], flatten, link 1, count, attach, scan, place, [emit + planes], permute        11
    one column (no link pass, no flatten, no attach): 9, 9 and -- no second launch at all, emit carries the planes -- 8."""
import numpy as np
import pytest

from dashing2_amd import synth

pytestmark = pytest.mark.gpu

SCHEDULES = {0: "classic", 1: "merged", 2: "planes-emit"}
KERNELS = {0: 13, 1: 11, 2: 11}
KERNELS_ONE_COLUMN = {0: 9, 1: 9, 2: 8}


def _ut_offsets(N):
    return np.concatenate([[0], np.cumsum(N - 1 - np.arange(N, dtype=np.int64))])


def _rows(N):
    """the first and the last rows that have pairs, and the seams of the 32-row bands and 256-column tiles"""
    want = [0, 1, 31, 32, 33, 255, 256, 257, N // 2, N - 258, N - 257, N - 34, N - 33, N - 3, N - 2]
    return sorted({min(max(r, 0), N - 2) for r in want})


def _rect(N):
    """a rectangle off the diagonal whose rows and columns cross a 32-row band and a 256-column tile seam, and whose columns end at the last sketch"""
    a0 = max(0, min(250, N // 2 - 20))
    return a0, a0 + 40, N - 70, N


def _to_dev(torch, regs):
    bits = np.ascontiguousarray(regs).view(np.uint64)
    return bits, torch.from_numpy(bits.view(np.int64)).to(torch.device("cuda", 0))


def _reference(torch, gpu_ctx, d2g, oracle, bits, t_dev, label, stream):
    """the direct kernel's whole triangle and rectangle, the triangle pinned on the oracle's rows; once per matrix, shared by the three schedules, never written again"""
    N, S = bits.shape
    a0, a1, b0, b1 = _rect(N)
    ref = torch.empty(N * (N - 1) // 2, dtype=torch.int32, device=t_dev.device)
    rect = torch.empty((a1 - a0, b1 - b0), dtype=torch.int32, device=t_dev.device)
    dr = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_DIRECT, stream=stream)
    dr.eqcount_ut_dev(ref.data_ptr(), 0, N, stream)
    dr.eqcount_rect_dev(rect.data_ptr(), a0, a1, b0, b1, stream)
    torch.cuda.synchronize()
    dr.close()
    off = _ut_offsets(N)
    m = bits.view(np.float64)
    for i in _rows(N):
        np.testing.assert_array_equal(ref[int(off[i]):int(off[i + 1])].cpu().numpy().view(np.uint32), oracle.eqcounts_rows(m, int(i), int(i) + 1),
                                      err_msg=f"{label}: direct kernel, row {i}")
    return ref, rect


def _force_small(monkeypatch):
    monkeypatch.setenv("D2G_BS_SPARSE_MIN_N", "1")
    monkeypatch.setenv("D2G_SP_TILE_FRAC", "1")                         # (matrices this small have few tiles: the families' share of them is large)
    monkeypatch.setenv("D2G_SP_PREDICT", "0")                           # (no first look: the set's first prepare already knows its path)
    monkeypatch.setenv("D2G_SP_LIST_FORM", "1")
    monkeypatch.setenv("D2G_SP_LIST_DIV", "1")                          # (a few columns and large families: the list may hold an entry per pair)
    monkeypatch.setenv("D2G_SP_REMEMBER", "0")                          # (where the ordering gives up, the next prepare runs it again: no remembered skip)
    monkeypatch.setenv("D2G_SP_OLINK", "1")


def _one_schedule(torch, gpu_ctx, d2g, monkeypatch, merge, t_dev, N, S, ref, rect, label, stream, prepares=2):
    """the matrix prepared `prepares` times (creation, then updates) under D2G_K2_MERGE=merge, each followed by a whole triangle and a rectangle into
    garbage; -> (sparse_info, sparse_detail, planes) of the last"""
    monkeypatch.setenv("D2G_K2_MERGE", str(merge))
    assert gpu_ctx.tuning()["resolved"]["D2G_K2_MERGE"] == merge        # (the context reports what the switch resolved to)
    a0, a1, b0, b1 = _rect(N)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    try:
        for rep in range(prepares):
            if rep:
                cs.update_dev(t_dev.data_ptr(), stream)
            out = torch.full((N * (N - 1) // 2,), -7, dtype=torch.int32, device=t_dev.device)
            got = torch.full((a1 - a0, b1 - b0), -7, dtype=torch.int32, device=t_dev.device)
            cs.eqcount_ut_dev(out.data_ptr(), 0, N, stream)
            info, detail, planes = cs.sparse_info(stream), cs.sparse_detail(stream), cs.planes(stream)
            cs.eqcount_rect_dev(got.data_ptr(), a0, a1, b0, b1, stream)
            cs.status(stream)
            torch.cuda.synchronize()
            print(f"{label} MERGE={merge} prepare {rep + 1}", info, {k: detail[k] for k in ("schedule", "merge", "prepare_kernels")}, planes)
            bad = torch.nonzero(out != ref)
            assert bad.numel() == 0, (label, merge, rep, "first differing pair index", int(bad[0]), "of", int(bad.numel()))
            badr = torch.nonzero(got != rect)
            assert badr.numel() == 0, (label, merge, rep, "rectangle: first differing cell", badr[0].tolist(), "of", int(badr.shape[0]))
            assert info["sorted_operand"] and not info["ordering_skipped"], (label, merge, info)
            assert (detail["schedule"], detail["merge"]) == (SCHEDULES[merge], merge), (label, merge, detail)
            assert detail["prepare_kernels"] == (KERNELS_ONE_COLUMN if S == 1 else KERNELS)[merge], (label, merge, detail)
        return info, detail, planes
    finally:
        cs.close()


def _three_schedules(torch, gpu_ctx, d2g, oracle, monkeypatch, regs, label):
    """-> {merge: (info, detail, planes)}; the three runs against one reference, their plane counts against each other.  (Whether the ordering keeps its
    order or gives up goes by the families the racing stores of the link pass found: at 300 sketches in three families it differs from prepare to prepare
    under ONE schedule -- 14 572 to 31 033 pairs listed, measured -- so the schedules are not compared in it; the counts are exact either way.)"""
    N, S = regs.shape
    stream = torch.cuda.current_stream().cuda_stream
    bits, t_dev = _to_dev(torch, regs)
    ref, rect = _reference(torch, gpu_ctx, d2g, oracle, bits, t_dev, label, stream)
    runs = {m: _one_schedule(torch, gpu_ctx, d2g, monkeypatch, m, t_dev, N, S, ref, rect, label, stream) for m in (0, 1, 2)}
    for m in (1, 2):
        assert runs[m][2] == runs[0][2], (label, "planes", m, runs[m][2], runs[0][2])
    return runs


def _families(N, S, nfam, collisions, seed):
    regs = synth.synthetic_registers(N, S, nclusters=nfam, seed=seed)
    return synth.add_chance_collisions(regs, 1, seed=seed + 1) if collisions else regs


# N, S, families -- what each shape is for (emit blocks [0, S); gx = ceil((Npad + 64) / 256) position blocks x ceil(S / 32) groups of planes items behind them):
SHAPES = [
    (300, 1, 3),        # one column, no link pass: 3 planes items, so a half-empty last rider block; emit carries the planes and no launch holds flatten
    (300, 33, 3),       # two register groups, 31 padding slots in the second
    (1300, 70, 8),      # S no multiple of 32
    (2100, 64, 14),     # 10 x 2 items: rider blocks of two DIFFERENT groups' halves behind 64 emit blocks
    (260, 4100, 3),     # S above BS_PLAN_MAXS: identity column order; 387 rider blocks behind 4100 emit blocks
    (2101, 64, 14),     # odd N: emit's 32-bit loads of id pairs (the last one half padding) beside the planes' 2-byte loads
]


@pytest.mark.parametrize("N,S,nfam", SHAPES)
def test_k2_planes_behind_emit_smallest_shapes(gpu_ctx, d2g, oracle, monkeypatch, N, S, nfam):
    """family matrices with a chance collision per sketch (mixed values: emit's long workgroups run beside the planes), 16-bit ids"""
    import torch
    _force_small(monkeypatch)
    regs = _families(N, S, nfam, collisions=True, seed=100 * S + N)
    _three_schedules(torch, gpu_ctx, d2g, oracle, monkeypatch, regs, f"N={N} S={S}")


def test_k2_planes_behind_emit_32_bit_ids(gpu_ctx, d2g, oracle, monkeypatch):
    """D2G_BS_ID16=0: the other instantiation of the launch (one 4-byte id per lane in either body)"""
    import torch
    _force_small(monkeypatch)
    monkeypatch.setenv("D2G_BS_ID16", "0")
    N, S = 1300, 70
    _three_schedules(torch, gpu_ctx, d2g, oracle, monkeypatch, _families(N, S, 8, True, seed=100 * S + N + 5), "ID16=0")


def test_k2_planes_behind_emit_when_the_ordering_gives_up_on_the_device(gpu_ctx, d2g, oracle, monkeypatch):
    """Three families and ONE value in a whole column, with a chance collision per sketch: every pair of different families is a list entry, more than the
    list holds (tests/test_gpu_k2_id16.py, the extreme columns) -- emit raises order[0] on the device, its blocks leave at their next look at that word, and
    with D2G_SP_REMEMBER=0 every prepare runs the ordering again.  The dense walk behind it, and the rectangle, read the caller's-order stream: complete,
    although the blocks in front of the planes' left at once."""
    import torch
    _force_small(monkeypatch)
    N, S = 1300, 64
    regs = synth.add_chance_collisions(synth.synthetic_registers(N, S, nclusters=3, seed=N + S + 1, share_lo=0.5), 1, seed=N + S + 2)
    regs[:, 9] = np.uint64(0x1234567890)                                 # one value: one rank, N holders
    runs = _three_schedules(torch, gpu_ctx, d2g, oracle, monkeypatch, regs, "give-up")
    for m, (info, detail, _) in runs.items():
        assert info["dense_decided_by_prepare"] and info["dense_kernel_ran"] and not info["ordering_skipped"], (m, info)


def test_k2_planes_behind_emit_carries_on_under_an_announced_fill(gpu_ctx, d2g, oracle, monkeypatch):
    """announce -> update -> launch with the table epilogue, twice into an output preset to garbage (the benchmark's step, as test_k2_timed_sequence runs
    it) at N = 2100: flatten, alone in its launch now, still hosts its share of the fill's riders; every word of the output is written in all schedules."""
    import torch
    _force_small(monkeypatch)
    N, S = 2100, 64
    stream = torch.cuda.current_stream().cuda_stream
    regs = _families(N, S, 14, True, seed=100 * S + N)
    bits, t_dev = _to_dev(torch, regs)
    ref, _ = _reference(torch, gpu_ctx, d2g, oracle, bits, t_dev, "announced", stream)
    lut_np = d2g.epilogue_lut(S, d2g.POISSON_LLR, 31, multiset_space=True)
    assert lut_np.view(np.uint32)[0] != 0                               # (the filled word is not zero)
    lut = torch.from_numpy(lut_np).to(t_dev.device)
    want = lut[ref.long()].view(torch.int32)
    fills = {}
    for merge in (0, 1, 2):
        monkeypatch.setenv("D2G_K2_MERGE", str(merge))
        cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
        try:
            for rep in range(2):
                buf = torch.full((ref.numel() + 2,), -3.0, dtype=torch.float32, device=t_dev.device)
                buf.view(torch.int32)[1:-1].fill_(0x7FC12345)           # garbage (a NaN pattern no table holds)
                out = buf[1:-1]
                cs.announce_ut_dev(out.data_ptr(), 0, N, lut_dev_ptr=lut.data_ptr())
                cs.update_dev(t_dev.data_ptr(), stream)
                cs.lut_ut_dev(lut.data_ptr(), out.data_ptr(), 0, N, stream)
                detail, fills[merge] = cs.sparse_detail(stream), cs.fill_detail()
                torch.cuda.synchronize()
                print(f"announced MERGE={merge} prepare {rep + 1}", detail["schedule"], detail["prepare_kernels"], fills[merge])
                assert torch.equal(out.view(torch.int32), want), (merge, rep)
                assert float(buf[0]) == -3.0 and float(buf[-1]) == -3.0, (merge, rep)
                assert (detail["schedule"], detail["merge"], detail["prepare_kernels"]) == (SCHEDULES[merge], merge, KERNELS[merge]), detail
                assert fills[merge]["announced"] > 0 and fills[merge]["rank"] + fills[merge]["riders"] + fills[merge]["launch"] == fills[merge]["announced"], fills[merge]
        finally:
            cs.close()
    assert fills[2] == fills[1], fills                                   # (the riders' weights are those of schedule 1: the same pieces on the same hosts)
