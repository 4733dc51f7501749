"""The FAST rank kernel writes the first pieces of an announced fill itself (bs_rank_kernel<false, true>, bit 64 of D2G_SP_RIDE, D2G_SP_RANK_SHARE).

announce -> update -> launch, as the benchmark's step does.  Every case checks
  * the output bit for bit against a CMP_DIRECT set's counts, mapped through the table (lut[0] != 0: the filled word is not zero) where the launch is a
    table launch,
  * a guard word on each side of the output, untouched, the launch going into a buffer pre-set to garbage,
  * `(schedule, prepare_kernels)` as tests/test_gpu_k2_prepare_merge.py states them: the fill moves between launches, it adds none,
  * `fill_detail`: rank + riders + launch == announced, and the rank kernel's part is what the case is about -- a silent fall-back to the riders shows
    as rank == 0, not as a pass.

Pieces are 32 KB (2048 vectors of 16 bytes); a rank workgroup holds at most six (twelve claim iterations x 1024 threads x 16 bytes)."""
import numpy as np
import pytest

from dashing2_amd import synth

pytestmark = pytest.mark.gpu

CLASSIC, MERGED, ONE_COLUMN = 13, 11, 9
PER_WG = 6
DEFAULT_SHARE = 35                                                      # D2G_SP_RANK_SHARE unset: the whole fill, as far as the grid holds it
GARBAGE = -3.0


def _ut_offsets(N):
    return np.concatenate([[0], np.cumsum(N - 1 - np.arange(N, dtype=np.int64))])


def _pieces(cnt):
    return -(-(cnt // 4 + 1) // 2048)


def _share(total, weight, cap):
    return min(total, cap, -(-total * weight // 35))


def _not_degenerate(regs, nclusters, collided):
    """a family of two or more members, and -- with collisions -- a pair of different families that shares a register (host arithmetic)"""
    N, S = regs.shape
    cl = np.arange(N) % nclusters
    fam = cross = False
    for j in range(min(N, 4 * nclusters)):
        c = (regs == regs[j]).sum(1)
        c[j] = 0
        fam |= bool((c[cl == cl[j]] >= min(S, 4)).any())
        cross |= bool((c[cl != cl[j]] >= 1).any())
    assert fam, "no family of two or more members"
    assert cross or not collided, "no cross-family entry"


def _force_small(monkeypatch):
    monkeypatch.setenv("D2G_BS_SPARSE_MIN_N", "1")
    monkeypatch.setenv("D2G_SP_TILE_FRAC", "1")
    monkeypatch.setenv("D2G_SP_PREDICT", "0")
    monkeypatch.setenv("D2G_SP_LIST_FORM", "1")
    monkeypatch.setenv("D2G_SP_LIST_DIV", "1")
    monkeypatch.setenv("D2G_SP_REMEMBER", "0")
    monkeypatch.setenv("D2G_K2_MERGE", "1")


_MATRICES = {}


def _matrix(torch, gpu_ctx, d2g, key, make, rows=None):
    """(device matrix, reference counts of rows [r0, r1) by a CMP_DIRECT set), made once per key and shared, never written again"""
    if key not in _MATRICES:
        regs = make()
        N, S = regs.shape
        r0, r1 = rows or (0, N)
        off = _ut_offsets(N)
        bits = np.ascontiguousarray(regs).view(np.uint64)
        t_dev = torch.from_numpy(bits.view(np.int64)).to(torch.device("cuda", 0))
        stream = torch.cuda.current_stream().cuda_stream
        ref = torch.empty(int(off[r1] - off[r0]), dtype=torch.int32, device=t_dev.device)
        dr = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_DIRECT, stream=stream)
        dr.eqcount_ut_dev(ref.data_ptr(), r0, r1, stream)
        torch.cuda.synchronize()
        dr.close()
        _MATRICES[key] = (t_dev, ref, (r0, r1))
    return _MATRICES[key]


def _families(N, S, nfam, collisions=1):
    def make():
        regs = synth.synthetic_registers(N, S, nclusters=nfam, seed=100 * S + N)
        if collisions:
            regs = synth.add_chance_collisions(regs, collisions, seed=N + S)
        _not_degenerate(regs, nfam, bool(collisions))
        return regs
    return make


def _lut(torch, d2g, S, device):
    lut_np = d2g.epilogue_lut(S, d2g.POISSON_LLR, 31, multiset_space=True)
    assert lut_np.view(np.uint32)[0] != 0
    return torch.from_numpy(lut_np).to(device)


def _step(torch, cs, t_dev, ref, ref_rows, lut, N, r0, r1, lead, stream, announce=True, counts=False):
    """announce -> update -> launch of rows [r0, r1) into garbage, `lead` words past a 16-byte boundary; -> (fill_detail, sparse_detail, sparse_info)"""
    off = _ut_offsets(N)
    cnt = int(off[r1] - off[r0])
    buf = torch.full((lead + cnt + 4,), GARBAGE, dtype=torch.float32, device=t_dev.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[lead:lead + cnt]
    if announce:
        cs.announce_ut_dev(out.data_ptr(), r0, r1, lut_dev_ptr=lut.data_ptr())
    else:
        cs.announce_ut_dev(out.data_ptr(), r0, r1, lut_dev_ptr=lut.data_ptr())
        cs.announce_ut_dev(None, r0, r1)                                # the cancelling form
    cs.update_dev(t_dev.data_ptr(), stream)
    fd = cs.fill_detail()                                               # (host bookkeeping: before anything is synchronised)
    if counts:
        cs.eqcount_ut_dev(out.data_ptr(), r0, r1, stream)
    else:
        cs.lut_ut_dev(lut.data_ptr(), out.data_ptr(), r0, r1, stream)
    detail, info = cs.sparse_detail(stream), cs.sparse_info(stream)
    torch.cuda.synchronize()
    base = int(off[r0] - off[ref_rows[0]])
    want = ref[base:base + cnt]
    if not counts:
        want = lut[want.long()]
    print(f"N={N} rows=[{r0},{r1}) lead={lead}", fd, detail["schedule"], detail["prepare_kernels"])
    bad = torch.nonzero(out.view(torch.int32) != want.view(torch.int32))
    assert bad.numel() == 0, ("first differing output", int(bad[0]), "of", int(bad.numel()), fd)
    assert bool((buf[:lead] == GARBAGE).all()) and bool((buf[lead + cnt:] == GARBAGE).all()), "a guard word was written"
    assert fd["rank"] + fd["riders"] + fd["launch"] == fd["announced"], fd
    assert fd["announced"] == (_pieces(cnt) if announce else 0), (fd, cnt)
    return fd, detail, info


@pytest.mark.parametrize("ride,share", [("64", None), ("64", "21"), ("127", None), ("127", "14"), ("96", "21"), ("63", None)])
def test_rank_kernel_writes_the_announced_fill(gpu_ctx, d2g, monkeypatch, ride, share):
    """N = 1300, S = 70: 104 pieces over 70 workgroups (not a multiple) for the whole triangle, a row range with the output 4 bytes past a 16-byte
    boundary.  The default share (35) is the whole fill: 104 pieces <= 6 x 70.  With a smaller share -- bit 64 alone: the launch fills what the rank kernel
    left; 127: the riders carry it by their weights; 96: the place kernel takes all of it; 63: the rank kernel writes nothing and everything rides, as
    before it."""
    import torch
    _force_small(monkeypatch)
    monkeypatch.setenv("D2G_SP_RIDE", ride)
    if share:
        monkeypatch.setenv("D2G_SP_RANK_SHARE", share)
    N, S, nfam = 1300, 70, 8
    stream = torch.cuda.current_stream().cuda_stream
    t_dev, ref, rr = _matrix(torch, gpu_ctx, d2g, (N, S, nfam, 1), _families(N, S, nfam))
    lut = _lut(torch, d2g, S, t_dev.device)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    try:
        for r0, r1, lead in ((0, N, 4), (N // 4 + 3, N // 4 + 500, 1)):
            fd, detail, info = _step(torch, cs, t_dev, ref, rr, lut, N, r0, r1, lead, stream)
            total = fd["announced"]
            assert total == 104 or (r0, r1) != (0, N)
            assert (detail["schedule"], detail["prepare_kernels"]) == ("merged", MERGED), detail
            assert info["tiles_and_pair_list"] and not info["dense_kernel_ran"], info
            if int(ride) & 64:
                assert fd["rank"] == _share(total, int(share or DEFAULT_SHARE), PER_WG * S) > 0, fd
            else:
                assert fd["rank"] == 0 and fd["riders"] == total, fd
            if share and ride != "64":
                assert fd["riders"] == total - fd["rank"] > 0, fd       # (the hosts behind the rank kernel really carried pieces)
            if ride == "64":
                assert fd["riders"] == 0, fd
            else:
                assert fd["launch"] == 0, fd                            # (the place kernel takes what is left)
    finally:
        cs.close()


@pytest.mark.parametrize("N,S,rows,lead,rank_pieces,kernels", [
    (300, 2, None, 4, 6, MERGED),                   # 6 pieces, two workgroups of three
    (300, 1, None, 4, 6, ONE_COLUMN),               # one workgroup, exactly its capacity
    (700, 1, None, 1, 6, ONE_COLUMN),               # 30 pieces, the grid holds six: riders and the launch carry the rest
    (300, 2, (298, 300), 4, 1, MERGED),             # one output, 16-byte aligned: piece 0's tail is the whole fill
    (300, 2, (298, 300), 1, 1, MERGED),             # one output, 4 bytes past: piece 0's head is
])
@pytest.mark.parametrize("ride", ["64", "127"])
def test_rank_fill_at_the_seams_of_a_workgroups_capacity(gpu_ctx, d2g, monkeypatch, N, S, rows, lead, rank_pieces, kernels, ride):
    """the whole share to the rank kernel (D2G_SP_RANK_SHARE=35): what bounds it is the grid, six pieces per column"""
    import torch
    _force_small(monkeypatch)
    monkeypatch.setenv("D2G_SP_RIDE", ride)
    monkeypatch.setenv("D2G_SP_RANK_SHARE", "35")
    nfam = 3
    stream = torch.cuda.current_stream().cuda_stream
    t_dev, ref, rr = _matrix(torch, gpu_ctx, d2g, (N, S, nfam, 1), _families(N, S, nfam))
    lut = _lut(torch, d2g, S, t_dev.device)
    r0, r1 = rows or (0, N)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    try:
        fd, detail, _ = _step(torch, cs, t_dev, ref, rr, lut, N, r0, r1, lead, stream)
        assert fd["announced"] == {(300, None): 6, (700, None): 30}.get((N, rows), 1), fd
        assert fd["rank"] == rank_pieces == min(fd["announced"], PER_WG * S), fd
        assert (fd["riders"] == 0) if ride == "64" else (fd["launch"] == 0), fd
        assert (detail["schedule"], detail["prepare_kernels"]) == ("merged", kernels), detail
    finally:
        cs.close()


@pytest.mark.parametrize("N,fast", [(12_288, True), (12_289, False)])
def test_rank_fill_at_the_seam_between_the_rank_kernels(gpu_ctx, d2g, monkeypatch, N, fast):
    """N = 12 288: the last set of the register kernel, twelve live values per thread; N = 12 289: the general kernel writes nothing, the riders carry
    the fill as before.  Rows [0, 64).  (The list's capacity and the tile budget stay at their defaults here: an entry per pair would be 600 MB.)"""
    import torch
    for k, v in (("D2G_BS_SPARSE_MIN_N", "1"), ("D2G_SP_PREDICT", "0"), ("D2G_SP_LIST_FORM", "1"), ("D2G_SP_REMEMBER", "0"), ("D2G_K2_MERGE", "1"), ("D2G_SP_RIDE", "127")):
        monkeypatch.setenv(k, v)
    S, nfam, r0, r1 = 32, 40, 0, 64
    stream = torch.cuda.current_stream().cuda_stream
    t_dev, ref, rr = _matrix(torch, gpu_ctx, d2g, (N, S, nfam, 0), _families(N, S, nfam, collisions=0), rows=(r0, r1))
    lut = _lut(torch, d2g, S, t_dev.device)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    try:
        fd, detail, info = _step(torch, cs, t_dev, ref, rr, lut, N, r0, r1, 1, stream)     # (64 rows that meet every family: the launch may walk all their tiles)
        assert info["sorted_operand"] and not info["ordering_skipped"], info
        assert (detail["schedule"], detail["prepare_kernels"]) == ("merged", MERGED), detail
        assert fd["rank"] == (_share(fd["announced"], DEFAULT_SHARE, PER_WG * S) if fast else 0), fd
        assert fd["launch"] == 0, fd
    finally:
        cs.close()


def test_rank_fill_waits_for_a_path_known_at_enqueue_time(gpu_ctx, d2g, monkeypatch):
    """N = 9 000, S = 64, default switches.  A prepare that takes the first look may still decide for the dense walk: the rank kernel in front of the look
    writes nothing (the riders behind it do).  The next one knows its path: merged, and the rank kernel takes its share.  Then a cancelled announcement."""
    import torch
    monkeypatch.setenv("D2G_SP_LIST_FORM", "1")
    monkeypatch.setenv("D2G_K2_MERGE", "1")
    monkeypatch.setenv("D2G_SP_RIDE", "127")                            # (said, not assumed: the suite also runs under D2G_SP_RIDE=63)
    N, S, nfam = 9_000, 64, 60
    stream = torch.cuda.current_stream().cuda_stream

    def make():
        regs = synth.add_chance_collisions(synth.synthetic_registers(N, S, nclusters=nfam, seed=18), 1, seed=19)
        _not_degenerate(regs, nfam, True)
        return regs
    t_dev, ref, rr = _matrix(torch, gpu_ctx, d2g, ("families+1", N, S), make)
    lut = _lut(torch, d2g, S, t_dev.device)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    try:
        assert cs.fill_detail() == {"announced": 0, "rank": 0, "riders": 0, "launch": 0}
        cs.forget()                                                     # (the next prepare decides as a set's first one does: it looks)
        fd, detail, info = _step(torch, cs, t_dev, ref, rr, lut, N, 0, N, 4, stream)
        assert detail["looked"] and not detail["looked_dense"], detail
        assert (detail["schedule"], detail["prepare_kernels"]) == ("classic", CLASSIC + 2), detail
        assert fd["rank"] == 0 and fd["riders"] == fd["announced"], fd
        fd, detail, info = _step(torch, cs, t_dev, ref, rr, lut, N, 0, N, 1, stream)
        assert not detail["looked"] and (detail["schedule"], detail["prepare_kernels"]) == ("merged", MERGED), detail
        assert fd["rank"] == _share(fd["announced"], DEFAULT_SHARE, PER_WG * S) > 0 and fd["launch"] == 0, fd
        fd, detail, info = _step(torch, cs, t_dev, ref, rr, lut, N, 0, N, 1, stream, announce=False)
        assert fd == {"announced": 0, "rank": 0, "riders": 0, "launch": 0}, fd
        assert (detail["schedule"], detail["prepare_kernels"]) == ("merged", MERGED), detail
    finally:
        cs.close()


def test_rank_fill_leaves_a_remembered_give_up_alone(gpu_ctx, d2g, monkeypatch):
    """a matrix the first look sends to the dense walk: the second prepare remembers, nothing rides -- the dense launch writes every output itself"""
    import torch
    monkeypatch.setenv("D2G_SP_LIST_FORM", "1")
    monkeypatch.setenv("D2G_K2_MERGE", "1")
    N, S = 9_000, 64
    stream = torch.cuda.current_stream().cuda_stream
    t_dev, ref, rr = _matrix(torch, gpu_ctx, d2g, ("skewed", N, S), lambda: synth.skewed_registers(N, S, seed=9))
    lut = _lut(torch, d2g, S, t_dev.device)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    try:
        fd, detail, info = _step(torch, cs, t_dev, ref, rr, lut, N, 0, N, 1, stream)
        assert info["ordering_skipped"] and info["dense_kernel_ran"] and not detail["looked"], (info, detail)
        assert (detail["schedule"], detail["prepare_kernels"]) == ("classic", 5), detail
        assert fd["rank"] == 0 and fd["riders"] == 0 and fd["launch"] == fd["announced"] > 0, fd
    finally:
        cs.close()


def test_rank_fill_of_a_table_value_is_not_taken_for_a_count_launch(gpu_ctx, d2g, monkeypatch):
    """announced for a table launch (fill value lut[0]), then a COUNT launch into the same buffer: the launch fills again and the counts are right"""
    import torch
    _force_small(monkeypatch)
    monkeypatch.setenv("D2G_SP_RIDE", "127")
    N, S, nfam = 1300, 70, 8
    stream = torch.cuda.current_stream().cuda_stream
    t_dev, ref, rr = _matrix(torch, gpu_ctx, d2g, (N, S, nfam, 1), _families(N, S, nfam))
    lut = _lut(torch, d2g, S, t_dev.device)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    try:
        fd, detail, _ = _step(torch, cs, t_dev, ref, rr, lut, N, 0, N, 1, stream, counts=True)
        assert fd["rank"] > 0 and fd["launch"] == 0, fd
        assert (detail["schedule"], detail["prepare_kernels"]) == ("merged", MERGED), detail
    finally:
        cs.close()

