"""The all-pairs sparse path (tiles of families + pair list, d2g_k2_sparse.h) at the shapes its other tests do not reach: sketch sizes of 2048
and more (the first look's per-sample sums), S = 65 535 (the largest the path takes), output bins 2048-8192 columns wide (cshift 11-13:
several 1024-column pieces per chunk in the composer) and the bin geometry's limit (1 277 952 sketches: one chunk of 2^21 columns; one
sketch more and the list is applied entry by entry).

Every matrix is checked three ways: equality counts against the direct kernel (whole triangle where it fits, row ranges otherwise),
32+ rows against the oracle (first and last rows, band / chunk / sample-row seams), the table epilogue bit for bit with lut[0] != 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dashing2_amd import synth

pytestmark = pytest.mark.gpu

SAMPLE_ROWS, SAMPLE_COLS, SAMPLE_FAM = 16, 32, 4


def _ut_offsets(N):
    return np.concatenate([[0], np.cumsum(N - 1 - np.arange(N, dtype=np.int64))])


def _lut(d2g, S):
    lut = d2g.epilogue_lut(S, d2g.POISSON_LLR, 31, multiset_space=True)
    assert lut.view(np.uint32)[0] != 0                                 # (the filled word is not zero)
    return lut


def _sample_rows(N):
    return [min(N - 1, (2 * k + 1) * N // (2 * SAMPLE_ROWS)) for k in range(SAMPLE_ROWS)]


def _first_look_reference(bits):
    """(E, F, shared values, planes) as sp_sample_kernel + sp_sample_fin_kernel define them, in exact integers"""
    N, S = bits.shape
    G = -(-S // SAMPLE_COLS)
    E = F = 0
    eq = np.zeros((N, G * SAMPLE_COLS), bool)
    for r in _sample_rows(N):
        eq[:, :S] = bits == bits[r]
        c = np.minimum(eq.reshape(N, G, SAMPLE_COLS).sum(2, dtype=np.int32), SAMPLE_FAM).sum(1, dtype=np.int64)
        c[r] = 0
        F += int((c >= SAMPLE_FAM).sum())
        E += int(c[(c > 0) & (c < SAMPLE_FAM)].sum())
    srt = np.sort(np.ascontiguousarray(bits.T), axis=1)               # [S][N]
    same = srt[:, 1:] == srt[:, :-1]
    first = same.copy()
    first[:, 1:] &= ~same[:, :-1]                                      # the first repeat of every value held by >= 2 sketches
    v = first.sum(1)
    planes = sum(int(x + 1).bit_length() for x in v)
    return E, F, int(v.sum()), planes


def _one_collision(regs, seed):
    """add_chance_collisions(regs, 1) without its per-sketch Python loop (millions of sketches)"""
    rng = np.random.default_rng(seed)
    N, S = regs.shape
    cols = rng.integers(0, S, N)
    other = rng.integers(0, N - 1, N)
    other = other + (other >= np.arange(N))
    out = regs.copy()
    out[np.arange(N), cols] = regs[other, cols]
    return out


def _oracle_rows(oracle, m, rows, host_of_row, label):
    for i in rows:
        np.testing.assert_array_equal(host_of_row(i), oracle.eqcounts_rows(m, int(i), int(i) + 1), err_msg=f"{label} row {i}")


def _check_whole(torch, gpu_ctx, d2g, oracle, cs, t_dev, m, N, S, lut_np, rows, label, stream):
    """whole triangle: counts vs the direct kernel, rows vs the oracle, the table epilogue bit for bit; -> (sparse_info, sparse_detail)"""
    dev = t_dev.device
    npairs = N * (N - 1) // 2
    out = torch.full((npairs,), -1, dtype=torch.int32, device=dev)
    cs.eqcount_ut_dev(out.data_ptr(), 0, N, stream)
    info, detail = cs.sparse_info(stream), cs.sparse_detail(stream)
    ref = torch.empty(npairs, dtype=torch.int32, device=dev)
    dr = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_DIRECT, stream=stream)
    dr.eqcount_ut_dev(ref.data_ptr(), 0, N, stream)
    torch.cuda.synchronize()
    dr.close()
    assert torch.equal(out, ref), label
    del out
    lut = torch.from_numpy(lut_np).to(dev)
    fout = torch.full((npairs,), -2.0, dtype=torch.float32, device=dev)
    cs.lut_ut_dev(lut.data_ptr(), fout.data_ptr(), 0, N, stream)
    torch.cuda.synchronize()
    step = 1 << 27
    for a in range(0, npairs, step):
        b = min(npairs, a + step)
        assert torch.equal(fout[a:b].view(torch.int32), lut[ref[a:b].long()].view(torch.int32)), (label, a)
    del fout
    off = _ut_offsets(N)
    _oracle_rows(oracle, m, rows, lambda i: ref[int(off[i]):int(off[i + 1])].cpu().numpy().view(np.uint32), label)
    return info, detail, ref


def _fam_cases(N, S, seed):
    fam = synth.synthetic_registers(N, S, nclusters=N // 150, seed=seed)
    return [("families", fam), ("families+1", synth.add_chance_collisions(fam, 1, seed=seed + 1)),
            ("families+10", synth.add_chance_collisions(fam, 10, seed=seed + 2)), ("paired", synth.paired_registers(N, S, seed=seed + 3)),
            ("skewed", synth.skewed_registers(N, S, seed=seed + 4)), ("unrelated", synth.unrelated_registers(N, S, seed=seed + 5))]


def _rows_9000(N):
    return sorted(set([0, 1, 2, 31, 32, 33, 255, 256, 4095, 4096, 4097] + _sample_rows(N) + [r + 1 for r in _sample_rows(N)][:8]
                      + list(range(N - 6, N - 1))) - {N - 1})


@pytest.mark.parametrize("S", [1024, 2048, 2080, 4096])
def test_k2_first_look_sums_are_exact_and_counts_hold_at_wide_sketches(gpu_ctx, d2g, oracle, monkeypatch, S):
    """The first look (sixteen sampled sketches against all, before the ordering of a set's first prepare) sums, per (sample, sketch), the
    equal registers of every 32-column group capped at 4: from 64 groups (S = 2048) on a sum reaches 256.  Its raw sums -- register counts
    below 4 (E), pairs at 4 or more (F), shared values, id planes -- equal a NumPy restatement exactly, and its decision is the one it takes at
    S = 1024: dense for a random pairing per column and for skewed columns, sparse for families and unrelated sketches.  Counts of every matrix
    against the direct kernel, the oracle and the table epilogue."""
    import torch
    monkeypatch.setenv("D2G_SP_REMEMBER", "0")
    N = 9_000
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    lut_np = _lut(d2g, S)
    rows = _rows_9000(N)
    want_dense = {"paired": True, "skewed": True, "families": False, "unrelated": False}
    for name, regs in _fam_cases(N, S, seed=S * 10 + 1):
        bits = np.ascontiguousarray(regs).view(np.uint64)
        t_dev = torch.from_numpy(bits.view(np.int64)).to(dev)
        cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)     # the set's first prepare: it looks
        info, detail, _ = _check_whole(torch, gpu_ctx, d2g, oracle, cs, t_dev, bits.view(np.float64), N, S, lut_np, rows, f"S={S} {name}", stream)
        cs.close()
        del t_dev
        assert detail["looked"], (S, name, detail)
        E, F, values, planes = _first_look_reference(bits)
        assert (detail["entries"], detail["family_pairs"], detail["shared_values"], detail["planes"]) == (E, F, values, planes), (S, name, detail)
        if name in want_dense:
            assert detail["looked_dense"] == want_dense[name], (S, name, detail)
            assert info["dense_kernel_ran"] == want_dense[name] and info["ordering_skipped"] == want_dense[name], (S, name, info)


@pytest.mark.parametrize("form", ["1", "2"])
@pytest.mark.parametrize("S", [2048, 2080, 4096])
def test_k2_both_list_forms_at_wide_sketches(gpu_ctx, d2g, oracle, monkeypatch, S, form):
    """Ten chance collisions per sketch on a family collection: a list of millions of entries over 64-128 register groups, applied entry by
    entry (D2G_SP_LIST_FORM=1) and binned + composed (=2).  (A list of up to pairs / 2 entries: at S = 4096 the family members that keep few
    of their parent's registers put more entries on it than the default pairs / 8 hold, and the ordering would give up.)"""
    import torch
    monkeypatch.setenv("D2G_SP_REMEMBER", "0")
    monkeypatch.setenv("D2G_SP_LIST_DIV", "2")
    monkeypatch.setenv("D2G_SP_LIST_FORM", form)
    N = 9_000
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    fam = synth.synthetic_registers(N, S, nclusters=N // 150, seed=S + 7)
    bits = np.ascontiguousarray(synth.add_chance_collisions(fam, 10, seed=S + 8)).view(np.uint64)
    t_dev = torch.from_numpy(bits.view(np.int64)).to(dev)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    info, detail, ref = _check_whole(torch, gpu_ctx, d2g, oracle, cs, t_dev, bits.view(np.float64), N, S, _lut(d2g, S), _rows_9000(N), f"S={S} form {form}", stream)
    assert info["tiles_and_pair_list"] and not info["dense_kernel_ran"] and info["pairs_listed"] > 0, info
    assert detail["binned"] == (form == "2"), detail
    off = _ut_offsets(N)
    for r0, r1 in ((37, 45), (N // 2 - 3, N // 2 + 1029), (N - 100, N)):
        np.testing.assert_array_equal(cs.eqcount_ut(r0, r1), ref[int(off[r0]):int(off[r1])].cpu().numpy().view(np.uint32), err_msg=f"rows {r0}:{r1}")
    cs.close()


@pytest.mark.parametrize("form", ["2", "1"])
@pytest.mark.parametrize("case", ["pair", "family"])
def test_k2_sparse_path_at_the_largest_sketch_size(gpu_ctx, d2g, oracle, monkeypatch, case, form):
    """S = 65 535, the largest sketch size the sparse path takes: a count still fits the 16-bit fields of the composer's LDS and of the sparse
    pair kernel's packed mismatch sums.  400 unrelated sketches and either one pair that shares every other register -- no family (no two
    adjacent registers agree): 32 768 list entries for one pair -- or a family of four identical sketches (65 535 equal registers: one
    listed tile).  No first look (its cost model sends so small a set to the dense walk) and a list as long as the triangle, so that the
    ordering keeps the sparse path; both list forms.  Regression (the pair): sp_emit_kernel's early projection of the list's length took the
    pairs so far and the columns so far from two atomics -- with 32 768 columns of one pair each finishing together the pairs ran ahead and
    the ordering gave up now and then; eight more prepares of the same matrix must all keep the sparse path."""
    import torch
    monkeypatch.setenv("D2G_BS_SPARSE_MIN_N", "256")
    monkeypatch.setenv("D2G_SP_PREDICT", "0")
    monkeypatch.setenv("D2G_SP_LIST_DIV", "1")
    monkeypatch.setenv("D2G_SP_REMEMBER", "0")
    monkeypatch.setenv("D2G_SP_LIST_FORM", form)
    N, S = 400, 65_535
    bits = synth.unrelated_registers(N, S, seed=77)
    if case == "pair":
        bits[250, 0::2] = bits[7, 0::2]                                # 32 768 equal registers
    else:
        for j in (100, 101, 102):
            bits[j] = bits[99]                                         # identical: all 65 535
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    t_dev = torch.from_numpy(bits.view(np.int64)).to(dev)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    rows = sorted(set(list(range(0, 12)) + [7, 31, 32, 63, 64, 98, 99, 100, 101, 102, 149, 150, 250, 255, 256] + list(range(N - 12, N - 1))))
    info, detail, ref = _check_whole(torch, gpu_ctx, d2g, oracle, cs, t_dev, bits.view(np.float64), N, S, _lut(d2g, S), rows, f"S=65535 {case} form {form}", stream)
    off = _ut_offsets(N)
    assert info["tiles_and_pair_list"] and not info["dense_kernel_ran"], info
    assert detail["binned"] == (form == "2"), detail
    if case == "pair":
        assert int(ref[int(off[7]) + 250 - 7 - 1]) == 32_768
        assert info["pairs_listed"] == 32_768 and info["tiles_listed"] == 0, info
    else:
        assert [int(ref[int(off[99]) + k]) for k in range(3)] == [S, S, S]
        assert info["tiles_listed"] > 0, info
    for r0, r1 in ((0, 1), (5, 9), (7, 8), (99, 130), (N - 40, N)):
        np.testing.assert_array_equal(cs.eqcount_ut(r0, r1), ref[int(off[r0]):int(off[r1])].cpu().numpy().view(np.uint32), err_msg=f"rows {r0}:{r1}")
    if case == "pair":
        out = torch.empty_like(ref)
        for step in range(8):
            cs.update_dev(t_dev.data_ptr(), stream)
            cs.eqcount_ut_dev(out.data_ptr(), 0, N, stream)
            info = cs.sparse_info(stream)
            assert info["tiles_and_pair_list"] and not info["dense_kernel_ran"] and info["pairs_listed"] == 32_768, (step, info)
            assert torch.equal(out, ref), step
    cs.close()


@pytest.mark.parametrize("N", [400, 8192 + 400])
def test_k2_segment_ends_stay_inside_the_collection(gpu_ctx, d2g, monkeypatch, N):
    """Regression: sp_scan_kernel wrote the end of the last segment of every 8192 counters from a running total that its thread 0 may already have
    advanced -- a segment [a, ~2N) for a sketch alone, whose tiles were then set past the tile bitmap, into the control words behind it (at 400
    sketches the order word: the ordering "gave up" now and then).  Unrelated sketches have no segment of two: every prepare of the set keeps
    the sparse path with no tile listed, and every count is 0."""
    import torch
    monkeypatch.setenv("D2G_BS_SPARSE_MIN_N", "256")
    monkeypatch.setenv("D2G_SP_PREDICT", "0")
    monkeypatch.setenv("D2G_SP_REMEMBER", "0")
    S = 64
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    bits = synth.unrelated_registers(N, S, seed=N)
    t_dev = torch.from_numpy(bits.view(np.int64)).to(dev)
    out = torch.empty(N * (N - 1) // 2, dtype=torch.int32, device=dev)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    for step in range(32):
        if step:
            cs.update_dev(t_dev.data_ptr(), stream)
        out.fill_(-1)
        cs.eqcount_ut_dev(out.data_ptr(), 0, N, stream)
        info = cs.sparse_info(stream)
        assert info["sorted_operand"] and info["tiles_and_pair_list"] and not info["callers_order_kept"], (step, info)
        assert info["tiles_listed"] == 0 and info["pairs_listed"] == 0, (step, info)
        assert int(torch.count_nonzero(out)) == 0, step
    cs.close()


def _seam_rows(N, cshift):
    rows = set(range(0, 6)) | set(range(N - 6, N - 1)) | {31, 32, 33, 37, 44, 45}
    for c in range(1 << cshift, N, 1 << cshift):
        rows |= {c - 1, c, c + 1}                                      # chunk seams
    rows |= {N // 2 - 33, N // 2 - 32, N // 2 - 4, N // 2 - 3, N // 2 + 1028, N // 2 + 1029}
    rows |= set(_sample_rows(N)[::2])
    return sorted(r for r in rows if 0 <= r < N - 1)


def _row_ranges(N):
    return ((N // 3, N // 3 + 1), (37, 45), (N // 2 - 3, N // 2 + 1029), (N - 333, N))


@pytest.mark.parametrize("form", ["2", "default"])
@pytest.mark.parametrize("N,cshift", [(40_000, 11), (60_000, 12), (80_000, 13)])
def test_k2_binned_list_with_wide_chunks(gpu_ctx, d2g, oracle, monkeypatch, N, cshift, form):
    """From 35 841 sketches on a chunk of the output bins is 2^cshift > 1024 columns wide and the composer walks it in 1024-column pieces
    (2, 4, 8 of them here).  S = 32, ten chance collisions per sketch: a list of millions of entries, binned.  Whole triangle (40 000 and 80 000)
    against the direct kernel; row ranges -- a single row, ranges that start and end inside a 32-row band and an 8-row group, one that ends at
    N -- against the whole-triangle launch, the direct kernel and the oracle; the table epilogue."""
    import torch
    monkeypatch.setenv("D2G_SP_REMEMBER", "0")
    if form != "default":
        monkeypatch.setenv("D2G_SP_LIST_FORM", form)
    S = 32
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    fam = synth.synthetic_registers(N, S, nclusters=N // 150, seed=N + 1)
    bits = np.ascontiguousarray(synth.add_chance_collisions(fam, 10, seed=N + 2)).view(np.uint64)
    m = bits.view(np.float64)
    lut_np = _lut(d2g, S)
    t_dev = torch.from_numpy(bits.view(np.int64)).to(dev)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    rows = _seam_rows(N, cshift)
    off = _ut_offsets(N)
    ref = None
    if N != 60_000:
        info, detail, ref = _check_whole(torch, gpu_ctx, d2g, oracle, cs, t_dev, m, N, S, lut_np, rows, f"N={N} form {form}", stream)
        assert info["tiles_and_pair_list"] and not info["dense_kernel_ran"], info
    else:
        cs.eqcount_ut(0, 1)
        detail = cs.sparse_detail()
    assert detail["binned"] and detail["bin_cshift"] == cshift, detail
    dr = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_DIRECT, stream=stream)
    for r0, r1 in _row_ranges(N):
        got = cs.eqcount_ut(r0, r1)
        want = dr.eqcount_ut(r0, r1)
        np.testing.assert_array_equal(got, want, err_msg=f"rows {r0}:{r1}")
        if ref is not None:
            np.testing.assert_array_equal(got, ref[int(off[r0]):int(off[r1])].cpu().numpy().view(np.uint32), err_msg=f"rows {r0}:{r1} (whole)")
        _oracle_rows(oracle, m, [r for r in rows if r0 <= r < r1], lambda i: got[int(off[i] - off[r0]):int(off[i + 1] - off[r0])], f"rows {r0}:{r1}")
        fgot = cs.lut_ut(lut_np, r0, r1)
        np.testing.assert_array_equal(fgot.view(np.uint32), lut_np[want].view(np.uint32), err_msg=f"table rows {r0}:{r1}")
        assert cs.sparse_detail()["binned"]
    if ref is None:                                                    # (no whole triangle: single-row launches at the seams)
        _oracle_rows(oracle, m, rows[:40], lambda i: cs.eqcount_ut(i, i + 1), f"N={N}")
    dr.close()
    cs.close()


def _geometry_in_a_child(N):
    """sparse_bin_geometry(N) in a child process: a host loop that does not end fails here instead of in the set's allocation"""
    code = "import sys; sys.path.insert(0, sys.argv[1]); import dashing2_amd as D; print(int(D.sparse_bin_geometry(int(sys.argv[2]))['binned_ok']))"
    r = subprocess.run([sys.executable, "-c", code, ROOT, str(N)], capture_output=True, text=True, timeout=60, env=dict(os.environ))
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip() == "1"


@pytest.mark.parametrize("N,binned", [(1_277_952, True), (1_300_000, False)])
def test_k2_sparse_path_at_the_bin_geometry_limit(gpu_ctx, d2g, oracle, monkeypatch, N, binned):
    """1 277 952 sketches: 39 936 bands of 32 rows, one chunk of 2^21 columns -- every bin the composer's LDS can hold; the binned form is
    forced and runs.  1 300 000: the bands alone are too many bins, and the forced form falls back to entry by entry.  S = 32, families of 32
    that keep at least half of their parent's registers, one chance collision per sketch (a list of tens of millions of entries: families of
    150 with members that keep almost nothing overflow the list's 2^27 entries at this N); three row ranges (64 rows: first rows, a band seam
    in the middle, last rows) against the direct kernel and the oracle."""
    import torch
    assert _geometry_in_a_child(N) == binned
    monkeypatch.setenv("D2G_SP_REMEMBER", "0")
    monkeypatch.setenv("D2G_SP_LIST_FORM", "2")
    S = 32
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    fam = synth.synthetic_registers(N, S, nclusters=N // 32, seed=17, share_lo=0.5)
    bits = np.ascontiguousarray(_one_collision(fam, seed=18)).view(np.uint64)
    del fam
    m = bits.view(np.float64)
    lut_np = _lut(d2g, S)
    t_dev = torch.from_numpy(bits.view(np.int64)).to(dev)
    cs = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_BITSLICE, stream=stream)
    dr = gpu_ctx.cmp_set_dev(t_dev.data_ptr(), N, S, algo=d2g.CMP_DIRECT, stream=stream)
    mid = N // 2 - N // 2 % 32
    ranges = ((0, 20), (mid - 5, mid + 19), (N - 20, N))
    off = lambda i, r0: (i - r0) * (N - 1) - (i - r0) * (i + r0 - 1) // 2       # offset of row i inside rows [r0, ...)
    for r0, r1 in ranges:
        got = cs.eqcount_ut(r0, r1)
        info, detail = cs.sparse_info(), cs.sparse_detail()
        assert info["tiles_and_pair_list"] and not info["dense_kernel_ran"] and info["pairs_listed"] > 0, (r0, info)
        assert detail["binned"] == binned and detail["bin_cshift"] == 21, detail
        want = dr.eqcount_ut(r0, r1)
        np.testing.assert_array_equal(got, want, err_msg=f"rows {r0}:{r1}")
        _oracle_rows(oracle, m, [i for i in range(r0, r1) if i < N - 1], lambda i: got[off(i, r0):off(i + 1, r0)], f"N={N} rows {r0}:{r1}")
        fgot = cs.lut_ut(lut_np, r0, r1)
        np.testing.assert_array_equal(fgot.view(np.uint32), lut_np[want].view(np.uint32), err_msg=f"table rows {r0}:{r1}")
    cs.close()
    dr.close()
