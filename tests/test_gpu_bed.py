"""K1i on the GPU, bit-exact against tests/bed_ref.py: interval files -> One-Permutation registers (d2g_interval_oph_sketch / _dev) and
--multiset BagMinHash sketches (d2g_interval_bmh_sketch).  One launch over all the files of FILES per sketch size: line lengths 0, 1,
K1_CHUNK - 1, K1_CHUNK, K1_CHUNK + 1; a file of exactly one workgroup's positions and that +- 1; 70 000 one-base lines (a workgroup
whose lines outnumber its chunks' search depth); one line of 300 000 (several workgroups of one line); overlapping, nested and
duplicate lines; the same coordinates on two chromosomes; chr1 against 1; positions at and above 2^32; an empty file between full ones.
Sketch sizes 1024 (a power of two), 100, 33 (m = 34), 8192 (more LDS than the default limit) and 16 386 / 32 768, whose registers do not fit LDS (both index rules)."""
import numpy as np
import pytest

import bed_ref as R

pytestmark = pytest.mark.gpu

B = R.K1_BLOCK_POSITIONS
C = R.K1_CHUNK


def _bed(lines):
    return b"".join(b"%s\t%d\t%d\n" % (c, a, b) for c, a, b in lines)


FILES = {
    "lengths": _bed([(b"chr1", 10, 10), (b"chr1", 20, 21), (b"chr2", 100, 100 + C - 1), (b"chr3", 7, 7 + C), (b"chr4", 1, 1 + C + 1),
                     (b"chr5", 9, 3)]),
    "block": _bed([(b"chr1", 0, B // 2), (b"chr2", 5, 5 + B // 2)]),
    "block-1": _bed([(b"chr1", 0, B // 2), (b"chr2", 5, 5 + B // 2 - 1)]),
    "block+1": _bed([(b"chr1", 0, B // 2), (b"chr2", 5, 5 + B // 2 + 1)]),
    "empty": b"#nothing here\n\n",
    "ones": _bed([(b"chr7", 3 * i, 3 * i + 1) for i in range(70000)]),
    "long": _bed([(b"chrX", 12345, 12345 + 300000)]),
    "overlaps": _bed([(b"chr1", 0, 500), (b"chr1", 100, 200), (b"chr1", 150, 700), (b"chr1", 100, 200), (b"chr2", 0, 500), (b"chr1", 699, 701)]),
    "chr1": _bed([(b"chr1", 1000, 3000), (b"Chr1", 2500, 2600)]),
    "1": _bed([(b"1", 1000, 3000), (b"1", 2500, 2600)]),
    "high": _bed([(b"chrY", (1 << 32) - 70, (1 << 32) + 70), (b"chrMT", (1 << 40) + 1, (1 << 40) + 200)]),
    "nofile": b"",
}
NAMES = list(FILES)


@pytest.fixture(scope="module")
def tables():
    return R.tables([FILES[n] for n in NAMES])


@pytest.fixture(scope="module")
def plan(gpu_ctx, tables):
    p = gpu_ctx.interval_plan(*tables)
    yield p
    p.close()


_ref = {}


def ref_regs(tables, S):
    if S not in _ref:
        h, a, b, off = tables
        _ref[S] = np.stack([R.oph_registers(list(zip(h[off[f]:off[f + 1]].tolist(), a[off[f]:off[f + 1]].tolist(), b[off[f]:off[f + 1]].tolist())), S)
                            for f in range(len(NAMES))])
        _ref[S].setflags(write=False)
    return _ref[S]


def test_the_plan_counts_every_position(plan, tables):
    h, a, b, off = tables
    assert plan.npositions == int(np.where(b > a, b - a, 0).sum()) == 193 + 3 * B + 70000 + 300000 + 1752 + 2 * 2100 + 339


@pytest.mark.parametrize("S", [1024, 100, 33, 8192, 16386, 32768])
def test_registers_match_the_reference(gpu_ctx, plan, tables, S):
    want = ref_regs(tables, S)
    got = gpu_ctx.interval_oph_sketch(plan, S)
    assert got.shape == want.shape == (len(NAMES), S + (S & 1))
    for f, name in enumerate(NAMES):
        assert np.array_equal(got[f], want[f]), name
    e, n = NAMES.index("empty"), NAMES.index("nofile")
    assert (got[e] == R.M64).all() and (got[n] == R.M64).all()                       # registers stay ~0
    assert np.array_equal(got[NAMES.index("chr1")], got[NAMES.index("1")])            # chr / Chr are trimmed


@pytest.mark.parametrize("S", [1024, 33])
def test_finalisation_matches_the_oracle(d2g, oracle, gpu_ctx, plan, S):
    regs = gpu_ctx.interval_oph_sketch(plan, S)
    sigs, cards = d2g.oph_finalize(regs, S)
    for f, name in enumerate(NAMES):
        esig, ecard = oracle.regs_finalize(regs[f])
        assert np.array_equal(sigs[f].view(np.uint64), esig[:S].view(np.uint64)), name
        assert cards[f] == ecard or (np.isnan(cards[f]) and np.isnan(ecard)), name


@pytest.mark.parametrize("S", [100, 16386])
def test_dev_form_on_a_callers_stream_over_a_prefilled_output(gpu_ctx, plan, tables, S):
    import torch
    m = S + (S & 1)
    side = torch.cuda.Stream()
    out = torch.full((len(NAMES) * m + 16,), 0x1234567, dtype=torch.int64, device="cuda")   # 16 guard words behind the registers
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        gpu_ctx.interval_oph_sketch_dev(plan, S, out.data_ptr(), stream=side.cuda_stream)
        got = out.clone()
    side.synchronize()
    got = got.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:len(NAMES) * m].reshape(len(NAMES), m), ref_regs(tables, S))
    assert (got[len(NAMES) * m:] == 0x1234567).all()


def test_bad_calls_write_nothing(d2g, gpu_ctx, plan):
    h = np.array([1, 2], np.uint64)
    for off in ([0, 3], [0, 2, 1], [1, 2]):
        with pytest.raises(d2g.D2GError):
            gpu_ctx.interval_plan(h, h, h + np.uint64(1), np.array(off, np.uint64))
    with pytest.raises(d2g.D2GError, match="2\\^44"):
        gpu_ctx.interval_plan(h[:1], np.array([0], np.uint64), np.array([(1 << 44) + 1], np.uint64), np.array([0, 1], np.uint64))
    with pytest.raises(d2g.D2GError):
        gpu_ctx.interval_oph_sketch(plan, 0)
    with pytest.raises(d2g.D2GError):
        gpu_ctx.interval_oph_sketch_dev(plan, 64, None)


# ---------------------------------------------------------------- --multiset
def _ms_files():
    h1, h2 = b"chr1", b"chr2"
    depth = [(h1, 10 * d, 400 - 10 * d) for d in range(5)]                           # depths 1 .. 5, nested
    return {
        "depths": _bed(depth),
        "dups": _bed([(h1, 0, 50), (h1, 0, 50), (h2, 0, 50), (h1, 25, 75), (h1, 80, 80), (h1, 90, 60)]),
        "empty": b"",
        "norm": _bed([(h1, 0, 3), (h1, 0, 7), (h1, 2, 3), (h1, 0, 3), (h2, 1, 8), (h1, 5, 6), (h1, 4, 7)]),   # lengths 1, 3, 7: inexact sums
        "norm-reordered": _bed([(h1, 0, 7), (h1, 0, 3), (h1, 0, 3), (h1, 2, 3), (h1, 4, 7), (h2, 1, 8), (h1, 5, 6)]),
        "high": _bed([(h2, (1 << 32) - 40, (1 << 32) + 40), (h2, (1 << 32) - 1, (1 << 32) + 1)]),
        "long": _bed([(h1, 1000, 9000), (h1, 2000, 3000)]),
    }


@pytest.mark.parametrize("normalize", [False, True], ids=["counts", "normalized"])
@pytest.mark.parametrize("S", [64, 100])
def test_multiset_sketches_match_bagminhash_over_the_reference_lists(oracle, gpu_ctx, S, normalize):
    files = _ms_files()
    names = list(files)
    h, a, b, off = R.tables([files[n] for n in names])
    p = gpu_ctx.interval_plan(h, a, b, off)
    try:
        sig, tw = gpu_ctx.interval_bmh_sketch(p, S, normalize=normalize)
        rh, rlo, rhi, rw, roff = p.runs(normalize)
    finally:
        p.close()
    lists = {}
    for f, name in enumerate(names):
        lines = list(zip(h[off[f]:off[f + 1]].tolist(), a[off[f]:off[f + 1]].tolist(), b[off[f]:off[f + 1]].tolist()))
        ids, ws, total = R.multiset_lists(lines, normalize)
        lists[name] = (ids, ws)
        # the sweep's runs, expanded, are the reference's dictionary bit for bit
        r0, r1 = int(roff[f]), int(roff[f + 1])
        gi = np.concatenate([np.uint64(rh[r]) ^ np.arange(int(rlo[r]), int(rhi[r]), dtype=np.uint64) for r in range(r0, r1)] or [np.zeros(0, np.uint64)])
        gw = np.concatenate([np.full(int(rhi[r] - rlo[r]), rw[r]) for r in range(r0, r1)] or [np.zeros(0)])
        assert np.array_equal(gi, ids) and np.array_equal(gw.view(np.uint64), ws.view(np.uint64)), name
        assert tw[f] == total, name
        if ids.size:
            esig, _ = oracle.bmh_from_weighted(ids, ws, S)
            assert np.array_equal(sig[f].view(np.uint64), esig.view(np.uint64)), name
        else:
            assert np.isinf(sig[f]).all() and tw[f] == 0.
    if normalize:                                                                     # the line order shows in the inexact sums
        assert not np.array_equal(lists["norm"][1].view(np.uint64), lists["norm-reordered"][1].view(np.uint64))
        assert np.array_equal(lists["norm"][0], lists["norm-reordered"][0])
    else:
        assert tw[names.index("depths")] == float(sum(400 - 20 * d for d in range(5)))
        assert set(lists["depths"][1].tolist()) == {1.0, 2.0, 3.0, 4.0, 5.0}


def test_multiset_redo_passes_leave_the_registers_unchanged(gpu_ctx, monkeypatch):
    """D2G_K3_GUESS_SCALE=0.001 makes the first guess of every file's bound a thousand times too small, so the walk over the expanded
    interval lists has to repeat its files under raised guesses.  Two files of very different weight -- overlapping and single-position
    lines on two chromosomes; one line of one position -- must give the registers of the default scale bit for bit, which are those
    of BagMinHash over the sweep's runs as explicit weighted sets."""
    S = 64
    h1, h2 = b"chr1", b"chr2"
    h, a, b, off = R.tables([_bed([(h1, 0, 1000), (h1, 500, 1500), (h2, 10, 11)]), _bed([(h1, 0, 1)])])
    p = gpu_ctx.interval_plan(h, a, b, off)
    try:
        sig, tw = gpu_ctx.interval_bmh_sketch(p, S)
        monkeypatch.setenv("D2G_K3_GUESS_SCALE", "0.001")
        rsig, rtw = gpu_ctx.interval_bmh_sketch(p, S)
        monkeypatch.delenv("D2G_K3_GUESS_SCALE")
        rh, rlo, rhi, rw, roff = p.runs()
    finally:
        p.close()
    assert np.array_equal(rsig.view(np.uint64), sig.view(np.uint64)) and np.array_equal(rtw.view(np.uint64), tw.view(np.uint64))
    assert tw.tolist() == [2001.0, 1.0] and np.isfinite(sig).all()
    ids = [np.uint64(rh[r]) ^ np.arange(int(rlo[r]), int(rhi[r]), dtype=np.uint64) for r in range(int(roff[2]))]
    ws = [np.full(int(rhi[r] - rlo[r]), rw[r]) for r in range(int(roff[2]))]
    eoff = np.cumsum([0] + [sum(x.size for x in ids[int(roff[f]):int(roff[f + 1])]) for f in range(2)]).astype(np.uint64)
    esig, etw = gpu_ctx.bmh_from_weighted(np.concatenate(ids), np.concatenate(ws), eoff, S)
    assert np.array_equal(sig.view(np.uint64), esig.view(np.uint64)) and np.array_equal(tw, etw)


def test_interval_kernels_are_timed_under_their_names(gpu_ctx, plan):
    h = np.array([R.chrom_hash(b"1")], np.uint64)
    gpu_ctx.set_timing(True)
    try:
        for which in ("k1i", "k1iexpand", "k1ibmh"):
            gpu_ctx.kernel_ms(which)
        gpu_ctx.interval_oph_sketch(plan, 64)
        assert gpu_ctx.kernel_ms("k1i")[0] == 1 and gpu_ctx.kernel_ms("k1iexpand")[0] == 0
        p = gpu_ctx.interval_plan(h, np.array([0], np.uint64), np.array([100], np.uint64), np.array([0, 1], np.uint64))
        gpu_ctx.interval_bmh_sketch(p, 64)
        p.close()
        assert gpu_ctx.kernel_ms("k1iexpand")[0] == 1 and gpu_ctx.kernel_ms("k1ibmh")[0] == 1 and gpu_ctx.kernel_ms("k1i")[0] == 0
    finally:
        gpu_ctx.set_timing(False)
