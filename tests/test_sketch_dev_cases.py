"""sketch_dev_cases.py held to what it promises, without a GPU: the layouts are what their docstrings say, and the expected values
of every layout agree bit for bit three ways -- the builder's (NumPy-rolled k-mers, oph_kmers_ref.closed_form and the oracle's heap
algorithm over explicit keys), the pure-Python enumerator of k3_seam_cases over the runs as ACGT strings, and the oracle's own walk
(d2o_sketch_buffer, d2o_bmh_sketch_buffer) over the runs rendered as FASTA."""
import numpy as np
import pytest

import k3_seam_cases as C
import oph_kmers_ref as R
import sketch_dev_cases as V

INF_BITS = np.float64(np.inf).view(np.uint64)


def three_ways(oracle, lay, k, canon, xormask, S, bmh=()):
    """bmh: (S3, threshold) pairs"""
    regs, cnts = lay.oph(k, canon, xormask, S)
    kc = lay.key_counts(k, canon, xormask)
    assert [nk for _, _, nk in kc] == lay.nkmers(k)
    for g in range(lay.n):
        what = f"{lay} genome {g} k {k} canon {canon} xormask {xormask:#x}"
        recs = lay.records(g)
        assert [len(r) for r in recs] == [int(lay.run_len[r]) for r in lay.runs_of(g)]
        keys, counts, nk = C.key_counts(tuple(recs), k, canon, xormask)        # the pure-Python enumerator
        assert nk == kc[g][2], what
        np.testing.assert_array_equal(keys, kc[g][0], err_msg=what + " (keys)")
        np.testing.assert_array_equal(counts, kc[g][1], err_msg=what + " (counts)")
        eregs, ecnts = R.genome_closed_form(recs, k, canon, xormask, S)
        np.testing.assert_array_equal(eregs, regs[g], err_msg=what + " (closed form, registers)")
        np.testing.assert_array_equal(ecnts, cnts[g], err_msg=what + " (closed form, counts)")
        fa = lay.fasta(g)
        oregs, _, _, onk = oracle.sketch_buffer(fa, k=k, canon=canon, xormask=xormask, S=S)
        assert onk == nk, what
        np.testing.assert_array_equal(oregs, regs[g], err_msg=what + " (oracle over the FASTA)")
        for S3, thr in bmh:
            sig, tw = lay.bmh(k, canon, xormask, S3, thr)
            osig, otw, _ = oracle.bmh_sketch_buffer(fa, k, S3, canon=canon, xormask=xormask, count_threshold=thr)
            assert otw == tw[g], what + f" (total weight, S {S3} threshold {thr})"
            np.testing.assert_array_equal(osig.view(np.uint64), sig[g].view(np.uint64), err_msg=what + f" (BagMinHash, S {S3} threshold {thr})")


def assert_random_between_runs(lay, min_gaps):
    gaps = [(lo, hi) for lo, hi in lay.gaps() if hi - lo >= 8]
    assert len(gaps) >= min_gaps
    for lo, hi in gaps:
        assert np.unique(lay.packed[lo:hi]).size > min(hi - lo, 256) // 4, f"{lay}: bytes {lo}..{hi} do not look random"
    assert lay.gaps()[-1][1] == lay.packed.size and lay.gaps()[-1][1] - lay.gaps()[-1][0] >= V.PAD


# ---------------------------------------------------------------- the packing and the roller
def test_decode_and_roll_on_a_hand_made_buffer():
    """base p = bits [2 (p % 4), +2) of byte p / 4: 0xE4 = 11 10 01 00 is ACGT, 0x1B is TGCA"""
    packed = np.array([0xE4, 0x1B, 0x00, 0xFF], np.uint8)
    codes = V.decode(packed)
    assert codes.tolist() == [0, 1, 2, 3, 3, 2, 1, 0, 0, 0, 0, 0, 3, 3, 3, 3]
    for k in (1, 3, 8, 15, 16):
        for canon in (True, False):
            rec = "ACGTTGCAAAAATTTT"
            assert V.kmers_np(codes, k, canon).tolist() == C.kmers_of([rec], k, canon)
    assert V.kmers_np(codes[:5], 6, True).size == 0
    rng = np.random.default_rng(5)
    codes = rng.integers(0, 4, 200, dtype=np.uint8)
    rec = "".join("ACGT"[c] for c in codes)
    for k in (31, 32):
        for canon in (True, False):
            assert V.kmers_np(codes, k, canon).tolist() == C.kmers_of([rec], k, canon)


def test_slots_is_the_benchmarks_layout():
    lens = [100, 257, 31]
    (packed, rs, rl, go), codes = V.slots(9, lens, 128)
    assert packed.size == 3 * 128 + 64 and packed.dtype == np.uint8
    assert rs.tolist() == [0, 512, 1024] and rl.tolist() == lens and go.tolist() == [0, 1, 2, 3]
    assert [c.size for c in codes] == lens
    assert np.array_equal(codes[1], V.decode(packed)[512:512 + 257])
    assert np.array_equal(V.slots(9, lens, 128)[0][0], packed) and not np.array_equal(V.slots(10, lens, 128)[0][0], packed)
    assert V.slot_bytes_for(100) == 64 and V.slot_bytes_for(256) == 64 and V.slot_bytes_for(257) == 128


# ---------------------------------------------------------------- a
@pytest.mark.parametrize("k,canon,xormask", [(31, True, V.SEEDED), (32, False, 0)])
def test_seam_genomes_land_on_the_plans_seams(oracle, k, canon, xormask):
    lay = V.seams(k)
    assert tuple(lay.nkmers(k)) == V.SEAM_KMERS == (1, 63, 64, 65, 65536, 65537, 131073)
    chunks = [-(-nk // V.CHUNK) for nk in lay.nkmers(k)]
    assert chunks == [1, 1, 1, 2, 1024, 1025, 2049]                     # workgroups: 1 1 1 1 1 2 3
    assert lay.run_start.tolist() == [g * lay.slot_bytes * 4 for g in range(7)] and lay.slot_bytes % 64 == 0
    assert_random_between_runs(lay, 7)
    other = V.seams(k, 3101)
    assert np.array_equal(other.run_len, lay.run_len) and not np.array_equal(other.packed, lay.packed)
    three_ways(oracle, lay, k, canon, xormask, 20000, bmh=[(64, 0.0)])
    m_lds, m_hbm = R.oph_m(16384), R.oph_m(16385)
    assert 8 * m_lds == 128 * 1024 and m_hbm == 16386 and m_hbm & (m_hbm - 1) and R.oph_m(20000) & (R.oph_m(20000) - 1)


def test_seam_genomes_fill_and_leave_registers(oracle):
    """the expected registers are neither all empty nor all full at the sizes of the test, and depend on canon and the mask"""
    lay = V.seams(31)
    for S in V.SEAM_SIZES:
        regs, cnts = lay.oph(31, True, 0, S)
        assert (regs[0] != R.M64).sum() == 1 and cnts[0].sum() == 1
        assert (regs[6] != R.M64).mean() > 0.99 and (regs[3] == R.M64).any()
        assert int(cnts[6].astype(np.int64).sum()) >= (regs[6] != R.M64).sum()
    a = lay.oph(31, True, 0, 1024)[0]
    assert not np.array_equal(a, lay.oph(31, False, 0, 1024)[0]) and not np.array_equal(a, lay.oph(31, True, V.SEEDED, 1024)[0])


# ---------------------------------------------------------------- the variants
@pytest.mark.parametrize("which", V.VARIANTS)
def test_variants_plant_what_they_say(oracle, which):
    k = 31
    lay = V.variant(which, k)
    assert np.array_equal(lay.packed, V.variant("unaligned", k).packed)    # the same bytes under every table
    rs, rl, go = (a.astype(np.int64) for a in lay.tables())
    if which == "unaligned":
        assert (rs % 4 != 0).all() and (rs % 16 != 0).all() and lay.nkmers(k)[2] == 64
    if which == "two_runs":
        assert (np.diff(go) == 2).all() and all(rs[r + 1] > rs[r] + rl[r] for r in range(0, 8, 2))      # a gap inside every genome
        c0, c1 = -(-(rl[0] - k + 1) // 64), -(-(rl[1] - k + 1) // 64)
        assert c0 < 1024 < c0 + c1                                       # genome 0's first workgroup ends inside its second run
        assert lay.nkmers(k)[2] == 1 + 4000 - k + 1
    if which == "descending":
        fwd = V.variant("two_runs", k)
        assert (np.diff(rs) < 0).all() and np.array_equal(rs[::-1], fwd.run_start.astype(np.int64))
        for g in range(4):                                               # genome g here is genome 3 - g there, its runs swapped
            a, b = lay.key_counts(k, True, 0)[g], fwd.key_counts(k, True, 0)[3 - g]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    if which == "overlap":
        assert rs[0] < rs[1] < rs[0] + rl[0] and rs[1] <= rs[2] and rs[2] + rl[2] <= rs[1] + rl[1]
        kc = lay.key_counts(k, True, 0)
        assert np.isin(kc[2][0], kc[1][0]).all() and np.isin(kc[1][0], kc[0][0]).any()
        assert int((kc[3][1] == 2).sum()) == 3000 - k + 1 and int(kc[3][1].max()) == 2
        sig, tw = lay.bmh(21, True, 0, 64, 1.0)
        assert tw[3] == 2.0 * (3000 - 21 + 1) and np.isfinite(sig[3]).all()
        assert (tw[:3] == 0).all() and (sig[:3].view(np.uint64) == INF_BITS).all()
    if which == "no_run":
        assert go.tolist() == [0, 1, 1, 2, 2] and lay.nkmers(k) == [6000 - k + 1, 0, 7000 - k + 1, 0]
        regs, cnts = lay.oph(k, True, 0, 1000)
        assert (regs[[1, 3]] == R.M64).all() and not cnts[[1, 3]].any()
    assert_random_between_runs(lay, 2)
    three_ways(oracle, lay, k, True, V.SEEDED, 1000)
    three_ways(oracle, lay, 21, True, 0, 1024, bmh=[(64, 0.0), (64, 1.0)])


# ---------------------------------------------------------------- b, d, e, f
def test_reuse_buffers_share_tables_and_nothing_else(oracle):
    lays = [V.reuse_buffer(i) for i in range(3)]
    for lay in lays[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(lay.tables(), lays[0].tables()))
        assert not np.array_equal(lay.packed, lays[0].packed)
    lay = lays[0]
    rs, rl, go = lay.head(3)
    assert rs.tolist() == [0, lay.slot_bytes * 4, lay.slot_bytes * 8] and go.tolist() == [0, 1, 2, 3]
    assert np.array_equal(lay.head(3, 3)[1], lay.run_len[3:])                  # the same plan fits at slot 3
    regs = lay.oph(31, True, 0, 1000)[0]
    assert all(not np.array_equal(regs[0], regs[g]) for g in range(1, 6))      # a wrong base pointer or row shows
    three_ways(oracle, lay, 31, True, 0, 1000)
    three_ways(oracle, lays[1], 32, False, V.SEEDED, 1024)


def test_multiset_inputs(oracle):
    lay = V.multiset_slots()
    assert lay.n == 5 and lay.slot_bytes == 2048 and lay.nkmers(21) == [7980] * 5
    assert_random_between_runs(lay, 5)
    assert lay.head(4, 1)[0].tolist() == lay.run_start[:4].tolist()
    three_ways(oracle, lay, 21, True, 0, 1024, bmh=[(64, 0.0), (1000, 0.0), (2048, 1.0)])
    sig, tw = lay.bmh(21, True, 0, 64, 1.0)
    # random 21-mers: none twice, but for genome 4, which holds a 22-base reverse palindrome (a 21-mer and, one base on, its reverse
    # complement): one canonical element of count 2
    assert tw.tolist() == [0, 0, 0, 0, 2] and np.isfinite(sig[4]).all()
    assert (np.delete(sig, 4, axis=0).view(np.uint64) == INF_BITS).all()
    assert (lay.bmh(21, True, 0, 64, 0.0)[1] == 7980.0).all()
    for step, n in ((0, 6), (1, 2), (2, 3)):
        lay = V.k3_reuse_step(step)
        assert lay.n == n
        three_ways(oracle, lay, 21, True, 0, 1024, bmh=[({0: 256, 1: 64, 2: 1000}[step], 0.0)])
    sig, tw = V.k3_reuse_step(1).bmh(21, True, 0, 64, 0.0)
    assert tw.tolist() == [6980.0, 0.0] and (sig[1].view(np.uint64) == INF_BITS).all()


def test_pipeline_batches_sit_on_the_light_seam(oracle):
    """the arithmetic of light_min_kmers, and the other conditions of the pipelined form: one bucket table per genome, no split"""
    gk = V.light_min_kmers(64)
    assert gk == 8153
    const = C.k3_constants()
    buckets = 1 << (-(-gk // const["K3_TARGET"]) - 1).bit_length()
    assert buckets == 8 and gk // buckets <= const["K3_SPLIT_MIN"]
    light, heavy = V.pipeline_batch(True), V.pipeline_batch(False)
    assert light.nkmers(21) == [gk] * 3 and heavy.nkmers(21) == [gk - 1] * 3
    assert C.predicted_light(light.nkmers(21), 64) and not C.predicted_light(heavy.nkmers(21), 64)
    assert np.array_equal(V.pipeline_batch(True, 3601).run_len, light.run_len)
    three_ways(oracle, light, 21, True, 0, 1024, bmh=[(64, 0.0)])


def test_empty_layouts():
    for n in (0, 3):
        lay = V.nothing(n)
        assert lay.n == n and lay.nrun == 0 and lay.packed.size == 64 and lay.nkmers(31) == [0] * n
        regs, cnts = lay.oph(31, True, 0, 1000)
        assert regs.shape == (n, 1000) and (regs == R.M64).all() and not cnts.any()
