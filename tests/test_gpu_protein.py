"""Amino-acid k-mers on the GPU (K1a: the AA mode of the shared walker, d2g_kmers.h) against the model of tests/protein_ref.py.
First the emitted multiset itself -- Sketcher.run_sets with counts is the exact (k-mer, occurrences) table of every genome -- at every
seam of the decomposition and at the exact counter's key-width seam; then every consumer against the helpers that turn (masked key,
count) pairs into expected registers, counts, sets and BagMinHash signatures.  Every comparison is exact."""
import numpy as np
import pytest

import oph_kmers_ref as R
import oph_mincount_ref as Q
import protein_ref as P

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -5                                          # D2G_ERR_INVALID, D2G_ERR_UNSUPPORTED (include/d2g.h)

# emissions of a run: around a dword's 4 residues, a window's 16, a lane's chunk (64), two chunks, one 256-lane pass (16384) and one
# workgroup (65536)
SEAMS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 16383, 16384, 16385, 65535, 65536, 65537)
AK = [(P.PROTEIN20, 1), (P.PROTEIN20, 5), (P.PROTEIN20, 14), (P.PROTEIN_14, 16), (P.PROTEIN_3BIT, 21), (P.PROTEIN_6, 24)]
WIDTH = [(P.PROTEIN20, 7), (P.PROTEIN20, 8), (P.PROTEIN_3BIT, 10), (P.PROTEIN_3BIT, 11), (P.PROTEIN_6, 12), (P.PROTEIN_6, 13)]


def _ids(pairs):
    return [f"A{P.size(a)}k{k}" for a, k in pairs]


def _pack(d2g, fastas, k, alphabet):
    sp = d2g.SeqPack(k, alphabet)
    for f in fastas:
        sp.add_fastx(f)
    return sp


def _sketcher(ctx, alphabet):
    sk = ctx.sketcher()
    sk.set_alphabet(alphabet)
    return sk


def _check_sets(sk, sp, expected, thr=0.0):
    """run_sets == the model's (masked key, count) pairs above the threshold, genome by genome"""
    keys, counts, off, cards = sk.run_sets(sp, canon=False, count_threshold=thr)
    assert len(off) == len(expected) + 1
    for g, (ek, ec) in enumerate(expected):
        keep = ec.astype(np.float64) > thr
        ek, ec = ek[keep], ec[keep]
        lo, hi = int(off[g]), int(off[g + 1])
        assert np.array_equal(keys[lo:hi], ek) and np.array_equal(counts[lo:hi], ec), (g, hi - lo, ek.size)
        assert cards[g].tolist() == [ek.size, int(ec.sum())]


@pytest.mark.parametrize("alphabet,k", AK, ids=_ids(AK))
def test_emitted_multiset_at_every_seam(d2g, gpu_ctx, alphabet, k):
    """one genome per seam: a run of k + r residues (r = 0..3 in turn, so that the seam's run starts at every byte offset of a dword),
    an invalid letter, then a single random run of E + k - 1 residues; a genome with no run; a genome that is the highest code only"""
    A = P.size(alphabet)
    top_letter = P.GROUPS[alphabet].split()[-1][-1].encode()
    fastas = []
    for i, E in enumerate(SEAMS):
        fastas.append(P.fa(P.random_protein(2000 + i, k + i % 4) + b"X" + P.random_protein(1000 + i, E + k - 1)))
    fastas.append(P.fa(P.random_protein(5, k - 1) + b"*" + P.random_protein(6, k - 1), "norun"))
    Etop = 1000
    fastas.append(P.fa(top_letter * (Etop + k - 1), "top"))
    sp = _pack(d2g, fastas, k, alphabet)
    starts = sp.arrays()[1]
    assert {int(s) % 4 for s in starts[1:2 * len(SEAMS):2]} == {0, 1, 2, 3}     # the seam runs really start at all four byte offsets
    assert [sp.nkmers(g) for g in range(len(fastas))] == [E + 1 + i % 4 for i, E in enumerate(SEAMS)] + [0, Etop]
    expected = [P.fasta_counts(f, k, alphabet) for f in fastas]
    assert expected[-2][0].size == 0
    tk, tc = P.masked_counts(np.array([A ** k - 1], np.uint64))
    assert np.array_equal(expected[-1][0], tk) and expected[-1][1].tolist() == [Etop]
    sk = _sketcher(gpu_ctx, alphabet)
    _check_sets(sk, sp, expected)
    sk.close()


def _width_inputs(alphabet):
    rnd = P.random_protein(77 + alphabet, 5000)
    unit = P.random_protein(78 + alphabet, 37)
    rep = (unit * 200)[:4000] + b"X" + rnd[:1500] + b"x" + rnd[:1500]      # heavy repetition: a unit of 37, and 1500 residues twice
    return [P.fa(rnd, "random"), P.fa(rep, "repeats")]


@pytest.mark.parametrize("alphabet,k", WIDTH, ids=_ids(WIDTH))
def test_k3_key_width_seam(d2g, gpu_ctx, oracle, alphabet, k, monkeypatch):
    """31/35, 30/33 and 32/34 key bits: on either side of the 32 bits a stored word of the compact counter holds.  The exact sets,
    the distinct count and BagMinHash, on the generic path and on the compact one"""
    S = 64
    fastas = _width_inputs(alphabet)
    expected = [P.fasta_counts(f, k, alphabet) for f in fastas]
    assert int(expected[1][1].max()) > 50 and (d2g.key_bits(k, alphabet) > 32) == (k in (8, 11, 13))
    esig = [oracle.bmh_from_weighted(ek, ec.astype(np.float64), S) for ek, ec in expected]
    sp = _pack(d2g, fastas, k, alphabet)
    sk = _sketcher(gpu_ctx, alphabet)
    try:
        for compact in (False, True):
            if compact:
                monkeypatch.setenv("D2G_K3_COMPACT", "1")
                gpu_ctx.reload_tuning()
            _check_sets(sk, sp, expected)
            assert sk.run_distinct(sp, canon=False).tolist() == [ek.size for ek, _ in expected]
            sig, tw = sk.run_bmh(sp, S, canon=False)
            for g, (es, etw) in enumerate(esig):
                assert tw[g] == etw and np.array_equal(sig[g].view(np.uint64), es.view(np.uint64)), (compact, g)
    finally:                                                           # whatever failed: the shared context leaves the compact path
        monkeypatch.delenv("D2G_K3_COMPACT", raising=False)
        gpu_ctx.reload_tuning()
        sk.close()


# ---- every consumer ---------------------------------------------------------------------------------------------------------------
CONS_A, CONS_K = P.PROTEIN20, 5
_CONS = {}


def _consumers():
    """a handful of random proteomes of <= 20 000 residues (one of them twice over, so that counts pass 1), one with many invalid
    letters, one without a k-mer"""
    if not _CONS:
        p0 = P.random_protein(300, 20000)
        p1 = P.random_protein(301, 7001)
        p2 = p1[:3000] + b"\n>again\n" + p1[:3000] + b"\n>more\n" + p1[100:600]      # records: no k-mer that p1 lacks
        noisy = bytearray(P.random_protein(302, 9000))
        rng = np.random.default_rng(303)
        for i in rng.integers(0, len(noisy), 1200):
            noisy[i] = ord("XBZJUO*-xz"[i % 10])
        fastas = [P.fa(p0, "p0"), P.fa(p1, "p1"), P.fa(p2, "p2"), P.fa(bytes(noisy), "noisy"), P.fa(b"ACDE", "tiny")]
        _CONS["fastas"] = fastas
        _CONS["counts"] = [P.fasta_counts(f, CONS_K, CONS_A) for f in fastas]
    return _CONS["fastas"], _CONS["counts"]


def _expected_k1(kc, m, c=0, drop=None):
    regs, counts = [], []
    for keys, cnts in kc:
        if drop is not None:
            keep = ~np.isin(keys, drop)
            keys, cnts = keys[keep], cnts[keep]
        r, n = Q.closed_form(keys, cnts, m, c)
        regs.append(r); counts.append(n)
    return np.stack(regs), np.stack(counts)


class DevArrays:
    """packed stream, registers and counts of one batch in device memory under a plan of the alphabet, the outputs pre-set to a pattern"""

    def __init__(self, ctx, sp, m, fill=0xAB):
        self.ctx = ctx
        packed, rs, rl, go = sp.arrays()
        self.n, self.m = go.size - 1, m
        self.plan = ctx.oph_plan(rs, rl, go, sp.k, alphabet=sp.alphabet)
        self.packed = ctx.malloc(max(packed.size, 4))
        ctx.h2d(self.packed, packed)
        self.regs, self.counts = ctx.malloc(self.n * m * 8), ctx.malloc(self.n * m * 4)
        ctx.h2d(self.regs, np.full(self.n * m * 8, fill, np.uint8))
        ctx.h2d(self.counts, np.full(self.n * m * 4, fill, np.uint8))

    def read(self):
        regs, counts = np.empty((self.n, self.m), np.uint64), np.empty((self.n, self.m), np.uint32)
        self.ctx.sync()
        self.ctx.d2h(regs, self.regs)
        self.ctx.d2h(counts, self.counts)
        return regs, counts

    def close(self):
        for p in (self.packed, self.regs, self.counts):
            self.ctx.free(p)
        self.plan.close()


@pytest.mark.parametrize("S", [64, 1000, 1024])
def test_every_consumer(d2g, gpu_ctx, oracle, S):
    fastas, kc = _consumers()
    m = d2g.oph_m(S)
    assert kc[4][0].size == 0 and int(kc[2][1].max()) >= 2 and len(kc[3][0]) < 9000 - 1200
    sp = _pack(d2g, fastas, CONS_K, CONS_A)
    sk = _sketcher(gpu_ctx, CONS_A)
    # K1 and K1b
    eregs, ecounts = _expected_k1(kc, m)
    assert (eregs[4] == R.M64).all() and (eregs[0] != R.M64).any()
    regs, counts = sk.run_counts(sp, S, canon=False)
    assert np.array_equal(regs, eregs) and np.array_equal(counts, ecounts)
    assert np.array_equal(sk.run(sp, S, canon=False), eregs)
    xm = 0x9E3779B97F4A7C15                                             # a seed's xormask: the key is masked as a DNA k-mer is
    kx = [P.fasta_counts(f, CONS_K, CONS_A, xm) for f in fastas]
    assert np.array_equal(sk.run(sp, S, canon=False, xormask=xm), _expected_k1(kx, m)[0])
    # -m c
    for c in (2, 3):
        er, ec = _expected_k1(kc, m, c)
        regs, counts = sk.run_mincount(sp, S, c, canon=False, counts=True)
        assert np.array_equal(regs, er) and np.array_equal(counts, ec), c
    # --multiset
    sig, tw = sk.run_bmh(sp, S, canon=False)
    for g, (ek, ec) in enumerate(kc):
        es, etw = oracle.bmh_from_weighted(ek, ec.astype(np.float64), S)
        assert tw[g] == etw and np.array_equal(sig[g].view(np.uint64), es.view(np.uint64)), g
    # --set / --countdict with a threshold
    _check_sets(sk, sp, kc, thr=1.0)
    assert sk.run_distinct(sp, canon=False).tolist() == [ek.size for ek, _ in kc]
    # the plan + _dev forms once each
    dv = DevArrays(gpu_ctx, sp, m)
    assert dv.plan.nkmers == sum(int(c.sum()) for _, c in kc)
    gpu_ctx.oph_sketch_dev(dv.plan, dv.packed, S, dv.regs, canon=False)
    gpu_ctx.oph_count_dev(dv.plan, dv.packed, S, dv.regs, dv.counts, canon=False)
    dregs, dcounts = dv.read()
    assert np.array_equal(dregs, eregs) and np.array_equal(dcounts, ecounts)
    gpu_ctx.oph_sketch_mincount_dev(dv.plan, dv.packed, S, 2, dv.regs, canon=False)
    assert np.array_equal(dv.read()[0], _expected_k1(kc, m, 2)[0])
    if S == 64:
        tw_dev = gpu_ctx.malloc(dv.n * 8)
        sig_dev = gpu_ctx.malloc(dv.n * S * 8)
        gpu_ctx.bmh_sketch_dev(dv.plan, dv.packed, S, sig_dev, tw_dev, canon=False)
        dsig, dtw = np.empty((dv.n, S), np.float64), np.empty(dv.n, np.float64)
        gpu_ctx.sync()
        gpu_ctx.d2h(dsig, sig_dev)
        gpu_ctx.d2h(dtw, tw_dev)
        assert np.array_equal(dsig.view(np.uint64), sig.view(np.uint64)) and np.array_equal(dtw, tw)
        gpu_ctx.free(tw_dev)
        gpu_ctx.free(sig_dev)
    # a plan under a protein alphabet takes no canon
    with pytest.raises(d2g.D2GError) as e:
        gpu_ctx.oph_sketch_dev(dv.plan, dv.packed, S, dv.regs, canon=True)
    assert e.value.status == INVALID and "canon" in str(e.value)
    dv.close()
    sk.close()


@pytest.mark.parametrize("S", [64, 1000, 1024])
def test_filter(d2g, gpu_ctx, oracle, S):
    """a filter built from one of the inputs: that input's own k-mers vanish everywhere, and an input filtered away entirely is empty"""
    fastas, kc = _consumers()
    m = d2g.oph_m(S)
    fsp = _pack(d2g, [fastas[1]], CONS_K, CONS_A)
    f = gpu_ctx.kmer_filter(fsp, canon=False)
    fkeys, fcnt = kc[1]
    assert f.info()[:2] == (int(fcnt.sum()), fkeys.size)
    raw = np.unique(P.fasta_keys(fastas[1], CONS_K, CONS_A))
    asked = np.concatenate([raw[:50], raw[:50] + np.uint64(20 ** 5)])   # keys of the input, and values no 5-mer of 20 letters has
    assert f.contains(asked).tolist() == [1] * 50 + [0] * 50
    sp = _pack(d2g, fastas, CONS_K, CONS_A)
    sk = _sketcher(gpu_ctx, CONS_A)
    sk.set_filter(f)
    eregs, ecounts = _expected_k1(kc, m, drop=fkeys)
    assert (eregs[1] == R.M64).all() and (eregs[2] == R.M64).all() and (eregs[0] != R.M64).any()      # p2 is made of pieces of p1
    assert np.isin(kc[0][0], fkeys).any() and not np.isin(kc[0][0], fkeys).all()                      # p0 shares a few k-mers with p1 by chance
    regs, counts = sk.run_counts(sp, S, canon=False)
    assert np.array_equal(regs, eregs) and np.array_equal(counts, ecounts)
    kept = [(ek[~np.isin(ek, fkeys)], ec[~np.isin(ek, fkeys)]) for ek, ec in kc]
    _check_sets(sk, sp, kept)
    assert sk.run_distinct(sp, canon=False).tolist() == [ek.size for ek, _ in kept]
    er2, ec2 = _expected_k1(kc, m, 2, drop=fkeys)
    regs, counts = sk.run_mincount(sp, S, 2, canon=False, counts=True)
    assert np.array_equal(regs, er2) and np.array_equal(counts, ec2)
    sig, tw = sk.run_bmh(sp, 64, canon=False)
    for g, (ek, ec) in enumerate(kept):
        es, etw = oracle.bmh_from_weighted(ek, ec.astype(np.float64), 64)
        assert tw[g] == etw and np.array_equal(sig[g].view(np.uint64), es.view(np.uint64)), g
    # the plan form: filter built from a plan and a device stream, attached to a plan
    dvf = DevArrays(gpu_ctx, fsp, m)
    f2 = gpu_ctx.kmer_filter_dev(dvf.plan, dvf.packed, canon=False)
    assert f2.info()[:2] == f.info()[:2]
    dv = DevArrays(gpu_ctx, sp, m)
    dv.plan.set_filter(f2)
    gpu_ctx.oph_sketch_dev(dv.plan, dv.packed, S, dv.regs, canon=False)
    assert np.array_equal(dv.read()[0], eregs)
    # a filter of another alphabet, and a DNA filter, are refused before anything is written
    for other in (P.PROTEIN_6, P.DNA):
        osp = d2g.SeqPack(CONS_K, other)
        osp.add_sequence(b"ACGTACGTACGTGGGACT")
        fo = gpu_ctx.kmer_filter(osp, canon=False)
        sk.set_filter(fo)
        for call in (lambda: sk.run(sp, S, canon=False), lambda: sk.run_bmh(sp, S, canon=False), lambda: sk.run_distinct(sp, canon=False)):
            with pytest.raises(d2g.D2GError) as e:
                call()
            assert e.value.status == INVALID and "another alphabet" in str(e.value)
        dv.plan.set_filter(fo)
        gpu_ctx.h2d(dv.regs, np.full(dv.n * m * 8, 0xAB, np.uint8))
        with pytest.raises(d2g.D2GError) as e:
            gpu_ctx.oph_sketch_dev(dv.plan, dv.packed, S, dv.regs, canon=False)
        assert e.value.status == INVALID and "another alphabet" in str(e.value) and (dv.read()[0] == 0xABABABABABABABAB).all()
        sk.set_filter(None)
        dv.plan.set_filter(None)
        fo.close()
    # ... and the protein filter on a DNA sketcher
    dna = d2g.SeqPack(CONS_K)
    dna.add_sequence(b"ACGTACGTACGTGGGACT")
    sk.set_alphabet(P.DNA)
    sk.set_filter(f)
    with pytest.raises(d2g.D2GError) as e:
        sk.run(dna, S, canon=False)
    assert e.value.status == INVALID and "another alphabet" in str(e.value)
    sk.set_filter(None)
    dv.close()
    dvf.close()
    f2.close()
    sk.close()
    f.close()


def test_by_record(d2g, gpu_ctx):
    """300 records of 20-400 residues, some shorter than k: one genome per record"""
    alphabet, k, S = P.PROTEIN20, 5, 64
    rng = np.random.default_rng(11)
    recs = []
    for i in range(300):
        n = int(rng.integers(20, 401)) if i % 17 else int(rng.integers(0, k))
        recs.append(P.fa(P.random_protein(4000 + i, n), f"r{i}"))
    fasta = b"".join(recs)
    sp = d2g.SeqPack(k, alphabet)
    sp.add_fastx_by_record(fasta)
    assert sp.ngenomes == 300 and [sp.name(g) for g in (0, 17, 299)] == ["r0", "r17", "r299"]
    kc = [P.fasta_counts(r, k, alphabet) for r in recs]
    assert sum(1 for ek, _ in kc if ek.size == 0) == 18
    sk = _sketcher(gpu_ctx, alphabet)
    eregs, ecounts = _expected_k1(kc, d2g.oph_m(S))
    regs, counts = sk.run_counts(sp, S, canon=False)
    assert np.array_equal(regs, eregs) and np.array_equal(counts, ecounts)
    _check_sets(sk, sp, kc)
    sk.close()


def test_dna_is_untouched_by_a_protein_sketcher_switched_back(d2g, gpu_ctx, oracle):
    from dashing2_amd import synth
    fa = synth.fasta_bytes("g", synth.random_genome(3, 30000))
    sp = d2g.SeqPack(31)
    sp.add_fastx(fa)
    sk = _sketcher(gpu_ctx, P.PROTEIN20)
    sk.set_alphabet(P.DNA)
    assert np.array_equal(sk.run(sp, 1024)[0], oracle.sketch_buffer(fa, k=31, S=1024)[0])
    sk.close()


def test_refusals(d2g, gpu_ctx):
    """the five library refusals return their status, with their text, before anything runs"""
    alphabet, k, S = P.PROTEIN20, 5, 64
    sp = _pack(d2g, [P.fa(P.random_protein(1, 500))], k, alphabet)
    packed, rs, rl, go = sp.arrays()
    sk = _sketcher(gpu_ctx, alphabet)
    # canon != 0
    for call in (lambda: sk.run(sp, S, canon=True), lambda: sk.run_counts(sp, S, canon=True), lambda: sk.run_bmh(sp, S, canon=True),
                 lambda: sk.run_sets(sp, canon=True), lambda: sk.run_distinct(sp, canon=True), lambda: sk.run_mincount(sp, S, 2, canon=True)):
        with pytest.raises(d2g.D2GError) as e:
            call()
        assert e.value.status == INVALID and "canon" in str(e.value)
    # k beyond the alphabet: a stream the packer would not make, handed over as arrays
    with pytest.raises(d2g.D2GError) as e:
        sk.run((packed, rs, rl, go, 15), S, canon=False)
    assert e.value.status == UNSUPPORTED and "largest exact k" in str(e.value)
    with pytest.raises(d2g.D2GError) as e:
        gpu_ctx.oph_plan(rs, rl, go, 15, alphabet=alphabet)
    assert e.value.status == UNSUPPORTED
    gpu_ctx.oph_plan(rs, rl, go, 14, alphabet=alphabet).close()
    # a window together with an alphabet
    sk.set_window(k + 3)
    with pytest.raises(d2g.D2GError) as e:
        sk.run(sp, S, canon=False)
    assert e.value.status == UNSUPPORTED and "window" in str(e.value)
    sk.set_window(k)                                                   # w <= k is no window
    assert sk.run(sp, S, canon=False).shape == (1, S)
    sk.set_window(0)
    # the device FASTA parser is a DNA parser
    with pytest.raises(d2g.D2GError) as e:
        sk.ingest_fasta([b">g\nACGTACGTACGTACGTACGT\n"], k)
    assert e.value.status == UNSUPPORTED and "DNA" in str(e.value)
    # the screen
    keys = np.arange(1, 9, dtype=np.uint64).reshape(1, 8)
    sc = gpu_ctx.screen(keys, k, canon=False, nrows=1)
    with pytest.raises(d2g.D2GError) as e:
        sk.run_screen(sp, sc, [0], canon=False)
    assert e.value.status == UNSUPPORTED and "screen" in str(e.value)
    plan = gpu_ctx.oph_plan(rs, rl, go, k, alphabet=alphabet)
    dev = gpu_ctx.malloc(packed.size)
    gpu_ctx.h2d(dev, packed)
    with pytest.raises(d2g.D2GError) as e:
        sc.add_dev(plan, dev, [0])
    assert e.value.status == UNSUPPORTED and "screen" in str(e.value)
    assert sc.fed(0) == 0
    gpu_ctx.free(dev)
    plan.close()
    sc.close()
    # an unknown alphabet
    with pytest.raises(d2g.D2GError) as e:
        sk.set_alphabet(1)
    assert e.value.status == INVALID
    # and the sketcher still works
    assert np.array_equal(sk.run(sp, S, canon=False)[0], _expected_k1([P.fasta_counts(P.fa(P.random_protein(1, 500)), k, alphabet)], S)[0][0])
    sk.close()
