"""K1b, the count pass behind sketch -N (k1_oph_count_kernel, d2g_k1.hip), through every entry point that reaches it: registers and
counts compared bit for bit with oph_kmers_ref.closed_form, whose inputs come from a pure-Python k-mer enumerator (genomes are lists
of plain ACGT records, so no parser decides anything).  The registers of the counting forms are also held to d2g_oph_sketch's."""
import functools

import numpy as np
import pytest

import k3_seam_cases as C
import oph_kmers_ref as R

pytestmark = pytest.mark.gpu

M64 = R.M64
K = 15
SEEDED = 0x9E3779B97F4A7C15                                            # a "seeded" xormask: any non-zero value is one
WG_KMERS = 1024 * 64                                                   # K1_BLOCK_CHUNKS chunks of K1_CHUNK k-mers: one workgroup's share


def seqpack(d2g, genomes, k):
    sp = d2g.SeqPack(k)
    for i, g in enumerate(genomes):
        sp.add_fastx(C.fasta(g, f"g{i}"))
    assert [sp.nkmers(i) for i in range(len(genomes))] == [sum(max(0, len(r) - k + 1) for r in g) for g in genomes]
    return sp


def expected(genomes, k, canon, xormask, S):
    m = R.oph_m(S)
    regs, cnts = np.empty((len(genomes), m), np.uint64), np.empty((len(genomes), m), np.uint32)
    for i, g in enumerate(genomes):
        regs[i], cnts[i] = R.genome_closed_form(g, k, canon, xormask, S)
    return regs, cnts


def check(gpu_ctx, d2g, genomes, k, S, canon=True, xormask=0, what=""):
    sp = seqpack(d2g, genomes, k)
    regs, cnts = gpu_ctx.oph_sketch_counts_seqpack(sp, S, canon=canon, xormask=xormask)
    eregs, ecnts = expected(genomes, k, canon, xormask, S)
    np.testing.assert_array_equal(regs, eregs, err_msg=f"{what} S {S} canon {canon}: registers")
    np.testing.assert_array_equal(cnts, ecnts, err_msg=f"{what} S {S} canon {canon}: counts")
    np.testing.assert_array_equal(regs, gpu_ctx.oph_sketch_seqpack(sp, S, canon=canon, xormask=xormask), err_msg="registers of d2g_oph_sketch")
    return regs, cnts


# ---------------------------------------------------------------- one genome over two workgroups
@functools.lru_cache(maxsize=None)
def doubled():
    """the same 35 000-base record twice: 69 972 k-mers in 2 x 547 chunks, so the second workgroup takes the last 70 chunks of the
    second record.  Every k-mer occurs an even number of times"""
    rec = C.random_bases(np.random.default_rng(1501), 35_000)
    return [rec, rec]


@pytest.mark.parametrize("xormask", [0, SEEDED], ids=["mask0", "seeded"])
@pytest.mark.parametrize("canon", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("S", [1, 3, 5, 1000, 1024, 10922, 10923])
def test_two_workgroups_every_sketch_size(gpu_ctx, d2g, S, canon, xormask):
    """m = 2, 4, 6 (not a power of two), 1000, 1024; 10 922 is the last m whose 12 m bytes fit the 128 KB of LDS, 10 923 (m = 10 924)
    the first that compares against HBM and adds globally"""
    g = doubled()
    assert 2 * (len(g[0]) - K + 1) > WG_KMERS
    regs, cnts = check(gpu_ctx, d2g, [g], K, S, canon, xormask, "doubled")
    assert not (cnts & 1).any() and int(cnts.max()) >= 2
    if S >= 1000:
        # registers whose k-mer sits in the part of the record that the SECOND workgroup walks in the second copy: their count of 2 (or
        # more) is one from each workgroup, added in HBM
        masked = R.masked_stream([g[0]], K, canon, xormask)
        first = {}
        for p, x in enumerate(masked):
            first.setdefault(x, p)
        nchunks = -(-len(masked) // 64)
        split = (1024 - nchunks) * 64                                  # k-mer position of the second copy where workgroup 1 begins
        dec = R.decode(regs[0])
        both = [r for r in range(regs.shape[1]) if regs[0, r] != M64 and first[int(dec[r])] >= split]
        assert len(both) >= 10 and all(cnts[0, r] >= 2 for r in both)


# ---------------------------------------------------------------- repeats at chunk and record edges
@functools.lru_cache(maxsize=None)
def edges():
    """one genome: poly-A of K + 1 bases behind 63 others (the same k-mer at k-mer positions 63 and 64 of its run: the last of one
    lane's chunk and the first of the next lane's); a k-mer X at the last position of one record and the first of the next; a record
    shorter than k between two others"""
    rng = np.random.default_rng(1502)
    x = "GATTACAGGCATCGT"
    assert len(x) == K
    r0 = C.random_bases(rng, 62) + "C" + "A" * (K + 1) + "G" + C.random_bases(rng, 150)
    r1 = C.random_bases(rng, 200) + x
    r2 = x + C.random_bases(rng, 120)
    return [r0, r1, "ACGTACG", r2, C.random_bases(rng, 90)], x


@pytest.mark.parametrize("canon", [True, False], ids=["canon", "fwd"])
def test_repeats_at_chunk_and_record_edges(gpu_ctx, d2g, canon):
    recs, x = edges()
    S = 4096                                                           # far more registers than k-mers: the planted ones own theirs
    regs, cnts = check(gpu_ctx, d2g, [recs], K, S, canon, 0, "edges")
    kmers = C.kmers_of([recs[0]], K, canon)
    assert kmers[63] == kmers[64] == 0 and kmers[62] != 0 and kmers[65] != 0
    assert C.kmers_of([recs[1]], K, canon)[-1] == C.kmers_of([recs[3]], K, canon)[0]
    for planted in (0, C.kmers_of([recs[3]], K, canon)[0]):
        i = R.oph_id_int(R.wang64_int(planted))
        r = (i & 0xFFFFFFFF) % S
        assert int(regs[0, r]) == i and int(cnts[0, r]) == 2, hex(planted)


# ---------------------------------------------------------------- canonical counts
def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


@pytest.mark.parametrize("canon", [True, False], ids=["canon", "fwd"])
def test_a_kmer_and_its_reverse_complement(gpu_ctx, d2g, canon):
    """count 2 with canon; without it two elements of count 1 (in two registers, or one register that kept the smaller id)"""
    rng = np.random.default_rng(1503)
    x = "ACGGTCATTGCAGTC"
    recs = [C.random_bases(rng, 80) + x + C.random_bases(rng, 70), C.random_bases(rng, 33) + revcomp(x) + C.random_bases(rng, 50)]
    S = 4096
    regs, cnts = check(gpu_ctx, d2g, [recs], K, S, canon, 0, "revcomp")
    fx = C.kmers_of([x], K, False)[0]
    fr = C.kmers_of([revcomp(x)], K, False)[0]
    if canon:
        i = R.oph_id_int(R.wang64_int(min(fx, fr)))
        assert int(regs[0, (i & 0xFFFFFFFF) % S]) == i and int(cnts[0, (i & 0xFFFFFFFF) % S]) == 2
    else:
        for v in (fx, fr):
            i = R.oph_id_int(R.wang64_int(v))
            assert int(regs[0, (i & 0xFFFFFFFF) % S]) == i and int(cnts[0, (i & 0xFFFFFFFF) % S]) == 1
    assert int(cnts.max()) == (2 if canon else 1)


@pytest.mark.parametrize("canon", [True, False], ids=["canon", "fwd"])
def test_a_palindromic_kmer_with_even_k(gpu_ctx, d2g, canon):
    """k = 14: a k-mer that is its own reverse complement, three times; canonical or not it is one element of count 3"""
    rng = np.random.default_rng(1504)
    k, half = 14, "ACGGTCA"
    pal = half + revcomp(half)
    assert revcomp(pal) == pal and len(pal) == k
    recs = [C.random_bases(rng, 40) + pal + C.random_bases(rng, 40), pal, C.random_bases(rng, 25) + pal]
    S = 4096
    regs, cnts = check(gpu_ctx, d2g, [recs], k, S, canon, 0, "palindrome")
    i = R.oph_id_int(R.wang64_int(C.kmers_of([pal], k, canon)[0]))
    assert int(regs[0, (i & 0xFFFFFFFF) % S]) == i and int(cnts[0, (i & 0xFFFFFFFF) % S]) == 3


# ---------------------------------------------------------------- the all-ones id
def ones_id_mask(oracle, x0):
    """the xormask under which the OPH id of k-mer x0 is 2^64-1: wang64(wang64(x0 ^ mask) ^ ophxor) = ~0"""
    mask = oracle.wang_inverse(oracle.wang_inverse(M64) ^ R.OPHXOR) ^ x0
    assert R.oph_id_int(R.wang64_int(x0 ^ mask)) == M64
    return mask


@pytest.mark.parametrize("S,alone", [(1024, True), (2, False)], ids=["alone_in_its_register", "beside_a_smaller_id"])
def test_the_all_ones_id_counts(gpu_ctx, d2g, oracle, S, alone):
    """a k-mer whose id is ~0 leaves its register at ~0 and still counts (oph.h:209).  m = 1024: nothing else maps to register 1023, so it
    stays ~0 and its count is the k-mer's multiplicity, 3.  m = 2: register 1 also gets smaller ids, so it holds the smallest and ITS
    multiplicity"""
    rng = np.random.default_rng(1505)
    unit = C.random_bases(rng, K + 25)
    recs = [unit, unit, unit, C.random_bases(rng, 30)]
    x0 = C.kmers_of([unit], K, True)[7]
    mask = ones_id_mask(oracle, x0)
    regs, cnts = check(gpu_ctx, d2g, [recs], K, S, True, mask, "all-ones id")
    r = 0xFFFFFFFF % R.oph_m(S)
    if alone:
        assert int(regs[0, r]) == M64 and int(cnts[0, r]) == 3
        assert int((regs[0] == M64).sum()) > 900 and int(cnts[0][regs[0] == M64].sum()) == 3      # every other empty register counts 0
    else:
        assert int(regs[0, r]) != M64 and int(cnts[0, r]) in (1, 3)
        keys, counts, _ = C.key_counts(tuple(recs), K, True, mask)
        assert int(cnts[0, r]) == int(counts[keys == R.decode(regs[0, r:r + 1])[0]][0])


# ---------------------------------------------------------------- a batch
def test_a_batch_of_four_genomes(gpu_ctx, d2g):
    """0 k-mers (a record shorter than k), 1 k-mer, 300 and 70 000: the empty one gives all-~0 registers and zero counts"""
    rng = np.random.default_rng(1506)
    genomes = [["ACGTACGTAC"], [C.random_bases(rng, K)], [C.random_bases(rng, 300 + K - 1)], doubled()]
    for S in (5, 1024):
        regs, cnts = check(gpu_ctx, d2g, genomes, K, S, True, 0, "batch")
        assert (regs[0] == M64).all() and not cnts[0].any()
        assert int(cnts[1].sum()) == 1 and int((regs[1] != M64).sum()) == 1


# ---------------------------------------------------------------- d2g_oph_count_dev over registers that K1 did not write
def test_count_dev_with_planted_registers(gpu_ctx, d2g):
    """defined for any registers: a value no k-mer has counts 0, a non-minimal id of its bucket counts its multiplicity; every word of
    the output is written (it starts as 0xAB bytes)"""
    rng = np.random.default_rng(1507)
    unit = C.random_bases(rng, 400)
    genomes = [[unit, unit[:200]], [C.random_bases(rng, 250)]]
    S, m = 6, 6
    sp = seqpack(d2g, genomes, K)
    packed, rs, rl, go = sp.arrays()
    regs, _ = expected(genomes, K, True, 0, S)
    kc = [C.key_counts(tuple(g), K, True, 0) for g in genomes]
    ids0 = np.sort(R.k0_ref.wang64(kc[0][0] ^ np.uint64(R.OPHXOR)))
    planted = regs.copy()
    for r in range(3):                                                 # genome 0, registers 0..2: the LARGEST id of the bucket
        planted[0, r] = ids0[(ids0 & np.uint64(0xFFFFFFFF)) % np.uint64(m) == r][-1]
        assert planted[0, r] != regs[0, r]
    planted[0, 3] = regs[0, 3] ^ np.uint64(1 << 40)                    # same bucket (low bits kept), an id no k-mer has
    assert planted[0, 3] not in ids0
    planted[1, 0] = regs[0, 0]                                         # another genome's register
    want = np.stack([R.counts_for(kc[g][0], kc[g][1], planted[g]) for g in range(2)])
    assert want[0, 3] == 0 and want[1, 0] == 0 and (want[0, :3] >= 1).all() and int(want[0, :3].max()) == 2
    plan = gpu_ctx.oph_plan(rs, rl, go, K)
    d_packed, d_regs, d_cnt = gpu_ctx.malloc(packed.size), gpu_ctx.malloc(planted.nbytes), gpu_ctx.malloc(4 * planted.size)
    try:
        gpu_ctx.h2d(d_packed, packed)
        gpu_ctx.h2d(d_regs, planted)
        gpu_ctx.h2d(d_cnt, np.full(planted.size, 0xABABABAB, np.uint32))
        gpu_ctx.oph_count_dev(plan, d_packed, S, d_regs, d_cnt)
        got = np.empty(planted.shape, np.uint32)
        gpu_ctx.d2h(got, d_cnt)                                        # the null stream: after the count pass
        np.testing.assert_array_equal(got, want)
    finally:
        plan.close()
        for p in (d_packed, d_regs, d_cnt):
            gpu_ctx.free(p)


# ---------------------------------------------------------------- the persistent form
def test_sketcher_run_counts_then_the_other_forms(gpu_ctx, d2g):
    """one sketcher, in this order: counts of 4 genomes, of 2 (the grow-only buffers are larger than the batch; what the first run left
    must not show), then d2g_sketcher_run and d2g_sketcher_run_bmh as if nothing had happened, then the device-parsed stream"""
    rng = np.random.default_rng(1508)
    big = [[C.random_bases(rng, 900), C.random_bases(rng, 40)], [C.random_bases(rng, 2000)], ["ACGT"], doubled()]
    small = [[C.random_bases(rng, 500)] * 3, [C.random_bases(rng, 70)]]
    S = 1000
    sk = gpu_ctx.sketcher()
    try:
        for genomes in (big, small):
            regs, cnts = sk.run_counts(seqpack(d2g, genomes, K), S)
            eregs, ecnts = expected(genomes, K, True, 0, S)
            np.testing.assert_array_equal(regs, eregs)
            np.testing.assert_array_equal(cnts, ecnts)
        assert int(ecnts[0].max()) == 3
        sp = seqpack(d2g, small, K)
        np.testing.assert_array_equal(sk.run(sp, S), eregs)
        sig, tw = sk.run_bmh(sp, 64)
        esig, etw = gpu_ctx.bmh_sketch_seqpack(sp, 64)
        assert np.array_equal(sig.view(np.uint64), esig.view(np.uint64)) and np.array_equal(tw, etw)
        fastas = [C.fasta(g, f"g{i}") for i, g in enumerate(big)]
        runs = sk.ingest_fasta(fastas, K)
        regs, cnts = sk.run_counts_ingested(runs, S)
        eregs, ecnts = expected(big, K, True, 0, S)
        np.testing.assert_array_equal(regs, eregs)
        np.testing.assert_array_equal(cnts, ecnts)
        hregs, hcnts = sk.run_counts(seqpack(d2g, big, K), S)            # host-parsed, same sketcher
        assert np.array_equal(hregs, regs) and np.array_equal(hcnts, cnts)
    finally:
        sk.close()


def test_the_count_pass_is_timed_under_its_own_name(gpu_ctx, d2g):
    gpu_ctx.set_timing(d2g.TIME_K1)
    try:
        gpu_ctx.kernel_ms("k1")
        gpu_ctx.kernel_ms("k1count")
        sp = seqpack(d2g, [[C.random_bases(np.random.default_rng(1509), 500)]], K)
        gpu_ctx.oph_sketch_seqpack(sp, 64)
        assert gpu_ctx.kernel_ms("k1", reset=False)[0] == 1 and gpu_ctx.kernel_ms("k1count", reset=False)[0] == 0
        gpu_ctx.oph_sketch_counts_seqpack(sp, 64)
        assert gpu_ctx.kernel_ms("k1")[0] == 2 and gpu_ctx.kernel_ms("k1count")[0] == 1
    finally:
        gpu_ctx.set_timing(False)


def test_a_genome_of_two_to_the_32_kmers_is_refused_before_anything_is_staged(gpu_ctx, d2g):
    """the tables alone decide: two runs of 2^31 bases at k = 1 are 2^32 k-mers.  The refusal comes before the plan, the upload and any
    launch (the 68-byte stream is never read), and in the sketcher form before the stage, so a stream ingested earlier stays usable"""
    packed = np.zeros(68, np.uint8)
    rs, rl, go = np.array([0, 1 << 31], np.uint64), np.array([1 << 31, 1 << 31], np.uint32), np.array([0, 2], np.uint64)
    with pytest.raises(d2g.D2GError) as e:
        gpu_ctx.oph_sketch_counts(packed, rs, rl, go, 1, 8)
    assert e.value.status == -5 and "2^32" in str(e.value)
    genomes = [[C.random_bases(np.random.default_rng(1510), 400)]]
    sk = gpu_ctx.sketcher()
    try:
        runs = sk.ingest_fasta([C.fasta(genomes[0], "g0")], K)
        with pytest.raises(d2g.D2GError) as e:
            sk.run_counts_ingested((rs, rl, go), 8, k=1)
        assert e.value.status == -5
        regs, cnts = sk.run_counts_ingested(runs, 64)                   # the ingested stream was not invalidated
        eregs, ecnts = expected(genomes, K, True, 0, 64)
        assert np.array_equal(regs, eregs) and np.array_equal(cnts, ecnts)
    finally:
        sk.close()
