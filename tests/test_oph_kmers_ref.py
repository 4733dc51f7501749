"""tests/oph_kmers_ref.py held to its own properties, on the reference alone: no GPU, no libd2g."""
import numpy as np
import pytest

import k0_ref
import k3_seam_cases as C
import oph_kmers_ref as R

M64 = R.M64


def test_the_hash_constants_are_the_oracles(oracle):
    lib = oracle.load()
    for x in (0, 1, 133348, M64, 0x0123456789ABCDEF):
        assert R.oph_id_int(x) == int(lib.d2o_oph_id(x))               # Wang(x ^ seed_ ^ CEIXOR)
        assert R.wang64_int(x) == oracle.wang_hash(x) == int(k0_ref.wang64(np.array([x], np.uint64))[0])


@pytest.mark.parametrize("m", [2, 4, 6, 1000, 1024])
def test_sequential_equals_closed_form_in_any_order(m):
    """random streams with duplicates, a narrow value range so that buckets collide and minima repeat; forward, reversed, sorted and
    shuffled: the result does not depend on the order"""
    rng = np.random.default_rng(m)
    for trial in range(3):
        distinct = rng.integers(0, 1 << 63, 40 + 30 * m // 8, dtype=np.uint64) * np.uint64(2) + np.uint64(trial & 1)
        stream = rng.choice(distinct, distinct.size * 3)
        keys, counts = np.unique(stream, return_counts=True)
        regs, cnts = R.closed_form(keys, counts, m)
        assert int(cnts.sum()) > 0 and int(cnts.max()) >= 2
        for order in (stream, stream[::-1], np.sort(stream), rng.permutation(stream)):
            sr, sc = R.sequential(order.tolist(), m)
            assert sr == regs.tolist() and sc == cnts.tolist()
        # what the counts mean: the multiplicity of the k-mer the register decodes to
        dec = R.decode(regs)
        for r in np.flatnonzero(cnts):
            assert int(cnts[r]) == int(counts[keys == dec[r]][0])


def test_closed_form_of_nothing():
    regs, cnts = R.closed_form(np.zeros(0, np.uint64), np.zeros(0, np.uint32), 6)
    assert regs.tolist() == [M64] * 6 and cnts.tolist() == [0] * 6
    assert R.sequential([], 6) == ([M64] * 6, [0] * 6)


def test_decode_inverts_the_hasher(oracle):
    rng = np.random.default_rng(11)
    r = np.concatenate([np.array([0, M64, 1, 1 << 63], np.uint64), rng.integers(0, 1 << 63, 2000, dtype=np.uint64) * np.uint64(3)])
    d = R.decode(r)
    assert np.array_equal(k0_ref.wang64(d ^ np.uint64(R.OPHXOR)), r)
    assert np.array_equal(k0_ref.wang64(R.wang64_inverse(r)), r) and np.array_equal(R.wang64_inverse(k0_ref.wang64(r)), r)
    for x, w in zip(r[:64].tolist(), R.wang64_inverse(r[:64]).tolist()):
        assert w == oracle.wang_inverse(x)
    assert R.decode(r.reshape(4, -1)).shape == (4, r.size // 4)


def test_detects_a_variant_that_skips_empty_registers():
    """a stream that holds the id ~0: its register stays ~0 and counts; the variant that never counts against ~0 gives 0 there"""
    ones = R.wang64_inverse(np.array([M64], np.uint64))[0] ^ np.uint64(R.OPHXOR)      # the masked k-mer whose id is ~0
    assert R.oph_id_int(int(ones)) == M64
    m = 6
    idx = (M64 & 0xFFFFFFFF) % m
    others = [x for x in range(1, 400) if (R.oph_id_int(x) & 0xFFFFFFFF) % m != idx][:20]
    stream = [int(ones)] + others + [int(ones), int(ones)]
    regs, cnts = R.sequential(stream, m)
    assert regs[idx] == M64 and cnts[idx] == 3
    keys, counts = np.unique(np.array(stream, np.uint64), return_counts=True)
    cr, cc = R.closed_form(keys, counts, m)
    assert cr.tolist() == regs and cc.tolist() == cnts
    wr, wc = R.sequential(stream, m, skip_empty=True)
    assert wr == regs and wc[idx] == 0 and wc != cnts


def test_detects_a_variant_that_does_not_canonicalise():
    """a genome that holds a k-mer and its reverse complement: one element of count 2 when canonical, two elements when not"""
    k, S = 15, 4
    x = "ACGGTCATTGCAGTC"
    rc = x[::-1].translate(str.maketrans("ACGT", "TGCA"))
    assert rc != x
    genome = [x, rc]
    rc_, cc_ = R.genome_closed_form(genome, k, True, 0, S)
    rn, cn = R.genome_closed_form(genome, k, False, 0, S)
    assert cc_.tolist().count(2) == 1 and int(cc_.sum()) == 2
    assert int(cn.max()) == 1 and int(cn.sum()) in (1, 2)              # 1 + 1 in two registers, or one register that kept the smaller id
    assert not (np.array_equal(rc_, rn) and np.array_equal(cc_, cn))
    for canon in (True, False):
        sr, sc = R.sequential(R.masked_stream(genome, k, canon, 0), R.oph_m(S))
        er, ec = R.genome_closed_form(genome, k, canon, 0, S)
        assert sr == er.tolist() and sc == ec.tolist()


def test_writers_lay_the_files_out_as_documented():
    ids = np.arange(6, dtype=np.uint64).reshape(2, 3)
    b = R.kmer64_bytes(ids, 3, 11, 11, True, 5)
    assert len(b) == 24 + 48 and np.frombuffer(b[:16], np.uint32).tolist() == [256, 3, 11, 11] and np.frombuffer(b[16:24], np.uint64)[0] == 5
    assert R.kmer64_bytes(ids, 3, 11, 0, False, 0)[:16] == np.array([0, 3, 11, 0], np.uint32).tobytes()
    assert R.kmer64_names_bytes(["a.fa", "b c.fa"]) == b"a.fa\nb c.fa\n"
    assert R.kmercounts_bytes(np.array([[1, 2, 70000]], np.uint32), 3) == np.array([1, 2, 70000], np.float32).tobytes()
    assert R.kmercounts_column("d/x.fa", 63, 11) == "d/x.fa.rc_canon.sketchsize63.k11.SetSpace.DNA.kmercounts.f64"
    assert R.kmercounts_column("d/x.fa", 8, 31, canon=False, seedseed=7) == "d/x.fa.seed7.sketchsize8.k31.SetSpace.DNA.kmercounts.f64"
    assert R.oph_m(63) == 64 and R.oph_m(1) == 2 and R.oph_m(1024) == 1024
