"""tests/oph_mincount_ref.py held to its own properties, on the reference alone: no GPU, no libd2g.

The claim the kernel rests on is that LazyOnePermSetSketch::update under set_mincount(c) does not depend on the order of the k-mers:
the one-at-a-time restatement (potentials map, promotion, erasure) must equal the closed form under every shuffle of one multiset."""
import numpy as np
import pytest

import k3_seam_cases as C
import oph_kmers_ref as R
import oph_mincount_ref as Q

M64 = R.M64


def multiset(rng, m, trial):
    """a stream with duplicates of 1 .. 6 occurrences, values from a narrow range so that buckets collide"""
    distinct = rng.integers(0, 1 << 63, 40 + 30 * m // 8, dtype=np.uint64) * np.uint64(2) + np.uint64(trial & 1)
    distinct = np.unique(distinct)
    return np.repeat(distinct, rng.integers(1, 7, distinct.size))


@pytest.mark.parametrize("m", [2, 4, 6, 1000, 1024])
def test_sequential_equals_closed_form_in_any_order(m):
    rng = np.random.default_rng(100 + m)
    for trial in range(2):
        stream = multiset(rng, m, trial)
        keys, counts = np.unique(stream, return_counts=True)
        orders = (stream, stream[::-1], rng.permutation(stream), rng.permutation(stream), rng.permutation(stream))
        for c in (2, 3, 4, 6, 7):
            regs, cnts = Q.closed_form(keys, counts, m, c)
            if c <= 6 and m <= 6:
                assert (regs != M64).any()
            if c == 7:
                assert (regs == M64).all() and int(cnts.sum()) == 0
            for order in orders:
                sr, sc = Q.sequential(order.tolist(), m, c)
                assert sr == regs.tolist() and sc == cnts.tolist(), (m, c)
            # a count is the full multiplicity of the k-mer behind the register, never less than c
            dec = R.decode(regs)
            for r in np.flatnonzero(regs != M64):
                assert int(cnts[r]) == int(counts[keys == dec[r]][0]) >= c


@pytest.mark.parametrize("c", [0, 1])
def test_mincount_below_two_is_the_plain_sketch(c):
    rng = np.random.default_rng(5)
    stream = multiset(rng, 6, 0)
    keys, counts = np.unique(stream, return_counts=True)
    assert Q.sequential(stream.tolist(), 6, c) == R.sequential(stream.tolist(), 6)
    pr, pc = R.closed_form(keys, counts, 6)
    qr, qc = Q.closed_form(keys, counts, 6, c)
    assert np.array_equal(pr, qr) and np.array_equal(pc, qc)
    assert Q.sequential(stream.tolist(), 6, c) == (pr.tolist(), pc.tolist())


def test_the_variants_differ_in_the_sequential_form_as_in_the_closed_one():
    rng = np.random.default_rng(6)
    stream = rng.permutation(multiset(rng, 4, 1))
    keys, counts = np.unique(stream, return_counts=True)
    for c in (2, 3):
        gr, gc = Q.closed_form(keys, counts, 4, c, "gt")
        assert Q.sequential(stream.tolist(), 4, c, "gt") == (gr.tolist(), gc.tolist())
        er, ec = Q.closed_form(keys, counts, 4, c + 1)
        assert np.array_equal(gr, er) and np.array_equal(gc, ec)       # `>` c is `>=` c + 1


# ---------------------------------------------------------------- the cases of the GPU tests
@pytest.mark.parametrize("canon", [True, False])
@pytest.mark.parametrize("k", Q.SEAM_K)
@pytest.mark.parametrize("c", Q.SEAM_C)
def test_ge_seam_cases_hold_their_conditions_and_detect_the_greater_than_variant(c, k, canon):
    for S in Q.SEAM_S:
        batch, eregs, ecnts = Q.ge_seam(c, S, k, canon)
        m = R.oph_m(S)
        assert len(batch.genomes) == Q.SEAM_GENOMES and eregs.shape == ecnts.shape == (Q.SEAM_GENOMES, m)
        regs, cnts = Q.expected(batch, S, c)
        assert np.array_equal(regs, eregs) and np.array_equal(cnts, ecnts)             # the closed form agrees with the construction
        assert set(np.unique(ecnts).tolist()) <= {0, c} and ((ecnts == c) == (eregs != M64)).all() and (eregs != M64).any()
        plain_regs, plain_cnts = Q.expected(batch, S, 1)
        gt_regs, _ = Q.expected(batch, S, c, variant="gt")
        for g, (keys, counts, _) in enumerate(batch.counts()):
            assert sorted(np.unique(counts).tolist()) == sorted({1, c - 1, c})
            assert not np.array_equal(plain_regs[g], eregs[g]) and (plain_cnts[g] == c - 1).any()
            assert (gt_regs[g] == M64).all()                                           # `>` drops B itself
        if S in (7, 64):
            for g, records in enumerate(batch.genomes):
                sr, sc = Q.sequential(R.masked_stream(records, k, canon, batch.xormask), m, c)
                assert sr == eregs[g].tolist() and sc == ecnts[g].tolist()


def test_planted_counts_under_every_threshold():
    batch = Q.planted()
    assert batch.nkmers()[2:] == [0, 0] and len(batch.genomes) == 4
    nonempty = []
    for c in (1, 2, 3, 4, 5):
        regs, cnts = Q.expected(batch, batch.S, c)
        assert (regs[2:] == M64).all() and (cnts[2:] == 0).all()
        assert (cnts[0][regs[0] != M64] >= c).all()
        nonempty.append(int((regs[0] != M64).sum()))
        if c >= 3:
            assert (regs[1] == M64).all()                              # genome 1 has only count 2
    assert nonempty[0] >= nonempty[1] >= nonempty[2] >= nonempty[3] > nonempty[4] == 0
    assert len({Q.expected(batch, batch.S, c)[0].tobytes() for c in (1, 2, 3, 4, 5)}) >= 4
    for c in (2, 4):
        sr, sc = Q.sequential(R.masked_stream(batch.genomes[0], batch.k, batch.canon, batch.xormask), R.oph_m(batch.S), c)
        regs, cnts = Q.expected(batch, batch.S, c)
        assert sr == regs[0].tolist() and sc == cnts[0].tolist()


def test_the_all_ones_id_case_detects_thresholded_counts():
    batch, c, r = Q.ones_id()
    regs, cnts = Q.expected(batch, batch.S, c)
    assert (regs[0] == M64).all() and cnts[0].tolist() == [1 if i == r else 0 for i in range(regs.shape[1])]
    assert regs[1][r] != M64 and cnts[1][r] == c
    wregs, wcnts = Q.expected(batch, batch.S, c, variant="thresholded_counts")
    assert np.array_equal(wregs, regs) and wcnts[0][r] == 0 and np.array_equal(wcnts[1], cnts[1])
    for g, records in enumerate(batch.genomes):
        sr, sc = Q.sequential(R.masked_stream(records, batch.k, batch.canon, batch.xormask), R.oph_m(batch.S), c)
        assert sr == regs[g].tolist() and sc == cnts[g].tolist()


@pytest.mark.parametrize("canon", [True, False])
@pytest.mark.parametrize("c", [2, 3])
def test_the_filter_case_removes_a_winner_and_keeps_its_neighbours(c, canon):
    batch, record, drop = Q.filtered(c, canon)
    keys, counts, _ = batch.counts()[0]
    assert int(counts[keys == drop[0]][0]) == c and len(record) == batch.k
    regs, cnts = Q.expected(batch, batch.S, c)
    fregs, fcnts = Q.expected(batch, batch.S, c, drop=drop)
    assert not np.array_equal(regs, fregs)
    assert int((fregs != regs).sum()) == 1                             # only the register that the filtered k-mer held
    assert (fcnts[0][fregs[0] != M64] == c).all() and int((fregs[0] != M64).sum()) >= int((regs[0] != M64).sum()) - 1 > 0


def test_the_k3_seam_batches_keep_something_under_two_and_three():
    """all_ones_generic('unit'): the key ~0 occurs three times and survives both thresholds; all_ones_only: counts 180 and 10; the
    compact batches hold k-mers that end in sixteen T five and six times; the table-round genomes, doubled, keep every k-mer under
    c = 2 and none under c = 3"""
    b = C.all_ones_generic("unit")
    keys, counts, _ = b.counts()[0]
    assert int(counts[keys == np.uint64(M64)][0]) == 3
    for c in (2, 3):
        assert (Q.expected(b, b.S, c)[0] != M64).any()
        assert (Q.expected(C.all_ones_only(), 16, c)[0][:2] != M64).any(axis=1).all()
        assert (Q.expected(C.all_ones_compact(17), 16, c)[0][:2] != M64).any(axis=1).all()
    d = Q.doubled(C.table_round_genomes())
    assert [2 * x for x in C.table_round_genomes().nkmers()] == d.nkmers()
    assert np.array_equal(Q.expected(d, 16, 2)[0], Q.expected(C.table_round_genomes(), 16, 1)[0])
    assert (Q.expected(d, 16, 3)[0] == M64).all() and (Q.expected(d, 16, 2)[1] == 2).all()
