"""contain_ref.py held to its own properties (no GPU, no library): the line-by-line restatement and the closed form agree on random
small cases; a key in two registers of one reference counts twice; sums wrap at 2^32; the epilogue is the integer quotient; the
text of single values equals fmt 12.1.0's own (tests/golden/contain_fmt.txt)."""
import os

import numpy as np
import pytest

import contain_ref as R
import k3_seam_cases as C
import oph_kmers_ref as K
from conftest import GOLDEN


def _db(rng, genomes, S, k, canon, xormask):
    regs = np.stack([K.genome_closed_form(g, k, canon, xormask, S)[0] for g in genomes])
    return K.decode(regs[:, :S])


@pytest.mark.parametrize("seed,k,S,canon,xormask", [(1, 6, 10, True, 0), (2, 11, 7, False, 0), (3, 21, 64, True, K.wang64_int(7)),
                                                     (4, 4, 33, False, 0x1234), (5, 31, 5, True, 0)])
def test_restatement_and_closed_form_agree(seed, k, S, canon, xormask):
    rng = np.random.default_rng(seed)
    base = C.random_bases(rng, 400)
    genomes = [[base[:200]], [base[100:350], C.random_bases(rng, 50)], [C.random_bases(rng, k + 2)], ["ACGT"[:min(4, k - 1)]]]
    db = _db(rng, genomes, S, k, canon, xormask)
    empty_key = int(K.decode(np.array([K.M64], np.uint64))[0])
    assert (db[3] == empty_key).all() and (db[2] == empty_key).sum() >= S - 3          # short references share the empty register's key
    queries = [[base[50:300], base[50:300]], [C.random_bases(rng, 300)], ["ACG"[:k - 1]], [base[:200] + "A" * 40, "A" * 40]]
    m, s = R.restatement(db, [R.masked_stream(q, k, canon, xormask) for q in queries])
    for q, recs in enumerate(queries):
        cm, cs = R.query_closed_form(db, recs, k, canon, xormask)
        np.testing.assert_array_equal(m[q], cm)
        np.testing.assert_array_equal(s[q], cs)
    assert m[0].max() > 0 and s[0].max() >= 2 * m[0].max() and not m[2].any()
    assert (m <= S).all()


def test_a_key_in_two_registers_counts_twice():
    db = np.array([[5, 5, 9], [9, 1, 2]], np.uint64)
    m, s = R.restatement(db, [[5, 5, 5, 9, 7]])
    assert m.tolist() == [[3, 1]] and s.tolist() == [[7, 1]]                           # 3 + 3 + 1; the reference pushes refid 0 twice for key 5
    cm, cs = R.closed_form(db, np.array([5, 7, 9], np.uint64), np.array([3, 1, 1], np.uint32))
    assert cm.tolist() == [3, 1] and cs.tolist() == [7, 1]


def test_sums_wrap_at_two_to_the_32_and_matches_do_not():
    db = np.array([[1, 2, 3]], np.uint64)
    cm, cs = R.closed_form(db, np.array([1, 2, 3], np.uint64), np.array([0xFFFFFFFF, 0xFFFFFFFF, 3], np.uint32))
    assert cm.tolist() == [3] and cs.tolist() == [(2 * 0xFFFFFFFF + 3) & 0xFFFFFFFF]
    cov, dep = R.epilogue(cm, cs, 3)
    assert cov[0] == np.float32(1) and dep[0] == np.float32(((2 * 0xFFFFFFFF + 3) & 0xFFFFFFFF) // 3)


def test_epilogue_is_the_floor_of_the_mean_and_zero_without_matches():
    cov, dep = R.epilogue(np.array([0, 3, 7, 1000], np.uint32), np.array([9, 10, 6, 999], np.uint32), 1000)
    assert dep.tolist() == [0.0, 3.0, 0.0, 0.0] and cov[0] == 0
    assert cov[1] == np.float32(np.float64(1) / np.float64(1000) * 3) and cov.dtype == np.float32 and dep.dtype == np.float32
    # the product in double then narrowed is not always the float product
    S = 1000
    m = np.arange(S + 1, dtype=np.uint32)
    cov, _ = R.epilogue(m, m, S)
    assert np.array_equal(cov, (np.float64(1) / np.float64(S) * m.astype(np.float64)).astype(np.float32))


def test_key_counts_of_db_lists_every_distinct_key_once():
    db = np.array([[5, 5, 9], [9, 1, 2]], np.uint64)
    d, c = R.key_counts_of_db(db, np.array([2, 5, 100], np.uint64), np.array([4, 3, 8], np.uint32))
    assert d.tolist() == [1, 2, 5, 9] and c.tolist() == [0, 4, 3, 0]


def test_value_text_equals_fmt_golden():
    n = 0
    with open(os.path.join(GOLDEN, "contain_fmt.txt")) as f:
        for line in f:
            kind, a, b, text = line.split()
            if kind == "g":
                cov = np.float32(np.float64(1) / np.float64(int(a)) * np.float64(int(b)))
                assert R.fmt_g6(np.float32(100) * cov) == text, line
            else:
                assert R.fmt_float(np.float32(int(b))) == text, line
            n += 1
    assert n > 2000


def test_writers_lay_the_table_out_as_the_reference_does():
    names, queries = ["r0", "r 1"], ["q.fq", "d/q2.fa.gz"]
    cov = np.array([[0, 3 / 1024], [1, 0.3]], np.float32)
    dep = np.array([[0, 3], [12, 1]], np.float32)
    t = R.text_bytes(names, queries, cov, dep).decode()
    assert t.split("\n")[:3] == ["#Dashing2 contain - a list of coverage %%s for the set of references, + mean coverage levels.",
                                 "#Each matrix entry consists of <coverage%%:mean depth of coverage>", "##References:\tr0\tr 1"]
    assert t.split("\n")[3:] == ["q.fq\t0%:0\t0.292969%:3", "d/q2.fa.gz\t100%:12\t30%:1", ""]
    b = R.binary_bytes(2, cov, dep)
    assert b[:16] == np.array([2, 2], np.uint64).tobytes() and b[16:32] == cov.tobytes() and b[32:] == dep.tobytes()
    assert R.binary_bytes(0, np.zeros((3, 0), np.float32), np.zeros((3, 0), np.float32)) == np.array([0, 3], np.uint64).tobytes()
