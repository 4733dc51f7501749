"""The amino-acid model (tests/protein_ref.py) held to its own properties.  No GPU, nothing of the product."""
import numpy as np
import pytest

import protein_ref as P

PAIRS = [(P.PROTEIN20, 1), (P.PROTEIN20, 5), (P.PROTEIN20, 14), (P.PROTEIN_14, 7), (P.PROTEIN_14, 16), (P.PROTEIN_3BIT, 11),
         (P.PROTEIN_3BIT, 21), (P.PROTEIN_6, 13), (P.PROTEIN_6, 24)]


def test_every_alphabet_covers_exactly_the_twenty_letters():
    for a in P.ALPHABETS:
        groups = P.GROUPS[a].split()
        assert sorted("".join(groups)) == sorted(P.LETTERS20) and len(set("".join(groups))) == 20
        t = P.code_table(a)
        valid = {chr(b) for b in range(256) if t[b] >= 0}
        assert valid == set(P.LETTERS20) | set(P.LETTERS20.lower())
        assert all(t[ord(c)] == t[ord(c.lower())] for c in P.LETTERS20)
        assert sorted(set(t[t >= 0].tolist())) == list(range(P.size(a)))
        assert all(t[ord(c)] < 0 for c in P.INVALID_LETTERS + P.INVALID_LETTERS.lower() + "\n >@0")
    assert [P.size(a) for a in P.ALPHABETS] == [20, 14, 8, 6]
    assert (P.PROTEIN20, P.PROTEIN_3BIT, P.PROTEIN_14, P.PROTEIN_6) == (2, 3, 4, 5)


def test_max_k_and_the_top_key():
    assert [P.max_k(a) for a in P.ALPHABETS] == [14, 16, 21, 24]
    for a in P.ALPHABETS:
        A, k = P.size(a), P.max_k(a)
        assert A ** k <= 2 ** 64 < A ** (k + 1)
        assert A ** k - 1 < 2 ** 63                                        # below the filter's free-slot value and its flag
        top = P.run_keys(np.full(k + 3, A - 1, np.uint8), k, a)
        assert top.tolist() == [A ** k - 1] * 4
        assert P.key_bits(k, a) == (A ** k - 1).bit_length() <= 63
    # the key-width seam of the exact counter: 31/35, 30/33 and 32/34 bits
    assert [P.key_bits(k, a) for a, k in [(2, 7), (2, 8), (3, 10), (3, 11), (5, 12), (5, 13)]] == [31, 35, 30, 33, 32, 34]


@pytest.mark.parametrize("alphabet,k", PAIRS)
def test_rolled_keys_equal_the_brute_force(alphabet, k):
    seq = P.random_protein(alphabet * 100 + k, 300)
    got = P.run_keys(P.runs(seq, alphabet)[0], k, alphabet)
    assert got.dtype == np.uint64 and got.tolist() == P.run_keys_brute(seq, k, alphabet)
    low = P.run_keys(P.runs(seq.lower(), alphabet)[0], k, alphabet)
    assert np.array_equal(low, got)
    # first residue most significant
    A = P.size(alphabet)
    assert int(got[0]) // A ** (k - 1) == int(P.code_table(alphabet)[seq[0]])


@pytest.mark.parametrize("alphabet,k", [(P.PROTEIN20, 5), (P.PROTEIN_6, 24)])
def test_runs_end_at_every_other_byte_and_at_records(alphabet, k):
    a, b, c = (P.random_protein(s, 60) for s in (1, 2, 3))
    for bad in P.INVALID_LETTERS + "x1 .":
        joined = a + bad.encode() + b
        ks = P.seq_keys(joined, k, alphabet)
        assert ks.tolist() == P.run_keys_brute(a, k, alphabet) + P.run_keys_brute(b, k, alphabet)
    two = P.fa(a, "r0") + P.fa(b[:k - 1], "short") + P.fa(c, "r2")
    assert P.fasta_keys(two, k, alphabet).tolist() == P.run_keys_brute(a, k, alphabet) + P.run_keys_brute(c, k, alphabet)
    # a line break inside a record does not end a run
    assert np.array_equal(P.fasta_keys(b">x\n" + a[:30] + b"\n" + a[30:] + b"\n", k, alphabet), P.seq_keys(a, k, alphabet))
    codes, rs, rl, go, nk = P.stream([two], k, alphabet)
    assert rl.tolist() == [60, 60] and rs.tolist() == [0, 60] and go.tolist() == [0, 2] and nk == [2 * (60 - k + 1)] and codes.size == 120
    codes, rs, rl, go, nk = P.stream([two], k, alphabet, by_record=True)
    assert go.tolist() == [0, 1, 1, 2] and nk == [60 - k + 1, 0, 60 - k + 1]


def test_masked_counts():
    seq = P.random_protein(9, 50) * 3
    keys = P.fasta_keys(P.fa(seq), 5, P.PROTEIN20)
    mk, cnt = P.masked_counts(keys, xormask=12345)
    assert int(cnt.sum()) == keys.size and (np.diff(mk.astype(object)) > 0).all() and cnt.max() >= 2
    assert P.masked_counts([])[0].size == 0
