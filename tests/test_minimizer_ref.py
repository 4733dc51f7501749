"""tests/minimizer_ref.py held to its own properties (no GPU): the deque enumerator against one brute-force min() per window, the two
hand-worked cases that pin the score mask, runs shorter than a window, w <= k, and the rewrite the GPU tests lean on."""
import numpy as np
import pytest

import filter_ref as FR
import minimizer_ref as MR
from dashing2_amd import synth


def _rand(seed, n):
    return synth.random_genome(seed, n).tobytes()


INPUTS = {
    "random": _rand(1, 700),
    "polyA": b"A" * 300,
    "AC": b"AC" * 150,
    "unit7": _rand(2, 7) * 60,
    "unit8": _rand(3, 8) * 60,
    "Ns": _rand(4, 200) + b"N" + _rand(5, 36) + b"NN" + _rand(6, 37) + b"R" + _rand(7, 9) + b"N" + _rand(8, 300),
}


@pytest.mark.parametrize("name", sorted(INPUTS))
@pytest.mark.parametrize("k,w", [(5, 7), (21, 22), (21, 36), (21, 37), (32, 33), (15, 120), (8, 8), (8, 3), (8, 0)])
@pytest.mark.parametrize("canon", [False, True])
def test_deque_equals_brute_force(name, k, w, canon):
    fa = b">a\n" + INPUTS[name] + b"\n"
    a = MR.fasta_emissions(fa, k, w, canon)
    b = MR.fasta_emissions(fa, k, w, canon, brute=True)
    c = MR.fasta_emissions(fa, k, w, canon, fast=True)
    assert a == b == c
    span = max(k, w)
    assert len(a) == sum(max(0, len(r) - span + 1) for r in MR.runs(INPUTS[name]))


def test_the_hand_worked_case_pins_the_mask():
    """ACGT, k = 2, w = 3.  AC = 0001, CG = 0110, GT = 1011; the mask's low four bits are 1101, so the scores are 12, 11, 6: the windows
    {AC, CG} and {CG, GT} emit CG and GT.  Plain lexicographic order would emit AC and CG."""
    assert MR.LEX_XOR & 15 == 0b1101
    assert [MR.encode(x) ^ (MR.LEX_XOR & 15) for x in (b"AC", b"CG", b"GT")] == [12, 11, 6]
    got = MR.fasta_emissions(b">x\nACGT\n", 2, 3, False)
    assert [MR.decode(v, 2) for v in got] == [b"CG", b"GT"]
    assert MR.fasta_emissions(b">x\nACGT\n", 2, 3, False, brute=True) == got
    # canonical: GT -> AC, so the k-mers are AC, CG, AC with scores 12, 11, 12: CG twice -- once per window position
    got = MR.fasta_emissions(b">x\nACGT\n", 2, 3, True)
    assert [MR.decode(v, 2) for v in got] == [b"CG", b"CG"]
    assert MR.rewrite(b">x\nACGT\n", 2, 3, True) == b">s\nCG\n>s\nCG\n"


def test_a_run_one_base_short_of_a_window_emits_nothing_and_nothing_spans_runs():
    k, w = 5, 9
    seq = _rand(11, 40)
    assert MR.fasta_emissions(b">a\n" + seq[:w - 1] + b"\n", k, w, True) == []
    assert len(MR.fasta_emissions(b">a\n" + seq[:w] + b"\n", k, w, True)) == 1
    cut = b">a\n" + seq[:20] + b"N" + seq[20:] + b"\n>b\n" + seq[:w - 1] + b"\n>c\n" + seq + b"\n"
    exp = MR.seq_emissions(seq[:20], k, w, True) + MR.seq_emissions(seq[20:], k, w, True) + MR.seq_emissions(seq, k, w, True)
    assert MR.fasta_emissions(cut, k, w, True) == exp and len(exp) == (20 - w + 1) * 2 + 40 - w + 1
    # multi-line records join before they are cut into runs
    assert MR.fasta_emissions(b">c\n" + seq[:13] + b"\n" + seq[13:] + b"\n", k, w, True) == MR.seq_emissions(seq, k, w, True)


@pytest.mark.parametrize("canon", [False, True])
def test_w_up_to_k_is_the_plain_enumeration(canon):
    fa = b">a\n" + INPUTS["Ns"] + b"\n>b\n" + INPUTS["random"] + b"\n"
    k = 11
    plain = [FR.encode(s) for s in FR.fasta_windows(fa, k, canon)]
    for w in (-1, 0, 1, k - 1, k):
        assert MR.fasta_emissions(fa, k, w, canon) == plain
        assert MR.rewrite(fa, k, w, canon) == b"".join(b">s\n" + s + b"\n" for s in FR.fasta_windows(fa, k, canon))
    assert MR.fasta_emissions(fa, k, k + 1, canon) != plain


def test_rewrite_holds_exactly_the_emitted_multiset():
    fa = b">a\n" + INPUTS["Ns"] + b"\n>b\n" + INPUTS["unit7"] + b"\n"
    for k, w, canon in [(7, 12, True), (7, 12, False), (32, 40, False)]:
        em = MR.fasta_emissions(fa, k, w, canon)
        rw = MR.rewrite(fa, k, w, canon)
        assert [FR.encode(s) for s in FR.fasta_windows(rw, k, canon)] == em          # read back by the PLAIN enumeration: the same k-mers
        by = MR.rewrite_by_record(fa, k, w, canon)
        assert [n for n, _ in by] == ["a", "b"] and b"".join(b for _, b in by) == rw
        keep = MR.rewrite(fa, k, w, canon, keep=lambda v: v & 1 == 0)
        assert [FR.encode(s) for s in FR.fasta_windows(keep, k, canon)] == [v for v in em if v & 1 == 0]
        keys, counts = MR.masked_counts(em)
        assert int(counts.sum()) == len(em) and keys.size == len(set(em)) and (np.diff(keys.astype(object)) > 0).all()


def test_wang_is_the_library_hash(d2g):
    x = np.array([0, 1, 2 ** 64 - 1, 0x0123456789ABCDEF, MR.LEX_XOR], np.uint64)
    assert [int(v) for v in MR.wang64(x)] == [d2g.wang_hash(int(v)) for v in x]
