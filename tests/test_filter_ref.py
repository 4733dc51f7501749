"""tests/filter_ref.py, the --filterset model the GPU tests compare against: the rewriting itself (an empty filter must change
nothing the oracle computes), and the two filters whose outcome is known without the model.  No GPU."""
import numpy as np
import pytest

import filter_ref as FR
from dashing2_amd import synth


def _input():
    """two records; N runs, a run shorter than every k tested but 5, a non-ACGT byte that is not N"""
    a = synth.random_genome(900, 2500).tobytes()
    b = synth.random_genome(901, 700).tobytes()
    a = a[:400] + b"NNNN" + a[400:420] + b"N" + a[420:1500] + b"R" + a[1500:] + a[100:300]      # the tail repeats 200 bases: counts > 1
    return synth.fasta_bytes("r0", np.frombuffer(a, np.uint8)) + synth.fasta_bytes("r1", np.frombuffer(b, np.uint8), width=61)


@pytest.mark.parametrize("canon", [True, False])
@pytest.mark.parametrize("k", [5, 21, 32])
def test_empty_filter_rewrites_to_the_same_multiset(oracle, k, canon):
    fa = _input()
    rw = FR.rewrite(fa, set(), k, canon)
    assert rw.count(b">") == len(FR.fasta_windows(fa, k, canon)) > 0
    for S in (64, 101):
        e, g = oracle.sketch_buffer(fa, k=k, canon=canon, S=S), oracle.sketch_buffer(rw, k=k, canon=canon, S=S)
        assert np.array_equal(e[0], g[0]) and np.array_equal(e[1].view(np.uint64), g[1].view(np.uint64)) and e[2:] == g[2:]
    ek, ec, en = oracle.kmer_count_buffer(fa, k, canon)
    gk, gc, gn = oracle.kmer_count_buffer(rw, k, canon)
    assert np.array_equal(ek, gk) and np.array_equal(ec, gc) and en == gn and ec.max() > 1
    for thr in (0.0, 1.0):
        e, g = oracle.bmh_sketch_buffer(fa, k, 64, canon, count_threshold=thr), oracle.bmh_sketch_buffer(rw, k, 64, canon, count_threshold=thr)
        assert np.array_equal(e[0].view(np.uint64), g[0].view(np.uint64)) and e[1:] == g[1:]


@pytest.mark.parametrize("canon", [True, False])
def test_filtering_a_genome_by_itself_leaves_nothing(oracle, canon):
    fa = _input()
    fset, nocc = FR.filter_set([fa], 21, canon)
    assert nocc == len(FR.fasta_windows(fa, 21, canon)) > len(fset)          # occurrences count duplicates, the set does not
    assert FR.rewrite(fa, fset, 21, canon) == b""
    assert oracle.sketch_buffer(b"", k=21, canon=canon, S=64)[3] == 0          # and the oracle takes an input without k-mers


def test_reverse_complement_filter_canon_on_and_off():
    k = 21
    g = synth.random_genome(902, 3000).tobytes()
    fa = synth.fasta_bytes("g", np.frombuffer(g, np.uint8))
    rc = synth.fasta_bytes("rc", np.frombuffer(FR.revcomp(g), np.uint8))
    assert FR.rewrite(fa, FR.filter_set([rc], k, True)[0], k, True) == b""
    # canon off: only the forward windows of the input that occur, as they are, among the forward windows of the reverse complement go
    fwd_rc = {FR.revcomp(g)[i:i + k] for i in range(len(g) - k + 1)}
    keep = [g[i:i + k] for i in range(len(g) - k + 1) if g[i:i + k] not in fwd_rc]
    assert len(keep) == len(g) - k + 1                                          # random sequence, odd k: nothing coincides
    assert FR.rewrite(fa, FR.filter_set([rc], k, False)[0], k, False) == b"".join(b">s\n" + w + b"\n" for w in keep)
    # ... and a planted reverse-complement palindrome does go
    pal = b"ACGTTGCAAGCTTGCAACGT" * 2
    assert FR.revcomp(pal) == pal
    fa2 = synth.fasta_bytes("p", np.frombuffer(g[:100] + pal + g[100:200], np.uint8))
    rc2 = synth.fasta_bytes("p", np.frombuffer(FR.revcomp(g[:100] + pal + g[100:200]), np.uint8))
    s2 = g[:100] + pal + g[100:200]
    inside = {pal[i:i + k] for i in range(len(pal) - k + 1)}                    # these occur, as they are, in the reverse complement too
    keep2 = [s2[i:i + k] for i in range(len(s2) - k + 1) if s2[i:i + k] not in inside]
    assert len(s2) - k + 1 - len(keep2) >= len(pal) - k + 1
    assert FR.rewrite(fa2, FR.filter_set([rc2], k, False)[0], k, False) == b"".join(b">s\n" + w + b"\n" for w in keep2)


def test_encode_orders_like_the_strings():
    assert FR.encode(b"A" * 32) == 0 and FR.encode(b"T" * 32) == 2 ** 64 - 1 and FR.encode(b"ACGT") == 0b00011011
    ws = FR.fasta_windows(_input(), 7, False)
    assert sorted(ws) == sorted(ws, key=FR.encode)
