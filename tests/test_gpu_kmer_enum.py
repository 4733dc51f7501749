"""d2g_for_each_kmer_its (d2g_kmers.h, the k-mer enumeration K1 and K3 share) through d2g_kmer_count, which loses nothing: every
k-mer of every run comes back as a key with its count.  Own run tables over ONE host-packed random stream put a run at every word
alignment (0..15) with every k-mer count around the enumeration's seams -- the 16-k-mer word of the main window, the 64-k-mer chunk
of a lane, two chunks -- for every k in 1..32, canonical and not; two runs cross the 1024-chunk share of a workgroup, and 1025
one-chunk runs make a workgroup search its runs (blk_run_lo / blk_run_hi).

Expected keys and counts: a pure-Python rolling enumerator and the key transform of the oracle (d2o_maskfn: wang64(kmer ^ xormask)),
restated in NumPy uint64 (k0_ref.wang64, pinned against the library by test_k0_ref.py)."""
import numpy as np
import pytest

import k0_ref

pytestmark = pytest.mark.gpu

NBASES = 70_000
ALIGNMENTS = range(16)
COUNTS = (1, 2, 15, 16, 17, 63, 64, 65, 128, 129)
STRIDE = 272                                                           # bases between the genomes' origins: a multiple of 16, > 15 + 32 + 129


@pytest.fixture(scope="module")
def stream():
    codes = np.random.default_rng(2024).integers(0, 4, NBASES).astype(np.uint8)
    codes[60_000:60_200] = 0                                           # poly-A: canonical k-mers that are their own reverse's minimum
    codes[61_000:61_100] = np.tile([0, 3], 50)                         # ATAT...: reverse-complement palindromes
    return codes, codes.tolist(), k0_ref.pack_codes(codes)


def enumerate_kmers(code_list, start, length, k, canon):
    """the k-mers of the run [start, start + length), rolled one base at a time: forward value (first base most significant) or the
    smaller of it and its reverse complement"""
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    fwd = rc = 0
    out = []
    for j in range(length):
        c = code_list[start + j]
        fwd = ((fwd << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << top)
        if j >= k - 1:
            out.append(min(fwd, rc) if canon else fwd)
    return out


def expected_counts(code_list, runs, k, canon, xormask):
    kmers = [x for s, n in runs for x in enumerate_kmers(code_list, s, n, k, canon)]
    keys, counts = np.unique(k0_ref.wang64(np.array(kmers, np.uint64) ^ np.uint64(xormask)), return_counts=True)
    return keys, counts.astype(np.uint32), len(kmers)


def check(gpu_ctx, stream, genomes, k, canon, xormask):
    """genomes: list of lists of (start, len)"""
    codes, code_list, packed = stream
    rs = [s for g in genomes for s, _ in g]
    rl = [n for g in genomes for _, n in g]
    go = np.concatenate([[0], np.cumsum([len(g) for g in genomes])])
    got = gpu_ctx.kmer_count(packed, rs, rl, go, k, canon=canon, xormask=xormask)
    assert len(got) == len(genomes)
    for gi, g in enumerate(genomes):
        ek, ec, nk = expected_counts(code_list, g, k, canon, xormask)
        what = f"k={k} canon={canon} genome {gi}: runs {g[:3]}{'...' if len(g) > 3 else ''}, {nk} k-mers"
        np.testing.assert_array_equal(got[gi][0], ek, err_msg=what + " (keys)")
        np.testing.assert_array_equal(got[gi][1], ec, err_msg=what + " (counts)")
        assert int(got[gi][1].sum()) == nk, what


@pytest.mark.parametrize("k", range(1, 33))
def test_every_alignment_and_count_seam(gpu_ctx, stream, k):
    genomes = [[(gi * STRIDE + a, k + n - 1)] for gi, (a, n) in enumerate((a, n) for a in ALIGNMENTS for n in COUNTS)]
    assert genomes[-1][0][0] + genomes[-1][0][1] <= 60_000
    check(gpu_ctx, stream, genomes, k, True, 0)
    check(gpu_ctx, stream, genomes, k, False, 0x0123456789ABCDEF)


@pytest.mark.parametrize("k,canon", [(1, True), (21, True), (31, False), (32, True)])
def test_runs_across_the_workgroup_seam_and_many_runs_per_workgroup(gpu_ctx, stream, k, canon):
    """1024 chunks of 64 k-mers per workgroup: 65536 k-mers fill one exactly, 65537 spill one k-mer into the next; 1025 runs of one
    chunk each (1..64 k-mers, every alignment, overlapping in the stream) make two workgroups that search 1024 runs and 1"""
    many = [((i * 37 + 40_000 * (i % 2)) % (NBASES - 200), k + (i % 64)) for i in range(1025)]
    genomes = [[(3, 65536 + k - 1)], [(1000 + 7, 65537 + k - 1)], many, [(60_000 - 5, 300 + k)], [(61_000 - 7, 150 + k)]]
    check(gpu_ctx, stream, genomes, k, canon, 0)
