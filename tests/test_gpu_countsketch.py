"""The count-sketch chain on the GPU (K3k: --multiset -c <cells>; k3k_add / k3k_count / k3k_scan / k3k_write and BagMinHash over the
device-resident lists, d2g_k3_bmh.hip) against the NumPy model of tests/countsketch_ref.py.  Every comparison is exact: the table cell
for cell and signed, the lists id for id, registers and totals bit for bit.  (Before the chain existed every test here fails at its
first library call: the package has no countsketch_table / countsketch_cells / bmh_sketch_cs_* and the library no such symbol.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import countsketch_ref as CS
import protein_ref as PR
from conftest import ROOT
from dashing2_amd import synth

pytestmark = pytest.mark.gpu
INVALID = -1                                                             # D2G_ERR_INVALID (include/d2g.h)
XORMASK = 0x9E3779B97F4A7C15


def _seq(seed, n):
    return synth.random_genome(seed, n).tobytes()


def _fa(seq, name="g"):
    return b">" + name.encode() + b"\n" + seq + b"\n"


def _pack(d2g, fastas, k, alphabet=None):
    sp = d2g.SeqPack(k) if alphabet is None else d2g.SeqPack(k, alphabet)
    for f in fastas:
        sp.add_fastx(f)
    return sp


def _batch():
    """3 000 random bases with a 500-base poly-A stretch (one k-mer hundreds of times in one cell with one sign); records with Ns and
    runs shorter than any k used here; an input without runs; 200 000 bases: four workgroups of 65 536 k-mers whose LDS flushes meet
    in the same cells"""
    a = bytearray(_seq(11, 3000))
    a[1200:1700] = b"A" * 500
    b = _seq(12, 900)
    recs = _fa(b[:300], "r0") + _fa(b[300:330] + b"N" + b[330:334] + b"NN" + b[334:600], "r1") + _fa(b"ACG", "r2") + _fa(b[600:900] + b"N", "r3")
    return [_fa(bytes(a), "polyA"), recs, b">none\nNNNNACGNNN\n", _fa(_seq(13, 200000), "big")]


_KMERS = {}


def _kmers(k, canon):
    """the model's k-mers of the batch, computed once per (k, canon) and left unchanged"""
    if (k, canon) not in _KMERS:
        _KMERS[(k, canon)] = [CS.kmers_dna(f, k, canon) for f in _batch()]
    return _KMERS[(k, canon)]


@pytest.mark.parametrize("k,canon", [(5, True), (5, False), (21, True), (21, False), (32, True), (32, False)],
                         ids=["k5c", "k5f", "k21c", "k21f", "k32c", "k32f"])
def test_table_signed_cell_for_cell(d2g, gpu_ctx, k, canon):
    L = d2g.countsketch_lds_cells()
    assert 1024 < L <= 40960
    kms = _kmers(k, canon)
    assert kms[2].size == 0 and kms[3].size == 200000 - k + 1 > 3 * 65536
    sp = _pack(d2g, _batch(), k)
    for cells in (1, 2, 3, 64, 1000, 1024, L - 1, L, L + 1, (1 << 20) + 1):
        got = gpu_ctx.countsketch_table(sp, cells, canon=canon, xormask=XORMASK)
        assert got.dtype == np.int32 and got.shape == (4, cells)
        for g, km in enumerate(kms):
            want = CS.table(km, cells, XORMASK)
            assert np.array_equal(got[g].astype(np.int64), want), (cells, g, int(np.abs(got[g] - want).sum()))
        assert not got[2].any()
    if k == 21:
        one = gpu_ctx.countsketch_table(sp, 64, canon=canon, xormask=XORMASK)
        assert int(np.abs(one[0]).max()) >= 400                            # the poly-A k-mer: one cell, one sign, hundreds of adds
        assert not np.array_equal(one, gpu_ctx.countsketch_table(sp, 64, canon=canon, xormask=0))


@pytest.mark.parametrize("cells", [1_000_000_007, 1 << 31])
def test_exact_remainder_at_large_divisors(d2g, gpu_ctx, cells):
    k, canon = 21, True
    km = _kmers(k, canon)[3]
    sp = _pack(d2g, [_batch()[3]], k)
    ids, w, off, tot = gpu_ctx.countsketch_cells(sp, cells, canon=canon, xormask=XORMASK)
    eids, ew, eoff, etot = CS.batch_lists([km], cells, XORMASK)
    assert np.array_equal(off, eoff) and np.array_equal(tot, etot)
    assert np.array_equal(ids, eids) and np.array_equal(w, ew)
    assert int(ids.max()) > (1 << 29) and ids.size > 190000                # the cells are spread over the whole row


def test_lists_with_thresholds_and_capacity(d2g, gpu_ctx):
    k, canon, cells = 21, True, 1000
    sp = _pack(d2g, _batch(), k)
    for thr in (0.0, 1.0, 2.0, 3.0, 1e9):
        ids, w, off, tot = gpu_ctx.countsketch_cells(sp, cells, canon=canon, xormask=XORMASK, count_threshold=thr)
        eids, ew, eoff, etot = CS.batch_lists(_kmers(k, canon), cells, XORMASK, thr)
        assert np.array_equal(off, eoff) and np.array_equal(tot, etot) and np.array_equal(ids, eids) and np.array_equal(w, ew), thr
    assert ids.size == 0 and not tot.any()
    with pytest.raises(d2g.D2GError) as e:
        gpu_ctx.countsketch_cells(sp, cells, canon=canon, cap=10)
    assert e.value.status == INVALID and "capacity" in str(e.value)


def _chain_inputs():
    return _batch() + [_fa(_seq(14, 60), "tiny")]


@pytest.mark.parametrize("S", [64, 100, 1024])
def test_chain_equals_bagminhash_of_the_models_lists(d2g, gpu_ctx, S):
    k, canon = 21, True
    fastas = _chain_inputs()
    kms = _kmers(k, canon) + [CS.kmers_dna(fastas[4], k, canon)]
    sp = _pack(d2g, fastas, k)
    L = d2g.countsketch_lds_cells()
    for cells in (4096, L + 1):
        for thr in (0.0, 1.0, 2.0, 3.0):
            ids, w, off, tot = CS.batch_lists(kms, cells, XORMASK, thr)
            esig, etw = gpu_ctx.bmh_from_weighted(ids, w, off, S)
            sig, tw = gpu_ctx.bmh_sketch_cs_seqpack(sp, S, cells, canon=canon, xormask=XORMASK, count_threshold=thr)
            assert np.array_equal(tw, etw) and np.array_equal(tw, tot.astype(np.float64)), (cells, thr)
            assert np.array_equal(sig.view(np.uint64), esig.view(np.uint64)), (cells, thr)
            assert tw[2] == 0 and np.isinf(sig[2]).all() and np.isfinite(sig[0]).all()
        # the tiny input: 40 distinct k-mers, every cell +-1 -- all below a threshold of 2
        assert tot[4] == 0 and tw[4] == 0 and np.isinf(sig[4]).all()
        assert CS.batch_lists(kms, cells, XORMASK, 1.0)[3][4] == 40


def test_chain_redo_passes_in_groups_leave_the_registers_unchanged(d2g, gpu_ctx, monkeypatch):
    """D2G_K3_GUESS_SCALE=0.001 makes the first guess of every list's bound a thousand times too small, so BagMinHash over the lists has
    to walk them again under raised guesses; D2G_CS_TABLE_BYTES = two rows sends the three inputs with k-mers in two table groups (the
    empty one, placed second, takes no row), each walked into its own slice of the registers.  Registers and total weights must be
    those of the default scale bit for bit, which are those of BagMinHash over the lists the chain itself hands out."""
    k, S, cells = 21, 64, 4096
    fastas = [_fa(_seq(21, 20000), "a"), b">none\nNNNN\n", _fa(_seq(22, 20000), "b"), _fa(_seq(23, 20000), "c")]
    sp = _pack(d2g, fastas, k)
    monkeypatch.setenv("D2G_CS_TABLE_BYTES", str(2 * cells * 4))
    groups0 = gpu_ctx.countsketch_stats()[1]
    sig, tw = gpu_ctx.bmh_sketch_cs_seqpack(sp, S, cells, xormask=XORMASK)
    assert gpu_ctx.countsketch_stats()[1] - groups0 >= 2
    monkeypatch.setenv("D2G_K3_GUESS_SCALE", "0.001")
    rsig, rtw = gpu_ctx.bmh_sketch_cs_seqpack(sp, S, cells, xormask=XORMASK)
    monkeypatch.delenv("D2G_K3_GUESS_SCALE")
    assert np.array_equal(rsig.view(np.uint64), sig.view(np.uint64)) and np.array_equal(rtw.view(np.uint64), tw.view(np.uint64))
    ids, w, off, tot = gpu_ctx.countsketch_cells(sp, cells, xormask=XORMASK)
    esig, etw = gpu_ctx.bmh_from_weighted(ids, w, off, S)
    assert np.array_equal(sig.view(np.uint64), esig.view(np.uint64)) and np.array_equal(tw, etw) and np.array_equal(tw, tot.astype(np.float64))
    assert tw[1] == 0 and np.isinf(sig[1]).all() and np.isfinite(sig[[0, 2, 3]]).all() and (tw[[0, 2, 3]] > 0).all()


def test_walker_modes(d2g, gpu_ctx):
    """one case each with a filter attached, with w > k and with a protein alphabet: the lists of the model fed by the matching enumerator"""
    S, cells = 64, 5000
    k, canon = 21, True
    fastas = _batch()
    sp = _pack(d2g, fastas, k)

    def check(sk, packed, kms, canon_, thr=1.0):
        ids, w, off, tot = CS.batch_lists(kms, cells, XORMASK, thr)
        esig, etw = gpu_ctx.bmh_from_weighted(ids, w, off, S)
        sig, tw = sk.run_bmh_cs(packed, S, cells, canon=canon_, xormask=XORMASK, count_threshold=thr)
        assert np.array_equal(tw, etw) and np.array_equal(sig.view(np.uint64), esig.view(np.uint64))
        return tw

    sk = gpu_ctx.sketcher()
    plain = check(sk, sp, _kmers(k, canon), canon)
    # --filterset: a slice of the big input and the poly-A stretch
    filt = [_fa(fastas[3].split(b"\n")[1][5000:30000], "slice"), _fa(b"A" * 40, "a")]
    f = gpu_ctx.kmer_filter(_pack(d2g, filt, k), canon)
    sk.set_filter(f)
    small = [_fa(fastas[3].split(b"\n")[1][:40000], "head"), fastas[0], fastas[1]]
    kms = [CS.kmers_filtered(x, filt, k, canon) for x in small]
    assert kms[0].size < 40000 - k + 1 - 20000 and kms[1].size < 3000 - k + 1 - 400
    check(sk, _pack(d2g, small, k), kms, canon)
    sk.set_filter(None)
    # -w > k: minimizers
    w = 35
    sk.set_window(w)
    kms = [CS.kmers_dna(x, k, canon, w=w) for x in fastas]
    tw = check(sk, sp, kms, canon)
    assert kms[3].size == 200000 - w + 1 and not np.array_equal(tw, plain)
    sk.set_window(0)
    assert np.array_equal(check(sk, sp, _kmers(k, canon), canon), plain)
    sk.close()
    f.close()
    # a protein alphabet
    pk = 7
    prots = [PR.fa(PR.random_protein(21, 70000)), PR.fa(PR.random_protein(22, 500) + b"X" + PR.random_protein(23, 4) + b"*" + PR.random_protein(24, 90)),
             PR.fa(b"XXXX")]
    sk = gpu_ctx.sketcher()
    sk.set_alphabet(PR.PROTEIN20)
    tw = check(sk, _pack(d2g, prots, pk, PR.PROTEIN20), [CS.kmers_protein(p, pk, PR.PROTEIN20) for p in prots], False)
    assert tw[0] > 0 and tw[2] == 0
    sk.close()


class _Dev:
    """packed stream under a plan, registers and totals of one batch in device memory, the outputs pre-set to a pattern"""

    def __init__(self, ctx, sp, S):
        self.ctx, self.S = ctx, S
        packed, rs, rl, go = sp.arrays()
        self.n = go.size - 1
        self.plan = ctx.oph_plan(rs, rl, go, sp.k)
        self.packed = ctx.malloc(max(packed.size, 4))
        ctx.h2d(self.packed, packed)
        self.sig, self.tw = ctx.malloc(self.n * S * 8), ctx.malloc(self.n * 8)
        ctx.h2d(self.sig, np.full(self.n * S * 8, 0xAB, np.uint8))
        ctx.h2d(self.tw, np.full(self.n * 8, 0xAB, np.uint8))

    def read(self):
        sig, tw = np.empty((self.n, self.S), np.float64), np.empty(self.n, np.float64)
        self.ctx.sync()
        self.ctx.d2h(sig, self.sig)
        self.ctx.d2h(tw, self.tw)
        return sig, tw

    def close(self):
        for p in (self.packed, self.sig, self.tw):
            self.ctx.free(p)
        self.plan.close()


def test_the_three_forms_agree(d2g, gpu_ctx):
    k, canon, S = 21, True, 100
    L = d2g.countsketch_lds_cells()
    sp = _pack(d2g, _batch(), k)
    other = _pack(d2g, [_fa(_seq(31, 70000), "o0"), _fa(_seq(32, 500), "o1")], k)
    big, small = 3 * L + 7, 50
    ref = {(name, c): gpu_ctx.bmh_sketch_cs_seqpack(p, S, c, canon=canon, xormask=XORMASK, count_threshold=1.0)
           for name, p in (("sp", sp), ("other", other)) for c in (big, small)}
    # the sketcher: cells large, then small, then large again on different inputs -- a cell left over from an earlier batch would show
    sk = gpu_ctx.sketcher()
    for name, p, c in (("sp", sp, big), ("other", other, small), ("other", other, big), ("sp", sp, small), ("sp", sp, big)):
        sig, tw = sk.run_bmh_cs(p, S, c, canon=canon, xormask=XORMASK, count_threshold=1.0)
        assert np.array_equal(tw, ref[(name, c)][1]) and np.array_equal(sig.view(np.uint64), ref[(name, c)][0].view(np.uint64)), (name, c)
    sk.close()
    # the device-resident form, twice on the context's own state
    for c in (big, small):
        dv = _Dev(gpu_ctx, sp, S)
        gpu_ctx.bmh_sketch_cs_dev(dv.plan, dv.packed, S, c, dv.sig, dv.tw, canon=canon, xormask=XORMASK, count_threshold=1.0)
        sig, tw = dv.read()
        assert np.array_equal(tw, ref[("sp", c)][1]) and np.array_equal(sig.view(np.uint64), ref[("sp", c)][0].view(np.uint64)), c
        dv.close()
    # what is refused, before anything is written
    dv = _Dev(gpu_ctx, sp, S)
    for bad in (0, (1 << 31) + 1):
        with pytest.raises(d2g.D2GError) as e:
            gpu_ctx.bmh_sketch_cs_dev(dv.plan, dv.packed, S, bad, dv.sig, dv.tw, canon=canon)
        assert e.value.status == INVALID and "cells" in str(e.value)
        with pytest.raises(d2g.D2GError) as e:
            gpu_ctx.bmh_sketch_cs_seqpack(sp, S, bad, canon=canon)
        assert e.value.status == INVALID and "cells" in str(e.value)
    assert (dv.read()[0].view(np.uint64) == 0xABABABABABABABAB).all()
    dv.close()


_CHILD = """
import sys, json
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import dashing2_amd as D
import test_gpu_countsketch as T
ctx = D.Context(0)
sp = T._pack(D, T._batch(), 21)
sig, tw = ctx.bmh_sketch_cs_seqpack(sp, 100, int(sys.argv[2]), canon=True, xormask=T.XORMASK, count_threshold=1.0)
np.save(sys.argv[3], np.concatenate([sig.view(np.uint64).ravel(), tw.view(np.uint64)]))
print(json.dumps(ctx.countsketch_stats()))
ctx.close()
"""


def test_groups_of_genomes_give_the_same_output(d2g, gpu_ctx, tmp_path):
    """D2G_CS_TABLE_BYTES = one row: the four inputs go in three groups (the input without k-mers takes no row and rides along)"""
    cells, S = 5000, 100
    sp = _pack(d2g, _batch(), 21)
    sig, tw = gpu_ctx.bmh_sketch_cs_seqpack(sp, S, cells, canon=True, xormask=XORMASK, count_threshold=1.0)
    want = np.concatenate([sig.view(np.uint64).ravel(), tw.view(np.uint64)])
    for table_bytes, groups in ((4 * cells, 3), (8 * cells, 2)):
        out = str(tmp_path / f"g{groups}.npy")
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(cells), out], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, D2G_CS_TABLE_BYTES=str(table_bytes)))
        assert r.returncode == 0, r.stderr[-3000:]
        stats = json.loads(r.stdout.strip().splitlines()[-1])
        assert stats == [table_bytes, groups, 1], stats
        assert np.array_equal(np.load(out), want)


def test_agreement_with_the_exact_chain(d2g, gpu_ctx):
    """cells so large that no two distinct k-mers of an input share one -- checked on the model, a condition on the input, not a
    tolerance: every k-mer then keeps its own cell and its own sign, and the total weight is the exact chain's"""
    k, canon, S, cells = 21, True, 64, (1 << 31) - 1
    fastas = _batch()[:3]
    kms = _kmers(k, canon)[:3]
    for km in kms:
        assert CS.collision_free(km, cells, XORMASK)
    sp = _pack(d2g, fastas, k)
    _, tw = gpu_ctx.bmh_sketch_cs_seqpack(sp, S, cells, canon=canon, xormask=XORMASK)
    _, etw = gpu_ctx.bmh_sketch_seqpack(sp, S, canon=canon, xormask=XORMASK)
    assert np.array_equal(tw, etw) and tw.tolist() == [float(km.size) for km in kms]
    ids, w, off, tot = gpu_ctx.countsketch_cells(sp, cells, canon=canon, xormask=XORMASK)
    assert [int(off[g + 1] - off[g]) for g in range(3)] == [np.unique(km).size for km in kms]
