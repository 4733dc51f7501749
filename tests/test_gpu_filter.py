"""--filterset on the GPU (K1f, d2g_filter.hip + the probe in d2g_kmers.h): the device table against the sets it was built from, and
K1, K1b, K3, K0 and the CLI with a filter attached against the model of tests/filter_ref.py -- the input rewritten as one k-base
record per surviving k-mer occurrence, sketched by the UNCHANGED oracle.  Everything is compared bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

import filter_ref as FR
import oph_kmers_ref as R
from conftest import ROOT
from dashing2_amd import synth

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "dashing2_amd", "bin", "dashing2")
INVALID = -1                                                           # D2G_ERR_INVALID (include/d2g.h)
INF_BITS = np.float64(np.inf).view(np.uint64)
BASES = np.frombuffer(b"ACGT", np.uint8)


def _kmer_string(v, k):
    return bytes(BASES[[(v >> (2 * (k - 1 - i))) & 3 for i in range(k)]])


def _filter_of(d2g, ctx, fastas, k, canon):
    sp = d2g.SeqPack(k)
    for f in fastas:
        sp.add_fastx(f)
    return ctx.kmer_filter(sp, canon)


# ---- membership through the device probe, exhaustively ------------------------------------------------------------------------
@pytest.mark.parametrize("size", [0, 1, 2, 2047, 2048, 2049, 4095, 4096])
def test_contains_is_the_subset_for_every_6mer(d2g, gpu_ctx, size):
    """the sizes sit on both sides of the capacity doublings (slots = the power of two >= twice the k-mers put in); every 6-mer is
    asked, so a probe starts at every slot that any 6-mer hashes to, the last one and its wrap-around included"""
    k = 6
    rng = np.random.default_rng(size)
    sub = np.sort(rng.choice(4096, size, replace=False)).astype(np.uint64)
    dup = sub[:size // 3]                                              # some k-mers twice: occurrences are not keys
    fasta = b"".join(b">x\n" + _kmer_string(int(v), k) + b"\n" for v in np.concatenate([sub, dup]))
    f = _filter_of(d2g, gpu_ctx, [fasta], k, canon=False)
    nocc, ndist, nbytes = f.info()
    assert nocc == size + dup.size and ndist == size
    slots = 16
    while slots < 2 * nocc:
        slots *= 2
    assert nbytes == (slots + 2) * 8
    got = f.contains(np.arange(4096, dtype=np.uint64))
    exp = np.zeros(4096, bool)
    exp[sub.astype(np.int64)] = True
    assert np.array_equal(got, exp)
    f.close()


@pytest.mark.parametrize("canon", [False, True])
def test_contains_at_k32_where_every_value_is_a_kmer(d2g, gpu_ctx, canon):
    """A x 32 is 0 and T x 32 (forward) is all ones: neither can mark a free slot.  With canon on, T x 32 is A x 32."""
    k, M = 32, 2 ** 64 - 1
    recs = [b"A" * 32, b"T" * 32, b"AC" * 16]
    fasta = b"".join(b">x\n" + r + b"\n" for r in recs)
    f = _filter_of(d2g, gpu_ctx, [fasta], k, canon)
    ac, gt = FR.encode(b"AC" * 16), FR.encode(b"GT" * 16)
    keys = {0, ac} if canon else {0, M, ac}                            # canonical: min(T x 32, A x 32) = 0; min((AC)16, (GT)16) = (AC)16
    assert f.info()[:2] == (3, len(keys))
    ask = np.array([0, M, ac, gt, 1, M - 1, ac + 1, 1 << 63], np.uint64)
    assert f.contains(ask).tolist() == [int(v) in keys for v in ask]
    # ... and through the walker: T x 32 is skipped -- with canon on through A x 32 -- and a stranger passes
    sk = gpu_ctx.sketcher()
    sk.set_filter(f)
    sp = d2g.SeqPack(k)
    for r in (b"T" * 32, b"A" * 40, b"AC" * 15 + b"AA", b"GT" * 16):
        sp.add_sequence(r)
    regs = sk.run(sp, 8, canon=canon)
    empty = [(row == R.M64).all() for row in regs]
    assert empty == [True, True, False, canon]                         # (GT)16 is the reverse complement of (AC)16
    sk.close()
    f.close()


def test_no_kmers_is_a_legal_filter_that_filters_nothing(d2g, gpu_ctx, oracle):
    f = _filter_of(d2g, gpu_ctx, [b">short\nACGTACGT\n", b">none\n\n"], 21, True)
    assert f.info()[:2] == (0, 0) and not f.contains(np.arange(64, dtype=np.uint64)).any()
    fa = synth.fasta_bytes("g", synth.random_genome(77, 5000))
    sp = d2g.SeqPack(21)
    sp.add_fastx(fa)
    sk = gpu_ctx.sketcher()
    sk.set_filter(f)
    assert np.array_equal(sk.run(sp, 64)[0], oracle.sketch_buffer(fa, k=21, S=64)[0])
    sk.close()
    f.close()


def test_racing_duplicates_leave_each_key_once(d2g, gpu_ctx):
    """one 300-base sequence 2000 times: every lane of the build inserts a key that thousands of others insert at the same moment"""
    k = 21
    seq = synth.random_genome(31, 300).tobytes()
    fasta = b"".join(b">r\n" + seq + b"\n" for _ in range(2000))
    f = _filter_of(d2g, gpu_ctx, [fasta], k, True)
    ws = FR.windows(seq, k, True)
    nocc, ndist, _ = f.info()
    assert nocc == 2000 * len(ws) == 2000 * 280 and ndist == len(set(ws))
    ask = np.array([FR.encode(w) for w in set(ws)] + [FR.encode(w) ^ 1 for w in set(ws)], np.uint64)   # the neighbours are not canonical k-mers of it
    exp = [True] * len(set(ws)) + [_kmer_string(int(v), k) in set(ws) for v in ask[len(set(ws)):]]
    assert f.contains(ask).tolist() == exp
    f.close()


# ---- K1, K1b, K3, K0 against the model ------------------------------------------------------------------------------------------
def _genomes():
    g0 = synth.random_genome(500, 70000)                               # two workgroups merge their registers
    g1 = synth.random_genome(501, 3000).tobytes()
    g1 = g1[:700] + b"N" * 9 + g1[700:1500] + b"N" + g1[1500:1510] + b"NN" + g1[1510:]
    inside = g0[1200:2400]                                             # every k-mer of it is in the filter
    filt = [synth.fasta_bytes("slice", g0[1000:6000]),
            synth.fasta_bytes("rc", np.frombuffer(FR.revcomp(g0[20000:22000].tobytes()), np.uint8)),
            synth.fasta_bytes("other", synth.random_genome(502, 1000))]
    # k-mers seen three times that survive and k-mers seen twice that are filtered: what a count threshold is applied to
    rep = b"".join(synth.fasta_bytes(f"r{i}", g0[30000:31000]) for i in range(3)) + 2 * synth.fasta_bytes("f", g0[3000:3500])
    return [synth.fasta_bytes("g0", g0), synth.fasta_bytes("g1", np.frombuffer(g1, np.uint8)), synth.fasta_bytes("in", inside), b">empty\n\n", rep], filt


_MODEL = {}


def _model(k, canon):
    """-> (genomes, filter fastas, rewritten genomes, k-mer occurrences in the filter), computed once per (k, canon)"""
    if (k, canon) not in _MODEL:
        gs, filt = _genomes()
        fset, nocc = FR.filter_set(filt, k, canon)
        _MODEL[(k, canon)] = (gs, filt, [FR.rewrite(g, fset, k, canon) for g in gs], nocc)
    return _MODEL[(k, canon)]


def _expected_k1(oracle, rw, k, S, canon):
    regs = np.stack([oracle.sketch_buffer(b, k=k, canon=canon, S=S)[0] for b in rw])
    counts = np.stack([R.counts_for(*oracle.kmer_count_buffer(b, k, canon)[:2], regs[i]) for i, b in enumerate(rw)])
    return regs, counts


def _pack(d2g, fastas, k):
    sp = d2g.SeqPack(k)
    for f in fastas:
        sp.add_fastx(f)
    return sp


class DevArrays:
    """packed stream, registers and counts of one batch in device memory (d2g_malloc), the outputs pre-set to a pattern"""

    def __init__(self, ctx, sp, m, fill=0xAB):
        self.ctx = ctx
        packed, rs, rl, go = sp.arrays()
        self.n, self.m = go.size - 1, m
        self.plan = ctx.oph_plan(rs, rl, go, sp.k)
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


@pytest.mark.parametrize("k,S,canon", [(21, 64, True), (31, 100, True), (32, 1024, False), (5, 7, True), (21, 20000, True)])
def test_k1_and_k1b_with_a_filter(d2g, gpu_ctx, oracle, k, S, canon):
    """S = 20 000: the kernels' variant without registers in LDS.  k = 5: the filter holds every canonical 5-mer, nothing survives"""
    gs, filt, rw, nocc = _model(k, canon)
    eregs, ecounts = _expected_k1(oracle, rw, k, S, canon)
    assert (eregs[2] == R.M64).all() and np.array_equal(eregs[2], eregs[3])     # all filtered = no k-mers
    assert k == 5 or ((eregs[0] != R.M64).any() and rw[0] != b"" and rw[0].count(b">") < 70000 - k + 1)
    f = _filter_of(d2g, gpu_ctx, filt, k, canon)
    assert f.info()[0] == nocc
    sp = _pack(d2g, gs, k)
    # the sketcher
    sk = gpu_ctx.sketcher()
    sk.set_filter(f)
    regs, counts = sk.run_counts(sp, S, canon=canon)
    assert np.array_equal(regs, eregs) and np.array_equal(counts, ecounts)
    assert np.array_equal(sk.run(sp, S, canon=canon), eregs)
    # a plan with the filter attached
    dv = DevArrays(gpu_ctx, sp, d2g.oph_m(S))
    dv.plan.set_filter(f)
    gpu_ctx.oph_sketch_dev(dv.plan, dv.packed, S, dv.regs, canon=canon)
    gpu_ctx.oph_count_dev(dv.plan, dv.packed, S, dv.regs, dv.counts, canon=canon)
    dregs, dcounts = dv.read()
    assert np.array_equal(dregs, eregs) and np.array_equal(dcounts, ecounts)
    # detached: the unfiltered oracle
    uregs, ucounts = _expected_k1(oracle, gs, k, S, canon)
    sk.set_filter(None)
    dv.plan.set_filter(None)
    regs, counts = sk.run_counts(sp, S, canon=canon)
    assert np.array_equal(regs, uregs) and np.array_equal(counts, ucounts)
    gpu_ctx.oph_sketch_dev(dv.plan, dv.packed, S, dv.regs, canon=canon)
    gpu_ctx.oph_count_dev(dv.plan, dv.packed, S, dv.regs, dv.counts, canon=canon)
    dregs, dcounts = dv.read()
    assert np.array_equal(dregs, uregs) and np.array_equal(dcounts, ucounts)
    assert k == 5 or not np.array_equal(uregs[0], eregs[0])
    dv.close()
    sk.close()
    f.close()


@pytest.mark.parametrize("k,canon", [(21, True), (32, False)])
def test_k3_with_a_filter(d2g, gpu_ctx, oracle, k, canon):
    S = 64
    gs, filt, rw, _ = _model(k, canon)
    f = _filter_of(d2g, gpu_ctx, filt, k, canon)
    sp = _pack(d2g, gs, k)
    sk = gpu_ctx.sketcher()
    sk.set_filter(f)
    for thr in (0.0, 1.0):
        exp = [oracle.bmh_sketch_buffer(b, k, S, canon, count_threshold=thr) for b in rw]
        sig, tw = sk.run_bmh(sp, S, canon=canon, count_threshold=thr)
        for i, e in enumerate(exp):
            assert tw[i] == e[1] and np.array_equal(sig[i].view(np.uint64), e[0].view(np.uint64)), (thr, i)
        assert tw[2] == 0 and (sig[2].view(np.uint64) == INF_BITS).all()
        assert tw[4] == 3 * (1000 - k + 1) and (tw[0] > 0) == (thr == 0)     # a random genome holds every k-mer once
    # the distinct count that --parse-by-seq substitutes
    nd = sk.run_distinct(sp, canon=canon)
    assert nd.tolist() == [oracle.kmer_count_buffer(b, k, canon)[0].size for b in rw] and nd[2] == 0 and nd[0] > 0
    # the device-resident form on a plan with the filter attached
    dv = DevArrays(gpu_ctx, sp, S)
    dv.plan.set_filter(f)
    tw_dev = gpu_ctx.malloc(dv.n * 8)
    gpu_ctx.bmh_sketch_dev(dv.plan, dv.packed, S, dv.regs, tw_dev, canon=canon)
    sig, tw = np.empty((dv.n, S), np.float64), np.empty(dv.n, np.float64)
    gpu_ctx.sync()
    gpu_ctx.d2h(sig, dv.regs)
    gpu_ctx.d2h(tw, tw_dev)
    for i, b in enumerate(rw):
        e = oracle.bmh_sketch_buffer(b, k, S, canon)
        assert tw[i] == e[1] and np.array_equal(sig[i].view(np.uint64), e[0].view(np.uint64)), i
    # detached: the unfiltered oracle
    sk.set_filter(None)
    sig, tw = sk.run_bmh(sp, S, canon=canon)
    e = oracle.bmh_sketch_buffer(gs[0], k, S, canon)
    assert tw[0] == e[1] == 70000 - k + 1 and np.array_equal(sig[0].view(np.uint64), e[0].view(np.uint64))
    gpu_ctx.free(tw_dev)
    dv.close()
    sk.close()
    f.close()


def test_k3_with_a_filter_many_buckets_and_the_compact_path(d2g, gpu_ctx, oracle, monkeypatch):
    """the two-level split (hist / scatter / refine) and the compact walkers (k3c_hist / k3c_scatter) drop the same k-mers"""
    k, S, canon = 21, 64, True
    gs, filt, rw, _ = _model(k, canon)
    exp = [oracle.bmh_sketch_buffer(b, k, S, canon) for b in rw]
    f = _filter_of(d2g, gpu_ctx, filt, k, canon)
    sp = _pack(d2g, gs, k)
    for env in ({"D2G_K3_BUCKET_KEYS": "16"}, {"D2G_K3_COMPACT": "1"}):
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        sk = gpu_ctx.sketcher()
        sk.set_filter(f)
        sig, tw = sk.run_bmh(sp, S, canon=canon)
        for i, e in enumerate(exp):
            assert tw[i] == e[1] and np.array_equal(sig[i].view(np.uint64), e[0].view(np.uint64)), (env, i)
        sk.close()
        for name in env:
            monkeypatch.delenv(name)
    f.close()


def test_k0_ingested_stream_with_a_filter(d2g, gpu_ctx, oracle):
    k, S, canon = 21, 64, True
    gs, filt, rw, _ = _model(k, canon)
    f = _filter_of(d2g, gpu_ctx, filt, k, canon)
    sk = gpu_ctx.sketcher()
    sk.set_filter(f)
    host = sk.run(_pack(d2g, gs, k), S)
    runs = sk.ingest_fasta(gs, k)
    assert np.array_equal(sk.run_ingested(runs, S), host)
    assert np.array_equal(host, np.stack([oracle.sketch_buffer(b, k=k, S=S)[0] for b in rw]))
    sk.close()
    f.close()


# ---- refusals write nothing ---------------------------------------------------------------------------------------------------------
def test_a_filter_of_another_k_canon_or_context_is_refused(d2g, gpu_ctx):
    gs, filt, _, _ = _model(21, True)
    sp = _pack(d2g, gs, 21)
    other = d2g.Context(0)
    bad = [(_filter_of(d2g, gpu_ctx, filt, 31, True), "another k"), (_filter_of(d2g, gpu_ctx, filt, 21, False), "another canonicalisation"),
           (_filter_of(d2g, other, filt, 21, True), "another context")]
    sk = gpu_ctx.sketcher()
    dv = DevArrays(gpu_ctx, sp, d2g.oph_m(64))
    for f, why in bad:
        sk.set_filter(f)
        dv.plan.set_filter(f)
        calls = [lambda: sk.run(sp, 64), lambda: sk.run_counts(sp, 64), lambda: sk.run_bmh(sp, 64), lambda: sk.run_distinct(sp),
                 lambda: gpu_ctx.oph_sketch_dev(dv.plan, dv.packed, 64, dv.regs), lambda: gpu_ctx.oph_count_dev(dv.plan, dv.packed, 64, dv.regs, dv.counts),
                 lambda: gpu_ctx.bmh_sketch_dev(dv.plan, dv.packed, 64, dv.regs, dv.counts)]
        for call in calls:
            with pytest.raises(d2g.D2GError) as e:
                call()
            assert e.value.status == INVALID and why in str(e.value)
        regs, counts = dv.read()
        assert (regs == 0xABABABABABABABAB).all() and (counts == 0xABABABAB).all()
    sk.set_filter(None)
    dv.plan.set_filter(None)
    dv.close()
    sk.close()
    for f, _ in bad:
        f.close()
    other.close()


# ---- the CLI, bytes against the model ---------------------------------------------------------------------------------------------
def _run(args, **kw):
    r = subprocess.run([EXE] + args, capture_output=True, **kw)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    """three genomes (the third entirely inside the filter), the filter as TWO files, and the genomes rewritten at k = 21"""
    d = tmp_path_factory.mktemp("filter_cli")
    gs, filt, rw, nocc = _model(21, True)
    paths, rpaths = [], []
    for i in range(3):
        p, q = d / f"g{i}.fa", d / f"g{i}.rewritten.fa"
        p.write_bytes(gs[i])
        q.write_bytes(rw[i])
        paths.append(str(p))
        rpaths.append(str(q))
    (d / "f0.fa").write_bytes(filt[0] + filt[1])
    (d / "f1.fa").write_bytes(filt[2])
    return paths, rpaths, f"{d}/f0.fa {d}/f1.fa", nocc


def _stacked(N, S, cards, sigs):
    return np.array([N, S], np.uint64).tobytes() + np.asarray(cards, np.float64).tobytes() + np.asarray(sigs, np.float64).tobytes()


def test_cli_sketch_filterset(oracle, cli_files, tmp_path):
    paths, rpaths, farg, nocc = cli_files
    k, S = 21, 64
    out, stats = tmp_path / "s.bin", tmp_path / "stats.json"
    _run(["sketch", "--filterset", farg, "-k", str(k), "-S", str(S), "-o", str(out), "--gpu-stats", str(stats)] + paths)
    esigs, ecards = oracle.sketch_files(rpaths, k=k, S=S)
    assert out.read_bytes() == _stacked(3, S, ecards, esigs)
    assert [l.split("\t")[0] for l in open(str(out) + ".names.txt").read().splitlines()[1:]] == paths
    fs = json.load(open(stats))["filter"]
    assert set(fs) == {"kmers", "distinct", "table_bytes", "build_ms"} and fs["kmers"] == nocc and 0 < fs["distinct"] <= nocc
    assert fs["table_bytes"] == (16384 + 2) * 8 and fs["build_ms"] > 0         # 7940 k-mers: 16384 slots
    # `:K` selects the same arm; the device FASTA parser feeds the same walker
    out2 = tmp_path / "s2.bin"
    _run(["sketch", "--filterset", farg + ":K", "-k", str(k), "-S", str(S), "-o", str(out2)] + paths, env=dict(os.environ, D2G_DEVICE_PARSE="1"))
    assert out2.read_bytes() == out.read_bytes()


def test_cli_sketch_filterset_kmers_and_counts(oracle, cli_files, tmp_path):
    paths, rpaths, farg, _ = cli_files
    k, S = 21, 64
    out = tmp_path / "n.bin"
    _run(["sketch", "--filterset", farg, "-N", "-k", str(k), "-S", str(S), "-o", str(out)] + paths)
    rw = [open(p, "rb").read() for p in rpaths]
    regs, counts = _expected_k1(oracle, rw, k, S, True)
    esigs, ecards = oracle.sketch_files(rpaths, k=k, S=S)
    assert out.read_bytes() == _stacked(3, S, ecards, esigs)
    assert open(str(out) + ".kmer64", "rb").read() == R.kmer64_bytes(R.decode(regs[:, :S]), S, k, k, True, 0)
    assert open(str(out) + ".kmercounts.f64", "rb").read() == R.kmercounts_bytes(counts[:, :S], S)
    assert counts[0].max() >= 1 and counts[2].max() == 0


def test_cli_sketch_filterset_multiset(oracle, cli_files, tmp_path):
    paths, rpaths, farg, _ = cli_files
    k, S = 21, 64
    out = tmp_path / "m.bin"
    _run(["sketch", "--filterset", farg, "--multiset", "-k", str(k), "-S", str(S), "-o", str(out)] + paths)
    esigs, ecards, _ = oracle.bmh_sketch_files(rpaths, k, S)
    assert out.read_bytes() == _stacked(3, S, ecards, esigs) and ecards[2] == 0


def test_cli_sketch_filterset_parse_by_seq(oracle, cli_files, tmp_path):
    """per record: registers of the record's surviving k-mers; the cardinality below 10 S is their exact distinct count"""
    _, _, farg, _ = cli_files
    k, S = 21, 64
    gs, filt, _, _ = _model(k, True)
    fset, _ = FR.filter_set(filt, k, True)
    small = synth.random_genome(503, 500)
    multi = gs[1] + synth.fasta_bytes("small", small) + gs[2] + b">empty\n\n" + synth.fasta_bytes("g0head", synth.random_genome(500, 9000))
    fa, out = tmp_path / "multi.fa", tmp_path / "b.bin"
    fa.write_bytes(multi)
    _run(["sketch", "--filterset", farg, "--parse-by-seq", "-k", str(k), "-S", str(S), "-o", str(out), str(fa)])
    sigs, cards, names = [], [], []
    for name, rw in FR.rewrite_by_record(multi, fset, k, True):
        _, sig, card, _ = oracle.sketch_buffer(rw, k=k, S=S)
        card = 0.0 if card != card else card                           # fastxsketchbyseq.cpp:410-414
        if card < 10.0 * S:                                             # :415-430
            card = float(oracle.kmer_count_buffer(rw, k, True)[0].size)
        sigs.append(sig), cards.append(card), names.append(name)
    assert names == ["g1", "small", "in", "empty", "g0head"] and cards[2] == 0 and cards[1] == 480 and cards[4] != float(int(cards[4]))
    assert out.read_bytes() == _stacked(5, S, cards, np.stack(sigs))
    assert [l.split("\t")[0] for l in open(str(out) + ".names.txt").read().splitlines()[1:]] == names


def test_cli_cmp_filterset(oracle, cli_files, tmp_path):
    paths, rpaths, farg, nocc = cli_files
    k, S = 21, 64
    mut, mutr = tmp_path / "mut.fa", tmp_path / "mut.rewritten.fa"
    gs, filt, _, _ = _model(k, True)
    mfa = synth.fasta_bytes("mut", synth.mutate(synth.random_genome(500, 70000), 0.01, 5))
    mut.write_bytes(mfa)
    mutr.write_bytes(FR.rewrite(mfa, FR.filter_set(filt, k, True)[0], k, True))
    three, threer = paths[:2] + [str(mut)], rpaths[:2] + [str(mutr)]
    b = tmp_path / "d.bin"
    _run(["cmp", "--filterset", farg, "-k", str(k), "-S", str(S), "--binary-output", "--cmpout", str(b)] + three)
    esigs, ecards = oracle.sketch_files(threer, k=k, S=S)
    dens = np.stack([oracle.densify(s)[0] for s in esigs])
    exp = oracle.allpairs_ut(dens, ecards, measure=oracle.SIMILARITY, k=k)
    assert np.array_equal(np.fromfile(b, np.float32).view(np.uint32), exp.view(np.uint32)) and exp.max() > 0.3
    # the options line of the text output carries the reference's suffix: occurrences, duplicates counted (d2.cpp:38-40)
    r = _run(["cmp", "--filterset", farg, "-k", str(k), "-S", str(S)] + three)
    assert f";canon;FilterSetSortedHashSet-size={nocc}\n" in r.stdout.decode()


def test_cli_cache_with_filterset_warns_and_keeps_the_cache_names(oracle, cli_files, tmp_path):
    paths, rpaths, farg, _ = cli_files
    k, S = 21, 64
    args = ["sketch", "--cache", "--outprefix", str(tmp_path), "-k", str(k), "-S", str(S)]
    r = _run(args + ["--filterset", farg] + paths[:2])
    warn = [l for l in r.stderr.decode().splitlines() if "--cache" in l and "--filterset" in l and not l.startswith("#Calling")]   # not the echo of the command
    assert len(warn) == 1 and "warning" in warn[0]
    esigs, ecards = oracle.sketch_files(rpaths[:2], k=k, S=S)
    for i, p in enumerate(paths[:2]):
        blob = np.fromfile(R.cache_name(p, S, k, outprefix=str(tmp_path)), np.float64)       # the name an unfiltered run gives
        assert blob[0] == ecards[i] and np.array_equal(blob[1:].view(np.uint64), esigs[i].view(np.uint64))
    # an existing cache is loaded as it is: the unfiltered run now reads the filtered sketches, and says nothing
    out = tmp_path / "again.bin"
    r = _run(args + ["-o", str(out)] + paths[:2])
    assert "--filterset" not in r.stderr.decode() and out.read_bytes() == _stacked(2, S, ecards, esigs)
