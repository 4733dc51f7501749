"""sketch -m c in set space: d2g_sketcher_run_mincount, d2g_oph_sketch_mincount and d2g_oph_sketch_mincount_dev (K3's exact counts ->
k3_ophmin_kernel -> K1b over the new registers) against oph_mincount_ref.closed_form over k3_seam_cases.key_counts -- a pure-Python
k-mer enumerator and NumPy's wang64; nothing the product computed.  Registers and counts are compared bit for bit.

Every output lies between guard words and starts as 0xAB bytes, which no result contains; the guard words must come back untouched.
The D2G_K3_* switches are set with monkeypatch.setenv: the session's context reads them again (conftest.py)."""
import numpy as np
import pytest

import k3_seam_cases as C
import oph_kmers_ref as R
import oph_mincount_ref as Q

pytestmark = pytest.mark.gpu

GUARD = 32                                                             # words in front of and behind every output
FILL = 0xAB
INVALID, UNSUPPORTED = -1, -5                                          # D2G_ERR_INVALID, D2G_ERR_UNSUPPORTED (include/d2g.h)
M64 = R.M64
FORMS = ("sketcher", "one_shot", "dev")


class HostOut:
    """n x m words of `dtype` between GUARD words on either side, every byte FILL"""

    def __init__(self, n, m, dtype):
        self.n, self.m = n, m
        self.a = np.frombuffer(bytes([FILL]) * ((2 * GUARD + n * m) * np.dtype(dtype).itemsize), dtype).copy()
        self.fill = self.a[0]

    @property
    def ptr(self):
        return self.a.ctypes.data + GUARD * self.a.itemsize

    def guards_intact(self):
        return (self.a[:GUARD] == self.fill).all() and (self.a[GUARD + self.n * self.m:] == self.fill).all()

    def read(self):
        assert self.guards_intact(), "the guard words around an output were written"
        return self.a[GUARD:GUARD + self.n * self.m].reshape(self.n, self.m)

    def untouched(self):
        return (self.a == self.fill).all()


class DevOut:
    """the same in device memory (a torch tensor)"""

    def __init__(self, torch, n, m, dtype):
        self.n, self.m, self.dtype = n, m, np.dtype(dtype)
        self.t = torch.full(((2 * GUARD + n * m) * self.dtype.itemsize,), FILL, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD * self.dtype.itemsize

    def read(self):
        a = self.t.cpu().numpy().view(self.dtype)
        fill = np.frombuffer(bytes([FILL]) * self.dtype.itemsize, self.dtype)[0]
        assert (a[:GUARD] == fill).all() and (a[GUARD + self.n * self.m:] == fill).all(), "the guard words around a device output were written"
        return a[GUARD:GUARD + self.n * self.m].reshape(self.n, self.m)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def sketcher(gpu_ctx):
    """ONE sketcher for the whole module: its grow-only buffers and K3 work state see every shape in turn"""
    sk = gpu_ctx.sketcher()
    yield sk
    sk.close()


def seqpack(d2g, batch):
    sp = d2g.SeqPack(batch.k)
    for f in batch.fastas():
        sp.add_fastx(f)
    assert [sp.nkmers(g) for g in range(len(batch.genomes))] == batch.nkmers()
    return sp


def host_call(d2g, gpu_ctx, sketcher, form, sp, S, c, canon, xormask, regs_ptr, counts_ptr, packed=True):
    """the C entry point itself, with the caller's output pointers -> status"""
    pk, rs, rl, go = sp.arrays()
    n = go.size - 1
    fn, h = (d2g.lib().d2g_sketcher_run_mincount, sketcher._h) if form == "sketcher" else (d2g.lib().d2g_oph_sketch_mincount, gpu_ctx._h)
    return fn(h, pk.ctypes.data if packed else None, pk.size if packed else 0, rs.ctypes.data, rl.ctypes.data, rs.size, go.ctypes.data, n,
              sp.k, int(canon), xormask, S, c, regs_ptr, counts_ptr)


def run_form(d2g, gpu_ctx, sketcher, torch, form, sp, S, c, canon, xormask, filt=None):
    """-> (registers [n][m], counts [n][m]) through one of the three forms, outputs between guard words"""
    pk, rs, rl, go = sp.arrays()
    n, m = go.size - 1, R.oph_m(S)
    if form == "dev":
        plan = gpu_ctx.oph_plan(rs, rl, go, sp.k)
        try:
            if filt is not None:
                plan.set_filter(filt)
            packed = torch.from_numpy(np.array(pk, np.uint8)).cuda()
            regs, cnts = DevOut(torch, n, m, np.uint64), DevOut(torch, n, m, np.uint32)
            torch.cuda.synchronize()
            gpu_ctx.oph_sketch_mincount_dev(plan, packed.data_ptr(), S, c, regs.ptr, canon=canon, xormask=xormask)
            gpu_ctx.oph_count_dev(plan, packed.data_ptr(), S, regs.ptr, cnts.ptr, canon=canon, xormask=xormask)
            gpu_ctx.sync()
            return regs.read(), cnts.read()
        finally:
            plan.close()
    regs, cnts = HostOut(n, m, np.uint64), HostOut(n, m, np.uint32)
    rc = host_call(d2g, gpu_ctx, sketcher, form, sp, S, c, canon, xormask, regs.ptr, cnts.ptr)
    assert rc == 0, f"{form}: status {rc}"
    return regs.read(), cnts.read()


def check(d2g, gpu_ctx, sketcher, torch, batch, c, exp=None, forms=("sketcher",), S=None):
    S = S or batch.S
    eregs, ecnts = exp if exp is not None else Q.expected(batch, S, c)
    sp = seqpack(d2g, batch)
    for form in forms:
        regs, cnts = run_form(d2g, gpu_ctx, sketcher, torch, form, sp, S, c, batch.canon, batch.xormask)
        np.testing.assert_array_equal(regs, eregs, err_msg=f"{batch} c={c} {form}: registers")
        np.testing.assert_array_equal(cnts, ecnts, err_msg=f"{batch} c={c} {form}: counts")
    # without the counts: the same registers, and the counts pointer is optional
    regs = HostOut(len(batch.genomes), R.oph_m(S), np.uint64)
    assert host_call(d2g, gpu_ctx, sketcher, "sketcher", sp, S, c, batch.canon, batch.xormask, regs.ptr, None) == 0
    np.testing.assert_array_equal(regs.read(), eregs, err_msg=f"{batch} c={c}: registers of the call without counts")


# ---------------------------------------------------------------- the >= seam, by construction
@pytest.mark.parametrize("canon", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("k", Q.SEAM_K)
@pytest.mark.parametrize("S", Q.SEAM_S)
@pytest.mark.parametrize("c", Q.SEAM_C)
def test_only_what_occurs_c_times_is_sketched(d2g, gpu_ctx, sketcher, torch, c, S, k, canon):
    """A once, B c times, D c - 1 times: the registers are the plain sketch of B alone and every count is c"""
    batch, eregs, ecnts = Q.ge_seam(c, S, k, canon)
    forms = FORMS if (c, S) in ((2, 7), (3, 1024), (4, 1)) else ("sketcher",)
    check(d2g, gpu_ctx, sketcher, torch, batch, c, exp=(eregs, ecnts), forms=forms)


# ---------------------------------------------------------------- planted counts 1 .. 4
@pytest.mark.parametrize("env", [{}, {"D2G_K3_COMPACT": "1"}], ids=["generic", "compact"])
@pytest.mark.parametrize("c", [1, 2, 3, 4, 5])
def test_planted_counts_under_every_threshold(d2g, gpu_ctx, sketcher, torch, monkeypatch, c, env):
    """counts 1 .. 4 under c = 1 .. 5, with an empty genome and one shorter than k in the same call; c = 5 leaves every register ~0
    and every count 0, and the finalised sketch is that of an input without k-mers"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    batch = Q.planted()
    check(d2g, gpu_ctx, sketcher, torch, batch, c, forms=FORMS if c in (2, 5) else ("sketcher",))
    if c == 5:
        regs = sketcher.run_mincount(seqpack(d2g, batch), batch.S, c, canon=batch.canon)
        assert (regs == M64).all()
        sig, card = d2g.oph_finalize(regs, batch.S)
        nsig, ncard = d2g.oph_finalize(sketcher.run(seqpack(d2g, C.Batch("none", batch.k, batch.S, True, 0, [[], [], [], []])), batch.S), batch.S)
        assert sig.tobytes() == nsig.tobytes() and card.tobytes() == ncard.tobytes()


# ---------------------------------------------------------------- K3's own seams
@pytest.mark.parametrize("c", [2, 3])
def test_table_rounds_at_their_size_seams(d2g, gpu_ctx, sketcher, torch, monkeypatch, c):
    """one bucket of 1399 .. 5601 distinct keys per genome (one round, two, four, the once-more split), as it is (nothing reaches c)
    and with every record twice (everything reaches 2, nothing 3)"""
    for name, value in C.ROUND_ENV.items():
        monkeypatch.setenv(name, value)
    check(d2g, gpu_ctx, sketcher, torch, C.table_round_genomes(), c)
    check(d2g, gpu_ctx, sketcher, torch, Q.doubled(C.table_round_genomes()), c, forms=("sketcher", "dev"))


@pytest.mark.parametrize("env", [{}, {"D2G_K3_ROUND_KEYS": "64"}, {"D2G_K3_BUCKET_KEYS": "16", "D2G_K3_L1BITS": "3"}],
                         ids=["defaults", "ROUND_KEYS=64", "many_buckets_refined"])
@pytest.mark.parametrize("c", [2, 3])
def test_the_all_ones_key_is_an_element_like_any_other(d2g, gpu_ctx, sketcher, torch, monkeypatch, c, env):
    """the masked key ~0 is the count table's EMPTY and is counted beside it: seen once (dropped), three times (kept), 180 and 10
    times, alone in its genome and among others"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    for batch in (C.all_ones_generic("backbone"), C.all_ones_generic("unit"), C.all_ones_only()):
        check(d2g, gpu_ctx, sketcher, torch, batch, c, forms=FORMS if not env else ("sketcher",))


@pytest.mark.parametrize("k", [16, 17, 21])
@pytest.mark.parametrize("c", [2, 3])
def test_the_all_ones_stored_word_of_the_compact_form(d2g, gpu_ctx, sketcher, torch, monkeypatch, c, k):
    """D2G_K3_COMPACT=1 stores a k-mer's low 32 bits: 0xFFFFFFFF for every k-mer that ends in sixteen T; the kernel rebuilds the
    k-mer from (bucket, stored word) and mixes it once per distinct k-mer"""
    monkeypatch.setenv("D2G_K3_COMPACT", "1")
    check(d2g, gpu_ctx, sketcher, torch, C.all_ones_compact(k), c, forms=FORMS if k == 17 else ("sketcher",))
    for S in (1, 7):
        check(d2g, gpu_ctx, sketcher, torch, C.all_ones_compact(k), c, S=S)


# ---------------------------------------------------------------- the id 2^64 - 1
def test_the_id_all_ones_counts_against_an_empty_register(d2g, gpu_ctx, sketcher, torch):
    """a k-mer whose OPH id is ~0, seen once under c = 3: the register stays ~0 and its count is 1; with a smaller winner planted in
    the same register the count is the winner's"""
    batch, c, r = Q.ones_id()
    eregs, ecnts = Q.expected(batch, batch.S, c)
    assert eregs[0][r] == M64 and ecnts[0][r] == 1 and eregs[1][r] != M64 and ecnts[1][r] == c
    check(d2g, gpu_ctx, sketcher, torch, batch, c, exp=(eregs, ecnts), forms=FORMS)


# ---------------------------------------------------------------- a filter
@pytest.mark.parametrize("canon", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("c", [2, 3])
def test_filtered_kmers_do_not_count(d2g, gpu_ctx, torch, c, canon):
    """the filter holds ONE k-mer of a unit that occurs c times: that k-mer is gone, its neighbours stay; detached, it is back"""
    batch, record, drop = Q.filtered(c, canon)
    plain, filtered = Q.expected(batch, batch.S, c), Q.expected(batch, batch.S, c, drop=drop)
    assert not np.array_equal(plain[0], filtered[0])
    fsp = d2g.SeqPack(batch.k)
    fsp.add_fastx(C.fasta([record], "filter"))
    filt = gpu_ctx.kmer_filter(fsp, canon)
    sk = gpu_ctx.sketcher()
    try:
        sp = seqpack(d2g, batch)
        sk.set_filter(filt)
        regs, cnts = run_form(d2g, gpu_ctx, sk, torch, "sketcher", sp, batch.S, c, canon, batch.xormask)
        np.testing.assert_array_equal(regs, filtered[0])
        np.testing.assert_array_equal(cnts, filtered[1])
        regs, cnts = run_form(d2g, gpu_ctx, sk, torch, "dev", sp, batch.S, c, canon, batch.xormask, filt=filt)
        np.testing.assert_array_equal(regs, filtered[0])
        np.testing.assert_array_equal(cnts, filtered[1])
        sk.set_filter(None)
        regs, cnts = run_form(d2g, gpu_ctx, sk, torch, "sketcher", sp, batch.S, c, canon, batch.xormask)
        np.testing.assert_array_equal(regs, plain[0])
        np.testing.assert_array_equal(cnts, plain[1])
    finally:
        sk.close()
        filt.close()


# ---------------------------------------------------------------- mincount 0 and 1
@pytest.mark.parametrize("c", [0, 1])
def test_mincount_below_two_is_run_and_run_counts(d2g, gpu_ctx, sketcher, torch, c):
    batch = Q.planted()
    sp = seqpack(d2g, batch)
    eregs, ecnts = sketcher.run_counts(sp, batch.S, batch.canon, batch.xormask)
    np.testing.assert_array_equal(sketcher.run(sp, batch.S, batch.canon, batch.xormask), eregs)
    np.testing.assert_array_equal(eregs, Q.expected(batch, batch.S, 1)[0])
    for form in FORMS:
        regs, cnts = run_form(d2g, gpu_ctx, sketcher, torch, form, sp, batch.S, c, batch.canon, batch.xormask)
        assert regs.tobytes() == eregs.tobytes() and cnts.tobytes() == ecnts.tobytes(), form
    assert sketcher.run_mincount(sp, batch.S, c, batch.canon, batch.xormask).tobytes() == eregs.tobytes()


# ---------------------------------------------------------------- refusals
def test_argument_refusals_come_before_anything_is_written(d2g, gpu_ctx, sketcher, torch):
    batch = Q.planted()
    sp = seqpack(d2g, batch)
    n, m = len(batch.genomes), R.oph_m(batch.S)
    for form in ("sketcher", "one_shot"):
        regs, cnts = HostOut(n, m, np.uint64), HostOut(n, m, np.uint32)
        for S in (0, 1 << 31):
            assert host_call(d2g, gpu_ctx, sketcher, form, sp, S, 2, True, 0, regs.ptr, cnts.ptr) == INVALID, (form, S)
        assert host_call(d2g, gpu_ctx, sketcher, form, sp, batch.S, 2, True, 0, None, cnts.ptr) == INVALID, form
        assert regs.untouched() and cnts.untouched()
    # no genome at all: fine, nothing is written, null outputs included
    none = C.Batch("none", batch.k, batch.S, True, 0, [])
    nsp = seqpack(d2g, none)
    for form in ("sketcher", "one_shot"):
        regs = HostOut(1, m, np.uint64)
        assert host_call(d2g, gpu_ctx, sketcher, form, nsp, batch.S, 2, True, 0, regs.ptr, None) == 0
        assert host_call(d2g, gpu_ctx, sketcher, form, nsp, batch.S, 2, True, 0, None, None) == 0
        assert regs.untouched()
    # the device form
    pk, rs, rl, go = sp.arrays()
    plan = gpu_ctx.oph_plan(rs, rl, go, sp.k)
    packed = torch.from_numpy(np.array(pk, np.uint8)).cuda()
    out = DevOut(torch, n, m, np.uint64)
    try:
        for S, ptr in ((0, out.ptr), (1 << 31, out.ptr), (batch.S, None)):
            with pytest.raises(d2g.D2GError) as e:
                gpu_ctx.oph_sketch_mincount_dev(plan, packed.data_ptr(), S, 2, ptr)
            assert e.value.status == INVALID
        with pytest.raises(d2g.D2GError) as e:
            gpu_ctx.oph_sketch_mincount_dev(plan, packed.data_ptr() + 2, batch.S, 2, out.ptr)       # not 4-byte aligned
        assert e.value.status == INVALID
        torch.cuda.synchronize()
        assert (out.t.cpu().numpy() == FILL).all()
    finally:
        plan.close()
    # a sketcher that refused goes on working
    check(d2g, gpu_ctx, sketcher, torch, batch, 2)


def test_counts_of_a_genome_of_two_to_the_32_kmers_are_refused(d2g, gpu_ctx, sketcher):
    """the tables alone decide (two runs of 2^31 bases at k = 1), before anything is staged; as d2g_oph_sketch_counts refuses it"""
    packed = np.zeros(68, np.uint8)
    rs, rl, go = np.array([0, 1 << 31], np.uint64), np.array([1 << 31, 1 << 31], np.uint32), np.array([0, 2], np.uint64)
    regs, cnts = HostOut(1, 8, np.uint64), HostOut(1, 8, np.uint32)
    for fn, h in ((d2g.lib().d2g_sketcher_run_mincount, sketcher._h), (d2g.lib().d2g_oph_sketch_mincount, gpu_ctx._h)):
        rc = fn(h, packed.ctypes.data, packed.size, rs.ctypes.data, rl.ctypes.data, 2, go.ctypes.data, 1, 1, 1, 0, 8, 2, regs.ptr, cnts.ptr)
        assert rc == UNSUPPORTED
    assert regs.untouched() and cnts.untouched()


# ---------------------------------------------------------------- the device parser's stream
def test_the_stream_parsed_on_the_device(d2g, gpu_ctx, torch):
    """d2g_sketcher_ingest_fasta, then run_mincount with packed == NULL: the host-parsed result"""
    batch = Q.planted()
    sk = gpu_ctx.sketcher()
    try:
        runs = sk.ingest_fasta(batch.fastas(), batch.k)
        for c in (2, 3):
            eregs, ecnts = Q.expected(batch, batch.S, c)
            regs, cnts = sk.run_mincount_ingested(runs, batch.S, c, canon=batch.canon, xormask=batch.xormask, counts=True)
            np.testing.assert_array_equal(regs, eregs)
            np.testing.assert_array_equal(cnts, ecnts)
        np.testing.assert_array_equal(sk.run_mincount_ingested(runs, batch.S, 4, canon=batch.canon), Q.expected(batch, batch.S, 4)[0])
        np.testing.assert_array_equal(sk.run_ingested(runs, batch.S, canon=batch.canon), Q.expected(batch, batch.S, 1)[0])   # still usable
    finally:
        sk.close()


def test_the_selection_is_timed_as_k3_and_the_count_pass_as_k1count(d2g, gpu_ctx, sketcher):
    sp = seqpack(d2g, Q.planted())
    gpu_ctx.set_timing(True)
    try:
        for which in ("k1", "k3", "k1count"):
            gpu_ctx.kernel_ms(which)
        sketcher.run_mincount(sp, 16, 2)
        assert gpu_ctx.kernel_ms("k3", reset=False)[0] == 1 and gpu_ctx.kernel_ms("k1count", reset=False)[0] == 0
        sketcher.run_mincount(sp, 16, 2, counts=True)
        assert gpu_ctx.kernel_ms("k3")[0] == 2 and gpu_ctx.kernel_ms("k1count")[0] == 1 and gpu_ctx.kernel_ms("k1")[0] == 0
    finally:
        gpu_ctx.set_timing(False)
