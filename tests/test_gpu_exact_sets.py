"""d2g_kmer_sets and d2g_kmer_sets_dev (K3's exact counts -> the sorted emission K3s) against exact_ref.exact_sets over
k3_seam_cases.key_counts -- a pure-Python k-mer enumerator and NumPy's wang64; nothing the product computed.  Keys, counts, offsets and
cards are compared bit for bit.

Every output lies between guard words and starts as 0xAB bytes; the guard words must come back untouched, and so must the whole
output after a call that was refused.  The D2G_K3* switches are set with monkeypatch.setenv: the session's context reads them again."""
import functools

import numpy as np
import pytest

import exact_ref as X
import k3_seam_cases as C

pytestmark = pytest.mark.gpu

GUARD, FILL = 32, 0xAB
INVALID = -1                                                           # D2G_ERR_INVALID (include/d2g.h)
M64 = C.M64


class HostOut:
    def __init__(self, n, dtype):
        self.n = n
        self.a = np.frombuffer(bytes([FILL]) * ((2 * GUARD + n) * np.dtype(dtype).itemsize), dtype).copy()
        self.fill = self.a[0]

    @property
    def ptr(self):
        return self.a.ctypes.data + GUARD * self.a.itemsize

    def read(self):
        assert (self.a[:GUARD] == self.fill).all() and (self.a[GUARD + self.n:] == self.fill).all(), "guard words around an output were written"
        return self.a[GUARD:GUARD + self.n]

    def untouched(self):
        return (self.a == self.fill).all()


class DevOut:
    def __init__(self, torch, n, dtype):
        self.n, self.dtype = n, np.dtype(dtype)
        self.t = torch.full(((2 * GUARD + n) * self.dtype.itemsize,), FILL, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD * self.dtype.itemsize

    def all(self):
        return self.t.cpu().numpy().view(self.dtype)

    def read(self):
        a, fill = self.all(), np.frombuffer(bytes([FILL]) * self.dtype.itemsize, self.dtype)[0]
        assert (a[:GUARD] == fill).all() and (a[GUARD + self.n:] == fill).all(), "guard words around a device output were written"
        return a[GUARD:GUARD + self.n]

    def untouched(self):
        return (self.all() == np.frombuffer(bytes([FILL]) * self.dtype.itemsize, self.dtype)[0]).all()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def seqpack(d2g, batch):
    sp = d2g.SeqPack(batch.k)
    for f in batch.fastas():
        sp.add_fastx(f)
    assert [sp.nkmers(g) for g in range(len(batch.genomes))] == batch.nkmers()
    return sp


def call(d2g, gpu_ctx, torch, form, sp, canon, xormask, thr, cap, want_counts=True, filt=None):
    """the C entry point with guarded outputs of `cap` entries -> (status, keys, counts, set_off, cards) as guarded buffers"""
    pk, rs, rl, go = sp.arrays()
    n = go.size - 1
    if form == "dev":
        plan = gpu_ctx.oph_plan(rs, rl, go, sp.k)
        try:
            if filt is not None:
                plan.set_filter(filt)
            packed = torch.from_numpy(np.array(pk, np.uint8)).cuda()
            outs = (DevOut(torch, cap, np.uint64), DevOut(torch, cap, np.uint32), DevOut(torch, n + 1, np.uint64), DevOut(torch, 2 * n, np.uint64))
            torch.cuda.synchronize()
            rc = d2g.lib().d2g_kmer_sets_dev(gpu_ctx._h, plan._h, packed.data_ptr(), int(canon), xormask, thr, outs[0].ptr,
                                             outs[1].ptr if want_counts else None, cap, outs[2].ptr, outs[3].ptr, None)
            gpu_ctx.sync()
            return (rc,) + outs
        finally:
            plan.close()
    assert filt is None
    outs = (HostOut(cap, np.uint64), HostOut(cap, np.uint32), HostOut(n + 1, np.uint64), HostOut(2 * n, np.uint64))
    rc = d2g.lib().d2g_kmer_sets(gpu_ctx._h, pk.ctypes.data, pk.size, rs.ctypes.data, rl.ctypes.data, rs.size, go.ctypes.data, n, sp.k, int(canon),
                                 xormask, thr, outs[0].ptr, outs[1].ptr if want_counts else None, cap, outs[2].ptr, outs[3].ptr)
    return (rc,) + outs


def check(d2g, gpu_ctx, torch, batch, thr=0.0, forms=("host", "dev"), expected=None, filt=None, slack=3):
    sets = expected if expected is not None else X.exact_sets(batch, thr)
    ekeys, ecnts, eoff, ecards = X.flat(sets)
    for s, (k_, _) in enumerate(sets):
        assert (np.diff(k_.astype(object)) > 0).all(), f"set {s} of the expectation is not strictly ascending"
    sp = seqpack(d2g, batch)
    total = int(eoff[-1])
    for form in forms:
        for want_counts in (True, False):
            rc, keys, cnts, off, cards = call(d2g, gpu_ctx, torch, form, sp, batch.canon, batch.xormask, thr, total + slack, want_counts, filt)
            assert rc == 0, f"{batch} {form}: status {rc}: {d2g.lib().d2g_last_error(gpu_ctx._h).decode()}"
            np.testing.assert_array_equal(off.read(), eoff, err_msg=f"{batch} thr={thr} {form}: offsets")
            np.testing.assert_array_equal(cards.read().reshape(-1, 2), ecards, err_msg=f"{batch} thr={thr} {form}: cards")
            np.testing.assert_array_equal(keys.read()[:total], ekeys, err_msg=f"{batch} thr={thr} {form}: keys")
            assert (keys.read()[total:].view(np.uint8) == FILL).all(), "keys past the total were written"
            if want_counts:
                np.testing.assert_array_equal(cnts.read()[:total], ecnts, err_msg=f"{batch} thr={thr} {form}: counts")
            else:
                assert cnts.untouched(), "counts were written although none were asked for"
    return sets


# ---------------------------------------------------------------- degenerate inputs
@functools.lru_cache(maxsize=None)
def degenerate():
    """no k-mer at all (no record; a record shorter than k), exactly one k-mer, one k-mer 180 times, and an ordinary genome"""
    rng = np.random.default_rng(3100)
    k = 21
    return C.Batch("degenerate", k, 16, True, 0x5a5a, [[], [C.random_bases(rng, k - 1)], [C.random_bases(rng, k)], ["A" * 200], [C.random_bases(rng, 900)]])


def test_inputs_without_k_mers_with_one_and_with_one_repeated(d2g, gpu_ctx, torch):
    sets = check(d2g, gpu_ctx, torch, degenerate())
    assert [len(k) for k, _ in sets] == [0, 0, 1, 1, 880] and sets[3][1].tolist() == [180]


def test_nothing_but_empty_inputs(d2g, gpu_ctx, torch):
    check(d2g, gpu_ctx, torch, C.Batch("empty", 21, 16, True, 0, [[], []]))


# ---------------------------------------------------------------- the count threshold: kept iff count > threshold
@pytest.mark.parametrize("thr", [0.0, 0.5, 1.0, 2.0, 2.5, 3.0, 4.0])
def test_counts_just_above_and_below_the_threshold(d2g, gpu_ctx, torch, thr):
    """counts 1, 2, 3, 4 (40 k-mers each) and a genome of count 2 only"""
    sets = check(d2g, gpu_ctx, torch, C.planted_counts(), thr, forms=("host", "dev") if thr in (1.0, 4.0) else ("host",))
    assert len(sets[0][0]) == 40 * sum(1 for c in (1, 2, 3, 4) if c > thr)


# ---------------------------------------------------------------- the ends of the key range
@functools.lru_cache(maxsize=None)
def extreme_key(which):
    """the xormask makes the masked key of one k-mer of the genome 0 or 2^64 - 1: the first or the last element of its set"""
    rng = np.random.default_rng(3200)
    k = 21
    rec = C.random_bases(rng, 5000)
    x0 = C._record_kmers(rec, k, True)[1234]
    target = 0 if which == "zero" else M64
    mask = C._oracle().wang_inverse(target) ^ x0
    return C.Batch(f"key_{which}", k, 16, True, mask, [[rec], [rec[:3000], rec[:3000]]], note={"target": target})


@pytest.mark.parametrize("which", ["zero", "ones"])
def test_the_smallest_and_the_largest_key(d2g, gpu_ctx, torch, which):
    b = extreme_key(which)
    sets = check(d2g, gpu_ctx, torch, b)
    for keys, _ in sets:
        assert int(keys[0 if which == "zero" else -1]) == b.note["target"]


def test_a_set_that_is_the_all_ones_key_alone(d2g, gpu_ctx, torch):
    """the key ~0 is what pads a sort range: a real one must keep its count (180, 10) and come last"""
    sets = check(d2g, gpu_ctx, torch, C.all_ones_only())
    assert sets[0][0].tolist() == [M64] and sets[0][1].tolist() == [180] and int(sets[1][0][-1]) == M64 and int(sets[1][1][-1]) == 10


# ---------------------------------------------------------------- many buckets, both bucket mappings, many sort ranges
@functools.lru_cache(maxsize=None)
def many_buckets():
    """k = 21 (the compact path applies): 30 000, 7 000 (every record twice) and 2 100 bases, an empty genome between them"""
    rng = np.random.default_rng(3300)
    r = C.random_bases(rng, 7000)
    return C.Batch("buckets", 21, 16, True, 0x77, [[C.random_bases(rng, 30000)], [], [r, r], [C.random_bases(rng, 2100)]])


BUCKET_ENVS = [{}, {"D2G_K3_COMPACT": "1"}, {"D2G_K3S_RANGE_KEYS": "16"}, {"D2G_K3_COMPACT": "1", "D2G_K3S_RANGE_KEYS": "100"},
               {"D2G_K3_ROUND_KEYS": "64"}, {"D2G_K3_SPLIT_MIN": "40", "D2G_K3_ROUND_KEYS": "200"}, {"D2G_K3_BUCKET_KEYS": "1000000"}]


@pytest.mark.parametrize("env", BUCKET_ENVS, ids=lambda e: ",".join(f"{k[4:]}={v}" for k, v in e.items()) or "default")
def test_many_buckets_under_both_bucket_mappings(d2g, gpu_ctx, torch, monkeypatch, env):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    check(d2g, gpu_ctx, torch, many_buckets(), forms=("host", "dev") if len(env) < 2 else ("host",))
    check(d2g, gpu_ctx, torch, many_buckets(), 1.0, forms=("host",))


@pytest.mark.parametrize("nk", [1023, 1024, 1025, 2048, 2049, 4096, 4097])
def test_sort_ranges_at_their_size_seams(d2g, gpu_ctx, torch, nk):
    """nk distinct k-mers in one genome: one sort range up to 1024 k-mers, two from 1025, four from 2049, eight from 4097"""
    rng = np.random.default_rng(3400 + nk)
    check(d2g, gpu_ctx, torch, C.Batch(f"range_{nk}", 31, 16, True, 0, [[C.random_bases(rng, nk + 30)]]), forms=("host",))


# ---------------------------------------------------------------- --filterset
def test_a_filter_drops_its_k_mers_from_every_set(d2g, gpu_ctx, torch):
    b = many_buckets()
    frecs = [b.genomes[0][0][1000:9000], b.genomes[2][0][:2000]]
    fkeys = C.key_counts(tuple(frecs), b.k, b.canon, b.xormask)[0]
    fsp = d2g.SeqPack(b.k)
    fsp.add_fastx(C.fasta(frecs, "filter"))
    filt = gpu_ctx.kmer_filter(fsp, canon=b.canon)
    try:
        for thr in (0.0, 1.0):
            want = []
            for keys, counts in X.exact_sets(b, thr):
                keep = ~np.isin(keys, fkeys)
                want.append((keys[keep], counts[keep]))
            assert sum(len(k) for k, _ in want) < sum(len(k) for k, _ in X.exact_sets(b, thr)) - 1900
            check(d2g, gpu_ctx, torch, b, thr, forms=("dev",), expected=want, filt=filt)
    finally:
        filt.close()


# ---------------------------------------------------------------- cap
@pytest.mark.parametrize("form", ["host", "dev"])
def test_a_cap_one_short_is_refused_and_nothing_is_written(d2g, gpu_ctx, torch, form):
    b = many_buckets()
    total = int(X.flat(X.exact_sets(b))[2][-1])
    sp = seqpack(d2g, b)
    rc, *outs = call(d2g, gpu_ctx, torch, form, sp, b.canon, b.xormask, 0.0, total - 1)
    assert rc == INVALID
    msg = d2g.lib().d2g_last_error(gpu_ctx._h).decode()
    assert "capacity too small" in msg and str(total) in msg and str(total - 1) in msg
    for o in outs:
        assert o.untouched(), "a refused call wrote to an output"
    rc, keys, cnts, off, cards = call(d2g, gpu_ctx, torch, form, sp, b.canon, b.xormask, 0.0, total)      # exactly enough
    assert rc == 0 and int(off.read()[-1]) == total
    keys.read(), cnts.read(), cards.read()
